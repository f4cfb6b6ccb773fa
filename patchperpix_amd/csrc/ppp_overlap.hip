// ppp_overlap.hip -- the contingency table of two label stacks in one streaming pass (ppp_label_overlap).
//
// A u32 [La][V] and B u32 [Lb][V], V = Z*Y*X voxels, 0 = background.  The result is the sorted list of
//   (a, b) : #{(i, j, v) : A[i][v] == a, B[j][v] == b}     a != 0, b != 0
//   (a, 0) : #{(i, v) : A[i][v] == a}                       (0, b) : #{(j, v) : B[j][v] == b}
// as rows of two u32 with an int64 count (include/ppp_mi355x.h).  Every (voxel, channel pair) and every
// (voxel, channel) is one INCIDENCE of a 64-bit key a << 32 | b; the result is the histogram of the keys.
//
// Pass 1, overlap_count_kernel.  The position of a voxel does not matter, so the volume is the flat array
// [V] and a row's length plays no part: a lane reads FOUR consecutive voxels of a channel with one 16-byte
// load.  A channel starts at c * V words, which is 16-byte aligned only when V % 4 == 0 -- the load is
// declared with 4-byte alignment (global_load_dwordx4 needs no more on gfx950), and the last, partial group
// of four is read word by word with zeros beyond V.  "One streaming read of both stacks" holds for La = 1 only:
// A is read once, B once per channel of A.  The repeats ask for the lines the same lane loaded a few
// instructions earlier; that they are served from cache is supposed, not measured (every timed case is 1 x 1).
// The work is La*Lb + La + Lb key streams per voxel whatever the reads cost: a one-instance-per-channel map of
// hundreds of channels is slow here, and above 65535 streams refused.
// For each of the La*Lb + La + Lb key streams:
//   - equal neighbours among the lane's four keys collapse into one (key, n) item;
//   - a lane whose four keys are equal AND equal to the last key of the lane before it emits nothing: the
//     head of such a chain finds its length in the ballot of these lanes and adds 4 per lane to its last item;
//   - a wave that holds background only skips the stream.
// The items go into a per-workgroup LDS table: kTableEntries slots, open addressing (linear probing) on
// the 64-bit key from overlap_slot(a, b), u32 counts, LDS atomics only.  Key 0 -- (0, 0), which is no key
// -- marks a free slot.  The table is FLUSHED to the global list of (key, count) partials when it holds
// kFlushAt keys (looked at after the first step and then every fourth, one workgroup barrier per look: a look
// after every step cost 8 % of the pass at 512^3) and at the workgroup's end: one global atomic per flush
// reserves the range.  Between two looks a lane that finds kSpillAt keys in the table, or no
// home within kMaxProbe slots, SPILLS its item to the list directly (one global atomic per wave and spill round); so
// the table is never full and a probe always ends.  There is no global atomic per voxel.
// A u32 count cannot overflow: a workgroup's share of the volume is bounded by (2^32 - 1) / (La*Lb + La + Lb)
// voxels (overlap_plan), and a voxel adds at most La*Lb to one key; the entry point refuses more than
// 65535 streams.
//
// Pass 2, rocPRIM: radix_sort_pairs on the 64-bit keys, reduce_by_key with 64-bit sums, then
// overlap_emit_kernel writes the rows when they fit `cap`.  Integer sums only: the order in which partials
// reach the list varies from run to run, the result does not.
//
// WORST CASE, every voxel its own pair: every incidence becomes a partial of its own, and there are at most
// V * (La*Lb + La + Lb) of them (a partial stands for at least one incidence).  The list is sized for that:
// two (u64 key, u64 count) buffers, handed to the sort as rocprim::double_buffer so that it keeps no copy of
// its own; the half the sort leaves free takes the reduced rows.  32 bytes per voxel and stream (96 bytes per
// voxel for La = Lb = 1) plus rocPRIM's temporary storage, which is histograms and scan states only.
// Writes to the list are bounds-checked all the same (counter [2] reports a refused write).
//
// The call synchronises the stream twice: rocPRIM takes the number of partials from the host, and n_rows is
// a host value.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "ppp_kernels.hpp"

namespace ppp {

constexpr int kOvBlock = 256;                          // threads of a workgroup
constexpr int kOvStepVoxels = kOvBlock * 4;            // voxels a workgroup reads per step and channel
constexpr int kTableBits = 11;
constexpr int kTableEntries = 1 << kTableBits;         // 2048 slots: 16 KiB of keys + 8 KiB of counts
constexpr unsigned kFlushAt = kTableEntries / 2;       // keys in the table at which a look flushes it
constexpr unsigned kSpillAt = kTableEntries * 3 / 4;   // keys at which a lane claims no new slot
constexpr int kMaxProbe = 64;
constexpr int kMaxBlocks = 2048;                       // 8 per CU: shares long enough to pay for the final flush
static_assert(kSpillAt + kOvBlock < kTableEntries, "every thread may claim one slot past kSpillAt: the table must not fill");

int overlap_table_entries() { return kTableEntries; }

// the last call's counters (this process, any thread): partials written, flushes inside the step loop,
// items spilled past the table -- for tests and tools, like ppp_last_error
static long long g_last_stats[3] = {0, 0, 0};
void overlap_last_stats(long long *out) {
    for (int i = 0; i < 3; ++i) out[i] = g_last_stats[i];
}

// the table's hash: the home slot of key (a, b)
__host__ __device__ __forceinline__ uint32_t overlap_slot(uint32_t a, uint32_t b) {
    return (a * 0x9E3779B1u + b * 0x85EBCA77u) >> (32 - kTableBits);
}
uint32_t overlap_slot_host(uint32_t a, uint32_t b) { return overlap_slot(a, b); }

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
struct Quad { uint32_t v[4]; };

// voxels [v0, v0 + 4) of one channel, zeros from V on
__device__ __forceinline__ Quad load_quad(const uint32_t *__restrict__ p, long long v0, long long V) {
    Quad q;
    if (v0 + 4 <= V) {
        const u32x4_a4 t = *reinterpret_cast<const u32x4_a4 *>(p + v0);
        q.v[0] = t.x; q.v[1] = t.y; q.v[2] = t.z; q.v[3] = t.w;
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) q.v[t] = v0 + t < V ? p[v0 + t] : 0u;
    }
    return q;
}

struct OvList {
    unsigned long long *keys, *vals;     // [cap]
    unsigned long long *counters;        // [0] partials written, [1] rows, [2] writes refused by the bound,
                                         // [3] flushes inside the step loop, [4] items spilled past the table
    unsigned long long cap;
};

// one item into the table; true: the item must go to the list instead
__device__ __forceinline__ bool table_add(unsigned long long *tkeys, uint32_t *tcnt, unsigned *fill,
                                          unsigned long long key, uint32_t n) {
    uint32_t slot = overlap_slot((uint32_t)(key >> 32), (uint32_t)key);
    for (int probe = 0; probe < kMaxProbe; ++probe, slot = (slot + 1) & (kTableEntries - 1)) {
        unsigned long long k = *(volatile unsigned long long *)&tkeys[slot];
        if (k == 0ull) {
            if (*(volatile unsigned *)fill >= kSpillAt) return true;
            k = atomicCAS(&tkeys[slot], 0ull, key);
            if (k == 0ull) {
                atomicAdd(fill, 1u);
                k = key;
            }
        }
        if (k == key) {
            atomicAdd(&tcnt[slot], n);
            return false;
        }
    }
    return true;
}

// the items of one key stream: the lane's four keys (0 = nothing to count), run-collapsed in the lane and
// along chains of uniform lanes; all 64 lanes call it
__device__ __forceinline__ void count_stream(unsigned long long *tkeys, uint32_t *tcnt, unsigned *fill, const OvList &L,
                                             const unsigned long long k[4], const int lane) {
    if (__ballot((k[0] | k[1] | k[2] | k[3]) != 0ull) == 0ull) return;
    const unsigned long long prev = __shfl_up(k[3], 1);
    const bool cont = lane > 0 && k[0] == k[1] && k[1] == k[2] && k[2] == k[3] && k[0] == prev;
    const unsigned long long cmask = __ballot(cont);
    const unsigned long long after = lane == 63 ? 0ull : cmask >> (lane + 1);
    const uint32_t chain = 4u * (uint32_t)__builtin_ctzll(~after);       // (bit 63 of `after` is clear)
    uint32_t n = 1;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const bool last = t == 3;
        const bool ends = last || k[t] != k[last ? t : t + 1];                     // the run of k[t] ends in this lane
        const bool item = ends && !cont && k[t] != 0ull;
        const uint32_t add = last ? n + chain : n;
        const bool spill = item && table_add(tkeys, tcnt, fill, k[t], add);
        const unsigned long long sm = __ballot(spill);
        if (sm) {                                                        // wave-uniform
            const int leader = __builtin_ctzll(sm);
            unsigned long long base = 0;
            if (lane == leader) {
                base = atomicAdd(&L.counters[0], (unsigned long long)__popcll(sm));
                atomicAdd(&L.counters[4], (unsigned long long)__popcll(sm));
            }
            base = __shfl(base, leader);
            if (spill) {
                const unsigned long long pos = base + (unsigned long long)__popcll(sm & ((1ull << lane) - 1ull));
                if (pos < L.cap) {
                    L.keys[pos] = k[t];
                    L.vals[pos] = add;
                } else {
                    atomicAdd(&L.counters[2], 1ull);
                }
            }
        }
        n = ends ? 1u : n + 1u;
    }
}

// the table's keys to the list, the table cleared; all threads call it, barriers inside
__device__ void table_flush(unsigned long long *tkeys, uint32_t *tcnt, unsigned *fill, unsigned long long *base_s,
                            unsigned *next_s, const OvList &L) {
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned n = *fill;
        *base_s = n ? atomicAdd(&L.counters[0], (unsigned long long)n) : 0ull;
        *next_s = 0u;
    }
    __syncthreads();
    const unsigned long long base = *base_s;
    for (int s = threadIdx.x; s < kTableEntries; s += kOvBlock) {
        const unsigned long long k = tkeys[s];
        if (k != 0ull) {
            const unsigned long long pos = base + atomicAdd(next_s, 1u);
            if (pos < L.cap) {
                L.keys[pos] = k;
                L.vals[pos] = tcnt[s];
            } else {
                atomicAdd(&L.counters[2], 1ull);
            }
            tkeys[s] = 0ull;
            tcnt[s] = 0u;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) *fill = 0u;
    __syncthreads();
}

__global__ void __launch_bounds__(kOvBlock)
    overlap_count_kernel(const uint32_t *__restrict__ A, const int La, const uint32_t *__restrict__ B, const int Lb,
                         const long long V, const int steps_per_block, const OvList L) {
    __shared__ unsigned long long tkeys[kTableEntries];
    __shared__ uint32_t tcnt[kTableEntries];
    __shared__ unsigned fill, next_s;
    __shared__ unsigned long long base_s;
    for (int s = threadIdx.x; s < kTableEntries; s += kOvBlock) {
        tkeys[s] = 0ull;
        tcnt[s] = 0u;
    }
    if (threadIdx.x == 0) fill = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long first = (long long)blockIdx.x * steps_per_block * kOvStepVoxels;
    for (int step = 0; step < steps_per_block; ++step) {            // (the trip count is the workgroup's)
        const long long v0 = first + (long long)step * kOvStepVoxels + 4ll * threadIdx.x;
        if (first + (long long)step * kOvStepVoxels < V) {           // workgroup-uniform
            unsigned long long k[4];
            for (int i = 0; i < La; ++i) {
                const Quad a = load_quad(A + (long long)i * V, v0, V);
                Quad next = load_quad(B, v0, V);                     // (in flight while A's stream is counted)
#pragma unroll
                for (int t = 0; t < 4; ++t) k[t] = (unsigned long long)a.v[t] << 32;
                count_stream(tkeys, tcnt, &fill, L, k, lane);
                for (int j = 0; j < Lb; ++j) {
                    const Quad b = next;
                    if (j + 1 < Lb) next = load_quad(B + (long long)(j + 1) * V, v0, V);
                    if (i == 0) {
#pragma unroll
                        for (int t = 0; t < 4; ++t) k[t] = b.v[t];
                        count_stream(tkeys, tcnt, &fill, L, k, lane);
                    }
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        k[t] = a.v[t] != 0u && b.v[t] != 0u ? (unsigned long long)a.v[t] << 32 | b.v[t] : 0ull;
                    count_stream(tkeys, tcnt, &fill, L, k, lane);
                }
            }
        }
        if ((step & 3) == 0 && step + 1 < steps_per_block && __syncthreads_or(*(volatile unsigned *)&fill >= kFlushAt)) {
            if (threadIdx.x == 0) atomicAdd(&L.counters[3], 1ull);
            table_flush(tkeys, tcnt, &fill, &base_s, &next_s, L);
        }
    }
    table_flush(tkeys, tcnt, &fill, &base_s, &next_s, L);
}

__global__ void __launch_bounds__(256)
    overlap_emit_kernel(const unsigned long long *__restrict__ keys, const unsigned long long *__restrict__ sums,
                        const long long n, uint32_t *__restrict__ rows, long long *__restrict__ counts) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    rows[2 * i] = (uint32_t)(keys[i] >> 32);
    rows[2 * i + 1] = (uint32_t)keys[i];
    counts[i] = (long long)sums[i];
}

// how the volume is shared out: steps of kOvStepVoxels per workgroup, such that a share stays below
// (2^32 - 1) / streams voxels (the u32 counts of the table) and the grid near kMaxBlocks
struct OvPlan {
    long long blocks;
    int steps_per_block;
};
static OvPlan overlap_plan(long long V, long long streams) {
    const long long steps = (V + kOvStepVoxels - 1) / kOvStepVoxels;
    const long long max_steps = (long long)(0xFFFFFFFFull / (unsigned long long)streams) / kOvStepVoxels;   // >= 64
    long long per = (steps + kMaxBlocks - 1) / kMaxBlocks;
    if (per > max_steps) per = max_steps;
    if (per < 1) per = 1;
    OvPlan P;
    P.steps_per_block = (int)per;
    P.blocks = (steps + per - 1) / per;
    return P;
}

struct OvWork {
    unsigned long long *keys[2], *vals[2];   // [items] each: the sort's double buffer
    unsigned long long *counters;            // [5], see OvList
    void *temp;
    size_t temp_bytes, items;
};
static OvWork overlap_layout(Carver &c, long long V, long long streams) {
    OvWork W;
    W.items = (size_t)V * (size_t)streams;
    for (int h = 0; h < 2; ++h) {
        W.keys[h] = c.take<unsigned long long>(W.items);
        W.vals[h] = c.take<unsigned long long>(W.items);
    }
    W.counters = (unsigned long long *)c.take_bytes(256);
    size_t a = 0, b = 0;
    rocprim::double_buffer<unsigned long long> k0(nullptr, nullptr), v0(nullptr, nullptr);
    (void)rocprim::radix_sort_pairs(nullptr, a, k0, v0, W.items, 0, 64, (hipStream_t)0);
    (void)rocprim::reduce_by_key(nullptr, b, (unsigned long long *)nullptr, (unsigned long long *)nullptr, W.items,
                                 (unsigned long long *)nullptr, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                 rocprim::plus<unsigned long long>(), rocprim::equal_to<unsigned long long>(), (hipStream_t)0);
    W.temp_bytes = up256(a > b ? a : b);
    W.temp = c.take_bytes(W.temp_bytes);
    return W;
}
size_t label_overlap_workspace_bytes(long long V, long long streams) {
    Carver c(nullptr);
    overlap_layout(c, V, streams);
    return c.used;
}

// rows u32 [cap][2], counts i64 [cap] (both may be NULL with cap = 0).  *n_rows always; the rows only when
// they fit.  hipErrorInvalidValue: a write to the list was refused by its bound (cannot happen, see above).
hipError_t run_label_overlap(const uint32_t *a, int La, const uint32_t *b, int Lb, long long V, uint32_t *rows,
                             long long *counts, long long cap, long long *n_rows, void *work, hipStream_t s) {
    const long long streams = (long long)La * Lb + La + Lb;
    const OvPlan P = overlap_plan(V, streams);
    PPP_GRID_CHECK(P.blocks, kOvBlock);
    Carver carver(work);
    const OvWork W = overlap_layout(carver, V, streams);
    hipError_t e;
    *n_rows = 0;
    if ((e = hipMemsetAsync(W.counters, 0, 40, s)) != hipSuccess) return e;
    OvList L;
    L.keys = W.keys[0];
    L.vals = W.vals[0];
    L.counters = W.counters;
    L.cap = (unsigned long long)W.items;
    overlap_count_kernel<<<dim3((unsigned)P.blocks), dim3(kOvBlock), 0, s>>>(a, La, b, Lb, V, P.steps_per_block, L);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    unsigned long long h[5] = {0, 0, 0, 0, 0};
    if ((e = hipMemcpyAsync(h, W.counters, 40, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    g_last_stats[0] = (long long)h[0];
    g_last_stats[1] = (long long)h[3];
    g_last_stats[2] = (long long)h[4];
    if (h[2] != 0 || h[0] > (unsigned long long)W.items) return hipErrorInvalidValue;
    const size_t n = (size_t)h[0];
    if (n == 0) return hipSuccess;
    size_t tb = W.temp_bytes;
    rocprim::double_buffer<unsigned long long> keys(W.keys[0], W.keys[1]), vals(W.vals[0], W.vals[1]);
    if ((e = rocprim::radix_sort_pairs(W.temp, tb, keys, vals, n, 0, 64, s)) != hipSuccess) return e;
    // sorted: keys.current() / vals.current(); the other half is free for the reduced rows
    unsigned long long *rk = keys.alternate(), *rv = vals.alternate();
    tb = W.temp_bytes;
    if ((e = rocprim::reduce_by_key(W.temp, tb, keys.current(), vals.current(), n, rk, rv, W.counters + 1,
                                    rocprim::plus<unsigned long long>(), rocprim::equal_to<unsigned long long>(), s)) != hipSuccess)
        return e;
    unsigned long long rows_found = 0;
    if ((e = hipMemcpyAsync(&rows_found, W.counters + 1, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    *n_rows = (long long)rows_found;
    if ((long long)rows_found > cap) return hipSuccess;
    PPP_GRID_CHECK((rows_found + 255) / 256, 256);
    overlap_emit_kernel<<<dim3((unsigned)((rows_found + 255) / 256)), dim3(256), 0, s>>>(rk, rv, (long long)rows_found,
                                                                                       rows, counts);
    return hipGetLastError();
}

}  // namespace ppp
