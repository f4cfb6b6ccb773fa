// ppp_postprocess.hip -- the whole-volume post-steps of the `label` driver on the device.
//
//   compact_ids  remove_small_components + relabel (PatchPerPix/util/postprocess.py:24-52): voxels
//                per id counted, ids of at most `compsize` voxels dropped, the survivors renumbered
//                in ascending order of the old id (an exclusive scan over the id-indexed keep flags).
//   dilate       the in-place ascending dilation loop (stitch_patch_graph.py:871-880) in closed form,
//                without the loop over instances (see "dilation" below).
//   clean_mask   stitch_patch_graph.py:46-57: connected components of a mask (union-find over linear
//                voxel indices), components of at most `size` voxels dropped.
//   fg_filter    postprocess_fg (PatchPerPix/util/postprocess.py:122-199): the same components, the small
//                ones dropped unless they lie near a big one (the distance transform of ppp_edt.hip),
//                the survivors numbered like scipy's labels of the cleaned mask.
//
// Ids are UNSIGNED 32-bit everywhere: they index tables as size_t and compare as uint32_t.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "ppp_kernels.hpp"

namespace ppp {

namespace {

constexpr int kMaxBlocks = 4096;   // grid-stride kernels: enough workgroups to fill 256 CUs

inline unsigned stride_blocks(long long items, int per_block = 256) {
    const long long b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

// A uint32 array seen as [head scalars | nvec 16-byte vectors | tail scalars]: the vectors start at
// the first 16-byte boundary.
struct Span {
    long long head, nvec, tail0, n;
};
inline Span make_span(const uint32_t *p, long long n) {
    Span s;
    long long head = (long long)(((16 - ((uintptr_t)p & 15)) & 15) / 4);
    s.head = head < n ? head : n;
    s.nvec = (n - s.head) / 4;
    s.tail0 = s.head + s.nvec * 4;
    s.n = n;
    return s;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// voxels per id
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void count_add(uint32_t *__restrict__ counts, uint32_t id, uint32_t max_id, uint32_t len,
                                          uint32_t *__restrict__ bad) {
    if (id > max_id) {
        atomicOr(bad, 1u);      // an id the table has no slot for: reported, never indexed
        return;
    }
    atomicAdd(&counts[id], len);
}

// Neighbouring voxels share ids, so runs are merged before memory is touched: a lane loads 16 bytes
// (4 voxels), an element is a run HEAD when it differs from the element before it (the first element
// of the wave's 256-voxel span always is), the heads of the wave are found with one ballot per
// element slot, and only a head adds -- its run length, the distance to the next head of the span --
// to the table.  Background (id 0) is skipped.
__global__ void __launch_bounds__(256)
    count_ids_kernel(const uint32_t *__restrict__ ids, const Span sp, const uint32_t max_id,
                     uint32_t *__restrict__ counts, uint32_t *__restrict__ bad) {
    const uint4 *__restrict__ vec = (const uint4 *)(ids + sp.head);
    const int lane = threadIdx.x & 63;
    const long long wave = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = (gridDim.x * (long long)blockDim.x) >> 6;
    for (long long base = wave * 64; base < sp.nvec; base += nwaves * 64) {   // (wave-uniform trip count)
        const long long i = base + lane;
        const bool live = i < sp.nvec;
        uint32_t v[4] = {0u, 0u, 0u, 0u};
        if (live) {
            const uint4 q = vec[i];
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        }
        const uint32_t prev = __shfl_up(v[3], 1);
        bool h[4];
        h[0] = live && (lane == 0 || v[0] != prev);
        h[1] = live && v[1] != v[0];
        h[2] = live && v[2] != v[1];
        h[3] = live && v[3] != v[2];
        const unsigned long long B0 = __ballot(h[0]), B1 = __ballot(h[1]), B2 = __ballot(h[2]), B3 = __ballot(h[3]);
        if (h[0] || h[1] || h[2] || h[3]) {
            const long long left = sp.nvec - base;
            const int span_end = (int)(left < 64 ? left : 64) * 4;
            const unsigned long long any = B0 | B1 | B2 | B3;
            const unsigned long long later = lane == 63 ? 0ull : any & (~0ull << (lane + 1));
            int next_lane_head = span_end;      // first head in a later lane
            if (later) {
                const int nl = __ffsll((long long)later) - 1;
                const int j = ((B0 >> nl) & 1) ? 0 : ((B1 >> nl) & 1) ? 1 : ((B2 >> nl) & 1) ? 2 : 3;
                next_lane_head = nl * 4 + j;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!h[k] || v[k] == 0u) continue;
                int nxt = next_lane_head;
#pragma unroll
                for (int j = 3; j > k; --j)
                    if (h[j]) nxt = lane * 4 + j;
                count_add(counts, v[k], max_id, (uint32_t)(nxt - (lane * 4 + k)), bad);
            }
        }
    }
}
// the (at most 3 + 3) voxels in front of and behind the 16-byte vectors
__global__ void count_ids_edges_kernel(const uint32_t *__restrict__ ids, const Span sp, const uint32_t max_id,
                                       uint32_t *__restrict__ counts, uint32_t *__restrict__ bad) {
    const long long t = threadIdx.x;
    if (t < sp.head && ids[t] != 0u) count_add(counts, ids[t], max_id, 1u, bad);
    if (sp.tail0 + t < sp.n && ids[sp.tail0 + t] != 0u) count_add(counts, ids[sp.tail0 + t], max_id, 1u, bad);
}

// counts[id] += voxels of id, for every id != 0 of ids[0 .. n); *bad |= 1 when an id exceeds max_id
static hipError_t launch_count_ids(const uint32_t *ids, long long n, uint32_t max_id, uint32_t *counts, uint32_t *bad,
                                   hipStream_t s) {
    const Span sp = make_span(ids, n);
    if (sp.nvec > 0)
        count_ids_kernel<<<dim3(stride_blocks(sp.nvec)), dim3(256), 0, s>>>(ids, sp, max_id, counts, bad);
    if (sp.head > 0 || sp.tail0 < sp.n)
        count_ids_edges_kernel<<<dim3(1), dim3(64), 0, s>>>(ids, sp, max_id, counts, bad);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// compact_ids
// ---------------------------------------------------------------------------------------------
// in place: table[i] = count of id i  ->  1 when id i stays (i != 0, present, more than compsize voxels)
__global__ void __launch_bounds__(256)
    keep_flags_kernel(uint32_t *__restrict__ table, const size_t slots, const size_t max_id, const long long compsize) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < slots; i += gridDim.x * (size_t)blockDim.x) {
        const uint32_t c = table[i];
        table[i] = (i != 0 && i <= max_id && c != 0u && (long long)c > compsize) ? 1u : 0u;
    }
}
__device__ __forceinline__ uint32_t new_id(uint32_t id, const uint32_t *__restrict__ keep,
                                           const uint32_t *__restrict__ rank, int relabel, uint32_t start) {
    if (id == 0u || keep[id] == 0u) return 0u;
    return relabel ? start + rank[id] : id;
}
__global__ void __launch_bounds__(256)
    apply_ids_kernel(uint32_t *__restrict__ ids, const Span sp, const uint32_t *__restrict__ keep,
                     const uint32_t *__restrict__ rank, const int relabel, const uint32_t start) {
    uint4 *__restrict__ vec = (uint4 *)(ids + sp.head);
    const long long gid = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    for (long long i = gid; i < sp.nvec; i += gridDim.x * (long long)blockDim.x) {
        uint4 q = vec[i];
        q.x = new_id(q.x, keep, rank, relabel, start);
        q.y = q.y == 0u ? 0u : new_id(q.y, keep, rank, relabel, start);
        q.z = q.z == 0u ? 0u : new_id(q.z, keep, rank, relabel, start);
        q.w = q.w == 0u ? 0u : new_id(q.w, keep, rank, relabel, start);
        vec[i] = q;
    }
    if (gid < sp.head) ids[gid] = new_id(ids[gid], keep, rank, relabel, start);
    if (sp.tail0 + gid < sp.n) ids[sp.tail0 + gid] = new_id(ids[sp.tail0 + gid], keep, rank, relabel, start);
}

struct CompactWork {
    uint32_t *table, *rank;    // [max_id + 2] each: counts, then keep flags (slot max_id + 1 stays 0); ranks
    uint32_t *bad;             // [1]
    void *temp;
    size_t temp_bytes, slots;
};
static CompactWork compact_layout(Carver &c, uint32_t max_id) {
    CompactWork W;
    W.slots = (size_t)max_id + 2;
    W.table = c.take<uint32_t>(W.slots);
    W.rank = c.take<uint32_t>(W.slots);
    W.bad = (uint32_t *)c.take_bytes(256);
    size_t tb = 0;
    (void)rocprim::exclusive_scan(nullptr, tb, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, W.slots,
                                  rocprim::plus<uint32_t>(), (hipStream_t)0);
    W.temp_bytes = up256(tb);
    W.temp = c.take_bytes(W.temp_bytes);
    return W;
}
size_t post_compact_workspace_bytes(uint32_t max_id) { Carver c(nullptr); compact_layout(c, max_id); return c.used; }

// hipErrorInvalidValue: the map holds an id above max_id (the map is then left as it was).  Synchronises.
hipError_t run_post_compact(uint32_t *ids, long long n, uint32_t max_id, long long compsize, int relabel,
                            uint32_t start, long long *n_kept, void *work, hipStream_t s) {
    Carver carver(work);
    const CompactWork W = compact_layout(carver, max_id);
    hipError_t e;
    if ((e = hipMemsetAsync(W.table, 0, W.slots * 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.bad, 0, 4, s)) != hipSuccess) return e;
    if ((e = launch_count_ids(ids, n, max_id, W.table, W.bad, s)) != hipSuccess) return e;
    keep_flags_kernel<<<dim3(stride_blocks((long long)W.slots)), dim3(256), 0, s>>>(W.table, W.slots, (size_t)max_id, compsize);
    size_t tb = W.temp_bytes;
    if ((e = rocprim::exclusive_scan(W.temp, tb, W.table, W.rank, 0u, W.slots, rocprim::plus<uint32_t>(), s)) != hipSuccess)
        return e;
    uint32_t bad = 0, kept = 0;
    if ((e = hipMemcpyAsync(&bad, W.bad, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&kept, W.rank + (W.slots - 1), 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    if (bad) return hipErrorInvalidValue;
    *n_kept = (long long)kept;
    const Span sp = make_span(ids, n);
    apply_ids_kernel<<<dim3(stride_blocks(sp.nvec > 0 ? sp.nvec : 1)), dim3(256), 0, s>>>(ids, sp, W.table, W.rank, relabel, start);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// dilation
// ---------------------------------------------------------------------------------------------
// The reference dilates label after label in ascending order, in place: when label L is dilated a voxel
// still equals L only if it was L originally and no smaller label's dilation has painted it over.  Call
// such a voxel a SURVIVOR.  With N[v] = v and its six face neighbours (outside the volume: background):
//     a voxel u with id a > 0 survives  iff  no face neighbour w with 0 < id(w) < a survives
//     result(v) = the largest id among the survivors in N[v], 0 when there is none
// Dependencies run along strictly decreasing ids, so the recursion is well founded.  One state byte per
// voxel; a decision is final and depends only on decisions already made, so the state is updated in
// place (a neighbour read as undecided only delays the decision to the next round).
struct Vol {
    int Z, Y, X;
    long long V, YX;
};
enum : uint8_t { ST_UNDECIDED = 0, ST_SURVIVOR = 1, ST_DEAD = 2 };

template <class F>
__device__ __forceinline__ void face_neighbours(const Vol &G, long long v, F f) {
    const int x = (int)(v % G.X), y = (int)((v / G.X) % G.Y), z = (int)(v / G.YX);
    if (x > 0) f(v - 1);
    if (x + 1 < G.X) f(v + 1);
    if (y > 0) f(v - G.X);
    if (y + 1 < G.Y) f(v + G.X);
    if (z > 0) f(v - G.YX);
    if (z + 1 < G.Z) f(v + G.YX);
}

// round 0: a voxel whose neighbours hold only its own id, larger ids or 0 survives at once; the others
// are compacted into a list (ballot / popcount, one atomic per wave) that the later rounds sweep
__global__ void __launch_bounds__(256)
    dilate_round0_kernel(const uint32_t *__restrict__ ids, uint8_t *__restrict__ state, int32_t *__restrict__ list,
                         uint32_t *__restrict__ n_list, const Vol G) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    bool undecided = false;
    if (v < G.V) {
        const uint32_t a = ids[v];
        uint8_t st = ST_DEAD;
        if (a != 0u) {
            bool smaller = false;
            face_neighbours(G, v, [&](long long w) { const uint32_t b = ids[w]; smaller |= (b != 0u && b < a); });
            st = smaller ? ST_UNDECIDED : ST_SURVIVOR;
        }
        state[v] = st;
        undecided = st == ST_UNDECIDED;
    }
    const unsigned long long m = __ballot(undecided);
    if (m) {
        const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(n_list, (uint32_t)__popcll(m));
        base = __shfl(base, leader);
        if (undecided) list[base + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)v;
    }
}
__global__ void __launch_bounds__(256)
    dilate_round_kernel(const uint32_t *__restrict__ ids, uint8_t *state, const int32_t *__restrict__ list,
                        const uint32_t n_list, uint32_t *__restrict__ n_left, const Vol G) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    bool still = false;
    if (i < (long long)n_list) {
        const long long v = list[i];
        if (state[v] == ST_UNDECIDED) {
            const uint32_t a = ids[v];
            bool killed = false, wait = false;
            face_neighbours(G, v, [&](long long w) {
                const uint32_t b = ids[w];
                if (b != 0u && b < a) {
                    const uint8_t sw = state[w];
                    killed |= sw == ST_SURVIVOR;
                    wait |= sw == ST_UNDECIDED;
                }
            });
            if (killed) state[v] = ST_DEAD;
            else if (!wait) state[v] = ST_SURVIVOR;
            else still = true;
        }
    }
    const unsigned long long m = __ballot(still);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(n_left, (uint32_t)__popcll(m));
}
__global__ void __launch_bounds__(256)
    dilate_write_kernel(const uint32_t *__restrict__ ids, const uint8_t *__restrict__ state, uint32_t *__restrict__ out,
                        const Vol G) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (v >= G.V) return;
    uint32_t best = state[v] == ST_SURVIVOR ? ids[v] : 0u;
    face_neighbours(G, v, [&](long long w) {
        if (state[w] == ST_SURVIVOR) { const uint32_t b = ids[w]; best = b > best ? b : best; }
    });
    out[v] = best;
}

struct DilateWork {
    uint8_t *state;      // [V]
    int32_t *list;       // [V]: the voxels round 0 left undecided
    uint32_t *counters;  // [0] list length, [1] undecided after the current round
};
static DilateWork dilate_layout(Carver &c, long long V) {
    DilateWork W;
    W.state = c.take<uint8_t>((size_t)V);
    W.list = c.take<int32_t>((size_t)V);
    W.counters = (uint32_t *)c.take_bytes(256);
    return W;
}
size_t post_dilate_workspace_bytes(long long V) { Carver c(nullptr); dilate_layout(c, V); return c.used; }

// out != in.  *rounds = 1 + the number of sweeps over the list.  Synchronises.
hipError_t run_post_dilate(const uint32_t *in, uint32_t *out, int Z, int Y, int X, int *rounds, void *work, hipStream_t s) {
    Vol G;
    G.Z = Z; G.Y = Y; G.X = X;
    G.YX = (long long)Y * X;
    G.V = G.YX * Z;
    PPP_GRID_CHECK((G.V + 255) / 256, 256);
    Carver carver(work);
    const DilateWork W = dilate_layout(carver, G.V);
    const dim3 block(256), vgrid((unsigned)((G.V + 255) / 256));
    hipError_t e;
    if ((e = hipMemsetAsync(W.counters, 0, 8, s)) != hipSuccess) return e;
    dilate_round0_kernel<<<vgrid, block, 0, s>>>(in, W.state, W.list, W.counters, G);
    uint32_t n_list = 0;
    if ((e = hipMemcpyAsync(&n_list, W.counters, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    *rounds = 1;
    uint32_t left = n_list;
    while (left > 0) {
        if ((e = hipMemsetAsync(W.counters + 1, 0, 4, s)) != hipSuccess) return e;
        dilate_round_kernel<<<dim3((n_list + 255) / 256), block, 0, s>>>(in, W.state, W.list, n_list, W.counters + 1, G);
        uint32_t now = 0;
        if ((e = hipMemcpyAsync(&now, W.counters + 1, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        ++*rounds;
        // the undecided voxel of smallest id always decides: a round without progress cannot happen
        if (now >= left) return hipErrorUnknown;
        left = now;
    }
    dilate_write_kernel<<<vgrid, block, 0, s>>>(in, W.state, out, G);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// clean_mask
// ---------------------------------------------------------------------------------------------
// Union-find over linear voxel indices: parent[v] <= v always, roots are the smallest index of their
// tree.  Every access to `parent` during the union pass is an agent-scope atomic (the eight XCDs keep
// private L2s); a link is made by atomicMin on a root, whose return value tells whether it still was one.
__device__ __forceinline__ int32_t cc_find(int32_t *parent, int32_t x) {
    for (;;) {
        const int32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
}
__device__ __forceinline__ void cc_unite(int32_t *parent, int32_t a, int32_t b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;            // a had been linked meanwhile: join what it was linked to with b
    }
}
__global__ void __launch_bounds__(256)
    cc_init_kernel(const uint8_t *__restrict__ mask, int32_t *__restrict__ parent, const long long V) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (v < V) parent[v] = mask[v] ? (int32_t)v : -1;
}
// the 13 forward neighbours (bits 14 .. 26 of the structure, bit = (dz+1)*9 + (dy+1)*3 + (dx+1)); the
// structure is centrosymmetric, so the backward ones are some other voxel's forward ones
__global__ void __launch_bounds__(256)
    cc_union_kernel(const uint8_t *__restrict__ mask, int32_t *parent, const Vol G, const uint32_t structure) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (v >= G.V || !mask[v]) return;
    const int x = (int)(v % G.X), y = (int)((v / G.X) % G.Y), z = (int)(v / G.YX);
    for (int bit = 14; bit < 27; ++bit) {
        if (!((structure >> bit) & 1u)) continue;
        const int zz = z + bit / 9 - 1, yy = y + (bit / 3) % 3 - 1, xx = x + bit % 3 - 1;
        if (zz < 0 || zz >= G.Z || yy < 0 || yy >= G.Y || xx < 0 || xx >= G.X) continue;
        const long long w = (long long)zz * G.YX + (long long)yy * G.X + xx;
        if (mask[w]) cc_unite(parent, (int32_t)v, (int32_t)w);
    }
}
// label = root + 1 (0: background); counters[0] += roots
__global__ void __launch_bounds__(256)
    cc_label_kernel(int32_t *parent, uint32_t *__restrict__ lab, const long long V, uint32_t *__restrict__ counters) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    bool root = false;
    if (v < V) {
        const int32_t p = parent[v];
        root = p == (int32_t)v;
        lab[v] = p < 0 ? 0u : (uint32_t)cc_find(parent, p) + 1u;
    }
    const unsigned long long m = __ballot(root);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(&counters[0], (uint32_t)__popcll(m));
}
__global__ void __launch_bounds__(256)
    cc_out_kernel(const uint32_t *__restrict__ lab, const uint32_t *__restrict__ counts, const long long size,
                  uint8_t *__restrict__ out, const long long V, uint32_t *__restrict__ counters) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    bool kept_root = false;
    if (v < V) {
        const uint32_t l = lab[v];
        const bool keep = l != 0u && (long long)counts[l] > size;
        out[v] = keep ? 1 : 0;
        kept_root = keep && l == (uint32_t)v + 1u;
    }
    const unsigned long long m = __ballot(kept_root);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(&counters[1], (uint32_t)__popcll(m));
}

struct CleanWork {
    int32_t *parent;     // [V]
    uint32_t *lab;       // [V]
    uint32_t *counts;    // [V + 2]: voxels per label (labels are 1 .. V)
    uint32_t *counters;  // [0] components, [1] components kept, [2] id out of range (cannot happen)
};
static CleanWork clean_layout(Carver &c, long long V) {
    CleanWork W;
    W.parent = c.take<int32_t>((size_t)V);
    W.lab = c.take<uint32_t>((size_t)V);
    W.counts = c.take<uint32_t>((size_t)V + 2);
    W.counters = (uint32_t *)c.take_bytes(256);
    return W;
}
size_t post_clean_mask_workspace_bytes(long long V) { Carver c(nullptr); clean_layout(c, V); return c.used; }

// out may be mask.  Synchronises (the two counters go to the host).
hipError_t run_post_clean_mask(const uint8_t *mask, uint8_t *out, int Z, int Y, int X, uint32_t structure,
                               long long size, long long *n_found, long long *n_kept, void *work, hipStream_t s) {
    Vol G;
    G.Z = Z; G.Y = Y; G.X = X;
    G.YX = (long long)Y * X;
    G.V = G.YX * Z;
    PPP_GRID_CHECK((G.V + 255) / 256, 256);
    Carver carver(work);
    const CleanWork W = clean_layout(carver, G.V);
    const dim3 block(256), vgrid((unsigned)((G.V + 255) / 256));
    hipError_t e;
    if ((e = hipMemsetAsync(W.counts, 0, ((size_t)G.V + 2) * 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.counters, 0, 12, s)) != hipSuccess) return e;
    cc_init_kernel<<<vgrid, block, 0, s>>>(mask, W.parent, G.V);
    cc_union_kernel<<<vgrid, block, 0, s>>>(mask, W.parent, G, structure);
    cc_label_kernel<<<vgrid, block, 0, s>>>(W.parent, W.lab, G.V, W.counters);
    if ((e = launch_count_ids(W.lab, G.V, (uint32_t)G.V, W.counts, W.counters + 2, s)) != hipSuccess) return e;
    cc_out_kernel<<<vgrid, block, 0, s>>>(W.lab, W.counts, size, out, G.V, W.counters);
    uint32_t h[2] = {0, 0};
    if ((e = hipMemcpyAsync(h, W.counters, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    *n_found = h[0];
    *n_kept = h[1];
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// fg_filter: postprocess_fg (PatchPerPix/util/postprocess.py:122-199)
// ---------------------------------------------------------------------------------------------
// 26-connected components of the mask; a component of more than `compsize` voxels is BIG, the others are
// SMALL.  A small component stays iff one of its voxels lies at a squared distance < min_d2 from a voxel
// of a big one (min_d2 = 0: no small component stays, and no distance transform runs).  Integers only:
// the host turns the reference's `dist >= max_distance_to_fg` into min_d2 once.  Labels are root + 1 with
// the root the smallest raster index of the component, so ascending label order is scipy's numbering,
// and the surviving components numbered 1, 2, ... in that order are scipy's labels of the cleaned mask.
__global__ void __launch_bounds__(256)
    fg_feature_kernel(const uint32_t *__restrict__ lab, const uint32_t *__restrict__ counts, const long long compsize,
                      uint8_t *__restrict__ feature, const long long V, uint32_t *__restrict__ counters) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    bool small_root = false;
    if (v < V) {
        const uint32_t l = lab[v];
        const bool big = l != 0u && (long long)counts[l] > compsize;
        feature[v] = big ? 1 : 0;
        small_root = l == (uint32_t)v + 1u && !big;
    }
    const unsigned long long m = __ballot(small_root);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(&counters[1], (uint32_t)__popcll(m));
}
// one atomicMin per voxel of a small component: at most `compsize` of them share an address
__global__ void __launch_bounds__(256)
    fg_min_d2_kernel(const uint32_t *__restrict__ lab, const uint32_t *__restrict__ counts, const long long compsize,
                     const uint32_t *__restrict__ d2, uint32_t *__restrict__ mind2, const long long V) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (v >= V) return;
    const uint32_t l = lab[v];
    if (l != 0u && (long long)counts[l] <= compsize) atomicMin(&mind2[l], d2[v]);
}
// in place: table[i] = voxels of label i  ->  1 when label i stays; counters[2] += small components removed
__global__ void __launch_bounds__(256)
    fg_keep_kernel(uint32_t *__restrict__ table, const uint32_t *__restrict__ mind2, const size_t slots,
                   const long long compsize, const uint32_t min_d2, uint32_t *__restrict__ counters) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    bool removed = false;
    if (i < slots) {
        const uint32_t c = table[i];
        const bool present = i != 0 && c != 0u;
        const bool keep = present && ((long long)c > compsize || (min_d2 != 0u && mind2[i] < min_d2));
        removed = present && !keep;
        table[i] = keep ? 1u : 0u;
    }
    const unsigned long long m = __ballot(removed);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(&counters[2], (uint32_t)__popcll(m));
}
__global__ void __launch_bounds__(256)
    fg_out_kernel(const uint32_t *__restrict__ lab, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ rank,
                  uint8_t *__restrict__ fg, uint32_t *__restrict__ inst, const long long V) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (v >= V) return;
    const uint32_t l = lab[v];
    const bool k = l != 0u && keep[l] != 0u;
    fg[v] = k ? 1 : 0;
    if (inst) inst[v] = k ? rank[l] + 1u : 0u;
}

struct FgWork {
    CleanWork cc;        // parent, labels, counts (then keep flags), counters: [0] found, [1] small, [2] removed, [3] bad id
    uint8_t *feature;    // [V]: voxels of big components
    uint32_t *d2;        // [V]: min(squared distance to a feature, min_d2)
    EdtWork edt;
    uint32_t *mind2;     // [V + 2]: per label, the minimum of d2 over its voxels
    uint32_t *rank;      // [V + 2]: exclusive scan of the keep flags
    void *temp;
    size_t temp_bytes, slots;
};
static FgWork fg_layout(Carver &c, long long V) {
    FgWork W;
    W.cc = clean_layout(c, V);
    W.slots = (size_t)V + 2;
    W.feature = c.take<uint8_t>((size_t)V);
    W.d2 = c.take<uint32_t>((size_t)V);
    W.edt = edt_layout(c, V);
    W.mind2 = c.take<uint32_t>(W.slots);
    W.rank = c.take<uint32_t>(W.slots);
    size_t tb = 0;
    (void)rocprim::exclusive_scan(nullptr, tb, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, W.slots,
                                  rocprim::plus<uint32_t>(), (hipStream_t)0);
    W.temp_bytes = up256(tb);
    W.temp = c.take_bytes(W.temp_bytes);
    return W;
}
size_t post_fg_filter_workspace_bytes(long long V) { Carver c(nullptr); fg_layout(c, V); return c.used; }

// fg may be mask; inst may be NULL.  Synchronises once (stats go to the host).  Without a big component
// the transform still runs and fills d2 with min_d2: no small component is below it, all are removed --
// the minimum over an empty set -- and the stream is not synchronised a second time to find that out.
hipError_t run_post_fg_filter(const uint8_t *mask, uint8_t *fg, uint32_t *inst, int Z, int Y, int X, long long compsize,
                              uint32_t min_d2, long long *stats, void *work, hipStream_t s) {
    Vol G;
    G.Z = Z; G.Y = Y; G.X = X;
    G.YX = (long long)Y * X;
    G.V = G.YX * Z;
    PPP_GRID_CHECK((G.V + 255) / 256, 256);
    Carver carver(work);
    const FgWork W = fg_layout(carver, G.V);
    const dim3 block(256), vgrid((unsigned)((G.V + 255) / 256)), sgrid((unsigned)((W.slots + 255) / 256));
    hipError_t e;
    if ((e = hipMemsetAsync(W.cc.counts, 0, W.slots * 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.cc.counters, 0, 16, s)) != hipSuccess) return e;
    cc_init_kernel<<<vgrid, block, 0, s>>>(mask, W.cc.parent, G.V);
    cc_union_kernel<<<vgrid, block, 0, s>>>(mask, W.cc.parent, G, 0x7FFFFFFu);
    cc_label_kernel<<<vgrid, block, 0, s>>>(W.cc.parent, W.cc.lab, G.V, W.cc.counters);
    if ((e = launch_count_ids(W.cc.lab, G.V, (uint32_t)G.V, W.cc.counts, W.cc.counters + 3, s)) != hipSuccess) return e;
    fg_feature_kernel<<<vgrid, block, 0, s>>>(W.cc.lab, W.cc.counts, compsize, W.feature, G.V, W.cc.counters);
    if (min_d2 != 0u) {
        if ((e = hipMemsetAsync(W.mind2, 0xFF, W.slots * 4, s)) != hipSuccess) return e;
        if ((e = launch_edt_sq(W.feature, W.d2, Z, Y, X, min_d2, W.edt, s)) != hipSuccess) return e;
        fg_min_d2_kernel<<<vgrid, block, 0, s>>>(W.cc.lab, W.cc.counts, compsize, W.d2, W.mind2, G.V);
    }
    fg_keep_kernel<<<sgrid, block, 0, s>>>(W.cc.counts, W.mind2, W.slots, compsize, min_d2, W.cc.counters);
    size_t tb = W.temp_bytes;
    if ((e = rocprim::exclusive_scan(W.temp, tb, W.cc.counts, W.rank, 0u, W.slots, rocprim::plus<uint32_t>(), s)) != hipSuccess)
        return e;
    fg_out_kernel<<<vgrid, block, 0, s>>>(W.cc.lab, W.cc.counts, W.rank, fg, inst, G.V);
    uint32_t h[3] = {0, 0, 0};
    if ((e = hipMemcpyAsync(h, W.cc.counters, 12, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    stats[0] = h[0];
    stats[1] = h[1];
    stats[2] = h[2];
    stats[3] = (long long)h[0] - (long long)h[2];
    return hipGetLastError();
}

}  // namespace ppp
