// ppp_cover.hip -- S3, the greedy foreground cover, as an EXACT priority-parallel algorithm.
//
// Reference: foreground_cover.py:111-180 (computeForegroundCoverLoop) walks the ranked patch
// list sequentially: a patch is selected iff more than pixTh voxels of the still uncovered mask
// lie inside its window where its prediction is > fc_threshold; those voxels are then cleared.
//
// The outcome for patch i only depends on the selected patches of HIGHER rank whose windows
// overlap win(i) (centres within p-1 per axis).  Hence rounds of
//   count   : h_i = |mask & win_i & bits_i| for every undecided patch; h_i <= pixTh can never
//             recover (the mask only shrinks) -> decided "not selected" at once;
//   ready   : an undecided patch is ready when no undecided patch of higher rank lies within
//             p-1 of it (3-d min filter over the volume of undecided ranks);
//   select  : every ready patch is selected and clears its voxels.  Ready patches never
//             overlap each other, and when i is decided every higher-ranked overlapping patch
//             is decided and no lower-ranked overlapping one has touched the mask, so win(i)
//             is exactly what the sequential loop would see at i's turn.
// reproduce the sequential result.  The loop's stop rule (it ends as soon as the interior of
// the mask is empty) is applied afterwards from the per-patch "cleared interior voxels"
// counts, in rank order (host side, foreground_cover.py driver).
//
// The undecided patches live in a volume (rank k at the patch centre), and every kernel of a
// round is a coalesced sweep over that volume: no lists, no compaction, no atomics on the data
// path.  A patch is only recounted when a patch selected in the previous round overlaps it
// (the selecting wave marks the (2p-1)^3 box of centres it can affect in a byte volume), the
// recount is one load stage for a group of lanes, and the host only synchronises once per batch
// of rounds.
//
// The sweeps at volumes that fit the caches (140^3, 7^3: 240 cover + 48 thinning rounds per step).
// profiles/r07_a_*_kernel_stats.txt has a cover round at 31 + 25 + 17 = 73 us and a thinning round at
// 38 + 31 + 18 = 87 us of kernel time (xy minimum, count, select) for sweeps whose bytes -- 11 to 44 MB,
// all cache resident -- cost 5-8 us at the rates the same kernels reach on large volumes.  The time was
// dependent latency inside a workgroup and launches of more than one generation of workgroups:
//   xy minimum  a staging loop of 14 serial load -> wait -> LDS write trips, 2 r + 1 LDS reads per output
//               and pass, 36 % of the lanes on padding -> cover_minfilter_xy_cubic_kernel (see there);
//   count       670 workgroups of 1024 threads, 512 resident -> 512 threads x 8 voxels, all resident, eight
//               loads in flight per pass.  ONE sweep, two instantiations: cover_count_kernel and
//               thin_count_kernel load and classify their voxels (ranks and witnesses / keys), then share the
//               compaction (compact_marked) and the window recount (group_hits);
//   select      one voxel per thread, 10 719 workgroups, each the chain own value -> own slice of the
//               filtered volume -> eight voxels per thread, both loads of all eight issued together
//               (ready_voxels).  ONE body (select_body) over what the algorithm makes of a key (CoverPick,
//               ThinPick): cover_select_kernel, cover_select_marked_kernel and thin_select_kernel instantiate it.
// After that (profiles/r12_a_*_kernel_stats.txt: count 27.5 / 21 us, select 17.2 / 25 us per launch, cover /
// thinning) the time left in count and select was again load latency paid in series inside a launch:
//   recount     a thread walked its patch's window plane by plane, each plane behind the last one's sum and the
//               next word of the bit string (up to 12 dependent stages at 7^3; the thinning row by row: 49), after
//               reloading the rank -> a GROUP of lanes per listed patch strides over the window rows, every load
//               of a patch in flight at once, sum and witness by shuffles, the table row carried in the list
//               (group_hits, compact_marked);
//   classify    the dirty bytes were read one by one, each behind the store that clears the one before; the
//               addresses of the witness words cost some 1 800 instructions a thread, most of them 64-bit
//               divisions -> the bytes asked for with the ranks, rows by steps (cover_count_kernel);
//   other slices  up to 2 (pz - 1) = 12 passes over the slices, each behind a wave-wide ballot -> the wave's few
//               candidates are dealt to groups of 16 lanes, one slice a lane, one stage (ready_voxels);
//   winners     one after another, each the chain key -> bit rows and mask rows -> atomics -> keys from the
//               registers, the rows of two winners asked for together, before the first atomic (select_body).
// profiles/r13_a_*: count 22.6 / 12.8 us, select 10.3 / 16.4 us, the step 173.6 -> 169.4 ms (medians of three).
// Measured and dropped (same profiles): the recount in two stages -- the first plane of rows, the others only
// where that does not settle "more than pix_th", second words only where the bits reach them -- asks for a
// seventh of the words for a surviving patch, and was SLOWER: cover 12.8 ms per step against 11.3 (parent
// 14.1): the recount's time is the number of its dependent stages, not its loads.  Four winners of a wave
// together: 78 / 88 VGPRs (two: 57 / 65), the 1 340 select workgroups no longer resident at once.  The witness
// loaded with the rank (2 more bytes per voxel where the sweep is bandwidth-bound, 512^3): not measured.
// The round keeps its three launches and every step leaves the state it left before (tests/test_shard_steps.py
// compares it step by step, tests/test_cover_sweeps.py the filter alone and the number of rounds):
//   * the xy minimum is NOT fused into select -- a workgroup would read a neighbour's rank that another
//     workgroup of the same launch has just retired and select a lower ranked overlapping patch whose
//     count predates the neighbour's clears; nbr_min is the snapshot that prevents it;
//   * count is NOT fused into the minimum -- every rejection would unblock its neighbours a round later;
//   * one persistent launch with a grid barrier per step was tried before and dropped.
// What a round cannot beat is three dependent launches: tools/ubench/launch_floor.hip times a chain of
// empty kernels at the grids of the three sweeps.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "ppp_kernels.hpp"

namespace ppp {

// "no patch here" of a key / filter volume: the largest value of the element type's byte pattern 0x7F..
template <typename T> struct FilterNone;
template <> struct FilterNone<int32_t> { static constexpr int32_t value = 0x7F7F7F7F; };
template <> struct FilterNone<long long> { static constexpr long long value = 0x7F7F7F7F7F7F7F7Fll; };
static constexpr int32_t RANK_NONE = FilterNone<int32_t>::value;
static constexpr int COVER_BATCH = 8;   // rounds per host synchronisation

// What a round works on, over the key type K: int32_t ranks in the greedy cover, long long keys in the
// thinning.  The head of every cover / thinning workspace (round_layout): a launcher that needs nothing
// else -- filter, alive, close, zones -- carves only this and serves both.
template <typename K> struct RoundArrays {
    K *key_vol, *nbr_min, *tmp;          // [V] each
    uint8_t *dirty;                      // [V]
    uint32_t *mbits;                     // [Z*Y][XW] running mask, one bit per voxel
    int32_t *counters;                   // [COVER_BATCH]
};
struct CoverWork : RoundArrays<int32_t> {
    int32_t *loc_vol;                    // [V] sharded cover only: index into the rank's own
                                         // state / cleared / bits tables, -1 off the own centres
    uint16_t *witness;                   // [V] pix_th == 0: ONE voxel of the window that the patch
                                         // centred here still covered at its last recount: window
                                         // row (dz * py + dy) << 5 | x offset (px <= 32: five bits; the row
                                         // keeps eleven, witness_ok); 0xFFFF = none known
};
static constexpr uint16_t WIT_NONE = 0xFFFFu;
// the 16-bit witness holds a window row in eleven bits (0x7FF | 31 would read as WIT_NONE); taller
// windows run without witnesses: dirty marks + windowed recounts, as the pix_th > 0 passes do
static inline bool witness_ok(const Geo &G) { return G.pz * G.py < 2047 && G.px <= 32; }

// words per row of the bit mask: one spare word so a window may be read as two words
__host__ __device__ __forceinline__ int row_words(const Geo &G) { return (G.X + 31) / 32 + 1; }

__device__ __forceinline__ void centre_of(const Geo &G, long long c, int &cz, int &cy, int &cx) {
    if (G.V < (1ll << 31)) {                                    // (32-bit divisions where the volume allows them)
        const int ci = (int)c, plane = G.X * G.Y;
        cz = ci / plane;
        cy = (ci - cz * plane) / G.X;
        cx = ci - cz * plane - cy * G.X;
        return;
    }
    cx = (int)(c % G.X);
    cy = (int)((c / G.X) % G.Y);
    cz = (int)(c / ((long long)G.X * G.Y));
}

// n (<= 32) bits starting at bit `start` of a little-endian bit string held in 32-bit words;
// `limit` = number of readable words
__device__ __forceinline__ uint32_t bit_window(const uint32_t *w, int start, int n, int limit) {
    const int i = start >> 5, sh = start & 31;
    const uint32_t lo = w[i];
    const uint32_t hi = (i + 1 < limit) ? w[i + 1] : 0u;
    const uint32_t v = (uint32_t)((((unsigned long long)hi << 32) | lo) >> sh);
    return n >= 32 ? v : (v & ((1u << n) - 1u));
}

// byte mask -> bit mask (thread per word) and back (thread per voxel)
__global__ void __launch_bounds__(256)
    cover_pack_kernel(const uint8_t *__restrict__ mask, uint32_t *__restrict__ mbits, const Geo G) {
    const int XW = row_words(G);
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (t >= (long long)G.Z * G.Y * XW) return;
    const int w = (int)(t % XW);
    const long long row = t / XW;
    uint32_t v = 0;
    for (int i = 0; i < 32; ++i) {
        const int x = w * 32 + i;
        if (x < G.X && mask[row * G.X + x] != 0) v |= 1u << i;
    }
    mbits[t] = v;
}
__global__ void __launch_bounds__(256)
    cover_unpack_kernel(const uint32_t *__restrict__ mbits, uint8_t *__restrict__ mask, const Geo G) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (v >= G.V) return;
    const int x = (int)(v % G.X);
    const long long row = v / G.X;
    // keep the caller's byte values where the bit survived
    if (!((mbits[row * row_words(G) + (x >> 5)] >> (x & 31)) & 1u)) mask[v] = 0;
}

// state[k] == 0: undecided.  Enter every undecided patch into the rank volume.
__global__ void __launch_bounds__(256)
    cover_init_kernel(const long long *__restrict__ lin, const int32_t *__restrict__ state, int n,
                      int32_t *__restrict__ rank_vol) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n && state[k] == 0) rank_vol[lin[k]] = k;
}

// Count step.  Thread per voxel; a workgroup of 1024 voxels first COMPACTS its undecided patches
// whose neighbourhood changed into a list in LDS (and consumes the dirty marks; "any patch still
// undecided" is flagged), then its first lanes recount them (per row of the window: mask bits AND
// patch bits, popcount) and reject those that can cover <= pix_th voxels.  Recounting inside the
// per-voxel sweep left one or two lanes of almost every wave walking the 49-row window while the
// others idled -- a few per cent of the voxels are dirty candidates, scattered.  (A global list
// costs a same-address atomic per wave: 4x slower than no compaction at all.)
// (512 threads x 8 voxels: the 4096 voxels of a workgroup as before, but four workgroups fit a CU, so the
// 670 workgroups of 140^3 are resident at once -- 1024 x 4 left a second generation that was 30 % full --
// and a thread has eight loads in flight per pass instead of four)
static constexpr int COUNT_THREADS = 512;
static constexpr int COUNT_VPT = 8;     // voxels per thread of the count sweeps
// (at least 6 waves a SIMD = three workgroups a CU: with more than 80 VGPRs the 670 workgroups of 140^3 are not
// resident at once; the recount's 32 loads in flight would take 89)
#define PPP_COUNT_BOUNDS __launch_bounds__(COUNT_THREADS, 6)
static inline dim3 count_grid(const Geo &G) {
    return dim3((unsigned)((G.V + COUNT_THREADS * COUNT_VPT - 1) / (COUNT_THREADS * COUNT_VPT)));
}

// First phase of a count sweep, after a kernel has loaded and classified its voxels (alive: an undecided
// patch of the rank's own; marked: its neighbourhood changed): the workgroup's voxels that are both are
// compacted into s_list (offsets from the block's first voxel; *s_n was zeroed before a barrier).  Returns
// their number, after a barrier.
// (row[j]: the voxel's row of the bit / state tables, carried with the list entry in s_row -- the recount
// starts from LDS, not from another load of the rank before the bits can be asked for)
__device__ __forceinline__ int compact_marked(const bool (&alive)[COUNT_VPT], const bool (&marked)[COUNT_VPT],
                                              const int (&row)[COUNT_VPT], uint16_t *s_list, int32_t *s_row,
                                              int *s_n, int32_t *__restrict__ n_alive) {
    bool rest = false;
#pragma unroll
    for (int j = 0; j < COUNT_VPT; ++j) {
        const unsigned long long m = __ballot(alive[j] && marked[j]);
        if (m != 0ull) {
            const int lane = threadIdx.x & 63;
            int base = 0;
            if (lane == 0) base = atomicAdd(s_n, __popcll(m));
            base = __shfl(base, 0);
            if (alive[j] && marked[j]) {
                const int at = base + __popcll(m & ((1ull << lane) - 1ull));
                s_list[at] = (uint16_t)(j * COUNT_THREADS + threadIdx.x);
                s_row[at] = row[j];
            }
        }
        rest = rest || (alive[j] && !marked[j]);
    }
    // "is any patch still undecided" AFTER this step: a plain store of the same value from
    // every wave that has one that is not recounted now (same-address atomics from ~V/64
    // waves would dominate the kernel); the recounted ones report after their recount if they survive
    if (__ballot(rest) != 0 && (threadIdx.x & 63) == 0) *n_alive = 1;
    __syncthreads();
    return *s_n;
}

// n (<= 32) bits from bit `sh` (< 32) of the 64-bit string hi:lo.  (hi may be any readable word where the
// bits do not reach it: what it shifts in lies at or above bit 32 - sh >= n)
__device__ __forceinline__ uint32_t window_of(uint32_t lo, uint32_t hi, int sh, int n) {
    const uint32_t v = (uint32_t)((((unsigned long long)hi << 32) | lo) >> sh);
    return n >= 32 ? v : (v & ((1u << n) - 1u));
}

__device__ __forceinline__ uint32_t low_bits(int n) { return n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u); }

// Second phase: |mask bits & patch bits| over the R = pz * py rows of the window of the patch centred at voxel
// v (b: its bit string, px bits per row), by a GROUP of gw lanes (a power of two, at most a wave; sub = the
// lane's place in it).  Lane `sub` takes the rows sub, sub + gw, ...: it asks for the two mask words and the two
// bit-string words of RECOUNT_ROWS rows at once -- every address follows from v and the row number alone,
// so all loads of a patch are in flight together -- forms the rows' hits, and the group adds up by
// shuffles.  Every lane of the group returns the full count; nothing stops early ("more than pix_th" is
// decided from the sum: the same decision), a rejected patch costs what a surviving one does.
//   WITNESS     wit = the first covered voxel in row order, window row << 5 | x offset: the minimum of the
//               lanes' codes (WIT_NONE, "none", is the largest).
// The sequential walk this replaces -- plane by plane, each plane behind the last one's sum and the next
// word of the bit string, up to 12 dependent load stages at 7^3, 49 in the thinning -- was the count kernels'
// time (profiles/r12_a_*_kernel_stats.txt: 27.5 and 21 us for sweeps whose bytes cost 5-8 us).
// All lanes of a wave call this together (the shuffles); a group without a patch repeats another one's.
static constexpr int RECOUNT_ROWS = 7;      // rows a lane has in flight (8 spills: the count kernels are held to 80 VGPRs)
// lanes per listed patch: the fewest that leave a lane at most RECOUNT_ROWS rows (5^3: 4 lanes x 7 rows, 7^3: 8 x
// 7, 64 patches per trip of a workgroup; 9^3: 16 x 6; 1 x 25 x 25: 4 x 7), a wave and several trips
// beyond 448 rows
__device__ __forceinline__ int recount_group(const Geo &G) {
    int w = 1;
    while (w < 64 && w * RECOUNT_ROWS < G.pz * G.py) w <<= 1;
    return w;
}
template <bool WITNESS>
__device__ __forceinline__ int group_hits(const uint32_t *__restrict__ mbits, const uint32_t *__restrict__ b,
                                          const long long v, const int sub, const int gw, unsigned &wit,
                                          const Geo &G) {
    const int words = (G.C + 31) / 32, XW = row_words(G), R = G.pz * G.py;
    int cz, cy, cx;
    centre_of(G, v, cz, cy, cx);
    const int start = cx - G.rx, wi = start >> 5, sh = start & 31;
    const uint32_t *m0 = mbits + ((long long)(cz - G.rz) * G.Y + (cy - G.ry)) * XW;
    int hits = 0;
    unsigned code = WIT_NONE;
    const int step_z = gw / G.py, step_y = gw - step_z * G.py;  // (one division a trip: the rows after the first by steps)
    for (int r0 = sub; r0 < R; r0 += gw * RECOUNT_ROWS) {
        uint32_t ml[RECOUNT_ROWS], mh[RECOUNT_ROWS], bl[RECOUNT_ROWS], bh[RECOUNT_ROWS];
        int dz = r0 / G.py, dy = r0 - dz * G.py;
#pragma unroll
        for (int i = 0; i < RECOUNT_ROWS; ++i) {
            // (a row past the window reads the last one: clamped, no branch between the loads)
            const bool in = r0 + i * gw < R;
            const int bi = ((in ? r0 + i * gw : R - 1) * G.px) >> 5;
            const uint32_t *row = m0 + ((long long)(in ? dz : G.pz - 1) * G.Y + (in ? dy : G.py - 1)) * XW;
            ml[i] = row[wi];
            mh[i] = row[min(wi + 1, XW - 1)];
            bl[i] = b[bi];
            bh[i] = b[min(bi + 1, words - 1)];
            dz += step_z;
            dy += step_y;
            if (dy >= G.py) { dy -= G.py; ++dz; }
        }
#pragma unroll
        for (int i = 0; i < RECOUNT_ROWS; ++i) {
            const int r = r0 + i * gw;
            if (r < R) {
                const uint32_t hm = window_of(ml[i], mh[i], sh, G.px) & window_of(bl[i], bh[i], (r * G.px) & 31, G.px);
                hits += __popc(hm);
                if (WITNESS && hm) code = min(code, ((unsigned)r << 5) | (unsigned)__builtin_ctz(hm));
            }
        }
    }
    for (int o = gw >> 1; o > 0; o >>= 1) {
        hits += __shfl_xor(hits, o);
        if (WITNESS) code = min(code, (unsigned)__shfl_xor((int)code, o));
    }
    wit = code;
    return hits;
}

__global__ void PPP_COUNT_BOUNDS
    cover_count_kernel(const uint32_t *__restrict__ mbits, const uint32_t *__restrict__ bits,
                       uint8_t *__restrict__ dirty, const int pix_th, int32_t *__restrict__ state,
                       int32_t *__restrict__ rank_vol, int32_t *__restrict__ n_alive,
                       const int32_t *__restrict__ loc_vol, uint16_t *__restrict__ witness,
                       const long long bits_vox, const Geo G) {
    // COUNT_VPT voxels per thread (v = block base + j * COUNT_THREADS + thread: every pass stays coalesced).  The
    // sweep is a chain of dependent loads per voxel -- rank, then witness, then one word of the mask --
    // and its time was their latency (1.17 ms for the 134 M voxels of 512^3 with one voxel per thread:
    // 0.8 TB/s); the loads of a thread's voxels are issued pass by pass, COUNT_VPT in flight each.
    // (the list: 24 KB of LDS, so the four workgroups a CU can hold by threads still fit it)
    __shared__ uint16_t s_list[COUNT_THREADS * COUNT_VPT];
    __shared__ int32_t s_row[COUNT_THREADS * COUNT_VPT];
    __shared__ int s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const long long v0 = blockIdx.x * (long long)(COUNT_THREADS * COUNT_VPT);
    int n;
    {
        const bool use_wit = pix_th == 0 && witness != nullptr;
        long long vv[COUNT_VPT];
        int kk[COUNT_VPT];
        bool alive[COUNT_VPT], marked[COUNT_VPT];
        unsigned wv[COUNT_VPT];
        // (the dirty bytes are asked for with the ranks: read one by one where they are cleared, each load
        // waited behind the store before it -- eight round trips in series in every pass with pix_th > 0)
        uint8_t mark[COUNT_VPT];
#pragma unroll
        for (int j = 0; j < COUNT_VPT; ++j) {
            vv[j] = v0 + j * COUNT_THREADS + threadIdx.x;
            kk[j] = rank_vol[min(vv[j], G.V - 1)];              // (clamped: no branch between the loads)
        }
        if (!use_wit) {
#pragma unroll
            for (int j = 0; j < COUNT_VPT; ++j) mark[j] = dirty[min(vv[j], G.V - 1)];
        }
#pragma unroll
        for (int j = 0; j < COUNT_VPT; ++j)
            if (vv[j] >= G.V) kk[j] = RANK_NONE;
        // sharded: rank_vol holds GLOBAL ranks (also of the neighbour's patches in the halo);
        // only the own centres are worked on, through their local table index
        if (loc_vol) {
            int loc[COUNT_VPT];
#pragma unroll
            for (int j = 0; j < COUNT_VPT; ++j) {
                loc[j] = -1;
                if (kk[j] != RANK_NONE) loc[j] = loc_vol[vv[j]];
            }
#pragma unroll
            for (int j = 0; j < COUNT_VPT; ++j)
                if (kk[j] != RANK_NONE) kk[j] = loc[j] < 0 ? RANK_NONE : loc[j];
        }
        // pix_th == 0 ("does the patch still cover ANY voxel"): a patch stays undecided as long as
        // its witness voxel is uncovered -- one bit of the running mask (16 MB at 512^3: cache
        // resident) decides it, no patch bits are read and no dirty marks are needed; only a patch
        // whose witness was cleared (or that has none yet) is recounted.  On a dense volume a patch
        // is looked at in hundreds of rounds and nearly always survives.
#pragma unroll
        for (int j = 0; j < COUNT_VPT; ++j) {
            alive[j] = kk[j] != RANK_NONE;
            wv[j] = WIT_NONE;
            if (use_wit) { if (alive[j]) wv[j] = witness[vv[j]]; }
            else { marked[j] = vv[j] < G.V && mark[j] != 0; if (marked[j]) dirty[vv[j]] = 0; }
        }
        if (use_wit) {
            uint32_t mw[COUNT_VPT];
            int xb[COUNT_VPT];
            // (row and x of a thread's voxels by steps from its first voxel, the witness row split by a
            // multiplication: written as vv / X, vv % X, wr / py and wr % py per voxel the addresses of the
            // eight mask words were some 1 800 instructions, two thirds of them 64-bit divisions)
            const long long vf = v0 + threadIdx.x;
            long long vrow = G.V < (1ll << 31) ? (long long)((int)vf / G.X) : vf / G.X;
            int vx = (int)(vf - vrow * G.X);
            const int step_row = COUNT_THREADS / G.X, step_x = COUNT_THREADS - step_row * G.X;
            const float inv_py = 1.0f / (float)G.py;
#pragma unroll
            for (int j = 0; j < COUNT_VPT; ++j) {
                mw[j] = 0u; xb[j] = 0;
                if (alive[j] && wv[j] != WIT_NONE) {
                    const int wr = (int)(wv[j] >> 5), xo = (int)(wv[j] & 0x1Fu);
                    // wr / py (wr < 2047): the float quotient is within one of it
                    int wz = (int)((float)wr * inv_py), wy = wr - wz * G.py;
                    if (wy < 0) { --wz; wy += G.py; }
                    if (wy >= G.py) { ++wz; wy -= G.py; }
                    const long long row = vrow + (long long)(wz - G.rz) * G.Y + (wy - G.ry);
                    const int x = vx - G.rx + xo;
                    mw[j] = mbits[row * row_words(G) + (x >> 5)];
                    xb[j] = x & 31;
                }
                vrow += step_row;
                vx += step_x;
                if (vx >= G.X) { vx -= G.X; ++vrow; }
            }
#pragma unroll
            for (int j = 0; j < COUNT_VPT; ++j) marked[j] = alive[j] && ((mw[j] >> xb[j]) & 1u) == 0u;
        }
        n = compact_marked(alive, marked, kk, s_list, s_row, &s_n, n_alive);
    }
    // the listed patches, a group of lanes each (group_hits); a wave's groups take neighbouring entries and
    // every wave runs whole trips: a group past the end repeats the trip's first entry and writes nothing
    const int gw = recount_group(G), per_wave = 64 / gw;
    const int sub = threadIdx.x & (gw - 1), in_wave = (threadIdx.x & 63) / gw;
    for (int base = (threadIdx.x >> 6) * per_wave; base < n; base += COUNT_THREADS / gw) {
        const bool mine = base + in_wave < n;
        const int e = mine ? base + in_wave : base;
        const long long v = v0 + s_list[e];
        const int k = s_row[e];
        // (bits_vox >= 0: the table has a row per VOXEL, its first row belongs to voxel bits_vox)
        const uint32_t *b = bits + (bits_vox >= 0 ? v - bits_vox : (long long)k) * ((G.C + 31) / 32);
        unsigned wit_new;
        const int hits = group_hits<true>(mbits, b, v, sub, gw, wit_new, G);
        if (!mine || sub != 0) continue;
        if (hits <= pix_th) {
            state[k] = 2;
            rank_vol[v] = RANK_NONE;
        } else {
            if (pix_th == 0 && witness != nullptr) witness[v] = (uint16_t)wit_new;
            *n_alive = 1;
        }
    }
}

// 1-d running minimum of width 2*radius+1 along one axis (stride in elements, n along axis)
template <typename T>
__global__ void __launch_bounds__(256)
    cover_minfilter_kernel(const T *__restrict__ in, T *__restrict__ out,
                           const long long V, const int n, const long long stride, const int radius) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int pos = (int)((v / stride) % n);
    T m = FilterNone<T>::value;
    for (int d = -radius; d <= radius; ++d) {
        const int q = pos + d;
        if (q >= 0 && q < n) m = min(m, in[v + (long long)d * stride]);
    }
    out[v] = m;
}

// x and y passes of the running minimum in one kernel: a block owns 8 rows x 64 columns of one
// z-slice, stages them with their (ry, rx) apron in LDS, takes the minimum along x into a second
// LDS array and then along y (one launch and one volume round trip less per round).
// (rows per block by element size: 32 rows of int32 / 16 of int64 -- with the (ry, rx) apron a block
// reads (TY + 2 ry)(64 + 2 rx) elements for TY * 64 results: 1.9 x at 32 rows, 3.75 x at 8)
static constexpr int MF_TX = 64;
template <typename T> struct MfRows { static constexpr int value = sizeof(T) == 4 ? 32 : 16; };
template <typename T, int MF_TY>
__global__ void __launch_bounds__(256)
    cover_minfilter_xy_kernel(const T *__restrict__ in, T *__restrict__ out, const Geo G,
                              const int rx, const int ry) {
    extern __shared__ long long mf_lds_raw[];
    const T RANK_NONE = FilterNone<T>::value;
    T *mf_lds = reinterpret_cast<T *>(mf_lds_raw);
    const int W = MF_TX + 2 * rx, H = MF_TY + 2 * ry;
    T *a = mf_lds;            // [H][W]   input tile with apron
    T *b = mf_lds + H * W;    // [H][MF_TX] minimum along x
    const int x0 = blockIdx.x * MF_TX, y0 = blockIdx.y * MF_TY, z = blockIdx.z;
    const long long zbase = (long long)z * G.Y * G.X;
    for (int i = threadIdx.x; i < H * W; i += 256) {
        const int yy = y0 - ry + i / W, xx = x0 - rx + i % W;
        a[i] = (yy >= 0 && yy < G.Y && xx >= 0 && xx < G.X) ? in[zbase + (long long)yy * G.X + xx] : RANK_NONE;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < H * MF_TX; i += 256) {
        const int r = i / MF_TX, c = i % MF_TX;
        T m = RANK_NONE;
        for (int d = 0; d <= 2 * rx; ++d) m = min(m, a[r * W + c + d]);
        b[i] = m;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < MF_TY * MF_TX; i += 256) {
        const int r = i / MF_TX, c = i % MF_TX;
        const int yy = y0 + r, xx = x0 + c;
        if (yy >= G.Y || xx >= G.X) continue;
        T m = RANK_NONE;
        for (int d = 0; d <= 2 * ry; ++d) m = min(m, b[(r + d) * MF_TX + c]);
        out[zbase + (long long)yy * G.X + xx] = m;
    }
}

// Running minimum of width W over a register array: a[i] <- min(a[i .. i + W - 1]) for i <= L - W, by
// doubling (a[i] covers 2, 4, .. P inputs, P the largest power of two <= W; the last step joins two
// windows of P that overlap by 2 P - W): 4 min per element at W = 13 instead of 12.  In place: every
// step reads entries above the one it writes.
template <typename T, int W, int L>
__device__ __forceinline__ void running_min(T (&a)[L]) {
    static_assert(W >= 1 && L >= W, "window longer than the run");
    constexpr int P = W >= 16 ? 16 : W >= 8 ? 8 : W >= 4 ? 4 : W >= 2 ? 2 : 1;
    static_assert(W < 2 * P, "window of more than 31 elements");
#pragma unroll
    for (int st = 1; st < P; st <<= 1) {
#pragma unroll
        for (int i = 0; i + st < L; ++i) a[i] = min(a[i], a[i + st]);
    }
    if (W > P) {
#pragma unroll
        for (int i = 0; i + W - P < L; ++i) a[i] = min(a[i], a[i + W - P]);
    }
}

// The same two passes for the cubic patches (radius R = p - 1 a template parameter: 2, 4, 6, 8), built
// for the SMALL volumes whose rounds are latency, not bytes (140^3: every volume of a round sits in
// L2 / Infinity Cache).  What the kernel above pays there and this one does not:
//   * its staging loop is one load, one wait and one LDS write per iteration, 14 dependent round trips
//     per wave, each with a division by the run-time tile width.  Here the y pass comes FIRST and straight
//     from global memory: a thread owns one column of the tile and MF_YR + 2 R rows of it, loads them all
//     (clamped addresses, no branch: every load is issued before the first wait; lanes along x, so every
//     load instruction is coalesced), takes the running minimum in registers and leaves MF_YR results in LDS;
//   * 2 r + 1 LDS reads per output and pass.  Here a thread makes a RUN of outputs (MF_YR along y, MF_XR
//     along x) from run + 2 R inputs, by doubling (running_min): 22 loads and 4 min per output / 10 at 7^3
//     in the y pass, 20 LDS reads / 8 in the x pass;
//   * one LDS array instead of two (the x pass reads its run, all threads meet, writes it back in place);
//     lanes walk the ROWS of the array, whose pitch is odd: reads and writes are free of bank conflicts;
//   * tiles of 48 x 40 or 64 x 30, whichever pads the slice less: 140 x 140 is 3 x 4 tiles of 48 x 40
//     (15 % of the launched outputs are padding; 3 x 5 tiles of 64 x 32 made it 36 %) and the 1 680
//     workgroups of 140^3 are resident at once (at most 72 VGPRs, 21 KB of LDS: seven or eight per CU).
// All index arithmetic divides by compile-time constants.
static constexpr int MF_YR = 10, MF_XR = 8;
template <typename T, int R, int TX, int YG>
__global__ void __launch_bounds__(256)
    cover_minfilter_xy_cubic_kernel(const T *__restrict__ in, T *__restrict__ out, const int X, const int Y) {
    constexpr int W = 2 * R + 1, CW = TX + 2 * R, PITCH = CW | 1, TY = YG * MF_YR;
    constexpr int LY = MF_YR + 2 * R, LX = MF_XR + 2 * R;
    constexpr int Y_ITEMS = CW * YG, X_ITEMS = TY * (TX / MF_XR);
    static_assert(TX % MF_XR == 0 && X_ITEMS <= 256, "one x run per thread");
    const T NONE = FilterNone<T>::value;
    __shared__ T tile[TY * PITCH];             // [TY][CW]: minimum along y, then (in place) along x too
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    const int zbase = blockIdx.z * Y * X;      // (a volume has fewer than 2^31 voxels)
#pragma unroll
    for (int it = 0; it < (Y_ITEMS + 255) / 256; ++it) {
        const int i = threadIdx.x + it * 256;
        if (i < Y_ITEMS) {
            const int c = i % CW, g = i / CW;
            const int xx = x0 - R + c, yb = y0 + g * MF_YR - R;
            const bool x_in = xx >= 0 && xx < X;
            const int col = zbase + min(max(xx, 0), X - 1);
            T a[LY];
#pragma unroll
            for (int k = 0; k < LY; ++k) a[k] = in[col + min(max(yb + k, 0), Y - 1) * X];
#pragma unroll
            for (int k = 0; k < LY; ++k)
                if (!x_in || yb + k < 0 || yb + k >= Y) a[k] = NONE;
            running_min<T, W, LY>(a);
#pragma unroll
            for (int k = 0; k < MF_YR; ++k) tile[(g * MF_YR + k) * PITCH + c] = a[k];
        }
    }
    __syncthreads();
    const int r = threadIdx.x % TY, j = threadIdx.x / TY;
    T *run = tile + r * PITCH + j * MF_XR;
    T b[LX];
    if (threadIdx.x < X_ITEMS) {
#pragma unroll
        for (int k = 0; k < LX; ++k) b[k] = run[k];
        running_min<T, W, LX>(b);
    }
    __syncthreads();
    if (threadIdx.x < X_ITEMS) {
#pragma unroll
        for (int k = 0; k < MF_XR; ++k) run[k] = b[k];       // column c of the tile: its first TX entries
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < (TY * TX + 255) / 256; ++it) {
        const int i = threadIdx.x + it * 256;
        const int rr = i / TX, cc = i % TX;
        if (i < TY * TX && y0 + rr < Y && x0 + cc < X) out[zbase + (y0 + rr) * X + x0 + cc] = tile[rr * PITCH + cc];
    }
}

// the cubic kernel's two tiles; false = the launch does not fit the grid limits (the caller falls back)
template <typename T, int R>
static bool minfilter_xy_cubic(const T *in, T *out, const Geo &G, hipStream_t s) {
    constexpr int YG_NARROW = 4, YG_WIDE = 3;            // 48 x 40 and 64 x 30: both 1920 outputs, <= 256 items a pass
    auto tiles = [](int n, int t) { return (n + t - 1) / t; };
    const long long area_narrow = (long long)tiles(G.X, 48) * 48 * tiles(G.Y, YG_NARROW * MF_YR) * (YG_NARROW * MF_YR);
    const long long area_wide = (long long)tiles(G.X, 64) * 64 * tiles(G.Y, YG_WIDE * MF_YR) * (YG_WIDE * MF_YR);
    // (the kernel indexes with 32-bit integers)
    if (G.V >= (1ll << 31) || G.Z > 65535 || tiles(G.Y, YG_WIDE * MF_YR) > 65535) return false;
    if (area_wide <= area_narrow)
        cover_minfilter_xy_cubic_kernel<T, R, 64, YG_WIDE><<<dim3((unsigned)tiles(G.X, 64), (unsigned)tiles(G.Y, YG_WIDE * MF_YR), (unsigned)G.Z), dim3(256), 0, s>>>(in, out, G.X, G.Y);
    else
        cover_minfilter_xy_cubic_kernel<T, R, 48, YG_NARROW><<<dim3((unsigned)tiles(G.X, 48), (unsigned)tiles(G.Y, YG_NARROW * MF_YR), (unsigned)G.Z), dim3(256), 0, s>>>(in, out, G.X, G.Y);
    return true;
}

// x and y passes of the neighbourhood minimum: in -> out (scratch: the x pass when the fused
// kernel's tile does not fit LDS).  The z pass is NOT a sweep of its own: only the few voxels that
// hold an undecided patch need the 3-d minimum, and the select kernels take it over the 2 pz - 1
// slices themselves (one volume write + read and one launch less per round).
// Cubic 3^3 .. 9^3 patches take the kernel with compile-time radii, every other shape (anisotropic, the
// 25-wide 2-d patches, anything whose tile does not fit LDS) the run-time one.
// (rx, ry: the radii -- p - 1 for the cover and the thinning, max(p - 1, 3) for a cover with marks; the
// cubic kernel serves radius p - 1 only)
template <typename T>
static void minfilter_xy(const T *in, T *scratch, T *out, const Geo &G, const int rx, const int ry, hipStream_t s) {
    if (G.px == G.py && G.py == G.pz && rx == G.px - 1 && ry == G.py - 1) {
        bool done = false;
        switch (G.px) {
        case 3: done = minfilter_xy_cubic<T, 2>(in, out, G, s); break;
        case 5: done = minfilter_xy_cubic<T, 4>(in, out, G, s); break;
        case 7: done = minfilter_xy_cubic<T, 6>(in, out, G, s); break;
        case 9: done = minfilter_xy_cubic<T, 8>(in, out, G, s); break;
        default: break;
        }
        if (done) return;
    }
    constexpr int TYB = MfRows<T>::value, TYS = 8;      // rows per block: the tall tile where it fits LDS
    auto lds_of = [&](int ty) { return (size_t)((ty + 2 * ry) * (MF_TX + 2 * rx) + (ty + 2 * ry) * MF_TX) * sizeof(T); };
    auto grid_of = [&](int ty) { return dim3((unsigned)((G.X + MF_TX - 1) / MF_TX), (unsigned)((G.Y + ty - 1) / ty), (unsigned)G.Z); };
    const dim3 vgrid((unsigned)((G.V + 255) / 256)), block(256);
    if (lds_of(TYB) <= 48 * 1024 && G.Z <= 65535) {
        cover_minfilter_xy_kernel<T, TYB><<<grid_of(TYB), block, lds_of(TYB), s>>>(in, out, G, rx, ry);
    } else if (lds_of(TYS) <= 48 * 1024 && G.Y <= 65535 * TYS && G.Z <= 65535) {
        cover_minfilter_xy_kernel<T, TYS><<<grid_of(TYS), block, lds_of(TYS), s>>>(in, out, G, rx, ry);
    } else {
        cover_minfilter_kernel<T><<<vgrid, block, 0, s>>>(in, scratch, G.V, G.X, 1, rx);
        cover_minfilter_kernel<T><<<vgrid, block, 0, s>>>(scratch, out, G.V, G.Y, G.X, ry);
    }
}
template <typename T>
static void minfilter_xy(const T *in, T *scratch, T *out, const Geo &G, hipStream_t s) {
    minfilter_xy<T>(in, scratch, out, G, G.px - 1, G.py - 1, s);
}
// the filter alone, on buffers of the caller (ppp_minfilter_xy: what the tests pin the tiling with)
hipError_t run_minfilter_xy(const void *in, void *scratch, void *out, int elem_bytes, const Geo &G, hipStream_t s) {
    if (elem_bytes == 4) minfilter_xy<int32_t>((const int32_t *)in, (int32_t *)scratch, (int32_t *)out, G, s);
    else if (elem_bytes == 8) minfilter_xy<long long>((const long long *)in, (long long *)scratch, (long long *)out, G, s);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
// minimum over the slices z - (pz-1) .. z + (pz-1) of the xy-filtered volume at voxel v
template <typename T>
__device__ __forceinline__ T zmin_at(const T *__restrict__ xy, long long v, const Geo &G) {
    const long long plane = (long long)G.X * G.Y;
    const int z = (int)(v / plane);
    T m = FilterNone<T>::value;
    for (int d = -(G.pz - 1); d <= G.pz - 1; ++d)
        if (z + d >= 0 && z + d < G.Z) m = min(m, xy[v + (long long)d * plane]);
    return m;
}

// The ready test of the select sweeps, SELECT_VPT voxels per thread (v = first + j * 256: every pass is
// coalesced): "is my value the minimum over the slices z - (pz-1) .. z + (pz-1) of the xy-filtered volume".
// Returns the voxels j for which it is, one bit each; mine[j] = the thread's own values.
// The own value and the own slice of the filtered volume are loaded for all of a thread's voxels before
// anything is tested (one thread per voxel was the dependent chain rank -> nbr_min in 10 719 workgroups of
// 256 at 140^3: five generations, each two memory latencies long).  On a dense volume a patch has a better
// ranked undecided neighbour in its own slice in all but a few thousand cases per round, so most waves read
// ONE slice instead of 2 pz - 1 and are done; the others ask for the remaining slices of their few
// candidates in one stage (below).
static constexpr int SELECT_VPT = 8;
static constexpr int READY_LANES = 16, READY_SLOTS = 64 / READY_LANES;   // lanes per candidate, candidates per trip
// winners of a wave handled together, window rows a lane each: 128 rows a trip (9^3 has 81).  (4 x 2 takes 78 /
// 88 VGPRs -- the 1 340 workgroups of 140^3 are resident at once up to 80 -- and spills 80-110 SGPRs; 2 x 2: 57 / 65)
static constexpr int SELECT_WINNERS = 2, SELECT_ROWS = 2;
static inline dim3 select_grid(const Geo &G) { return dim3((unsigned)((G.V + 256 * SELECT_VPT - 1) / (256 * SELECT_VPT))); }
// a[j] for a wave-uniform j, by masks: written as a chain of selects the compiler sees an indexed array and
// moves it to LDS
template <typename T>
__device__ __forceinline__ T pick_voxel(const T (&a)[SELECT_VPT], const int j) {
    T r = 0;
#pragma unroll
    for (int i = 0; i < SELECT_VPT; ++i) r |= a[i] & -(T)(j == i);
    return r;
}
// lane src's value of v, wave-uniform
__device__ __forceinline__ int32_t lane_value(const int32_t v, const int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ long long lane_value(const long long v, const int src) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)v >> 32), src);
    return (long long)(((unsigned long long)hi << 32) | lo);
}
template <typename T>
__device__ __forceinline__ unsigned ready_voxels(const T *own, const T *__restrict__ xy,
                                                 const long long first, T (&mine)[SELECT_VPT], const Geo &G) {
    const T NONE = FilterNone<T>::value;
    T here[SELECT_VPT];
#pragma unroll
    for (int j = 0; j < SELECT_VPT; ++j) {
        const long long v = min(first + j * 256, G.V - 1);        // (clamped: no branch between the loads)
        mine[j] = own[v];
        here[j] = xy[v];
    }
    unsigned cand = 0;
#pragma unroll
    for (int j = 0; j < SELECT_VPT; ++j)
        if (first + j * 256 < G.V && mine[j] != NONE && !(here[j] < mine[j])) cand |= 1u << j;
    if (__ballot(cand != 0u) == 0ull || G.pz == 1) return cand;
    // The other slices.  The survivors of the own-slice test are few, so the wave deals them out, READY_SLOTS
    // at a time, to groups of READY_LANES lanes: lane i of a group asks for slice -1, +1, -2, +2, ... number i of
    // its candidate (a slice outside the volume, or a group without a candidate, reads a voxel of its own
    // again: a select between addresses, not a branch around the load), the group takes the minimum by
    // shuffles and the candidate's lane learns the outcome from a ballot.  One load stage for all slices of
    // up to four candidates (pz <= 9), where the pass-by-pass loop this replaces paid up to 2 (pz - 1) = 12
    // round trips in series, each behind a wave-wide ballot.
    const long long plane = (long long)G.X * G.Y;
    const int lane = threadIdx.x & 63, slot = lane / READY_LANES, sub = lane % READY_LANES;
    const long long wave_first = first - lane;
    unsigned todo = cand;
    for (;;) {
        int srcs[READY_SLOTS] = {}, js[READY_SLOTS] = {}, n_slots = 0;   // (wave-uniform)
        int my_src = -1, my_j = 0;                                // the group's candidate
        T my_val = NONE;
#pragma unroll
        for (int s = 0; s < READY_SLOTS; ++s) {
            const unsigned long long m = __ballot(todo != 0u);
            if (m != 0ull) {
                const int src = __builtin_ctzll(m);
                const int j = __builtin_ctz((unsigned)__builtin_amdgcn_readlane((int)todo, src));
                if (lane == src) todo &= todo - 1u;
                const T val = lane_value(pick_voxel(mine, j), src);
                if (slot == s) { my_src = src; my_j = j; my_val = val; }
                srcs[s] = src; js[s] = j; n_slots = s + 1;
            }
        }
        if (n_slots == 0) break;
        const long long vc = my_src >= 0 ? wave_first + my_src + my_j * 256 : min(first, G.V - 1);
        const int z = G.V < (1ll << 31) ? (int)vc / (int)plane : (int)(vc / plane);   // (32-bit division where it can be)
        T m = NONE;
        for (int i = sub; i < 2 * (G.pz - 1); i += READY_LANES) {
            const int d = (i & 1) ? (i >> 1) + 1 : -((i >> 1) + 1);
            const bool ask = my_src >= 0 && z + d >= 0 && z + d < G.Z;
            const T there = xy[ask ? vc + (long long)d * plane : vc];
            if (ask) m = min(m, there);
        }
        for (int o = READY_LANES >> 1; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
        const unsigned long long beaten = __ballot(sub == 0 && my_src >= 0 && m < my_val);
#pragma unroll
        for (int s = 0; s < READY_SLOTS; ++s)
            if (s < n_slots && ((beaten >> (s * READY_LANES)) & 1ull) && lane == srcs[s]) cand &= ~(1u << js[s]);
    }
    return cand;
}

// ---- `mark_close_neighboorhood` (foreground_cover.py:141-143, 162-168) ------------------------------
// The mark volume has the layout of the running mask bits ([Z*Y][row_words]).  A ranked patch whose centre
// is marked is skipped; a selected patch sets marked[cz, cy-3:cy+4, cx-3:cx+4] with NumPy's slice rules:
// the high end clips, a NEGATIVE start (cy < 3 or cx < 3) on an axis of at least 7 voxels gives an empty
// slice -- that patch marks nothing at all.  (On a shorter axis the slice wraps to the far end: such
// volumes keep the host loop, the entry points refuse them.)
// The fate of patch i then also depends on the selected patches of higher rank whose centre lies within
// (0, +-3, +-3) of i, so the ready test's y/x radius becomes max(p - 1, 3) (the z radius stays p_z - 1:
// marks never leave the centre's slice) -- a lower ranked patch within that radius of an undecided one is
// never ready, so no mark reaches a centre before its turn that the sequential loop would not have set.
// The 7 x 7 box is wider than the dirty box of a 3^3 selection and witnesses suppress recounts at
// pix_th == 0, so the mark test is a sweep of its own over every undecided patch, before every count.
static constexpr int MARK_R = 3;
__host__ __device__ __forceinline__ int mark_radius(int p) { return p - 1 > MARK_R ? p - 1 : MARK_R; }

// row `dy` (0..6) of the mark box of a patch selected at (cz, cy, cx).  Ready patches of one round can touch
// the same word: atomic OR.
__device__ __forceinline__ void mark_box_row(uint32_t *__restrict__ mark_bits, int cz, int cy, int cx, int dy,
                                             const Geo &G) {
    if (cy < MARK_R || cx < MARK_R) return;                   // negative slice start: empty slice
    const int y = cy - MARK_R + dy;
    if (y >= G.Y) return;                                     // the high end clips
    const int x0 = cx - MARK_R, nb = min(cx + MARK_R + 1, G.X) - x0, sh = x0 & 31;
    const uint32_t m = (1u << nb) - 1u;                       // nb in 1..7
    uint32_t *row = mark_bits + ((long long)cz * G.Y + y) * row_words(G) + (x0 >> 5);
    atomicOr(row, m << sh);
    if (sh && (m >> (32 - sh))) atomicOr(row + 1, m >> (32 - sh));   // (the row's spare word keeps this in bounds)
}

// the mark test: every undecided patch whose centre is marked is decided "not selected"
static constexpr int MARKTEST_VPT = 4;
__global__ void __launch_bounds__(256)
    cover_marktest_kernel(const uint32_t *__restrict__ mark_bits, int32_t *__restrict__ state,
                          int32_t *__restrict__ rank_vol, const Geo G) {
    const long long v0 = blockIdx.x * (long long)(256 * MARKTEST_VPT) + threadIdx.x;
    int kk[MARKTEST_VPT];
#pragma unroll
    for (int j = 0; j < MARKTEST_VPT; ++j) {
        const long long v = v0 + j * 256;
        kk[j] = v < G.V ? rank_vol[v] : RANK_NONE;
    }
#pragma unroll
    for (int j = 0; j < MARKTEST_VPT; ++j) {
        if (kk[j] == RANK_NONE) continue;
        const long long v = v0 + j * 256;
        const int x = (int)(v % G.X);
        if ((mark_bits[(v / G.X) * row_words(G) + (x >> 5)] >> (x & 31)) & 1u) {
            state[kk[j]] = 2;
            rank_vol[v] = RANK_NONE;
        }
    }
}

// the marks of a list of centres (sel == nullptr: all of them, else those with sel[k] != 0): thread per
// (centre, box row)
__global__ void __launch_bounds__(256)
    cover_marks_from_list_kernel(const long long *__restrict__ lin, const uint8_t *__restrict__ sel, long long n,
                                 uint32_t *__restrict__ mark_bits, const Geo G) {
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (t >= n * 7) return;
    const long long k = t / 7;
    if (sel && !sel[k]) return;
    int cz, cy, cx;
    centre_of(G, lin[k], cz, cy, cx);
    mark_box_row(mark_bits, cz, cy, cx, (int)(t % 7), G);
}

// The select sweep of a round, SELECT_VPT voxels per thread: the undecided patch with the best key of its
// neighbourhood selects itself; its wave clears the voxels (lane per window row) and marks the centres whose
// counts may have changed.  Selected patches never share a voxel, but they may share a mask word.
// The buffer starts at slice oz of a volume of gZ slices (the interior that `cleared` counts is the volume's).
// (MARKS: `mark_close_neighboorhood` -- a selected patch also sets the (0, +-3, +-3) box around its centre
// in the mark bits, see mark_box_row)
// P says what the algorithm makes of a key: K, index(key) = the winner's row of the tables where loc_vol does
// not give it, bits_row, marks_dirty and what the winner records.
template <bool MARKS, typename P>
__device__ __forceinline__ void
    select_body(uint32_t *__restrict__ mbits, const uint32_t *__restrict__ bits,
                const typename P::K *__restrict__ nbr_min, typename P::K *__restrict__ key_vol,
                uint8_t *__restrict__ dirty, const int32_t *__restrict__ loc_vol, const int oz, const int gZ,
                uint32_t *__restrict__ mark_bits, const P pick, const Geo &G) {
    using K = typename P::K;
    const long long first = blockIdx.x * (long long)(256 * SELECT_VPT) + threadIdx.x;
    const int lane = threadIdx.x & 63;
    K mine[SELECT_VPT];
    unsigned ready_bits = ready_voxels<K>(key_vol, nbr_min, first, mine, G);   // nbr_min: xy-filtered keys
    if (__ballot(ready_bits != 0u) == 0ull) return;
    if (loc_vol) {                                              // own centres only
#pragma unroll
        for (int j = 0; j < SELECT_VPT; ++j)
            if (((ready_bits >> j) & 1u) && loc_vol[first + j * 256] < 0) ready_bits &= ~(1u << j);
    }
    // The wave's winners, over all of its voxels, SELECT_WINNERS at a time: the key comes from the registers
    // of the lane that holds it, and the mask rows and bit rows of ALL of them (lane per window row,
    // SELECT_ROWS rows a lane) are asked for before the first atomic -- ready patches never share a voxel,
    // so the bits a winner clears are the same whether its rows are read before or after another winner's
    // atomics.  The cleared counts, the dirty boxes and the mark rows stay per winner.  (One winner after
    // another, each the chain key -> bit rows and mask rows -> atomics, was a chain per winner.)
    const int words = (G.C + 31) / 32, XW = row_words(G), R = G.pz * G.py;
    const long long wave_first = blockIdx.x * (long long)(256 * SELECT_VPT) +
                                 __builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u));
    unsigned todo = ready_bits;
    for (;;) {
        long long ccs[SELECT_WINNERS] = {};                             // (wave-uniform, all of these)
        K keys[SELECT_WINNERS] = {};
        int srcs[SELECT_WINNERS] = {}, kks[SELECT_WINNERS] = {}, n_win = 0;
#pragma unroll
        for (int s = 0; s < SELECT_WINNERS; ++s) {
            const unsigned long long m = __ballot(todo != 0u);
            if (m != 0ull) {
                const int src = __builtin_ctzll(m);
                const int j = __builtin_ctz((unsigned)__builtin_amdgcn_readlane((int)todo, src));
                if (lane == src) todo &= todo - 1u;
                keys[s] = lane_value(pick_voxel(mine, j), src);
                ccs[s] = wave_first + src + j * 256;
                srcs[s] = src;
                n_win = s + 1;
            }
        }
        if (n_win == 0) break;
        int cleared[SELECT_WINNERS] = {}, czs[SELECT_WINNERS] = {}, cys[SELECT_WINNERS] = {}, cxs[SELECT_WINNERS] = {};
#pragma unroll
        for (int s = 0; s < SELECT_WINNERS; ++s)
            if (s < n_win) {
                kks[s] = loc_vol ? loc_vol[ccs[s]] : P::index(keys[s]);                 // local index
                centre_of(G, ccs[s], czs[s], cys[s], cxs[s]);
            }
        for (int rb = 0; rb < R; rb += 64 * SELECT_ROWS) {
            uint32_t ml[SELECT_WINNERS][SELECT_ROWS], mh[SELECT_WINNERS][SELECT_ROWS];
            uint32_t bl[SELECT_WINNERS][SELECT_ROWS], bh[SELECT_WINNERS][SELECT_ROWS];
            // the lane's rows (the same for every winner; a row past the window reads the last one: clamped, no
            // branch between the loads)
            int dzs[SELECT_ROWS], dys[SELECT_ROWS];
#pragma unroll
            for (int i = 0; i < SELECT_ROWS; ++i) {
                const int r = min(rb + i * 64 + lane, R - 1);
                dzs[i] = r / G.py;
                dys[i] = r - dzs[i] * G.py;
            }
#pragma unroll
            for (int s = 0; s < SELECT_WINNERS; ++s) {
                if (s >= n_win) continue;
                const int cz = czs[s], cy = cys[s], cx = cxs[s];
                const uint32_t *b = bits + pick.bits_row(ccs[s], kks[s]) * words;
                const int wi = (cx - G.rx) >> 5;
#pragma unroll
                for (int i = 0; i < SELECT_ROWS; ++i) {
                    if (rb + i * 64 >= R) continue;
                    const int dz = dzs[i], dy = dys[i], bi = (min(rb + i * 64 + lane, R - 1) * G.px) >> 5;
                    const uint32_t *row = mbits + ((long long)(cz + dz - G.rz) * G.Y + (cy + dy - G.ry)) * XW;
                    ml[s][i] = row[wi];
                    mh[s][i] = row[min(wi + 1, XW - 1)];
                    bl[s][i] = b[bi];
                    bh[s][i] = b[min(bi + 1, words - 1)];
                }
            }
#pragma unroll
            for (int s = 0; s < SELECT_WINNERS; ++s) {
                if (s >= n_win) continue;
                const int cz = czs[s], cy = cys[s], cx = cxs[s];
                const int start = cx - G.rx, sh = start & 31;
                // window bits whose voxel is an interior x position: bits [lo, hi)
                const int lo = max(G.rx - start, 0), hi = min(G.X - G.rx - start, G.px);
                const uint32_t xin = hi > lo ? (low_bits(hi) & ~low_bits(lo)) : 0u;
#pragma unroll
                for (int i = 0; i < SELECT_ROWS; ++i) {
                    const int r = rb + i * 64 + lane;
                    if (r >= R) continue;
                    const int z = cz + dzs[i] - G.rz, y = cy + dys[i] - G.ry;
                    uint32_t *row = mbits + ((long long)z * G.Y + y) * XW;
                    const uint32_t cl = window_of(ml[s][i], mh[s][i], sh, G.px) &
                                        window_of(bl[s][i], bh[s][i], (r * G.px) & 31, G.px);
                    if (cl) {
                        atomicAnd(row + (start >> 5), ~(cl << sh));
                        if (sh && (cl >> (32 - sh))) atomicAnd(row + (start >> 5) + 1, ~(cl >> (32 - sh)));
                        if (z + oz >= G.rz && z + oz < gZ - G.rz && y >= G.ry && y < G.Y - G.ry)
                            cleared[s] += __popc(cl & xin);
                    }
                }
            }
        }
        auto finish = [&](const int s) {
            const int cz = czs[s], cy = cys[s], cx = cxs[s];
            int n_cleared = cleared[s];
            for (int o = 32; o > 0; o >>= 1) n_cleared += __shfl_xor(n_cleared, o);
            // every centre within p-1 of this one has a window that overlaps the cleared voxels
            const int z0 = max(cz - (G.pz - 1), 0), z1 = min(cz + G.pz - 1, G.Z - 1);
            const int y0 = max(cy - (G.py - 1), 0), y1 = min(cy + G.py - 1, G.Y - 1);
            const int x0 = max(cx - (G.px - 1), 0), x1 = min(cx + G.px - 1, G.X - 1);
            const int ny = y1 - y0 + 1, nx = x1 - x0 + 1;
            const int rows = pick.marks_dirty() ? (z1 - z0 + 1) * ny : 0;
            for (int row = lane; row < rows; row += 64) {
                uint8_t *d = dirty + vox(G, z0 + row / ny, y0 + row % ny, x0);
                for (int x = 0; x < nx; ++x) d[x] = 1;
            }
            if (MARKS && lane < 7) mark_box_row(mark_bits, cz, cy, cx, lane, G);
            if (lane == srcs[s]) {
                key_vol[ccs[s]] = FilterNone<K>::value;
                pick.record(kks[s], keys[s], n_cleared);
            }
        };
#pragma unroll
        for (int s = 0; s < SELECT_WINNERS; ++s)
            if (s < n_win) finish(s);
    }
}

// the greedy cover's: the key is the rank, which is the row of state / cleared / bits on one device
struct CoverPick {
    using K = int32_t;
    int32_t *__restrict__ state, *__restrict__ cleared;
    long long bits_vox;                  // >= 0: the bit table has a row per VOXEL, its first row belongs to this voxel
    int mark_dirty;                      // 0 at pix_th == 0: the count step asks every undecided patch's witness instead
    __device__ static int index(K key) { return key; }
    __device__ long long bits_row(long long cc, int kk) const { return bits_vox >= 0 ? cc - bits_vox : (long long)kk; }
    __device__ bool marks_dirty() const { return mark_dirty != 0; }
    __device__ void record(int kk, K, int n_cleared) const { state[kk] = 1; cleared[kk] = n_cleared; }
};
__global__ void __launch_bounds__(256)
    cover_select_kernel(uint32_t *__restrict__ mbits, const uint32_t *__restrict__ bits,
                        const int32_t *__restrict__ nbr_min, int32_t *__restrict__ state,
                        int32_t *__restrict__ rank_vol, int32_t *__restrict__ cleared_interior,
                        uint8_t *__restrict__ dirty, const int32_t *__restrict__ loc_vol, const int oz,
                        const int gZ, const long long bits_vox, const int mark_dirty, const Geo G) {
    select_body<false>(mbits, bits, nbr_min, rank_vol, dirty, loc_vol, oz, gZ, nullptr,
                       CoverPick{state, cleared_interior, bits_vox, mark_dirty}, G);
}
__global__ void __launch_bounds__(256)
    cover_select_marked_kernel(uint32_t *__restrict__ mbits, const uint32_t *__restrict__ bits,
                               const int32_t *__restrict__ nbr_min, int32_t *__restrict__ state,
                               int32_t *__restrict__ rank_vol, int32_t *__restrict__ cleared_interior,
                               uint8_t *__restrict__ dirty, const int oz, const int gZ, const long long bits_vox,
                               const int mark_dirty, uint32_t *__restrict__ mark_bits, const Geo G) {
    select_body<true>(mbits, bits, nbr_min, rank_vol, dirty, nullptr, oz, gZ, mark_bits,
                      CoverPick{state, cleared_interior, bits_vox, mark_dirty}, G);
}

template <typename K> static void round_layout(Carver &c, const Geo &G, RoundArrays<K> &W) {
    W.key_vol = c.take<K>(G.V);
    W.nbr_min = c.take<K>(G.V);
    W.tmp = c.take<K>(G.V);
    W.dirty = c.take<uint8_t>(G.V);
    W.mbits = c.take<uint32_t>((size_t)G.Z * G.Y * row_words(G));
    W.counters = (int32_t *)c.take_bytes(256);
}
template <typename K> static RoundArrays<K> carve_round(void *work, const Geo &G) {
    Carver c(work);
    RoundArrays<K> W;
    round_layout(c, G, W);
    return W;
}

// What every start of a cover or a thinning does to the arrays of a round: no patch anywhere, every centre marked
// (count everything once), the mask as bits.
template <typename K>
static hipError_t round_reset(const RoundArrays<K> &W, const uint8_t *mask, const Geo &G, hipStream_t s) {
    hipError_t e;
    if ((e = hipMemsetD32Async((hipDeviceptr_t)W.key_vol, (int)(FilterNone<K>::value & 0xFFFFFFFF),
                               (size_t)G.V * (sizeof(K) / 4), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.dirty, 1, (size_t)G.V, s)) != hipSuccess) return e;
    const long long n_words = (long long)G.Z * G.Y * row_words(G);
    cover_pack_kernel<<<dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, s>>>(mask, W.mbits, G);
    return hipSuccess;
}

// Rounds in batches of COVER_BATCH with one host synchronisation each, until the counter of a batch's last
// round reads zero: no patch was undecided at its start, so that round was a no-op and nothing is left.
// round(counter) launches one round, whose count step raises *counter; *rounds = the rounds run so far (what
// after_batch, called after every batch's synchronisation, may report).
template <typename Round, typename AfterBatch>
static hipError_t run_rounds(int32_t *counters, hipStream_t s, int *rounds, Round round, AfterBatch after_batch) {
    *rounds = 0;
    int32_t n_alive = 1;
    while (n_alive > 0) {
        hipError_t e;
        if ((e = hipMemsetAsync(counters, 0, COVER_BATCH * 4, s)) != hipSuccess) return e;
        for (int r = 0; r < COVER_BATCH; ++r) round(counters + r);
        *rounds += COVER_BATCH;
        if ((e = hipMemcpyAsync(&n_alive, counters + COVER_BATCH - 1, 4, hipMemcpyDeviceToHost, s)) != hipSuccess)
            return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        if ((e = hipGetLastError()) != hipSuccess) return e;
        after_batch();
    }
    return hipSuccess;
}

// (the same layout serves run_cover_pass and the sharded steps; n does not enter it)
static CoverWork cover_layout(Carver &c, const Geo &G) {
    CoverWork W;
    round_layout(c, G, W);
    W.loc_vol = c.take<int32_t>(G.V);
    W.witness = c.take<uint16_t>(G.V);
    return W;
}
size_t cover_workspace_bytes(long long, const Geo &G) { Carver c(nullptr); cover_layout(c, G); return c.used; }
static CoverWork carve(void *work, const Geo &G) { Carver c(work); return cover_layout(c, G); }

// One pass of the cover loop without the stop rule.  Returns the number of rounds in *rounds.
hipError_t run_cover_pass(uint8_t *mask, const uint32_t *bits, long long bits_vox, const long long *lin,
                          long long n, int pix_th, int32_t *state, int32_t *cleared, void *work,
                          const Geo &G, hipStream_t s, int *rounds, uint32_t *mark_bits) {
    *rounds = 0;
    if (n <= 0) return hipSuccess;
    PPP_GRID_CHECK((G.V + 255) / 256, 256);
    if (mark_bits && (G.Y < 2 * MARK_R + 1 || G.X < 2 * MARK_R + 1)) return hipErrorNotSupported;
    CoverWork W = carve(work, G);
    hipError_t e;
    if ((e = round_reset(W, mask, G, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.witness, 0xFF, (size_t)G.V * 2, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(cleared, 0, (size_t)n * 4, s)) != hipSuccess) return e;
    const dim3 vgrid((unsigned)((G.V + 255) / 256)), block(256);
    cover_init_kernel<<<dim3((unsigned)((n + 255) / 256)), block, 0, s>>>(lin, state, (int)n, W.key_vol);
    const int mark_dirty = (pix_th != 0 || !witness_ok(G)) ? 1 : 0;
    e = run_rounds(W.counters, s, rounds, [&](int32_t *counter) {
        if (mark_bits)
            cover_marktest_kernel<<<dim3((unsigned)((G.V + 256 * MARKTEST_VPT - 1) / (256 * MARKTEST_VPT))), block, 0, s>>>(
                mark_bits, state, W.key_vol, G);
        cover_count_kernel<<<count_grid(G), dim3(COUNT_THREADS), 0, s>>>(
            W.mbits, bits, W.dirty, pix_th, state, W.key_vol, counter, nullptr, witness_ok(G) ? W.witness : nullptr, bits_vox, G);
        // x, y, z; radius p-1: two windows overlap iff |dc| <= p-1 on every axis
        if (!mark_bits) {
            minfilter_xy<int32_t>(W.key_vol, W.tmp, W.nbr_min, G, s);
            cover_select_kernel<<<select_grid(G), block, 0, s>>>(W.mbits, bits, W.nbr_min, state, W.key_vol, cleared,
                                                        W.dirty, nullptr, G.oz, G.Z + G.oz, bits_vox, mark_dirty, G);
        } else {
            // (with marks: y / x radius max(p - 1, 3), see mark_box_row)
            minfilter_xy<int32_t>(W.key_vol, W.tmp, W.nbr_min, G, mark_radius(G.px), mark_radius(G.py), s);
            cover_select_marked_kernel<<<select_grid(G), block, 0, s>>>(W.mbits, bits, W.nbr_min, state, W.key_vol, cleared,
                                                               W.dirty, G.oz, G.Z + G.oz, bits_vox, mark_dirty, mark_bits, G);
        }
    }, [&] {
        static EnvSwitch trace("PPP_COVER_TRACE");
        if (trace.get()) {   // development aid: undecided / selected patches per batch
            std::vector<int32_t> h((size_t)n);
            (void)hipMemcpy(h.data(), state, (size_t)n * 4, hipMemcpyDeviceToHost);
            long long a = 0, sel = 0;
            for (long long i = 0; i < n; ++i) { a += h[i] == 0; sel += h[i] == 1; }
            fprintf(stderr, "cover rounds %d: undecided %lld selected %lld\n", *rounds, a, sel);
        }
    });
    if (e != hipSuccess) return e;
    cover_unpack_kernel<<<vgrid, block, 0, s>>>(W.mbits, mask, G);
    return hipGetLastError();
}

// bytes of a mark volume
size_t cover_mark_bits_bytes(const Geo &G) { return (size_t)G.Z * G.Y * row_words(G) * sizeof(uint32_t); }

// The mark volume of a set of selected centres, rebuilt from nothing: what the marks are after the stop
// rule has cut a pass's selections (marks may only come from patches that survive the cut), and what a
// second pass or the ring cover starts from.
hipError_t run_cover_marks_from_selected(const long long *lin, const uint8_t *sel, long long n, uint32_t *mark_bits,
                                         const Geo &G, hipStream_t s) {
    if (G.Y < 2 * MARK_R + 1 || G.X < 2 * MARK_R + 1) return hipErrorNotSupported;
    hipError_t e;
    if ((e = hipMemsetAsync(mark_bits, 0, cover_mark_bits_bytes(G), s)) != hipSuccess) return e;
    if (n <= 0) return hipSuccess;
    PPP_GRID_CHECK((n * 7 + 255) / 256, 256);
    cover_marks_from_list_kernel<<<dim3((unsigned)((n * 7 + 255) / 256)), dim3(256), 0, s>>>(lin, sel, n, mark_bits, G);
    return hipGetLastError();
}

// ---- `select_patches_overlap_neighborhood` (foreground_cover.py:53-85): binary dilation ----------------
// One round of 6-neighbour dilation on bit rows (scipy.ndimage.binary_dilation's default cross, border
// value 0): a word ORs itself shifted by one bit either way (with the carry of the neighbouring words),
// the same word of the rows y - 1 and y + 1 and -- use_z -- of the slices z - 1 and z + 1.  Bits past the
// end of a row stay clear.
__global__ void __launch_bounds__(256)
    mask_dilate_bits_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, const int use_z, const Geo G) {
    const int XW = row_words(G);
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (t >= (long long)G.Z * G.Y * XW) return;
    const int w = (int)(t % XW);
    const long long row = t / XW;
    const int y = (int)(row % G.Y), z = (int)(row / G.Y);
    const uint32_t c = in[t], l = w > 0 ? in[t - 1] : 0u, r = w + 1 < XW ? in[t + 1] : 0u;
    uint32_t v = c | (c << 1) | (l >> 31) | (c >> 1) | (r << 31);
    if (y > 0) v |= in[t - XW];
    if (y + 1 < G.Y) v |= in[t + XW];
    if (use_z) {
        const long long plane = (long long)G.Y * XW;
        if (z > 0) v |= in[t - plane];
        if (z + 1 < G.Z) v |= in[t + plane];
    }
    const int left = G.X - w * 32;                            // voxels of the row from this word on
    out[t] = left >= 32 ? v : left <= 0 ? 0u : (v & ((1u << left) - 1u));
}
__global__ void __launch_bounds__(256)
    mask_bits_to_bytes_kernel(const uint32_t *__restrict__ mbits, uint8_t *__restrict__ mask, const Geo G) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (v >= G.V) return;
    const int x = (int)(v % G.X);
    mask[v] = (uint8_t)((mbits[(v / G.X) * row_words(G) + (x >> 5)] >> (x & 31)) & 1u);
}

struct DilateWork { uint32_t *a, *b; };
static DilateWork dilate_layout(Carver &c, const Geo &G) {
    DilateWork W;
    W.a = c.take<uint32_t>((size_t)G.Z * G.Y * row_words(G));
    W.b = c.take<uint32_t>((size_t)G.Z * G.Y * row_words(G));
    return W;
}
size_t mask_dilate_workspace_bytes(const Geo &G) { Carver c(nullptr); dilate_layout(c, G); return c.used; }

// out = `iterations` rounds of dilation of (in != 0), one byte per voxel (0 / 1); in == out is allowed
hipError_t run_mask_dilate(const uint8_t *in, uint8_t *out, int iterations, int use_z, void *work, const Geo &G,
                           hipStream_t s) {
    const long long n_words = (long long)G.Z * G.Y * row_words(G);
    PPP_GRID_CHECK((G.V + 255) / 256, 256);
    Carver c(work);
    DilateWork W = dilate_layout(c, G);
    const dim3 wgrid((unsigned)((n_words + 255) / 256)), vgrid((unsigned)((G.V + 255) / 256)), block(256);
    cover_pack_kernel<<<wgrid, block, 0, s>>>(in, W.a, G);
    for (int i = 0; i < iterations; ++i) {
        mask_dilate_bits_kernel<<<wgrid, block, 0, s>>>(W.a, W.b, use_z, G);
        std::swap(W.a, W.b);
    }
    mask_bits_to_bytes_kernel<<<vgrid, block, 0, s>>>(W.a, out, G);
    return hipGetLastError();
}

// ---- S4: set-cover thinning of the selected patches, on the device --------------------------
//
// Reference: foreground_cover.py:183-256 (thinOutForegroundCover, sample == 1.0).  Its loop picks,
// while the interior of the running mask is not empty, the FIRST patch with the largest number
// of still uncovered voxels (np.argmax over len(set_i), sets = window & (pred > fc_threshold) &
// running mask), keeps it and clears its voxels.  That is a greedy cover with the DYNAMIC
// priority key_i = (count_i descending, index_i ascending).
//
// Priority-parallel form (exact).  Counts only shrink, so the best key of the sequential loop
// never improves over time.  A patch whose key beats the key of every undecided patch within
// p-1 of it (the only patches whose windows intersect its own) can not be overtaken: none of
// them can become the global best while it is undecided with an unchanged count, and its count
// only changes when one of them is kept.  So it is kept by the sequential loop with exactly its
// current count, and all such local winners of a round may be kept at once (they never overlap:
// keys are distinct).  The sequential ORDER of the kept patches is the order of their keys at
// the time they were kept (strictly worsening along the loop), so the loop's stop rule ("interior
// empty", tested before every pick) is applied afterwards: sort the kept patches by (count
// descending, index ascending), cut after the one at which the cumulative number of cleared
// interior voxels reaches the initial interior count.  A patch with count 0 is never a winner;
// when every count is 0 but the interior is not empty the reference's argmax returns patch 0 and
// its empty index tuple zeroes the whole mask (:210-216), which ends the loop: keep[0] = 1.
//
// Kernels: same volume sweeps as the cover above; the rank volume becomes a 64-bit key volume
//   key = (THIN_MAXC - count) << 32 | index       (smaller is better; NONE = 0x7F7F..)
// and the ready test is "my key is the minimum of my (p-1)-neighbourhood".
static constexpr long long THIN_NONE = FilterNone<long long>::value;
static constexpr long long THIN_MAXC = 1ll << 20;

struct ThinWork : RoundArrays<long long> {
    unsigned long long *interior;        // [1] set interior voxels of the mask
    int32_t *state, *sel_count, *cleared;  // [n] each
};
static ThinWork thin_layout(Carver &c, long long n, const Geo &G) {
    ThinWork W;
    round_layout(c, G, W);
    W.interior = (unsigned long long *)c.take_bytes(256);
    const size_t per = (size_t)(n > 0 ? n : 1);
    W.state = c.take<int32_t>(per);
    W.sel_count = c.take<int32_t>(per);
    W.cleared = c.take<int32_t>(per);
    return W;
}
size_t thin_workspace_bytes(long long n, const Geo &G) { Carver c(nullptr); thin_layout(c, n, G); return c.used; }
static ThinWork carve_thin(void *work, long long n, const Geo &G) { Carver c(work); return thin_layout(c, n, G); }

__global__ void __launch_bounds__(256)
    thin_init_kernel(const long long *__restrict__ lin, int n, long long *__restrict__ key_vol) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    // (count not known yet.)  A centre listed twice -- possible in a list from outside, never in
    // one made by the greedy cover -- keeps its FIRST index, like the reference's np.argmax: the
    // later copy has the same voxel set, which is empty once the first is kept.
    if (k < n) atomicMin(&key_vol[lin[k]], (THIN_MAXC << 32) | (long long)k);
}
// ... and the later copies are retired at once
__global__ void __launch_bounds__(256)
    thin_dups_kernel(const long long *__restrict__ lin, int n, const long long *__restrict__ key_vol,
                     int32_t *__restrict__ state) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n && (int)(key_vol[lin[k]] & 0xFFFFFFFFll) != k) state[k] = 2;
}

// set voxels of the bit mask that are interior voxels of the volume (thread per mask word)
__global__ void __launch_bounds__(256)
    thin_interior_kernel(const uint32_t *__restrict__ mbits, unsigned long long *__restrict__ total,
                         const Geo G) {
    const int XW = row_words(G);
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    int c = 0;
    if (t < (long long)G.Z * G.Y * XW) {
        const int w = (int)(t % XW);
        const long long row = t / XW;
        const int y = (int)(row % G.Y), z = (int)(row / G.Y);
        if (z >= G.rz && z < G.Z - G.rz && y >= G.ry && y < G.Y - G.ry) {
            const int lo = max(G.rx - w * 32, 0), hi = min(G.X - G.rx - w * 32, 32);   // bits [lo, hi)
            if (lo < hi) {
                const uint32_t m = (hi >= 32 ? 0xFFFFFFFFu : ((1u << hi) - 1u)) & ~((1u << lo) - 1u);
                c = __popc(mbits[t] & m);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    __shared__ int part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int sum = part[0] + part[1] + part[2] + part[3];
        if (sum) atomicAdd(total, (unsigned long long)sum);
    }
}

// The count sweep over keys (the loads of a thread's voxels issued pass by pass): the undecided patches of a
// workgroup whose neighbourhood changed are compacted in LDS, then recounted in full and their keys
// rewritten; a patch that covers nothing any more is retired.
__global__ void PPP_COUNT_BOUNDS
    thin_count_kernel(const uint32_t *__restrict__ mbits, const uint32_t *__restrict__ bits,
                      uint8_t *__restrict__ dirty, int32_t *__restrict__ state,
                      long long *__restrict__ key_vol, int32_t *__restrict__ n_alive,
                      const int32_t *__restrict__ loc_vol, const Geo G) {
    __shared__ uint16_t s_list[COUNT_THREADS * COUNT_VPT];
    __shared__ int32_t s_row[COUNT_THREADS * COUNT_VPT];
    __shared__ int s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const long long v0 = blockIdx.x * (long long)(COUNT_THREADS * COUNT_VPT);
    int n;
    {
        long long vv[COUNT_VPT], key[COUNT_VPT];
        uint8_t mark[COUNT_VPT];
        int kl[COUNT_VPT];                                       // row of `bits` / `state`
        bool alive[COUNT_VPT], marked[COUNT_VPT];
#pragma unroll
        for (int j = 0; j < COUNT_VPT; ++j) {
            vv[j] = v0 + j * COUNT_THREADS + threadIdx.x;
            const long long vc = min(vv[j], G.V - 1);            // (clamped: no branch between the loads)
            key[j] = key_vol[vc];
            mark[j] = dirty[vc];
        }
        // (sharded: loc_vol = local list index of an OWN centre, -1 elsewhere -- the keys a rank sees in
        // its halo slices belong to patches their owner counts)
#pragma unroll
        for (int j = 0; j < COUNT_VPT; ++j) {
            alive[j] = vv[j] < G.V && key[j] != THIN_NONE;
            kl[j] = (int)(key[j] & 0xFFFFFFFFll);
            if (loc_vol && alive[j]) { kl[j] = loc_vol[vv[j]]; alive[j] = kl[j] >= 0; }
            marked[j] = vv[j] < G.V && mark[j] != 0;
            if (marked[j]) dirty[vv[j]] = 0;
        }
        n = compact_marked(alive, marked, kl, s_list, s_row, &s_n, n_alive);
    }
    // the listed patches, a group of lanes each, as in cover_count_kernel: the full count, no witness
    const int gw = recount_group(G), per_wave = 64 / gw;
    const int sub = threadIdx.x & (gw - 1), in_wave = (threadIdx.x & 63) / gw;
    for (int base = (threadIdx.x >> 6) * per_wave; base < n; base += COUNT_THREADS / gw) {
        const bool mine = base + in_wave < n;
        const int e = mine ? base + in_wave : base;
        const long long v = v0 + s_list[e];
        const int kl = s_row[e];
        // position in the (global) list, the key's tie-break: asked for beside the rows, not before them
        const int k = (int)(key_vol[v] & 0xFFFFFFFFll);
        unsigned wit;
        const int hits = group_hits<false>(mbits, bits + (long long)kl * ((G.C + 31) / 32), v, sub, gw, wit, G);
        if (!mine || sub != 0) continue;
        if (hits == 0) {
            state[kl] = 2;
            key_vol[v] = THIN_NONE;
        } else {
            key_vol[v] = ((THIN_MAXC - (long long)hits) << 32) | (long long)k;
            *n_alive = 1;
        }
    }
}

// select_body for the thinning: the key's low word is the row where loc_vol does not give it, and the winner also
// records the count it was kept with (the key's high word): the stop rule sorts by it
struct ThinPick {
    using K = long long;
    int32_t *__restrict__ state, *__restrict__ sel_count, *__restrict__ cleared;
    __device__ static int index(K key) { return (int)(key & 0xFFFFFFFFll); }
    __device__ static long long bits_row(long long, int kk) { return kk; }
    __device__ static constexpr bool marks_dirty() { return true; }
    __device__ void record(int kk, K key, int n_cleared) const {
        state[kk] = 1;
        sel_count[kk] = (int32_t)(THIN_MAXC - (key >> 32));
        cleared[kk] = n_cleared;
    }
};
__global__ void __launch_bounds__(256)
    thin_select_kernel(uint32_t *__restrict__ mbits, const uint32_t *__restrict__ bits,
                       const long long *__restrict__ nbr_min, int32_t *__restrict__ state,
                       long long *__restrict__ key_vol, int32_t *__restrict__ sel_count,
                       int32_t *__restrict__ cleared_interior, uint8_t *__restrict__ dirty,
                       const int32_t *__restrict__ loc_vol, const int oz, const int gZ, const Geo G) {
    select_body<false>(mbits, bits, nbr_min, key_vol, dirty, loc_vol, oz, gZ, nullptr,
                       ThinPick{state, sel_count, cleared_interior}, G);
}

// keep u8 [n] (device).  Synchronises the stream.
hipError_t run_thin_cover(const uint8_t *mask, const uint32_t *bits, const long long *lin, long long n,
                          uint8_t *keep, void *work, const Geo &G, hipStream_t s, int *rounds,
                          const long long *slice_interior) {
    *rounds = 0;
    if (n <= 0) return hipSuccess;
    if (n >= (1ll << 31) || G.C >= THIN_MAXC) return hipErrorInvalidValue;
    PPP_GRID_CHECK((G.V + 255) / 256, 256);
    ThinWork W = carve_thin(work, n, G);
    hipError_t e;
    if ((e = round_reset(W, mask, G, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.state, 0, (size_t)n * 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.sel_count, 0, (size_t)n * 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.cleared, 0, (size_t)n * 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.interior, 0, 8, s)) != hipSuccess) return e;
    const dim3 block(256);
    const long long n_words = (long long)G.Z * G.Y * row_words(G);
    thin_interior_kernel<<<dim3((unsigned)((n_words + 255) / 256)), block, 0, s>>>(W.mbits, W.interior, G);
    thin_init_kernel<<<dim3((unsigned)((n + 255) / 256)), block, 0, s>>>(lin, (int)n, W.key_vol);
    thin_dups_kernel<<<dim3((unsigned)((n + 255) / 256)), block, 0, s>>>(lin, (int)n, W.key_vol, W.state);
    e = run_rounds(W.counters, s, rounds, [&](int32_t *counter) {
        thin_count_kernel<<<count_grid(G), dim3(COUNT_THREADS), 0, s>>>(
            W.mbits, bits, W.dirty, W.state, W.key_vol, counter, nullptr, G);
        minfilter_xy<long long>(W.key_vol, W.tmp, W.nbr_min, G, s);
        thin_select_kernel<<<select_grid(G), block, 0, s>>>(W.mbits, bits, W.nbr_min, W.state, W.key_vol,
                                                   W.sel_count, W.cleared, W.dirty, nullptr, 0, G.Z, G);
    }, [] {});
    if (e != hipSuccess) return e;
    // ---- the stop rule: kept patches in the order the sequential loop picks them
    std::vector<int32_t> st((size_t)n), cnt((size_t)n), clr((size_t)n);
    unsigned long long interior = 0;
    if ((e = hipMemcpyAsync(st.data(), W.state, (size_t)n * 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(cnt.data(), W.sel_count, (size_t)n * 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(clr.data(), W.cleared, (size_t)n * 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(&interior, W.interior, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    std::vector<long long> order;
    for (long long i = 0; i < n; ++i)
        if (st[(size_t)i] == 1) order.push_back(((THIN_MAXC - (long long)cnt[(size_t)i]) << 32) | i);
    std::sort(order.begin(), order.end());
    std::vector<uint8_t> k8((size_t)n, 0);
    if (!slice_interior) {
        long long remaining = (long long)interior;
        for (size_t j = 0; j < order.size() && remaining > 0; ++j) {
            const long long i = order[j] & 0xFFFFFFFFll;
            k8[(size_t)i] = 1;
            remaining -= clr[(size_t)i];
        }
        if (remaining > 0) k8[0] = 1;   // every count is 0 with voxels left: np.argmax picks patch 0
    } else {
        // a stack of independent 2-d images (pz = 1: no window reaches another slice, so the rounds
        // above are every image's own): the stop rule per slice, on the slice's subsequence of the
        // keys (the order its own loop keeps them in) and the slice's interior count; "patch 0" is
        // the first patch of the slice in list order
        std::vector<long long> hz((size_t)n);
        if ((e = hipMemcpyAsync(hz.data(), lin, (size_t)n * 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        const long long plane = (long long)G.Y * G.X;
        std::vector<long long> remaining(slice_interior, slice_interior + G.Z);
        std::vector<long long> first((size_t)G.Z, -1);
        for (long long i = n - 1; i >= 0; --i) first[(size_t)(hz[(size_t)i] / plane)] = i;
        for (size_t j = 0; j < order.size(); ++j) {
            const long long i = order[j] & 0xFFFFFFFFll;
            const size_t z = (size_t)(hz[(size_t)i] / plane);
            if (remaining[z] <= 0) continue;
            k8[(size_t)i] = 1;
            remaining[z] -= clr[(size_t)i];
        }
        for (int z = 0; z < G.Z; ++z)
            if (remaining[(size_t)z] > 0 && first[(size_t)z] >= 0) k8[(size_t)first[(size_t)z]] = 1;
    }
    if ((e = hipMemcpyAsync(keep, k8.data(), (size_t)n, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
    return hipStreamSynchronize(s);
}

// ---- the same rounds, one step at a time, on the z-range of one rank (sharded cover) -------
//
// Every rank keeps the round state (rank volume, bit mask, dirty marks) for its own slices
// plus a halo of p-1 slices and works on its OWN patch centres only.  What a round needs from
// the neighbours lives in the "zones" of 2(p-1) slices around every slab boundary; they are
// made consistent twice per round by the caller (all-reduces of small buffers):
//   after count  : rank volume -- every slice is owned by one rank, the others contribute
//                  INT_MAX, MIN combines;
//   after select : mask (a voxel stays set only if nobody cleared it: MIN of 0/1 bytes) and
//                  dirty marks (kept inverted so that MIN combines them as well).
// Ready patches of two ranks never overlap (each sees the other's rank in its halo), so the
// combined mask is exactly what one device would hold.
__global__ void __launch_bounds__(256)
    cover_init_local_kernel(const long long *__restrict__ lin, const int32_t *__restrict__ rankid,
                            const int32_t *__restrict__ state, int n, int32_t *__restrict__ rank_vol,
                            int32_t *__restrict__ loc_vol) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    loc_vol[lin[i]] = i;
    if (state[i] == 0) rank_vol[lin[i]] = rankid[i];
}

hipError_t cover_open(const uint8_t *mask, const long long *lin, const int32_t *rankid, long long n,
                      const int32_t *state, int32_t *cleared, void *work, const Geo &G, hipStream_t s) {
    PPP_GRID_CHECK((G.V + 255) / 256, 256);
    CoverWork W = carve(work, G);
    hipError_t e;
    if ((e = round_reset(W, mask, G, s)) != hipSuccess) return e;
    if ((e = hipMemsetD32Async((hipDeviceptr_t)W.loc_vol, 0xFFFFFFFF, (size_t)G.V, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.witness, 0xFF, (size_t)G.V * 2, s)) != hipSuccess) return e;
    if (n && (e = hipMemsetAsync(cleared, 0, (size_t)n * 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.counters, 0, COVER_BATCH * 4, s)) != hipSuccess) return e;
    if (n)
        cover_init_local_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(
            lin, rankid, state, (int)n, W.key_vol, W.loc_vol);
    return hipGetLastError();
}

hipError_t cover_step_count(const uint32_t *bits, int pix_th, int32_t *state, void *work,
                            const Geo &G, hipStream_t s) {
    CoverWork W = carve(work, G);
    hipError_t e;
    if ((e = hipMemsetAsync(W.counters, 0, 4, s)) != hipSuccess) return e;
    cover_count_kernel<<<count_grid(G), dim3(COUNT_THREADS), 0, s>>>(
        W.mbits, bits, W.dirty, pix_th, state, W.key_vol, W.counters, W.loc_vol, witness_ok(G) ? W.witness : nullptr, -1ll, G);
    return hipGetLastError();
}

hipError_t cover_step_select(const uint32_t *bits, int pix_th, int32_t *state, int32_t *cleared, void *work,
                             int gZ, const Geo &G, hipStream_t s) {
    CoverWork W = carve(work, G);
    cover_select_kernel<<<select_grid(G), dim3(256), 0, s>>>(
        W.mbits, bits, W.nbr_min, state, W.key_vol, cleared, W.dirty, W.loc_vol, G.oz, gZ, -1ll,
        (pix_th != 0 || !witness_ok(G)) ? 1 : 0, G);
    return hipGetLastError();
}

// ---- set-cover thinning, one round step at a time on the z-range of one rank (round 6) --------
//
// The same rounds as run_thin_cover with the volume split by z, after the pattern of the sharded greedy
// cover above: every rank keeps key volume, bit mask and dirty marks for its own slices + p-1 halo slices
// and decides its OWN patches; the caller makes the zones of 2(p-1) slices around every slab boundary
// consistent twice per round -- keys after the count step (every slice has one owner, the others
// contribute "none", MIN combines), mask and dirty marks after the select step.  A key's low word is the
// patch's position in the GLOBAL selected list (the sequential loop's tie-break, foreground_cover.py:210);
// loc_vol maps an own centre to its row in the rank's own lists.  The stop rule (foreground_cover.py:
// 206-216) needs every rank's kept patches: the caller gathers (key at selection, cleared interior voxels).
struct ThinShardWork : RoundArrays<long long> {
    int32_t *loc_vol;                    // [V]
};
static ThinShardWork thin_shard_layout(Carver &c, const Geo &G) {
    ThinShardWork W;
    round_layout(c, G, W);
    W.loc_vol = c.take<int32_t>(G.V);
    return W;
}
size_t thin_shard_workspace_bytes(const Geo &G) { Carver c(nullptr); thin_shard_layout(c, G); return c.used; }
static ThinShardWork carve_thin_shard(void *work, const Geo &G) { Carver c(work); return thin_shard_layout(c, G); }
__global__ void __launch_bounds__(256)
    thin_init_local_kernel(const long long *__restrict__ lin, const int32_t *__restrict__ gidx, int n,
                           long long *__restrict__ key_vol, int32_t *__restrict__ loc_vol) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    key_vol[lin[i]] = (THIN_MAXC << 32) | (long long)gidx[i];     // (count not known yet; centres are distinct)
    loc_vol[lin[i]] = i;
}
hipError_t thin_open(const uint8_t *mask, const long long *lin, const int32_t *gidx, long long n, int32_t *state,
                     int32_t *sel_count, int32_t *cleared, void *work, const Geo &G, hipStream_t s) {
    if (n >= (1ll << 31) || G.C >= THIN_MAXC) return hipErrorInvalidValue;
    PPP_GRID_CHECK((G.V + 255) / 256, 256);
    ThinShardWork W = carve_thin_shard(work, G);
    hipError_t e;
    if ((e = round_reset(W, mask, G, s)) != hipSuccess) return e;
    if ((e = hipMemsetD32Async((hipDeviceptr_t)W.loc_vol, 0xFFFFFFFF, (size_t)G.V, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.counters, 0, COVER_BATCH * 4, s)) != hipSuccess) return e;
    if (n) {
        if ((e = hipMemsetAsync(state, 0, (size_t)n * 4, s)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(sel_count, 0, (size_t)n * 4, s)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(cleared, 0, (size_t)n * 4, s)) != hipSuccess) return e;
    }
    if (n) thin_init_local_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(lin, gidx, (int)n, W.key_vol, W.loc_vol);
    return hipGetLastError();
}
hipError_t thin_step_count(const uint32_t *bits, int32_t *state, void *work, const Geo &G, hipStream_t s) {
    ThinShardWork W = carve_thin_shard(work, G);
    hipError_t e;
    if ((e = hipMemsetAsync(W.counters, 0, 4, s)) != hipSuccess) return e;
    thin_count_kernel<<<count_grid(G), dim3(COUNT_THREADS), 0, s>>>(
        W.mbits, bits, W.dirty, state, W.key_vol, W.counters, W.loc_vol, G);
    return hipGetLastError();
}
hipError_t thin_step_select(const uint32_t *bits, int32_t *state, int32_t *sel_count, int32_t *cleared, void *work,
                            int gZ, const Geo &G, hipStream_t s) {
    ThinShardWork W = carve_thin_shard(work, G);
    thin_select_kernel<<<select_grid(G), dim3(256), 0, s>>>(
        W.mbits, bits, W.nbr_min, state, W.key_vol, sel_count, cleared, W.dirty, W.loc_vol, G.oz, gZ, G);
    return hipGetLastError();
}

// ---- the steps that the sharded cover (K = int32_t) and the sharded thinning (K = long long) share: they
// touch the arrays of a round only, which both workspaces begin with -----------------------------------
template <typename K> hipError_t round_step_filter(void *work, const Geo &G, hipStream_t s) {
    RoundArrays<K> W = carve_round<K>(work, G);
    minfilter_xy<K>(W.key_vol, W.tmp, W.nbr_min, G, s);
    return hipGetLastError();
}
template <typename K> hipError_t round_alive(void *work, const Geo &G, int32_t *alive, hipStream_t s) {
    RoundArrays<K> W = carve_round<K>(work, G);
    hipError_t e;
    if ((e = hipMemcpyAsync(alive, W.counters, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    return hipStreamSynchronize(s);
}
template <typename K> hipError_t round_close(uint8_t *mask, void *work, const Geo &G, hipStream_t s) {
    RoundArrays<K> W = carve_round<K>(work, G);
    cover_unpack_kernel<<<dim3((unsigned)((G.V + 255) / 256)), dim3(256), 0, s>>>(W.mbits, mask, G);
    return hipGetLastError();
}

// zone = local slices [z_lo, z_hi); the rank owns the local slices [own_lo, own_hi).  In an exported zone
// "not my slice" is the largest K (what MIN leaves alone); in the volume "none" is FilterNone<K>::value.
template <typename K> static constexpr K ZONE_NONE = std::numeric_limits<K>::max();
template <typename K>
__global__ void __launch_bounds__(256)
    zone_export_kernel(const K *__restrict__ key_vol, const uint32_t *__restrict__ mbits,
                       const uint8_t *__restrict__ dirty, const int z_lo, const int z_hi, const int own_lo,
                       const int own_hi, K *__restrict__ out_key, uint8_t *__restrict__ out_mask,
                       uint8_t *__restrict__ out_clean, const Geo G) {
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long plane = (long long)G.Y * G.X;
    if (t >= (long long)(z_hi - z_lo) * plane) return;
    const int z = z_lo + (int)(t / plane);
    const long long v = (long long)z * plane + t % plane;
    const int x = (int)(v % G.X);
    const long long row = v / G.X;
    if (out_key) out_key[t] = (z >= own_lo && z < own_hi) ? key_vol[v] : ZONE_NONE<K>;
    if (out_mask) {
        out_mask[t] = (mbits[row * row_words(G) + (x >> 5)] >> (x & 31)) & 1u;
        out_clean[t] = dirty[v] ? 0 : 1;
    }
}
template <typename K>
__global__ void __launch_bounds__(256)
    zone_import_kernel(K *__restrict__ key_vol, uint32_t *__restrict__ mbits, uint8_t *__restrict__ dirty,
                       const int z_lo, const int z_hi, const K *__restrict__ in_key,
                       const uint8_t *__restrict__ in_mask, const uint8_t *__restrict__ in_clean, const Geo G) {
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long plane = (long long)G.Y * G.X;
    if (t >= (long long)(z_hi - z_lo) * plane) return;
    const int z = z_lo + (int)(t / plane);
    const long long v = (long long)z * plane + t % plane;
    const int x = (int)(v % G.X);
    const long long row = v / G.X;
    if (in_key) key_vol[v] = in_key[t] == ZONE_NONE<K> ? FilterNone<K>::value : in_key[t];
    if (in_mask) {
        if (!in_mask[t]) atomicAnd(&mbits[row * row_words(G) + (x >> 5)], ~(1u << (x & 31)));
        if (!in_clean[t]) dirty[v] = 1;
    }
}
// import: keys / mask / clean are read into the zone; else they are written from it
template <typename K>
hipError_t round_zone(bool import, void *work, int z_lo, int z_hi, int own_lo, int own_hi, K *keys, uint8_t *mask,
                      uint8_t *clean, const Geo &G, hipStream_t s) {
    RoundArrays<K> W = carve_round<K>(work, G);
    const long long n = (long long)(z_hi - z_lo) * G.Y * G.X;
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (import)
        zone_import_kernel<K><<<grid, block, 0, s>>>(W.key_vol, W.mbits, W.dirty, z_lo, z_hi, keys, mask, clean, G);
    else
        zone_export_kernel<K><<<grid, block, 0, s>>>(W.key_vol, W.mbits, W.dirty, z_lo, z_hi, own_lo, own_hi, keys, mask,
                                                     clean, G);
    return hipGetLastError();
}
#define PPP_ROUND_STEPS(K)                                                                                      \
    template hipError_t round_step_filter<K>(void *, const Geo &, hipStream_t);                                  \
    template hipError_t round_alive<K>(void *, const Geo &, int32_t *, hipStream_t);                             \
    template hipError_t round_close<K>(uint8_t *, void *, const Geo &, hipStream_t);                             \
    template hipError_t round_zone<K>(bool, void *, int, int, int, int, K *, uint8_t *, uint8_t *, const Geo &, hipStream_t);
PPP_ROUND_STEPS(int32_t)
PPP_ROUND_STEPS(long long)
#undef PPP_ROUND_STEPS

}  // namespace ppp
