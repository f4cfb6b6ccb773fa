// ppp_consensus_sparse.hip -- S1 on sparse foreground: which work items can vote at all.
//
// The packed kernel (ppp_consensus_v3.hip) runs its whole vote chain for every item = (x-run of 64
// base voxels x 2 slices, offset row (dz, dy)) and multiplies every result by
// ok = [u valid] && [w = u + d valid] when it writes.  On tubes (a few percent foreground) nine
// items in ten have no lane with ok: they store exact zeros after ~10^5 votes per voxel.  The
// reference's thread returns at once for a background voxel (fillConsensusArray.cu:25-32).
//
// An item is ACTIVE iff for some slice s in {0, 1} and some lane of the run
//     u exists (lane_ok; slice 1 only when the compute box has it),
//     u is valid: pred[mid][u] > TH and not overlapped,
//     for some dx in [-(PX-1), PX-1] (dx > 0 only in offset row 0): w = u + (dz, dy, dx) lies in
//     the volume and is valid
// -- the write stage's `ok`, taken over the wave.  Exact, so an inactive item stores only +0.0f.
//
//   1. valid_bits_kernel   validity packed to one bit per voxel (64 voxels of a line per word), for
//                          the slices the compute box and its offset rows reach
//   2. item_flags_kernel   thread per item: the run's u bits AND the w bits dilated over dx (shifts
//                          and ORs of a 128-bit string; the prediction is not read again)
//   3. rocprim::partition  the item numbers, active ones first in their order, the others behind
//                          them (in reverse order), and the number of active ones
// The lists feed the V3_LIST / V3_ZERO instantiations of consensus_v3_kernel (launch_consensus_v3_lists).
#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "ppp_kernels.hpp"

namespace ppp {

// one wave per word: 64 voxels of a line, lane 0 stores the ballot.  Bits beyond X stay 0.
template <typename T>
__global__ void __launch_bounds__(256)
    valid_bits_kernel(const T *__restrict__ mid, const uint8_t *__restrict__ ov,
                      unsigned long long *__restrict__ bits, const Geo G, const int wpl, const int z_lo,
                      const long long n_words) {
    const long long word = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (word >= n_words) return;
    const int lane = threadIdx.x & 63;
    const long long line = word / wpl + (long long)z_lo * G.Y;      // z * Y + y
    const int x = (int)(word % wpl) * 64 + lane;
    bool v = false;
    if (x < G.X) {
        const long long l = line * G.X + x;
        v = ldf(mid, l) > G.th_gt && (!G.use_overlap || ov[l] == 0);
    }
    const unsigned long long b = __ballot(v);
    if (lane == 0) bits[line * wpl + word % wpl] = b;
}

// bits of the voxels x0 .. x0 + 63 of line (z, y); voxels outside [0, X) are 0
__device__ __forceinline__ unsigned long long line_bits(const unsigned long long *__restrict__ bits, int wpl,
                                                        long long line, int x0) {
    const int w = x0 >> 6, sh = x0 & 63;          // (arithmetic shift: floor for negative x0)
    const unsigned long long lo = (w >= 0 && w < wpl) ? bits[line * wpl + w] : 0ull;
    const unsigned long long hi = (w + 1 >= 0 && w + 1 < wpl) ? bits[line * wpl + w + 1] : 0ull;
    return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

// the geometry of consensus_v3_kernel, item by item (wid -> run, row; run -> base voxels)
template <bool FLAT>
__global__ void __launch_bounds__(256)
    item_flags_kernel(const unsigned long long *__restrict__ bits, uint8_t *__restrict__ flags, const Geo G,
                      const int wpl, const int n_rows, const int runs_per_line, const long long n_items) {
    const long long wid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (wid >= n_items) return;
    const int PX = G.px;
    const int row = (int)(wid % n_rows);
    long long run = wid / n_rows;
    int dz, dy;
    if (row < G.py) { dz = 0; dy = row; }
    else { const int t = row - G.py; dz = 1 + t / G.wy; dy = t % G.wy - (G.py - 1); }
    const int xr = (int)(run % runs_per_line);
    run /= runs_per_line;
    int uy, uz, ux0, nA;
    if (FLAT) {
        const int flat0 = xr * 64;
        uy = G.cy0 + flat0 / G.cX;
        uz = G.cz0 + 2 * (int)run;
        ux0 = G.cx0 + flat0 % G.cX;
        nA = min(64, G.cX - flat0 % G.cX);
    } else {
        uy = G.cy0 + (int)(run % G.cY);
        uz = G.cz0 + 2 * (int)(run / G.cY);
        ux0 = G.cx0 + xr * 64;
        nA = min(64, G.cx0 + G.cX - ux0);          // (lane_ok: ux < cx0 + cX)
    }
    const bool have_s1 = uz + 1 < G.cz0 + G.cZ;
    const bool have_b = FLAT && nA < 64 && uy + 1 < G.cy0 + G.cY;
    const bool row0 = dz == 0 && dy == 0;
    const int k_lo = row0 ? PX : 0, k_hi = 2 * (PX - 1);          // k = dx + PX - 1
    bool active = false;
    for (int s = 0; s < 2; ++s) {
        if (s == 1 && !have_s1) break;
        for (int b = 0; b < (have_b ? 2 : 1); ++b) {
            const int xs = b ? G.cx0 : ux0, n = b ? 64 - nA : nA, yu = uy + b;
            const unsigned long long m = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
            const unsigned long long U = line_bits(bits, wpl, (long long)(uz + s) * G.Y + yu, xs) & m;
            if (U == 0ull) continue;
            const int zw = uz + s + dz, yw = yu + dy;
            if (zw >= G.Z || yw < 0 || yw >= G.Y) continue;
            const long long lw = (long long)zw * G.Y + yw;
            const unsigned long long w0 = line_bits(bits, wpl, lw, xs - (PX - 1)),
                                     w1 = line_bits(bits, wpl, lw, xs - (PX - 1) + 64);
            // D bit j = OR over dx of valid[w = (xs + j) + dx]: string index j + k
            unsigned long long D = 0ull;
            for (int k = k_lo; k <= k_hi; ++k) D |= k ? (w0 >> k) | (w1 << (64 - k)) : w0;
            active = active || (U & D) != 0ull;
        }
    }
    flags[wid] = active ? 1 : 0;
}

struct SparseWork {
    unsigned long long *bits;   // [Z * Y * wpl]
    uint8_t *flags;             // [n_items]
    uint32_t *items;            // [n_items]: active ones first, the others behind them in reverse order
    unsigned long long *count;  // [1]
    void *temp;
    size_t temp_bytes;
};
static size_t partition_temp_bytes(long long n) {
    size_t a = 0;
    (void)rocprim::partition(nullptr, a, rocprim::counting_iterator<uint32_t>(0), (uint8_t *)nullptr,
                             (uint32_t *)nullptr, (unsigned long long *)nullptr, (size_t)n, (hipStream_t)0);
    return up256(a);
}
static int words_per_line(const Geo &G) { return (G.X + 63) / 64; }

static SparseWork consensus_sparse_layout(Carver &c, const Geo &G, const V3Items &I) {
    SparseWork W;
    W.bits = c.take<unsigned long long>((size_t)G.Z * G.Y * words_per_line(G));
    W.flags = c.take<uint8_t>(I.n_items);
    W.items = c.take<uint32_t>(I.n_items);
    W.count = (unsigned long long *)c.take_bytes(256);
    W.temp_bytes = partition_temp_bytes(I.n_items);
    W.temp = c.take_bytes(W.temp_bytes);
    return W;
}
// 0: not supported (no packed kernel for these parameters, or more items than 32-bit item numbers hold)
size_t consensus_sparse_workspace_bytes(const Geo &G) {
    if (!consensus_v3_supported(G) || (G.layout != PPP_CONS_COMPACT && G.layout != PPP_CONS_VOXEL_MAJOR)) return 0;
    const V3Items I = consensus_v3_items(G);
    if (I.n_items <= 0 || I.n_items >= (1ll << 31)) return 0;
    Carver c(nullptr);
    consensus_sparse_layout(c, G, I);
    return c.used;
}

// at or above this share of active items the lists gain nothing over the dense launch (auto mode).
// Measured break-even less the run-to-run spread of the dense launch: DESIGN.md, "S1 on sparse foreground".
#ifndef PPP_S1_SPARSE_SHARE
#define PPP_S1_SPARSE_SHARE 0.5
#endif

hipError_t run_consensus_sparse(const void *pred, int dtype, const uint8_t *ov, float *cons, float *cnt,
                                const Geo &G, void *work, int mode, long long *total, long long *active,
                                int *took_lists, hipStream_t s) {
    const V3Items I = consensus_v3_items(G);
    note_consensus_short_form(0);
    if (consensus_sparse_workspace_bytes(G) == 0) return hipErrorNotSupported;
    Carver carver(work);
    const SparseWork W = consensus_sparse_layout(carver, G, I);
    const int wpl = words_per_line(G);
    // slices the base voxels and their partners (dz >= 0) lie in
    const int z_lo = G.cz0, z_hi = std::min(G.Z, G.cz0 + G.cZ + G.pz - 1);
    const long long n_words = (long long)(z_hi - z_lo) * G.Y * wpl;
    PPP_GRID_CHECK((n_words + 3) / 4, 256);
    PPP_GRID_CHECK((I.n_items + 255) / 256, 256);
    const dim3 bgrid((unsigned)((n_words + 3) / 4)), block(256);
    {
        const hipError_t e_ = with_pred_type(dtype, [&](auto tag) {
            using T = PPP_PRED_T(tag);
            valid_bits_kernel<T><<<bgrid, block, 0, s>>>((const T *)pred + (long long)G.mid * G.V, ov, W.bits, G, wpl, z_lo, n_words);
            return hipSuccess;
        });
        if (e_ != hipSuccess) return e_;
    }
    const dim3 igrid((unsigned)((I.n_items + 255) / 256));
    if (I.flat)
        item_flags_kernel<true><<<igrid, block, 0, s>>>(W.bits, W.flags, G, wpl, I.n_rows, I.runs_per_line, I.n_items);
    else
        item_flags_kernel<false><<<igrid, block, 0, s>>>(W.bits, W.flags, G, wpl, I.n_rows, I.runs_per_line, I.n_items);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t tb = W.temp_bytes;
    if ((e = rocprim::partition(W.temp, tb, rocprim::counting_iterator<uint32_t>(0), W.flags, W.items, W.count,
                                (size_t)I.n_items, s)) != hipSuccess) return e;
    unsigned long long n_act = 0;
    if ((e = hipMemcpyAsync(&n_act, W.count, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    *total = I.n_items;
    *active = (long long)n_act;
    const bool lists = mode == 1 || (double)n_act < PPP_S1_SPARSE_SHARE * (double)I.n_items;
    *took_lists = lists ? 1 : 0;
    if (!lists) {
        // today's launch, unchanged: same kernel, same grid
        note_consensus_kernel("consensus_v3_kernel");
        return launch_consensus_v3(pred, dtype, ov, cons, cnt, G, s);
    }
    note_consensus_kernel("consensus_v3_kernel<lists>");
    return launch_consensus_v3_lists(pred, dtype, ov, cons, cnt, G, W.items, (long long)n_act, W.items + n_act,
                                     I.n_items - (long long)n_act, s);
}

}  // namespace ppp
