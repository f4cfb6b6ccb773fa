// ppp_eval.hip -- evaluate_patch (PatchPerPix/evaluate/evaluate_prediction.py:38-150) as one streaming
// reduction over the dense prediction [C][tz][Y][X] of a z-tile.
//
//   ov[v]   = more than one label channel is positive at v
//   G'[e,v] = !ov[v], v + off(e) inside the volume, and the ONE positive channel c of v has
//             labels[c][v] == labels[c][v + off(e)]                 (the ground-truth affinity, never stored)
//   P_t[e,v] = (ov[v] ? 0 : pred[e,v]) > thresholds[t]              (float compare; NaN: false)
//   counts: num_gt = sum G', num_pred_t = sum P_t, tp_t = sum P_t & G'
//   maps:   inter_t[v] = sum_e P_t & G', union_t[v] = sum_e P_t | G'
//
// Two kernels.  eval_centre_kernel: per voxel of the tile (label, channel) of the single positive label
// channel, label 0 for background and -1 for an overlap voxel -- so G' is one label load per element.
// eval_patch_kernel: lanes along the flat voxel index of the tile, VEC consecutive voxels per lane (one
// 16-byte load per channel when the tile's voxel count is a multiple of VEC, else VEC = 1), the channel
// loop inside the lane.  The prediction AND the neighbours' labels of channel e + 1 are loaded while channel
// e is counted: with the label load issued where its value is needed, the kernel waited on it once per
// channel (1.23 -> 0.83 ms at 343 x 140^3 float16, L = 1).  Lanes whose voxels are all
// background or overlap issue no label load, lanes whose voxels are all overlap no prediction load.
// Per voxel and threshold a lane keeps ONE register, (predicted, true positives) packed as 16 + 16 bits
// (tp <= predicted <= C < 65536), and per voxel the number of ground-truth entries: an element costs
// compare, select, add per threshold (inc = 1 + (g << 16) is added where the element is predicted);
// inter = tp and union = predicted + gt - tp come out at the end.  The kernel is instantiated per number of
// thresholds in a pass (1 .. kEvalT), so a pass computes nothing it does not report; more thresholds than
// kEvalT: more passes over the prediction.  kEvalT = 4: with 16-bit elements (VEC = 8) that is 32
// accumulator registers, 123 VGPRs in all and 4 waves per SIMD (115 .. 123 for 1 .. 4 thresholds; float32,
// VEC = 4: 66 .. 72 and 7 waves); 8 thresholds per pass would add 32 more and drop to 3 waves.
// Counters are integers: lane -> wave (shuffles) -> workgroup (LDS) -> one 64-bit atomic add per counter
// and workgroup, so the result does not depend on the order.
#include "ppp_kernels.hpp"

namespace ppp {

namespace {

constexpr int kBlock = 256;

struct EvalTh {
    float th[kEvalT];
};

__global__ void __launch_bounds__(kBlock)
    eval_centre_kernel(const int32_t *__restrict__ labels, const int L, const long long V, const long long v0,
                       const long long n, int32_t *__restrict__ clab, int32_t *__restrict__ cch) {
    const long long i = blockIdx.x * (long long)kBlock + threadIdx.x;
    if (i >= n) return;
    int cnt = 0, lab = 0, ch = 0;
    for (int c = 0; c < L; ++c) {
        const int32_t l = labels[(long long)c * V + v0 + i];
        if (l > 0 && cnt++ == 0) { lab = l; ch = c; }
    }
    clab[i] = cnt == 1 ? lab : (cnt == 0 ? 0 : -1);
    cch[i] = cnt == 1 ? ch : 0;
}

__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(__half v) { return __half2float(v); }
__device__ __forceinline__ float widen(bf16_t v) { return __uint_as_float((unsigned)v.bits << 16); }

template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) EvalPack {
    T v[VEC];
};

template <typename T, int VEC, int NT>
__global__ void __launch_bounds__(kBlock)
    eval_patch_kernel(const T *__restrict__ pred, const int32_t *__restrict__ labels, const int32_t *__restrict__ clab,
                      const int32_t *__restrict__ cch, const int Z, const int Y, const int X, const int rz, const int ry,
                      const int rx, const int z0, const long long n, const EvalTh th, const int first,
                      unsigned long long *__restrict__ counts, int32_t *__restrict__ inter, int32_t *__restrict__ uni) {
    using Pack = EvalPack<T, VEC>;
    const long long V = (long long)Z * Y * X;
    const long long base = (blockIdx.x * (long long)kBlock + threadIdx.x) * VEC;   // (n % VEC == 0)
    const bool active = base < n;
    const int C = (2 * rz + 1) * (2 * ry + 1) * (2 * rx + 1);

    int lab[VEC], xs[VEC], ys[VEC], zs[VEC];
    long long loff[VEC];           // element of labels at the voxel, in its centre channel
    bool any_fg = false, all_ov = true;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        lab[k] = 0; xs[k] = ys[k] = zs[k] = 0; loff[k] = 0;
        if (active) {
            const long long lin = base + k;
            lab[k] = clab[lin];
            xs[k] = (int)(lin % X);
            ys[k] = (int)((lin / X) % Y);
            zs[k] = (int)(lin / ((long long)X * Y)) + z0;
            loff[k] = (long long)cch[lin] * V + ((long long)zs[k] * Y + ys[k]) * X + xs[k];
            any_fg |= lab[k] > 0;
            all_ov &= lab[k] < 0;
        }
    }
    const bool loads = active && !all_ov;

    unsigned acc[NT][VEC];         // predicted | true positives << 16
    unsigned gc[VEC];              // ground-truth entries
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        gc[k] = 0;
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t][k] = 0;
    }

    const Pack *src = (const Pack *)(pred + base);
    const long long step = n / VEC;             // Packs per channel
    // The prediction AND the neighbours' labels of channel e + 1 are loaded while channel e is counted.
    // lv[k]: the label at v + off(e) in the centre's channel, or kNone where the centre is no single-label
    // voxel or the neighbour lies outside (kNone equals no centre label: those are > 0 where they count).
    constexpr int kNone = -2;
    Pack cur = {}, nxt = {};
    int lv[VEC], lvn[VEC];
    bool rowok[VEC];                            // of the row (dz, dy) the NEXT loads come from
    long long roff = 0;
    int dz = -rz, dy = -ry, dx = -rx;           // of the element being LOADED
    auto load_labels = [&](int *out) {
        if (dx == -rx) {
            roff = ((long long)dz * Y + dy) * X;
#pragma unroll
            for (int k = 0; k < VEC; ++k)
                rowok[k] = lab[k] > 0 && (unsigned)(zs[k] + dz) < (unsigned)Z && (unsigned)(ys[k] + dy) < (unsigned)Y;
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            out[k] = kNone;
            if (rowok[k] && (unsigned)(xs[k] + dx) < (unsigned)X) out[k] = labels[loff[k] + roff + dx];
        }
    };
#pragma unroll
    for (int k = 0; k < VEC; ++k) lv[k] = lvn[k] = kNone;
    if (loads) cur = src[0];
    if (any_fg) load_labels(lv);
    for (int e = 0; e < C; ++e) {
        if (++dx > rx) {
            dx = -rx;
            if (++dy > ry) { dy = -ry; ++dz; }
        }
        if (e + 1 < C) {
            if (loads) nxt = src[(long long)(e + 1) * step];
            if (any_fg) load_labels(lvn);
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float val = lab[k] < 0 ? 0.0f : widen(cur.v[k]);
            const unsigned g = lv[k] == lab[k] ? 1u : 0u;
            gc[k] += g;
            const unsigned inc = 1u + (g << 16);     // what a predicted element adds: compare, select, add
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t][k] += val > th.th[t] ? inc : 0u;
        }
        cur = nxt;
#pragma unroll
        for (int k = 0; k < VEC; ++k) lv[k] = lvn[k];
    }

    // per-lane sums: [0] = gt, [1 + 2t] = pred, [2 + 2t] = tp
    unsigned long long sums[1 + 2 * NT];
#pragma unroll
    for (int j = 0; j < 1 + 2 * NT; ++j) sums[j] = 0;
    if (active) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            sums[0] += gc[k];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const unsigned P = acc[t][k] & 0xFFFFu, I = acc[t][k] >> 16, U = P + gc[k] - I;
                sums[1 + 2 * t] += P;
                sums[2 + 2 * t] += I;
                if (inter != nullptr) {
                    inter[(long long)t * n + base + k] = (int32_t)I;
                    uni[(long long)t * n + base + k] = (int32_t)U;
                }
            }
        }
    }
    __shared__ unsigned long long red[kBlock / 64][1 + 2 * NT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 1 + 2 * NT; ++j) {
        unsigned long long s = sums[j];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) red[wave][j] = s;
    }
    __syncthreads();
    const int j = threadIdx.x;
    if (j < 1 + 2 * NT && (j > 0 || first)) {
        unsigned long long s = 0;
        for (int w = 0; w < kBlock / 64; ++w) s += red[w][j];
        if (s) atomicAdd(&counts[j], s);
    }
}

struct EvalWork {
    int32_t *clab;      // [n]: the voxel's single positive label, 0 background, -1 overlap
    int32_t *cch;       // [n]: the label channel that holds it
};
EvalWork eval_layout(Carver &c, long long n) {
    EvalWork W;
    W.clab = c.take<int32_t>((size_t)n);
    W.cch = c.take<int32_t>((size_t)n);
    return W;
}

template <typename T, int VEC>
hipError_t launch_eval_passes(const T *pred, const int32_t *labels, const EvalWork &W, int Z, int Y, int X, const int *r,
                              int z0, long long n, const float *th, int T_, unsigned long long *counts, int32_t *inter,
                              int32_t *uni, hipStream_t s) {
    const long long threads = n / VEC, blocks = (threads + kBlock - 1) / kBlock;
    PPP_GRID_CHECK(blocks, kBlock);
    for (int t0 = 0; t0 < T_; t0 += kEvalT) {
        const int nt = T_ - t0 < kEvalT ? T_ - t0 : kEvalT;
        EvalTh h;
        for (int t = 0; t < kEvalT; ++t) h.th[t] = t < nt ? th[t0 + t] : 0.0f;
        // counts of this pass: [0] stays num_gt (added by the first pass only), the pairs follow at 1 + 2 t0
        auto launch = [&](auto kernel) {
            kernel<<<dim3((unsigned)blocks), dim3(kBlock), 0, s>>>(
                pred, labels, W.clab, W.cch, Z, Y, X, r[0], r[1], r[2], z0, n, h, t0 == 0 ? 1 : 0, counts + 2 * t0,
                inter ? inter + (long long)t0 * n : nullptr, uni ? uni + (long long)t0 * n : nullptr);
        };
        static_assert(kEvalT == 4, "one kernel per number of thresholds in a pass");
        if (nt == 1) launch(eval_patch_kernel<T, VEC, 1>);
        else if (nt == 2) launch(eval_patch_kernel<T, VEC, 2>);
        else if (nt == 3) launch(eval_patch_kernel<T, VEC, 3>);
        else launch(eval_patch_kernel<T, VEC, 4>);
    }
    return hipGetLastError();
}

}  // namespace

size_t eval_patch_workspace_bytes(long long n) { Carver c(nullptr); eval_layout(c, n); return c.used; }

// Does not synchronise.  counts[0] is touched by the first pass only; a later pass gets counts + 2 t0, whose
// element 0 it never adds to (first = 0).
hipError_t run_eval_patch(const void *pred, int dtype, const int32_t *labels, int L, int Z, int Y, int X, int pz, int py,
                          int px, int z0, int tz, const float *th, int T_, long long *counts, int32_t *inter, int32_t *uni,
                          void *work, hipStream_t s) {
    Carver carver(work);
    const long long V = (long long)Z * Y * X, n = (long long)tz * Y * X;
    const EvalWork W = eval_layout(carver, n);
    PPP_GRID_CHECK((n + kBlock - 1) / kBlock, kBlock);
    eval_centre_kernel<<<dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s>>>(
        labels, L, V, (long long)z0 * Y * X, n, W.clab, W.cch);
    const int r[3] = {pz / 2, py / 2, px / 2};
    return with_pred_type(dtype, [&](auto tag) {
        using T = PPP_PRED_T(tag);
        constexpr int WIDE = 16 / (int)sizeof(T);
        if (n % WIDE == 0 && ((uintptr_t)pred & 15) == 0)
            return launch_eval_passes<T, WIDE>((const T *)pred, labels, W, Z, Y, X, r, z0, n, th, T_,
                                               (unsigned long long *)counts, inter, uni, s);
        return launch_eval_passes<T, 1>((const T *)pred, labels, W, Z, Y, X, r, z0, n, th, T_,
                                        (unsigned long long *)counts, inter, uni, s);
    });
}

}  // namespace ppp
