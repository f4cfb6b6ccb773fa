// ppp_patch_loss.hip -- the masked BCE-with-logits patch loss FROM THE LABELS, forward and backward, without the
// target ever being stored (experiments/flylight/setups/setup01/torch_loss.py:47-67 over
// PatchPerPix/util/train_util.py:523-610).
//
//   G[b][e][v]  the multi-channel dense predicate of ppp_gt_affs.hip, for the voxels v of the box
//   l(x, g)   = max(x, 0) - x g + log1p(exp(-|x|))
//   forward     loss = sum_{b,e,v} w[b][v] l(x[b][e][v], G[b][e][v]) / cnt,   cnt = num_channels sum w  (0 if cnt == 0)
//               without weights w = 1 and cnt = B E bV
//   backward    grad[b][e][v] = (s grad_out) w[b][v] (sigmoid(x) - g),  s = 1 / cnt (0 if cnt == 0)
//   A voxel with w == 0 contributes 0 and gets gradient 0 whatever its logits hold (NaN included); a 16-byte group
//   whose weights are all zero is not read at all unless the counters are asked for.
//
// patch_loss_kernel walks the tiles exactly as gt_dense_kernel does (same planner, same staging of labels plus
// halo in LDS, same compare in the pass layout, __ballot as the change of layout) and CONSUMES the bits where
// gt_dense_kernel stores them: lane j of a chunk holds VEC consecutive voxels, loads their logits of one edge
// with one 16-byte load (the loads of the next four edges are in flight while an edge is consumed) and
//   FWD   adds l into VEC float32 accumulators, one per voxel, over the edges of its range; after the range each
//         is multiplied ONCE by w and widened to double.  Doubles are added lane -> wave (xor shuffles) ->
//         workgroup (LDS, wave order) and ONE double per workgroup goes into the workgroup's own slot; sum w the
//         same way, from the workgroups of edge range 0 / part 0 only, so each voxel counts once.
//         patch_loss_finalize (one workgroup) adds the slots: thread t the slots t, t + 256, ... in index order,
//         then the 256 partial sums in a fixed tree.  No floating-point atomic anywhere: the loss, s and with
//         them the gradient have the same bits in every run.  The three integer counters use 64-bit atomic adds.
//   BWD   t = exp(-|x|), r = 1 / (1 + t); sigmoid(x) - g = g ? -sigmoid(-x) : sigmoid(x), each t r or r by the
//         sign of x: no cancellation at either end.  The product with (s grad_out) w is rounded to the element
//         type AFTER the multiplication; every element of grad is written with 16-byte stores, zeros included.
// The staging code is this file's own copy: ppp_gt_affs.hip compiles to what it compiled to before.
// patch_loss_samples_kernel: one wave per sample row, lanes over e (gt_samples_kernel's walk).
#include "ppp_kernels.hpp"

namespace ppp {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kRegCh = 4;            // channels whose centre labels a lane keeps in registers
constexpr int kFill = 8;             // loads a thread has in flight while the region is staged
constexpr int kFinal = 256;          // threads of the finalize workgroup
constexpr int kAhead = 4;            // edges whose logits a lane has in flight (divides 64)

struct LossDense {
    int B, L, Z, Y, X, E;
    int bz0, by0, bx0, bZ, bY, bX;   // the box
    int TZ, TY, TX, shx, shy;        // tile; TX = 1 << shx, TY = 1 << shy
    int ntz, nty, ntx;               // tiles per axis of the box
    int hz0, hy0, hx0, hz1, hy1, hx1;   // halo, widened to hold offset 0
    int RZ, RY, RX;                  // staged region = tile + halo
    unsigned mRZ, mRY, mRX;          // ceil(2^32 / R*)
    int esplit;                      // edge ranges per tile (gridDim.y)
};

__device__ __forceinline__ int udiv(const int n, const int d, const unsigned m) {
    return d == 1 ? n : (int)__umulhi((unsigned)n, m);
}

// ---- element types: VEC elements are 16 bytes, kept as four raw dwords until they are used ----
template <typename T> __device__ __forceinline__ float widen(unsigned bits);
template <> __device__ __forceinline__ float widen<float>(unsigned bits) { return __uint_as_float(bits); }
template <> __device__ __forceinline__ float widen<__half>(unsigned bits) { return __half2float(__ushort_as_half((unsigned short)bits)); }
template <> __device__ __forceinline__ float widen<bf16_t>(unsigned bits) { return __uint_as_float(bits << 16); }

// round to nearest-even into the element type
template <typename T> __device__ __forceinline__ unsigned narrow(float v);
template <> __device__ __forceinline__ unsigned narrow<float>(float v) { return __float_as_uint(v); }
template <> __device__ __forceinline__ unsigned narrow<__half>(float v) { return (unsigned)__half_as_ushort(__float2half_rn(v)); }
template <> __device__ __forceinline__ unsigned narrow<bf16_t>(float v) {
    const unsigned u = __float_as_uint(v);
    if (v != v) return 0x7FC0u | (u >> 31 << 15);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

template <typename T> __device__ __forceinline__ float elem(const unsigned (&r)[4], const int i) {
    if constexpr (sizeof(T) == 4) return widen<T>(r[i]);
    else return widen<T>((r[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
}

// the VEC elements at p, of which the first nval exist (nval == 0: nothing is read); the rest read as 0.
// ALIGNED: every group is whole or empty and 16-byte aligned.  Otherwise the widest aligned pieces, as
// gt_dense_kernel stores them.
template <typename T, bool ALIGNED>
__device__ __forceinline__ void load_group(const T *p, const int nval, unsigned (&r)[4]) {
    constexpr int VEC = 16 / (int)sizeof(T);
    r[0] = r[1] = r[2] = r[3] = 0u;
    if (nval <= 0) return;
    const uintptr_t a = (uintptr_t)p;
    if (ALIGNED || (nval == VEC && (a & 15) == 0)) {
        const uint4 v = *(const uint4 *)p;
        r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
    } else if (nval == VEC && (a & 7) == 0) {
        const uint2 v0 = *(const uint2 *)p, v1 = *((const uint2 *)p + 1);
        r[0] = v0.x; r[1] = v0.y; r[2] = v1.x; r[3] = v1.y;
    } else if (nval == VEC && (a & 3) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = ((const unsigned *)p)[q];
    } else {
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < nval) r[q] = ((const unsigned *)p)[q];
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (q < nval) r[q >> 1] |= (unsigned)((const unsigned short *)p)[q] << (16 * (q & 1));
        }
    }
}

template <typename T, bool ALIGNED>
__device__ __forceinline__ void store_group(T *p, const int nval, const unsigned (&r)[4]) {
    constexpr int VEC = 16 / (int)sizeof(T);
    if (nval <= 0) return;
    const uintptr_t a = (uintptr_t)p;
    if (ALIGNED || (nval == VEC && (a & 15) == 0)) {
        *(uint4 *)p = make_uint4(r[0], r[1], r[2], r[3]);
    } else if (nval == VEC && (a & 7) == 0) {
        *(uint2 *)p = make_uint2(r[0], r[1]);
        *((uint2 *)p + 1) = make_uint2(r[2], r[3]);
    } else if (nval == VEC && (a & 3) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) ((unsigned *)p)[q] = r[q];
    } else {
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < nval) ((unsigned *)p)[q] = r[q];
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (q < nval) ((unsigned short *)p)[q] = (unsigned short)(r[q >> 1] >> (16 * (q & 1)));
        }
    }
}

// exp(-|x|) from the hardware's 2^h (v_exp_f32, 1 ulp).  h = -|x| log2(e) is rounded once; what the rounding
// and the float32 constant drop, l, comes back as the factor 1 + l ln 2, so the error does not grow with |x|
// (a plain 2^(x log2 e) is off by |x| 2^-24 relative: 50 ulp at |x| = 100).  |x| > 200, infinity included, gives
// the 0 it rounds to; a NaN stays a NaN (the compare is false).
__device__ __forceinline__ float exp_neg_abs(const float x) {
    const float a = fabsf(x);
    const float y = a > 200.0f ? -200.0f : -a;
    const float h = y * 1.44269502e+0f;
    const float l = __builtin_fmaf(y, 1.44269502e+0f, -h) + y * 1.92596303e-8f;
    const float e = __builtin_amdgcn_exp2f(h);
    return __builtin_fmaf(e, l * 6.93147182e-1f, e);
}

// log1p(t) for 0 <= t <= 1 from the hardware's log2 (v_log_f32): u = 1 + t drops d = t - (u - 1), exactly
// representable, which returns as d / u; d <= 2^-24 u, so 1 - t serves for 1 / u (exact to t^2 where the term
// counts, below 2^-25 of the result where it does not).  t < 2^-24 gives t.
__device__ __forceinline__ float log1p_unit(const float t) {
    const float u = 1.0f + t;
    const float d = t - (u - 1.0f);
    return __builtin_fmaf(__builtin_amdgcn_logf(u), 6.93147182e-1f, d * (1.0f - t));
}

// l(x, g) = max(x, 0) - x g + log1p(exp(-|x|))
__device__ __forceinline__ float bce_term(const float x, const bool g) {
    const float lin = g ? fmaxf(-x, 0.0f) : fmaxf(x, 0.0f);       // max(x, 0) - x g, exact
    return lin + log1p_unit(exp_neg_abs(x));
}

// sigmoid(x) - g without cancellation: g ? -sigmoid(-x) : sigmoid(x)
__device__ __forceinline__ float bce_slope(const float x, const bool g) {
    const float t = exp_neg_abs(x);
    const float r = __builtin_amdgcn_rcpf(1.0f + t);
    const float big = r, small = t * r;                            // sigmoid(|x|), sigmoid(-|x|)
    if (g) return x >= 0.0f ? -small : -big;
    return x >= 0.0f ? big : small;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sums in LDS by wave order; thread 0 returns the workgroup's totals.  `lds` holds 2 kWaves doubles.
__device__ __forceinline__ void block_slots(double a, double b, double *lds, double *slot_a, double *slot_b, const long long slot) {
    a = wave_sum(a);
    b = wave_sum(b);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                     // the staged labels are no longer read
    if (lane == 0) { lds[wave] = a; lds[kWaves + wave] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sa = 0.0, sb = 0.0;
        for (int w = 0; w < kWaves; ++w) { sa += lds[w]; sb += lds[kWaves + w]; }
        slot_a[slot] = sa;
        if (slot_b) slot_b[slot] = sb;
    }
}

// FWD: slots_l / slots_w receive the workgroup's sums, counts (or NULL) the three integer sums.
// !FWD: grad is written; state[0] = s, grad_out[0] the incoming gradient.
template <typename T, bool STAGED, bool ALIGNED, bool FWD>
__global__ void __launch_bounds__(kBlock)
    patch_loss_kernel(const T *__restrict__ logits, const int32_t *__restrict__ labels, const int32_t *__restrict__ nhood,
                      const float *__restrict__ weight, double *__restrict__ slots_l, double *__restrict__ slots_w,
                      unsigned long long *__restrict__ counts, const double *__restrict__ state,
                      const float *__restrict__ grad_out, T *__restrict__ grad, const LossDense G) {
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr int CH = 64 * VEC;
    extern __shared__ __align__(16) int32_t pl_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    // Workgroups are dealt to the 8 XCDs in turn, each with an L2 of its own.  A tile row is 32 voxels wide and
    // starts on no 128-byte line, so x-neighbours share the lines at their common edge: consecutive tiles (x
    // fastest) go to ONE XCD, which then fetches such a line once.
    const unsigned per = gridDim.x / 8;
    unsigned t = blockIdx.x < 8 * per ? (blockIdx.x % 8) * per + blockIdx.x / 8 : blockIdx.x;
    const int tix = (int)(t % (unsigned)G.ntx); t /= (unsigned)G.ntx;
    const int tiy = (int)(t % (unsigned)G.nty); t /= (unsigned)G.nty;
    const int tiz = (int)(t % (unsigned)G.ntz);
    const int b = (int)(t / (unsigned)G.ntz);
    const int oz = tiz * G.TZ, oy = tiy * G.TY, ox = tix * G.TX;            // in box coordinates
    const int w0 = (int)((long long)G.E * blockIdx.y / G.esplit), w1 = (int)((long long)G.E * (blockIdx.y + 1) / G.esplit);
    const long long V = (long long)G.Z * G.Y * G.X;
    const long long bV = (long long)G.bZ * G.bY * G.bX;
    const int32_t *lab = labels + (long long)b * G.L * V;
    const T *xb = logits + (long long)b * G.E * bV;
    T *gb = FWD ? nullptr : grad + (long long)b * G.E * bV;
    const float *wb = weight ? weight + (long long)b * bV : nullptr;
    const int CS = G.RZ * G.RY * G.RX;                                       // words per staged channel
    const bool want_counts = FWD && counts != nullptr;
    float coef = 0.0f;
    if (!FWD) coef = (float)(state[0] * (double)grad_out[0]);

    if (STAGED) {
        const int gz0 = G.bz0 + oz + G.hz0, gy0 = G.by0 + oy + G.hy0, gx0 = G.bx0 + ox + G.hx0;
        const int total = G.L * CS;
        for (int base = threadIdx.x; base < total; base += kBlock * kFill) {
            int32_t v[kFill];
#pragma unroll
            for (int j = 0; j < kFill; ++j) {
                const int idx = base + j * kBlock;
                v[j] = 0;
                if (idx < total) {
                    const int row = udiv(idx, G.RX, G.mRX), x = idx - row * G.RX;
                    const int zc = udiv(row, G.RY, G.mRY), y = row - zc * G.RY;
                    const int c = udiv(zc, G.RZ, G.mRZ), z = zc - c * G.RZ;
                    const int gz = gz0 + z, gy = gy0 + y, gx = gx0 + x;
                    if ((unsigned)gz < (unsigned)G.Z && (unsigned)gy < (unsigned)G.Y && (unsigned)gx < (unsigned)G.X)
                        v[j] = lab[(long long)c * V + ((long long)gz * G.Y + gy) * G.X + gx];
                }
            }
#pragma unroll
            for (int j = 0; j < kFill; ++j)
                if (base + j * kBlock < total) pl_lds[base + j * kBlock] = v[j];
        }
        __syncthreads();
    }

    double lane_l = 0.0, lane_w = 0.0;
    unsigned long long c_pos = 0, c_gt = 0, c_both = 0;

    const int nchunks = (G.TZ * G.TY * G.TX) / CH;
    const int esub = nchunks < kWaves ? kWaves / nchunks : 1;
    for (int unit = wave; unit < nchunks * esub; unit += kWaves) {
        const int chunk = unit % nchunks, part = unit / nchunks;
        const int e0 = w0 + (int)((long long)(w1 - w0) * part / esub), e1 = w0 + (int)((long long)(w1 - w0) * (part + 1) / esub);
        // ---- pass layout: the centres ----
        int cidx[VEC];
        int vz[VEC], vy[VEC], vx[VEC];
        int32_t cl[VEC][kRegCh];
        bool fg[VEC];
        unsigned long long fgm[VEC];
        unsigned long long any_fg = 0, any_in = 0;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const int tt = chunk * CH + 64 * k + lane;
            const int tx = tt & (G.TX - 1), ty = (tt >> G.shx) & (G.TY - 1), tz = tt >> (G.shx + G.shy);
            const bool inb = oz + tz < G.bZ && oy + ty < G.bY && ox + tx < G.bX;
            cidx[k] = ((tz - G.hz0) * G.RY + (ty - G.hy0)) * G.RX + (tx - G.hx0);
            vz[k] = G.bz0 + oz + tz; vy[k] = G.by0 + oy + ty; vx[k] = G.bx0 + ox + tx;
            const long long cv = ((long long)vz[k] * G.Y + vy[k]) * G.X + vx[k];
            bool f = false;
#pragma unroll
            for (int c = 0; c < kRegCh; ++c) {
                cl[k][c] = 0;
                if (c < G.L && inb) cl[k][c] = STAGED ? pl_lds[cidx[k] + c * CS] : lab[(long long)c * V + cv];
                f |= cl[k][c] != 0;
            }
            for (int c = kRegCh; c < G.L; ++c)
                if (inb) f |= (STAGED ? pl_lds[cidx[k] + c * CS] : lab[(long long)c * V + cv]) != 0;
            fg[k] = f && inb;
            fgm[k] = __ballot(fg[k]);
            any_fg |= fgm[k];
            any_in |= __ballot(inb);
        }
        if (any_in == 0) continue;       // a chunk of the tile's overhang past the box

        // ---- the lane's VEC consecutive voxels ----
        const int ts = chunk * CH + VEC * lane;
        const int sx = ts & (G.TX - 1), sy = (ts >> G.shx) & (G.TY - 1), sz = ts >> (G.shx + G.shy);
        int nval = 0;
        if (oz + sz < G.bZ && oy + sy < G.bY) nval = min(max(G.bX - (ox + sx), 0), VEC);
        const long long sbase = ((long long)(oz + sz) * G.bY + (oy + sy)) * G.bX + (ox + sx);
        const int which = (VEC * lane) >> 6, shift = (VEC * lane) & 63;

        float wv[VEC];
        bool live = false;               // some voxel of the group has weight
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            wv[i] = 0.0f;
            if (i < nval) wv[i] = wb ? wb[sbase + i] : 1.0f;
            live |= wv[i] != 0.0f;
        }
        // a group without weight is not read (its logits may hold anything) unless it is counted
        const int nload = live || want_counts ? nval : 0;

        float acc[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;

        // the logits of the next kAhead edges are on their way while an edge is compared and consumed: at two
        // workgroups per CU one load per wave in flight leaves the memory idle
        unsigned buf[kAhead][4];
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            buf[j][0] = buf[j][1] = buf[j][2] = buf[j][3] = 0u;
            if (e0 + j < e1) load_group<T, ALIGNED>(xb + (long long)(e0 + j) * bV + sbase, nload, buf[j]);
        }
        for (int eb = e0; eb < e1; eb += 64) {
            // 64 edges, one per lane; v_readlane hands them round
            int dz = 0, dy = 0, dx = 0;
            if (any_fg != 0 && eb + lane < e1) {
                dz = nhood[3 * (long long)(eb + lane)];
                dy = nhood[3 * (long long)(eb + lane) + 1];
                dx = nhood[3 * (long long)(eb + lane) + 2];
            }
            int offl = 0;
            if (STAGED) {
                // an offset outside the halo the caller gave would leave the region: it reads the centre instead
                const bool inside = dz >= G.hz0 && dz <= G.hz1 && dy >= G.hy0 && dy <= G.hy1 && dx >= G.hx0 && dx <= G.hx1;
                offl = inside ? (dz * G.RY + dy) * G.RX + dx : 0;
            } else {
                // |n| >= S gives zeros like |n| == S, and v + n then stays within 32 bits
                dz = min(max(dz, -G.Z), G.Z); dy = min(max(dy, -G.Y), G.Y); dx = min(max(dx, -G.X), G.X);
            }
            const int ne = min(64, e1 - eb);
            for (int q0 = 0; q0 < ne; q0 += kAhead) {
#pragma unroll
              for (int j = 0; j < kAhead; ++j) {            // edge e0 + r lives in buf[r % kAhead]; 64 % kAhead == 0
                const int q = q0 + j;
                if (q >= ne) break;
                unsigned (&cur)[4] = buf[j];
                const long long eo = (long long)(eb + q) * bV;
                unsigned bits = 0u;
                if (any_fg != 0) {       // chunks without foreground read no neighbour: G = 0
                    const int off = __builtin_amdgcn_readlane(offl, q);
                    const int ez = __builtin_amdgcn_readlane(dz, q), ey = __builtin_amdgcn_readlane(dy, q),
                              ex = __builtin_amdgcn_readlane(dx, q);
                    const long long goff = ((long long)ez * G.Y + ey) * G.X + ex;
                    unsigned long long m[VEC];
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        m[k] = 0;
                        if (fgm[k] == 0) continue;              // wave-uniform
                        bool ok = true;                          // !STAGED: the neighbour lies inside the volume
                        long long nv = 0;
                        if (!STAGED) {
                            ok = (unsigned)vz[k] + (unsigned)ez < (unsigned)G.Z && (unsigned)vy[k] + (unsigned)ey < (unsigned)G.Y &&
                                 (unsigned)vx[k] + (unsigned)ex < (unsigned)G.X;
                            nv = ((long long)vz[k] * G.Y + vy[k]) * G.X + vx[k] + goff;
                        }
                        bool p = false;
                        if (fg[k]) {
#pragma unroll
                            for (int c = 0; c < kRegCh; ++c) {
                                if (c < G.L) {
                                    const int32_t n = STAGED ? pl_lds[cidx[k] + c * CS + off]
                                                             : (ok ? lab[(long long)c * V + nv] : 0);
                                    p |= n == cl[k][c] && n != 0;
                                }
                            }
                            for (int c = kRegCh; c < G.L; ++c) {
                                const int32_t cc = STAGED ? pl_lds[cidx[k] + c * CS] : lab[(long long)c * V + nv - goff];
                                const int32_t n = STAGED ? pl_lds[cidx[k] + c * CS + off]
                                                         : (ok ? lab[(long long)c * V + nv] : 0);
                                p |= n == cc && n != 0;
                            }
                        }
                        m[k] = __ballot(p);
                    }
                    unsigned long long mine = m[0];
#pragma unroll
                    for (int k = 1; k < VEC; ++k) mine = which == k ? m[k] : mine;
                    bits = (unsigned)(mine >> shift) & ((1u << VEC) - 1u);
                }
                if (FWD) {
                    if (nload) {
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            const float x = elem<T>(cur, i);
                            const bool g = (bits >> i) & 1u;
                            if (wv[i] != 0.0f) acc[i] += bce_term(x, g);
                            if (want_counts && i < nval) {
                                c_pos += x > 0.0f;
                                c_gt += g;
                                c_both += x > 0.0f && g;
                            }
                        }
                    }
                } else {
                    unsigned out[4] = {0u, 0u, 0u, 0u};
                    if (nload) {
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            float gv = 0.0f;
                            if (wv[i] != 0.0f) gv = coef * wv[i] * bce_slope(elem<T>(cur, i), (bits >> i) & 1u);
                            if constexpr (sizeof(T) == 4) out[i] = narrow<T>(gv);
                            else out[i >> 1] |= narrow<T>(gv) << (16 * (i & 1));
                        }
                    }
                    store_group<T, ALIGNED>(gb + eo + sbase, nval, out);
                }
                if (eb + q + kAhead < e1) load_group<T, ALIGNED>(xb + eo + kAhead * bV + sbase, nload, cur);
              }
            }
        }
        if (FWD) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                if (wv[i] != 0.0f) lane_l += (double)(wv[i] * acc[i]);
                if (blockIdx.y == 0 && part == 0) lane_w += (double)wv[i];
            }
        }
    }

    if (FWD) {
        block_slots(lane_l, lane_w, (double *)pl_lds, slots_l, slots_w, (long long)blockIdx.y * gridDim.x + blockIdx.x);
        if (want_counts) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                c_pos += __shfl_xor(c_pos, o, 64);
                c_gt += __shfl_xor(c_gt, o, 64);
                c_both += __shfl_xor(c_both, o, 64);
            }
            if (lane == 0) {
                if (c_pos) atomicAdd(counts, c_pos);
                if (c_gt) atomicAdd(counts + 1, c_gt);
                if (c_both) atomicAdd(counts + 2, c_both);
            }
        }
    }
}

// One workgroup.  Thread t adds the slots t, t + kFinal, ... in index order, then a fixed tree over the threads.
// cnt = has_w ? num_channels * sum w : denom;  s = cnt == 0 ? 0 : 1 / cnt;  state = (s, sum w)
__global__ void __launch_bounds__(kFinal)
    patch_loss_finalize(const double *__restrict__ slots_l, const double *__restrict__ slots_w, const long long n,
                        const int has_w, const double num_channels, const double denom, float *__restrict__ loss,
                        double *__restrict__ state) {
    __shared__ double sl[kFinal], sw[kFinal];
    double a = 0.0, b = 0.0;
    for (long long i = threadIdx.x; i < n; i += kFinal) {
        a += slots_l[i];
        if (has_w) b += slots_w[i];
    }
    sl[threadIdx.x] = a;
    sw[threadIdx.x] = b;
    __syncthreads();
    for (int o = kFinal / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sl[threadIdx.x] += sl[threadIdx.x + o];
            sw[threadIdx.x] += sw[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double cnt = has_w ? num_channels * sw[0] : denom;
        const bool live = cnt > 0.0 || cnt < 0.0;              // a NaN count gives 0 like an empty one
        loss[0] = live ? (float)(sl[0] / cnt) : 0.0f;
        state[0] = live ? 1.0 / cnt : 0.0;
        state[1] = has_w ? sw[0] : denom;
    }
}

struct LossSamples {
    int B, L, Z, Y, X, E;
    int pz, py, px, cz, cy, cx;
    long long N;
};

template <typename T, bool FWD>
__global__ void __launch_bounds__(kBlock)
    patch_loss_samples_kernel(const T *__restrict__ logits, const int32_t *__restrict__ labels,
                              const int32_t *__restrict__ samples, const int32_t *__restrict__ nhood,
                              double *__restrict__ slots_l, const double *__restrict__ state,
                              const float *__restrict__ grad_out, T *__restrict__ grad, const LossSamples G) {
    __shared__ double red[2 * kWaves];
    const int lane = threadIdx.x & 63;
    const long long n = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    double lane_l = 0.0;
    if (n < G.N) {
        const long long V = (long long)G.Z * G.Y * G.X;
        const int sb = samples[4 * n];
        const long long z0 = samples[4 * n + 1], y0 = samples[4 * n + 2], x0 = samples[4 * n + 3];
        const bool bok = sb >= 0 && sb < G.B;
        const int32_t *lab = labels + (long long)(bok ? sb : 0) * G.L * V;
        const long long zc = z0 + G.cz, yc = y0 + G.cy, xc = x0 + G.cx;
        const bool cok = bok && zc >= 0 && zc < G.Z && yc >= 0 && yc < G.Y && xc >= 0 && xc < G.X;
        const long long cv = (zc * G.Y + yc) * G.X + xc;
        float coef = 0.0f;
        if (!FWD) coef = (float)(state[0] * (double)grad_out[0]);
        float acc = 0.0f;
        for (int e = lane; e < G.E; e += 64) {
            const int nz = nhood[3 * (long long)e], ny = nhood[3 * (long long)e + 1], nx = nhood[3 * (long long)e + 2];
            const long long z = z0 + nz, y = y0 + ny, x = x0 + nx;
            // inside the patch and inside the volume; everything else reads as background
            const bool ok = cok && (unsigned)nz < (unsigned)G.pz && (unsigned)ny < (unsigned)G.py && (unsigned)nx < (unsigned)G.px &&
                            z >= 0 && z < G.Z && y >= 0 && y < G.Y && x >= 0 && x < G.X;
            bool p = false;
            if (ok) {
                const long long nv = (z * G.Y + y) * G.X + x;
                for (int c = 0; c < G.L; ++c) {
                    const int32_t cc = lab[(long long)c * V + cv], nn = lab[(long long)c * V + nv];
                    p |= nn == cc && nn != 0;
                }
            }
            unsigned raw;
            if constexpr (sizeof(T) == 4) raw = ((const unsigned *)logits)[n * G.E + e];
            else raw = ((const unsigned short *)logits)[n * G.E + e];
            const float xv = widen<T>(raw);
            if (FWD) {
                acc += bce_term(xv, p);
            } else {
                const unsigned o = narrow<T>(coef * bce_slope(xv, p));
                if constexpr (sizeof(T) == 4) ((unsigned *)grad)[n * G.E + e] = o;
                else ((unsigned short *)grad)[n * G.E + e] = (unsigned short)o;
            }
        }
        lane_l = (double)acc;
    }
    if (FWD) block_slots(lane_l, 0.0, red, slots_l, nullptr, (long long)blockIdx.x);
}

struct LossWork {
    double *slots_l, *slots_w;
    long long n;
};

LossWork loss_layout(Carver &c, long long workgroups) {
    LossWork W;
    W.n = workgroups;
    W.slots_l = c.take<double>((size_t)workgroups);
    W.slots_w = c.take<double>((size_t)workgroups);
    return W;
}

// the geometry of a dense call and its grid (x: tiles of all batch items, y: edge ranges)
hipError_t dense_geometry(int B, int L, int Z, int Y, int X, int E, const int *halo, const int *box, LossDense &G,
                          bool &staged, long long &blocks) {
    int32_t plan[5];
    gt_affs_dense_plan(B, L, E, halo, box, plan);
    G.B = B; G.L = L; G.Z = Z; G.Y = Y; G.X = X; G.E = E;
    G.bz0 = box[0]; G.by0 = box[2]; G.bx0 = box[4];
    G.bZ = box[1] - box[0]; G.bY = box[3] - box[2]; G.bX = box[5] - box[4];
    G.TZ = plan[0]; G.TY = plan[1]; G.TX = plan[2];
    G.shx = __builtin_ctz((unsigned)G.TX); G.shy = __builtin_ctz((unsigned)G.TY);
    G.ntz = (G.bZ + G.TZ - 1) / G.TZ; G.nty = (G.bY + G.TY - 1) / G.TY; G.ntx = (G.bX + G.TX - 1) / G.TX;
    staged = plan[3] != 0;
    G.hz0 = staged && halo[0] < 0 ? halo[0] : 0; G.hz1 = staged && halo[1] > 0 ? halo[1] : 0;
    G.hy0 = staged && halo[2] < 0 ? halo[2] : 0; G.hy1 = staged && halo[3] > 0 ? halo[3] : 0;
    G.hx0 = staged && halo[4] < 0 ? halo[4] : 0; G.hx1 = staged && halo[5] > 0 ? halo[5] : 0;
    G.RZ = G.TZ + G.hz1 - G.hz0; G.RY = G.TY + G.hy1 - G.hy0; G.RX = G.TX + G.hx1 - G.hx0;
    G.esplit = plan[4];
    auto magic = [](int d) { return d > 1 ? (unsigned)(((1ull << 32) + d - 1) / d) : 0u; };
    G.mRZ = magic(G.RZ); G.mRY = magic(G.RY); G.mRX = magic(G.RX);
    blocks = (long long)B * G.ntz * G.nty * G.ntx;
    PPP_GRID_CHECK(blocks, kBlock);
    return hipSuccess;
}

template <typename T, bool FWD>
void launch_dense(bool staged, bool aligned, dim3 grid, size_t lds, hipStream_t s, const void *logits, const int32_t *labels,
                  const int32_t *nhood, const float *weight, double *slots_l, double *slots_w, long long *counts,
                  const double *state, const float *grad_out, void *grad, const LossDense &G) {
    auto go = [&](auto kernel) {
        kernel<<<grid, dim3(kBlock), lds, s>>>((const T *)logits, labels, nhood, weight, slots_l, slots_w,
                                               (unsigned long long *)counts, state, grad_out, (T *)grad, G);
    };
    if (staged && aligned) go(patch_loss_kernel<T, true, true, FWD>);
    else if (staged) go(patch_loss_kernel<T, true, false, FWD>);
    else if (aligned) go(patch_loss_kernel<T, false, true, FWD>);
    else go(patch_loss_kernel<T, false, false, FWD>);
}

}  // namespace

size_t patch_loss_workspace_bytes(int B, int L, int E, const int *halo, const int *box, long long N) {
    Carver c(nullptr);
    if (box) {
        int32_t plan[5];
        gt_affs_dense_plan(B, L, E, halo, box, plan);
        long long tiles = B;
        for (int a = 0; a < 3; ++a) tiles *= (box[2 * a + 1] - box[2 * a] + plan[a] - 1) / plan[a];
        loss_layout(c, tiles * plan[4]);
    } else {
        loss_layout(c, (N + kWaves - 1) / kWaves);
    }
    return c.used;
}

// Neither call synchronises.  The caller has checked the sizes (ppp_patch_loss_dense_*).
hipError_t run_patch_loss_dense(bool fwd, const void *logits, int dtype, const int32_t *labels, int B, int L, int Z, int Y,
                                int X, const int32_t *nhood, int E, const int *halo, const int *box, const float *weight,
                                double num_channels, float *loss, double *state, long long *counts, const float *grad_out,
                                void *grad, void *work, hipStream_t s) {
    LossDense G;
    bool staged;
    long long blocks;
    hipError_t err = dense_geometry(B, L, Z, Y, X, E, halo, box, G, staged, blocks);
    if (err != hipSuccess) return err;
    const dim3 grid((unsigned)blocks, (unsigned)G.esplit);
    // the sums of the waves reuse the staged region: at least their 2 kWaves doubles
    size_t lds = staged ? (size_t)L * G.RZ * G.RY * G.RX * sizeof(int32_t) : 0;
    if (lds < 2 * kWaves * sizeof(double)) lds = 2 * kWaves * sizeof(double);
    const int vec = dtype == PPP_F32 ? 4 : 8;
    const bool aligned = G.bX % vec == 0 && ((uintptr_t)logits & 15) == 0 && (fwd || ((uintptr_t)grad & 15) == 0);
    LossWork W{nullptr, nullptr, 0};
    if (fwd) {
        Carver carver(work);
        W = loss_layout(carver, blocks * G.esplit);
        if (counts) {
            err = hipMemsetAsync(counts, 0, 3 * sizeof(long long), s);
            if (err != hipSuccess) return err;
        }
    }
    err = with_pred_type(dtype, [&](auto tag) {
        using T = PPP_PRED_T(tag);
        if (fwd) launch_dense<T, true>(staged, aligned, grid, lds, s, logits, labels, nhood, weight, W.slots_l, W.slots_w, counts,
                                       nullptr, nullptr, nullptr, G);
        else launch_dense<T, false>(staged, aligned, grid, lds, s, logits, labels, nhood, weight, nullptr, nullptr, nullptr,
                                    state, grad_out, grad, G);
        return hipGetLastError();
    });
    if (err != hipSuccess || !fwd) return err;
    const double denom = (double)B * (double)E * (double)G.bZ * (double)G.bY * (double)G.bX;
    patch_loss_finalize<<<dim3(1), dim3(kFinal), 0, s>>>(W.slots_l, W.slots_w, W.n, weight ? 1 : 0, num_channels, denom, loss, state);
    return hipGetLastError();
}

hipError_t run_patch_loss_samples(bool fwd, const void *logits, int dtype, const int32_t *labels, int B, int L, int Z, int Y,
                                  int X, const int32_t *samples, long long N, const int32_t *nhood, int E, const int *ps,
                                  const int *ctr, float *loss, double *state, const float *grad_out, void *grad, void *work,
                                  hipStream_t s) {
    LossSamples G;
    G.B = B; G.L = L; G.Z = Z; G.Y = Y; G.X = X; G.E = E;
    G.pz = ps[0]; G.py = ps[1]; G.px = ps[2];
    G.cz = ctr[0]; G.cy = ctr[1]; G.cx = ctr[2];
    G.N = N;
    const long long blocks = (N + kWaves - 1) / kWaves;
    PPP_GRID_CHECK(blocks, kBlock);
    LossWork W{nullptr, nullptr, 0};
    if (fwd) {
        Carver carver(work);
        W = loss_layout(carver, blocks);
    }
    hipError_t err = with_pred_type(dtype, [&](auto tag) {
        using T = PPP_PRED_T(tag);
        if (fwd)
            patch_loss_samples_kernel<T, true><<<dim3((unsigned)blocks), dim3(kBlock), 0, s>>>(
                (const T *)logits, labels, samples, nhood, W.slots_l, nullptr, nullptr, nullptr, G);
        else
            patch_loss_samples_kernel<T, false><<<dim3((unsigned)blocks), dim3(kBlock), 0, s>>>(
                (const T *)logits, labels, samples, nhood, nullptr, state, grad_out, (T *)grad, G);
        return hipGetLastError();
    });
    if (err != hipSuccess || !fwd) return err;
    patch_loss_finalize<<<dim3(1), dim3(kFinal), 0, s>>>(W.slots_l, W.slots_w, W.n, 0, 1.0, (double)N * (double)E, loss, state);
    return hipGetLastError();
}

}  // namespace ppp
