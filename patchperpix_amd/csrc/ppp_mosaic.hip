// ppp_mosaic.hip -- the patch mosaic of `visualize_patches` (PatchPerPix/visualize/patches.py:12-98,
// reshape_affinities / reshape_affinities_3d) as one streaming re-arrangement of a z-tile.
//
//   in  [C][tz][Y][X], C = pz py px, channel c = (k py + j) px + i
//   out [tz][Y py][X px]:  out[z][y py + j][x px + i] = 1                        if j == 0 or i == 0
//                                                    = max_k in[(k py + j) px + i][z][y][x]   otherwise
//   (NumPy's maximum: the running value stays where it is >= the new one or is NaN, so a NaN among the
//   pz values gives NaN.)  pz = 1 is the 2-d mosaic; with a selected block u8 [S][tz][Y][X], S in {1, 3},
//   the output has three channels [3][tz][Y py][X px] and the whole tile of a voxel goes to ONE of them
//   (S = 1: channel 0 where selected, else 2; S = 3: the first of 0, 1, 2 whose flag is set, none where
//   no flag is).  The kernel writes every element of all three channels, zeros included: the caller
//   does not clear the output.
//
// Shape.  A work item is (z, j, a run of kRun = 64 VEC consecutive voxels of the slice's flat (y, x) index);
// one WAVE serves an item, four waves share a workgroup.  A slice is contiguous in a channel, so a run reads
// full lines whatever X is (X = 1 included) and the ragged end is the slice's, not each row's.
//   load:   lane l holds the voxels f0 + l VEC .. + VEC - 1.  For i = 1 .. px - 1 it reads the pz channels of
//           (j, i) -- one coalesced line per channel, VEC elements per lane -- keeps the running maximum in
//           registers and puts the result into the wave's LDS tile at [voxel][i].  Four values of i go
//           together (mosaic_lines), so a lane has four independent loads in flight per step of k.  Channels
//           with j == 0 or i == 0 are never read (their output is 1); every other element is read exactly once.
//   store:  the tile holds, voxel after voxel, the px values of output row y py + j: lanes walk it in
//           order, W elements per lane, and write out[...][x px + i ..].  Consecutive lanes write consecutive
//           addresses; a segment ends where the run crosses into the next y (the output row stride is
//           py X px there).  W is the widest of 16 bytes, 4 bytes (2-byte elements) and one element for
//           which X px and the output base are multiples of W elements: a run starts at a multiple of 64
//           voxels, so W consecutive tile elements starting at a multiple of W then lie in one output row
//           at an aligned address, and the run's element count is a multiple of W.
// LDS.  Tile stride PS = px | 1 elements per voxel (odd).  4-byte elements: lane l writes dword l PS + i,
// 32 lanes on 32 banks.  2-byte elements, VEC = 2: lane l writes elements (2 l + e) PS + i, dword
// l PS + (e PS + i) / 2 -- again stride PS dwords (the arrangement of ppp_rows.hip).  The reading side is
// linear in the tile when px is odd (PS = px): one aligned read of W elements per lane; with an even px the
// tile has one unused element per voxel and the W elements are read one by one.
// 2-byte elements are loaded as one 4-byte pair per lane when every channel line starts 4-byte aligned (Y X
// even, base aligned), else as two 2-byte loads.
// Registers (hipcc -O3, gfx950): 51 .. 56 VGPRs over the 14 instantiations, no spills, no scratch; LDS
// 4 x 64 VEC x (PS sizeof(T) + 1) bytes, 25.5 KiB at px = 25 with 2-byte elements.
// Measured: 343 x 140^3 float16 0.430 ms, 625 x 696 x 520 float16 0.181 ms -- 98 % and 95 %
// of a device-to-device copy of the same byte count.  The first form (one line per step, one element per
// store) took 0.477 ms and 0.460 ms: the 2-d mosaic writes as many bytes as it reads and was bound by
// its 2-byte stores.
#include "ppp_kernels.hpp"

namespace ppp {

namespace {

constexpr int kWaves = 4;
constexpr int kBlock = 64 * kWaves;

// element <-> the float it is compared as; `one` = 1.0 in the element type
__device__ __forceinline__ float mz_widen(float v) { return v; }
__device__ __forceinline__ float mz_widen(__half v) { return __half2float(v); }
__device__ __forceinline__ float mz_widen(bf16_t v) { return __uint_as_float((unsigned)v.bits << 16); }
template <typename T> __device__ __forceinline__ T mz_narrow(float v);
template <> __device__ __forceinline__ float mz_narrow<float>(float v) { return v; }
// (exact: v is the widened value of an element)
template <> __device__ __forceinline__ __half mz_narrow<__half>(float v) { return __float2half(v); }
template <> __device__ __forceinline__ bf16_t mz_narrow<bf16_t>(float v) {
    bf16_t r;
    r.bits = (unsigned short)(__float_as_uint(v) >> 16);
    return r;
}
template <typename T> __device__ __forceinline__ T mz_zero() { return mz_narrow<T>(0.0f); }

template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) MosaicPack {
    T v[VEC];
};

// U lines (channels i0 .. i0 + U - 1 of row j) at once: U independent loads per step of k, so a lane has
// U loads in flight instead of one load and a dependent compare.
template <typename T, int VEC, bool WIDE, int U>
__device__ __forceinline__ void mosaic_lines(const T *p, const long long n, const long long kstep, const int pz, const int nv,
                                             T *trow, const int PS) {
    float m[U][VEC];
    for (int k = 0; k < pz; ++k, p += kstep) {
        float v[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (WIDE) {
                const MosaicPack<T, VEC> pk = *(const MosaicPack<T, VEC> *)(p + u * n);
#pragma unroll
                for (int e = 0; e < VEC; ++e) v[u][e] = mz_widen(pk.v[e]);
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) v[u][e] = e < nv ? mz_widen(p[u * n + e]) : 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                // NumPy's maximum.reduce: keep m where m >= v or m is NaN
                if (k == 0 || (!(v[u][e] <= m[u][e]) && m[u][e] == m[u][e])) m[u][e] = v[u][e];
            }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int e = 0; e < VEC; ++e) trow[e * PS + u] = mz_narrow<T>(m[u][e]);
}

// VEC: voxels per lane in the load phase; WIDE: they are one load; W: output elements per lane and store
// (W > 1: the launcher has checked that X px and the output base are multiples of W elements -- then W
// consecutive elements of the tile, starting at a multiple of W, lie in one output row, at an aligned address)
template <typename T, int VEC, bool WIDE, int W>
__global__ void __launch_bounds__(kBlock)
    patch_mosaic_kernel(const T *__restrict__ in, const uint8_t *__restrict__ sel, const int S, T *__restrict__ out,
                        const int tz, const int Y, const int X, const int pz, const int py, const int px, const int PS,
                        const int runs, const long long items) {
    constexpr int kRun = 64 * VEC;
    constexpr int U = 4;
    extern __shared__ __align__(16) unsigned char mosaic_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T *tile = (T *)mosaic_lds + (size_t)wave * kRun * PS;
    unsigned char *route = mosaic_lds + (size_t)kWaves * kRun * PS * sizeof(T) + wave * kRun;

    const long long item = (long long)blockIdx.x * kWaves + wave;
    const bool live = item < items;
    const int YX = Y * X;                           // (tz Y X < 2^31: the launcher checks)
    const long long n = (long long)tz * YX;         // channel stride
    int z = 0, j = 0, f0 = 0;
    if (live) {
        const int r = (int)(item % runs);
        const long long zj = item / runs;
        j = (int)(zj % py);
        z = (int)(zj / py);
        f0 = r * kRun;
    }
    const int nvox = live ? (YX - f0 < kRun ? YX - f0 : kRun) : 0;      // voxels of this run
    const long long slice = (long long)z * YX + f0;                     // of the run's first voxel in a channel

    // ---- load: running maxima of (j, i) into the tile, [voxel][i] ----
    const int v0 = lane * VEC;
    if (v0 < nvox) {
        const int nv = nvox - v0 < VEC ? nvox - v0 : VEC;
        if (S > 0) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                if (e >= nv) break;
                const uint8_t *sp = sel + slice + v0 + e;
                unsigned char r;
                if (S == 1) r = sp[0] ? 0 : 2;
                else r = sp[0] ? 0 : (sp[n] ? 1 : (sp[2 * n] ? 2 : 3));
                route[v0 + e] = r;
            }
        }
        const T one = mz_narrow<T>(1.0f);
        T *trow = tile + v0 * PS;
#pragma unroll
        for (int e = 0; e < VEC; ++e) trow[e * PS] = one;               // i == 0
        if (j == 0) {
            for (int i = 1; i < px; ++i)
#pragma unroll
                for (int e = 0; e < VEC; ++e) trow[e * PS + i] = one;
        } else {
            const long long kstep = (long long)py * px * n;             // channel (k + 1, j, i) - (k, j, i)
            const T *p = in + (long long)j * px * n + slice + v0;       // channel (0, j, 0) at the lane's voxels
            int i = 1;
            for (; i + U <= px; i += U) mosaic_lines<T, VEC, WIDE, U>(p + i * n, n, kstep, pz, nv, trow + i, PS);
            for (; i < px; ++i) mosaic_lines<T, VEC, WIDE, 1>(p + i * n, n, kstep, pz, nv, trow + i, PS);
        }
    }
    __syncthreads();

    // ---- store: the tile in order, element t = v px + i of the run's part of output row(s) y py + j ----
    if (nvox > 0) {
        const int total = nvox * px;                                    // (a multiple of W)
        const int dv = (64 * W) / px, di = 64 * W - dv * px;            // t += 64 W
        int v = (lane * W) / px, i = lane * W - v * px;
        const long long orow = (long long)X * px;                       // output row length
        const long long ochan = n * py * px;                            // output channel (S > 0)
        const T zero = mz_zero<T>();
        const bool linear = PS == px;                                   // the tile has no gaps: one LDS read
        for (int t = lane * W; t < total; t += 64 * W) {
            const int f = f0 + v;
            const int y = f / X, x = f - y * X;
            const long long o = (((long long)z * Y + y) * py + j) * orow + (long long)x * px + i;
            MosaicPack<T, W> val, c0, c1, c2;
            if (W > 1 && linear) val = *(const MosaicPack<T, W> *)(tile + t);
            int ve = v, ie = i;
#pragma unroll
            for (int e = 0; e < W; ++e) {
                if (!(W > 1 && linear)) val.v[e] = tile[ve * PS + ie];
                if (S > 0) {
                    const int r = route[ve];
                    c0.v[e] = r == 0 ? val.v[e] : zero;
                    c1.v[e] = r == 1 ? val.v[e] : zero;
                    c2.v[e] = r == 2 ? val.v[e] : zero;
                }
                if (++ie == px) { ie = 0; ++ve; }
            }
            if (S == 0) {
                *(MosaicPack<T, W> *)(out + o) = val;
            } else {
                *(MosaicPack<T, W> *)(out + o) = c0;
                *(MosaicPack<T, W> *)(out + o + ochan) = c1;
                *(MosaicPack<T, W> *)(out + o + 2 * ochan) = c2;
            }
            v += dv;
            i += di;
            if (i >= px) { i -= px; ++v; }
        }
    }
}

template <typename T, int VEC, bool WIDE, int W>
hipError_t launch_mosaic_w(const T *in, const uint8_t *sel, int S, T *out, int tz, int Y, int X, int pz, int py, int px,
                           hipStream_t s) {
    constexpr int kRun = 64 * VEC;
    const int PS = px | 1;
    const int YX = Y * X, runs = (YX + kRun - 1) / kRun;
    const long long items = (long long)tz * py * runs, blocks = (items + kWaves - 1) / kWaves;
    PPP_GRID_CHECK(blocks, kBlock);
    const size_t lds = (size_t)kWaves * kRun * ((size_t)PS * sizeof(T) + 1);
    patch_mosaic_kernel<T, VEC, WIDE, W><<<dim3((unsigned)blocks), dim3(kBlock), lds, s>>>(in, sel, S, out, tz, Y, X, pz,
                                                                                          py, px, PS, runs, items);
    return hipGetLastError();
}

// the widest store the output allows: 16 bytes, else (2-byte elements) 4, else one element
template <typename T, int VEC, bool WIDE>
hipError_t launch_mosaic(const T *in, const uint8_t *sel, int S, T *out, int tz, int Y, int X, int pz, int py, int px,
                         hipStream_t s) {
    const long long orow = (long long)X * px;
    auto fits = [&](int w) { return orow % w == 0 && ((uintptr_t)out % (w * sizeof(T))) == 0; };
    constexpr int W16 = 16 / (int)sizeof(T);
    if (fits(W16)) return launch_mosaic_w<T, VEC, WIDE, W16>(in, sel, S, out, tz, Y, X, pz, py, px, s);
    if constexpr (sizeof(T) == 2) {
        if (fits(2)) return launch_mosaic_w<T, VEC, WIDE, 2>(in, sel, S, out, tz, Y, X, pz, py, px, s);
    }
    return launch_mosaic_w<T, VEC, WIDE, 1>(in, sel, S, out, tz, Y, X, pz, py, px, s);
}

}  // namespace

// The sizes a launch accepts: the tile below 2^31 voxels (the kernel's voxel index is an int), the output
// row and column counts too, px small enough for four LDS tiles of 128 voxels in 64 KiB, and a grid the
// device runs whole.  *why names the first limit that is exceeded.
bool patch_mosaic_supported(int tz, int Y, int X, int pz, int py, int px, const char **why) {
    (void)pz;
    const long long n = (long long)tz * Y * X;
    if (n >= (1ll << 31)) { *why = "z-tiles of 2^31 voxels or more"; return false; }
    if ((long long)Y * py >= (1ll << 31) || (long long)X * px >= (1ll << 31)) { *why = "output sides of 2^31 or more"; return false; }
    if (px > kMosaicMaxPx) { *why = "patches wider than 63 voxels"; return false; }
    // (the smaller run, 64 voxels, gives the larger grid)
    const long long runs = ((long long)Y * X + 63) / 64, blocks = ((long long)tz * py * runs + kWaves - 1) / kWaves;
    if (grid_too_big((unsigned long long)blocks, kBlock)) { *why = "z-tiles of more than 2^32 work-items"; return false; }
    return true;
}

// Does not synchronise.  sel: u8 [S][tz][Y][X] (S = 1 or 3) or null with S = 0; out: [tz][Y py][X px], or three
// such channels when S > 0.  Every element of `out` is written.
hipError_t run_patch_mosaic(const void *in, int dtype, const uint8_t *sel, int S, void *out, int tz, int Y, int X, int pz,
                            int py, int px, hipStream_t s) {
    const char *why = nullptr;
    if (!patch_mosaic_supported(tz, Y, X, pz, py, px, &why)) return hipErrorInvalidConfiguration;
    return with_pred_type(dtype, [&](auto tag) {
        using T = PPP_PRED_T(tag);
        if constexpr (sizeof(T) == 4) {
            return launch_mosaic<T, 1, true>((const T *)in, sel, S, (T *)out, tz, Y, X, pz, py, px, s);
        } else {
            const long long YX = (long long)Y * X;
            if (YX % 2 == 0 && ((uintptr_t)in & 3) == 0)        // (then tz YX, the channel stride, is even too)
                return launch_mosaic<T, 2, true>((const T *)in, sel, S, (T *)out, tz, Y, X, pz, py, px, s);
            return launch_mosaic<T, 2, false>((const T *)in, sel, S, (T *)out, tz, Y, X, pz, py, px, s);
        }
    });
}

}  // namespace ppp
