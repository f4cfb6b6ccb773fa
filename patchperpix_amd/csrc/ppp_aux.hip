// ppp_aux.hip -- small helpers around the hot path: the patch bits of the greedy cover and the
// thinning (per centre, and for every voxel of a volume), the "clean" check S1 picks its
// classification by, the procedural synthetic prediction generator used by bench / tests, and the
// counter calibration kernels.  The bit kernels and the check each read the prediction on their
// own; on the resident single box of cubic 5 / 7 / 9 patches one pass serves all of them and S2's
// masks (ppp_prepass.hip), and these kernels serve every other path and geometry.
#include "ppp_kernels.hpp"

namespace ppp {

// ---- patch bits: bit r of centre k = (pred[r][c_k] > thresh) ---------------------------
// One wave per centre; lane l handles channels l, l+64, ...; a ballot packs 64 bits at a
// time (two uint32 words), so the only global traffic is the C channel values.
template <typename T>
__global__ void __launch_bounds__(256)
    patch_bits_kernel(const T *__restrict__ pred, const uint32_t *__restrict__ centres, uint64_t n,
                      float thresh, uint32_t *__restrict__ bits, const Geo G) {
    const uint64_t k = (uint64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    if (k >= n) return;
    const int lane = threadIdx.x & 63;
    const int words = (G.C + 31) / 32;
    const long long lc = vox(G, (int)centres[k * 3], (int)centres[k * 3 + 1], (int)centres[k * 3 + 2]);
    for (int base = 0; base < G.C; base += 64) {
        const int r = base + lane;
        const bool on = r < G.C && ldf(pred, (long long)r * G.V + lc) > thresh;
        const unsigned long long m = __ballot(on);
        if (lane == 0) {
            bits[k * words + base / 32] = (uint32_t)m;
            if (base / 32 + 1 < words) bits[k * words + base / 32 + 1] = (uint32_t)(m >> 32);
        }
    }
}

hipError_t launch_patch_bits(const void *pred, int dtype, const uint32_t *centres, uint64_t n,
                             float thresh, uint32_t *bits, const Geo &G, hipStream_t s) {
    // a wave per centre: at most 2^24 centres per launch (64 work-items each; grid limit 2^32)
    const int words = (G.C + 31) / 32;
    for (uint64_t k0 = 0; k0 < n; k0 += (1ull << 24)) {
        const uint64_t m = n - k0 < (1ull << 24) ? n - k0 : (1ull << 24);
        const dim3 grid((unsigned)((m + 3) / 4));
        const hipError_t e = with_pred_type(dtype, [&](auto tag) {
            using T = PPP_PRED_T(tag);
            patch_bits_kernel<T><<<grid, dim3(256), 0, s>>>((const T *)pred, centres + k0 * 3, m, thresh, bits + k0 * words, G);
            return hipSuccess;
        });
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

// The same bits for EVERY voxel of the volume, bits_vol u32[V][words]: thread per voxel (lanes
// along x: every channel plane is read once, coalesced).  The wave-per-centre kernel above
// touches one cache line per (centre, channel) -- 48 GB for the 2.2 M cover candidates of the
// 140^3 benchmark; this one reads the 1.9 GB prediction once and the caller gathers the rows of
// its centres.
template <typename T>
__global__ void __launch_bounds__(256)
    patch_bits_volume_kernel(const T *__restrict__ pred, float thresh, uint32_t *__restrict__ bits_vol,
                             const Geo G) {
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= G.V) return;
    const int words = (G.C + 31) / 32;
    int r = 0;
    for (int w = 0; w < words; ++w) {
        uint32_t m = 0;
        for (int b = 0; b < 32 && r < G.C; ++b, ++r)
            m |= (ldf(pred, (long long)r * G.V + v) > thresh ? 1u : 0u) << b;
        bits_vol[v * words + w] = m;
    }
}

hipError_t launch_patch_bits_volume(const void *pred, int dtype, float thresh, uint32_t *bits_vol,
                                    const Geo &G, hipStream_t s) {
    PPP_GRID_CHECK((G.V + 255) / 256, 256);
    const dim3 grid((unsigned)((G.V + 255) / 256));
    return with_pred_type(dtype, [&](auto tag) {
        using T = PPP_PRED_T(tag);
        patch_bits_volume_kernel<T><<<grid, dim3(256), 0, s>>>((const T *)pred, thresh, bits_vol, G);
        return hipGetLastError();
    });
}

// ---- synthetic prediction (patchperpix_amd/synth.py::pred_from_labels) ------------------
__device__ __forceinline__ uint32_t hash_u32(uint32_t x) {
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}

template <typename T>
__global__ void __launch_bounds__(256)
    synth_kernel(const int32_t *__restrict__ labels, T *__restrict__ pred, uint32_t seed_mix,
                 float hi, float lo, float noise, unsigned long long voxel_offset, const Geo G) {
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= G.V) return;
    const int r = blockIdx.y;
    const int x = (int)(v % G.X);
    const long long t = v / G.X;
    const int y = (int)(t % G.Y), z = (int)(t / G.Y);
    const int nz = z + r / (G.py * G.px) - G.rz;
    const int ny = y + (r / G.px) % G.py - G.ry;
    const int nx = x + r % G.px - G.rx;
    const int lab = labels[v];
    int nb = -1;
    if (nz >= 0 && nz < G.Z && ny >= 0 && ny < G.Y && nx >= 0 && nx < G.X) nb = labels[vox(G, nz, ny, nx)];
    const float base = (nb == lab && lab != 0) ? hi : lo;
    // counter = lin * C + r + seed_mix   (mod 2^32, like the uint64 NumPy code masked to 32 bit)
    // counter of the GLOBAL voxel, so a slab of a larger volume gets the same values
    const uint32_t ctr = (uint32_t)(((unsigned long long)v + voxel_offset) * (unsigned long long)G.C +
                                    (unsigned long long)r + (unsigned long long)seed_mix);
    const float u = (float)(hash_u32(ctr) >> 8) * (1.0f / 16777216.0f);
    const float val = base + noise * (2.0f * u - 1.0f);
    const __half h = __float2half_rn(val);  // through float16, like the zarr on disk
    static_assert(std::is_same<T, __half>::value || std::is_same<T, float>::value, "the generator writes float16 / float32");
    if constexpr (std::is_same<T, __half>::value) pred[(long long)r * G.V + v] = h;
    else pred[(long long)r * G.V + v] = __half2float(h);
}

// The same generator for a BOX of a larger volume (tile-wise generation: a rank of the 1024^3
// workload never holds more than one tile + halo of the prediction).  pred: (C, bz, by, bx) for
// the box at G.oz / oy / ox (G.Z / Y / X = box extent); labels: an int32 array over the label box
// lb = (z0, y0, x0, z1, y1, x1) that holds the box grown by the patch radius (clipped to the
// volume gdim); the noise counter is that of the GLOBAL voxel: bit-identical to generating the
// whole volume at once.
template <typename T>
__global__ void __launch_bounds__(256)
    synth_box_kernel(const int32_t *__restrict__ labels, T *__restrict__ pred, uint32_t seed_mix,
                     float hi, float lo, float noise, const int lz0, const int ly0, const int lx0,
                     const int lY, const int lX, const int gZ, const int gY, const int gX, const Geo G) {
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= G.V) return;
    const int r = blockIdx.y;
    const int x = (int)(v % G.X) + G.ox;
    const long long t = v / G.X;
    const int y = (int)(t % G.Y) + G.oy, z = (int)(t / G.Y) + G.oz;
    const int nz = z + r / (G.py * G.px) - G.rz;
    const int ny = y + (r / G.px) % G.py - G.ry;
    const int nx = x + r % G.px - G.rx;
    auto lab_at = [&](int gz, int gy, int gx) -> int {
        return labels[((long long)(gz - lz0) * lY + (gy - ly0)) * lX + (gx - lx0)];
    };
    const int lab = lab_at(z, y, x);
    int nb = -1;
    if (nz >= 0 && nz < gZ && ny >= 0 && ny < gY && nx >= 0 && nx < gX) nb = lab_at(nz, ny, nx);
    const float base = (nb == lab && lab != 0) ? hi : lo;
    const unsigned long long glin = ((unsigned long long)z * gY + y) * gX + x;
    const uint32_t ctr = (uint32_t)(glin * (unsigned long long)G.C + (unsigned long long)r + (unsigned long long)seed_mix);
    const float u = (float)(hash_u32(ctr) >> 8) * (1.0f / 16777216.0f);
    const float val = base + noise * (2.0f * u - 1.0f);
    const __half h = __float2half_rn(val);
    static_assert(std::is_same<T, __half>::value || std::is_same<T, float>::value, "the generator writes float16 / float32");
    if constexpr (std::is_same<T, __half>::value) pred[(long long)r * G.V + v] = h;
    else pred[(long long)r * G.V + v] = __half2float(h);
}

hipError_t launch_synth_box(const int32_t *labels, const int *lb, void *pred, int dtype, uint32_t seed,
                            float hi, float lo, float noise, const int *gdim, const Geo &G, hipStream_t s) {
    PPP_GRID_CHECK((G.V + 255) / 256, 256);
    const dim3 grid((unsigned)((G.V + 255) / 256), (unsigned)G.C);
    const uint32_t seed_mix = (uint32_t)(((unsigned long long)seed * 0x9E3779B1ull) & 0xFFFFFFFFull);
    const int lY = lb[4] - lb[1], lX = lb[5] - lb[2];
    return with_f32_f16_type(dtype, [&](auto tag) {
        using T = PPP_PRED_T(tag);
        synth_box_kernel<T><<<grid, dim3(256), 0, s>>>(labels, (T *)pred, seed_mix, hi, lo, noise,
                                                       lb[0], lb[1], lb[2], lY, lX, gdim[0], gdim[1], gdim[2], G);
        return hipGetLastError();
    });
}

hipError_t launch_synth(const int32_t *labels, void *pred, int dtype, uint32_t seed, float hi,
                        float lo, float noise, unsigned long long voxel_offset, const Geo &G,
                        hipStream_t s) {
    PPP_GRID_CHECK((G.V + 255) / 256, 256);
    const dim3 grid((unsigned)((G.V + 255) / 256), (unsigned)G.C);
    const uint32_t seed_mix = (uint32_t)(((unsigned long long)seed * 0x9E3779B1ull) & 0xFFFFFFFFull);
    return with_f32_f16_type(dtype, [&](auto tag) {
        using T = PPP_PRED_T(tag);
        synth_kernel<T><<<grid, dim3(256), 0, s>>>(labels, (T *)pred, seed_mix, hi, lo, noise, voxel_offset, G);
        return hipGetLastError();
    });
}

// ---- counter calibration (bench / profiles only) ---------------------------------------------
// MI355X_MICROARCH.md: FETCH_SIZE / WRITE_SIZE are exact only for some access widths; "calibrate
// on a known byte count in your own access pattern".  These two kernels move a KNOWN number of
// bytes with the widths of the hot kernels' global accesses -- one element of the prediction's
// type per lane and load (S1's staging loads), one float per lane and store -- so that a PMC pass
// that contains them yields the counter / true-bytes ratios next to the kernels' raw values.
template <typename T>
__global__ void __launch_bounds__(256)
    calib_read_kernel(const T *__restrict__ src, const long long n, float *__restrict__ sink) {
    float acc = 0.0f;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        acc += ldf(src, i);
    if (acc == 123456.789f) sink[0] = acc;          // keeps the loads alive; practically never taken
}
__global__ void __launch_bounds__(256) calib_write_kernel(float *__restrict__ dst, const long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dst[i] = (float)(i & 1023);
}
hipError_t launch_counter_calibration(const void *src, int dtype, long long n_read, float *dst, long long n_write,
                                      hipStream_t s) {
    const dim3 grid(256 * 32), block(256);
    if (n_read > 0) {
        const hipError_t e = with_f32_f16_type(dtype, [&](auto tag) {
            using T = PPP_PRED_T(tag);
            calib_read_kernel<T><<<grid, block, 0, s>>>((const T *)src, n_read, dst);
            return hipSuccess;
        });
        if (e != hipSuccess) return e;
    }
    if (n_write > 0) calib_write_kernel<<<grid, block, 0, s>>>(dst, n_write);
    return hipGetLastError();
}

// ---- ppp_pred_check: is the prediction "clean" for S1's short classification? -------------------
// One streaming pass (16-byte loads) over a contiguous prediction buffer: *unclean |= 1 when a value
// lies outside [0, 1] as a bit pattern (negative, -0, > 1, inf, nan), |= 2 when a value is neither
// > TH nor < BG (with the shipped rule: exactly 0.5 -- an operand that votes nowhere,
// fillConsensusArray.cu:44-47, 94-124).
template <typename T> struct PredBits;
template <> struct PredBits<__half> {
    static constexpr int PER16 = 8;
    static __device__ __forceinline__ unsigned bits(unsigned short h) { return h; }
    static constexpr unsigned ONE = 0x3C00u;
    static __device__ __forceinline__ float val(unsigned short h) { return (float)__builtin_bit_cast(_Float16, h); }
};
template <> struct PredBits<bf16_t> {
    static constexpr int PER16 = 8;
    static __device__ __forceinline__ unsigned bits(unsigned short h) { return h; }
    static constexpr unsigned ONE = 0x3F80u;
    static __device__ __forceinline__ float val(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
};
template <typename T>
__device__ __forceinline__ unsigned pred_check_one(float v, unsigned bits, unsigned one, float th_gt, float bg_lt) {
    return (bits > one ? 1u : 0u) | ((!(v > th_gt) && !(v < bg_lt)) ? 2u : 0u);
}
template <typename T>
__global__ void __launch_bounds__(256)
    pred_check_kernel(const T *__restrict__ src, const long long n, const float th_gt, const float bg_lt,
                      int *__restrict__ unclean) {
    unsigned bad = 0u;
    const long long tid = blockIdx.x * (long long)blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
    if constexpr (std::is_same<T, __half>::value || std::is_same<T, bf16_t>::value) {
        // head up to the first 16-byte boundary, body as uint4, tail
        const long long head = min(n, (long long)(((16 - ((uintptr_t)src & 15)) & 15) / 2));
        const unsigned short *s16 = reinterpret_cast<const unsigned short *>(src);
        for (long long i = tid; i < head; i += nth) bad |= pred_check_one<T>(PredBits<T>::val(s16[i]), s16[i], PredBits<T>::ONE, th_gt, bg_lt);
        const long long nv = (n - head) / 8;
        const uint4 *s128 = reinterpret_cast<const uint4 *>(s16 + head);
        for (long long i = tid; i < nv; i += nth) {
            const uint4 q = s128[i];
            const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned short a = (unsigned short)(w[k] & 0xFFFFu), b = (unsigned short)(w[k] >> 16);
                bad |= pred_check_one<T>(PredBits<T>::val(a), a, PredBits<T>::ONE, th_gt, bg_lt);
                bad |= pred_check_one<T>(PredBits<T>::val(b), b, PredBits<T>::ONE, th_gt, bg_lt);
            }
        }
        for (long long i = head + nv * 8 + tid; i < n; i += nth) bad |= pred_check_one<T>(PredBits<T>::val(s16[i]), s16[i], PredBits<T>::ONE, th_gt, bg_lt);
    } else {
        static_assert(std::is_same<T, float>::value, "pred_check_kernel: float32, float16 or bfloat16");
        const long long head = min(n, (long long)(((16 - ((uintptr_t)src & 15)) & 15) / 4));
        const unsigned *s32 = reinterpret_cast<const unsigned *>(src);
        for (long long i = tid; i < head; i += nth) bad |= pred_check_one<T>(__uint_as_float(s32[i]), s32[i], 0x3F800000u, th_gt, bg_lt);
        const long long nv = (n - head) / 4;
        const uint4 *s128 = reinterpret_cast<const uint4 *>(s32 + head);
        for (long long i = tid; i < nv; i += nth) {
            const uint4 q = s128[i];
            const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) bad |= pred_check_one<T>(__uint_as_float(w[k]), w[k], 0x3F800000u, th_gt, bg_lt);
        }
        for (long long i = head + nv * 4 + tid; i < n; i += nth) bad |= pred_check_one<T>(__uint_as_float(s32[i]), s32[i], 0x3F800000u, th_gt, bg_lt);
    }
    if (__ballot(bad != 0u) != 0ull) {
        for (int o = 32; o > 0; o >>= 1) bad |= (unsigned)__shfl_xor((int)bad, o);
        if ((threadIdx.x & 63) == 0) atomicOr(unclean, (int)bad);
    }
}
hipError_t launch_pred_check(const void *pred, int dtype, long long n, const Geo &G, int *unclean, hipStream_t s) {
    hipError_t e = hipMemsetAsync(unclean, 0, sizeof(int), s);
    if (e != hipSuccess || n <= 0) return e;
    const dim3 grid(256 * 16), block(256);
    return with_pred_type(dtype, [&](auto tag) {
        using T = PPP_PRED_T(tag);
        pred_check_kernel<T><<<grid, block, 0, s>>>((const T *)pred, n, G.th_gt, G.bg_lt, unclean);
        return hipGetLastError();
    });
}

}  // namespace ppp
