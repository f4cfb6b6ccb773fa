// ppp_edt.hip -- the exact squared Euclidean distance transform of a (Z, Y, X) volume, in integers.
//
//   d2[v] = min over feature voxels w of |v - w|^2            (0xFFFFFFFF: the volume holds no feature)
//
// The squared distance separates over the axes: three passes x -> y -> z, each
//   out[i] = min_j (in[j] + (i - j)^2)                       along its axis,
// the x pass starting from 0 at a feature voxel and infinity elsewhere.
//
// A pass is an EXPANDING WINDOW: best = in[i], then the two terms at distance k = 1, 2, ... while
// k^2 < best.  A term at distance k is at least k^2, so nothing beyond the stop can lower the minimum:
// the result is exact.  Every voxel is an independent thread with no per-lane stack, and in all three
// passes the lanes of a wave run along x, so a step reads two coalesced rows.  The cost per voxel is its
// distance along the axis: under a cap (best starts at min(in[i], cap), so k <= ceil(sqrt(cap))) that is
// bounded; without a cap it is the sum of the distances, worse than a stack algorithm's O(n) per line
// on a nearly empty volume -- accepted, the consumer in this library (ppp_post_fg_filter) always caps.
//
// 0xFFFFFFFF is infinity and is never added to; a sum is never formed before it is known to be below
// `best` (t < best and k^2 < best - t), so nothing wraps whatever the cap.
#include "ppp_kernels.hpp"

namespace ppp {

namespace {

constexpr uint32_t kInf = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t edt_load(const uint8_t *__restrict__ in, long long i) { return in[i] ? 0u : kInf; }
__device__ __forceinline__ uint32_t edt_load(const uint32_t *__restrict__ in, long long i) { return in[i]; }

// One pass along the axis of `n` elements and element stride `stride`; v is the voxel's linear index,
// pos its coordinate on the axis.  T = uint8_t: the x pass over the feature mask; uint32_t: y and z.
template <typename T>
__global__ void __launch_bounds__(256)
    edt_pass_kernel(const T *__restrict__ in, uint32_t *__restrict__ out, const long long V, const long long stride,
                    const int n, const uint32_t cap) {
    const long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int pos = (int)((v / stride) % n);
    uint32_t best = edt_load(in, v);
    if (cap != 0u && best > cap) best = cap;
    // (n <= 65535: k * k fits 32 bits)
    for (uint32_t k = 1; k * k < best && ((int)k <= pos || pos + (int)k < n); ++k) {
        const uint32_t k2 = k * k;
        if ((int)k <= pos) {
            const uint32_t t = edt_load(in, v - (long long)k * stride);
            if (t < best && k2 < best - t) best = t + k2;
        }
        if (pos + (int)k < n) {
            const uint32_t t = edt_load(in, v + (long long)k * stride);
            if (t < best && k2 < best - t) best = t + k2;
        }
    }
    out[v] = best;
}

}  // namespace

EdtWork edt_layout(Carver &c, long long V) {
    EdtWork W;
    W.tmp = c.take<uint32_t>((size_t)V);
    return W;
}
size_t post_edt_workspace_bytes(long long V) { Carver c(nullptr); edt_layout(c, V); return c.used; }

// feature -> out (x), out -> tmp (y), tmp -> out (z).  Does not synchronise.
hipError_t launch_edt_sq(const uint8_t *feature, uint32_t *out, int Z, int Y, int X, uint32_t cap, const EdtWork &W,
                         hipStream_t s) {
    const long long YX = (long long)Y * X, V = YX * Z;
    PPP_GRID_CHECK((V + 255) / 256, 256);
    const dim3 block(256), grid((unsigned)((V + 255) / 256));
    edt_pass_kernel<uint8_t><<<grid, block, 0, s>>>(feature, out, V, 1, X, cap);
    edt_pass_kernel<uint32_t><<<grid, block, 0, s>>>(out, W.tmp, V, X, Y, cap);
    edt_pass_kernel<uint32_t><<<grid, block, 0, s>>>(W.tmp, out, V, YX, Z, cap);
    return hipGetLastError();
}

hipError_t run_post_edt_sq(const uint8_t *feature, uint32_t *out, int Z, int Y, int X, uint32_t cap, void *work,
                           hipStream_t s) {
    Carver carver(work);
    const EdtWork W = edt_layout(carver, (long long)Z * Y * X);
    return launch_edt_sq(feature, out, Z, Y, X, cap, W, s);
}

}  // namespace ppp
