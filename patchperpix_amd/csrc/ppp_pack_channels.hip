// ppp_pack_channels.hip -- `no_overlap_per_channel` (graph_to_labeling.py:57-115) without the loop
// over components: sizes and overlapping label pairs in one device pass, and the paint by channel.
//
// The closed form.  Component k (label k + 1, k = 0 .. K-1, in component order) has the mask M_k =
// the union over its patches of the window voxels whose patch value is > patch_threshold, clipped
// to the volume; n_k = |M_k|.  The reference paints every component into a volume of its own and
// places it:
//     component 0                       -> channel 0
//     n_k <= 2000 (n_k = 0 included)    -> channel 0, painted over whatever is there
//     n_k >  2000                       -> the first channel in which no voxel of M_k is non-zero,
//                                          a new channel when there is none
// (1) Overwrites keep voxels non-zero, so a channel's non-zero set before step k is the union of the
//     masks placed there earlier: component k conflicts with channel c exactly when some j < k with
//     chan[j] == c has M_j and M_k intersecting.
// (2) The assignment therefore needs only the sizes n_k and the set of overlapping label pairs
//     (j < k): a greedy walk over a small graph (ppp_host_pack_channels, ppp_host_pack.cpp).
// (3) Given chan[], channel c holds at voxel v the LARGEST label among the components of channel c
//     that cover v (large components of one channel never overlap; in channel 0 the later component
//     overwrites): one "largest label wins" paint with a channel offset per label
//     (paint_channels_kernel).
//
// The pass (scatter work n_nodes x C like paint_kernel, never a p^3 gather over every voxel):
//     L1[v]  = largest covering label                        (launch_paint)
//     Lc[c]  = label of the node centred on c, else 0        (scatter_centres_kernel)
//     flag[v] = 1 where a covering label is < L1[v]          (flag_kernel, a plain store)
//     sweep over the OWN voxels: size[L1[v]] += 1 with runs merged inside a wave; flagged voxels
//     compacted into a list by ballot                        (sweep_kernel)
//     peel, one wave per listed voxel: the lanes stride over the C window offsets r, the centre is
//     c = v - off(r); it covers v when it is in bounds, Lc[c] != 0 and pred[r][c] > TH.  below(b) =
//     the largest covering label < b.  Count: every label found below L1[v] adds 1 to its size, a
//     voxel of m labels announces m (m - 1) / 2 pairs.  Fill (after an exclusive scan): for every
//     covering b, from the top, every covering a < b is found by an inner peel and (a, b) is
//     written -- no per-voxel storage, no cap on how many components meet in one voxel.
// Pair keys are (b << 32) | a with a < b; a pair comes out once per shared voxel, the caller
// dedupes.  A tile counts only its own voxels (the `own` box) and reads centres from its frame.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "ppp_kernels.hpp"

namespace ppp {

namespace {

constexpr int kMaxBlocks = 4096;

struct PackWork {
    uint32_t *L1, *Lc;         // [V]
    uint8_t *flag;             // [V]
    uint32_t *list;            // [own voxels]
    long long *cnt, *off;      // [own voxels + 1]
    unsigned long long *n_list;
    void *temp;
    size_t temp_bytes;
    long long cap;
};
PackWork pack_layout(Carver &c, const Geo &G, long long own_voxels) {
    PackWork W;
    W.cap = own_voxels;
    W.L1 = c.take<uint32_t>((size_t)G.V);
    W.Lc = c.take<uint32_t>((size_t)G.V);
    W.flag = c.take<uint8_t>((size_t)G.V);
    W.list = c.take<uint32_t>((size_t)own_voxels);
    W.cnt = c.take<long long>((size_t)own_voxels + 1);
    W.off = c.take<long long>((size_t)own_voxels + 1);
    W.n_list = (unsigned long long *)c.take_bytes(256);
    size_t tb = 0;
    (void)rocprim::exclusive_scan(nullptr, tb, (long long *)nullptr, (long long *)nullptr, 0ll, (size_t)own_voxels + 1,
                                  rocprim::plus<long long>(), (hipStream_t)0);
    W.temp_bytes = up256(tb);
    W.temp = c.take_bytes(W.temp_bytes);
    return W;
}

}  // namespace

size_t pack_scan_workspace_bytes(const Geo &G, const ppp_box &own) {
    Carver c(nullptr);
    pack_layout(c, G, (long long)(own.z1 - own.z0) * (own.y1 - own.y0) * (own.x1 - own.x0));
    return c.used;
}

__global__ void __launch_bounds__(256)
    scatter_centres_kernel(const uint32_t *__restrict__ nodes, const uint32_t *__restrict__ labels, const uint64_t n,
                           uint32_t *__restrict__ Lc, const Geo G) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t lab = labels[k];
    if (lab == 0) return;
    const int cz = (int)nodes[k * 3], cy = (int)nodes[k * 3 + 1], cx = (int)nodes[k * 3 + 2];
    if (cz < 0 || cz >= G.Z || cy < 0 || cy >= G.Y || cx < 0 || cx >= G.X) return;
    Lc[vox(G, cz, cy, cx)] = lab;
}

// the paint's thread per (node, pixel): a painted pixel whose label lost against L1 marks its voxel
template <typename T>
__global__ void __launch_bounds__(256)
    flag_kernel(const T *__restrict__ pred, const uint32_t *__restrict__ nodes, const uint32_t *__restrict__ labels,
                const uint64_t n, const uint32_t *__restrict__ L1, uint8_t *__restrict__ flag, const float th_f32,
                const Geo G) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * (uint64_t)G.C) return;
    const uint64_t k = t / G.C;
    const int r = (int)(t % G.C);
    const uint32_t lab = labels[k];
    if (lab == 0) return;
    const int cz = (int)nodes[k * 3], cy = (int)nodes[k * 3 + 1], cx = (int)nodes[k * 3 + 2];
    if (cz < 0 || cz >= G.Z || cy < 0 || cy >= G.Y || cx < 0 || cx >= G.X) return;
    if (!(ldf(pred, (long long)r * G.V + vox(G, cz, cy, cx)) > th_f32)) return;
    const int z = cz + r / (G.py * G.px) - G.rz;
    const int y = cy + (r / G.px) % G.py - G.ry;
    const int x = cx + r % G.px - G.rx;
    if (z < 0 || z >= G.Z || y < 0 || y >= G.Y || x < 0 || x >= G.X) return;
    const long long v = vox(G, z, y, x);
    if (lab < L1[v]) flag[v] = 1;
}

// One thread per own voxel, x fastest.  Neighbouring voxels share labels: a lane is a run HEAD when
// its label differs from the lane before it (lane 0 always is), and only a head adds -- the distance
// to the next head of the wave -- to the size table.  Flagged voxels go to the list, one atomic per
// wave.  (No lane leaves before the ballots.)
__global__ void __launch_bounds__(256)
    sweep_kernel(const uint32_t *__restrict__ L1, const uint8_t *__restrict__ flag, const ppp_box own,
                 const long long n_own, const uint32_t n_labels, unsigned long long *__restrict__ sizes,
                 uint32_t *__restrict__ list, unsigned long long *__restrict__ n_list, const long long cap,
                 const Geo G) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int oY = own.y1 - own.y0, oX = own.x1 - own.x0;
    uint32_t lab = 0;
    bool f = false;
    long long v = 0;
    if (i < n_own) {
        const int x = own.x0 + (int)(i % oX), y = own.y0 + (int)((i / oX) % oY), z = own.z0 + (int)(i / ((long long)oX * oY));
        v = vox(G, z, y, x);
        lab = L1[v];
        f = flag[v] != 0;
    }
    const uint32_t prev = __shfl_up(lab, 1);
    const bool head = lane == 0 || lab != prev;
    const unsigned long long H = __ballot(head);
    if (head && lab != 0 && lab <= n_labels) {
        const unsigned long long later = lane == 63 ? 0ull : H & (~0ull << (lane + 1));
        const int nxt = later ? __ffsll((long long)later) - 1 : 64;
        atomicAdd(&sizes[lab], (unsigned long long)(nxt - lane));
    }
    const unsigned long long F = __ballot(f);
    if (F) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(n_list, (unsigned long long)__popcll(F));
        base = __shfl(base, 0);
        if (f) {
            const long long at = (long long)base + __popcll(F & ((1ull << lane) - 1ull));
            if (at < cap) list[at] = (uint32_t)v;
        }
    }
}

// the largest label < bound among the components that cover voxel (z, y, x); 0 when there is none.
// Whole-wave call: every lane gets the result.
template <typename T>
__device__ __forceinline__ uint32_t below(const T *__restrict__ pred, const uint32_t *__restrict__ Lc, const int z,
                                          const int y, const int x, const uint32_t bound, const float th_f32,
                                          const int lane, const Geo &G) {
    uint32_t best = 0;
    for (int r = lane; r < G.C; r += 64) {
        const int cz = z - (r / (G.py * G.px) - G.rz);
        const int cy = y - ((r / G.px) % G.py - G.ry);
        const int cx = x - (r % G.px - G.rx);
        if (cz < 0 || cz >= G.Z || cy < 0 || cy >= G.Y || cx < 0 || cx >= G.X) continue;
        const long long c = vox(G, cz, cy, cx);
        const uint32_t l = Lc[c];
        if (l == 0 || l >= bound || l <= best) continue;
        if (ldf(pred, (long long)r * G.V + c) > th_f32) best = l;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = __shfl_xor(best, d);
        best = o > best ? o : best;
    }
    return best;
}

template <typename T, bool FILL>
__global__ void __launch_bounds__(256)
    peel_kernel(const T *__restrict__ pred, const uint32_t *__restrict__ Lc, const uint32_t *__restrict__ L1,
                const uint32_t *__restrict__ list, const long long n_list, const uint32_t n_labels,
                unsigned long long *__restrict__ sizes, long long *__restrict__ cnt, const long long *__restrict__ off,
                unsigned long long *__restrict__ pairs, const long long n_pairs, const float th_f32, const Geo G) {
    const int lane = threadIdx.x & 63;
    const long long wave = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = (gridDim.x * (long long)blockDim.x) >> 6;
    for (long long item = wave; item < n_list; item += nwaves) {      // (wave-uniform trip count)
        const long long v = (long long)list[item];
        const int x = (int)(v % G.X), y = (int)((v / G.X) % G.Y), z = (int)(v / ((long long)G.X * G.Y));
        const uint32_t top = L1[v];
        if (!FILL) {
            long long m = 1;
            for (uint32_t a = below(pred, Lc, z, y, x, top, th_f32, lane, G); a != 0;
                 a = below(pred, Lc, z, y, x, a, th_f32, lane, G)) {
                ++m;
                if (lane == 0 && a <= n_labels) atomicAdd(&sizes[a], 1ull);
            }
            if (lane == 0) cnt[item] = m * (m - 1) / 2;
        } else {
            long long out = off[item];
            for (uint32_t b = top; b != 0; b = below(pred, Lc, z, y, x, b, th_f32, lane, G))
                for (uint32_t a = below(pred, Lc, z, y, x, b, th_f32, lane, G); a != 0;
                     a = below(pred, Lc, z, y, x, a, th_f32, lane, G)) {
                    if (lane == 0 && out < n_pairs) pairs[out] = ((unsigned long long)b << 32) | a;
                    ++out;
                }
        }
    }
}

static unsigned wave_blocks(long long items) {
    const long long b = (items + 3) / 4;
    return (unsigned)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

// sizes[label] += voxels of the own box the label covers; *n_pairs = pair keys run_pack_scan_fill will
// write (one per pair and shared own voxel).  Synchronises.  The workspace carries L1, Lc, the list and
// its offsets to the fill.
hipError_t run_pack_scan_count(const void *pred, int dtype, const uint32_t *nodes, const uint32_t *labels, uint64_t n_nodes,
                               uint32_t n_labels, const ppp_box &own, unsigned long long *sizes, long long *n_pairs,
                               void *work, const Geo &G, hipStream_t s) {
    const long long n_own = (long long)(own.z1 - own.z0) * (own.y1 - own.y0) * (own.x1 - own.x0);
    Carver carver(work);
    const PackWork W = pack_layout(carver, G, n_own);
    hipError_t e;
    *n_pairs = 0;
    if ((e = hipMemsetAsync(W.L1, 0, (size_t)G.V * 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.Lc, 0, (size_t)G.V * 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.flag, 0, (size_t)G.V, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.n_list, 0, 8, s)) != hipSuccess) return e;
    if (n_nodes == 0 || n_own == 0) return hipStreamSynchronize(s);
    if ((e = launch_paint(pred, dtype, nodes, labels, n_nodes, W.L1, G, s)) != hipSuccess) return e;
    PPP_GRID_CHECK((n_nodes + 255) / 256, 256);
    scatter_centres_kernel<<<dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, s>>>(nodes, labels, n_nodes, W.Lc, G);
    const uint64_t per = ((1ull << 31) / (uint64_t)G.C) & ~255ull;      // chunks below the 2^32 grid limit, as the paint
    for (uint64_t k0 = 0; k0 < n_nodes; k0 += per) {
        const uint64_t m = n_nodes - k0 < per ? n_nodes - k0 : per;
        const dim3 grid((unsigned)((m * (uint64_t)G.C + 255) / 256));
        {
            const hipError_t e_ = with_pred_type(dtype, [&](auto tag) {
                using T = PPP_PRED_T(tag);
                flag_kernel<T><<<grid, dim3(256), 0, s>>>((const T *)pred, nodes + k0 * 3, labels + k0, m, W.L1, W.flag, G.th_rn, G);
                return hipSuccess;
            });
            if (e_ != hipSuccess) return e_;
        }
    }
    PPP_GRID_CHECK((n_own + 255) / 256, 256);
    sweep_kernel<<<dim3((unsigned)((n_own + 255) / 256)), dim3(256), 0, s>>>(W.L1, W.flag, own, n_own, n_labels, sizes, W.list,
                                                                             W.n_list, W.cap, G);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    unsigned long long n_list = 0;
    if ((e = hipMemcpyAsync(&n_list, W.n_list, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    if ((long long)n_list > W.cap) return hipErrorInvalidValue;       // (cannot happen: a voxel is listed once)
    if (n_list == 0) return hipSuccess;
    {
        const hipError_t e_ = with_pred_type(dtype, [&](auto tag) {
            using T = PPP_PRED_T(tag);
            peel_kernel<T, false><<<dim3(wave_blocks((long long)n_list)), dim3(256), 0, s>>>( (const T *)pred, W.Lc, W.L1, W.list, (long long)n_list, n_labels, sizes, W.cnt, nullptr, nullptr, 0, G.th_rn, G);
            return hipSuccess;
        });
        if (e_ != hipSuccess) return e_;
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.cnt + n_list, 0, 8, s)) != hipSuccess) return e;
    size_t tb = W.temp_bytes;
    if ((e = rocprim::exclusive_scan(W.temp, tb, W.cnt, W.off, 0ll, (size_t)n_list + 1, rocprim::plus<long long>(), s)) != hipSuccess)
        return e;
    long long total = 0;
    if ((e = hipMemcpyAsync(&total, W.off + n_list, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    *n_pairs = total;
    return hipSuccess;
}

// after run_pack_scan_count on the same workspace, prediction and box: pairs[0 .. n_pairs) written
hipError_t run_pack_scan_fill(const void *pred, int dtype, const ppp_box &own, unsigned long long *pairs, long long n_pairs,
                              void *work, const Geo &G, hipStream_t s) {
    if (n_pairs == 0) return hipSuccess;
    Carver carver(work);
    const PackWork W = pack_layout(carver, G, (long long)(own.z1 - own.z0) * (own.y1 - own.y0) * (own.x1 - own.x0));
    hipError_t e;
    unsigned long long n_list = 0;
    long long total = 0;
    if ((e = hipMemcpyAsync(&n_list, W.n_list, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    if (n_list == 0 || (long long)n_list > W.cap) return hipErrorInvalidValue;
    if ((e = hipMemcpyAsync(&total, W.off + n_list, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    if (total != n_pairs) return hipErrorInvalidValue;               // not the workspace of the count
    {
        const hipError_t e_ = with_pred_type(dtype, [&](auto tag) {
            using T = PPP_PRED_T(tag);
            peel_kernel<T, true><<<dim3(wave_blocks((long long)n_list)), dim3(256), 0, s>>>( (const T *)pred, W.Lc, W.L1, W.list, (long long)n_list, 0u, nullptr, nullptr, W.off, pairs, n_pairs, G.th_rn, G);
            return hipSuccess;
        });
        if (e_ != hipSuccess) return e_;
    }
    return hipGetLastError();
}

// ---- paint by channel: paint_kernel with out[chan[label]][v] ------------------------------------
template <typename T>
__global__ void __launch_bounds__(256)
    paint_channels_kernel(const T *__restrict__ pred, const uint32_t *__restrict__ nodes,
                          const uint32_t *__restrict__ labels, const uint64_t n, const uint32_t *__restrict__ chan,
                          const uint32_t n_labels, const uint32_t n_channels, uint32_t *out, const float th_f32,
                          const Geo G) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * (uint64_t)G.C) return;
    const uint64_t k = t / G.C;
    const int r = (int)(t % G.C);
    const uint32_t lab = labels[k];
    if (lab == 0 || lab > n_labels) return;
    const uint32_t ch = chan[lab];
    if (ch >= n_channels) return;
    const int cz = (int)nodes[k * 3], cy = (int)nodes[k * 3 + 1], cx = (int)nodes[k * 3 + 2];
    if (cz < 0 || cz >= G.Z || cy < 0 || cy >= G.Y || cx < 0 || cx >= G.X) return;
    if (!(ldf(pred, (long long)r * G.V + vox(G, cz, cy, cx)) > th_f32)) return;
    const int z = cz + r / (G.py * G.px) - G.rz;
    const int y = cy + (r / G.px) % G.py - G.ry;
    const int x = cx + r % G.px - G.rx;
    if (z < 0 || z >= G.Z || y < 0 || y >= G.Y || x < 0 || x >= G.X) return;
    atomicMax(&out[(long long)ch * G.V + vox(G, z, y, x)], lab);
}

hipError_t launch_paint_channels(const void *pred, int dtype, const uint32_t *nodes, const uint32_t *labels, uint64_t n,
                                 const uint32_t *chan, uint32_t n_labels, uint32_t n_channels, uint32_t *out,
                                 const Geo &G, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t per = ((1ull << 31) / (uint64_t)G.C) & ~255ull;
    for (uint64_t k0 = 0; k0 < n; k0 += per) {
        const uint64_t m = n - k0 < per ? n - k0 : per;
        const dim3 grid((unsigned)((m * (uint64_t)G.C + 255) / 256));
        {
            const hipError_t e_ = with_pred_type(dtype, [&](auto tag) {
                using T = PPP_PRED_T(tag);
                paint_channels_kernel<T><<<grid, dim3(256), 0, s>>>((const T *)pred, nodes + k0 * 3, labels + k0, m, chan, n_labels, n_channels, out, G.th_rn, G);
                return hipSuccess;
            });
            if (e_ != hipSuccess) return e_;
        }
    }
    return hipGetLastError();
}

}  // namespace ppp
