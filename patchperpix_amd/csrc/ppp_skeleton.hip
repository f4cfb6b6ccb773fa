// ppp_skeleton.hip -- the 3-d thinning behind `skeletonize_foreground` on the device: the result is, voxel
// for voxel, that of ppp_host_skeletonize_3d (ppp_host_skel.cpp; Lee / Kashyap / Chu 1994).
//
// WORKING IMAGE: one BIT per voxel, packed along x, with one empty voxel of padding all around: padded
// voxel (z, y, x), 0 <= x <= X + 1, is bit (x & 31) of word img[(z * pY + y) * W + (x >> 5)], pY = Y + 2,
// W = 2 * ceil((X + 2) / 64) words per row (even, so a wave of 64 lanes owns exactly two whole words of a
// row: lanes 0..31 the first, lanes 32..63 the second).  A second bit image of the same layout, `open`,
// marks the OPEN candidates of the running sub-iteration.  A 3x3x3 neighbourhood is nine row reads of one
// word each (two where x - 1 .. x + 1 straddles a word).
//
// A sub-iteration for border direction d (host order -y, +y, +x, -x, +z, -z):
//   candidates  one lane per padded voxel of a row: foreground, d-neighbour empty, removable
//               (ppp_skel_rule.hpp).  The wave's ballot IS the two `open` words it owns (a plain store by
//               lanes 0 and 32: nobody else writes these words in this launch) and compacts the voxels
//               into the open list (popcount below the lane, one atomicAdd per wave).
//   rounds      the host re-checks the candidates one at a time in raster order against the current image.
//               A re-check reads only the 26 neighbours and only candidates change, so a candidate's
//               verdict is fixed once no OPEN candidate is left among its 13 raster-preceding neighbours.
//               A round is two launches:
//                 partition  every open candidate reads the `open` bits of those 13 neighbours -- the state
//                            at the START of the round: this launch writes no `open` bit -- and goes to the
//                            READY list or to the next open list;
//                 decide     every ready candidate gathers its neighbourhood from the image, deletes itself
//                            when still removable (vector atomicAnd on the word: x and x + 2 can be ready
//                            together and share it) and leaves the open set either way (atomicAnd on the
//                            `open` word).  Two ready candidates are never 26-neighbours -- the later one
//                            would have had the earlier one open among its 13 -- so no verdict reads a bit
//                            this launch changes.
//               The raster-first open candidate is always ready: every round decides at least one.
//
// LAUNCH STRUCTURE: rounds are issued in batches of kBatch = 16 (32 launches) without a look at their
// result; list lengths live on the device (one counter slot per round of the batch), a launch whose list is
// empty returns at once, grids are sized by a host-side upper bound (the foreground count) and stride.  The
// host reads the counters back ONCE per batch: the open count after the batch, the rounds that had work, the
// deletions.  No launch waits for another workgroup.
//
// CAPACITY: a candidate for direction d is foreground with an empty d-neighbour, so two candidates are never
// adjacent along d's axis: at most ceil(n / 2) per line of n voxels.  The three lists (open, next open,
// ready) hold cap = max over the peeled axes of (V / n) * ceil(n / 2) entries each, about V / 2.
//
// LABELS (ppp_skeletonize_labels): every instance of a u32 id map thinned in the same launches; for every id L
// the result is that of ppp_host_skeletonize_3d(labels == L).  Instances are disjoint and a verdict of that
// thinning reads voxels of L only, so the sub-iterations run over the whole map at once with "neighbour
// present" = "alive AND of the centre's id": within an instance the same candidates are re-checked in the same
// raster order, and an instance at its fixed point loses nothing in the passes another one still needs.
// The mutable state stays the two bit images (`img`: label != 0).  One STATIC word per voxel, eq[v] (v the
// unpadded linear index), has bit n set when neighbour n lies inside the volume and carries v's id; one
// streaming pass over the labels fills it, and thinning never changes it (it clears alive bits only).  The
// neighbourhood word is gather27(img) & eq[v]; the border test reads the d-neighbour's bit of that word; the
// partition masks the 13 `open` bits with eq[v] too -- a candidate of another id changes no bit this verdict
// reads -- so touching instances do not serialise each other's rounds.  Ready candidates of DIFFERENT ids can
// then be 26-neighbours in one decide launch: neither reads the other's bit, and the word updates are
// atomicAnd.  A candidate's d-neighbour may be alive (of another id), so candidates can be adjacent along d's
// axis: the three lists hold V entries each.  The kernels are the binary ones: every body is a device function
// with the compile-time switch kLabels, and the binary kernels instantiate it with false (the strided loops'
// start and step come from the kernel, which is where the compiler folds the launch bounds into them).
#include "ppp_kernels.hpp"
#include "ppp_skel_rule.hpp"

namespace ppp {

namespace {

constexpr int kBatch = 16;           // rounds per counter read-back (even: the batch ends on list 0 again)
constexpr int kMaxBlocks = 2048;     // strided list kernels

struct SkelGeo {
    int Z, Y, X;
    int pY, W;                       // padded rows per slice, words per row
    long long YX;
};

__device__ __forceinline__ size_t row_word(const SkelGeo &G, int pz, int py) { return ((size_t)pz * G.pY + py) * G.W; }

// bits x - 1, x, x + 1 (padded x, 1 <= x <= X) of a row, as bits 0 .. 2
__device__ __forceinline__ uint32_t row3(const uint32_t *row, int x) {
    const int w = x >> 5, b = x & 31;
    const uint32_t v = row[w];
    if (b == 0) return (row[w - 1] >> 31) | ((v & 3u) << 1);
    if (b == 31) return (v >> 30) | ((row[w + 1] & 1u) << 2);
    return (v >> (b - 1)) & 7u;
}

// the 27-bit neighbourhood word of padded voxel (z, y, x), 1 <= z <= Z, 1 <= y <= Y, 1 <= x <= X
__device__ __forceinline__ uint32_t gather27(const uint32_t *img, const SkelGeo &G, int z, int y, int x) {
    uint32_t w = 0;
#pragma unroll
    for (int dz = 0; dz < 3; ++dz)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) w |= row3(img + row_word(G, z + dz - 1, y + dy - 1), x) << (dz * 9 + dy * 3);
    return w;
}

// bits 0 .. 12 of the neighbourhood word: the 13 raster-preceding neighbours
__device__ __forceinline__ uint32_t gather_before(const uint32_t *img, const SkelGeo &G, int z, int y, int x) {
    uint32_t w = 0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) w |= row3(img + row_word(G, z - 1, y + dy - 1), x) << (dy * 3);
    w |= row3(img + row_word(G, z, y - 1), x) << 9;
    w |= (row3(img + row_word(G, z, y), x) & 1u) << 12;
    return w;
}

}  // namespace

// One wave per 64 padded x of a row; block (64, 4): four rows.  grid (W / 2, ceil(Y / 4), Z).
// img words of the rows 1 .. Y of the slices 1 .. Z are written whole (the padding stays as the memset left it).
template <typename T>
__device__ __forceinline__ void skel_pack_body(const T *__restrict__ mask, uint32_t *__restrict__ img,
                                               uint32_t *__restrict__ n_fg, const SkelGeo G) {
    const int lane = threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, z = blockIdx.z;
    if (y >= G.Y) return;                                                  // (wave-uniform)
    const int px = blockIdx.x * 64 + lane;
    const bool on = px >= 1 && px <= G.X && mask[(size_t)z * G.YX + (size_t)y * G.X + (px - 1)] != 0;
    const unsigned long long m = __ballot(on);
    if ((lane & 31) == 0) img[row_word(G, z + 1, y + 1) + blockIdx.x * 2 + (lane >> 5)] = (uint32_t)(m >> (lane & 32));
    if (lane == 0 && m) atomicAdd(n_fg, (uint32_t)__popcll(m));
}
__global__ void __launch_bounds__(256)
    skel_pack_kernel(const uint8_t *__restrict__ mask, uint32_t *__restrict__ img, uint32_t *__restrict__ n_fg,
                     const SkelGeo G) {
    skel_pack_body(mask, img, n_fg, G);
}
__global__ void __launch_bounds__(256)
    skel_pack_labels_kernel(const uint32_t *__restrict__ labels, uint32_t *__restrict__ img, uint32_t *__restrict__ n_fg,
                            const SkelGeo G) {
    skel_pack_body(labels, img, n_fg, G);
}

__global__ void __launch_bounds__(256)
    skel_unpack_kernel(const uint32_t *__restrict__ img, uint8_t *__restrict__ out, const SkelGeo G) {
    const int y = blockIdx.y * 4 + threadIdx.y, z = blockIdx.z;
    const int px = blockIdx.x * 64 + threadIdx.x;
    if (y >= G.Y || px < 1 || px > G.X) return;
    const uint32_t w = img[row_word(G, z + 1, y + 1) + (px >> 5)];
    out[(size_t)z * G.YX + (size_t)y * G.X + (px - 1)] = (uint8_t)((w >> (px & 31)) & 1u);
}

// LABELS: out[v] = labels[v] where v is alive, else 0 (out may be labels: a thread reads and writes its own voxel)
__global__ void __launch_bounds__(256)
    skel_unpack_labels_kernel(const uint32_t *__restrict__ img, const uint32_t *labels, uint32_t *out, const SkelGeo G) {
    const int y = blockIdx.y * 4 + threadIdx.y, z = blockIdx.z;
    const int px = blockIdx.x * 64 + threadIdx.x;
    if (y >= G.Y || px < 1 || px > G.X) return;
    const uint32_t w = img[row_word(G, z + 1, y + 1) + (px >> 5)];
    const size_t v = (size_t)z * G.YX + (size_t)y * G.X + (px - 1);
    out[v] = ((w >> (px & 31)) & 1u) ? labels[v] : 0u;
}

// LABELS: the static word of every voxel.  One lane per UNPADDED voxel; block (64, 4), the grid of the pack
// kernel (it covers X + 2 >= X lanes per row).  Every index is checked against the volume before the read.
__global__ void __launch_bounds__(256)
    skel_eq_kernel(const uint32_t *__restrict__ labels, uint32_t *__restrict__ eq, const SkelGeo G) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, z = blockIdx.z;
    if (y >= G.Y || x >= G.X) return;
    const size_t v = (size_t)z * G.YX + (size_t)y * G.X + x;
    const uint32_t id = labels[v];
    uint32_t w = 0;
    if (id != 0u) {
#pragma unroll
        for (int dz = 0; dz < 3; ++dz) {
            const int zz = z + dz - 1;
            if (zz < 0 || zz >= G.Z) continue;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const int yy = y + dy - 1;
                if (yy < 0 || yy >= G.Y) continue;
                const uint32_t *row = labels + (size_t)zz * G.YX + (size_t)yy * G.X;
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int xx = x + dx - 1;
                    if (xx >= 0 && xx < G.X && row[xx] == id) w |= 1u << (dz * 9 + dy * 3 + dx);
                }
            }
        }
    }
    eq[v] = w;
}

// Candidates of one direction: (ez, ey, ex) is the neighbour that must be empty.  list entries are UNPADDED
// linear voxel indices (< 2^31).  *n_list must be 0 on entry; the `open` words this wave owns are all 0 on
// entry (every candidate of the sub-iteration before was decided).
// kLabels: eq is the static word of every voxel (else unused), and a d-neighbour of another id is empty too.
template <bool kLabels>
__device__ __forceinline__ void skel_candidates_body(const uint32_t *__restrict__ img, const uint32_t *__restrict__ eq,
                                                     uint32_t *__restrict__ open, uint32_t *__restrict__ list,
                                                     uint32_t *__restrict__ n_list, const int ez, const int ey,
                                                     const int ex, const SkelGeo G) {
    const int lane = threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, z = blockIdx.z;
    if (y >= G.Y) return;                                                  // (wave-uniform)
    const int px = blockIdx.x * 64 + lane;
    const size_t row = row_word(G, z + 1, y + 1);
    const uint32_t own = img[row + blockIdx.x * 2 + (lane >> 5)];
    bool cand = false;
    if (px >= 1 && px <= G.X && ((own >> (px & 31)) & 1u)) {
        const int bx = px + ex;
        const uint32_t nbw = img[row_word(G, z + 1 + ez, y + 1 + ey) + (bx >> 5)];
        if constexpr (kLabels) {
            const uint32_t same = eq[(size_t)z * G.YX + (size_t)y * G.X + (px - 1)];
            if (!(((nbw >> (bx & 31)) & 1u) && ((same >> ((ez + 1) * 9 + (ey + 1) * 3 + (ex + 1))) & 1u)))
                cand = ppp_skel::removable(gather27(img, G, z + 1, y + 1, px) & same);
        } else {
            if (!((nbw >> (bx & 31)) & 1u)) cand = ppp_skel::removable(gather27(img, G, z + 1, y + 1, px));
        }
    }
    const unsigned long long m = __ballot(cand);
    if (!m) return;
    if ((lane & 31) == 0) {
        const uint32_t half = (uint32_t)(m >> (lane & 32));
        if (half) open[row + blockIdx.x * 2 + (lane >> 5)] = half;
    }
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(n_list, (uint32_t)__popcll(m));
    base = __shfl(base, leader);
    if (cand) list[base + __popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)((size_t)z * G.YX + (size_t)y * G.X + (px - 1));
}
__global__ void __launch_bounds__(256)
    skel_candidates_kernel(const uint32_t *__restrict__ img, uint32_t *__restrict__ open, uint32_t *__restrict__ list,
                           uint32_t *__restrict__ n_list, const int ez, const int ey, const int ex, const SkelGeo G) {
    skel_candidates_body<false>(img, nullptr, open, list, n_list, ez, ey, ex, G);
}
__global__ void __launch_bounds__(256)
    skel_candidates_labels_kernel(const uint32_t *__restrict__ img, const uint32_t *__restrict__ eq,
                                  uint32_t *__restrict__ open, uint32_t *__restrict__ list, uint32_t *__restrict__ n_list,
                                  const int ez, const int ey, const int ex, const SkelGeo G) {
    skel_candidates_body<true>(img, eq, open, list, n_list, ez, ey, ex, G);
}

// counters of one batch: open[k] = open candidates at the start of round k (open[kBatch]: after the batch),
// ready[k] = candidates round k decides, deleted = voxels the batch deleted
struct SkelCounters {
    uint32_t open[kBatch + 1];
    uint32_t ready[kBatch];
    uint32_t deleted;
};

// round k, first launch.  n_known >= 0: the length of `in` (the host knows it); else counters->open[k].
// kLabels: only an open candidate of the same id blocks.
template <bool kLabels>
__device__ __forceinline__ void skel_partition_body(const uint32_t *__restrict__ open, const uint32_t *__restrict__ eq,
                                                    const uint32_t *__restrict__ in, uint32_t *__restrict__ next,
                                                    uint32_t *__restrict__ ready, SkelCounters *__restrict__ counters,
                                                    const int k, const long long n_known, const uint32_t first,
                                                    const uint32_t step, const SkelGeo G) {
    const uint32_t n = n_known >= 0 ? (uint32_t)n_known : counters->open[k];
    if (n_known >= 0 && blockIdx.x == 0 && threadIdx.x == 0) counters->open[k] = n;   // (for the read-back)
    const int lane = threadIdx.x & 63;
    // (wave-uniform trip count: the ballots see whole waves)
    for (uint32_t base = first; base < n; base += step) {
        const uint32_t i = base + lane;
        uint32_t v = 0;
        bool is_ready = false, blocked = false;
        if (i < n) {
            v = in[i];
            const int x = (int)(v % (uint32_t)G.X), y = (int)((v / (uint32_t)G.X) % (uint32_t)G.Y), z = (int)(v / (uint32_t)G.YX);
            if constexpr (kLabels) blocked = (gather_before(open, G, z + 1, y + 1, x + 1) & eq[v]) != 0u;
            else blocked = gather_before(open, G, z + 1, y + 1, x + 1) != 0u;
            is_ready = !blocked;
        }
        const unsigned long long mr = __ballot(is_ready), mb = __ballot(blocked);
        const unsigned long long below = (1ull << lane) - 1ull;
        uint32_t br = 0, bb = 0;
        if (lane == 0) {
            if (mr) br = atomicAdd(&counters->ready[k], (uint32_t)__popcll(mr));
            if (mb) bb = atomicAdd(&counters->open[k + 1], (uint32_t)__popcll(mb));
        }
        br = __shfl(br, 0);
        bb = __shfl(bb, 0);
        if (is_ready) ready[br + __popcll(mr & below)] = v;
        if (blocked) next[bb + __popcll(mb & below)] = v;
    }
}
__global__ void __launch_bounds__(256)
    skel_partition_kernel(const uint32_t *__restrict__ open, const uint32_t *__restrict__ in, uint32_t *__restrict__ next,
                          uint32_t *__restrict__ ready, SkelCounters *__restrict__ counters, const int k,
                          const long long n_known, const SkelGeo G) {
    skel_partition_body<false>(open, nullptr, in, next, ready, counters, k, n_known,
                               (blockIdx.x * blockDim.x + threadIdx.x) & ~63u, gridDim.x * blockDim.x, G);
}
__global__ void __launch_bounds__(256)
    skel_partition_labels_kernel(const uint32_t *__restrict__ open, const uint32_t *__restrict__ eq,
                                 const uint32_t *__restrict__ in, uint32_t *__restrict__ next, uint32_t *__restrict__ ready,
                                 SkelCounters *__restrict__ counters, const int k, const long long n_known, const SkelGeo G) {
    skel_partition_body<true>(open, eq, in, next, ready, counters, k, n_known,
                              (blockIdx.x * blockDim.x + threadIdx.x) & ~63u, gridDim.x * blockDim.x, G);
}

// round k, second launch: the verdicts
template <bool kLabels>
__device__ __forceinline__ void skel_decide_body(uint32_t *img, uint32_t *open, const uint32_t *__restrict__ eq,
                                                 const uint32_t *__restrict__ ready, SkelCounters *__restrict__ counters,
                                                 const int k, const uint32_t first, const uint32_t step, const SkelGeo G) {
    const uint32_t n = counters->ready[k];
    const int lane = threadIdx.x & 63;
    for (uint32_t base = first; base < n; base += step) {
        const uint32_t i = base + lane;
        bool gone = false;
        if (i < n) {
            const uint32_t v = ready[i];
            const int x = (int)(v % (uint32_t)G.X) + 1, y = (int)((v / (uint32_t)G.X) % (uint32_t)G.Y) + 1, z = (int)(v / (uint32_t)G.YX) + 1;
            if constexpr (kLabels) gone = ppp_skel::removable(gather27(img, G, z, y, x) & eq[v]);
            else gone = ppp_skel::removable(gather27(img, G, z, y, x));
            const size_t word = row_word(G, z, y) + (x >> 5);
            const uint32_t keep = ~(1u << (x & 31));
            if (gone) atomicAnd(&img[word], keep);
            atomicAnd(&open[word], keep);            // decided: out of the open set, deleted or not
        }
        const unsigned long long m = __ballot(gone);
        if (m && lane == 0) atomicAdd(&counters->deleted, (uint32_t)__popcll(m));
    }
}
__global__ void __launch_bounds__(256)
    skel_decide_kernel(uint32_t *img, uint32_t *open, const uint32_t *__restrict__ ready,
                       SkelCounters *__restrict__ counters, const int k, const SkelGeo G) {
    skel_decide_body<false>(img, open, nullptr, ready, counters, k, (blockIdx.x * blockDim.x + threadIdx.x) & ~63u,
                            gridDim.x * blockDim.x, G);
}
__global__ void __launch_bounds__(256)
    skel_decide_labels_kernel(uint32_t *img, uint32_t *open, const uint32_t *__restrict__ eq,
                              const uint32_t *__restrict__ ready, SkelCounters *__restrict__ counters, const int k,
                              const SkelGeo G) {
    skel_decide_body<true>(img, open, eq, ready, counters, k, (blockIdx.x * blockDim.x + threadIdx.x) & ~63u,
                           gridDim.x * blockDim.x, G);
}

struct SkelWork {
    uint32_t *img, *open;            // [img_words] each
    uint32_t *list[2], *ready;       // [cap] each
    SkelCounters *counters;
    uint32_t *eq;                    // labels: [Z * Y * X]; else nullptr
    size_t img_words, cap;
};
static SkelWork skel_layout(Carver &c, int Z, int Y, int X, bool labels) {
    SkelWork W;
    const size_t words = 2 * (((size_t)X + 2 + 63) / 64);
    W.img_words = ((size_t)Z + 2) * ((size_t)Y + 2) * words;
    const size_t V = (size_t)Z * Y * X;
    const size_t by_y = V / Y * (((size_t)Y + 1) / 2), by_x = V / X * (((size_t)X + 1) / 2);
    const size_t by_z = Z > 1 ? V / Z * (((size_t)Z + 1) / 2) : 0;     // a single slice peels no z border
    W.cap = by_y > by_x ? by_y : by_x;
    if (by_z > W.cap) W.cap = by_z;
    if (labels) W.cap = V;           // a d-neighbour of another id is alive: candidates can be adjacent along d
    W.img = c.take<uint32_t>(W.img_words);
    W.open = c.take<uint32_t>(W.img_words);
    W.list[0] = c.take<uint32_t>(W.cap);
    W.list[1] = c.take<uint32_t>(W.cap);
    W.ready = c.take<uint32_t>(W.cap);
    W.counters = (SkelCounters *)c.take_bytes(sizeof(SkelCounters));
    W.eq = labels ? c.take<uint32_t>(V) : nullptr;
    return W;
}
size_t skeleton_workspace_bytes(int Z, int Y, int X) { Carver c(nullptr); skel_layout(c, Z, Y, X, false); return c.used; }
size_t skeleton_labels_workspace_bytes(int Z, int Y, int X) { Carver c(nullptr); skel_layout(c, Z, Y, X, true); return c.used; }

// The thinning of a mask (kLabels = false: In = Out = uint8_t) or of every instance of an id map (kLabels = true:
// In = Out = uint32_t).  out may be in.  stats: passes, sub-iterations, rounds that had work.  Synchronises.
template <bool kLabels, typename T>
static hipError_t skel_run(const T *in, T *out, int Z, int Y, int X, long long *n_kept, int *stats, void *work,
                           hipStream_t s) {
    static_assert(kBatch % 2 == 0, "a batch must end on the list it began with");
    SkelGeo G;
    G.Z = Z; G.Y = Y; G.X = X;
    G.pY = Y + 2;
    G.W = 2 * (int)(((long long)X + 2 + 63) / 64);
    G.YX = (long long)Y * X;
    Carver carver(work);
    const SkelWork W = skel_layout(carver, Z, Y, X, kLabels);
    const dim3 block(64, 4), grid((unsigned)(G.W / 2), (unsigned)((Y + 3) / 4), (unsigned)Z);
    if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidConfiguration;
    hipError_t e;
    if ((e = hipMemsetAsync(W.img, 0, W.img_words * 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.open, 0, W.img_words * 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(W.counters, 0, sizeof(SkelCounters), s)) != hipSuccess) return e;
    // (the `deleted` slot serves as the foreground count here)
    if constexpr (kLabels) {
        skel_pack_labels_kernel<<<grid, block, 0, s>>>(in, W.img, &W.counters->deleted, G);
        skel_eq_kernel<<<grid, block, 0, s>>>(in, W.eq, G);
    } else {
        skel_pack_kernel<<<grid, block, 0, s>>>(in, W.img, &W.counters->deleted, G);
    }
    uint32_t n_fg = 0;
    if ((e = hipMemcpyAsync(&n_fg, &W.counters->deleted, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;

    // border directions in the host's order: the neighbour that must be empty, as (dz, dy, dx)
    static const int DIRS[6][3] = {{0, -1, 0}, {0, 1, 0}, {0, 0, 1}, {0, 0, -1}, {1, 0, 0}, {-1, 0, 0}};
    const int n_dirs = Z > 1 ? 6 : 4;
    long long alive = n_fg;
    int unchanged = 0;
    stats[0] = stats[1] = stats[2] = 0;
    SkelCounters h;
    while (unchanged < n_dirs) {
        unchanged = 0;
        ++stats[0];
        for (int d = 0; d < n_dirs; ++d) {
            ++stats[1];
            long long n_open = -1;          // -1: the candidates kernel leaves it in counters->open[0]
            uint32_t deleted = 0;
            while (n_open != 0) {
                // candidates <= foreground voxels (and <= cap); later batches know their list length
                const long long bound = n_open < 0 ? (alive < (long long)W.cap ? alive : (long long)W.cap) : n_open;
                long long nb = (bound + 255) / 256;
                const dim3 lgrid((unsigned)(nb < 1 ? 1 : (nb > kMaxBlocks ? kMaxBlocks : nb)));
                if ((e = hipMemsetAsync(W.counters, 0, sizeof(SkelCounters), s)) != hipSuccess) return e;
                if (n_open < 0) {
                    if constexpr (kLabels)
                        skel_candidates_labels_kernel<<<grid, block, 0, s>>>(W.img, W.eq, W.open, W.list[0], &W.counters->open[0],
                                                                             DIRS[d][0], DIRS[d][1], DIRS[d][2], G);
                    else
                        skel_candidates_kernel<<<grid, block, 0, s>>>(W.img, W.open, W.list[0], &W.counters->open[0],
                                                                      DIRS[d][0], DIRS[d][1], DIRS[d][2], G);
                }
                for (int k = 0; k < kBatch; ++k) {
                    if constexpr (kLabels) {
                        skel_partition_labels_kernel<<<lgrid, dim3(256), 0, s>>>(W.open, W.eq, W.list[k & 1], W.list[(k + 1) & 1],
                                                                                 W.ready, W.counters, k, k == 0 ? n_open : -1ll, G);
                        skel_decide_labels_kernel<<<lgrid, dim3(256), 0, s>>>(W.img, W.open, W.eq, W.ready, W.counters, k, G);
                    } else {
                        skel_partition_kernel<<<lgrid, dim3(256), 0, s>>>(W.open, W.list[k & 1], W.list[(k + 1) & 1], W.ready,
                                                                          W.counters, k, k == 0 ? n_open : -1ll, G);
                        skel_decide_kernel<<<lgrid, dim3(256), 0, s>>>(W.img, W.open, W.ready, W.counters, k, G);
                    }
                }
                if ((e = hipGetLastError()) != hipSuccess) return e;
                if ((e = hipMemcpyAsync(&h, W.counters, sizeof(SkelCounters), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
                if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
                for (int k = 0; k < kBatch; ++k) {
                    if (h.open[k] == 0) break;
                    // every round decides the raster-first open candidate at least
                    if (h.ready[k] == 0 || h.open[k + 1] + h.ready[k] != h.open[k] || h.open[k] > W.cap) return hipErrorUnknown;
                    ++stats[2];
                }
                deleted += h.deleted;
                n_open = h.open[kBatch];
            }
            alive -= deleted;
            if (deleted == 0) ++unchanged;
        }
    }
    if constexpr (kLabels) skel_unpack_labels_kernel<<<grid, block, 0, s>>>(W.img, in, out, G);
    else skel_unpack_kernel<<<grid, block, 0, s>>>(W.img, out, G);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    *n_kept = alive;
    return hipSuccess;
}

hipError_t run_skeletonize_3d(const uint8_t *mask, uint8_t *out, int Z, int Y, int X, long long *n_kept, int *stats,
                              void *work, hipStream_t s) {
    return skel_run<false>(mask, out, Z, Y, X, n_kept, stats, work, s);
}

// every instance of the id map at once; out may be labels
hipError_t run_skeletonize_labels(const uint32_t *labels, uint32_t *out, int Z, int Y, int X, long long *n_kept, int *stats,
                                  void *work, hipStream_t s) {
    return skel_run<true>(labels, out, Z, Y, X, n_kept, stats, work, s);
}

}  // namespace ppp
