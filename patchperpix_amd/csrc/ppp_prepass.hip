// ppp_prepass.hip -- ONE read of the prediction for everything that is a compare of its values against a
// threshold: the "clean" flag S1 picks its classification by (ppp_pred_check), S2's interleaved masks, pair
// counts and border / background scores (rank_masks_il_kernel), and the cover's per-voxel patch bits
// (patch_bits_volume_kernel).  Each of those kernels streams the whole tensor on its own; here a value is
// loaded once and compared four times.
//
// pred_prepass_kernel<T, P>: a workgroup of 256 threads owns 256 consecutive voxels (lanes along x: every
// channel plane is read coalesced, base pointer in scalar registers, lane offset = the thread's number).  The
// channels are walked in chunks of 64 -- one quad of mask words, two words of patch bits -- and within a chunk
// in four batches of 16 independent loads (plus, for a foreground interior centre, the 16 partners' bytes of
// `valid`, which rank_valid2_kernel wrote one launch earlier: partner r of centre v is voxel v + a constant,
// so those loads are coalesced too).  All bit positions are compile-time constants; the chunk number is the
// only run-time index, and it only addresses memory.
//   * M: a centre's quad leaves as ONE 16-byte store; the 16 x-neighbours of a mask row write 256 contiguous
//     bytes.
//   * bits_vol: a voxel's row (11 words at 7^3) is collected in LDS and the workgroup's 256 rows -- contiguous
//     in memory -- are copied out with 16-byte stores.
//   * unclean: the largest bit pattern and an "in the dead zone" flag per lane, one atomicOr per wave that saw
//     something.
// patch_bits_from_table_kernel copies the rows of a centre list out of bits_vol (the thinning's centres).
#include "ppp_kernels.hpp"
#include "ppp_rank_masks.hpp"

namespace ppp {

// the raw element (what the range test looks at) and its float32 value
template <typename T> struct PreVal;
template <> struct PreVal<__half> {
    typedef unsigned short raw_t;
    static constexpr unsigned ONE = 0x3C00u;
    static __device__ __forceinline__ float val(unsigned h) { return (float)__builtin_bit_cast(_Float16, (unsigned short)h); }
};
template <> struct PreVal<bf16_t> {
    typedef unsigned short raw_t;
    static constexpr unsigned ONE = 0x3F80u;
    static __device__ __forceinline__ float val(unsigned h) { return __uint_as_float(h << 16); }
};
template <> struct PreVal<float> {
    typedef unsigned raw_t;
    static constexpr unsigned ONE = 0x3F800000u;
    static __device__ __forceinline__ float val(unsigned w) { return __uint_as_float(w); }
};

static constexpr int PRE_THREADS = 256;

template <typename T, int P>
__global__ void __launch_bounds__(PRE_THREADS)
    pred_prepass_kernel(const typename PreVal<T>::raw_t *__restrict__ pred, const uint8_t *__restrict__ valid_v,
                        const ppp_box sb, const float fc_thresh, uint32_t *__restrict__ M, uint32_t *__restrict__ info,
                        float *__restrict__ score, uint32_t *__restrict__ bits_vol, int *__restrict__ unclean, const Geo G) {
    constexpr int R = P / 2, C = P * P * P, WORDS = (C + 31) / 32, CHUNKS = (C + 63) / 64, NW16 = (C + 15) / 16;
    static_assert(CHUNKS == rw_mask_words(C) / 4, "64 channels are one quad of mask words");
    static_assert(NW16 == 2 * WORDS, "the 16-bit pieces of a voxel's patch bits fill its words");
    __shared__ __attribute__((aligned(16))) uint32_t rows[PRE_THREADS * WORDS];

    const int tid = threadIdx.x;
    const long long v0 = (long long)blockIdx.x * PRE_THREADS, v = v0 + tid;
    const bool inb = v < G.V;
    int x = 0, y = 0, z = 0;
    if (inb) {
        x = (int)(v % G.X);
        const long long zy = v / G.X;
        y = (int)(zy % G.Y), z = (int)(zy / G.Y);
    }
    const int sX = sb.x1 - sb.x0, sY = sb.y1 - sb.y0;
    const bool in_sb = inb && x >= sb.x0 && x < sb.x1 && y >= sb.y0 && y < sb.y1 && z >= sb.z0 && z < sb.z1;
    const bool inter = in_sb && interior(G, z, y, x);
    // (only a foreground interior centre of the score box has masks: the others never load `valid`)
    const bool active = inter && PreVal<T>::val(pred[(long long)G.mid * G.V + v]) > G.th_gt;
    long long t = 0, q0 = 0;
    if (in_sb) {
        const long long line = (long long)(z - sb.z0) * sY + (y - sb.y0);
        t = line * sX + (x - sb.x0);
        q0 = rw_mask_quad0(line, x - sb.x0, sX, CHUNKS);
    }

    // Channel r of this workgroup's voxels is plane[lane] with a uniform, WALKED base (a lane past the volume reads
    // voxel v0 and drops what it makes of it).  Partner r = (dz, dy, dx) of centre v is voxel v + o(r),
    // o(r) = ((dz - R) Y + (dy - R)) X + dx - R: read at vlow[tid + u], vlow = valid + v0 + o(0) uniform and
    // u = o(r) - o(0) >= 0 walked in 32 bits (pred_prepass_supported bounds it) -- no division, no 64-bit lane
    // arithmetic.  Only foreground interior centres read `valid`: one branch per batch, a wave of background skips it.
    const typename PreVal<T>::raw_t *plane = pred + v0;
    const int lane = inb ? tid : 0;
    const uint8_t *vlow = valid_v + (v0 - (((long long)R * G.Y + R) * G.X + R));
    const unsigned x_wrap = (unsigned)(G.X - P + 1), y_wrap = (unsigned)(G.Y - P) * (unsigned)G.X + x_wrap;
    unsigned u = 0u;
    int dx = 0, dy = 0;
    unsigned mx = 0u, nP = 0u, nV = 0u;
    uint32_t dead = 0u;
    uint32_t m0 = 0u, m1 = 0u, m2 = 0u, m3 = 0u;
    unsigned short *rows16 = reinterpret_cast<unsigned short *>(rows);
    // channels [16 c, 16 c + N)
    auto batch = [&](const int c, auto n_tag) {
        constexpr int N = decltype(n_tag)::value;
        unsigned raw[N], ok[N], uo[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            raw[j] = plane[lane];
            plane += G.V;
            uo[j] = u;
            ++dx;
            u += dx == P ? (dy + 1 == P ? y_wrap : x_wrap) : 1u;
            dy = dx == P ? (dy + 1 == P ? 0 : dy + 1) : dy;
            dx = dx == P ? 0 : dx;
            ok[j] = 0u;
        }
        if (active) {
#pragma unroll
            for (int j = 0; j < N; ++j) ok[j] = vlow[uo[j] + (unsigned)tid];
        }
        // the four compares of a value, each into bit j of its own word (`valid` holds 0 / 1: rank_valid2_kernel)
        uint32_t g = 0u, l = 0u, f = 0u, vb = 0u;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float val = PreVal<T>::val(raw[j]);
            mx = raw[j] > mx ? raw[j] : mx;
            g |= (val > G.th_gt ? 1u : 0u) << j;
            l |= (val < G.bg_lt ? 1u : 0u) << j;
            f |= (val > fc_thresh ? 1u : 0u) << j;
            vb |= ok[j] << j;
        }
        dead |= ~(g | l) & ((1u << N) - 1u);
        const uint32_t w = interleave16(g & vb, l & vb);
        nV += __popc(vb);
        nP += __popc(g & vb);
        rows16[tid * (2 * WORDS) + c] = (unsigned short)f;
        // a quad of mask words leaves as one 16-byte store (the last quad's missing words are zero)
        const int k = c & 3;
        m0 = k == 0 ? w : m0; m1 = k == 1 ? w : m1; m2 = k == 2 ? w : m2; m3 = k == 3 ? w : m3;
        if (k == 3 || c == NW16 - 1) {
            if (active) reinterpret_cast<uint4 *>(M)[q0 + (long long)(c >> 2) * RW_QSTRIDE] = make_uint4(m0, m1, m2, m3);
            m0 = m1 = m2 = m3 = 0u;
        }
    };
#pragma unroll 1
    for (int c = 0; c < C / 16; ++c) batch(c, std::integral_constant<int, 16>{});
    if constexpr (C % 16 != 0) batch(C / 16, std::integral_constant<int, C % 16>{});

    // ---- the clean flag, bits as ppp_pred_check
    unsigned bad = inb ? ((mx > PreVal<T>::ONE ? 1u : 0u) | (dead != 0u ? 2u : 0u)) : 0u;
    if (__ballot(bad != 0u) != 0ull) {
        for (int o = 32; o > 0; o >>= 1) bad |= (unsigned)__shfl_xor((int)bad, o);
        if ((tid & 63) == 0) atomicOr(unclean, (int)bad);
    }

    // ---- pair count; the scores that need no consensus
    if (in_sb) {
        uint32_t inf = 0u;
        if (!inter) {
            score[v] = G.norm_rank ? -1.0f : -9999999.0f;
        } else if (!active) {
            score[v] = 0.0f;   // the reference leaves the allocation's zero
        } else {
            // fgCnt = |P| (|V| - 1) - |P| (|P| - 1) / 2   (rankPatches.cu:139, see ppp_rank_v2.hip)
            const unsigned fg_cnt = nP ? nP * (nV - 1u) - nP * (nP - 1u) / 2u : 0u;
            inf = 0x80000000u | fg_cnt;
            if (nP == 0u) score[v] = 0.0f;   // no first pixel: acc = 0, 0 / max(1, 0)
        }
        info[t] = inf;
    }

    // ---- the workgroup's patch-bit rows: contiguous in bits_vol
    __syncthreads();
    const long long left = G.V - v0;
    const int n_words = (int)(left < PRE_THREADS ? left : PRE_THREADS) * WORDS;
    uint32_t *dst = bits_vol + v0 * WORDS;
    if (n_words == PRE_THREADS * WORDS && ((uintptr_t)bits_vol & 15) == 0) {
        // (v0 * WORDS * 4 is a multiple of 16: v0 is a multiple of 256)
        for (int i = tid; i < PRE_THREADS * WORDS / 4; i += PRE_THREADS)
            reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(rows)[i];
    } else {
        for (int i = tid; i < n_words; i += PRE_THREADS) dst[i] = rows[i];
    }
}

bool pred_prepass_supported(const Geo &G) {
    // what the kernel compiles in, and only where the ranking kernel that reads its masks serves the call
    Geo Gv = G;
    Gv.layout = PPP_CONS_VOXEL_MAJOR;
    // (the partner offsets of a workgroup's 256 voxels, walked from the lowest one, stay below 2^31)
    const long long span = (long long)(G.px - 1) * ((long long)G.Y * G.X + G.X + 1) + PRE_THREADS;
    return rank_wg_supported(Gv) && !G.ring && span < (1LL << 31);
}

PrepassWork pred_prepass_layout(Carver &c, const ppp_box &sb, const Geo &G) {
    PrepassWork W;
    const RankMasks m = rank_masks_layout(c, sb, G);     // first: launch_rank_wg_prepared carves the same
    W.M = m.M; W.info = m.info; W.valid = m.valid;
    W.bits_vol = c.take<uint32_t>((size_t)G.V * ((G.C + 31) / 32));
    W.unclean = c.take<int32_t>(1);
    return W;
}
size_t pred_prepass_workspace_bytes(const ppp_box &sb, const Geo &G) { Carver c(nullptr); pred_prepass_layout(c, sb, G); return c.used; }

template <typename T>
static hipError_t launch_prepass_t(const void *pred, float fc_thresh, float *score, const ppp_box &sb,
                                   const PrepassWork &W, const Geo &G, hipStream_t s) {
    typedef typename PreVal<T>::raw_t raw_t;
    const dim3 grid((unsigned)((G.V + PRE_THREADS - 1) / PRE_THREADS));
#define PPP_PRE_CASE(P)                                                                                       \
    case P:                                                                                                   \
        pred_prepass_kernel<T, P><<<grid, dim3(PRE_THREADS), 0, s>>>((const raw_t *)pred, W.valid, sb, fc_thresh, W.M, W.info, \
                                                                     score, W.bits_vol, W.unclean, G);        \
        break;
    switch (G.px) {
        PPP_PRE_CASE(5)
        PPP_PRE_CASE(7)
        PPP_PRE_CASE(9)
    default:
        return hipErrorNotSupported;
    }
#undef PPP_PRE_CASE
    return hipGetLastError();
}

hipError_t launch_pred_prepass(const void *pred, int dtype, const uint8_t *ov, float fc_thresh, float *score,
                               const ppp_box &sb, void *work, const Geo &G, hipStream_t s) {
    if (!pred_prepass_supported(G)) return hipErrorNotSupported;
    PPP_GRID_CHECK((G.V + PRE_THREADS - 1) / PRE_THREADS, PRE_THREADS);
    Carver carver(work);
    const PrepassWork W = pred_prepass_layout(carver, sb, G);
    hipError_t e = hipMemsetAsync(W.unclean, 0, sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    // (the partners' validity first, one channel: recomputing it per partner cost 1.6 ms in round 12)
    e = launch_rank_valid(pred, dtype, ov, W.valid, G, s);
    if (e != hipSuccess) return e;
    return with_pred_type(dtype, [&](auto tag) {
        using T = PPP_PRED_T(tag);
        return launch_prepass_t<T>(pred, fc_thresh, score, sb, W, G, s);
    });
}

// ---- rows of a centre list out of the per-voxel table ---------------------------------------------------------
// thread per (centre, word): a centre's words are neighbouring lanes, its row one or two cache lines
__global__ void __launch_bounds__(256)
    patch_bits_from_table_kernel(const uint32_t *__restrict__ bits_vol, const uint32_t *__restrict__ centres,
                                 const unsigned long long n_items, const int words, uint32_t *__restrict__ bits, const Geo G) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const unsigned long long k = i / (unsigned)words;
    const int w = (int)(i - k * (unsigned)words);
    const long long lc = vox(G, (int)centres[k * 3], (int)centres[k * 3 + 1], (int)centres[k * 3 + 2]);
    bits[i] = bits_vol[lc * words + w];
}

hipError_t launch_patch_bits_from_table(const uint32_t *bits_vol, const uint32_t *centres, uint64_t n, uint32_t *bits,
                                        const Geo &G, hipStream_t s) {
    const int words = (G.C + 31) / 32;
    const unsigned long long n_items = (unsigned long long)n * words;
    PPP_GRID_CHECK((n_items + 255) / 256, 256);
    patch_bits_from_table_kernel<<<dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, s>>>(bits_vol, centres, n_items, words, bits, G);
    return hipGetLastError();
}

}  // namespace ppp
