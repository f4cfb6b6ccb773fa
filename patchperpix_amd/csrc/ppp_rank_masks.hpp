// ppp_rank_masks.hpp -- the layout of S2's two-bit masks, shared by the kernel that reads them
// (ppp_rank_wg.hip), its own pre-pass, and the fused pre-pass over the prediction (ppp_prepass.hip).
#pragma once
#include "ppp_common.hpp"

namespace ppp {

// Mask words per centre, padded to whole 16-byte loads.  The masks are stored CENTRE-MAJOR,
// M[centre][word]: a lane reads the 184 bytes of ITS centre with twelve 16-byte loads, and the
// centres of a wave's chunk (9-runs of x neighbours) cover their cache lines densely.  The earlier
// word-major layout M[word][centre] made each of the 46 loads of a chunk touch eight 128-byte lines
// for 36 bytes apiece: 47 KB of line traffic per chunk for 11.8 KB of masks -- and because a
// workgroup's masks (377 KB) are re-read on every one of the 729 steps while 128 workgroups per
// XCD share a 4 MB L2, most of those lines came over the fabric (the kernel ran at the fabric's
// bandwidth: profiles/r04_b_s2_ablations.txt -- 205 ms, 126 ms without the mask loads).
static constexpr int rw_mask_words(int C) { return (((C + 15) / 16) + 3) & ~3; }
// Round 5: the two-bit masks in ROWS OF 16 X-NEIGHBOURS, M[row][quad of words][centre in row][4 words]:
// the 16-byte load of quad q by the nine x-neighbours of a run touches 144 contiguous bytes (two or
// three lines) instead of nine lines 184 bytes apart -- the bytes fetched stay the same, the
// addresses the vector cache has to look up per load fall to a quarter.
// index (in 16-byte units) of quad 0 of the centre at x of line zy (score-box coordinates)
__host__ __device__ __forceinline__ long long rw_mask_quad0(long long zy, int x, int sX, int quads) {
    return ((zy * ((sX + 15) >> 4) + (x >> 4)) * quads) * 16 + (x & 15);
}
static constexpr int RW_QSTRIDE = 16;      // 16-byte units between a centre's quads
static inline size_t rw_mask_bytes(int sZ, int sY, int sX, int C) {
    const size_t cols = (size_t)((sX + 15) >> 4) * 16;
    return (size_t)sZ * sY * cols * rw_mask_words(C) * 4;
}

// 16 P bits and 16 N bits -> one word: byte j = P nibble j | N nibble j << 4
__host__ __device__ __forceinline__ uint32_t interleave16(uint32_t p, uint32_t n) {
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        out |= (((p >> (4 * j)) & 0xFu) | (((n >> (4 * j)) & 0xFu) << 4)) << (8 * j);
    return out;
}

// What a pre-pass leaves for rank_wg_kernel.  Described once: the ranking launcher's own workspace
// begins with it, and so does the workspace of the fused pre-pass.
struct RankMasks {
    uint32_t *M, *info;       // the masks of the score box (rw_mask_bytes); [score box]
    uint8_t *valid;           // [V]
};
static inline RankMasks rank_masks_layout(Carver &c, const ppp_box &sb, const Geo &G) {
    const int sX = sb.x1 - sb.x0, sY = sb.y1 - sb.y0, sZ = sb.z1 - sb.z0;
    RankMasks W;
    W.M = (uint32_t *)c.take_bytes(rw_mask_bytes(sZ, sY, sX, G.C));
    W.info = c.take<uint32_t>((size_t)sX * sY * sZ);
    W.valid = c.take<uint8_t>(G.V);
    return W;
}

}  // namespace ppp
