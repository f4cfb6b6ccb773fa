// ppp_skel_rule.hpp -- the deletion rule of the 3-d thinning (Lee / Kashyap / Chu 1994) as ONE pure
// function of a voxel's 3x3x3 neighbourhood, for the host and the device alike.
//
// A neighbourhood is a 27-bit word: bit (dz+1)*9 + (dy+1)*3 + (dx+1) is set when the voxel at offset
// (dz, dy, dx) is foreground.  The centre (bit 13) is ignored: the rule is a function of the other 26.
//
//   removable(w)  <=>  the centre is no arc end point (it has not exactly one 26-neighbour),
//                      deleting it keeps the Euler characteristic of the neighbourhood, and
//                      its 26-neighbours form exactly ONE 26-connected component without it.
//
// This is what `removable` in ppp_host_skel.cpp computes from a byte neighbourhood with a counting loop,
// a cell count and a stack flood fill; here the Euler term is 26 mask tests (a face / an edge / a vertex
// of the centre cube is owned by it alone iff the 1 / 3 / 7 other cubes around that cell are empty) and
// the component test a bit-parallel flood (dilation of the seed by the 3x3x3 box = three shifts with
// wrap masks, intersected with the neighbours, until it stops growing).
// ppp_host_skel_rule_mismatches (ppp_host_skel.cpp) compares the two forms word by word.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define PPP_SKEL_HD __host__ __device__
#else
#define PPP_SKEL_HD
#endif

namespace ppp_skel {

constexpr uint32_t kAll = (1u << 27) - 1u;
constexpr uint32_t kCentre = 1u << 13;

PPP_SKEL_HD constexpr uint32_t off_bit(int dz, int dy, int dx) { return 1u << ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)); }

// the six face neighbours
constexpr uint32_t kFaces = off_bit(-1, 0, 0) | off_bit(1, 0, 0) | off_bit(0, -1, 0) | off_bit(0, 1, 0) |
                            off_bit(0, 0, -1) | off_bit(0, 0, 1);

// the 3 other cubes around edge k of the centre cube: k = axis * 4 + (s1 > 0) * 2 + (s2 > 0), the edge
// runs along `axis` and sits on the s1 side of axis + 1 and the s2 side of axis + 2 (axes mod 3)
PPP_SKEL_HD constexpr uint32_t edge_mask(int k) {
    const int ax = k >> 2, s1 = (k & 2) ? 1 : -1, s2 = (k & 1) ? 1 : -1;
    int o1[3] = {0, 0, 0}, o2[3] = {0, 0, 0};
    o1[(ax + 1) % 3] = s1;
    o2[(ax + 2) % 3] = s2;
    return off_bit(o1[0], o1[1], o1[2]) | off_bit(o2[0], o2[1], o2[2]) |
           off_bit(o1[0] + o2[0], o1[1] + o2[1], o1[2] + o2[2]);
}
// the 7 other cubes of octant k = (sz > 0) * 4 + (sy > 0) * 2 + (sx > 0)
PPP_SKEL_HD constexpr uint32_t vert_mask(int k) {
    const int sz = (k & 4) ? 1 : -1, sy = (k & 2) ? 1 : -1, sx = (k & 1) ? 1 : -1;
    uint32_t m = 0;
    for (int j = 1; j < 8; ++j) m |= off_bit((j & 4) ? sz : 0, (j & 2) ? sy : 0, (j & 1) ? sx : 0);
    return m;
}

// bits of the cube with x = 0 / y = 0 (the low side a shift must not wrap across)
constexpr uint32_t kXLo = 0x1249249u;                       // bits 0, 3, 6, ..., 24
constexpr uint32_t kYLo = 0x7u | (0x7u << 9) | (0x7u << 18);

// every cell within the 3x3x3 box around a set cell, clipped to the cube
PPP_SKEL_HD inline uint32_t dilate_box(uint32_t s) {
    s |= ((s & ~(kXLo << 2)) << 1) | ((s & ~kXLo) >> 1);
    s |= ((s & ~(kYLo << 6)) << 3) | ((s & ~kYLo) >> 3);
    s |= (s << 9) | (s >> 9);
    return s & kAll;
}

PPP_SKEL_HD inline bool removable(uint32_t w) {
    const uint32_t n = w & kAll & ~kCentre;
    if (n == 0u) return false;                                // an isolated voxel stays
    if ((n & (n - 1u)) == 0u) return false;                   // arc end point: exactly one neighbour
    // chi(with) - chi(without) = vertices - edges + faces - 1 over the cells the centre cube owns alone
    int delta = 6 - __builtin_popcount(n & kFaces) - 1;
#if defined(__HIP__)
#pragma unroll
#endif
    for (int k = 0; k < 12; ++k) delta -= (n & edge_mask(k)) == 0u ? 1 : 0;
#if defined(__HIP__)
#pragma unroll
#endif
    for (int k = 0; k < 8; ++k) delta += (n & vert_mask(k)) == 0u ? 1 : 0;
    if (delta != 0) return false;
    uint32_t s = n & (0u - n);                                // the lowest neighbour seeds the flood
    for (;;) {
        const uint32_t g = dilate_box(s) & n;
        if (g == s) break;
        s = g;
    }
    return s == n;
}

}  // namespace ppp_skel
