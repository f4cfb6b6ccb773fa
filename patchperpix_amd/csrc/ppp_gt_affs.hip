// ppp_gt_affs.hip -- the ground-truth patch affinities of a label volume as an ARRAY
// (PatchPerPix/util/train_util.py:349-775, the seg_to_affgraph_*_torch* family).
//
//   multi:   G[b][e][v] = 1 iff v + nhood[e] lies inside the volume and some channel c has
//            labels[b][c][v] != 0 and labels[b][c][v] == labels[b][c][v + nhood[e]]          (else 0)
//   single:  G[b][e][v] = float(c * c), c = labels[b][v], where c == labels[b][v + nhood[e]]   (else 0)
//
// A voxel outside the volume reads as label 0, which gives both forms their zero: a non-zero centre never
// equals it, and a zero centre contributes 0 (multi: the centre must be non-zero; single: 0 * 0).
//
// gt_dense_kernel.  The kernel is bound by its stores: B E V elements out against B L V words in.  A
// workgroup owns a tile of TZ x TY x TX output voxels (TY, TX powers of two) and an edge range.  STAGED: the
// labels of the tile plus the halo of nhood, all L channels, are read ONCE into LDS (word by word, eight
// independent loads per thread in flight, zero outside the volume) and every edge reads its neighbours from
// there; where tile plus halo do not fit the 64 KiB the kernel asks for (a large L, an offset as long as an
// axis), the same code reads the neighbours from global memory with a bounds check (STAGED = false).
//   A wave's unit of work is a chunk and, where the tile has fewer chunks than the workgroup has waves
//   (2-byte elements), a part of the edge range: all four waves store.
//   A wave takes chunks of 64 VEC consecutive voxels of the tile (VEC = 16 bytes / element size) and works
//   on a chunk in two lane layouts:
//   pass layout   pass k, lane i: voxel 64 k + i of the chunk.  Lanes are consecutive in x, so the LDS reads
//                 are consecutive words in each 32-lane half: no bank conflict at any row pitch.  The centre's
//                 labels of the first kRegCh channels stay in registers over the edge loop.
//   store layout  lane j: voxels VEC j .. VEC j + VEC - 1, one 16-byte store, contiguous in x over the wave.
//   The result of an element is one bit, so the change of layout is free: __ballot of pass k IS the 64 results
//   of that pass, a wave-uniform mask, and lane j takes its VEC bits out of mask (VEC j) / 64.
//   A store that is not 16-byte aligned (a box whose x extent is no multiple of VEC shifts every row) or
//   that crosses the end of a row goes out in the widest aligned pieces, down to single elements.
//   Chunks without a foreground centre write their zeros without reading a neighbour; passes without one are
//   skipped.  Edges are read 64 at a time, one per lane, and handed round with v_readlane.
//   The single-channel form (float32 only) has no bit to ballot: it writes one dword per lane from the pass
//   layout, 256 contiguous bytes per wave instruction.
// gt_samples_kernel: one wave per sample row (b, z, y, x), lanes over e; the centre's labels are wave-uniform.
#include "ppp_kernels.hpp"

namespace ppp {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kLdsWords = 16384;     // 64 KiB of staged labels: two workgroups per CU
constexpr int kRegCh = 4;            // channels whose centre labels a lane keeps in registers
constexpr int kFill = 8;             // loads a thread has in flight while the region is staged

struct GtDense {
    int B, L, Z, Y, X, E;
    int bz0, by0, bx0, bZ, bY, bX;   // the output box
    int TZ, TY, TX, shx, shy;        // tile; TX = 1 << shx, TY = 1 << shy
    int ntz, nty, ntx;               // tiles per axis of the box
    int hz0, hy0, hx0, hz1, hy1, hx1;   // halo, widened to hold offset 0
    int RZ, RY, RX;                  // staged region = tile + halo
    unsigned mRZ, mRY, mRX;          // ceil(2^32 / R*): n / R* = umulhi(n, m) for the n < 2^14 of the region (udiv)
    int esplit;                      // edge ranges per tile (gridDim.y)
    unsigned one;                    // the bits of 1 in a 16-bit element type
};

// tiles the launcher chooses from: each a multiple of 512 voxels (one chunk of 2-byte elements)
constexpr int kTiles[][3] = {{4, 8, 32}, {2, 16, 32}, {1, 32, 32}, {1, 16, 64}, {2, 8, 32}, {1, 16, 32}, {1, 8, 64}};
constexpr int kNTiles = sizeof(kTiles) / sizeof(kTiles[0]);

// n / d for n < 2^16 and 1 < d < 2^16 with m = ceil(2^32 / d): exact, n (m d - 2^32) < 2^32
__device__ __forceinline__ int udiv(const int n, const int d, const unsigned m) {
    return d == 1 ? n : (int)__umulhi((unsigned)n, m);
}

__device__ __forceinline__ void store_bits(float *p, const unsigned bits, const int nval) {
    const float v0 = bits & 1u ? 1.0f : 0.0f, v1 = bits & 2u ? 1.0f : 0.0f, v2 = bits & 4u ? 1.0f : 0.0f,
                v3 = bits & 8u ? 1.0f : 0.0f;
    const uintptr_t a = (uintptr_t)p;
    if (nval == 4 && (a & 15) == 0) {
        *(float4 *)p = make_float4(v0, v1, v2, v3);
    } else if (nval == 4 && (a & 7) == 0) {
        *(float2 *)p = make_float2(v0, v1);
        *(float2 *)(p + 2) = make_float2(v2, v3);
    } else {
        if (nval > 0) p[0] = v0;
        if (nval > 1) p[1] = v1;
        if (nval > 2) p[2] = v2;
        if (nval > 3) p[3] = v3;
    }
}

// 16-bit elements (float16 / bfloat16 differ in the bits of 1 only)
__device__ __forceinline__ void store_bits(uint16_t *p, const unsigned bits, const int nval, const unsigned one) {
    unsigned w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = ((bits >> (2 * q)) & 1u) * one | ((bits >> (2 * q + 1)) & 1u) * (one << 16);
    const uintptr_t a = (uintptr_t)p;
    if (nval == 8 && (a & 15) == 0) {
        *(uint4 *)p = make_uint4(w[0], w[1], w[2], w[3]);
    } else if (nval == 8 && (a & 7) == 0) {
        *(uint2 *)p = make_uint2(w[0], w[1]);
        *(uint2 *)(p + 4) = make_uint2(w[2], w[3]);
    } else if (nval == 8 && (a & 3) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) ((unsigned *)p)[q] = w[q];
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (q < nval) p[q] = (uint16_t)((bits >> q) & 1u ? one : 0u);
    }
}

// ALIGNED (the box's x extent a multiple of VEC, the output 16-byte aligned): every group is whole or empty and
// every store one 16-byte store.  A kernel of its own: in one function the compiler merges the aligned store
// with the piecewise ones into dword + dwordx2 + dword.
template <bool ALIGNED>
__device__ __forceinline__ void store_group(float *p, const unsigned bits, const int nval, const unsigned) {
    if (ALIGNED) {
        if (nval) *(float4 *)p = make_float4(bits & 1u ? 1.0f : 0.0f, bits & 2u ? 1.0f : 0.0f, bits & 4u ? 1.0f : 0.0f,
                                             bits & 8u ? 1.0f : 0.0f);
    } else {
        store_bits(p, bits, nval);
    }
}
template <bool ALIGNED>
__device__ __forceinline__ void store_group(uint16_t *p, const unsigned bits, const int nval, const unsigned one) {
    if (ALIGNED) {
        unsigned w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = ((bits >> (2 * q)) & 1u) * one | ((bits >> (2 * q + 1)) & 1u) * (one << 16);
        if (nval) *(uint4 *)p = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        store_bits(p, bits, nval, one);
    }
}

template <typename T, bool STAGED, bool SINGLE, bool ALIGNED>
__global__ void __launch_bounds__(kBlock)
    gt_dense_kernel(const int32_t *__restrict__ labels, const int32_t *__restrict__ nhood, T *__restrict__ out,
                    const GtDense G) {
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr int CH = 64 * VEC;
    extern __shared__ __align__(16) int32_t gt_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    // the tile and the edge range of this workgroup
    unsigned t = blockIdx.x;
    const int tix = (int)(t % (unsigned)G.ntx); t /= (unsigned)G.ntx;
    const int tiy = (int)(t % (unsigned)G.nty); t /= (unsigned)G.nty;
    const int tiz = (int)(t % (unsigned)G.ntz);
    const int b = (int)(t / (unsigned)G.ntz);
    const int oz = tiz * G.TZ, oy = tiy * G.TY, ox = tix * G.TX;            // in box coordinates
    const int w0 = (int)((long long)G.E * blockIdx.y / G.esplit), w1 = (int)((long long)G.E * (blockIdx.y + 1) / G.esplit);
    const long long V = (long long)G.Z * G.Y * G.X;
    const long long bV = (long long)G.bZ * G.bY * G.bX;
    const int32_t *lab = labels + (long long)b * G.L * V;
    T *outb = out + (long long)b * G.E * bV;
    const int CS = G.RZ * G.RY * G.RX;                                       // words per staged channel

    if (STAGED) {
        // the region word by word, kFill independent loads per thread in flight; zero outside the volume
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
                if (base + j * kBlock < total) gt_lds[base + j * kBlock] = v[j];
        }
        __syncthreads();
    }

    // a wave's unit of work: a chunk, and -- where the tile has fewer chunks than the workgroup waves -- a part
    // of the edge range
    const int nchunks = (G.TZ * G.TY * G.TX) / CH;
    const int esub = nchunks < kWaves ? kWaves / nchunks : 1;
    for (int unit = wave; unit < nchunks * esub; unit += kWaves) {
        const int chunk = unit % nchunks, part = unit / nchunks;
        const int e0 = w0 + (int)((long long)(w1 - w0) * part / esub), e1 = w0 + (int)((long long)(w1 - w0) * (part + 1) / esub);
        // ---- pass layout: the centres ----
        int cidx[VEC];                   // STAGED: the centre's word in channel 0 of the region
        int vz[VEC], vy[VEC], vx[VEC];   // !STAGED: the centre in volume coordinates
        long long pbase[VEC];            // SINGLE: the centre's element of one edge's output
        int32_t cl[VEC][kRegCh];
        bool inb[VEC], fg[VEC];
        unsigned long long fgm[VEC];
        unsigned long long any_fg = 0, any_in = 0;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const int tt = chunk * CH + 64 * k + lane;
            const int tx = tt & (G.TX - 1), ty = (tt >> G.shx) & (G.TY - 1), tz = tt >> (G.shx + G.shy);
            inb[k] = oz + tz < G.bZ && oy + ty < G.bY && ox + tx < G.bX;
            cidx[k] = ((tz - G.hz0) * G.RY + (ty - G.hy0)) * G.RX + (tx - G.hx0);
            vz[k] = G.bz0 + oz + tz; vy[k] = G.by0 + oy + ty; vx[k] = G.bx0 + ox + tx;
            pbase[k] = ((long long)(oz + tz) * G.bY + (oy + ty)) * G.bX + (ox + tx);
            const long long cv = ((long long)vz[k] * G.Y + vy[k]) * G.X + vx[k];
            bool f = SINGLE;             // single: every in-box centre is computed (0 gives 0)
#pragma unroll
            for (int c = 0; c < kRegCh; ++c) {
                cl[k][c] = 0;
                if (c < G.L && inb[k]) cl[k][c] = STAGED ? gt_lds[cidx[k] + c * CS] : lab[(long long)c * V + cv];
                f |= cl[k][c] != 0;
            }
            for (int c = kRegCh; c < G.L; ++c)
                if (inb[k]) f |= (STAGED ? gt_lds[cidx[k] + c * CS] : lab[(long long)c * V + cv]) != 0;
            fg[k] = f && inb[k];
            fgm[k] = __ballot(fg[k]);
            any_fg |= fgm[k];
            any_in |= __ballot(inb[k]);
        }
        if (any_in == 0) continue;       // a chunk of the tile's overhang past the box

        // ---- store layout ----
        const int ts = chunk * CH + VEC * lane;
        const int sx = ts & (G.TX - 1), sy = (ts >> G.shx) & (G.TY - 1), sz = ts >> (G.shx + G.shy);
        int nval = 0;
        if (oz + sz < G.bZ && oy + sy < G.bY) nval = min(max(G.bX - (ox + sx), 0), VEC);
        const long long sbase = ((long long)(oz + sz) * G.bY + (oy + sy)) * G.bX + (ox + sx);
        const int which = (VEC * lane) >> 6, shift = (VEC * lane) & 63;

        if (any_fg == 0) {               // background only: zeros, no neighbour is read
            for (int e = e0; e < e1; ++e) {
                if (SINGLE) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k)
                        if (inb[k]) ((float *)outb)[(long long)e * bV + pbase[k]] = 0.0f;
                } else {
                    store_group<ALIGNED>(outb + (long long)e * bV + sbase, 0u, nval, G.one);
                }
            }
            continue;
        }

        for (int eb = e0; eb < e1; eb += 64) {
            // 64 edges, one per lane; v_readlane hands them round
            int dz = 0, dy = 0, dx = 0;
            if (eb + lane < e1) {
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
            for (int q = 0; q < ne; ++q) {
                const int off = __builtin_amdgcn_readlane(offl, q);
                const int ez = __builtin_amdgcn_readlane(dz, q), ey = __builtin_amdgcn_readlane(dy, q),
                          ex = __builtin_amdgcn_readlane(dx, q);
                const long long goff = ((long long)ez * G.Y + ey) * G.X + ex;
                const long long eo = (long long)(eb + q) * bV;
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
                    if (SINGLE) {
                        int32_t n = 0;
                        if (fg[k]) n = STAGED ? gt_lds[cidx[k] + off] : (ok ? lab[nv] : 0);
                        const int32_t c = cl[k][0];
                        const float val = n == c ? (float)(int32_t)((uint32_t)c * (uint32_t)c) : 0.0f;
                        if (inb[k]) ((float *)outb)[eo + pbase[k]] = val;
                    } else {
                        bool p = false;
                        if (fg[k]) {
#pragma unroll
                            for (int c = 0; c < kRegCh; ++c) {
                                if (c < G.L) {
                                    const int32_t n = STAGED ? gt_lds[cidx[k] + c * CS + off]
                                                             : (ok ? lab[(long long)c * V + nv] : 0);
                                    p |= n == cl[k][c] && n != 0;
                                }
                            }
                            for (int c = kRegCh; c < G.L; ++c) {
                                const int32_t cc = STAGED ? gt_lds[cidx[k] + c * CS] : lab[(long long)c * V + nv - goff];
                                const int32_t n = STAGED ? gt_lds[cidx[k] + c * CS + off]
                                                         : (ok ? lab[(long long)c * V + nv] : 0);
                                p |= n == cc && n != 0;
                            }
                        }
                        m[k] = __ballot(p);
                    }
                }
                if (!SINGLE) {
                    unsigned long long mine = m[0];
#pragma unroll
                    for (int k = 1; k < VEC; ++k) mine = which == k ? m[k] : mine;
                    const unsigned bits = (unsigned)(mine >> shift) & ((1u << VEC) - 1u);
                    store_group<ALIGNED>(outb + eo + sbase, bits, nval, G.one);
                }
            }
        }
    }
}

struct GtSamples {
    int B, L, Z, Y, X, E;
    int pz, py, px, cz, cy, cx;
    long long N;
    unsigned one;
};

template <typename T>
__global__ void __launch_bounds__(kBlock)
    gt_samples_kernel(const int32_t *__restrict__ labels, const int32_t *__restrict__ samples,
                      const int32_t *__restrict__ nhood, T *__restrict__ out, const GtSamples G) {
    const int lane = threadIdx.x & 63;
    const long long n = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (n >= G.N) return;
    const long long V = (long long)G.Z * G.Y * G.X;
    const int sb = samples[4 * n];
    const long long z0 = samples[4 * n + 1], y0 = samples[4 * n + 2], x0 = samples[4 * n + 3];
    const bool bok = sb >= 0 && sb < G.B;
    const int32_t *lab = labels + (long long)(bok ? sb : 0) * G.L * V;
    const long long zc = z0 + G.cz, yc = y0 + G.cy, xc = x0 + G.cx;
    const bool cok = bok && zc >= 0 && zc < G.Z && yc >= 0 && yc < G.Y && xc >= 0 && xc < G.X;
    const long long cv = (zc * G.Y + yc) * G.X + xc;
    T one, zero;
    if constexpr (sizeof(T) == 4) { one = 1.0f; zero = 0.0f; }
    else { one = (T)G.one; zero = 0; }
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
        out[n * G.E + e] = p ? one : zero;
    }
}

long long region_words(const int *t, const long long *h, int L) {
    return (long long)L * (t[0] + h[0]) * (t[1] + h[1]) * (t[2] + h[2]);
}

unsigned one_bits(int dtype) { return dtype == PPP_F16 ? 0x3C00u : 0x3F80u; }

}  // namespace

// The launcher's choice for a call, without a launch: out = tile z, y, x; 1 when tile + halo are staged in LDS;
// edge ranges per tile.  Among the tiles whose region fits, the one that stages the fewest words in all.
void gt_affs_dense_plan(int B, int L, int E, const int *halo, const int *box, int32_t out[5]) {
    long long h[3];
    for (int a = 0; a < 3; ++a) h[a] = (long long)(halo[2 * a + 1] > 0 ? halo[2 * a + 1] : 0) - (halo[2 * a] < 0 ? halo[2 * a] : 0);
    const int ext[3] = {box[1] - box[0], box[3] - box[2], box[5] - box[4]};
    int best = -1;
    long long best_cost = 0, best_tiles = 0;
    for (int i = 0; i < kNTiles; ++i) {
        if (h[0] > kLdsWords || h[1] > kLdsWords || h[2] > kLdsWords || L > kLdsWords) break;
        const long long words = region_words(kTiles[i], h, L);
        if (words > kLdsWords) continue;
        long long tiles = 1;
        for (int a = 0; a < 3; ++a) tiles *= (ext[a] + kTiles[i][a] - 1) / kTiles[i][a];
        const long long cost = tiles * (words + 1024);
        if (best < 0 || cost < best_cost) { best = i; best_cost = cost; best_tiles = tiles; }
    }
    const int staged = best >= 0;
    if (!staged) {
        best = 5;                        // direct loads: 1 x 16 x 32
        best_tiles = 1;
        for (int a = 0; a < 3; ++a) best_tiles *= (ext[a] + kTiles[best][a] - 1) / kTiles[best][a];
    }
    // enough workgroups to fill the device, at least 32 edges each
    long long split = 2048 / (best_tiles * B > 0 ? best_tiles * B : 1);
    if (split > E / 32) split = E / 32;
    if (split < 1) split = 1;
    out[0] = kTiles[best][0]; out[1] = kTiles[best][1]; out[2] = kTiles[best][2];
    out[3] = staged;
    out[4] = (int32_t)split;
}

// Does not synchronise; no workspace.  The caller has checked the sizes (ppp_gt_affs_dense).
hipError_t run_gt_affs_dense(const int32_t *labels, int B, int L, int Z, int Y, int X, const int32_t *nhood, int E,
                             const int *halo, const int *box, void *out, int dtype, int single, hipStream_t s) {
    int32_t plan[5];
    gt_affs_dense_plan(B, L, E, halo, box, plan);
    GtDense G;
    G.B = B; G.L = L; G.Z = Z; G.Y = Y; G.X = X; G.E = E;
    G.bz0 = box[0]; G.by0 = box[2]; G.bx0 = box[4];
    G.bZ = box[1] - box[0]; G.bY = box[3] - box[2]; G.bX = box[5] - box[4];
    G.TZ = plan[0]; G.TY = plan[1]; G.TX = plan[2];
    G.shx = __builtin_ctz((unsigned)G.TX); G.shy = __builtin_ctz((unsigned)G.TY);
    G.ntz = (G.bZ + G.TZ - 1) / G.TZ; G.nty = (G.bY + G.TY - 1) / G.TY; G.ntx = (G.bX + G.TX - 1) / G.TX;
    const bool staged = plan[3] != 0;
    // the direct kernel takes no halo: it never forms a region
    G.hz0 = staged && halo[0] < 0 ? halo[0] : 0; G.hz1 = staged && halo[1] > 0 ? halo[1] : 0;
    G.hy0 = staged && halo[2] < 0 ? halo[2] : 0; G.hy1 = staged && halo[3] > 0 ? halo[3] : 0;
    G.hx0 = staged && halo[4] < 0 ? halo[4] : 0; G.hx1 = staged && halo[5] > 0 ? halo[5] : 0;
    G.RZ = G.TZ + G.hz1 - G.hz0; G.RY = G.TY + G.hy1 - G.hy0; G.RX = G.TX + G.hx1 - G.hx0;
    G.esplit = plan[4];
    G.one = one_bits(dtype);
    const long long blocks = (long long)B * G.ntz * G.nty * G.ntx;
    PPP_GRID_CHECK(blocks, kBlock);
    const dim3 grid((unsigned)blocks, (unsigned)G.esplit);
    const size_t lds = staged ? (size_t)L * G.RZ * G.RY * G.RX * sizeof(int32_t) : 0;
    auto magic = [](int d) { return d > 1 ? (unsigned)(((1ull << 32) + d - 1) / d) : 0u; };
    G.mRZ = magic(G.RZ); G.mRY = magic(G.RY); G.mRX = magic(G.RX);
    const int vec = dtype == PPP_F32 ? 4 : 8;
    const bool aligned = !single && G.bX % vec == 0 && ((uintptr_t)out & 15) == 0;
    auto launch = [&](auto kernel, auto *o) { kernel<<<grid, dim3(kBlock), lds, s>>>(labels, nhood, o, G); };
    if (single) {
        if (staged) launch(gt_dense_kernel<float, true, true, false>, (float *)out);
        else launch(gt_dense_kernel<float, false, true, false>, (float *)out);
    } else if (dtype == PPP_F32) {
        if (staged && aligned) launch(gt_dense_kernel<float, true, false, true>, (float *)out);
        else if (staged) launch(gt_dense_kernel<float, true, false, false>, (float *)out);
        else if (aligned) launch(gt_dense_kernel<float, false, false, true>, (float *)out);
        else launch(gt_dense_kernel<float, false, false, false>, (float *)out);
    } else {
        if (staged && aligned) launch(gt_dense_kernel<uint16_t, true, false, true>, (uint16_t *)out);
        else if (staged) launch(gt_dense_kernel<uint16_t, true, false, false>, (uint16_t *)out);
        else if (aligned) launch(gt_dense_kernel<uint16_t, false, false, true>, (uint16_t *)out);
        else launch(gt_dense_kernel<uint16_t, false, false, false>, (uint16_t *)out);
    }
    return hipGetLastError();
}

hipError_t run_gt_affs_samples(const int32_t *labels, int B, int L, int Z, int Y, int X, const int32_t *samples,
                               long long N, const int32_t *nhood, int E, const int *ps, const int *ctr, void *out,
                               int dtype, hipStream_t s) {
    GtSamples G;
    G.B = B; G.L = L; G.Z = Z; G.Y = Y; G.X = X; G.E = E;
    G.pz = ps[0]; G.py = ps[1]; G.px = ps[2];
    G.cz = ctr[0]; G.cy = ctr[1]; G.cx = ctr[2];
    G.N = N;
    G.one = one_bits(dtype);
    const long long blocks = (N + kWaves - 1) / kWaves;
    PPP_GRID_CHECK(blocks, kBlock);
    if (dtype == PPP_F32)
        gt_samples_kernel<float><<<dim3((unsigned)blocks), dim3(kBlock), 0, s>>>(labels, samples, nhood, (float *)out, G);
    else
        gt_samples_kernel<uint16_t><<<dim3((unsigned)blocks), dim3(kBlock), 0, s>>>(labels, samples, nhood, (uint16_t *)out, G);
    return hipGetLastError();
}

}  // namespace ppp
