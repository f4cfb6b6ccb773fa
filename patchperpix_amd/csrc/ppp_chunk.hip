// ppp_chunk.hip -- one stored zarr chunk, decompressed on the host but still Blosc-shuffled, to its place in
// a device tensor: un-shuffle, optional value flags and scatter in one pass (ppp_chunk_scatter).
//
// Block rule (minizarr.bit_unshuffle / byte_unshuffle, c-blosc + bitshuffle): block b covers bytes
// [b * blocksize, min(nbytes, (b + 1) * blocksize)).  In a bit-shuffled block of nel elements of t bytes the
// first n = nel / 8 * 8 elements are stored as 8 t planes of n / 8 bytes, plane 8 j + k holding bit k of
// byte j, element e at bit e % 8 of byte e / 8; the other elements follow as they are.  A byte-shuffled
// block is t runs of nel bytes.
//
// Work: a wave takes 2048 consecutive elements of a block.  Lane l owns elements [32 l, 32 l + 32): it
// loads one dword of each plane (the wave reads 256 contiguous bytes per plane), transposes the 8 x 32 bit
// matrix of every byte position with the masked-shift butterfly and leaves its 32 elements in the wave's
// LDS slice.  The wave then walks the slice in pieces of 16 bytes, lane after lane, so that consecutive
// lanes store consecutive addresses: a piece that lies in one row of the chunk's fastest axis, inside the
// selection, goes out as the widest aligned store (16, 8, 4 bytes, then elements); a piece that crosses a
// row end goes out element by element.
#include "ppp_kernels.hpp"

namespace ppp {

namespace {

constexpr int CHUNK_THREADS = 256;              // 4 waves, each with a slice of its own
constexpr int LANE_ELEMS = 32;
constexpr int WAVE_ELEMS = 64 * LANE_ELEMS;

template <int T> struct ElemWord;
template <> struct ElemWord<1> { using type = uint8_t; };
template <> struct ElemWord<2> { using type = uint16_t; };
template <> struct ElemWord<4> { using type = uint32_t; };

struct Flags {
    bool neg = false, gt1 = false, nan = false;
    __device__ __forceinline__ void see(float x) {
        neg = neg || x < 0.0f;
        gt1 = gt1 || x > 1.0f;
        nan = nan || x != x;
    }
};

// the value of one stored element (T bytes, little endian, in the low bits of `bits`)
template <int T>
__device__ __forceinline__ void see_elem(Flags &f, int fkind, uint32_t bits) {
    if (T == 2 && fkind == PPP_F16) f.see(__half2float(__ushort_as_half((unsigned short)bits)));
    if (T == 4 && fkind == PPP_F32) f.see(__uint_as_float(bits));
}
template <int T>
__device__ __forceinline__ void see_word(Flags &f, int fkind, uint32_t w) {
    if (T == 2) {
        see_elem<2>(f, fkind, w & 0xffffu);
        see_elem<2>(f, fkind, w >> 16);
    }
    if (T == 4) see_elem<4>(f, fkind, w);
}

// 8 x 8 bit transpose of every byte position of eight words at once: afterwards bit k of byte q of w[c] is
// what bit c of byte q of w[k] was
__device__ __forceinline__ void butterfly8(uint32_t (&w)[8]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t t = ((w[k] >> 4) ^ w[k + 4]) & 0x0f0f0f0fu;
        w[k + 4] ^= t;
        w[k] ^= t << 4;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (!(k & 2)) {
            const uint32_t t = ((w[k] >> 2) ^ w[k + 2]) & 0x33333333u;
            w[k + 2] ^= t;
            w[k] ^= t << 2;
        }
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        const uint32_t t = ((w[k] >> 1) ^ w[k + 1]) & 0x55555555u;
        w[k + 1] ^= t;
        w[k] ^= t << 1;
    }
}

// position in the chunk (4 axes, C order) and the destination of its row
struct Walk {
    int c[4];
    bool row_ok;        // the row (c[0], c[1], c[2]) lies in the chunk and in the selection
    long long row_off;  // destination element offset of chunk column xlo of that row
};

__device__ __forceinline__ void walk_row(const ChunkGeo &g, Walk &w) {
    bool ok = w.c[0] < g.cs[0];
    long long off = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        ok = ok && w.c[a] >= g.clo[a] && w.c[a] < g.chi[a];
        off += (long long)(w.c[a] - g.clo[a]) * g.dstride[a];
    }
    w.row_ok = ok;
    w.row_off = off;
}

__device__ __forceinline__ void walk_from(const ChunkGeo &g, long long lin, Walk &w) {
    if (g.small) {
        // fewer than 2^31 elements in the chunk: 32-bit divisions (a 64-bit one costs several times as much)
        unsigned l = (unsigned)lin, q = l / (unsigned)g.cs[3];
        w.c[3] = (int)(l - q * (unsigned)g.cs[3]);
        l = q;
        q = l / (unsigned)g.cs[2];
        w.c[2] = (int)(l - q * (unsigned)g.cs[2]);
        l = q;
        q = l / (unsigned)g.cs[1];
        w.c[1] = (int)(l - q * (unsigned)g.cs[1]);
        w.c[0] = (int)q;
        walk_row(g, w);
        return;
    }
    w.c[3] = (int)(lin % g.cs[3]);
    lin /= g.cs[3];
    w.c[2] = (int)(lin % g.cs[2]);
    lin /= g.cs[2];
    w.c[1] = (int)(lin % g.cs[1]);
    w.c[0] = (int)(lin / g.cs[1]);
    walk_row(g, w);
}

__device__ __forceinline__ void walk_next(const ChunkGeo &g, Walk &w) {
    if (++w.c[3] < g.cs[3]) return;
    w.c[3] = 0;
    if (++w.c[2] == g.cs[2]) {
        w.c[2] = 0;
        if (++w.c[1] == g.cs[1]) {
            w.c[1] = 0;
            ++w.c[0];
        }
    }
    walk_row(g, w);
}

template <int T>
__global__ __launch_bounds__(CHUNK_THREADS) void chunk_scatter_kernel(const ChunkGeo g) {
    using E = typename ElemWord<T>::type;
    constexpr int LANE_WORDS = LANE_ELEMS * T / 4;      // dwords a lane's 32 elements take
    constexpr int PIECE_ELEMS = 16 / T;
    __shared__ uint4 lds[CHUNK_THREADS * LANE_WORDS / 4];

    const int lane = threadIdx.x & 63, wave_in_wg = threadIdx.x >> 6;
    const long long wave = (long long)blockIdx.x * (CHUNK_THREADS / 64) + wave_in_wg;
    const long long b = wave / g.waves_per_block;       // Blosc block
    const int wi = (int)(wave % g.waves_per_block);
    const bool live = b < g.nblocks;
    const long long base = b * g.blocksize;
    const long long bsize = live ? (g.nbytes - base < g.blocksize ? g.nbytes - base : g.blocksize) : 0;
    const int nel = (int)(bsize / T);                   // elements of this block
    const uint8_t *src = g.src + base;
    const int e0 = wi * WAVE_ELEMS + lane * LANE_ELEMS; // this lane's first element within the block

    // ---- un-shuffle: the lane's 32 elements, packed little endian in o[]
    uint32_t o[LANE_WORDS];
#pragma unroll
    for (int m = 0; m < LANE_WORDS; ++m) o[m] = 0;
    if (e0 < nel) {
        const bool whole = e0 + LANE_ELEMS <= nel;
        if (g.shuffle == PPP_SHUFFLE_BIT) {
            const int n = nel / 8 * 8, pb = n / 8;      // transposed elements, bytes per plane
            const int p0 = e0 / 8;                      // this lane's first byte within a plane
            const bool fast = e0 + LANE_ELEMS <= n && (pb & 3) == 0 && (base & 3) == 0;
            uint32_t r[T][8];
#pragma unroll
            for (int j = 0; j < T; ++j) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint8_t *p = src + (long long)(8 * j + k) * pb + p0;
                    uint32_t v = 0;
                    if (fast) {
                        v = *reinterpret_cast<const uint32_t *>(p);
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (p0 + q < pb) v |= (uint32_t)p[q] << (8 * q);
                    }
                    r[j][k] = v;
                }
                butterfly8(r[j]);       // byte q of r[j][c]: byte j of element 8 q + c
            }
#pragma unroll
            for (int m = 0; m < LANE_WORDS; ++m) {
                uint32_t v = 0;
#pragma unroll
                for (int bb = 0; bb < 4; ++bb) {
                    const int gb = 4 * m + bb, e = gb / T, j = gb % T;
                    v |= ((r[j][e % 8] >> (8 * (e / 8))) & 0xffu) << (8 * bb);
                }
                o[m] = v;
            }
            if (e0 + LANE_ELEMS > n) {
                // the elements behind the transposed ones are stored as they are
                const uint8_t *raw = src + (long long)n * T;
#pragma unroll
                for (int gb = 0; gb < LANE_ELEMS * T; ++gb) {
                    const int e = e0 + gb / T;
                    if (e >= n && e < nel) {
                        const uint32_t byte = raw[(long long)(e - n) * T + gb % T];
                        o[gb / 4] = (o[gb / 4] & ~(0xffu << (8 * (gb % 4)))) | (byte << (8 * (gb % 4)));
                    }
                }
            }
        } else if (g.shuffle == PPP_SHUFFLE_BYTE) {
#pragma unroll
            for (int gb = 0; gb < LANE_ELEMS * T; ++gb) {
                const int e = e0 + gb / T;
                if (e < nel) o[gb / 4] |= (uint32_t)src[(long long)(gb % T) * nel + e] << (8 * (gb % 4));
            }
        } else if (whole && (base & 3) == 0) {
            const uint32_t *p = reinterpret_cast<const uint32_t *>(src + (long long)e0 * T);
#pragma unroll
            for (int m = 0; m < LANE_WORDS; ++m) o[m] = p[m];
        } else {
#pragma unroll
            for (int gb = 0; gb < LANE_ELEMS * T; ++gb)
                if (e0 + gb / T < nel) o[gb / 4] |= (uint32_t)src[(long long)e0 * T + gb] << (8 * (gb % 4));
        }
    }
    uint4 *mine = lds + (size_t)threadIdx.x * (LANE_WORDS / 4);
#pragma unroll
    for (int m = 0; m < LANE_WORDS / 4; ++m) mine[m] = make_uint4(o[4 * m], o[4 * m + 1], o[4 * m + 2], o[4 * m + 3]);
    __syncthreads();

    // ---- scatter: the wave's 2048 elements in pieces of 16 bytes, lane after lane
    Flags f;
    const uint4 *slice = lds + (size_t)wave_in_wg * 64 * (LANE_WORDS / 4);
    const long long block_elem0 = b * (g.blocksize / T);     // chunk-linear index of the block's first element
    const uintptr_t dst0 = (uintptr_t)g.dst;
#pragma unroll 1
    for (int pass = 0; pass < LANE_WORDS / 4; ++pass) {
        const int piece = pass * 64 + lane;
        const int eb = wi * WAVE_ELEMS + piece * PIECE_ELEMS;       // first element of the piece within the block
        if (eb >= nel) continue;
        const uint4 v = slice[piece];
        const uint32_t q[4] = {v.x, v.y, v.z, v.w};
        Walk w;
        walk_from(g, block_elem0 + eb, w);
        const int x = w.c[3];
        if (eb + PIECE_ELEMS <= nel && x + PIECE_ELEMS <= g.cs[3]) {
            // one row: every part is either written as a whole or, below a dword, by element
            if (!w.row_ok || x + PIECE_ELEMS <= g.clo[3] || x >= g.chi[3]) continue;
            const long long d = w.row_off + (x - g.clo[3]);         // destination element of the piece's first one
            // part of `bytes` bytes at byte offset `at`: inside the selection and aligned?
            auto ok = [&](int at, int bytes) {
                const int xa = x + at / T;
                return xa >= g.clo[3] && xa + bytes / T <= g.chi[3] && ((dst0 + (uintptr_t)((d + at / T) * T)) & (uintptr_t)(bytes - 1)) == 0;
            };
            uint8_t *out = (uint8_t *)g.dst + d * T;
            if (ok(0, 16)) {
                *reinterpret_cast<uint4 *>(out) = v;
#pragma unroll
                for (int m = 0; m < 4; ++m) see_word<T>(f, g.fkind, q[m]);
                continue;
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (ok(8 * h, 8)) {
                    *reinterpret_cast<uint2 *>(out + 8 * h) = make_uint2(q[2 * h], q[2 * h + 1]);
                    see_word<T>(f, g.fkind, q[2 * h]);
                    see_word<T>(f, g.fkind, q[2 * h + 1]);
                    continue;
                }
#pragma unroll
                for (int m = 2 * h; m < 2 * h + 2; ++m) {
                    if (ok(4 * m, 4)) {
                        *reinterpret_cast<uint32_t *>(out + 4 * m) = q[m];
                        see_word<T>(f, g.fkind, q[m]);
                        continue;
                    }
                    if (T < 4) {
#pragma unroll
                        for (int i = 0; i < 4 / T; ++i) {
                            const int xa = x + (4 * m) / T + i;
                            if (xa >= g.clo[3] && xa < g.chi[3]) {
                                const uint32_t bits = (q[m] >> (8 * T * i)) & (T == 1 ? 0xffu : 0xffffu);
                                *reinterpret_cast<E *>(out + 4 * m + T * i) = (E)bits;
                                see_elem<T>(f, g.fkind, bits);
                            }
                        }
                    }
                }
            }
        } else {
            // the piece crosses a row end (or the block's): element by element
#pragma unroll
            for (int i = 0; i < PIECE_ELEMS; ++i) {
                if (eb + i < nel && w.row_ok && w.c[3] >= g.clo[3] && w.c[3] < g.chi[3]) {
                    const uint32_t word = q[(i * T) / 4];
                    const uint32_t bits = T == 4 ? word : (word >> (8 * ((i * T) % 4))) & (T == 1 ? 0xffu : 0xffffu);
                    reinterpret_cast<E *>(g.dst)[w.row_off + (w.c[3] - g.clo[3])] = (E)bits;
                    see_elem<T>(f, g.fkind, bits);
                }
                walk_next(g, w);
            }
        }
    }
    if (g.flags) {
        // every lane of the wave comes here; one lane writes a flag the wave has seen (a plain store of 1)
        const bool neg = __any(f.neg), gt1 = __any(f.gt1), nan = __any(f.nan);
        if (lane == 0) {
            if (neg) g.flags[0] = 1;
            if (gt1) g.flags[1] = 1;
            if (nan) g.flags[2] = 1;
        }
    }
}

}  // namespace

hipError_t launch_chunk_scatter(ChunkGeo g, int typesize, hipStream_t s) {
    if (g.nbytes <= 0) return hipSuccess;
    const long long nel_block = g.blocksize / typesize;
    g.nblocks = (g.nbytes + g.blocksize - 1) / g.blocksize;
    g.small = g.nbytes / typesize < (1ll << 31) - WAVE_ELEMS;     // (a wave's last pieces may lie behind the chunk)
    g.waves_per_block = (int)((nel_block + WAVE_ELEMS - 1) / WAVE_ELEMS);
    const long long waves = g.nblocks * g.waves_per_block;
    const long long blocks = (waves + CHUNK_THREADS / 64 - 1) / (CHUNK_THREADS / 64);
    PPP_GRID_CHECK(blocks, CHUNK_THREADS);
    const dim3 grid((unsigned)blocks), block(CHUNK_THREADS);
    if (typesize == 1) chunk_scatter_kernel<1><<<grid, block, 0, s>>>(g);
    else if (typesize == 2) chunk_scatter_kernel<2><<<grid, block, 0, s>>>(g);
    else if (typesize == 4) chunk_scatter_kernel<4><<<grid, block, 0, s>>>(g);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace ppp
