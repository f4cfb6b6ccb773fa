// ppp_rows.hip -- a prediction kept as ROWS for the foreground voxels only.
//
// No counterpart in the reference: its decode writes a dense (C, Z, Y, X) array that is zero outside the
// foreground (decode.py:43-65).  Here the prediction of a mask M (uint8 (Z, Y, X), non-zero = has a row) is
// the table rows[n_rows][C], row k belonging to the k-th voxel of M in raster order (x fastest), and the
// dense box a tile of the assembly needs is made from it on demand:
//     expand :  box[c][z][y][x] = M(z, y, x) ? rows[row(z, y, x)][c] : 0       for every voxel of the box
//     compact:  rows[row(z, y, x)][c] = box[c][z][y][x]                        for the mask voxels of the box
// Elements are moved as bits (2- or 4-byte words), never converted: float32, float16 and bfloat16 are the
// same two kernels.
//
// INDEX (described once, rows_index_layout): the mask as 64-bit words over the LINEAR voxel index
// (word w = voxels [64 w, 64 w + 64)), next to an int64 count of the mask voxels before each word:
//     row(v) = counts[v >> 6] + popcount(words[v >> 6] & ((1 << (v & 63)) - 1))
// 16 bytes per 64 voxels = 0.25 B per voxel (plus one int64 per 1024 words for the scan and the slot
// rounding of the Carver, under 1 KiB).  Built by three launches, no host loop: words + per-word counts +
// per-chunk sums; exclusive scan of the chunk sums (one workgroup); exclusive scan inside every chunk.
//
// MOVE KERNEL: raster order makes the mask voxels of one x-line of a box ONE contiguous piece of the
// table, so a workgroup takes 64 voxels of a box line x RX_CC channels:
//   * rows <-> LDS: per row a run of cc elements, as aligned dwords with 2-byte edges (rows of an odd C
//     are 2-byte aligned only; a tile's LDS image starts at the parity of its first global element, so
//     that with odd C -- every patch volume is odd -- all dwords of all rows are aligned on both sides);
//   * LDS <-> box: channel-major, neighbouring x adjacent.  4-byte elements: a lane per voxel, a channel
//     per wave and step.  2-byte elements: a lane per PAIR of x-neighbours on the box's dword grid, two
//     channels per wave and step (two 128-B segments), the odd voxel in front of a misaligned line as a
//     2-byte store of lane 0.  The zeros of voxels without a row are written by the same stores.
//   * LDS row stride RX_CC + 1 elements (odd): the transposed access of lane p to row 2p (2-byte) or
//     row p (4-byte) lands on dword 129 p + const -- 32 lanes, 32 banks.
//   * LDS: 64 x 129 elements = 16.1 KB (2-byte) / 32.3 KB (4-byte) per workgroup of 256 threads.
// A tile without a mask voxel never touches the table or the LDS: it stores zeros (expand) or returns
// (compact).
#include "ppp_kernels.hpp"

namespace ppp {

static constexpr int RW_CHUNK = 1024;          // index words per scan chunk (one workgroup, 4 words per thread)
static constexpr int RX_CC = 128;              // channels per tile
static constexpr int RX_RS = RX_CC + 1;        // LDS row stride in elements (odd)
static constexpr int RX_TILE = 64 * RX_RS + 2; // elements of the LDS image (+ the parity shift, + even size)

struct RowsIndex {
    unsigned long long *words;   // [n_words]      the mask, bit b of word w = voxel 64 w + b
    long long *counts;           // [n_words + 1]  mask voxels before word w; [n_words] = n_rows
    long long *chunk;            // [n_chunks]     mask voxels before chunk k of RW_CHUNK words
    long long n_words, n_chunks;
};

static RowsIndex rows_index_layout(Carver &c, long long V) {
    RowsIndex I;
    I.n_words = (V + 63) / 64;
    I.n_chunks = (I.n_words + RW_CHUNK - 1) / RW_CHUNK;
    I.words = c.take<unsigned long long>((size_t)I.n_words);
    I.counts = c.take<long long>((size_t)I.n_words + 1);
    I.chunk = c.take<long long>((size_t)I.n_chunks);
    return I;
}

size_t rows_index_bytes(long long V) { Carver c(nullptr); rows_index_layout(c, V); return c.used; }

// ---- index build ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rows_words_kernel(const uint8_t *__restrict__ mask, const long long V, const RowsIndex I) {
    __shared__ long long part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long w0 = (long long)blockIdx.x * RW_CHUNK;
    long long sum = 0;
    for (int i = wave; i < RW_CHUNK; i += 4) {
        const long long w = w0 + i;
        if (w >= I.n_words) break;                  // (wave-uniform)
        const long long v = w * 64 + lane;
        const bool on = v < V && mask[v] != 0;
        const unsigned long long word = __ballot(on);
        const long long cnt = __popcll(word);
        if (lane == 0) { I.words[w] = word; I.counts[w] = cnt; }
        sum += cnt;
    }
    if (lane == 0) part[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) I.chunk[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// exclusive scan of 256 partial sums held in LDS by thread 0 (256 additions), `base` in front; returns the total
__device__ __forceinline__ long long scan256(long long *s, const long long base) {
    long long run = base;
    for (int k = 0; k < 256; ++k) {
        const long long v = s[k];
        s[k] = run;
        run += v;
    }
    return run;
}

__global__ void __launch_bounds__(256) rows_chunk_scan_kernel(const RowsIndex I) {
    __shared__ long long s[256];
    const int t = threadIdx.x;
    const long long per = (I.n_chunks + 255) / 256;
    const long long a = t * per < I.n_chunks ? t * per : I.n_chunks, b = a + per < I.n_chunks ? a + per : I.n_chunks;
    long long sum = 0;
    for (long long i = a; i < b; ++i) sum += I.chunk[i];
    s[t] = sum;
    __syncthreads();
    if (t == 0) I.counts[I.n_words] = scan256(s, 0);
    __syncthreads();
    long long run = s[t];
    for (long long i = a; i < b; ++i) {
        const long long v = I.chunk[i];
        I.chunk[i] = run;
        run += v;
    }
}

__global__ void __launch_bounds__(256) rows_counts_scan_kernel(const RowsIndex I) {
    __shared__ long long s[256];
    const int t = threadIdx.x;
    const long long w0 = (long long)blockIdx.x * RW_CHUNK + 4 * t;
    long long c[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        c[k] = w0 + k < I.n_words ? I.counts[w0 + k] : 0;
        sum += c[k];
    }
    s[t] = sum;
    __syncthreads();
    if (t == 0) scan256(s, I.chunk[blockIdx.x]);
    __syncthreads();
    long long run = s[t];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (w0 + k < I.n_words) I.counts[w0 + k] = run;
        run += c[k];
    }
}

hipError_t run_rows_index_build(const uint8_t *mask, long long V, void *index, long long *n_rows, hipStream_t s) {
    Carver carver(index);
    const RowsIndex I = rows_index_layout(carver, V);
    PPP_GRID_CHECK(I.n_chunks, 256);
    rows_words_kernel<<<dim3((unsigned)I.n_chunks), dim3(256), 0, s>>>(mask, V, I);
    rows_chunk_scan_kernel<<<dim3(1), dim3(256), 0, s>>>(I);
    rows_counts_scan_kernel<<<dim3((unsigned)I.n_chunks), dim3(256), 0, s>>>(I);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = hipMemcpyAsync(n_rows, I.counts + I.n_words, sizeof(long long), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    return hipStreamSynchronize(s);
}

// ---- expand / compact ----------------------------------------------------------------------------
struct RowsMove {
    int C, Y, X;                  // row length, volume line geometry
    int z0, y0, x0, bZ, bY, bX;   // the box
    int nxt, nch;                 // 64-voxel tiles per box line, channel chunks
};

// what a workgroup knows of its tile: 64 voxels (nx of them inside the box) of one box line, cc channels
struct RowsTile {
    unsigned long long tm;   // bit q: voxel q of the tile has a row
    long long r0;            // row of the tile's first mask voxel
    int n, nx, xt, ly, lz, c0, cc, bs;
};

// rows <-> LDS.  Slot d of row j holds the aligned global dword with the row-relative elements
// (2d - h, 2d - h + 1), h = parity of the row's first global element; a slot with one element inside the
// run is a 2-byte access.  4-byte elements: one element per slot.
template <typename E, bool TO_LDS>
__device__ __forceinline__ void rows_phase(E *rows, E *tile, const RowsTile &T, const int C) {
    const int tid = threadIdx.x;
    if constexpr (sizeof(E) == 4) {
        for (int idx = tid; idx < T.n * T.cc; idx += 256) {
            const int j = idx / T.cc, d = idx - j * T.cc;
            E *g = rows + ((T.r0 + j) * (long long)C + T.c0 + d), *l = tile + j * RX_RS + d;
            if (TO_LDS) *l = *g; else *g = *l;
        }
    } else {
        const int DW = T.cc / 2 + 1;
        for (int idx = tid; idx < T.n * DW; idx += 256) {
            const int j = idx / DW, d = idx - j * DW;
            const long long g0 = (T.r0 + j) * (long long)C + T.c0;
            const int e0 = 2 * d - (int)(g0 & 1);
            const bool va = e0 >= 0 && e0 < T.cc, vb = e0 + 1 < T.cc;
            E *g = rows + (g0 + e0), *l = tile + (T.bs + j * RX_RS + e0);
            if (va && vb) {
                const bool lds_aligned = (((uintptr_t)l) & 3) == 0;
                if (TO_LDS) {
                    const uint32_t two = *reinterpret_cast<const uint32_t *>(g);
                    if (lds_aligned) *reinterpret_cast<uint32_t *>(l) = two;
                    else { l[0] = (E)(two & 0xffffu); l[1] = (E)(two >> 16); }
                } else {
                    const uint32_t two = lds_aligned ? *reinterpret_cast<const uint32_t *>(l)
                                                     : ((uint32_t)l[0] | ((uint32_t)l[1] << 16));
                    *reinterpret_cast<uint32_t *>(g) = two;
                }
            } else if (va) {
                if (TO_LDS) l[0] = g[0]; else g[0] = l[0];
            } else if (vb) {
                if (TO_LDS) l[1] = g[1]; else g[1] = l[1];
            }
        }
    }
}

// LDS <-> box, channel-major.  TO_LDS = false: the whole tile of the box is written, zeros included.
template <typename E, bool TO_LDS>
__device__ __forceinline__ void box_phase(E *box, E *tile, const RowsTile &T, const RowsMove &M) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // LDS offset of the row of tile voxel q, -1 without one (or outside the box)
    auto row_of = [&](const int q) -> int {
        if (q >= T.nx || !((T.tm >> q) & 1ull)) return -1;
        return T.bs + __popcll(T.tm & ((1ull << q) - 1ull)) * RX_RS;
    };
    if constexpr (sizeof(E) == 4) {
        const int off = row_of(lane);
        if (TO_LDS && off < 0) return;
        if (lane >= T.nx) return;
        const long long plane = (long long)M.bZ * M.bY * M.bX;         // elements of one channel of the box
        long long o = (((long long)(T.c0 + wave) * M.bZ + T.lz) * M.bY + T.ly) * M.bX + T.xt + lane;
        for (int cr = wave; cr < T.cc; cr += 4, o += 4 * plane) {
            if (TO_LDS) tile[off + cr] = box[o];
            else box[o] = off >= 0 ? tile[off + cr] : (E)0;
        }
    } else {
        const int half = lane >> 5, p = lane & 31;
        const int off0 = row_of(2 * p), off1 = row_of(2 * p + 1), off2 = 2 * p + 2 < 64 ? row_of(2 * p + 2) : -1;
        // tile voxel 0 of the lane's first channel; a lane's channels are 8 apart, so the parity of the line's
        // start -- which pairs of x-neighbours share a dword of the box -- is the same for all of them
        const long long plane = (long long)M.bZ * M.bY * M.bX;
        long long o = (((long long)(T.c0 + 2 * wave + half) * M.bZ + T.lz) * M.bY + T.ly) * M.bX + T.xt;
        const int par = (int)(o & 1);
        const int qa = 2 * p + par;                       // o + qa is even: a dword of the box
        const int oa = par ? off1 : off0, ob = par ? off2 : off1;
        for (int cr = 2 * wave + half; cr < T.cc; cr += 8, o += 8 * plane) {
            if (TO_LDS) {
                if (qa + 1 < T.nx) {
                    const uint32_t two = *reinterpret_cast<const uint32_t *>(box + o + qa);
                    if (oa >= 0) tile[oa + cr] = (E)(two & 0xffffu);
                    if (ob >= 0) tile[ob + cr] = (E)(two >> 16);
                } else if (qa < T.nx && oa >= 0) {
                    tile[oa + cr] = box[o + qa];
                }
                if (par && p == 0 && off0 >= 0) tile[off0 + cr] = box[o];
            } else {
                const uint32_t a = oa >= 0 ? tile[oa + cr] : 0u, b = ob >= 0 ? tile[ob + cr] : 0u;
                if (qa + 1 < T.nx) *reinterpret_cast<uint32_t *>(box + o + qa) = a | (b << 16);
                else if (qa < T.nx) box[o + qa] = (E)a;
                if (par && p == 0) box[o] = off0 >= 0 ? tile[off0 + cr] : (E)0;
            }
        }
    }
}

template <typename E, bool EXPAND>
__global__ void __launch_bounds__(256)
    rows_move_kernel(E *rows, const unsigned long long *__restrict__ words, const long long *__restrict__ counts,
                     E *box, const RowsMove M) {
    __shared__ uint32_t lds[RX_TILE * sizeof(E) / 4];
    E *tile = reinterpret_cast<E *>(lds);
    RowsTile T;
    long long b = blockIdx.x;
    const int ch = (int)(b % M.nch);
    b /= M.nch;
    T.xt = (int)(b % M.nxt) * 64;
    b /= M.nxt;
    T.ly = (int)(b % M.bY);
    T.lz = (int)(b / M.bY);
    T.nx = M.bX - T.xt < 64 ? M.bX - T.xt : 64;
    T.c0 = ch * RX_CC;
    T.cc = M.C - T.c0 < RX_CC ? M.C - T.c0 : RX_CC;
    const long long v0 = ((long long)(M.z0 + T.lz) * M.Y + (M.y0 + T.ly)) * M.X + (M.x0 + T.xt);
    const long long w = v0 >> 6;
    const int sh = (int)(v0 & 63);
    const unsigned long long first = words[w];
    T.tm = first >> sh;
    if (sh && sh + T.nx > 64) T.tm |= words[w + 1] << (64 - sh);     // (the tile's last voxel lies in word w + 1)
    if (T.nx < 64) T.tm &= (1ull << T.nx) - 1ull;
    T.n = __popcll(T.tm);
    T.r0 = counts[w] + __popcll(first & ((1ull << sh) - 1ull));
    T.bs = sizeof(E) == 2 ? (int)((T.r0 * (long long)M.C + T.c0) & 1) : 0;
    // (everything above is the same in every thread of the workgroup: the branches below are uniform)
    if (EXPAND) {
        if (T.n) {
            rows_phase<E, true>(rows, tile, T, M.C);
            __syncthreads();
        }
        box_phase<E, false>(box, tile, T, M);
    } else {
        if (!T.n) return;
        box_phase<E, true>(box, tile, T, M);
        __syncthreads();
        rows_phase<E, false>(rows, tile, T, M.C);
    }
}

hipError_t launch_rows_move(bool expand, void *rows, int elem_bytes, int C, const void *index, int Z, int Y, int X,
                            const ppp_box &bx, void *box, hipStream_t s) {
    Carver carver(const_cast<void *>(index));
    const RowsIndex I = rows_index_layout(carver, (long long)Z * Y * X);
    RowsMove M;
    M.C = C; M.Y = Y; M.X = X;
    M.z0 = bx.z0; M.y0 = bx.y0; M.x0 = bx.x0;
    M.bZ = bx.z1 - bx.z0; M.bY = bx.y1 - bx.y0; M.bX = bx.x1 - bx.x0;
    M.nxt = (M.bX + 63) / 64;
    M.nch = (C + RX_CC - 1) / RX_CC;
    const long long blocks = (long long)M.bZ * M.bY * M.nxt * M.nch;
    PPP_GRID_CHECK(blocks, 256);
    const dim3 grid((unsigned)blocks), wg(256);
    if (elem_bytes == 4) {
        if (expand) rows_move_kernel<uint32_t, true><<<grid, wg, 0, s>>>((uint32_t *)rows, I.words, I.counts, (uint32_t *)box, M);
        else rows_move_kernel<uint32_t, false><<<grid, wg, 0, s>>>((uint32_t *)rows, I.words, I.counts, (uint32_t *)box, M);
    } else {
        if (expand) rows_move_kernel<uint16_t, true><<<grid, wg, 0, s>>>((uint16_t *)rows, I.words, I.counts, (uint16_t *)box, M);
        else rows_move_kernel<uint16_t, false><<<grid, wg, 0, s>>>((uint16_t *)rows, I.words, I.counts, (uint16_t *)box, M);
    }
    return hipGetLastError();
}

}  // namespace ppp
