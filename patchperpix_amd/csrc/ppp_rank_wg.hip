// ppp_rank_wg.hip -- S2 (patch ranking) on the VOXEL-MAJOR consensus, row-stationary, one
// WORKGROUP (four waves) per tile of centres.
//
// Reference: cuda/rankPatches.cu:28-147; same sums in the same order as ppp_rank_vm.hip (whose
// header states the decomposition: walk the voxels u of the tile grown by the patch radius in
// raster order, stage the consensus row S[u][.] in LDS, every centre of the tile whose window
// holds u takes its step a = u - c + rad; lane = (centre, a); accumulators live in LDS between
// the steps of a centre).  What differs from the one-wave kernel:
//
//   * four waves share ONE row image, ONE coefficient table and a tile of 8 x 16 x 16 (or
//     8 x 8 x 16) centres: the one-wave kernel needs 26 KB of LDS per wave at 9^3 (6 waves per
//     CU, 1.5 per SIMD -- an LDS read then runs at a fraction of its rate and nothing hides
//     the dependent fma chain); here a workgroup needs 30 KB for four waves (16 waves per CU at
//     <= 128 VGPRs).  The items of a row are dealt to the waves in chunks of 64, the wave that
//     takes the odd chunk rotates from row to row.
//   * a row is staged (tz + 2 rz)(ty + 2 ry)(tx + 2 rx) / (tz ty tx) = 4.5 times per centre at
//     9^3 instead of 8 times (HBM fetches of the launch: 0.45 of the one-wave kernel's).
//   * a term is ONE instruction: v_fma_mix_f32 takes its coefficient +-1/32 / 0 as a float16 from
//     either half of a register (no v_perm_b32 to build a float32 coefficient).  fma(32 S, c, acc)
//     with c = +-2^-5 has an exact product and rounds once, like the reference's acc += / -= S.
//   * the P / N masks of a centre are stored interleaved by the pre-pass -- byte j of word k holds
//     the P bits (low nibble) and the N bits (high nibble) of the four partners 16 k + 4 j .. + 3 --
//     so that ONE byte indexes ONE 256-entry table of four float16 coefficients (2 KB; 8-byte
//     reads): 0.25 table reads and 0.25 address operations per term instead of 0.25 + 0.6.
//
// Measured and dropped on a 128^3 / 9^3 launch (this kernel: 204 ms; profiles/r03_e_pmc_s2_wg_*,
// r03_f_s2_variants_timing.txt; all bit-identical):
//   * a two-line row image of 8-byte elements {S[q], S[q + one line]} read by ds_read_b64 (256
//     instead of 128 B per LDS cycle, 12 instead of 16 waves per CU): 227 ms -- fewer LDS cycles
//     (4.6 vs 6.7 * 10^10) but the LDS is only half busy in either form;
//   * a slot-stationary form (a centre always meets the same lane, masks and accumulator stay in
//     registers for the p rows of an x-run: a ninth of the mask loads, which are 60 % of this
//     kernel's 482 GB of fetches): 402 ms -- one 12-wave workgroup per CU does one chunk per
//     barrier interval and nothing overlaps the row publication.
// Round 5, designed and not built: the masks are 60 % of the fetches and, by the
// constant-mask ablation, 39 % of the time, and every chunk waits for its twelve mask loads before
// its chain can start.  A walk along x-lines with lanes bound to (centre line, slot = cx mod 9)
// keeps a centre's masks and accumulator in registers for its nine rows (a ninth of the loads);
// with four waves a line's <= 64 centre lines need ~2.3 groups, i.e. the rows of the line staged
// 2.3 x (from L2) -- the bytes the masks save -- so what it can win is the LATENCY: only if the
// masks of the ONE centre per line that enters at the next row are prefetched (28 x 192 B per row
// and group) by a fifth, helper wave into a 10 KB LDS double buffer while the four compute waves
// run the current row.  Rows that are skipped (no valid voxel) make several centres enter at once:
// those lanes load directly, as every lane does today.
// What holds the kernel back is neither unit alone (VALU 24 %, LDS 54 % busy of which half bank
// conflicts, 2.35 TB/s of fetches) but the stalls of its dependent chains at 16 waves per CU.
//
// Round 5, measured (profiles/r05_z*; DESIGN.md section 7 has the numbers):
//   * kept: the four reads of a group are issued last element first (one s_waitcnt per group); the
//     two-bit masks lie in rows of 16 x-neighbours (a quad load of an x-run touches 144 contiguous
//     bytes); the tiles of a launch are dealt HEAVIEST FIRST inside every XCD's range (a launch ends
//     with its slowest workgroup: one round of 1 024 workgroups 146 ms, every further round 64 ms);
//   * dropped, all bit-identical: TWO x-neighbouring centres per lane sharing their row reads
//     (0.58 reads per term, two independent chains: 476 vs 253 ms -- five chunks of double work per
//     row for four waves, and the second mask set costs a wave per SIMD); three waves per workgroup;
//     ds_read2_b32 through a non-volatile pointer; 8 x 8 x 8 tiles; staggered starts of the first round;
//   * the instruction cache serves 100 % hits and s_waitcnt / s_nop cost next to nothing
//     (tools/ubench/issue_mix.hip); v_fma_mix_f32 issues in 4.6-5.0 cycles per SIMD against 2.9 for
//     v_fma_f32; a conflict-free ds_read_b32 costs the CU 2.6 cycles; with 1 / 2 / 3 / 4 resident
//     workgroups per CU the 112 x 176 x 176 launch takes 579 / 348 / 279 / 248 ms (a fifth would
//     give ~6 %); without masks, table and row reads at all it takes 180 ms.
//
// Round 7, the default benchmark's launch (140^3 centres, 7^3; profiles/r07_b_*):
//   * kept: the items of a row dealt to the lanes by bank (rank_deal_table_kernel; 7^3 only) and the lightest
//     tiles of a launch's part-filled last round split into halves (rw_choose_splits): the S2 call
//     66.7 -> 55.6 ms (59.9 with the dealing alone), the kernel 64.0 -> 52.4 ms; SQ_LDS_BANK_CONFLICT /
//     SQ_LDS_IDX_ACTIVE 8.22e9 / 20.23e9 = 0.41 -> 3.06e9 / 15.56e9 = 0.20 (tools/s2_bank_sim.py: 0.44 ->
//     0.20), SQ_WAIT_ANY / SQ_WAVE_CYCLES 0.60 -> 0.63, FETCH_SIZE 65 -> 86 GB (the lanes of a chunk no
//     longer hold whole x-runs of centres: their mask loads touch more lines).  The dealing also takes the
//     kernel from 100 to 95 VGPRs -- FIVE workgroups per CU instead of four (the divisions by nx, ny of the
//     enumeration are gone) -- and five are faster than four here: 59.9 against 64.0 ms with the fifth kept
//     out by unused LDS.
//   * dropped: splitting the HEAVIEST tiles (64.3 ms: their halves are dealt in the middle of the launch and
//     the whole light tiles still run last and alone); splitting fewer tiles than the last round holds (12 of
//     23 per XCD: 59.9 ms, no gain) or many more (46: 57.5, 80: 57.9, every tile: 62.5 ms); 8 x 8 x 16 or
//     16 x 8 x 16 tiles for the whole launch (66.4 / 66.1 against 66.5 ms on the parent).
//   * not done: the XCDs of the launch still end between 36 and 56 ms (the y-edge slabs of the y-major
//     numbering are light): ranges of equal WEIGHT instead of equal tile count would need slots to spare.
//
// Round 12, the SHAPE of that launch (profiles/r12_a_*; tools/s2_tile_model.py is the CPU
// model the sweep is set against).  1 458 tiles of 8 x 16 x 16 are 183 per XCD for 160 resident slots (five workgroups
// per CU): one round and a tail.  All kept, all bit-identical (same kernel body, same summation order per centre):
//   * TILE FIT: the tile's thickness in z is a run-time value (template parameter DZ; TZ = 16 sizes the LDS arrays:
//     29 KB, 91 VGPRs, still five workgroups per CU).  A 7^3 launch that 8 x 16 x 16 puts between one and two rounds
//     per XCD takes the smallest z step in 8 .. 16 whose tiles fit the resident slots (rw_plan): 10 at 140^3, 142 tiles
//     per XCD, no splits.  S2 call 53.9 -> 49.1 ms; z step 9 (162, two over) 50.0; z steps 11 .. 16 are SLOWER than the
//     parent's launch (54.4 .. 62.8 ms) although they stage fewer rows: fewer than 4.4 workgroups per CU cost more.
//   * RANGES OF EQUAL WEIGHT (rank_tile_order_kernel cuts the y-major sequence at the prefix sums of the weight; an
//     XCD's range may grow by a quarter, clamped): 49.1 -> 48.3 ms at z step 10 (XCD ends 38.0 - 50.6 -> 42.6 - 49.8 ms).
//     Chosen with the tile fit only; PPP_RANK_WG_XCD=weight gives them to any launch (the parent's: 53.9 -> 50.2 ms).
//   * PRE-PASS with the cubic window compiled in and partner validity read from `valid`: 55.5 -> 53.9 ms per call.
//   5^3 and 9^3 launches keep their code and their plan: no workload of theirs was swept.
//
// Round 14, the SIXTH workgroup per CU of that launch (profiles/r14_a_*; all bit-identical):
//   * kept: the run-time-thickness kernel in four LDS sizes -- accs, act_bits and uvalid_bits for 8 / 10 / 12 / 16 slices
//     (RW_FIT_TZ): 20 208 / 22 448 / 24 688 / 29 152 B, which 160 KB hold 8 / 7 / 6 / 5 times (before: 29 152 B and 5 for every
//     z step) -- at six waves per SIMD, __launch_bounds__(256, 6): 80 VGPRs, nothing spilled, because a quad of mask words is
//     loaded one quad ahead of its terms (LAZY) instead of all six before the first term.  The occupancy is asked about the
//     instantiation that is launched, and rw_plan takes the smallest z step in 8 .. 16 whose tiles fit the slots ITS LDS size
//     gives: 8 at 140^3, 183 tiles per XCD for 192 slots.  S2 call at 140^3 (synthetic cells): 48.1 - 48.6 -> 47.2 - 47.4 ms;
//     rank_patches per step of the default benchmark 50.52 - 50.60 -> 47.03 - 47.21 ms, the kernel 49.41 -> 46.61 ms per launch.
//     SQ_WAIT_ANY / SQ_WAVE_CYCLES 0.61 -> 0.62: a wave waits as much as before, a fifth more wave-cycles run beside it.
//   * dropped: 80 VGPRs with the six mask loads first (10 - 11 registers spilled around the term loop: 66.1 against 48.1 ms at
//     z step 10); three waves per workgroup at 94 - 95 VGPRs (six workgroups are 18 waves per CU, the parent held 20: 49.1 ms at
//     z step 8, 51.0 at z step 10); two quads ahead (3 registers spilled, not run).
//   * the z-step sweep under six per CU: 8 / 9 / 10 / 11 / 12 -> 47.3 / 49.3 / 47.8 / 52.6 / 53.1 ms (parent 51.0 / 49.5 / 48.1 /
//     53.4 / 53.8): the smallest fitting step still wins.
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "ppp_kernels.hpp"
#include "ppp_rank_masks.hpp"

namespace ppp {

// waves per SIMD the register budget must allow.  More
// resident waves do not help: 9^3 at 5 per SIMD (96 VGPRs, 14 spilled) 205 -> 247 ms on the 128^3
// launch, 7^3 at 6 per SIMD (75 VGPRs, nothing spilled) 72.5 -> 73.1 ms at 140^3.
static constexpr int RW_MINWAVES = 4;
// LDS bank conflicts of the row reads.  A half-wave is 32 consecutive items; an item reads the row
// image at -(plane * az + 17 * ay + ax) + const.  Enumerated (ax, ay, az) -- x-runs of nine lanes,
// consecutive runs 17 floats apart -- the runs of ay and ay + 2 share seven banks: every read
// took two passes (half of the LDS's active cycles were conflicts, r03/r04 profiles).  Enumerated
// (ax, az, ay) with the image's PLANE stride padded from 289 to 297 (= 9 mod 32), consecutive
// runs sit 9 banks apart -- 0-8, 9-17, 18-26, 27-31 -- and conflicts remain only where a
// half-wave straddles the step from the last az of one ay to the first of the next.
// Measured (tools/time_s2.py, profiles/r04_j_s2_zruns.txt): 9^3 190 -> 166 ms at 128^3, 102 -> 84 ms
// at 96^3; 7^3 62.2 -> 64.7 ms at 140^3 -- so only 9^3 takes it.  At 7^3 the conflicts were as bad as at
// 9^3 -- SQ_LDS_BANK_CONFLICT 8.46e9 of SQ_LDS_IDX_ACTIVE 20.75e9, 41 % of the LDS cycles, at 140^3
// (profiles/r07_a_bench_flylight140_p7_pmc_sq.txt) -- and the z-runs do not remove them there: a tile is 8
// thick, so most rows have fewer than seven az (or ax) and the lattice of runs breaks; counted per row
// class on the CPU (tools/s2_bank_sim.py) the share of conflict passes is 0.44 for x-runs on strides
// 13 / 169, 0.38 at best for z-runs, 0.33 at best for any of the six enumerations on any pair of strides
// (x-runs, line stride 39, plane stride 529), 0.30 with the enumeration chosen per row, and 0.10 with x-runs
// padded to 8 lanes on a line stride of 40 -- which walks 1.4 x the chunks.  7^3 therefore deals its items
// BY BANK (rw_bankdeal, round 7): 0.20 predicted on the unchanged image with the dense number of chunks.  With all nine az present (rows in the z-interior of a tile at
// least 9 thick) the step to the next ay continues the lattice (81 = 17 mod 32 = the y stride):
// the 16 x 8 x 16 tile has half of its items in such rows.
static constexpr bool rw_zruns(int PX) { return PX == 9; }
// Round 7, 7^3: the items of a row are dealt to the lanes BY BANK (see rank_deal_table_kernel below).
static constexpr bool rw_bankdeal(int PX) { return PX == 7; }
static constexpr int RW_PAD = 8;
static constexpr int RW_WAVES = 4;     // waves per workgroup
// Round 14, the run-time-thickness kernel of 7^3 (DZ): its accumulators and bit arrays are sized by one of a few
// thicknesses RW_FIT_TZ (the plan takes the smallest >= the z step), so that 160 KB of LDS hold six workgroups
// and more where the old TZ = 16 sizing (29 KB) stopped at five.  The registers must then allow them too: six
// workgroups of four waves are six waves per SIMD, 80 VGPRs (see LAZY in the kernel).
static constexpr int RW_FIT_MINWAVES = 6;
static constexpr int RW_FIT_NTZ = 4;
static constexpr int RW_FIT_TZ[RW_FIT_NTZ] = {8, 10, 12, 16};
static constexpr int rw_fit_index(int tz_step) { return tz_step <= 8 ? 0 : (tz_step <= 10 ? 1 : (tz_step <= 12 ? 2 : 3)); }
// (the masks' layout -- rw_mask_words, rw_mask_quad0, RW_QSTRIDE, rw_mask_bytes, interleave16 -- is in
// ppp_rank_masks.hpp: the fused pre-pass of ppp_prepass.hip writes it too)
typedef const volatile __attribute__((address_space(3))) float *lds_f32_cvp2;

// acc + r * c with c a float16 in the low / high half of a register: the compiler selects
// v_fma_mix_f32 (op_sel picks the half; the float16 -> float32 conversion is exact and part of the
// fused operation, which rounds once)
typedef _Float16 rw_h2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float fma_mix_lo(float r, uint32_t c, float acc) {
    return __builtin_fmaf(r, (float)__builtin_bit_cast(rw_h2, c).x, acc);
}
__device__ __forceinline__ float fma_mix_hi(float r, uint32_t c, float acc) {
    return __builtin_fmaf(r, (float)__builtin_bit_cast(rw_h2, c).y, acc);
}

template <int I, int END>
struct StaticFor {
    template <class F>
    static __device__ __forceinline__ void run(F &&f) {
        f(std::integral_constant<int, I>{});
        StaticFor<I + 1, END>::run(f);
    }
};
template <int END>
struct StaticFor<END, END> {
    template <class F>
    static __device__ __forceinline__ void run(F &&) {}
};

// ---- pre-pass: interleaved masks, pair counts, border / background scores ------------------
// thread per centre of the score box; each centre's masks go to its slot of the row-of-16 layout
// (rw_mask_quad0), one 4-byte word at a time.  This is the pre-pass of a caller that brings no masks; a
// caller on the fused path (ppp_pred_prepass, ppp_prepass.hip) hands M / info / valid in and neither this
// kernel nor rank_valid2_kernel is launched (launch_rank_wg_prepared).
// Round 12: the cubic window P = 5 / 7 / 9 is compiled in (as PaGeo does for S5): the partner loop runs
// over (dz, dy, dx) with constant bounds -- no division per partner -- and reads the partner's validity from
// `valid`, which rank_valid2_kernel wrote one launch earlier, instead of evaluating pred[mid] > th && ov == 0
// again for each of the C partners.
template <typename T, int P>
__global__ void __launch_bounds__(256)
    rank_masks_il_kernel(const T *__restrict__ pred, const uint8_t *__restrict__ valid_v, const ppp_box sb,
                         uint32_t *__restrict__ M, uint32_t *__restrict__ info, float *__restrict__ score, const Geo G) {
    const int sX = sb.x1 - sb.x0, sY = sb.y1 - sb.y0, sZ = sb.z1 - sb.z0;
    const long long sbV = (long long)sX * sY * sZ;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= sbV) return;
    const int cx = sb.x0 + (int)(t % sX), cy = sb.y0 + (int)((t / sX) % sY), cz = sb.z0 + (int)(t / ((long long)sX * sY));
    const long long lc = vox(G, cz, cy, cx);
    const T *mid = pred + (long long)G.mid * G.V;
    uint32_t inf = 0;
    if (!interior(G, cz, cy, cx)) {
        score[lc] = G.norm_rank ? -1.0f : -9999999.0f;
    } else if (!(ldf(mid, lc) > G.th_gt)) {
        score[lc] = 0.0f;   // the reference leaves the allocation's zero
    } else {
        const int words16 = (G.C + 15) / 16;
        const long long q0 = rw_mask_quad0(t / sX, (int)(t % sX), sX, rw_mask_words(G.C) / 4);
        unsigned nP = 0, nV = 0;
        int r = 0;
        constexpr int R = P / 2, C = P * P * P;
        uint32_t p = 0, n = 0;
        for (int dz = 0; dz < P; ++dz)
            for (int dy = 0; dy < P; ++dy) {
                const uint8_t *vrow = valid_v + vox(G, cz + dz - R, cy + dy - R, cx - R);
#pragma unroll
                for (int dx = 0; dx < P; ++dx, ++r) {
                    const bool valid = vrow[dx] != 0;
                    const float val = ldf(pred, (long long)r * G.V + lc);
                    const int b = r & 15;
                    if (valid) ++nV;
                    if (valid && val > G.th_gt) p |= 1u << b;
                    if (valid && val < G.bg_lt) n |= 1u << b;
                    if (b == 15 || r == C - 1) {
                        const int w = r >> 4;
                        M[(q0 + (long long)(w >> 2) * RW_QSTRIDE) * 4 + (w & 3)] = interleave16(p, n);
                        nP += __popc(p);
                        p = n = 0;
                    }
                }
            }
        for (int w = words16; w < rw_mask_words(G.C); ++w) M[(q0 + (long long)(w >> 2) * RW_QSTRIDE) * 4 + (w & 3)] = 0u;
        // fgCnt = |P| (|V| - 1) - |P| (|P| - 1) / 2   (rankPatches.cu:139, see ppp_rank_v2.hip)
        const unsigned fg_cnt = nP ? nP * (nV - 1u) - nP * (nP - 1u) / 2u : 0u;
        inf = 0x80000000u | fg_cnt;
        if (nP == 0) score[lc] = 0.0f;   // no first pixel: acc = 0, 0 / max(1, 0)
    }
    info[t] = inf;
}

template <typename T>
__global__ void __launch_bounds__(256)
    rank_valid2_kernel(const T *__restrict__ pred, const uint8_t *__restrict__ ov, uint8_t *__restrict__ valid,
                       const Geo G) {
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= G.V) return;
    valid[v] = (ldf(pred, (long long)G.mid * G.V + v) > G.th_gt && (!G.use_overlap || ov[v] == 0)) ? 1 : 0;
}

// ---- heavy tiles first (round 5) -----------------------------------------------------------
// A launch ends with its slowest workgroup, and the tiles of centres differ: by the valid voxels
// of their grown box (rows walked) and by their foreground centres (items with work).  On a 264^2
// column one round of 1 024 workgroups takes 146 ms, every further round 64 ms
// (profiles/r05_zl_s2_rounds.txt) -- the dispatcher hands out blocks in index order, so with the
// tiles in spatial order the heavy ones of the LAST round decide the end.  Launches of up to
// RW_ORDER_MAX tiles are therefore dealt heaviest first; every XCD keeps its contiguous range of
// tiles (neighbours share rows in its L2) and walks it in descending order of weight.
// order[slot] = tile, or -1 for the padding slots.
static constexpr int RW_ORDER_MAX = 16384;
// Tile number -> (tz, ty, tx).  Round 6: Y-MAJOR numbering (y_major = 1).  Every XCD takes a contiguous range
// of tile numbers; numbered z-major, XCD 0 held the launch's lowest z-tiles and XCD 7 its highest, and a
// launch's z-edge tiles run ~20 % longer than its inner ones -- per-workgroup start / end stamps
// (tools/s2_wg_times.py, profiles/r06_h*): the XCDs of a 2 048-tile launch finished between 134 and 178 ms.
// Numbered y-major an XCD's range is a slab of y-tiles with EVERY z-tile in it (and z-neighbours, which
// share half of their rows, still meet in one L2).  PPP_RANK_TILE_MAJOR=z: the old numbering.
__device__ __forceinline__ void rw_tile_decode(int bid, int n_tiles, int tiles_y, int tiles_x, int y_major,
                                               int &tz_i, int &ty_i, int &tx_i) {
    tx_i = bid % tiles_x;
    if (y_major) {
        const int tiles_z = n_tiles / (tiles_y * tiles_x);
        tz_i = (bid / tiles_x) % tiles_z;
        ty_i = bid / (tiles_x * tiles_z);
    } else {
        ty_i = (bid / tiles_x) % tiles_y;
        tz_i = bid / (tiles_x * tiles_y);
    }
}
// weight of a tile = the chunks of 64 items its workgroup walks: over the VALID voxels u of the tile
// grown by the radius, ceil(items of u / 64) (+ 1 for the row's staging and barriers); 0 without an
// active centre (the workgroup leaves at once).
__global__ void __launch_bounds__(256)
    rank_tile_weight_kernel(const uint32_t *__restrict__ info, const uint8_t *__restrict__ valid, const ppp_box sb,
                            const int TZ, const int TY, const int TX, const int tiles_y, const int tiles_x,
                            const int y_major, int32_t *__restrict__ weight, const Geo G) {
    const int bid = blockIdx.x;
    int tx_i, ty_i, tz_i;
    rw_tile_decode(bid, (int)gridDim.x, tiles_y, tiles_x, y_major, tz_i, ty_i, tx_i);
    const int sX = sb.x1 - sb.x0, sY = sb.y1 - sb.y0, sZ = sb.z1 - sb.z0;
    int c = 0, w = 0;
    for (int cl = threadIdx.x; cl < TZ * TY * TX; cl += blockDim.x) {
        const int z = tz_i * TZ + cl / (TX * TY), y = ty_i * TY + (cl / TX) % TY, x = tx_i * TX + cl % TX;
        if (z < sZ && y < sY && x < sX) c += (int)(info[((long long)z * sY + y) * sX + x] >> 31);
    }
    const int c0z = sb.z0 + tz_i * TZ, c0y = sb.y0 + ty_i * TY, c0x = sb.x0 + tx_i * TX;
    const int tz = min(TZ, sb.z1 - c0z), ty = min(TY, sb.y1 - c0y), tx = min(TX, sb.x1 - c0x);
    const int uz0 = max(c0z - G.rz, G.bz0), uz1 = min(c0z + tz - 1 + G.rz, G.bz0 + G.bZ - 1);
    const int uy0 = max(c0y - G.ry, G.by0), uy1 = min(c0y + ty - 1 + G.ry, G.by0 + G.bY - 1);
    const int ux0 = max(c0x - G.rx, G.bx0), ux1 = min(c0x + tx - 1 + G.rx, G.bx0 + G.bX - 1);
    const int nuy = uy1 - uy0 + 1, nux = ux1 - ux0 + 1, nu = (uz1 - uz0 + 1) * nuy * nux;
    for (int k = threadIdx.x; k < nu; k += blockDim.x) {
        const int uz = uz0 + k / (nuy * nux), uy = uy0 + (k / nux) % nuy, ux = ux0 + k % nux;
        if (!valid[vox(G, uz, uy, ux)]) continue;
        const int nz = min(G.pz - 1, uz + G.rz - c0z) - max(0, uz + G.rz - (c0z + tz - 1)) + 1;
        const int ny = min(G.py - 1, uy + G.ry - c0y) - max(0, uy + G.ry - (c0y + ty - 1)) + 1;
        const int nx = min(G.px - 1, ux + G.rx - c0x) - max(0, ux + G.rx - (c0x + tx - 1)) + 1;
        if (nz > 0 && ny > 0 && nx > 0) w += (nz * ny * nx + 63) / 64 + 1;
    }
    for (int o = 32; o > 0; o >>= 1) { c += __shfl_xor(c, o); w += __shfl_xor(w, o); }
    __shared__ int part[2][4];
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = c; part[1][threadIdx.x >> 6] = w; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int cs = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        const int ws = part[1][0] + part[1][1] + part[1][2] + part[1][3];
        weight[bid] = cs ? ws : 0;
    }
}
// one workgroup per XCD range: its tiles in descending order of weight (position = the number of tiles
// of the range that come before: heavier, or as heavy with a smaller index).
// Round 7, split tiles: the `splits` lightest tiles of the range -- those that the dispatcher hands out last,
// into the launch's part-filled last round -- become two RECORDS each, the tile's lower and upper half in y
// (the kernel takes ragged tiles, a half is a tile of TY / 2 lines), weighed at half the tile; the records
// are dealt heaviest first.  record = tile | RW_HALF_LO / RW_HALF_HI; an XCD's range
// of the order array has per_xcd + splits slots.
static constexpr int32_t RW_HALF_LO = 1 << 28, RW_HALF_HI = 2 << 28, RW_TILE_MASK = (1 << 28) - 1;
// Round 12, ranges of equal WEIGHT (by_weight; PPP_RANK_WG_XCD=weight): the y-major tile sequence is cut where
// the prefix sum of the weights passes k / 8 of the total instead of every per_xcd tiles -- the y-edge slabs of
// the numbering are light, so their XCDs take more tiles.  The ranges stay contiguous (neighbours meet in one
// L2) and heaviest first inside.  The grid is made before the weights exist: an XCD's part of the order array
// has `slots` entries, so a range is clamped to cap = slots - splits tiles (and to what the ranges after it
// can still hold: cap >= per_xcd, so every tile finds a slot).  Every workgroup works out all eight cuts.
__global__ void __launch_bounds__(256)
    rank_tile_order_kernel(const int32_t *__restrict__ weight, const int n_tiles, const int per_xcd, const int splits,
                           const int slots, const int by_weight, int32_t *__restrict__ order) {
    __shared__ int32_t w[RW_ORDER_MAX / 8 + 8];
    __shared__ int32_t key[RW_ORDER_MAX / 8 + 8];      // weight of the tile's records; bit 30: the tile is split
    __shared__ int part_sum[256];
    __shared__ int cut[9];
    int lo = blockIdx.x * per_xcd, hi = min(lo + per_xcd, n_tiles);
    if (by_weight) {
        // chunk sums, then cut k = the first tile at which the running weight reaches k / 8 of the total
        const int ch = (n_tiles + 255) / 256;
        int ps = 0;
        for (int i = threadIdx.x * ch; i < min((threadIdx.x + 1) * ch, n_tiles); ++i) ps += weight[i];
        part_sum[threadIdx.x] = ps;
        __syncthreads();
        if (threadIdx.x < 9) {
            long long total = 0;
            for (int c = 0; c < 256; ++c) total += part_sum[c];
            int at = threadIdx.x == 8 ? n_tiles : 0;
            if (threadIdx.x > 0 && threadIdx.x < 8) {
                const long long want = (total * threadIdx.x + 7) / 8;
                long long run = 0;
                int c = 0;
                while (c < 256 && run + part_sum[c] < want) run += part_sum[c++];
                at = min(c * ch, n_tiles);
                while (at < n_tiles && run < want) run += weight[at++];
            }
            cut[threadIdx.x] = at;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cap = min(slots - splits, RW_ORDER_MAX / 8);
            for (int k = 1; k < 8; ++k)
                cut[k] = min(max(max(cut[k], cut[k - 1]), n_tiles - (8 - k) * cap), cut[k - 1] + cap);
        }
        __syncthreads();
        lo = cut[blockIdx.x]; hi = cut[blockIdx.x + 1];
    }
    const int n = max(hi - lo, 0);
    const int slot0 = blockIdx.x * slots;
    for (int i = threadIdx.x; i < n; i += blockDim.x) w[i] = weight[lo + i];
    for (int t = threadIdx.x; t < slots; t += blockDim.x) order[slot0 + t] = -1;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int wi = w[i];
        int before = 0, with_work = 0;
        for (int j = 0; j < n; ++j) {
            before += (w[j] > wi || (w[j] == wi && j < i)) ? 1 : 0;
            with_work += w[j] > 0 ? 1 : 0;
        }
        // (the tiles without work rank last and leave at once: the lightest WITH work are split)
        key[i] = (wi > 0 && before >= with_work - splits) ? (((wi + 1) >> 1) | (1 << 30)) : wi;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int ki = key[i] & ~(1 << 30);
        int before = 0;
        for (int j = 0; j < n; ++j) {
            const int kj = key[j] & ~(1 << 30), cj = (key[j] >> 30) + 1;
            before += (kj > ki || (kj == ki && j < i)) ? cj : 0;
        }
        if (key[i] >> 30) {
            order[slot0 + before] = (lo + i) | RW_HALF_LO;
            order[slot0 + before + 1] = (lo + i) | RW_HALF_HI;
        } else {
            order[slot0 + before] = lo + i;
        }
    }
    // (fewer records than slots where the range is short or has fewer tiles with work than `splits`: the
    // slots are cleared first, the records written after the barrier)

}

// ---- items dealt by bank (round 7) -----------------------------------------------------------
// A lane reads the row image at base - (az SZ + ay SY + ax) + immediate: the banks of one read are those of
// the lanes' (ax + SY ay + SZ az) mod 32, whatever the partner.  A row of a tile is a box of nx x ny x nz
// items, n = 1 .. P per axis (P only where the voxel lies at least the radius inside the tile): P^3 classes
// of rows.  For every class this kernel writes which item the lane of slot i0 + lane takes: lane l of a
// half-wave takes items of bank class l -- half-wave k the k-th such item in (az, ay) order -- so a
// half-wave is conflict-free by construction.  The row keeps its dense number of chunks, ceil(n / 64): where
// a bank class holds more items than the row has half-waves, the surplus goes, in order, to the lanes left
// empty (each costs its half-wave one further pass -- far less than a chunk more for the whole wave).
// tools/s2_bank_sim.py restates this dealing and counts the passes.
// entry: bit 15 = the slot holds an item, az << 8 | ay << 4 | ax relative to the row's first item.
static constexpr int rw_deal_slots(int P) { return (P * P * P + 63) / 64 * 64; }
static size_t rw_deal_bytes(int P) { return rw_bankdeal(P) ? (size_t)P * P * P * rw_deal_slots(P) * 2 : 0; }
template <int P>
__global__ void __launch_bounds__(32) rank_deal_table_kernel(uint16_t *__restrict__ T, const int SY, const int SZ) {
    constexpr int SLOTS = rw_deal_slots(P), MAXOVER = 16;
    __shared__ uint16_t slot[SLOTS];
    __shared__ uint16_t over[32][MAXOVER];
    __shared__ int n_over[32];
    const int cls = blockIdx.x, r = threadIdx.x;
    const int nx = cls % P + 1, ny = (cls / P) % P + 1, nz = cls / (P * P) + 1;
    const int H = (nx * ny * nz + 63) / 64 * 2;
    for (int i = r; i < SLOTS; i += 32) slot[i] = 0;
    __syncthreads();
    int k = 0;
    for (int az = 0; az < nz; ++az)
        for (int ay = 0; ay < ny; ++ay) {
            const int ax = (r - SY * ay - SZ * az) & 31;
            if (ax >= nx) continue;
            const uint16_t e = (uint16_t)(0x8000 | (az << 8) | (ay << 4) | ax);
            if (k < H) slot[32 * k + r] = e;
            else if (k - H < MAXOVER) over[r][k - H] = e;     // (a class holds at most ceil(P^3 / 32) + 1 items)
            ++k;
        }
    n_over[r] = k > H ? min(k - H, MAXOVER) : 0;
    __syncthreads();
    if (r == 0) {
        int f = 0;
        for (int rr = 0; rr < 32; ++rr)
            for (int o = 0; o < n_over[rr]; ++o) {
                while (f < 32 * H && slot[f] != 0) ++f;
                if (f < 32 * H) slot[f] = over[rr][o];
            }
    }
    __syncthreads();
    for (int i = r; i < SLOTS; i += 32) T[(size_t)cls * SLOTS + i] = slot[i];
}

// ---- main kernel ---------------------------------------------------------------------------
// DZ (round 12): the tile's thickness in z is the run-time `tz_step` <= TZ -- TZ then only sizes accs, act_bits and
// uvalid_bits (round 14: the smallest of RW_FIT_TZ that holds tz_step); the tile origin is tz_i * tz_step and the kernel's ragged-tile handling does the rest.  !DZ:
// tz_step is TZ (the launches that do not choose their thickness keep their code).
// MINW (round 14): the waves per SIMD the registers must allow -- RW_MINWAVES for every launch but the DZ one
// (RW_FIT_MINWAVES).
//
// The LDS arrays of an instantiation, in elements, and their bytes as the plan counts them (every array rounded up to
// 16 bytes: an upper bound of the kernel's group segment, which tools/kernel_regs.py prints).
template <int P, int TZ, int TY, int TX>
struct RwLds {
    static constexpr int W1 = 2 * P - 1, SZ = W1 * W1;
    static constexpr int SZP = rw_zruns(P) ? SZ + ((9 - SZ % 32) + 32) % 32 : SZ;      // plane stride of the row image (see rw_zruns)
    static constexpr int ROW = W1 * SZP + 2 * RW_PAD;
    static constexpr int NT = TZ * TY * TX;
    static constexpr int ACT = (NT + 31) / 32;
    static constexpr int UB = (TZ + 2 * (P / 2)) * (TY + 2 * (P / 2)) * (TX + 2 * (P / 2));
    static constexpr int UV = (UB + 63) / 64 * 2;
    static constexpr int up16(int b) { return (b + 15) & ~15; }
    static constexpr int bytes = up16(4 * ROW) + up16(4 * NT) + up16(4 * ACT) + 256 * 8 + up16(4 * UV) + 16;
};
static constexpr int RW_LDS_PER_CU = 160 * 1024;

template <int PZ, int PY, int PX, int TZ, int TY, int TX, bool DZ = false, int MINW = RW_MINWAVES>
__global__ void __launch_bounds__(64 * RW_WAVES, MINW)
    rank_wg_kernel(const float *__restrict__ S, const uint32_t *__restrict__ M,
                   const uint32_t *__restrict__ info, const uint8_t *__restrict__ valid,
                   float *__restrict__ score, const ppp_box sb, const Geo G, const int tiles_y,
                   const int tiles_x, const int n_tiles, const int32_t *__restrict__ order, const int y_major, const uint16_t *__restrict__ dealT,
                   const int tz_step
#ifdef PPP_RW_STAMPS
                   , uint32_t *__restrict__ stamps
#endif
                   ) {
#ifdef PPP_RW_STAMPS
    // (diagnostic build -DPPP_RW_STAMPS, tools/s2_wg_times.py: when does every workgroup start and
    // end, and on which CU -- the tile weights' array of the workspace is free once the order is made)
    // (wall_clock64: the 100 MHz counter the whole device shares -- the cycle counter is a clock per CU)
    const unsigned long long t_start = wall_clock64();
#endif
    constexpr int C = PZ * PY * PX, W16 = (C + 15) / 16, RZ = PZ / 2, RY = PY / 2, RX = PX / 2;
    constexpr int W16P = rw_mask_words(C);   // mask words per centre in M
    constexpr int NMW = W16;                 // ... that hold bits
    constexpr int WZ = 2 * PZ - 1, WY = 2 * PY - 1, WX = 2 * PX - 1, W = WZ * WY * WX, LC = (W - 1) / 2;
    constexpr int NTHR = 64 * RW_WAVES;
    constexpr int NST = (W + NTHR - 1) / NTHR;
    constexpr int NT = TZ * TY * TX;
    constexpr int UB = (TZ + 2 * RZ) * (TY + 2 * RY) * (TX + 2 * RX);
    // plane stride of the row image (see rw_zruns)
    constexpr int SZ = WY * WX;
    constexpr int SZP = rw_zruns(PX) ? SZ + ((9 - SZ % 32) + 32) % 32 : SZ;
    constexpr int LCP = LC + (PZ - 1) * (SZP - SZ);
    auto img = [](int e) -> int { return SZP == SZ ? e : (e / SZ) * SZP + e % SZ; };
    using Lds = RwLds<PX, TZ, TY, TX>;
    static_assert(PZ == PX && PY == PX && Lds::ROW == WZ * SZP + 2 * RW_PAD && Lds::NT == NT && Lds::UB == UB, "RwLds restates these arrays");
    __shared__ float rowbuf[Lds::ROW];
    __shared__ float accs[Lds::NT];
    __shared__ uint32_t act_bits[Lds::ACT];
    __shared__ uint2 coefT[256];
    __shared__ uint32_t uvalid_bits[Lds::UV];
    __shared__ int any_act;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sX = sb.x1 - sb.x0, sY = sb.y1 - sb.y0, sZ = sb.z1 - sb.z0;
    const long long sbV = (long long)sX * sY * sZ;
    // XCD-aware order: consecutive blocks go to different XCDs; give each XCD a contiguous range
    // of tiles so that x-neighbours (which share a third of their rows) meet in one L2
    const int n_blocks = gridDim.x;
    const int per_xcd = (n_blocks + 7) / 8;
    const int slot = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    // (heavy tiles first within the XCD's range when the launcher made an order)
    const int rec = order ? order[slot] : slot;
    if (rec < 0) return;
    // (a record of the order is a tile or, round 7, the lower / upper half in y of a split tile)
    const int bid = rec & RW_TILE_MASK, half_hi = (rec & RW_HALF_HI) ? 1 : 0, halved = (rec & (RW_HALF_LO | RW_HALF_HI)) ? 1 : 0;
    if (bid >= n_tiles) return;
    int tx_i, ty_i, tz_i;
    rw_tile_decode(bid, n_tiles, tiles_y, tiles_x, y_major, tz_i, ty_i, tx_i);
    const int tzs = DZ ? min(tz_step, TZ) : TZ;
    const int c0z = sb.z0 + tz_i * tzs, c0y = sb.y0 + ty_i * TY + half_hi * (TY / 2), c0x = sb.x0 + tx_i * TX;
    const int tz = min(tzs, sb.z1 - c0z), ty = min(halved ? TY / 2 : TY, sb.y1 - c0y), tx = min(TX, sb.x1 - c0x);
    if (tz <= 0 || ty <= 0 || tx <= 0) return;

    auto sb_index = [&](int lz, int ly, int lx) -> long long {
        return ((long long)(c0z + lz - sb.z0) * sY + (c0y + ly - sb.y0)) * sX + (c0x + lx - sb.x0);
    };
    // coefficient table: entry e -> four float16 {+2^-5 (P bit), -2^-5 (N bit), 0}
    for (int e = tid; e < 256; e += NTHR) {
        uint32_t h[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = ((e >> i) & 1) ? 0x2800u : (((e >> (4 + i)) & 1) ? 0xA800u : 0u);
        coefT[e] = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
    }
    if (tid == 0) any_act = 0;
    __syncthreads();
    static_assert(NT % 64 == 0 && (TY * TX) % 64 == 0, "tile size must be a multiple of the wave size");
    const int nt_used = DZ ? tz * TY * TX : NT;      // (a multiple of 64 either way)
    for (int cl = tid; cl < nt_used; cl += NTHR) {
        const int lx = cl % TX, ly = (cl / TX) % TY, lz = cl / (TX * TY);
        uint32_t v = 0;
        if (lz < tz && ly < ty && lx < tx) v = info[sb_index(lz, ly, lx)];
        const unsigned long long m = __ballot((v >> 31) != 0);
        if (lane == 0) {
            act_bits[cl >> 5] = (uint32_t)m; act_bits[(cl >> 5) + 1] = (uint32_t)(m >> 32);
            if (m) any_act = 1;
        }
        accs[cl] = 0.0f;
    }
    __syncthreads();
    if (!any_act) return;

    const long long rsY = G.bX, rsZ = (long long)G.bX * G.bY;
    const int uz0 = max(c0z - RZ, G.bz0), uz1 = min(c0z + tz - 1 + RZ, G.bz0 + G.bZ - 1);
    const int uy0 = max(c0y - RY, G.by0), uy1 = min(c0y + ty - 1 + RY, G.by0 + G.bY - 1);
    const int ux0 = max(c0x - RX, G.bx0), ux1 = min(c0x + tx - 1 + RX, G.bx0 + G.bX - 1);
    const int nuy = uy1 - uy0 + 1, nux = ux1 - ux0 + 1, nu = (uz1 - uz0 + 1) * nuy * nux;
    for (int k0 = 64 * wave; k0 < nu; k0 += NTHR) {
        const int k = k0 + lane;
        const bool ok = k < nu && valid[vox(G, uz0 + k / (nuy * nux), uy0 + (k / nux) % nuy, ux0 + k % nux)] != 0;
        const unsigned long long m = __ballot(ok);
        if (lane == 0) { uvalid_bits[k0 >> 5] = (uint32_t)m; uvalid_bits[(k0 >> 5) + 1] = (uint32_t)(m >> 32); }
    }
    __syncthreads();
    auto next_valid = [&](int k) -> int {
        while (k < nu) {
            const uint32_t wbits = uvalid_bits[k >> 5] >> (k & 31);
            if (wbits) return k + __builtin_ctz(wbits);
            k = (k | 31) + 1;
        }
        return nu;
    };
    auto row_src = [&](int k) -> const float * {
        const int uz = uz0 + k / (nuy * nux), uy = uy0 + (k / nux) % nuy, ux = ux0 + k % nux;
        return S + (((long long)row_slice(G, uz) * rsZ + (long long)(uy - G.by0) * rsY + (ux - G.bx0)) * W);
    };
    float st[NST];
    int uk = __builtin_amdgcn_readfirstlane(next_valid(0));
    if (uk < nu) {
        const float *src = row_src(uk);
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int e = tid + i * NTHR;
            if (e < W) rowbuf[RW_PAD + img(e)] = src[e] * 32.0f;
        }
    }
    __syncthreads();
    int turn = 0;   // rotates the wave that takes the first chunk of a row
    // geometry of a row (which pixels a of voxel u have their centre in the tile) and of the item a
    // lane takes in chunk i0 of it
    struct RowG { int uz, uy, ux, az0, ay0, ax0, nz, ny, nx, n_box, cls; };
    struct ItemG { bool in; int cl, a, az, ay, ax; long long t, q0; };
    auto row_geom = [&](int k) -> RowG {
        RowG r;
        r.uz = uz0 + k / (nuy * nux); r.uy = uy0 + (k / nux) % nuy; r.ux = ux0 + k % nux;
        r.az0 = max(0, r.uz + RZ - (c0z + tz - 1));
        r.ay0 = max(0, r.uy + RY - (c0y + ty - 1));
        r.ax0 = max(0, r.ux + RX - (c0x + tx - 1));
        r.nz = min(PZ - 1, r.uz + RZ - c0z) - r.az0 + 1;
        r.ny = min(PY - 1, r.uy + RY - c0y) - r.ay0 + 1;
        r.nx = min(PX - 1, r.ux + RX - c0x) - r.ax0 + 1;
        r.n_box = (r.nz <= 0 || r.ny <= 0 || r.nx <= 0) ? 0 : r.nz * r.ny * r.nx;
        r.cls = r.n_box ? ((r.nz - 1) * PY + (r.ny - 1)) * PX + (r.nx - 1) : 0;      // (its class in the dealing table)
        return r;
    };
    auto item_geom = [&](const RowG &r, int i0) -> ItemG {
        ItemG g;
        const int i = i0 + lane;
        if constexpr (rw_bankdeal(PX)) {
            // (dealt by bank: i0 + lane < 64 ceil(n_box / 64) <= the slots of a class; an empty slot reads
            // the row's first item, like a lane beyond the row in the enumeration below)
            const uint32_t e = dealT[r.cls * rw_deal_slots(PX) + i];
            g.in = (e >> 15) != 0;
            g.ax = r.ax0 + (int)(e & 15u); g.ay = r.ay0 + (int)((e >> 4) & 15u); g.az = r.az0 + (int)((e >> 8) & 15u);
        } else {
        g.in = i < r.n_box;
        const int ii = g.in ? i : 0;
        g.ax = r.ax0 + ii % r.nx;
        g.ay = rw_zruns(PX) ? r.ay0 + ii / (r.nx * r.nz) : r.ay0 + (ii / r.nx) % r.ny;
        g.az = rw_zruns(PX) ? r.az0 + (ii / r.nx) % r.nz : r.az0 + ii / (r.nx * r.ny);
        }
        const int lz = r.uz + RZ - g.az - c0z, ly = r.uy + RY - g.ay - c0y, lx = r.ux + RX - g.ax - c0x;
        g.cl = (lz * TY + ly) * TX + lx;
        g.a = (g.az * PY + g.ay) * PX + g.ax;
        g.t = sb_index(lz, ly, lx);     // (nothing reads it: without it the compiler allocates other registers)
        // (quad 0 of the centre's masks, in 16-byte units)
        g.q0 = rw_mask_quad0((long long)(c0z + lz - sb.z0) * sY + (c0y + ly - sb.y0), c0x + lx - sb.x0, sX, W16P / 4);
        return g;
    };
    while (uk < nu) {
        const int uk_next = __builtin_amdgcn_readfirstlane(next_valid(uk + 1));
        if (uk_next < nu) {
            const float *src = row_src(uk_next);
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                const int e = tid + i * NTHR;
                st[i] = e < W ? src[e] : 0.0f;
            }
        }
        // pixels a of this voxel whose centre c = u + R - a lies in the tile
        const RowG R = row_geom(uk);
        const int n_box = R.n_box;
        const int first = (wave + RW_WAVES - turn) % RW_WAVES;
        turn = (turn + ((n_box + 63) >> 6)) % RW_WAVES;
        for (int i0 = 64 * first; i0 < n_box; i0 += NTHR) {
            const ItemG it = item_geom(R, i0);
            const int ax = it.ax, ay = it.ay, az = it.az, cl = it.cl, a = it.a;
            const long long q0 = it.q0;
            bool active = it.in && ((act_bits[cl >> 5] >> (cl & 31)) & 1u) != 0;
            uint32_t mw[NMW];
            // is a in P?  P bit of partner s: bit 8 (s >> 2 & 3) + (s & 3) of word s >> 4
            if (active)
                active = ((M[(q0 + (long long)(a >> 6) * RW_QSTRIDE) * 4 + ((a >> 4) & 3)] >> (8 * ((a >> 2) & 3) + (a & 3))) & 1u) != 0;
            if (__ballot(active) == 0) continue;
            // (unconditional loads -- t is a centre of the tile for every lane -- then one select
            // per word: a predicated load is a branch per word)
            const uint4 *mc = reinterpret_cast<const uint4 *>(M) + q0;
            // LAZY (round 14, the six-waves-per-SIMD build): a quad of mask words is loaded one quad ahead of its
            // terms instead of all six before the first term -- 8 instead of 22 registers hold masks: 80 VGPRs and
            // nothing spilled (with the six loads up front: 80 and 10 spilled around the term loop, 66 against 48 ms;
            // two quads ahead: 3 spilled)
            constexpr bool LAZY = DZ && MINW > RW_MINWAVES;
            auto load_quad = [&](auto qc) {
                constexpr int q = decltype(qc)::value;
                const uint4 v = mc[q * RW_QSTRIDE];
                if (4 * q < NMW) mw[4 * q] = active ? v.x : 0u;
                if (4 * q + 1 < NMW) mw[4 * q + 1] = active ? v.y : 0u;
                if (4 * q + 2 < NMW) mw[4 * q + 2] = active ? v.z : 0u;
                if (4 * q + 3 < NMW) mw[4 * q + 3] = active ? v.w : 0u;
            };
            if constexpr (LAZY) {
                load_quad(std::integral_constant<int, 0>{});
            } else {
#pragma unroll
            for (int q = 0; q < W16P / 4; ++q) {
                const uint4 v = mc[q * RW_QSTRIDE];
                if (4 * q < NMW) mw[4 * q] = v.x;
                if (4 * q + 1 < NMW) mw[4 * q + 1] = v.y;
                if (4 * q + 2 < NMW) mw[4 * q + 2] = v.z;
                if (4 * q + 3 < NMW) mw[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int w = 0; w < W16; ++w) mw[w] = active ? mw[w] : 0u;
            }
            float acc = active ? accs[cl] : 0.0f;
            lds_f32_cvp2 row = (lds_f32_cvp2)(rowbuf + RW_PAD + LCP - (az * SZP + ay * WX + ax));
            // (one copy of the row pointer per read of a group: with a single pointer the compiler emits other code)
            lds_f32_cvp2 rowc[4];
#pragma unroll
            for (int i2 = 0; i2 < 4; ++i2) rowc[i2] = row;
            const int aw = a >> 4;
            // b in P counts only for b > a: P bits of the partners <= a go (N bits stay)
            const uint32_t above16 = ~((2u << (a & 15)) - 1u) & 0xFFFFu;
            const uint32_t keep_a = interleave16(above16, 0xFFFFu);
            // (a compile-time recursion, not a loop: at 9^3 the 46 x 16 terms exceed the size up to
            // which the compiler honours an unroll pragma, and a rolled loop computes every LDS
            // offset at run time)
            StaticFor<0, W16>::run([&](auto wc) {
                constexpr int w = decltype(wc)::value;
                if constexpr (LAZY && w % 4 == 0 && w / 4 + 1 < W16P / 4) load_quad(std::integral_constant<int, w / 4 + 1>{});
                const uint32_t m = mw[w] & (w < aw ? 0xF0F0F0F0u : (w > aw ? 0xFFFFFFFFu : keep_a));
                if (__ballot(m != 0u) == 0) return;
                // table reads of the word first; then the four groups of four partners, the row
                // values of the next group in flight while the current chain runs
                uint2 cf[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (w * 16 + j * 4 < C) cf[j] = coefT[(m >> (8 * j)) & 0xFFu];
                float rv[2][4];
                // (the reads of a group are issued LAST ELEMENT FIRST: the LDS returns in order, so the
                // wait of the group's first term covers the other three -- one s_waitcnt per group
                // instead of one per term, and an s_waitcnt costs its wave an issue slot like any
                // instruction)
                auto load_rows = [&](int j, float (&r)[4]) {
#pragma unroll
                    for (int i3 = 0; i3 < 4; ++i3) {
                        const int i2 = 3 - i3;
                        const int b = w * 16 + j * 4 + i2;
                        if (b < C) r[i2] = rowc[i2][(b / (PY * PX)) * SZP + ((b / PX) % PY) * WX + b % PX];
                    }
                };
                load_rows(0, rv[0]);
                if (w * 16 + 4 < C) load_rows(1, rv[1]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (w * 16 + j * 4 < C) {
                        float r0[4];
#pragma unroll
                        for (int i2 = 0; i2 < 4; ++i2) r0[i2] = rv[j & 1][i2];
                        if (j + 2 < 4 && w * 16 + (j + 2) * 4 < C) load_rows(j + 2, rv[j & 1]);
#pragma unroll
                        for (int i2 = 0; i2 < 4; ++i2) {
                            const int b = w * 16 + j * 4 + i2;
                            if (b < C) {
                                const uint32_t c2 = i2 < 2 ? cf[j].x : cf[j].y;
                                acc = (i2 & 1) ? fma_mix_hi(r0[i2], c2, acc) : fma_mix_lo(r0[i2], c2, acc);
                            }
                        }
                    }
                }
            });
            if (active) accs[cl] = acc;
        }
        // ---- publish the next row
        __syncthreads();
        if (uk_next < nu) {
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                const int e = tid + i * NTHR;
                if (e < W) rowbuf[RW_PAD + img(e)] = st[i] * 32.0f;
            }
        }
        __syncthreads();
        uk = uk_next;
    }
    // ---- scores of the tile
    for (int cl = tid; cl < nt_used; cl += NTHR) {
        const int lx = cl % TX, ly = (cl / TX) % TY, lz = cl / (TX * TY);
        if (lz < tz && ly < ty && lx < tx && ((act_bits[cl >> 5] >> (cl & 31)) & 1u)) {
            const unsigned fg_cnt = info[sb_index(lz, ly, lx)] & 0x7FFFFFFFu;
            const float acc = accs[cl];
            score[vox(G, c0z + lz, c0y + ly, c0x + lx)] = G.norm_rank ? acc / (float)(fg_cnt > 1u ? fg_cnt : 1u) : acc;
        }
    }
#ifdef PPP_RW_STAMPS
    if (tid == 0 && stamps && blockIdx.x < RW_ORDER_MAX / 4) {
        const unsigned long long t_end = wall_clock64();
        unsigned hw_id;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
        unsigned xcc_id;          // (the tool reports per XCD)
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
        stamps[4 * blockIdx.x + 0] = (uint32_t)t_start;     // (10 ns units: 32 bits hold 42 s)
        stamps[4 * blockIdx.x + 1] = (uint32_t)t_end;
        stamps[4 * blockIdx.x + 2] = hw_id;
        stamps[4 * blockIdx.x + 3] = (uint32_t)bid | ((xcc_id & 0xFu) << 24) | ((uint32_t)halved << 23);
    }
#endif
}

bool rank_wg_supported(const Geo &G) {
    static EnvSwitch wg_sw("PPP_RANK_WG");
    const bool off = wg_sw.get() && wg_sw.get()[0] == '0';
    if (off) return false;       // (PPP_RANK_WG=0: the one-wave kernel of ppp_rank_vm.hip, read once)
    return G.pz == G.py && G.py == G.px && (G.px == 5 || G.px == 7 || G.px == 9) && !G.count_pos_neg &&
           G.layout == PPP_CONS_VOXEL_MAJOR;
}

struct RankWgWork {
    uint32_t *M, *info;       // the masks of the score box (rw_mask_bytes); [score box]
    uint8_t *valid;           // [V]
    int32_t *weight, *order;  // [RW_ORDER_MAX] each; a PPP_RW_STAMPS build reuses `weight` for its stamps
    uint16_t *dealT;          // rw_deal_bytes
};
// the launch's own part (a caller that hands the masks in brings only this: rank_wg_prepared_workspace_bytes)
static void rank_wg_sched_layout(Carver &c, const Geo &G, RankWgWork &W) {
    W.weight = c.take<int32_t>(RW_ORDER_MAX);
    W.order = c.take<int32_t>(RW_ORDER_MAX);
    W.dealT = (uint16_t *)c.take_bytes(rw_deal_bytes(G.px));
}
static RankWgWork rank_wg_layout(Carver &c, const ppp_box &sb, const Geo &G) {
    const RankMasks m = rank_masks_layout(c, sb, G);
    RankWgWork W;
    W.M = m.M; W.info = m.info; W.valid = m.valid;
    rank_wg_sched_layout(c, G, W);
    return W;
}
size_t rank_wg_workspace_bytes(const ppp_box &sb, const Geo &G) { Carver c(nullptr); rank_wg_layout(c, sb, G); return c.used; }
size_t rank_wg_prepared_workspace_bytes(const Geo &G) { Carver c(nullptr); RankWgWork W; rank_wg_sched_layout(c, G, W); return c.used; }
#ifdef PPP_RW_STAMPS
size_t rank_wg_stamps_offset(const ppp_box &sb, const Geo &G) {      // (tools/s2_wg_times.py reads them back)
    char base;                                                       // (any base: only the difference counts)
    Carver c(&base);
    return (size_t)((char *)rank_wg_layout(c, sb, G).weight - &base);
}
#endif

// ---- how many tiles of a launch to split (round 7) ---------------------------------------------
// Every XCD deals its range of tiles, heaviest first, to the workgroups its 32 CUs hold at a time, and a launch
// ends with its last workgroup.  140^3 centres are 183 tiles of 8 x 16 x 16 per XCD: one round, and a second one
// that is a fraction full (per-workgroup stamps, 7^3 at four workgroups per CU: 41 % of the launch's CU time
// with fewer than four resident, 16 % with none).  The tiles of the last round are the lightest, and they run
// alone on their CUs: cut in two they run side by side in half the time.  So the lightest k tiles are split,
// k = the tiles beyond the launch's last full round -- unless their halves would not fit that round either;
// a launch of less than one round is left alone.  A half costs 0.57 of a tile (it stages (8 + 2 r) / (16 + 2 r)
// of the tile's rows for half of its items), which is why nothing else is split.  From the box shape and the
// kernel's occupancy alone, so that the grid is known when the launch is made.
static int rw_choose_splits(int tiles_per_xcd, int slots_per_xcd) {
    if (slots_per_xcd <= 0 || tiles_per_xcd <= slots_per_xcd) return 0;
    const int rem = tiles_per_xcd % slots_per_xcd;
    return 2 * rem <= slots_per_xcd ? rem : 0;
}
// workgroups of the kernel that is launched a CU holds (registers and LDS; asked once per instantiation):
// the 8 x 16 x 16 tile, or (FIT, 7^3 only) the tile of run-time thickness up to 16
// Round 14: FIT asks about the instantiation of thickness TZ that the launch will use -- the answer is a function
// of the z step (registers allow RW_FIT_MINWAVES waves per SIMD, the LDS what RwLds<7, TZ, 16, 16> leaves).
template <int P, bool FIT, int TZ = 8>
static int rw_resident_per_cu() {
    static thread_local int memo = 0;
    if (memo == 0) {
        int nb = 0;
        hipError_t e;
        if constexpr (FIT) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, rank_wg_kernel<P, P, P, TZ, 16, 16, true, RW_FIT_MINWAVES>, 64 * RW_WAVES, 0);
        else e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, rank_wg_kernel<P, P, P, 8, 16, 16>, 64 * RW_WAVES, 0);
        if (e != hipSuccess || nb < 1) nb = RW_MINWAVES;
        memo = nb;
    }
    return memo;
}
// LDS bytes of the instantiation a plan launches (RwLds)
static int rw_lds_bytes(int P, bool fit, int TZ, int TY) {
    if (fit) return TZ <= 8 ? RwLds<7, 8, 16, 16>::bytes : (TZ <= 10 ? RwLds<7, 10, 16, 16>::bytes : (TZ <= 12 ? RwLds<7, 12, 16, 16>::bytes : RwLds<7, 16, 16, 16>::bytes));
#define PPP_RW_LDS(P_) (TZ == 16 ? RwLds<P_, 16, 8, 16>::bytes : (TY == 16 ? RwLds<P_, 8, 16, 16>::bytes : RwLds<P_, 8, 8, 16>::bytes))
    return P == 5 ? PPP_RW_LDS(5) : (P == 7 ? PPP_RW_LDS(7) : PPP_RW_LDS(9));
#undef PPP_RW_LDS
}
static int rw_cus_per_xcd() {
    static thread_local int memo = 0;
    if (memo == 0) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 8)
            cus = 256;
        memo = cus / 8;
    }
    return memo;
}

// ---- the plan of a launch (round 12) -----------------------------------------------------------
// Which tile, how thick in z, how many tiles, splits and order slots per XCD, which kind of XCD ranges: a host
// function of the score box, the patch size, the workgroups a CU holds and the CUs of an XCD -- all known when
// the launch is made (ppp_rank_wg_plan asks it without launching).
//   * The tile: 8 x 16 x 16 when that still gives every CU four workgroups (a row is then staged 4.5 times per
//     centre at 9^3), else 8 x 8 x 16 (6 times).  9^3 with the z-run enumeration: 8 x 8 x 16 also at large boxes
//     (a 112 x 176 x 176 launch: 256 ms against 265 ms for 8 x 16 x 16 -- and for a 16 x 8 x 16 tile, which has
//     half of its items in conflict-free rows: profiles/r04_k_s2_tiles*.txt).  ppp_params.rank_tile is the
//     caller's choice (which shape is faster depends on the box: profiles/r06_l_bench_ab_tiles.txt), and
//     PPP_RANK_WG_TILE=8x8x16 | 8x16x16 | 16x8x16, a development aid, wins over both.
//   * Splits: rw_choose_splits for the 8 x 16 x 16 tile chosen by the rule; PPP_RANK_WG_SPLIT=<tiles per XCD>
//     overrides (0: whole tiles only), also with a forced tile shape.
//   * Tile fit (7^3 only): a launch that the 8 x 16 x 16 tiling puts between one and two rounds per XCD takes the
//     smallest z step in 8 .. 16 whose tiles all fit the resident slots OF THAT STEP'S INSTANTIATION (round 14: the LDS
//     arrays are sized by the thickness, so a thinner tile may have more slots) -- one round, no tail, no splits, and
//     (t + 6) / t instead of 14 / 8 rows staged per centre in z where t > 8.  PPP_RANK_WG_TZ=<t> forces the z step (tile
//     t x 16 x 16, 7^3 only; it wins over the tile switches).
//   * XCD ranges: by tile count, or of equal weight (rank_tile_order_kernel) -- PPP_RANK_WG_XCD=count | weight.
struct RwPlan {
    int TZ, TY, TX;            // the instantiation's tile
    int tz_step;               // thickness of a tile in z (= TZ unless `fit`)
    bool fit;                  // the instantiation with a run-time z step
    int lds_tz;                // thickness that sizes its LDS arrays (one of RW_FIT_TZ when `fit`, else TZ)
    int resident, lds_bytes;   // workgroups per CU the plan assumed for that instantiation, and its LDS bytes
    int tiles_z, tiles_y, tiles_x;
    long long n_tiles;
    int per_xcd, splits, slots;   // slots: an XCD's part of the order array = grid / 8
    bool ordered, by_weight;
};
static int rw_env_int(EnvSwitch &sw, int none) {
    const char *e = sw.get();
    return (e && e[0] >= '0' && e[0] <= '9') ? atoi(e) : none;
}
// workgroups per CU of the 8 x 16 x 16 instantiation and of the run-time-thickness instantiations RW_FIT_TZ
struct RwResident { int base, fit[RW_FIT_NTZ]; };
static RwPlan rw_plan(const ppp_box &sb, const Geo &G, const RwResident &res, int cus_per_xcd) {
    const int resident = res.base;
    const int sX = sb.x1 - sb.x0, sY = sb.y1 - sb.y0, sZ = sb.z1 - sb.z0;
    RwPlan p{};
    const long long big_tiles = (long long)((sZ + 7) / 8) * ((sY + 15) / 16) * ((sX + 15) / 16);
    bool big = big_tiles >= 4 * 256;
    static EnvSwitch tile_sw("PPP_RANK_WG_TILE");
    if (const char *e = tile_sw.get()) big = strcmp(e, "8x16x16") == 0 ? true : (strcmp(e, "8x8x16") == 0 ? false : big);
    if (rw_zruns(G.px) && !tile_sw.get()) big = false;
    bool tall = tile_sw.get() && strcmp(tile_sw.get(), "16x8x16") == 0;
    if (G.rank_tile && !tile_sw.get()) { big = G.rank_tile == 2; tall = G.rank_tile == 3; }
    const bool by_rule = big && !tall && !tile_sw.get() && !G.rank_tile;
    p.TZ = tall ? 16 : 8; p.TY = tall ? 8 : (big ? 16 : 8); p.TX = 16;
    p.tz_step = p.TZ;
    static EnvSwitch order_sw("PPP_RANK_ORDER");
    static EnvSwitch split_sw("PPP_RANK_WG_SPLIT");
    static EnvSwitch tz_sw("PPP_RANK_WG_TZ");
    static EnvSwitch xcd_sw("PPP_RANK_WG_XCD");
    const int split_env = rw_env_int(split_sw, -1);
    const int tz_env = G.px == 7 ? rw_env_int(tz_sw, 0) : 0;
    const int slots_res = resident * cus_per_xcd;
    auto tiles_of = [&](int t, int ty) { return (long long)((sZ + t - 1) / t) * ((sY + ty - 1) / ty) * ((sX + 15) / 16); };
    if (tz_env > 0) {
        p.fit = true; p.TZ = 16; p.TY = 16; p.TX = 16;
        p.tz_step = tz_env < 16 ? tz_env : 16;
    } else if (by_rule && G.px == 7 && split_env < 0) {
        const long long per0 = (tiles_of(8, 16) + 7) / 8;
        if (slots_res > 0 && per0 > slots_res && per0 < 2LL * slots_res)
            for (int t = 8; t <= 16; ++t)
                if ((tiles_of(t, 16) + 7) / 8 <= (long long)res.fit[rw_fit_index(t)] * cus_per_xcd) { p.fit = true; p.TZ = 16; p.tz_step = t; break; }
    }
    p.lds_tz = p.fit ? RW_FIT_TZ[rw_fit_index(p.tz_step)] : p.TZ;
    p.resident = p.fit ? res.fit[rw_fit_index(p.tz_step)] : resident;
    p.lds_bytes = rw_lds_bytes(G.px, p.fit, p.lds_tz, p.TY);
    p.tiles_z = (sZ + p.tz_step - 1) / p.tz_step; p.tiles_y = (sY + p.TY - 1) / p.TY; p.tiles_x = (sX + p.TX - 1) / p.TX;
    p.n_tiles = (long long)p.tiles_z * p.tiles_y * p.tiles_x;
    p.per_xcd = (int)((p.n_tiles + 7) / 8);
    // heavy tiles first (PPP_RANK_ORDER=0: spatial order)
    p.ordered = !(p.n_tiles > RW_ORDER_MAX || (order_sw.get() && order_sw.get()[0] == '0'));
    p.slots = p.per_xcd;
    if (p.ordered) {
        if (split_env >= 0) p.splits = split_env;
        else if (by_rule && !p.fit) p.splits = rw_choose_splits(p.per_xcd, slots_res);
        p.splits = p.splits < p.per_xcd ? p.splits : p.per_xcd;
        if (8LL * (p.per_xcd + p.splits) > RW_ORDER_MAX) p.splits = RW_ORDER_MAX / 8 - p.per_xcd;
        // ranges of equal weight: where the rule fitted the tiles to one round (the spare slots are what such
        // ranges need), or by the switch; a range may grow by a quarter beyond per_xcd (clamped in the kernel)
        p.by_weight = p.fit && tz_env == 0;
        if (const char *e = xcd_sw.get()) p.by_weight = strcmp(e, "weight") == 0 ? true : (strcmp(e, "count") == 0 ? false : p.by_weight);
        p.slots = p.per_xcd + p.splits;
        if (p.by_weight) {
            p.slots += (p.per_xcd + 3) / 4;
            if (8LL * p.slots > RW_ORDER_MAX) p.slots = RW_ORDER_MAX / 8;
        }
    }
    return p;
}
static RwPlan rw_plan_device(const ppp_box &sb, const Geo &G) {
    RwResident res;
    res.base = G.px == 5 ? rw_resident_per_cu<5, false>() : (G.px == 7 ? rw_resident_per_cu<7, false>() : rw_resident_per_cu<9, false>());
    for (int i = 0; i < RW_FIT_NTZ; ++i) res.fit[i] = res.base;
    if (G.px == 7) {
        res.fit[0] = rw_resident_per_cu<7, true, 8>(); res.fit[1] = rw_resident_per_cu<7, true, 10>();
        res.fit[2] = rw_resident_per_cu<7, true, 12>(); res.fit[3] = rw_resident_per_cu<7, true, 16>();
    }
    return rw_plan(sb, G, res, rw_cus_per_xcd());
}
// a device that is not there: `resident` workgroups per CU by its registers, fewer where the LDS of the
// instantiation holds fewer
static RwPlan rw_plan_assumed(const ppp_box &sb, const Geo &G, int resident, int cus_per_xcd) {
    RwResident res;
    res.base = resident;
    for (int i = 0; i < RW_FIT_NTZ; ++i) {
        const int by_lds = RW_LDS_PER_CU / rw_lds_bytes(7, true, RW_FIT_TZ[i], 16);
        res.fit[i] = resident < by_lds ? resident : by_lds;
    }
    return rw_plan(sb, G, res, cus_per_xcd);
}
// out: tile z, y, x; z step; tiles; splits per XCD; slots per XCD; 1 = ranges of equal weight.
// resident_per_cu / cus_per_xcd <= 0: ask the device
void rank_wg_plan(const ppp_box &sb, const Geo &G, int resident_per_cu, int cus_per_xcd, int32_t out[8]) {
    const RwPlan p = (resident_per_cu > 0 && cus_per_xcd > 0) ? rw_plan_assumed(sb, G, resident_per_cu, cus_per_xcd)
                                                              : rw_plan_device(sb, G);
    out[0] = p.TZ; out[1] = p.TY; out[2] = p.TX; out[3] = p.tz_step;
    out[4] = (int32_t)p.n_tiles; out[5] = p.splits; out[6] = p.slots; out[7] = p.by_weight ? 1 : 0;
}
// ... and what that plan assumed of the CU: out = the thickness that sizes the kernel's LDS arrays, the
// workgroups per CU, the LDS bytes per workgroup, the CUs per XCD
void rank_wg_plan_residency(const ppp_box &sb, const Geo &G, int resident_per_cu, int cus_per_xcd, int32_t out[4]) {
    const bool assumed = resident_per_cu > 0 && cus_per_xcd > 0;
    const RwPlan p = assumed ? rw_plan_assumed(sb, G, resident_per_cu, cus_per_xcd) : rw_plan_device(sb, G);
    const int by_lds = RW_LDS_PER_CU / p.lds_bytes;
    out[0] = p.lds_tz; out[1] = (assumed && by_lds < p.resident) ? by_lds : p.resident; out[2] = p.lds_bytes;
    out[3] = assumed ? cus_per_xcd : rw_cus_per_xcd();
}

static hipError_t launch_rwg_main(const float *S, const RankWgWork &W, float *score, const ppp_box &sb, const Geo &G,
                                  hipStream_t s);

template <typename T>
static hipError_t launch_rwg(const T *pred, const float *S, const uint8_t *ov, float *score,
                             const ppp_box &sb, void *work, const Geo &G, hipStream_t s) {
    const int sX = sb.x1 - sb.x0, sY = sb.y1 - sb.y0, sZ = sb.z1 - sb.z0;
    const size_t sbV = (size_t)sX * sY * sZ;
    Carver carver(work);
    auto [M, info, valid, weight, order, dealT] = rank_wg_layout(carver, sb, G);
    if (!cons_box_covers(G, sb)) return hipErrorInvalidValue;
    PPP_GRID_CHECK((G.V + 255) / 256, 256);
    PPP_GRID_CHECK((sbV + 255) / 256, 256);
    rank_valid2_kernel<T><<<dim3((unsigned)((G.V + 255) / 256)), dim3(256), 0, s>>>(pred, ov, valid, G);
    note_rank_kernel("rank_wg_kernel");
    // (rank_wg_supported admits only the cubic windows the pre-pass compiles in)
    const dim3 pre_grid((unsigned)((sbV + 255) / 256));
#define PPP_RW_PRE(P)                                                                                       \
    case P:                                                                                                 \
        rank_masks_il_kernel<T, P><<<pre_grid, dim3(256), 0, s>>>(pred, valid, sb, M, info, score, G);      \
        break;
    switch (G.px) {
        PPP_RW_PRE(5)
        PPP_RW_PRE(7)
        PPP_RW_PRE(9)
    default:
        return hipErrorNotSupported;
    }
#undef PPP_RW_PRE
    return launch_rwg_main(S, RankWgWork{M, info, valid, weight, order, dealT}, score, sb, G, s);
}

// everything after the pre-pass: tile weights and order, the dealing table, the kernel
static hipError_t launch_rwg_main(const float *S, const RankWgWork &W, float *score, const ppp_box &sb, const Geo &G,
                                  hipStream_t s) {
    uint32_t *const M = W.M, *const info = W.info;
    uint8_t *const valid = W.valid;
    int32_t *const weight = W.weight, *order = W.order;
    uint16_t *const dealT = W.dealT;
    const RwPlan plan = rw_plan_device(sb, G);
    const bool tall = plan.TZ == 16 && !plan.fit, big = plan.TY == 16, fit = plan.fit;
    const int tiles_y = plan.tiles_y, tiles_x = plan.tiles_x, per_xcd = plan.per_xcd, splits = plan.splits, tz_step = plan.tz_step;
    const long long n_tiles = plan.n_tiles;
    if (!plan.ordered) order = nullptr;
    const long long n_blocks = 8LL * plan.slots;
    PPP_GRID_CHECK(n_blocks, 64 * RW_WAVES);
    static EnvSwitch major_sw("PPP_RANK_TILE_MAJOR");
    const int y_major = (major_sw.get() && major_sw.get()[0] == 'z') ? 0 : 1;
    if (order) {
        rank_tile_weight_kernel<<<dim3((unsigned)n_tiles), dim3(256), 0, s>>>(info, valid, sb, tz_step, plan.TY, plan.TX, tiles_y, tiles_x,
                                                                              y_major, weight, G);
        rank_tile_order_kernel<<<dim3(8), dim3(256), 0, s>>>(weight, (int)n_tiles, per_xcd, splits, plan.slots,
                                                             plan.by_weight ? 1 : 0, order);
    }
    // (the dealing table of the row classes; the strides are those of the kernel's row image)
    if (rw_bankdeal(G.px))
        rank_deal_table_kernel<7><<<dim3(7 * 7 * 7), dim3(32), 0, s>>>(dealT, 2 * 7 - 1, (2 * 7 - 1) * (2 * 7 - 1));
#ifdef PPP_RW_STAMPS
    (void)hipMemsetAsync(weight, 0, (size_t)RW_ORDER_MAX * 4, s);      // (the weights are spent: room for the stamps)
#define PPP_RW_STAMP_ARG , (uint32_t *)weight
#else
#define PPP_RW_STAMP_ARG
#endif
#define PPP_RW_ARGS S, M, info, valid, score, sb, G, tiles_y, tiles_x, (int)n_tiles, order, y_major, dealT, tz_step PPP_RW_STAMP_ARG
#define PPP_RW_LAUNCH(A_, D_, E_, F_, DZ_)                                                                  \
    rank_wg_kernel<A_, A_, A_, D_, E_, F_, DZ_><<<dim3((unsigned)n_blocks), dim3(64 * RW_WAVES), 0, s>>>(PPP_RW_ARGS)
#define PPP_RW_LAUNCH_FIT(TZ_)                                                                              \
    rank_wg_kernel<7, 7, 7, TZ_, 16, 16, true, RW_FIT_MINWAVES>                                             \
        <<<dim3((unsigned)n_blocks), dim3(64 * RW_WAVES), 0, s>>>(PPP_RW_ARGS)
#define PPP_RW_CASE(P)                                                                                      \
    case P:                                                                                                 \
        if (tall) PPP_RW_LAUNCH(P, 16, 8, 16, false);                                                       \
        else if (big) PPP_RW_LAUNCH(P, 8, 16, 16, false);                                                   \
        else PPP_RW_LAUNCH(P, 8, 8, 16, false);                                                             \
        break;
    if (fit) {
        // (the tile of run-time thickness: built for 7^3 alone, the only size the plan gives it to)
        if (G.px != 7) return hipErrorNotSupported;
        // (tz_step <= lds_tz: the kernel clamps, and the plan never asks for more)
        switch (plan.lds_tz) {
        case 8: PPP_RW_LAUNCH_FIT(8); break;
        case 10: PPP_RW_LAUNCH_FIT(10); break;
        case 12: PPP_RW_LAUNCH_FIT(12); break;
        default: PPP_RW_LAUNCH_FIT(16); break;
        }
    } else
    switch (G.px) {
        PPP_RW_CASE(5)
        PPP_RW_CASE(7)
        PPP_RW_CASE(9)
    default:
        return hipErrorNotSupported;
    }
#undef PPP_RW_LAUNCH
#undef PPP_RW_LAUNCH_FIT
#undef PPP_RW_ARGS
#undef PPP_RW_STAMP_ARG
#undef PPP_RW_CASE
    return hipGetLastError();
}

hipError_t launch_rank_wg(const void *pred, int dtype, const float *S, const uint8_t *ov, float *score,
                          const ppp_box &sb, void *work, const Geo &G, hipStream_t s) {
    if (!rank_wg_supported(G)) return hipErrorNotSupported;
    return with_pred_type(dtype, [&](auto tag) {
        using T = PPP_PRED_T(tag);
        return launch_rwg<T>((const T *)pred, S, ov, score, sb, work, G, s);
    });
}

// rank_valid2_kernel on its own (the fused pre-pass of ppp_prepass.hip reads `valid` as the kernel above does)
hipError_t launch_rank_valid(const void *pred, int dtype, const uint8_t *ov, uint8_t *valid, const Geo &G, hipStream_t s) {
    PPP_GRID_CHECK((G.V + 255) / 256, 256);
    return with_pred_type(dtype, [&](auto tag) {
        using T = PPP_PRED_T(tag);
        rank_valid2_kernel<T><<<dim3((unsigned)((G.V + 255) / 256)), dim3(256), 0, s>>>((const T *)pred, ov, valid, G);
        return hipGetLastError();
    });
}

// The same launch for a caller that has M / info / valid of this score box already (and the border,
// background and nP == 0 scores in `score`): ppp_pred_prepass made them in its one read of the prediction.
// `pre_work` is that pre-pass's workspace, which begins with rank_masks_layout; `work` holds
// rank_wg_prepared_workspace_bytes.
hipError_t launch_rank_wg_prepared(const float *S, float *score, const ppp_box &sb, void *pre_work, void *work,
                                   const Geo &G, hipStream_t s) {
    if (!rank_wg_supported(G) || G.ring) return hipErrorNotSupported;
    if (!cons_box_covers(G, sb)) return hipErrorInvalidValue;
    Carver pre(pre_work), own(work);
    const RankMasks m = rank_masks_layout(pre, sb, G);
    RankWgWork W;
    W.M = m.M; W.info = m.info; W.valid = m.valid;
    rank_wg_sched_layout(own, G, W);
    note_rank_kernel("rank_wg_kernel");
    return launch_rwg_main(S, W, score, sb, G, s);
}

}  // namespace ppp
