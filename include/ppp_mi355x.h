/*
 * ppp_mi355x.h -- C ABI of libppp_mi355x.so: the MI355X (gfx950) implementation of
 * PatchPerPix's vote_instances device path.
 *
 * This is the drop-in boundary.  In the reference the plug is the pycuda shim
 * PatchPerPix/vote_instances/cuda_code.py:5-59 (make_kernel / alloc_zero_array / sync)
 * plus the four JIT-templated kernels under PatchPerPix/vote_instances/cuda/.  Here the
 * kernels are compiled ahead of time for gfx950; shapes, thresholds and the
 * reference's -D build flags are run-time fields of ppp_params.
 *
 * Conventions
 *  - every pointer named d_* is a DEVICE pointer owned by the caller (the Python
 *    host code carries them as torch-ROCm tensors); the library never allocates,
 *    frees or retains them.  h_* pointers are host pointers.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are
 *    asynchronous on that stream unless stated otherwise.
 *  - return value 0 = success, negative = error; ppp_last_error() gives the message
 *    (thread-local).  Nothing falls back to the CPU: without a HIP device every
 *    compute entry point fails with PPP_ERR_NO_DEVICE.
 *  - volumes are (Z, Y, X) C-contiguous; predictions are (C, Z, Y, X) with
 *    C = pz*py*px, channel r = (z*py + y)*px + x of the patch, float32 or float16
 *    (the zarr dtype written by experiments/flylight/setups/setup01/predict_no_gp.py:
 *    243-257; widening to f32 is exact, which is what the reference does on load,
 *    vote_instances.py:193-200).
 *
 * Consensus layout (ppp_params.cons_layout)
 *  PPP_CONS_COMPACT   [n_planes][bz][by][bx] float32 over the base-voxel box cons_box,
 *                     one plane per lexicographically positive pixel offset
 *                     d = (dz,dy,dx), |d_i| <= p_i-1: plane = L-1 with
 *                     L = (dz*(2py-1) + dy)*(2px-1) + dx  (L > 0 <=> d positive).
 *                     These are exactly the planes the reference ever writes.
 *  PPP_CONS_VOXEL_MAJOR [bz][by][bx][W] float32, W = (2pz-1)(2py-1)(2px-1): for every base
 *                     voxel v the consensus between v and v+q for ALL signed offsets q
 *                     (index Lc + (qz*(2py-1)+qy)*(2px-1)+qx, Lc = (W-1)/2); written directly by
 *                     ppp_consensus where ppp_consensus_writes_voxel_major() says so, else made from a
 *                     COMPACT array by ppp_cons_to_voxel_major; the layout ppp_patch_graph
 *                     is fastest on (every lane sweeps contiguous memory).
 *  PPP_CONS_REFERENCE [NSZ][NSY][NSX][Z][Y][X] float32, index o = d + p - 1,
 *                     NS = 2p (NSZ = 1 when pz == 1): the reference's array
 *                     (consensus_array.py:99-106); cons_box must be the whole volume.
 */
#ifndef PPP_MI355X_H
#define PPP_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPP_ABI_VERSION 5

enum ppp_error {
    PPP_OK = 0,
    PPP_ERR_INVALID_ARG = -1,
    PPP_ERR_NO_DEVICE = -2,
    PPP_ERR_HIP = -3,
    PPP_ERR_UNSUPPORTED = -4,
    PPP_ERR_WORKSPACE = -5
};

/* Element type of a prediction buffer.  PPP_BF16 (bfloat16: 1 sign, 8 exponent, 7 mantissa bits) is
 * read by every entry point that READS a prediction; a value widens to float32 exactly (its 16 bits
 * are the float's upper half), so every result is that of the float32 buffer holding the same
 * values.  The entry points that WRITE a prediction or serve benches only (ppp_synth_pred,
 * ppp_synth_pred_box, ppp_decode_tail, ppp_counter_calibration) take PPP_F32 / PPP_F16 only.
 * ppp_pred_dtype_supported() tells what a given library reads. */
enum ppp_dtype { PPP_F32 = 0, PPP_F16 = 1, PPP_BF16 = 2 };

/* background rule for the second pixel of a pair: -DUSE_INV_TH / -DUSE_HALF_TH /
 * -DUSE_LESS_THAN_TH (utilVoteInstances.py:389-406) */
enum ppp_bg_rule { PPP_BG_INV_TH = 0, PPP_BG_HALF_TH = 1, PPP_BG_LESS_THAN_TH = 2 };
/* vote value: (none = 1) / -DPROB_PRODUCT / -DNORM_PROB_PRODUCT (utilVoteInstances.py:412-427) */
enum ppp_value_rule { PPP_VAL_COUNT = 0, PPP_VAL_PROB_PRODUCT = 1, PPP_VAL_NORM_PROB_PRODUCT = 2 };
enum ppp_cons_layout { PPP_CONS_COMPACT = 0, PPP_CONS_REFERENCE = 1, PPP_CONS_VOXEL_MAJOR = 2 };

typedef struct ppp_box {
    int32_t z0, y0, x0; /* inclusive */
    int32_t z1, y1, x1; /* exclusive */
} ppp_box;

typedef struct ppp_params {
    int32_t abi_version;   /* PPP_ABI_VERSION */
    int32_t Z, Y, X;       /* DATAZSIZE, DATAYSIZE, DATAXSIZE                            */
    int32_t pz, py, px;    /* PSZ, PSY, PSX (odd)                                        */
    double th;             /* TH  = patch_threshold, compared in double like the         */
    double thi;            /* THI   reference's literal (utilVoteInstances.py:361-375)   */
    int32_t bg_rule;       /* enum ppp_bg_rule                                           */
    int32_t value_rule;    /* enum ppp_value_rule                                        */
    int32_t use_overlap;   /* -DOVERLAP: skip pixels whose overlap mask is non-zero      */
    int32_t normalise;     /* consensus_norm_aff: cons /= count (normConsensusArray.cu)  */
    int32_t norm_rank;     /* -DNORM_PATCH_RANK                                          */
    int32_t count_pos_neg; /* -DCOUNT_POS_NEG                                            */
    int32_t norm_aff;      /* -DNORM_PATCH_AFFINITY                                      */
    int32_t cons_layout;   /* enum ppp_cons_layout                                       */
    ppp_box cons_box;      /* base voxels held by the consensus buffer (tile)            */
    int32_t origin_z, origin_y, origin_x; /* global coordinate of local voxel (0,0,0) when the
                              buffers hold a sub-volume (slab of a larger volume); only the
                              per-pair LCG seed of ppp_patch_graph depends on absolute
                              coordinates (computePatchGraph.cu:24-27)                          */
    int32_t ring_z;        /* 0, or -- VOXEL_MAJOR rows only -- the number of z-slices of a RING the
                              row buffer holds: the row of voxel (z, y, x) lives in slice
                              (z + origin_z) mod ring_z of a [ring_z][by][bx][W] buffer, cons_box
                              (at most ring_z slices thick) says which slices are current.  A caller
                              that sweeps a column of tiles upwards computes every base voxel once
                              (ppp_consensus_part over the new slices) and keeps the rows its next
                              tile still needs; read by ppp_rank_patches_vm and
                              ppp_patch_graph_by_patch*.  (The reference holds the whole array in
                              managed memory: consensus_array.py:99-106.)                         */
    int32_t pred_clean;    /* 1: the caller KNOWS (ppp_pred_check said so for the buffer it passes as
                              d_pred) that every prediction value lies in [0, 1] and none falls
                              between the two class tests (with the shipped rule: none equals TH);
                              S1 then takes a shorter classification of its operands -- same bits.
                              0 (or anything else): not known; every kernel serves any input.      */
    int32_t rank_tile;     /* ppp_rank_patches_vm, cubic 5 / 7 / 9 patches: the tile of centres a workgroup
                              takes -- 0: the library's rule; 1: 8 x 8 x 16; 2: 8 x 16 x 16; 3: 16 x 8 x 16
                              (z, y, x).  Same scores whichever; larger tiles stage fewer rows per centre
                              (4.5 instead of 6 times) and win where the memory system is the slower part
                              (measured per box: profiles/r06_l_*), smaller ones where it is not -- a
                              caller with many launches times one of each and keeps the faster.            */
} ppp_params;

/* --- library / device ------------------------------------------------------------- */
int ppp_abi_version(void);
const char *ppp_last_error(void);
/* name of the kernel the last ppp_consensus call launched (which generation / specialisation
 * served the shape): "consensus_v3_kernel", "consensus_v2_kernel" or "consensus_gather_kernel" */
const char *ppp_consensus_kernel_name(void);
/* 1 when the last S1 call (ppp_consensus, ppp_consensus_rows, ppp_consensus_part, ppp_consensus_sparse)
 * chose the packed kernel's CLEAN instantiation, the one with the short operand classification, for the votes
 * it launched (pred_clean == 1 in its parameters and the development switch PPP_S1_CLEAN not "0"); 0 after any
 * other S1 call -- one over item lists without an active item included: it launches zero stores only -- and
 * before the first.  A host variable set at launch, like the kernel names: what tests assert to know which
 * form they compared.                                                                              */
int ppp_consensus_short_form(void);
/* the same for the last S2 call (ppp_rank_patches: "rank_v2_kernel" or "rank_kernel"; ppp_rank_patches_vm:
 * "rank_wg_kernel" or "rank_vm_kernel") and the last S5 call (ppp_patch_graph:
 * "patch_graph_kernel", "patch_graph_vm_kernel" or "patch_graph_vm2_kernel"; ppp_patch_graph_by_patch*:
 * "patch_graph_pa_kernel", or "patch_graph_pa_kernel<small>" with the small chunk); "none" before the first */
const char *ppp_rank_kernel_name(void);
const char *ppp_patch_graph_kernel_name(void);
/* which instantiation of the per-patch kernel the last ppp_patch_graph_by_patch* call took: "cube" = the
 * window's sizes compiled in (pz == py == px in {3, 5, 7, 9}, and the development switch PPP_PA_CUBE not
 * "0"), "generic" = read from the parameters at run time; "none" before the first such call and after a
 * ppp_patch_graph call.  The kernel NAME above is the same for both.                                */
const char *ppp_patch_graph_kernel_geometry(void);
/* Development switches (PPP_* environment variables naming a kernel variant or a tile shape)
 * are read once per process, at their first use; ppp_reload_env() makes the next use read them
 * again (tests that compare variants within one process).                                   */
void ppp_reload_env(void);
/* number of HIP devices visible; 0 if none (never fails) */
int ppp_device_count(void);
/* 1 if this library reads predictions of the ppp_dtype code `dtype`, else 0 (needs no device; a
 * caller that may hold an older library asks before it hands over a PPP_BF16 buffer) */
int ppp_pred_dtype_supported(int dtype);

/* number of consensus planes and floats of a consensus buffer for these params */
int64_t ppp_cons_planes(const ppp_params *p);
int64_t ppp_cons_elems(const ppp_params *p);

/* --- S1: consensus = scoring + vote + (count) + normalise ---------------------------
 * replaces  create_consensus_array_cuda (consensus_array.py:71-206) and the kernels
 * fillConsensusArray_allPatches (cuda/fillConsensusArray.cu:179-218, run once or twice)
 * + normConsensusArray (cuda/normConsensusArray.cu:32-43).
 * Deterministic: every consensus entry is the float sum of its votes in raster order of
 * the voting patch centres (a legal serialisation of the reference's atomicAdd).
 * d_cons : out, layout per p->cons_layout, fully overwritten (no pre-zeroing needed)
 * d_count: optional out (same layout), the vote counts (-DOUTPUT_CNT pass); may be NULL
 * d_overlap: uint8 (Z,Y,X) or NULL when !use_overlap                                   */
int ppp_consensus(const void *d_pred, int pred_dtype, const uint8_t *d_overlap, float *d_cons,
                  float *d_count, const ppp_params *p, void *stream);
/* 1 when ppp_consensus can write p->cons_layout = PPP_CONS_VOXEL_MAJOR directly for these
 * parameters (then no COMPACT array and no ppp_cons_to_voxel_major are needed); 0 otherwise
 * (write COMPACT, then convert).  d_count must be NULL for that layout. */
int ppp_consensus_writes_voxel_major(const ppp_params *p);
/* ppp_consensus for p->cons_layout = PPP_CONS_VOXEL_MAJOR when the rows are only read by
 * ppp_rank_patches_vm / ppp_patch_graph_by_patch: the entries S[w][-d] whose SOURCE voxel w - d
 * lies outside cons_box are left UNDEFINED instead of being zeroed.  Those consumers never read
 * them: a partner pixel of a patch that lies inside the volume is a voxel of the same window, and
 * the caller's box holds every window it asks about (the tile grown by the radius for the scores,
 * by radius + p - 1 for the pair rows); on a 144 x 152 x 152 box at 9^3 the zeroing pass is 8.7 GB
 * of scattered 4-byte stores, 40 ms next to the kernel's 220.  Same interface and errors as
 * ppp_consensus otherwise (fillConsensusArray.cu:5-218, normConsensusArray.cu:5-43). */
int ppp_consensus_rows(const void *d_pred, int pred_dtype, const uint8_t *d_overlap, float *d_cons,
                       const ppp_params *p, void *stream);

/* The same votes for the base voxels of `part` only (a non-empty sub-box of p->cons_box, which
 * keeps indexing the output): COMPACT planes or open VOXEL_MAJOR rows, nothing outside `part` is
 * touched except the mirrored entries S[u + d][-d] of voxel-major rows, which land wherever u + d
 * lies in cons_box.  What a caller builds with it: a consensus CACHE over a large box filled piece
 * by piece (every base voxel computed once: consensus_array.py:71-206 run over the whole block,
 * fillConsensusArray.cu:5-218), from which ppp_cons_planes_to_rows cuts the rows of a tile for the
 * ranking and, later, for the patch graph -- instead of computing them a second time.  Packed
 * kernel only (ppp_consensus_writes_voxel_major). */
int ppp_consensus_part(const void *d_pred, int pred_dtype, const uint8_t *d_overlap, float *d_cons,
                       const ppp_params *p, const ppp_box *part, void *stream);

/* S1 on SPARSE foreground (tubes: a few percent of the volume).  The reference's thread returns at
 * once when its voxel is not foreground (fillConsensusArray.cu:25-32); the packed kernel votes for
 * every work item (run of 64 base voxels x 2 slices, offset row (dz, dy)) and masks when it writes.
 * An item is ACTIVE iff some base voxel u of the run is valid foreground AND some w = u + (dz, dy, dx)
 * inside the volume is; every other item stores only +0.0f.
 * Bytes of device work space ppp_consensus_sparse needs for these parameters and this part (NULL =
 * cons_box): validity bits, item flags, the item list.  0 when the packed kernel does not serve the
 * parameters (ppp_consensus_writes_voxel_major; COMPACT or VOXEL_MAJOR only) -- use the dense
 * entry points then.  (fillConsensusArray.cu:25-32) */
int64_t ppp_consensus_sparse_workspace_bytes(const ppp_params *p, const ppp_box *part);
/* ppp_consensus (part NULL, open_rows 0), ppp_consensus_rows (part NULL, open_rows 1) or
 * ppp_consensus_part (part given; d_count NULL) with the work taken from item lists: a pre-pass
 * flags the active items from the centre channel and the overlap mask alone, the packed kernel runs
 * over the active ones and a light kernel stores the zeros the others owe -- the same entries, bit
 * for bit, as the dense call writes (the output stays fully overwritten).
 * mode 0 = auto: one device -> host read of the active count; at or above the measured break-even
 *          share the dense launch of today is made (same kernel, same grid), below it the lists;
 * mode 1 = always the lists.  Synchronises `stream` once (the count).
 * The reference's per-thread foreground return: fillConsensusArray.cu:25-32. */
int ppp_consensus_sparse(const void *d_pred, int pred_dtype, const uint8_t *d_overlap, float *d_cons,
                         float *d_count, const ppp_params *p, const ppp_box *part, int open_rows, void *d_work,
                         int mode, void *stream);
/* what the last ppp_consensus_sparse call counted and chose: all items, active items, 1 when it
 * launched over the lists (the per-item form of the return at fillConsensusArray.cu:25-32) */
void ppp_consensus_last_items(int64_t *total, int64_t *active, int *took_lists);

/* --- S2: patch ranking ---------------------------------------------------------------
 * replaces rank_patches_cuda (ranked_patches.py:33-74) + kernel rankPatches
 * (cuda/rankPatches.cu:1-161).  Scores are written for the voxels of `score_box`
 * (NULL = whole volume) into d_score (Z,Y,X) float32; border voxels get -1 / -9999999,
 * interior non-foreground voxels 0.  The consensus buffer must cover score_box grown by
 * the patch radius (clipped to the volume).                                             */
int ppp_rank_patches(const void *d_pred, int pred_dtype, const float *d_cons,
                     const uint8_t *d_overlap, float *d_score, const ppp_box *score_box,
                     const ppp_params *p, void *stream);

/* The same scores from a VOXEL_MAJOR consensus (p->cons_layout), row-stationary: every
 * consensus row is staged in LDS once per tile of centres and serves all centres of the tile
 * whose window holds its voxel (csrc/ppp_rank_vm.hip) -- the gather form above re-fetches each
 * entry ~50 times from HBM.  Cubic patches of 3 / 5 / 7 / 9, count_pos_neg = 0; otherwise
 * PPP_ERR_UNSUPPORTED (ppp_rank_workspace_bytes returns 0).  d_work: ppp_rank_workspace_bytes.
 * Rows in a RING (p->ring_z) are read by the workgroup-per-tile kernel only (patches of 5 / 7 / 9):
 * ppp_rank_workspace_bytes with ring_z set returns 0 for any other shape -- ask before planning a ring. */
int64_t ppp_rank_workspace_bytes(const ppp_box *score_box, const ppp_params *p);
int ppp_rank_patches_vm(const void *d_pred, int pred_dtype, const float *d_cons_vm,
                        const uint8_t *d_overlap, float *d_score, const ppp_box *score_box,
                        void *d_work, const ppp_params *p, void *stream);
/* How ppp_rank_patches_vm would launch the workgroup-per-tile kernel (cubic 5 / 7 / 9 patches) for this box,
 * without launching: plan[0..2] the tile of centres of the kernel (z, y, x), plan[3] the thickness in z the
 * tiles are cut at (<= plan[0]), plan[4] the tiles, plan[5] the tiles per XCD that are split into halves,
 * plan[6] the order slots per XCD (grid = 8 x slots workgroups), plan[7] 1 when the XCDs take ranges of equal
 * weight and 0 for ranges of equal tile count.  The plan is a function of the box, the patch size, the
 * workgroups a CU holds and the CUs of an XCD: pass the last two to ask about a device that is not there
 * (no GPU is touched then), or <= 0 for the current device's.  PPP_ERR_UNSUPPORTED where another kernel ranks. */
int ppp_rank_wg_plan(const ppp_box *score_box, const ppp_params *p, int resident_per_cu, int cus_per_xcd,
                     int32_t plan[8]);
/* What that plan assumed of a CU, same arguments: res[0] the thickness in z that sizes the LDS arrays of the kernel
 * it launches (7^3 tiles of a run-time thickness come in a few such sizes, >= plan[3]; otherwise plan[0]), res[1]
 * the workgroups of that kernel a CU holds (with resident_per_cu given: that number, or fewer where 160 KB of LDS
 * hold fewer), res[2] the kernel's LDS bytes per workgroup, res[3] the CUs of an XCD. */
int ppp_rank_wg_plan_residency(const ppp_box *score_box, const ppp_params *p, int resident_per_cu, int cus_per_xcd,
                               int32_t res[4]);

/* --- S5: patch graph (edge emission) --------------------------------------------------
 * replaces computePatchGraph_cuda (aff_patch_graph.py:113-187) + kernel computePatchGraph
 * (cuda/computePatchGraph.cu:3-136).  d_pairs u32[n_pairs][6] = (z,y,x) of patch A and B,
 * d_aff f32[n_pairs] out (d_aff[i] belongs to row i whatever the processing order).
 * The reference's 512-pairs-per-launch loop with its `offset` argument
 * (aff_patch_graph.py:137-159) is one launch here.
 * d_order (optional, may be NULL): a permutation of 0..n_pairs-1 giving the order in which
 * rows are assigned to lanes.  Results do not depend on it; speed does: rows with the same
 * patch offset (B - A) placed next to each other run with wave-uniform control flow.      */
int ppp_patch_graph(const void *d_pred, int pred_dtype, const float *d_cons,
                    const uint32_t *d_pairs, const uint32_t *d_order, uint64_t n_pairs,
                    float *d_aff, const ppp_params *p, void *stream);

/* Same result, different work decomposition: one workgroup per patch A stages the consensus
 * row of every pixel of A once in LDS and serves all pairs (A, *) from it (VOXEL_MAJOR layout
 * only; px in {3,5,7,9}, otherwise PPP_ERR_UNSUPPORTED).  The caller groups the rows by patch A:
 *   d_order            row ids, rows of one patch A contiguous (any order inside a group; rows
 *                      with similar B - A next to each other diverge least)
 *   d_group_start      int64 [n_groups + 1], positions in d_order where the groups start
 *   d_chunk_offsets    int64 [n_groups + 1], exclusive scan of ceil(group size / chunk) with
 *                      chunk = ppp_patch_graph_by_patch_chunk(p) (rows per workgroup, 0 if
 *                      the patch shape is unsupported); n_blocks = d_chunk_offsets[n_groups] */
int32_t ppp_patch_graph_by_patch_chunk(const ppp_params *p);
/* A second, smaller workgroup size for lists with few rows per patch (e.g. after set-cover
 * thinning): ppp_patch_graph_by_patch_chunked takes the chunk the caller built
 * d_chunk_offsets with -- either of the two values above.                                 */
int32_t ppp_patch_graph_by_patch_chunk_small(const ppp_params *p);
int ppp_patch_graph_by_patch_chunked(const void *d_pred, int pred_dtype, const float *d_cons_vm,
                                     const uint32_t *d_pairs, const uint32_t *d_order,
                                     const int64_t *d_group_start, const int64_t *d_chunk_offsets,
                                     int32_t n_groups, int64_t n_blocks, int32_t chunk, float *d_aff,
                                     const ppp_params *p, void *stream);
/* The thinning decisions of the patch intersection made beforehand (computePatchGraph.cu:75-86:
 * the pair's LCG advances on every combination of foreground pixels z1 of A, z2 of B that both
 * lie in the intersection of the two windows; the decisions depend on the two foreground sets and
 * the pair's seed only).  For pair rows whose windows intersect, ppp_patch_graph_lcg writes, at
 * uint64 word d_drop_off[pos] of d_drops (pos = position of the row in d_order), the masks of
 * DROPPED candidates [intersection pixel of A][intersection plane of B][chunk of candidate rows]:
 * ppp_patch_graph_lcg_words(dz, dy, dx) words for patch offset B - A (0 = no intersection).
 *   d_lcg_pos   int64 [n_lcg] positions in d_order of the rows to serve (d_drop_off[pos] >= 0;
 *               rows of similar offset next to each other run with uniform control flow)
 *   d_drop_off  int64 [rows in d_order], < 0 = no masks for this row
 * ppp_patch_graph_by_patch_lcg = ppp_patch_graph_by_patch_chunked that reads those masks and
 * runs the generator itself only for rows without (d_drop_off/d_drops NULL: for all).  Same bits.
 * ppp_patch_graph_lcg_words is 0 for every offset when the per-patch kernel of this patch width
 * does not read masks (the 25-wide 2-d kernel: it runs the generator itself). */
int64_t ppp_patch_graph_lcg_words(int32_t dz, int32_t dy, int32_t dx, const ppp_params *p);
/* Host only, no device needed: the foreground bits of a px^3 patch (n_words = ceil(px^3 / 32) words, bit r
 * of the window raster = bit r & 31 of word r >> 5, as ppp_patch_fg_bits writes them) as values per
 * candidate plane -- the function with which the cubic small-chunk per-patch kernels form the values a lane
 * keeps in registers.  px in {3, 5, 7}: planes[z] = bits [z px^2, (z + 1) px^2), px values.  px = 9: a
 * plane is two chunks of candidate rows, planes[z] = rows 0-6 (bits [81 z, 81 z + 63)) and planes[9 + z] =
 * rows 7-8 (bits [81 z + 63, 81 z + 81)), 18 values. */
int ppp_patch_plane_bits(const uint32_t *words, int32_t n_words, int32_t px, uint64_t *planes);
int ppp_patch_graph_lcg(const void *d_pred, int pred_dtype, const uint32_t *d_pairs,
                        const uint32_t *d_order, const int64_t *d_lcg_pos, int64_t n_lcg,
                        const int64_t *d_drop_off, uint64_t *d_drops, const ppp_params *p, void *stream);
int ppp_patch_graph_by_patch_lcg(const void *d_pred, int pred_dtype, const float *d_cons_vm,
                                 const uint32_t *d_pairs, const uint32_t *d_order,
                                 const int64_t *d_group_start, const int64_t *d_chunk_offsets,
                                 int32_t n_groups, int64_t n_blocks, int32_t chunk, float *d_aff,
                                 const int64_t *d_drop_off, const uint64_t *d_drops,
                                 const ppp_params *p, void *stream);
/* The foreground bits of a patch made once per patch.  The per-patch kernel needs, for patch A and
 * for the patch B of every pair row, the C = pz*py*px bits  mid[u_r] > th && pred[r][c] > th  (u_r =
 * the r-th voxel of the window of centre c; th as in the patch graph); built inside the kernel they
 * cost 2 C scattered loads per row.  ppp_patch_fg_bits writes ceil(C / 32) uint32 words per centre
 * (bit r of the patch = bit r % 32 of word r / 32) for
 *   d_centres   int64 [n] linear voxel indices (z*Y + y)*X + x, ASCENDING, windows inside the volume
 * ppp_patch_graph_by_patch_bits = ppp_patch_graph_by_patch_lcg (slices != 0: its _slices form) that
 * reads the bits of A and of every B from that table (a binary search per row in d_bits_centres,
 * which must hold the centre of every patch of the dispatched rows) -- d_bits NULL: built in the
 * kernel, as by the entry points above.  Same bits.  The table depends on d_pred and the patch shape
 * only, not on cons_box or ring_z. */
int ppp_patch_fg_bits(const void *d_pred, int pred_dtype, const int64_t *d_centres, int64_t n,
                      uint32_t *d_bits, const ppp_params *p, void *stream);
int ppp_patch_graph_by_patch_bits(const void *d_pred, int pred_dtype, const float *d_cons_vm,
                                  const uint32_t *d_pairs, const uint32_t *d_order,
                                  const int64_t *d_group_start, const int64_t *d_chunk_offsets,
                                  int32_t n_groups, int64_t n_blocks, int32_t chunk, float *d_aff,
                                  const int64_t *d_drop_off, const uint64_t *d_drops,
                                  const int64_t *d_bits_centres, int64_t n_bits, const uint32_t *d_bits,
                                  int32_t slices, const ppp_params *p, void *stream);
int ppp_patch_graph_by_patch(const void *d_pred, int pred_dtype, const float *d_cons_vm,
                             const uint32_t *d_pairs, const uint32_t *d_order,
                             const int64_t *d_group_start, const int64_t *d_chunk_offsets,
                             int32_t n_groups, int64_t n_blocks, float *d_aff,
                             const ppp_params *p, void *stream);

/* --- S6: labelling -------------------------------------------------------------------
 * replaces setAffgraph (aff_patch_graph.py:31-40) + the connected-components branch of
 * affGraphToInstances (graph_to_labeling.py:50-54,61-86).
 *
 * ppp_label_components: union-find (global atomics) over the rows with aff > 0; nodes are
 * patch centres identified by their linear voxel index.  Output, for every node k of the
 * caller's node list d_nodes u32[n_nodes][3] (normally the selected patches):
 *   d_node_key[k] (uint32): the ORDER KEY of the component node k belongs to, or 0xFFFFFFFF
 *   if it is in no component (no positive edge).  The key of a component is the smallest
 *   position 2*row+side at which any of its members first appears among the rows with
 *   aff != 0 -- sorting the distinct keys ascending reproduces networkx's component
 *   enumeration order (graph_to_labeling.py:54-61).
 * d_work: workspace of ppp_label_workspace_bytes(p) bytes.                              */
size_t ppp_label_workspace_bytes(const ppp_params *p);
int ppp_label_components(const uint32_t *d_pairs, const float *d_aff, uint64_t n_pairs,
                         const uint32_t *d_nodes, uint64_t n_nodes, uint32_t *d_node_key,
                         void *d_work, const ppp_params *p, void *stream);

/* The same labelling in STREAMING form: the pair rows of a large volume need not exist at
 * the same time (tile by tile on one GPU), nor on one device (every rank labels the rows of
 * its own patches; the forests are merged afterwards -- the boundary-label merge).  Both
 * stitch_patch_graph.py's "one global graph from per-block pair lists" (:110-399) and
 * setAffgraph + connected_components (see above) are covered.
 *   ppp_label_begin        state of every node of d_nodes (parent = itself, no key)
 *   ppp_label_add          a batch of rows with their affinities; the row ids are GLOBAL
 *                          positions in the canonical pair list (d_row_ids int64[n], or
 *                          first_row_id + i when d_row_ids is NULL).  Order-free: atomicMin of
 *                          2*id+side on the nodes of rows with aff != 0, lock-free unions
 *                          (CAS hooking under the smaller root) for rows with aff > 0.
 *   ppp_label_union_edges  unions given as node pairs (linear voxel indices, int64): how
 *                          another rank's forest (node, parent[node]) is merged
 *   ppp_label_finish       d_node_key int64[n_nodes]: the component's order key (smallest
 *                          2*id+side of a member with a positive edge) or PPP_LABEL_NONE_KEY
 * Workspace (ppp_label_workspace_bytes): four volumes indexed by linear voxel index,
 * parent u32[V] | has_positive_edge u32[V] | firstpos u64[V] | key u64[V]; callers that merge
 * ranks read / write the node entries of these arrays directly.                           */
#define PPP_LABEL_NONE_KEY (1ull << 62)
int ppp_label_begin(const uint32_t *d_nodes, uint64_t n_nodes, void *d_work, const ppp_params *p,
                    void *stream);
int ppp_label_add(const uint32_t *d_pairs, const float *d_aff, const int64_t *d_row_ids,
                  int64_t first_row_id, uint64_t n_pairs, void *d_work, const ppp_params *p,
                  void *stream);
int ppp_label_union_edges(const int64_t *d_a, const int64_t *d_b, uint64_t n, void *d_work,
                          const ppp_params *p, void *stream);
int ppp_label_finish(const uint32_t *d_nodes, uint64_t n_nodes, int64_t *d_node_key, void *d_work,
                     const ppp_params *p, void *stream);

/* ppp_paint_instances: for every node k (d_nodes u32[n_nodes][3]) with label
 * d_labels[k] > 0, write the label into every voxel of its window whose patch value is
 * > TH, keeping the maximum label per voxel ("later components overwrite earlier ones",
 * graph_to_labeling.py:73-84, with labels = component rank + 1).  d_instances u32 (Z,Y,X)
 * is updated in place (caller zero-initialises).                                        */
int ppp_paint_instances(const void *d_pred, int pred_dtype, const uint32_t *d_nodes,
                        const uint32_t *d_labels, uint64_t n_nodes, uint32_t *d_instances,
                        const ppp_params *p, void *stream);

/* --- `no_overlap_per_channel` without the loop over components (ppp_pack_channels.hip) -------
 * Replaces graph_to_labeling.py:57-115 (per component: a zeroed volume, the paint, np.sum, a masked
 * test per channel tried) by sizes + overlap pairs (below), ppp_host_pack_channels and one paint.
 * Labels are 1 .. n_labels; `own` is the sub-box of the frame (Z,Y,X of ppp_params) whose voxels the
 * call counts (NULL = the whole frame): a tile counts its own voxels and reads patch centres from
 * its frame, grown by the patch radius.  Nodes must lie inside the frame.
 * ppp_pack_scan_count: d_sizes u64 [n_labels + 1] += the number of own voxels each label covers
 *   (slot 0 unused; the caller zeroes the table once and may sum several boxes into it);
 *   *n_pairs = the keys ppp_pack_scan_fill will write.  Synchronises the stream.
 * ppp_pack_scan_fill: after the count, on the same workspace, prediction, frame and box: d_pairs
 *   u64 [n_pairs] = (b << 32) | a for every own voxel and every two labels a < b that cover it (a
 *   pair comes once per shared voxel -- the caller dedupes; exact, nothing dropped, no cap on the
 *   labels that meet in a voxel).
 * ppp_paint_instances_channels: ppp_paint_instances into d_out u32 (n_channels, Z, Y, X):
 *   label l is painted into channel d_chan[l] (u32 [n_labels + 1], slot 0 unused), the largest
 *   label of a channel wins a voxel (graph_to_labeling.py:93-106 given the assignment).       */
int64_t ppp_pack_scan_workspace_bytes(const ppp_params *p, const ppp_box *own);
int ppp_pack_scan_count(const void *d_pred, int pred_dtype, const uint32_t *d_nodes, const uint32_t *d_labels,
                        uint64_t n_nodes, uint32_t n_labels, const ppp_box *own, uint64_t *d_sizes,
                        int64_t *n_pairs, void *d_work, const ppp_params *p, void *stream);
int ppp_pack_scan_fill(const void *d_pred, int pred_dtype, const ppp_box *own, uint64_t *d_pairs, int64_t n_pairs,
                       void *d_work, const ppp_params *p, void *stream);
int ppp_paint_instances_channels(const void *d_pred, int pred_dtype, const uint32_t *d_nodes,
                                 const uint32_t *d_labels, uint64_t n_nodes, const uint32_t *d_chan,
                                 uint32_t n_labels, uint32_t n_channels, uint32_t *d_out,
                                 const ppp_params *p, void *stream);

/* ppp_paint_patch_rows: the same painting with the patches given as a table instead of a dense
 * prediction block: d_rows [n_nodes][C] (float16 / float32), row k = pred[:, node k].  Serves
 * affGraphToInstances(sparse_labels=True) of the blockwise driver (graph_to_labeling.py:66-72,
 * stitch_patch_graph.py:388-396), where the patch of every node of the GLOBAL graph is read
 * from the prediction store -- here gathered chunk by chunk into the table.               */
int ppp_paint_patch_rows(const void *d_rows, int rows_dtype, const uint32_t *d_nodes,
                         const uint32_t *d_labels, uint64_t n_nodes, uint32_t *d_instances,
                         const ppp_params *p, void *stream);

/* --- the reference's NumPy-semantics stages (`cuda=False`) ------------------
 * A different function from the kernels above: integer votes.  Per interior foreground centre c
 * (utilVoteInstances.py:59-92, get_patch_sets.py:32-79; float32 compares):
 *     pf_c = { v in win(c) : pred[r_v][c] > th     and foreground[v] }
 *     pb_c = { v in win(c) : pred[r_v][c] < 1 - th and foreground[v] }
 * Votes: int16 [ppp_np_vote_planes(p)][Z][Y][X]; plane q >= 1 = the lexicographically positive
 * offset with linear signed index (dz (2py-1) + dy)(2px-1) + dx = q (the COMPACT plane order),
 * plane 0 = the zero offset (only ever non-zero for th < 0.5).  cons_box must be the whole volume.
 *
 * ppp_np_consensus    replaces create_consensus_array (consensus_array.py:18-68) + fillLookup
 *                     (utilVoteInstances.py:19-56): +1 per centre on the key of every unordered
 *                     pair of pf_c, -1 per centre on every DISTINCT key of a pair (pf_c, pb_c).
 * ppp_np_rank_patches replaces rank_patches (ranked_patches.py:76-105): d_score int32 (Z,Y,X),
 *                     #(ff votes > 0) - #(ff votes <= 0) + #(fb votes < 0) - #(fb votes >= 0) for
 *                     interior foreground centres, 0 elsewhere.
 * ppp_np_patch_graph  replaces computePatchGraph's NumPy branch (aff_patch_graph.py:209-282) for
 *                     the candidate rows d_rows int32 [n][6] = (A, B): d_weight[i] = sum of the
 *                     votes over all (p in pf_A, q in pf_B), |p - q| < patch shape on every axis,
 *                     p != q, with pf taken against d_mask (= mask_to_cover); d_count[i] = the
 *                     number of such pairs (the edge exists iff it is > 0).                      */
int64_t ppp_np_vote_planes(const ppp_params *p);
int ppp_np_consensus(const void *d_pred, int pred_dtype, const uint8_t *d_foreground, int16_t *d_votes,
                     const ppp_params *p, void *stream);
int ppp_np_rank_patches(const void *d_pred, int pred_dtype, const uint8_t *d_foreground, const int16_t *d_votes,
                        int32_t *d_score, const ppp_params *p, void *stream);
int ppp_np_patch_graph(const void *d_pred, int pred_dtype, const uint8_t *d_mask, const int16_t *d_votes,
                       const int32_t *d_rows, uint64_t n_rows, int64_t *d_weight, int32_t *d_count,
                       const ppp_params *p, void *stream);

/* --- layout helper ---------------------------------------------------------------------
 * expand a whole-volume COMPACT consensus into the reference's [NSZ][NSY][NSX][Z][Y][X]
 * array (what create_consensus_array_cuda returns / save_consensus writes).             */
int ppp_cons_to_reference(const float *d_cons_compact, float *d_cons_reference,
                          const ppp_params *p, void *stream);

/* re-layout a COMPACT consensus (p->cons_box, p->cons_layout ignored) as VOXEL_MAJOR       */
int ppp_cons_to_voxel_major(const float *d_cons_compact, float *d_cons_voxel_major,
                            const ppp_params *p, void *stream);

/* VOXEL_MAJOR rows of p->cons_box from COMPACT planes that are indexed by a box of their own,
 * `planes_box` (it must hold cons_box; same coordinate frame): S[v][+d] = planes[d][v],
 * S[v][-d] = planes[d][v - d], 0 where v - d lies outside planes_box (an entry nothing reads, as
 * with ppp_consensus_rows).  ppp_cons_to_voxel_major is the case planes_box == cons_box.
 * (aff_patch_graph.py:113-187 / ranked_patches.py:33-74 read the consensus array the
 * reference keeps whole in managed memory; this is how a tile's share of it reaches HBM rows.) */
int ppp_cons_planes_to_rows(const float *d_planes, const ppp_box *planes_box, float *d_rows,
                            const ppp_params *p, void *stream);

/* --- foreground / patch bit helpers used by the host stages --------------------------
 * ppp_patch_bits: for n centres (d_centres u32[n][3]) pack (pred[r][c] > thresh) for
 * r = 0..C-1 into ceil(C/32) uint32 words each (bit r%32 of word r/32), d_bits
 * u32[n][ceil(C/32)].  The compare is float32 against (float)thresh, which is how NumPy
 * evaluates `patch > fc_threshold` for a float32 patch (foreground_cover.py:156-158).      */
int ppp_patch_bits(const void *d_pred, int pred_dtype, const uint32_t *d_centres,
                   uint64_t n, double thresh, uint32_t *d_bits, const ppp_params *p,
                   void *stream);
/* the same bits for every voxel, d_bits_vol u32[Z*Y*X][ceil(C/32)] (the prediction is read once,
 * coalesced; callers with many centres gather their rows from it)                          */
int ppp_patch_bits_volume(const void *d_pred, int pred_dtype, double thresh, uint32_t *d_bits_vol,
                          const ppp_params *p, void *stream);

/* --- greedy foreground cover on the device ---------------------------------------------
 * ppp_cover_pass: one pass of computeForegroundCoverLoop (foreground_cover.py:111-180) as an
 * exact priority-parallel algorithm (csrc/ppp_cover.hip): every patch whose state is 0 takes
 * part; it ends up 1 (selected: more than pix_th voxels of the running mask were inside its
 * window where its prediction is > fc_threshold when its turn came) or 2 (not selected).
 *   d_mask    u8  [Z][Y][X]         running mask, cleared in place like mask_running
 *   d_bits    u32 [n][ceil(C/32)]   ppp_patch_bits(fc_threshold) of the ranked patches
 *   d_lin     i64 [n]               linear centre index of ranked patch k (interior centres)
 *   d_state   i32 [n]               in/out, see above (1 / 2 on entry: does not take part)
 *   d_cleared i32 [n]               out: interior voxels patch k cleared (0 if not selected)
 *   d_work    ppp_cover_workspace_bytes(n, p) bytes
 * The loop's stop rule ("interior of the mask is empty", checked before every patch) is not
 * applied here: the caller cuts the selected list, in rank order, after the patch at which
 * the running sum of d_cleared reaches the number of set interior voxels.  *rounds (may be
 * NULL) returns the number of parallel rounds.  Synchronises the stream.                   */
int64_t ppp_cover_workspace_bytes(int64_t n, const ppp_params *p);
int ppp_cover_pass(uint8_t *d_mask, const uint32_t *d_bits, const int64_t *d_lin, int64_t n,
                   int32_t pix_th, int32_t *d_state, int32_t *d_cleared, void *d_work,
                   const ppp_params *p, void *stream, int32_t *rounds);
/* The same pass with the patch bits in a table that has one row per VOXEL (row of patch k =
 * d_bits_by_voxel + (d_lin[k] - first_voxel) * words): the tiled assembly fills such a table
 * tile by tile while the prediction of a tile is resident (prediction provider: the bits cannot
 * be recomputed later) -- reordering it into rank order would need a second copy of it (92 bytes
 * per voxel at 9^3).  Same selections as ppp_cover_pass (foreground_cover.py:111-180).        */
int ppp_cover_pass_voxel_bits(uint8_t *d_mask, const uint32_t *d_bits_by_voxel, int64_t first_voxel,
                              const int64_t *d_lin, int64_t n, int32_t pix_th, int32_t *d_state,
                              int32_t *d_cleared, void *d_work, const ppp_params *p, void *stream,
                              int32_t *rounds);

/* --- the cover's two optional branches on the device ---------------------------------------
 * ppp_cover_pass_marked: ppp_cover_pass with `mark_close_neighboorhood` (foreground_cover.py:141-143,
 * 162-168).  d_mark_bits u32 [Z*Y][(X+31)/32 + 1] (ppp_cover_mark_bits_bytes(p) bytes; bit x%32 of word
 * x/32 of row z*Y+y), in/out, shared by the passes of one cover and its ring cover: a patch whose centre is
 * marked is skipped (before the count), a selected patch marks marked[cz, cy-3:cy+4, cx-3:cx+4] with
 * NumPy's slice rules -- the high end clips, a negative start (cy < 3 or cx < 3) marks nothing.  Exact:
 * the rounds' ready test uses the y/x radius max(p-1, 3).  As in ppp_cover_pass the stop rule is the
 * caller's; marks may only come from patches that survive its cut, so the caller rebuilds the volume from
 * the surviving set (ppp_cover_marks_from_selected) after the pass.  y or x axes shorter than 7 (the
 * slice would wrap to the far end): PPP_ERR_UNSUPPORTED.                                      */
int ppp_cover_pass_marked(uint8_t *d_mask, const uint32_t *d_bits, const int64_t *d_lin, int64_t n,
                          int32_t pix_th, int32_t *d_state, int32_t *d_cleared, uint32_t *d_mark_bits,
                          void *d_work, const ppp_params *p, void *stream, int32_t *rounds);
/* ... with the patch bits in a row per voxel, see ppp_cover_pass_voxel_bits (foreground_cover.py:141-143,
 * 162-168)                                                                                   */
int ppp_cover_pass_marked_voxel_bits(uint8_t *d_mask, const uint32_t *d_bits_by_voxel, int64_t first_voxel,
                                     const int64_t *d_lin, int64_t n, int32_t pix_th, int32_t *d_state,
                                     int32_t *d_cleared, uint32_t *d_mark_bits, void *d_work,
                                     const ppp_params *p, void *stream, int32_t *rounds);
int64_t ppp_cover_mark_bits_bytes(const ppp_params *p);
/* ppp_cover_marks_from_selected: the mark volume of a set of selected centres, rebuilt from nothing
 * (foreground_cover.py:162-168 applied to each): d_lin i64 [n] linear centres, d_selected u8 [n] (NULL:
 * all n) picks among them.                                                                    */
int ppp_cover_marks_from_selected(const int64_t *d_lin, const uint8_t *d_selected, int64_t n,
                                  uint32_t *d_mark_bits, const ppp_params *p, void *stream);
/* ppp_mask_dilate: scipy.ndimage.binary_dilation(d_in != 0, iterations=k) with the default 6-neighbour
 * cross (foreground_cover.py:57-60, `select_patches_overlap_neighborhood`: the ring between 2 and 5
 * dilations of the overlap voxels); use_z = 0 leaves the z neighbours out (a stack of independent
 * slices).  d_in, d_out u8 [Z][Y][X] (d_out 0 / 1; may be d_in), d_work
 * ppp_mask_dilate_workspace_bytes(p) bytes.                                                   */
int64_t ppp_mask_dilate_workspace_bytes(const ppp_params *p);
int ppp_mask_dilate(const uint8_t *d_in, uint8_t *d_out, int32_t iterations, int32_t use_z, void *d_work,
                    const ppp_params *p, void *stream);

/* The x and y passes of the rounds' neighbourhood minimum on their own (what ppp_cover_pass and
 * ppp_thin_cover run once per round between their count and select steps): d_out[z][y][x] = the minimum
 * of d_in over [y - (py-1), y + (py-1)] x [x - (px-1), x + (px-1)] of slice z, clipped to the slice.
 * elem_bytes 4: int32 ranks ("none" = 0x7F7F7F7F), 8: int64 keys ("none" = 0x7F7F7F7F7F7F7F7F);
 * d_in, d_out and d_scratch hold Z*Y*X elements each and are distinct.                          */
int ppp_minfilter_xy(const void *d_in, void *d_out, void *d_scratch, int32_t elem_bytes, const ppp_params *p,
                     void *stream);

/* --- S4: set-cover thinning on the device -------------------------------------------------
 * replaces thinOutForegroundCover (foreground_cover.py:183-256, sample == 1.0; a host loop in the
 * reference): while the interior of the running mask is not empty, keep the first patch that
 * covers the most still uncovered voxels and clear them.  Exact priority-parallel form of that
 * loop (csrc/ppp_cover.hip): rounds of count / 3-d neighbourhood minimum of the key
 * (count descending, index ascending) / keep-and-clear, then the stop rule from the kept
 * patches' keys and cleared-interior counts.
 *   d_mask  u8  [Z][Y][X]        mask_to_cover (not modified)
 *   d_bits  u32 [n][ceil(C/32)]  ppp_patch_bits(fc_threshold) of the selected patches, in the
 *                                order of the selected list (= rank order)
 *   d_lin   i64 [n]              linear centre index of selected patch k
 *   d_keep  u8  [n]              out: 1 = kept
 *   d_work  ppp_thin_workspace_bytes(n, p) bytes
 * *rounds (may be NULL): number of parallel rounds.  Synchronises the stream.               */
int64_t ppp_thin_workspace_bytes(int64_t n, const ppp_params *p);
int ppp_thin_cover(const uint8_t *d_mask, const uint32_t *d_bits, const int64_t *d_lin, int64_t n,
                   uint8_t *d_keep, void *d_work, const ppp_params *p, void *stream,
                   int32_t *rounds);

/* The same rounds one step at a time, for a cover SHARDED over ranks by z (every rank: its
 * own slices + a halo of p-1 slices, local coordinates, origin_z = first global slice).
 *   ppp_cover_open    d_lin int64[n]: LOCAL linear index of the rank's own ranked patches (rank
 *                     order), d_rank_id int32[n]: their GLOBAL rank (what neighbours compare
 *                     with); d_state / d_cleared as in ppp_cover_pass, but indexed locally
 *   ppp_cover_step    PPP_COVER_COUNT / _FILTER / _SELECT (d_bits u32[n][words] local table;
 *                     global_z: slices of the whole volume, for the interior test)
 *   ppp_cover_alive   *alive = some own patch was undecided at the last count (host sync)
 *   ppp_cover_zone    export (import = 0) / import (1) of the local slices [z_lo, z_hi) around
 *                     a slab boundary: d_rank int32 (own slices [own_lo, own_hi), INT32_MAX
 *                     elsewhere -> MIN over ranks), d_mask u8 0/1 and d_clean u8 (1 = not dirty)
 *                     (-> MIN over ranks); d_rank or the d_mask/d_clean pair may be NULL
 *   ppp_cover_close   the running mask back into d_mask (bytes whose bit was cleared -> 0)
 * Workspace: ppp_cover_workspace_bytes of the LOCAL geometry.                               */
#define PPP_COVER_COUNT 0
#define PPP_COVER_FILTER 1
#define PPP_COVER_SELECT 2
int ppp_cover_open(const uint8_t *d_mask, const int64_t *d_lin, const int32_t *d_rank_id, int64_t n,
                   const int32_t *d_state, int32_t *d_cleared, void *d_work, const ppp_params *p,
                   void *stream);
int ppp_cover_step(int32_t what, const uint32_t *d_bits, int32_t pix_th, int32_t *d_state,
                   int32_t *d_cleared, void *d_work, int32_t global_z, const ppp_params *p,
                   void *stream);
int ppp_cover_alive(void *d_work, const ppp_params *p, void *stream, int32_t *alive);
int ppp_cover_close(uint8_t *d_mask, void *d_work, const ppp_params *p, void *stream);
int ppp_cover_zone(int32_t import, void *d_work, int32_t z_lo, int32_t z_hi, int32_t own_lo,
                   int32_t own_hi, int32_t *d_rank, uint8_t *d_mask, uint8_t *d_clean,
                   const ppp_params *p, void *stream);

/* The set-cover thinning (ppp_thin_cover, foreground_cover.py:183-256) one round step at a time, SHARDED
 * over ranks by z like the cover above (round 6): every rank holds its own slices + p-1 halo slices
 * (local coordinates, origin_z = first global slice) and thins its OWN selected patches.
 *   ppp_thin_open    d_lin int64[n]: LOCAL linear index of the own selected patches, d_index int32[n]:
 *                    their positions in the GLOBAL selected list (the tie-break of the loop's argmax,
 *                    :210); d_state / d_count / d_cleared int32[n] are zeroed here and filled by the
 *                    steps: state 1 = kept in some round, 2 = retired with nothing left to cover;
 *                    count = voxels it covered when it was kept; cleared = interior voxels among them
 *   ppp_thin_step    PPP_COVER_COUNT / _FILTER / _SELECT (d_bits u32[n][words], the own patches' bits)
 *   ppp_thin_alive   *alive = some own patch was undecided at the last count (host sync)
 *   ppp_thin_zone    export / import of the local slices [z_lo, z_hi) around a slab boundary: d_key
 *                    int64 (own slices [own_lo, own_hi), INT64_MAX elsewhere -> MIN over ranks),
 *                    d_mask / d_clean as in ppp_cover_zone
 *   ppp_thin_close   the running mask back into d_mask
 * The loop's stop rule ("interior empty", tested before every pick) is the caller's: the kept patches
 * of all ranks in the order of their keys (count descending, index ascending), cut where the cumulative
 * cleared interior voxels reach the interior voxels the mask held at the start.
 * Workspace: ppp_thin_shard_workspace_bytes of the LOCAL geometry.                             */
int64_t ppp_thin_shard_workspace_bytes(const ppp_params *p);
int ppp_thin_open(const uint8_t *d_mask, const int64_t *d_lin, const int32_t *d_index, int64_t n, int32_t *d_state,
                  int32_t *d_count, int32_t *d_cleared, void *d_work, const ppp_params *p, void *stream);
int ppp_thin_step(int32_t what, const uint32_t *d_bits, int32_t *d_state, int32_t *d_count, int32_t *d_cleared,
                  void *d_work, int32_t global_z, const ppp_params *p, void *stream);
int ppp_thin_alive(void *d_work, const ppp_params *p, void *stream, int32_t *alive);
int ppp_thin_close(uint8_t *d_mask, void *d_work, const ppp_params *p, void *stream);
int ppp_thin_zone(int32_t import, void *d_work, int32_t z_lo, int32_t z_hi, int32_t own_lo, int32_t own_hi,
                  int64_t *d_key, uint8_t *d_mask, uint8_t *d_clean, const ppp_params *p, void *stream);

/* --- patch pairs on the device ---------------------------------------------------------
 * replaces computeAndStorePatchPairs (aff_patch_graph.py:43-110).  d_sorted_zyx int32[n][3]
 * is the selected list stably sorted by x (aff_patch_graph.py:45).  Two calls: count the
 * partners j > i of every patch i, then -- after an exclusive scan of the counts by the
 * caller -- write the rows (pts[i], pts[j]) in (i, j) order, followed by the n self pairs
 * when include_single (includeSinglePatchCCS).  Rows: d_rows u32[n_pair_rows (+ n)][6].   */
int ppp_patch_pairs_count(const int32_t *d_sorted_zyx, int64_t n, int32_t max_ps_dist,
                          int64_t *d_counts, const ppp_params *p, void *stream);
int ppp_patch_pairs_fill(const int32_t *d_sorted_zyx, int64_t n, int32_t max_ps_dist,
                         const int64_t *d_offsets, int64_t n_pair_rows, int32_t include_single,
                         uint32_t *d_rows, const ppp_params *p, void *stream);
/* The rows of a SUBSET of first patches (the patches of one tile / one rank; the blockwise
 * form of computeAndStorePatchPairs, stitch_patch_graph.py:209-248).  d_subset int64[m]:
 * indices into the x-sorted list.  count: d_counts[d_subset[k]] only.  fill: rows of subset
 * entry k start at local row d_local_offsets[k]; d_row_ids receives the GLOBAL row id of every
 * local row (d_global_offsets[i] + j; the self pair of patch i has id n_rows_total + i and
 * local position n_local_rows + k).                                                       */
int ppp_patch_pairs_count_subset(const int32_t *d_sorted_zyx, int64_t n, int32_t max_ps_dist,
                                 const int64_t *d_subset, int64_t m, int64_t *d_counts,
                                 const ppp_params *p, void *stream);
int ppp_patch_pairs_fill_subset(const int32_t *d_sorted_zyx, int64_t n, int32_t max_ps_dist,
                                const int64_t *d_subset, int64_t m, const int64_t *d_local_offsets,
                                const int64_t *d_global_offsets, int64_t n_local_rows,
                                int64_t n_rows_total, int32_t include_single, uint32_t *d_rows,
                                int64_t *d_row_ids, const ppp_params *p, void *stream);
/* --- a stack of independent 2-d images (pz = 1) ----------------------------------------------
 * The z axis is a batch of N images that one call per image would vote separately; these entry
 * points give, slice by slice, exactly what such a call computes.  Additive: ppp_params is the
 * same, and every other entry point keeps its meaning.
 *   ppp_patch_pairs_count_slices / _fill_slices  as ppp_patch_pairs_count / _fill, on the selected
 *       list sorted by (z, x) (stably): partners only in the same slice, scanned up to the end of
 *       it -- the rows of slice k are those of slice k's own list, in its canonical order.
 *   ppp_patch_graph_slices / ppp_patch_graph_lcg_slices / ppp_patch_graph_by_patch_lcg_slices
 *       as the entry points without the suffix, with the per-pair LCG seed of every image's own
 *       coordinates (z = 0: the seed is 0, computePatchGraph.cu:24-27).
 *   ppp_thin_cover_slices  as ppp_thin_cover with the loop's stop rule per slice:
 *       h_slice_interior int64[Z] (HOST) = set interior voxels of every slice of d_mask.
 *   ppp_label_slice_renumber  d_labels int32[n] (in/out): ranks over the stack ascending by
 *       (slice, order key) in, ids numbered from 1 in every slice out (0 stays 0);
 *       d_slice_min / d_slice_max int32[Z] out: smallest rank / largest id of every slice.     */
int ppp_patch_pairs_count_slices(const int32_t *d_sorted_zyx, int64_t n, int32_t max_ps_dist,
                                 int64_t *d_counts, const ppp_params *p, void *stream);
int ppp_patch_pairs_fill_slices(const int32_t *d_sorted_zyx, int64_t n, int32_t max_ps_dist,
                                const int64_t *d_offsets, int64_t n_pair_rows, int32_t include_single,
                                uint32_t *d_rows, const ppp_params *p, void *stream);
int ppp_patch_graph_slices(const void *d_pred, int pred_dtype, const float *d_cons,
                           const uint32_t *d_pairs, const uint32_t *d_order, uint64_t n_pairs,
                           float *d_aff, const ppp_params *p, void *stream);
int ppp_patch_graph_lcg_slices(const void *d_pred, int pred_dtype, const uint32_t *d_pairs,
                               const uint32_t *d_order, const int64_t *d_lcg_pos, int64_t n_lcg,
                               const int64_t *d_drop_off, uint64_t *d_drops, const ppp_params *p,
                               void *stream);
int ppp_patch_graph_by_patch_lcg_slices(const void *d_pred, int pred_dtype, const float *d_cons_vm,
                                        const uint32_t *d_pairs, const uint32_t *d_order,
                                        const int64_t *d_group_start, const int64_t *d_chunk_offsets,
                                        int32_t n_groups, int64_t n_blocks, int32_t chunk, float *d_aff,
                                        const int64_t *d_drop_off, const uint64_t *d_drops,
                                        const ppp_params *p, void *stream);
int ppp_thin_cover_slices(const uint8_t *d_mask, const uint32_t *d_bits, const int64_t *d_lin, int64_t n,
                          uint8_t *d_keep, void *d_work, const int64_t *h_slice_interior,
                          const ppp_params *p, void *stream, int32_t *rounds);
int ppp_label_slice_renumber(const uint32_t *d_nodes, uint64_t n_nodes, int32_t *d_labels,
                             int32_t *d_slice_min, int32_t *d_slice_max, const ppp_params *p, void *stream);

/* sort keys (int64) that group pair rows by patch offset B - A, then by position of A: an
 * argsort of them is a good d_order for ppp_patch_graph                                    */
int ppp_pair_sort_keys(const uint32_t *d_rows, uint64_t n_rows, int64_t *d_keys,
                       const ppp_params *p, void *stream);
/* sort keys (int64) for ppp_patch_graph_by_patch: key >> 18 is the linear index of patch A (the
 * group), the low bits order a group's rows (intersecting windows first, then by B - A).
 * Rows whose patches are too far apart to share a stored consensus offset (|B - A|_i >
 * 2 (p_i - 1) on some axis) get PPP_PAIR_KEY_FAR: their affinity is exactly 0.0 whatever the
 * data, so a caller that pre-zeroes d_aff leaves them out of the groups.                    */
#define PPP_PAIR_KEY_FAR 0x7FFFFFFFFFFFFFFFll
int ppp_pair_group_keys(const uint32_t *d_rows, uint64_t n_rows, int64_t *d_keys,
                        const ppp_params *p, void *stream);

/* --- host stages (host pointers; they are host code in the reference as well) ---------
 * ppp_host_rank_order: all_patches + rank_patches_by_score (vote_instances.py:276,286-287,
 *   ranked_patches.py:21-30): interior foreground voxels in raster order, stably sorted by
 *   score descending.  out_lin holds linear voxel indices (capacity Z*Y*X); returns count. */
int64_t ppp_host_rank_order(const float *h_score, const uint8_t *h_foreground, const int32_t *vol,
                            const int32_t *patchshape, int64_t *out_lin);
/* ppp_host_cover_pass: one computeForegroundCoverLoop pass (foreground_cover.py:111-180) over
 *   n ranked patches; bits from ppp_patch_bits with fc_threshold; selected / mask / remaining
 *   are updated in place; score_threshold NaN = off, *stopped = 1 when it ended the pass.
 *   Returns #newly selected.                                                               */
int64_t ppp_host_cover_pass(uint8_t *h_mask_running, const uint8_t *h_overlap, const int32_t *vol,
                            const int32_t *patchshape, const int64_t *ranked_lin,
                            const float *ranked_score, const uint32_t *bits, int64_t n,
                            int32_t pix_th, double score_threshold, uint8_t *selected,
                            int64_t *remaining, int32_t *stopped);
/* ppp_host_cover_pass_marked: the same pass with `mark_close_neighboorhood`
 * (foreground_cover.py:141-143, 162-168): h_marked uint8 (Z,Y,X), in/out, shared by the passes of
 * one cover (NULL = the plain pass); a ranked patch with a marked centre is skipped, a selected
 * patch marks the box (0, +-3, +-3) around its centre with NumPy's slice semantics.         */
int64_t ppp_host_cover_pass_marked(uint8_t *h_mask_running, const uint8_t *h_overlap, const int32_t *vol,
                                   const int32_t *patchshape, const int64_t *ranked_lin,
                                   const float *ranked_score, const uint32_t *bits, int64_t n,
                                   int32_t pix_th, double score_threshold, uint8_t *selected,
                                   int64_t *remaining, int32_t *stopped, uint8_t *h_marked);
/* ppp_host_thin_cover: thinOutForegroundCover (foreground_cover.py:183-256), keep[n] out.   */
int64_t ppp_host_thin_cover(const uint8_t *h_mask, const int32_t *vol, const int32_t *patchshape,
                            const int64_t *sel_lin, const uint32_t *bits, int64_t n,
                            uint8_t *keep);

/* ppp_host_skeletonize_3d: the 3-d thinning behind `skeletonize_foreground` (vote_instances.py:
 * 219-224, stitch_patch_graph.py:756-759: skimage.morphology.skeletonize_3d = Lee / Kashyap / Chu
 * 1994, restated from the publication -- scikit-image is absent here, PARITY UNPINNED).
 * h_mask uint8 (Z,Y,X) 0 / non-zero, vol = {Z,Y,X}, h_out uint8 (Z,Y,X) 0 / 1; returns the number
 * of voxels kept or -1. */
int64_t ppp_host_skeletonize_3d(const uint8_t *h_mask, const int32_t *vol, uint8_t *h_out);
/* ppp_host_skel_rule_mismatches: the deletion rule of the thinning exists twice -- the predicates of
 * ppp_host_skeletonize_3d and the function of a 27-bit neighbourhood word that the device kernels
 * evaluate (csrc/ppp_skel_rule.hpp).  Neighbour pattern k < 2^26 enumerates the 26 neighbour bits (the
 * word without its centre bit 13, higher bits moved down; the centre is set).  Returns the number of
 * patterns in [first, first + count) on which the two disagree (0 over all 2^26), -1 when the range
 * leaves [0, 2^26].  Host only; large ranges are split over up to 16 threads. */
int64_t ppp_host_skel_rule_mismatches(uint32_t first, uint32_t count);
/* ppp_host_patch_pairs: computeAndStorePatchPairs (aff_patch_graph.py:43-110) with a grid
 *   hash instead of cKDTree; canonical row order (see file header of ppp_host.cpp).
 *   pairs == NULL returns the row count only.                                               */
int64_t ppp_host_patch_pairs(const int32_t *sel_zyx, int64_t n, const int32_t *patchshape,
                             int32_t max_ps_dist, int32_t include_single, int32_t *sorted_zyx,
                             uint32_t *pairs);

/* ppp_host_mws: mutex watershed on the patch graph (graph_mws.py:7-85 on the graph of
 *   setAffgraph, aff_patch_graph.py:31-40), host code like the reference.  pairs u32 [n][6],
 *   aff f32 [n]; vol = (Z,Y,X).  Writes every node of the graph (rows with aff != 0, first
 *   appearance order) to out_nodes int32 [cap][3] with its instance label in out_labels
 *   (1 + position of its component in the reference's output list; 0 = in no component).
 *   *n_labels = length of that list (emptied components included).  Returns the number of
 *   nodes, or -1 when cap is too small.                                                     */
int64_t ppp_host_mws(const uint32_t *pairs, const float *aff, int64_t n_rows, const int32_t *vol,
                     int32_t *out_nodes, int32_t *out_labels, int64_t cap, int64_t *n_labels);

/* ppp_host_mws_sorted: the loop of graph_mws.mws (:31-77) over an edge list that is already in
 *   the order the reference visits it (ppp_mws_edges makes it on the device): eu / ev int32
 *   [n_edges] node numbers, bit 31 of ev = attractive.  labels int32 [n_nodes] out (1 + position
 *   of the node's component in the reference's output list, 0 = none).  Returns the number of
 *   ids issued (emptied components included).                                               */
int64_t ppp_host_mws_sorted(const int32_t *eu, const int32_t *ev, int64_t n_edges, int64_t n_nodes,
                            int32_t *labels);

/* ppp_host_mws_sorted_stats: ppp_host_mws_sorted, which walks a long list in blocks and drops,
 *   between blocks and on several threads, the unvisited edges that can do nothing any more
 *   (csrc/ppp_host_mws.cpp; PPP_MWS_PRUNE=0: the plain loop, PPP_MWS_PRUNE_BLOCK / _MIN: block
 *   size and shortest list in edges).  Same labels and return value; stats int64
 *   [PPP_MWS_N_STATS] (may be null): [0] blocks run (0 = the plain loop), [1]-[4] edges dropped
 *   by rules 1-4, [5] edges visited, [6] threads, [7] prune passes; [1]+..+[5] = n_edges.    */
#define PPP_MWS_N_STATS 8
int64_t ppp_host_mws_sorted_stats(const int32_t *eu, const int32_t *ev, int64_t n_edges, int64_t n_nodes,
                                  int32_t *labels, int64_t *stats);

/* ppp_host_mws_sorted_classes: the plain loop, noting what each edge did in cls uint8 [n_edges]:
 *   attractive 0 new component, 1 joined one, 2 merged two, 3 same cluster, 4 refused by a mutex
 *   key; repulsive 5 same cluster, 6 key already there, 7 key inserted (tools/time_mws.py).  */
int64_t ppp_host_mws_sorted_classes(const int32_t *eu, const int32_t *ev, int64_t n_edges, int64_t n_nodes,
                                    int32_t *labels, uint8_t *cls);

/* ppp_host_pack_channels: the channel assignment of `no_overlap_per_channel`
 *   (graph_to_labeling.py:86-106: one painted volume, one .sum() and one masked test per component
 *   and channel) as a greedy walk over sizes and overlap pairs (closed form: ppp_pack_channels.hip).
 *   sizes int64 [n_labels]: voxels of component k (label k + 1); pairs u64 [n_pairs]: keys
 *   (b << 32) | a of overlapping labels 1 <= a < b <= n_labels, any order, repeats allowed.
 *   Component 0 and every component of at most min_voxels voxels (2000 in the reference) go to
 *   channel 0; any other goes to the first channel none of whose earlier components overlaps it,
 *   a new one if there is none.  chan_out int32 [n_labels], *n_channels_out = channels opened (0
 *   without components).  Returns the number of channels, -1 on bad arguments.              */
int64_t ppp_host_pack_channels(int64_t n_labels, const int64_t *sizes, const uint64_t *pairs, int64_t n_pairs,
                               int64_t min_voxels, int32_t *chan_out, int32_t *n_channels_out);

/* --- order-defining stages as device sorts (rocPRIM inside the library) ------------------
 * ppp_rank_order: all_patches + rank_patches_by_score (vote_instances.py:276,286-287,
 *   ranked_patches.py:21-30): the interior voxels with d_foreground != 0 in raster order, stably
 *   sorted by score descending.  d_lin int64 [capacity >= count], d_rank_score f32 (may be NULL);
 *   *count out.  Synchronises the stream.  Workspace: ppp_rank_order_workspace_bytes(p).
 * ppp_mws_edges: the edge list of the mutex watershed (setAffgraph + graph_mws.py:17-26): rows
 *   with aff != 0, in networkx's edge order (first appearance of the earlier endpoint, then row),
 *   stably sorted by |aff| descending.  Node numbers are positions in d_nodes u32 [n_nodes][3];
 *   d_eu / d_ev int32 [n_rows] out, bit 31 of d_ev = attractive (aff > 0); *n_edges out.  The
 *   rows must not repeat a node pair (the library's own pair lists never do).  Synchronises.  */
int64_t ppp_rank_order_workspace_bytes(const ppp_params *p);
int ppp_rank_order(const float *d_score, const uint8_t *d_foreground, int64_t *d_lin,
                   float *d_rank_score, int64_t *count, void *d_work, const ppp_params *p,
                   void *stream);
int64_t ppp_mws_edges_workspace_bytes(int64_t n_rows, int64_t n_nodes, const ppp_params *p);
int ppp_mws_edges(const uint32_t *d_pairs, const float *d_aff, int64_t n_rows, const uint32_t *d_nodes,
                  int64_t n_nodes, int32_t *d_eu, int32_t *d_ev, int64_t *n_edges, void *d_work,
                  const ppp_params *p, void *stream);

/* --- whole-volume post-steps of the label driver (ppp_postprocess.hip) ----------------------
 * They take no ppp_params: a map is described by its voxel count or its (Z, Y, X) extent.  Maps of
 * 2^31 voxels or more return PPP_ERR_UNSUPPORTED (the size queries return it as a negative value).
 * Ids are UNSIGNED: ids >= 2^31 order and index like any other.  All three synchronise the stream.
 *
 * ppp_post_compact_ids: remove_small_components + relabel (PatchPerPix/util/postprocess.py:24-37,
 *   :40-52; the driver's use: stitch_patch_graph.py:831-848), in place on d_ids u32 [n].  max_id
 *   bounds the ids of the map (a larger id: PPP_ERR_INVALID_ARG, map unchanged); the workspace holds
 *   two u32 tables of max_id + 2 slots.  Ids with at most `compsize` voxels become 0 (compsize < 0
 *   removes nothing); with relabel != 0 the surviving non-zero ids become start, start + 1, ... in
 *   ascending order of the old id (arithmetic modulo 2^32).  *n_kept = number of surviving ids.
 * ppp_post_dilate: the in-place ascending loop of stitch_patch_graph.py:871-880 (every instance, in
 *   ascending id order, dilated by one step of the 6-neighbourhood and painted over what is there)
 *   in closed form: a voxel of id a "survives" iff no face neighbour of smaller non-zero id survives;
 *   d_out[v] = the largest id among the survivors in v and its six face neighbours, else 0.  d_out
 *   must not be d_in.  *rounds = 1 + the number of sweeps over the voxels the first pass left open.
 * ppp_post_clean_mask: clean_mask (stitch_patch_graph.py:46-57: scipy.ndimage.label + bincount):
 *   d_out u8 [Z][Y][X] = 1 where d_mask != 0 and the voxel's connected component has more than `size`
 *   voxels, else 0 (d_out may be d_mask).  structure: 27 bits, bit (dz+1)*9 + (dy+1)*3 + (dx+1) set
 *   when offset (dz, dy, dx) connects; it must be centrosymmetric (scipy demands the same).
 *   *n_found / *n_kept = components found / kept.                                              */
int64_t ppp_post_compact_ids_workspace_bytes(int64_t n, uint32_t max_id);
int ppp_post_compact_ids(uint32_t *d_ids, int64_t n, uint32_t max_id, int64_t compsize, int32_t relabel,
                         uint32_t start, int64_t *n_kept, void *d_work, void *stream);
int64_t ppp_post_dilate_workspace_bytes(int32_t Z, int32_t Y, int32_t X);
int ppp_post_dilate(const uint32_t *d_in, uint32_t *d_out, int32_t Z, int32_t Y, int32_t X, int32_t *rounds,
                    void *d_work, void *stream);
int64_t ppp_post_clean_mask_workspace_bytes(int32_t Z, int32_t Y, int32_t X);
int ppp_post_clean_mask(const uint8_t *d_mask, uint8_t *d_out, int32_t Z, int32_t Y, int32_t X, uint32_t structure,
                        int64_t size, int64_t *n_found, int64_t *n_kept, void *d_work, void *stream);

/* --- postprocess_fg on the device (csrc/ppp_edt.hip, csrc/ppp_postprocess.hip) ------------------
 * The reference's `process_fg_prediction` branch (PatchPerPix/util/postprocess.py:122-199): the
 * thresholded foreground is labelled with the 3 x 3 x 3 structure, and a component of at most
 * `remove_small_comps` voxels is removed when all its voxels lie at a distance >= max_distance_to_fg
 * from the larger components (scipy.ndimage.distance_transform_edt).  Both calls work in integers only:
 * the distance is the exact SQUARED Euclidean distance, and the caller turns the reference's float
 * comparison into one integer bound (patchperpix_amd.postprocess.min_sq_distance).  Volumes of 2^31
 * voxels or more, or with Z^2 + Y^2 + X^2 >= 2^32 - 1 (a squared distance could reach the 32-bit
 * infinity), return PPP_ERR_UNSUPPORTED; the size queries return it as a negative value.
 *
 * ppp_post_edt_sq: d_out u32 [Z][Y][X], d_out[v] = min(min over voxels w with d_feature[w] != 0 of
 *   |v - w|^2, cap); cap = 0 means no cap, and then 0xFFFFFFFF is written where the volume holds no
 *   feature.  Three separable passes x -> y -> z between d_out and the workspace (one u32 volume),
 *   each an expanding window that stops at k^2 >= the best value so far: exact, and bounded by
 *   ceil(sqrt(cap)) steps per pass under a cap; without one the cost is the sum of the distances.
 *   Does not synchronise the stream.
 * ppp_post_fg_filter: the whole step.  d_mask u8 [Z][Y][X], 0 / non-zero.  Components are 26-connected;
 *   BIG: more than `compsize` voxels, SMALL: the others.  d_fg u8 (may be d_mask) = 1 on the voxels of
 *   big components and of small components with a voxel at a squared distance < min_d2 from a voxel of
 *   a big one, else 0.  min_d2 = 0: every small component is removed and no transform runs (the
 *   reference's else branch, remove_small_components).  No big component: every small component is
 *   removed (the minimum over an empty set; the reference's result is an artefact of scipy there).
 *   d_inst u32 (or NULL): the surviving components numbered 1, 2, ... in ascending order of their
 *   smallest raster index -- scipy.ndimage.label of d_fg.  stats[4] = components found, small ones,
 *   small ones removed, components kept.  Synchronises the stream once.  The workspace holds the
 *   union-find, label, count, distance and scan volumes: about 29 bytes per voxel.              */
int64_t ppp_post_edt_sq_workspace_bytes(int32_t Z, int32_t Y, int32_t X);
int ppp_post_edt_sq(const uint8_t *d_feature, uint32_t *d_out, int32_t Z, int32_t Y, int32_t X, uint32_t cap,
                    void *d_work, void *stream);
int64_t ppp_post_fg_filter_workspace_bytes(int32_t Z, int32_t Y, int32_t X);
int ppp_post_fg_filter(const uint8_t *d_mask, uint8_t *d_fg /* may be d_mask */, uint32_t *d_inst /* or NULL */,
                       int32_t Z, int32_t Y, int32_t X, int64_t compsize, uint32_t min_d2,
                       int64_t *stats /* [4]: found, small, removed, kept */, void *d_work, void *stream);

/* --- evaluate_patch on the device (csrc/ppp_eval.hip) --------------------------------------------
 * The reference's `evaluate_patch` (PatchPerPix/evaluate/evaluate_prediction.py:38-150) scores the dense
 * patch prediction against the ground-truth affinities of the label volume, per threshold.  Here it is
 * one streaming reduction: every prediction element is read once per pass of
 * ppp_eval_patch_thresholds_per_pass() thresholds, the ground-truth affinity is computed from the labels
 * on the fly and never stored.
 *   d_pred   [C][tz][Y][X], elements of PPP_F32 / PPP_F16 / PPP_BF16: the slices z0 .. z0 + tz of the
 *            prediction of the volume vol = (Z, Y, X); C = pz * py * px, patch = (pz, py, px), all odd;
 *            channel e = ((dz + rz) py + (dy + ry)) px + (dx + rx), r = patch / 2.  No halo.
 *   d_labels int32 [L][Z][Y][X], the WHOLE volume, values >= 0 (the caller checks; a negative value counts
 *            as background here).
 *   numinst[v] = #{c : labels[c][v] > 0}, ov[v] = numinst[v] > 1.
 *   G'[e][v] = 1 iff !ov[v], v + off(e) lies inside the volume and some channel c has labels[c][v] != 0 and
 *            labels[c][v] == labels[c][v + off(e)]  (gunpowder's seg_to_affgraph* as restated by the
 *            reference's util/train_util.py:523-695, with the centre's overlap zeroed as evaluate_patch does).
 *   P_t[e][v] = (ov[v] ? 0 : pred[e][v]) > thresholds[t]: the element widened exactly to float, a float
 *            compare, NaN false.  `thresholds` is a HOST array the caller has already rounded to the
 *            element type (float32 rounding for PPP_F32 and PPP_BF16, float16 rounding for PPP_F16: NumPy's
 *            compare of an array with a Python float); a value that is not finite: PPP_ERR_INVALID_ARG.
 *   d_counts int64 [1 + 2T], ADDED to (zero it before the first tile): num_gt = sum G', then per threshold
 *            num_pred_t = sum P_t and tp_t = sum P_t & G'.  Integer atomics: independent of the order.
 *   d_inter, d_union int32 [T][tz][Y][X], both or neither (NULL): per voxel sum_e P_t & G' and sum_e P_t | G'.
 * PPP_ERR_INVALID_ARG: C != pz py px, an even patch side, T < 1 or T > ppp_eval_patch_max_thresholds() (32),
 * z0 + tz > Z, tz < 1, L < 1.  PPP_ERR_UNSUPPORTED: volumes of 2^31 voxels or more, patches of more than
 * 65535 elements (the size query returns it as a negative value).  Does not synchronise the stream.
 * The workspace holds two int32 per voxel of the tile.                                              */
int32_t ppp_eval_patch_thresholds_per_pass(void);
int32_t ppp_eval_patch_max_thresholds(void);
int64_t ppp_eval_patch_workspace_bytes(const int32_t *vol /* [3] */, int32_t tz);
int ppp_eval_patch(const void *d_pred, int pred_dtype, int32_t C, const int32_t *d_labels, int32_t L,
                   const int32_t *vol /* [3] */, const int32_t *patch /* [3] */, int32_t z0, int32_t tz,
                   const float *thresholds /* host [T] */, int32_t T, int64_t *d_counts /* [1 + 2T] */,
                   int32_t *d_inter, int32_t *d_union /* [T][tz][Y][X] or NULL */, void *d_work, void *stream);

/* --- 3-d thinning of the foreground on the device (csrc/ppp_skeleton.hip) ----------------------
 * `skeletonize_foreground` (vote_instances.py:219-224, stitch_patch_graph.py:756-759: the cover mask, or
 * the bounding box in blockwise mode, is the 3-d skeleton of the foreground).  The result is DEFINED as
 * that of ppp_host_skeletonize_3d on the same mask, voxel for voxel (Lee / Kashyap / Chu 1994, the host
 * function's sequential re-check in its exact priority-parallel form); parity with scikit-image's
 * skeletonize_3d stays UNPINNED, as for the host function.
 * d_mask u8 [Z][Y][X], 0 / non-zero; d_out u8 [Z][Y][X], 0 / 1 (d_out may be d_mask).  *n_kept = voxels
 * kept; stats[3] = passes over the border directions, sub-iterations, rounds that had candidates to
 * decide.  The call synchronises the stream.  PPP_ERR_NO_DEVICE without a device (there is no CPU path
 * behind it); maps of 2^31 voxels or more, of more than 65535 slices or more than 262140 rows per slice:
 * PPP_ERR_UNSUPPORTED (the size query returns it as a negative value).  The workspace holds two bit
 * images of the padded volume, three lists of about Z*Y*X / 2 u32 entries and the round counters. */
int64_t ppp_skeletonize_3d_workspace_bytes(int32_t Z, int32_t Y, int32_t X);
int ppp_skeletonize_3d(const uint8_t *d_mask, uint8_t *d_out, int32_t Z, int32_t Y, int32_t X,
                       int64_t *n_kept, int32_t *stats /* [3]: passes, sub-iterations, rounds */,
                       void *d_work, void *stream);

/* --- the 3-d skeleton of EVERY instance of an id map in one pass (csrc/ppp_skeleton.hip) --------
 * The reference's `postprocess` task (util/postprocess.py:105-119, export_skeleton_nrrds) thins
 * `inst == label` once per instance.  Instances are disjoint and a verdict of the thinning reads voxels
 * of its own instance only, so the kernels of ppp_skeletonize_3d run over the whole map at once with
 * "neighbour present" = "alive and of the centre's id".
 * DEFINITION of the result: for every id L, { v : d_out[v] == L } equals
 * ppp_host_skeletonize_3d(d_labels == L) on the whole volume; parity with scikit-image's skeletonize_3d
 * stays UNPINNED, as for ppp_skeletonize_3d.
 * d_labels u32 [Z][Y][X]: 0 is background, every other 32-bit value is an id (ids of 2^31 and above
 * included: only equality is used, there is no table and no id limit).  d_out u32 [Z][Y][X]:
 * d_out[v] = d_labels[v] where v survives, else 0 (d_out may be d_labels).  *n_kept = voxels kept;
 * stats[3] as ppp_skeletonize_3d (a map with one id gives that function's counts).  The call
 * synchronises the stream.  Size limits, PPP_ERR_NO_DEVICE and PPP_ERR_UNSUPPORTED as
 * ppp_skeletonize_3d.  The workspace holds the two bit images, one u32 word per voxel (which of the 26
 * neighbours carry the voxel's id), three lists of Z*Y*X u32 entries and the round counters: about
 * 16 bytes per voxel.
 * (PPP_ABI_VERSION counts changes to ppp_params and to existing signatures; new entry points leave it.) */
int64_t ppp_skeletonize_labels_workspace_bytes(int32_t Z, int32_t Y, int32_t X);
int ppp_skeletonize_labels(const uint32_t *d_labels, uint32_t *d_out, int32_t Z, int32_t Y, int32_t X,
                           int64_t *n_kept, int32_t *stats /* [3] as ppp_skeletonize_3d */,
                           void *d_work, void *stream);

/* --- the contingency table of two label stacks in one pass (csrc/ppp_overlap.hip) ---------------
 * What every instance metric of the reference's `evaluate` step (run_ppp.py:1239-1262, evaluate_file of the
 * package evaluate-instance-segmentation) needs of the volumes: which id of A meets which id of B in how
 * many voxels, and every id's size.  The package is not vendored by the reference, so nothing here is
 * pinned to it: the DEFINITION is the one below, stated again in NumPy as
 * patchperpix_amd.evaluate_instances.overlap_counts_host.
 * d_a u32 [La][Z][Y][X], d_b u32 [Lb][Z][Y][X]: 0 is background, every other 32-bit value is an id (2^31 and
 * above and 0xFFFFFFFF included; no table, no id limit).  The result is a list of rows (a, b) with an int64
 * count:
 *   (a, b), a != 0 and b != 0 :  #{(i, j, v) : A[i][v] == a and B[j][v] == b}
 *   (a, 0)                    :  #{(i, v) : A[i][v] == a}
 *   (0, b)                    :  #{(j, v) : B[j][v] == b}
 * Rows with a zero count do not exist; rows are sorted ascending by (a, b) as unsigned pairs, so the
 * result is unique.  Integer sums only: bit-identical from run to run.
 * *n_rows (host) ALWAYS receives the number of rows.  With n_rows <= cap the rows are written to d_rows
 * u32 [cap][2] and d_counts i64 [cap]; with n_rows > cap NOTHING is written to either, the return code is
 * PPP_OK and the caller calls again with a larger cap.  cap = 0 with NULL outputs is the size query.
 * The call synchronises the stream twice: the number of partial counts sizes the rocPRIM sort on the host,
 * and n_rows is a host value.  The rows are written by a launch after the second synchronisation.
 * PPP_ERR_INVALID_ARG: La < 1, Lb < 1, cap < 0, a bad volume, NULL or misaligned pointers.
 * PPP_ERR_UNSUPPORTED (the size query returns it as a negative value): volumes of 2^31 voxels or more,
 * La Lb + La + Lb > 65535.  PPP_ERR_NO_DEVICE without a device.
 * The workspace covers the worst case, every voxel its own pair: 32 bytes per voxel and key stream, of
 * which there are La Lb + La + Lb (96 bytes per voxel for La = Lb = 1), plus rocPRIM's temporary storage
 * (histograms and scan states: the sort works in the two halves of the list and keeps no copy).
 * Cost: d_a is read once, d_b once per channel of d_a (one read of both for La = 1), and every voxel is
 * La Lb + La + Lb keys of work: maps with hundreds of channels a side are slow, not a case this pass is for.
 * ppp_label_overlap_table_entries: slots of the per-workgroup LDS table the pass counts in (tests size
 * their table-pressure cases by it); ppp_label_overlap_slot: that table's hash, the home slot of key (a, b)
 * (host function; tests build colliding keys from it); ppp_label_overlap_last_stats: of the last call in this
 * process, stats[3] = partial counts written, table flushes inside the pass's loop, items that went past
 * the table (tests assert by them that a case reached the path it is about). */
int32_t ppp_label_overlap_table_entries(void);
void ppp_label_overlap_last_stats(int64_t *stats /* [3] */);
uint32_t ppp_label_overlap_slot(uint32_t a, uint32_t b);
int64_t ppp_label_overlap_workspace_bytes(int32_t La, int32_t Lb, int32_t Z, int32_t Y, int32_t X);
int ppp_label_overlap(const uint32_t *d_a, int32_t La, const uint32_t *d_b, int32_t Lb,
                      int32_t Z, int32_t Y, int32_t X,
                      uint32_t *d_rows /* [cap][2] */, int64_t *d_counts /* [cap] */, int64_t cap,
                      int64_t *n_rows /* host */, void *d_work, void *stream);

/* --- the patch mosaic of visualize_patches on the device (csrc/ppp_mosaic.hip) ------------------
 * The reference's `reshape_affinities` / `reshape_affinities_3d` (PatchPerPix/visualize/patches.py:12-98)
 * show the predicted patch of every voxel as one tile of a mosaic, with a Python loop over the voxels.
 * Here it is one pass over a z-tile: a pure re-arrangement, no workspace.
 *   d_pred   [C][tz][Y][X], elements of PPP_F32 / PPP_F16 / PPP_BF16, C = pz py px, patch = (pz, py, px), sides
 *            >= 1 (neither odd nor equal sides are required); channel c = (k py + j) px + i.  Read-only:
 *            the ones the reference writes into its input are NOT written.
 *   d_out    [tz][Y py][X px] of the same element type:
 *              out[z][y py + j][x px + i] = 1                                          if j == 0 or i == 0
 *                                         = max over k of pred[(k py + j) px + i][z][y][x]   otherwise,
 *            the maximum NumPy's: a NaN among the pz values gives NaN.  pz = 1 is the 2-d mosaic.
 *   d_selected u8 [S][tz][Y][X] with S = 1 or 3 (pz = 1 only), or NULL with S = 0.  With it d_out is
 *            [3][tz][Y py][X px] and the tile of a voxel goes to ONE channel: S = 1, channel 0 where
 *            selected[0] is set, else channel 2; S = 3, the first of channels 0, 1, 2 whose flag is set, and
 *            to none where no flag is.  The other channels are zero there.
 * EVERY element of d_out is written, those zeros included: the caller does not clear it.  Channels with
 * j == 0 or i == 0 are not read; every other element of d_pred is read exactly once.
 * PPP_ERR_INVALID_ARG: C != pz py px, a side < 1, S not in {0, 1, 3}, S > 0 with pz > 1, d_selected and S
 * disagreeing.  PPP_ERR_UNSUPPORTED, by the sizes alone: a z-tile of 2^31 voxels or more, Y py or X px of 2^31
 * or more, px > 63 (the tile the kernel keeps in LDS), a grid the device would not run whole.
 * PPP_ERR_NO_DEVICE without a device.  Does not synchronise the stream.                            */
int ppp_patch_mosaic(const void *d_pred, int pred_dtype, int32_t C, const uint8_t *d_selected, int32_t S,
                     void *d_out, int32_t tz, int32_t Y, int32_t X, const int32_t *patch /* [3] */, void *stream);

/* --- the ground-truth patch affinities of a label volume as an array (csrc/ppp_gt_affs.hip) -----
 * The reference's `seg_to_affgraph_*_torch*` family (PatchPerPix/util/train_util.py:349-775): the BCE target
 * of the patch loss, made from the labels inside every training step (torch_model.py:201-223, :366-370,
 * :429-441) with a Python loop over the E edges.  Here it is one launch: the labels are read once, the output
 * is written once and never read back.  Only equality and "!= 0" are used: 0 is background, every other
 * 32-bit value is an id, negative ones included.  No workspace; neither call synchronises the stream.
 *   d_labels int32 [B][L][Z][Y][X], vol = (Z, Y, X); 2-d data is Z = 1 with zero z-offsets.
 *   d_nhood  int32 [E][3] on the DEVICE.
 * ppp_gt_affs_dense: nhood[e] is an offset of any size and sign.
 *   multi  (single = 0): out[b][e][v] = 1 iff v + nhood[e] lies inside the volume and some channel c has
 *          labels[b][c][v] != 0 and labels[b][c][v] == labels[b][c][v + nhood[e]], else 0: the same id in
 *          the SAME channel (train_util.py:523-610; its two foreground factors are implied).
 *   single (single = 1, L = 1, PPP_F32): out[b][e][v] = float(c * c) with c = labels[b][v] where
 *          c == labels[b][v + nhood[e]], else 0 -- the id SQUARED, the reference multiplies by the label
 *          values (train_util.py:613-695); the product is the 32-bit one, exact for |id| <= 46340.
 *   An offset with |n| >= the axis gives zeros (the reference: zeros at |n| == S, an exception beyond).
 *   halo   HOST [6] = min z, max z, min y, max y, min x, max x over nhood: it sizes the tile of labels a
 *          workgroup stages in LDS.  An edge outside it gets UNDEFINED values (never an access out of bounds).
 *   box    HOST [6] = z0, z1, y0, y1, x0, x1, non-empty and inside the volume: the voxels v that are written.
 *   d_out  [B][E][z1-z0][y1-y0][x1-x0] of out_dtype (0 and 1 are exact in all three); EVERY element is
 *          written, the caller does not clear it.  Offsets are 64-bit: E V may pass 2^31.
 *   ppp_gt_affs_dense_plan: what a call with these sizes does, without a launch (tests size their cases by it):
 *          plan[5] = tile z, y, x of a workgroup; 1 when tile + halo are staged in LDS, 0 when every neighbour is
 *          loaded from global memory (they do not fit 64 KiB); edge ranges a tile is split into.
 * ppp_gt_affs_samples: the patch form (train_util.py:349-520).
 *   d_samples int32 [N][4], rows (b, z, y, x): the CORNER of a patch of ps = (pz, py, px) voxels; nhood[e] is an
 *          index INTO the patch, ctr[3] the patch's centre index.  Duplicate rows are fine.
 *   d_out  [N][E] of out_dtype: out[n][e] = 1 iff some c has P[c][ctr] != 0 and P[c][ctr] == P[c][nhood[e]],
 *          P the patch of row n.  A voxel outside the volume reads as 0, as does an index outside [0, ps) and a
 *          row whose b is outside [0, B).  N = 0 returns PPP_OK and touches nothing.
 * PPP_ERR_INVALID_ARG: B < 1, L < 1, E < 1, a bad volume, an empty box or one that leaves the volume, a halo
 * minimum above its maximum, single with L != 1 or another type than PPP_F32, ctr outside [0, ps), N < 0, NULL
 * or misaligned pointers.  PPP_ERR_UNSUPPORTED: V >= 2^31 per batch item, E > 65535, a grid the device would
 * not run whole.  PPP_ERR_NO_DEVICE without a device.                                              */
int ppp_gt_affs_dense_plan(int32_t B, int32_t L, const int32_t *vol /* [3] */, int32_t E, const int32_t *halo /* [6] */,
                           const int32_t *box /* [6] */, int out_dtype, int32_t single, int32_t *plan /* [5] */);
int ppp_gt_affs_dense(const int32_t *d_labels, int32_t B, int32_t L, const int32_t *vol /* [3] */,
                      const int32_t *d_nhood, int32_t E, const int32_t *halo /* host [6] */,
                      const int32_t *box /* host [6] */, void *d_out, int out_dtype, int32_t single, void *stream);
int ppp_gt_affs_samples(const int32_t *d_labels, int32_t B, int32_t L, const int32_t *vol /* [3] */,
                        const int32_t *d_samples /* [N][4] */, int64_t N, const int32_t *d_nhood, int32_t E,
                        const int32_t *ps /* [3] */, const int32_t *ctr /* [3] */, void *d_out, int out_dtype,
                        void *stream);

/* --- the fused patch loss from the labels: masked BCE with logits, forward and backward (csrc/ppp_patch_loss.hip) ---
 * The reference's `add_affinities = "loss"` makes the target above only to feed it to MaskedBCEWithLogitsLoss
 * (experiments/flylight/setups/setup01/torch_loss.py:47-67, called at :127-129).  Here the target is consumed
 * where it is made and never stored: the forward reads the logits once, the backward reads them once and
 * writes the gradient once; nothing else of that size exists.
 *   G[b][e][v]  exactly the multi predicate of ppp_gt_affs_dense (same id in the same channel, offsets of any
 *               size, zero outside the volume), for the voxels v of `box`; labels, vol, nhood, halo, box as there.
 *   l(x, g)   = max(x, 0) - x g + log1p(exp(-|x|))
 * Dense form.  d_logits [B][E][bZ][bY][bX] of `dtype` (PPP_F32 / PPP_F16 / PPP_BF16, widened exactly in registers,
 *   float32 arithmetic per element), the box's extents; d_weight float32 [B][bZ][bY][bX] >= 0, or NULL.
 *     with weights     cnt = num_channels * sum w;  loss = sum w[b][v] l(x[b][e][v], G[b][e][v]) / cnt, 0 when cnt == 0
 *     without          cnt = B E bV (num_channels is not used)
 *     backward         d_grad[b][e][v] = s w[b][v] (sigmoid(x) - g) grad_out, s = 1 / cnt, 0 when cnt == 0 (the
 *                      reference's mean(loss) * 0.0); sigmoid(x) - g is formed as g ? -sigmoid(-x) : sigmoid(x)
 *                      from exp(-|x|), and the product is rounded to nearest-even into `dtype` AFTER the
 *                      multiplication by s w grad_out (a GradScaler's factor keeps float16 out of the subnormals).
 *   A voxel with w == 0 contributes 0 and gets gradient 0 WHATEVER its logits hold; a 16-byte group of logits whose
 *   weights are all zero is not read.  (The reference gives NaN there for a non-finite logit: 0 * inf.)
 *   d_loss   float32 [1].   d_state double [2] = (s, sum w -- B E bV without weights): carries s from the forward
 *            to the backward ON THE DEVICE.   d_grad_out float32 [1] on the DEVICE.
 *   d_counts int64 [3] or NULL: over ALL elements of the box, unweighted, the number with x > 0, with G, and with
 *            x > 0 && G (torch_loss.py:133-141 needs no more for jaccard and accuracy).  The call clears them;
 *            with counters every element is read, w == 0 or not.
 *   d_grad   the shape and type of d_logits; EVERY element is written, zeros included.
 *   d_work   ppp_patch_loss_workspace_bytes(B, L, vol, E, halo, box, dtype, 0) bytes, 8-byte aligned, forward only:
 *            one double per workgroup and sum.  Each workgroup writes its own slot and one workgroup adds the
 *            slots in a fixed order; there is no floating-point atomic, so loss, s and gradient have the same
 *            bits in every run.  Tiles and the staged / direct choice are ppp_gt_affs_dense_plan's.
 *   Offsets are 64-bit: B E bV may pass 2^31.
 * Sampled form (train_code; the reference passes no mask there).  d_logits / d_grad [N][E]; G[n][e], d_samples, ps,
 *   ctr as ppp_gt_affs_samples defines them; loss = sum l / (N E).  Workspace: box = NULL and N.  N = 0 returns
 *   PPP_OK and touches nothing (the caller's loss is 0, its gradient empty).
 * The one-channel "id squared" target is not served: a BCE against c * c has no meaning.
 * No entry point synchronises the stream or reads back to the host.  Errors as ppp_gt_affs_dense /
 * ppp_gt_affs_samples (PPP_ERR_INVALID_ARG: sizes, box, halo, ctr, N < 0, with weights a num_channels that is not
 * positive and finite, NULL or misaligned pointers; PPP_ERR_UNSUPPORTED: V >= 2^31, E > 65535, a grid the device
 * would not run whole; PPP_ERR_NO_DEVICE); ppp_patch_loss_workspace_bytes returns the negative code.            */
int64_t ppp_patch_loss_workspace_bytes(int32_t B, int32_t L, const int32_t *vol /* [3] */, int32_t E,
                                       const int32_t *halo /* [6], dense */, const int32_t *box /* [6], or NULL: sampled */,
                                       int dtype, int64_t N /* sampled */);
int ppp_patch_loss_dense_fwd(const void *d_logits, int dtype, const int32_t *d_labels, int32_t B, int32_t L,
                             const int32_t *vol /* [3] */, const int32_t *d_nhood, int32_t E, const int32_t *halo /* host [6] */,
                             const int32_t *box /* host [6] */, const float *d_weight /* or NULL */, double num_channels,
                             float *d_loss /* [1] */, double *d_state /* [2] */, int64_t *d_counts /* [3] or NULL */,
                             void *d_work, void *stream);
int ppp_patch_loss_dense_bwd(const void *d_logits, int dtype, const int32_t *d_labels, int32_t B, int32_t L,
                             const int32_t *vol /* [3] */, const int32_t *d_nhood, int32_t E, const int32_t *halo /* host [6] */,
                             const int32_t *box /* host [6] */, const float *d_weight /* or NULL */,
                             const double *d_state /* [2] */, const float *d_grad_out /* device [1] */, void *d_grad,
                             void *stream);
int ppp_patch_loss_samples_fwd(const void *d_logits, int dtype, const int32_t *d_labels, int32_t B, int32_t L,
                               const int32_t *vol /* [3] */, const int32_t *d_samples /* [N][4] */, int64_t N,
                               const int32_t *d_nhood, int32_t E, const int32_t *ps /* [3] */, const int32_t *ctr /* [3] */,
                               float *d_loss /* [1] */, double *d_state /* [2] */, void *d_work, void *stream);
int ppp_patch_loss_samples_bwd(const void *d_logits, int dtype, const int32_t *d_labels, int32_t B, int32_t L,
                               const int32_t *vol /* [3] */, const int32_t *d_samples /* [N][4] */, int64_t N,
                               const int32_t *d_nhood, int32_t E, const int32_t *ps /* [3] */, const int32_t *ctr /* [3] */,
                               const double *d_state /* [2] */, const float *d_grad_out /* device [1] */, void *d_grad,
                               void *stream);

/* --- synthetic input (bench / tests only; same hash as patchperpix_amd/synth.py) ------
 * fills d_pred (C,Z,Y,X) from a label volume d_labels int32 (Z,Y,X).  voxel_offset is the
 * linear index of local voxel 0 in the global volume (0 unless the buffers are a slab).    */
int ppp_synth_pred(const int32_t *d_labels, void *d_pred, int pred_dtype, uint32_t seed,
                   float hi, float lo, float noise, uint64_t voxel_offset, const ppp_params *p,
                   void *stream);
/* Counter calibration (bench / profiles only; no counterpart in the reference): moves a KNOWN
 * number of bytes -- n_read elements of d_src read with one element per lane and load, n_write
 * floats written to d_dst with one float per lane and store -- so that a rocprofv3 --pmc pass
 * containing the call yields counter / true-bytes ratios for FETCH_SIZE and WRITE_SIZE
 * (kernels calib_read_kernel / calib_write_kernel).                                          */
int ppp_counter_calibration(const void *d_src, int src_dtype, int64_t n_read, float *d_dst, int64_t n_write,
                            void *stream);

/* Is a prediction buffer "clean" (ppp_params.pred_clean)?  One streaming read of n_values
 * contiguous values: *d_unclean (device int32, overwritten) = 0 when every value lies in [0, 1]
 * (as a bit pattern: no negative zero, inf or nan) and is either > TH or < BG of p (the two class
 * tests of fillConsensusArray.cu:44-47, 94-124; with the shipped rule the only value in between is
 * TH itself); bit 0 set: a value outside [0, 1]; bit 1: a value in the dead zone.  The caller reads
 * the flag and sets p->pred_clean = 1 for calls on THAT buffer while its contents stay unchanged.
 * The reference has no such notion: its kernels branch per operand (fillConsensusArray.cu:44-60). */
int ppp_pred_check(const void *d_pred, int pred_dtype, int64_t n_values, int32_t *d_unclean, const ppp_params *p,
                   void *stream);

/* --- one read of the prediction for every compare against a threshold (csrc/ppp_prepass.hip) ---------
 * ppp_pred_check, the pre-pass of ppp_rank_patches_vm and ppp_patch_bits_volume each stream the whole
 * prediction and evaluate compares of the same values.  ppp_pred_prepass reads it once and leaves, in d_work:
 *   unclean   i32           the bits of ppp_pred_check over all C * Z * Y * X values
 *   M, info   the interleaved P / N masks and pair counts of the centres of score_box, byte for byte what the
 *             ranking call's own pre-pass writes; valid u8 [Z*Y*X] likewise (d_overlap as in ppp_rank_patches_vm)
 *   bits_vol  u32 [Z*Y*X][ceil(C/32)]   ppp_patch_bits_volume for fc_threshold (independent of p's thresholds)
 * and writes into d_score (float [Z][Y][X]) the scores that need no consensus: border centres, background
 * centres, centres without a first pixel.  Served: cubic patches of 5 / 7 / 9 without count_pos_neg and
 * ring_z -- ppp_pred_prepass_workspace_bytes returns 0 otherwise (-1: invalid parameters) and the caller keeps
 * the separate calls.  ppp_pred_prepass_layout: the byte offsets of {M, info, valid, bits_vol, unclean} in
 * d_work (the size query, the launch and this answer share one description).  p->cons_box is not looked at.
 * d_work: 16-byte aligned.  Does not synchronise.
 * ppp_rank_patches_vm_prepared: ppp_rank_patches_vm for a caller that holds such a d_work for the same score_box
 * and the same p (thresholds, overlap): no pre-pass runs, the prediction is not read; d_score must still hold
 * what ppp_pred_prepass wrote.  d_work: ppp_rank_prepared_workspace_bytes(p) (0: not served).
 * ppp_patch_bits_from_table: d_bits[k] = row of centre k (d_centres u32[n][3], inside the volume) of such a
 * bits_vol: ppp_patch_bits for a list of centres without touching the prediction again.                    */
int64_t ppp_pred_prepass_workspace_bytes(const ppp_box *score_box, const ppp_params *p);
int ppp_pred_prepass_layout(const ppp_box *score_box, const ppp_params *p, int64_t *offsets /* [5] */);
int ppp_pred_prepass(const void *d_pred, int pred_dtype, const uint8_t *d_overlap, double fc_threshold, float *d_score,
                     const ppp_box *score_box, void *d_work, const ppp_params *p, void *stream);
int64_t ppp_rank_prepared_workspace_bytes(const ppp_params *p);
int ppp_rank_patches_vm_prepared(const float *d_cons_vm, float *d_score, const ppp_box *score_box, void *d_prepass_work,
                                 void *d_work, const ppp_params *p, void *stream);
int ppp_patch_bits_from_table(const uint32_t *d_bits_vol, const uint32_t *d_centres, uint64_t n, uint32_t *d_bits,
                              const ppp_params *p, void *stream);

/* The same generator for a BOX of a larger volume (tile-wise generation, BASELINE config [3]:
 * a rank of the 1024^3 workload holds one tile + halo of the prediction at a time).
 * p: Z / Y / X = extent of the prediction box, origin_* = its position in the volume;
 * d_labels: int32 labels over label_box = {z0, y0, x0, z1, y1, x1} (global), which must hold the
 * box grown by the patch radius (clipped to global_dims = {Z, Y, X}); the noise counter is the
 * global voxel's: bit-identical to ppp_synth_pred on the whole volume. */
int ppp_synth_pred_box(const int32_t *d_labels, const int32_t *label_box, void *d_pred, int pred_dtype,
                       uint32_t seed, float hi, float lo, float noise, const int32_t *global_dims,
                       const ppp_params *p, void *stream);

/* --- ppp+dec: tail of the patch decoder, fused with the scatter into the prediction block ------
 * replaces, for the shipped decoder (default_train_code.toml [model.autoencoder]: num_fmaps
 * [64, 128], kernel_size 3, num_repetitions 2, resize_conv, patchshape 7^3), the last stage of
 * Autoencoder.forward (torch_model.py:537-544: up[1] = nearest upsampling x2 + conv 64 -> 1 + ReLU,
 * up_conv[1] = two 1 -> 1 convolutions without activation, centre crop 8^3 -> 7^3) and the
 * per-voxel scatter of decode_sample (decode.py:61-65) with its float32 (C, Z, Y, X) array.
 * d_x   : float32 [n][fmaps = 64][side^3 = 4^3], the output of up_conv[0] for n foreground voxels
 * d_w1  : float32 [64][27] (= the conv weight [1][64][3][3][3]); d_w2, d_w3: float32 [27]; b*: biases
 * d_dst : int64 [n] linear voxel index of every decoded voxel in the prediction block
 * d_pred: the (C = 343, Z, Y, X) block described by p (float16 or float32): pred[r][dst] written
 * float arithmetic: f32 MFMA over the channels, f32 sums over the taps; checked against the torch
 * restatement of the same layers within a tolerance (the reference ships no decoder to pin to). */
int ppp_decode_tail(const float *d_x, int64_t n, int32_t fmaps, int32_t side, const float *d_w1, float b1,
                    const float *d_w2, float b2, const float *d_w3, float b3, const int64_t *d_dst,
                    void *d_pred, int pred_dtype, const ppp_params *p, void *stream);
/* The same tail, arithmetic and float16 rounding included, with patch b stored as the ROW
 * d_rows[d_dst[b]][0 .. C) of a rows table (below) instead of a column of a block: d_dst holds row
 * numbers, C must be 343.  PPP_F32 / PPP_F16, as ppp_decode_tail. */
int ppp_decode_tail_rows(const float *d_x, int64_t n, int32_t fmaps, int32_t side, const float *d_w1, float b1,
                         const float *d_w2, float b2, const float *d_w3, float b3, const int64_t *d_dst,
                         void *d_rows, int rows_dtype, int32_t C, void *stream);

/* --- a prediction kept as ROWS for the voxels of a mask only (no counterpart in the reference, whose
 * decode writes the dense array, zero outside the foreground: decode.py:43-65) ---------------------
 * d_mask  uint8 (Z, Y, X), non-zero = the voxel has a row; row k belongs to the k-th such voxel in
 *         raster order (x fastest).
 * d_rows  [n_rows][C], C contiguous, elements of PPP_F32 / PPP_F16 / PPP_BF16: moved as bits, never
 *         converted.  Row numbers and n_rows * C are 64-bit.
 * d_index ppp_rows_index_bytes(Z, Y, X) bytes (8-byte aligned), filled by ppp_rows_index_build: the
 *         mask as 64-bit words over the linear voxel index and an int64 count of the mask voxels
 *         before each word -- any voxel's row number in O(1), 0.25 bytes per voxel (plus under 1 KiB).
 *         ppp_rows_index_build runs on the device, writes *n_rows and synchronises the stream.
 * ppp_rows_expand   writes the WHOLE (C, bz, by, bx) box at d_pred_box: a voxel with a row gets the
 *         row's C values, every other voxel zeros in all C channels (the kernel stores them itself).
 * ppp_rows_compact  the inverse on a box: the rows of the box's mask voxels are written from the dense
 *         box, every other row stays untouched.
 * d_rows and d_pred_box must be 4-byte aligned.  PPP_ERR_UNSUPPORTED for 2^31 voxels or more (the size
 * query returns that code too). */
int64_t ppp_rows_index_bytes(int32_t Z, int32_t Y, int32_t X);
int ppp_rows_index_build(const uint8_t *d_mask, int32_t Z, int32_t Y, int32_t X,
                         void *d_index, int64_t *n_rows, void *stream);
int ppp_rows_expand(const void *d_rows, int dtype, int32_t C, const void *d_index,
                    int32_t Z, int32_t Y, int32_t X, const ppp_box *box,
                    void *d_pred_box, void *stream);
int ppp_rows_compact(const void *d_pred_box, int dtype, int32_t C, const ppp_box *box,
                     const void *d_index, int32_t Z, int32_t Y, int32_t X,
                     void *d_rows, void *stream);

/* --- a stored zarr chunk to its place in a device tensor (csrc/ppp_chunk.hip) -------------------------
 * The reference loads a prediction with zarr / numcodecs on the host (utilVoteInstances.py:136-251); here the
 * host runs the codec only (zstd, lz4, zlib) and the device does the rest in one pass over the chunk:
 * un-shuffle, optional value flags, scatter.  There is no un-shuffled copy of the chunk on the device.
 *
 * d_src (4-byte aligned): the `nbytes` decompressed, still shuffled bytes of ONE chunk, the blocks of a
 *   Blosc-1 frame back to back: block b covers bytes [b * blocksize, min(nbytes, (b + 1) * blocksize)).
 *   PPP_SHUFFLE_BIT: of the nel = bsize / typesize elements of a block the first n = nel / 8 * 8 are held as
 *   8 * typesize planes of n / 8 bytes, plane 8 j + k = bit k of byte j, element e at bit e % 8 of byte e / 8
 *   (little bit order); the remaining elements follow as they are.  PPP_SHUFFLE_BYTE: typesize runs of nel
 *   bytes, run j = byte j of every element.  PPP_SHUFFLE_NONE: the chunk as it is (uncompressed, zlib and
 *   gzip arrays); blocksize is ignored.  nbytes must be the chunk's element count times typesize and
 *   blocksize a multiple of typesize, at most 2^30.
 * geometry: ndim <= 4 axes, C order; chunk_shape; chunk_origin = the array coordinate of the chunk's first
 *   element; the selection [sel_lo, sel_hi) in array coordinates.  d_dst is a C-contiguous tensor of shape
 *   sel_hi - sel_lo with elements of typesize bytes (aligned to typesize).  The intersection of chunk and
 *   selection is written to its place and NOTHING else; an empty intersection is a successful call without a
 *   launch.  Runs of the fastest axis go out as 16-, 8- or 4-byte stores where they land so aligned, else by
 *   element.
 * flags: d_flags = NULL, or three device int32 {any x < 0, any x > 1, any NaN} over the ELEMENTS WRITTEN, read
 *   as flags_dtype = PPP_F16 (typesize 2, compared after exact widening) or PPP_F32 (typesize 4).  A flag is
 *   only ever set to 1: the caller zeroes the three once and reads them once after all the calls of a load.
 *   -0.0 sets none.
 * typesize other than 1, 2, 4 (and more than 4 axes): PPP_ERR_UNSUPPORTED -- the caller un-shuffles on the
 * host.  Asynchronous on `stream`; no workspace. */
enum ppp_shuffle { PPP_SHUFFLE_NONE = 0, PPP_SHUFFLE_BYTE = 1, PPP_SHUFFLE_BIT = 2 };
int ppp_chunk_scatter(const void *d_src, int64_t nbytes, int32_t typesize, int64_t blocksize, int32_t shuffle,
                      int32_t ndim, const int64_t *chunk_shape, const int64_t *chunk_origin,
                      const int64_t *sel_lo, const int64_t *sel_hi, void *d_dst,
                      int32_t flags_dtype, int32_t *d_flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PPP_MI355X_H */
