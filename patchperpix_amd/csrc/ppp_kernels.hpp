// ppp_kernels.hpp -- launchers implemented by the .hip translation units.
#pragma once
#include <stdlib.h>
#include <string.h>
#include "ppp_common.hpp"

namespace ppp {

// Development switches (PPP_* environment variables that select a kernel variant or a tile
// shape) are read ONCE per process -- at their first use, and again only after ppp_reload_env()
// (what the tests call after changing one) -- never on every launch.
int env_epoch();
void env_reload();
struct EnvSwitch {
    const char *name;
    int seen = -1;
    bool is_set = false;
    char val[32] = {0};
    explicit EnvSwitch(const char *n) : name(n) {}
    // the variable's value, nullptr when unset
    const char *get() {
        if (seen != env_epoch()) {
            const char *e = getenv(name);
            is_set = e != nullptr;
            if (e) { strncpy(val, e, sizeof(val) - 1); val[sizeof(val) - 1] = 0; }
            seen = env_epoch();
        }
        return is_set ? val : nullptr;
    }
};


hipError_t launch_consensus(const void *pred, int dtype, const uint8_t *ov, float *cons,
                            float *cnt, const Geo &G, hipStream_t s);
hipError_t launch_consensus_v2(const void *pred, int dtype, const uint8_t *ov, float *cons,
                               float *cnt, const Geo &G, hipStream_t s);
const char *last_consensus_kernel();
bool consensus_v3_supported(const Geo &G);
hipError_t launch_consensus_v3(const void *pred, int dtype, const uint8_t *ov, float *cons,
                               float *cnt, const Geo &G, hipStream_t s);
// S1 over item lists (ppp_consensus_sparse.hip, ppp_consensus_v3.hip).  item = run * n_rows + row
struct V3Items { int flat, n_rows, runs_per_line, bZ2; long long n_runs, n_items; };
V3Items consensus_v3_items(const Geo &G);
hipError_t launch_consensus_v3_lists(const void *pred, int dtype, const uint8_t *ov, float *cons, float *cnt,
                                     const Geo &G, const uint32_t *active, long long n_active,
                                     const uint32_t *inactive, long long n_inactive, hipStream_t s);
size_t consensus_sparse_workspace_bytes(const Geo &G);
// counts the items (total, active: one device -> host read, synchronises `s`), then launches: the
// lists when mode = 1, or mode = 0 and the active share is below the measured break-even; the dense
// kernel otherwise.  took_lists: what it chose.
hipError_t run_consensus_sparse(const void *pred, int dtype, const uint8_t *ov, float *cons, float *cnt,
                                const Geo &G, void *work, int mode, long long *total, long long *active,
                                int *took_lists, hipStream_t s);
void note_consensus_kernel(const char *name);
// 1 when the last S1 launch was the packed kernel's short classification (CLEAN = true), else 0
// (ppp_consensus_short_form)
int last_consensus_short_form();
void note_consensus_short_form(int on);
// the S2 / S5 kernel the last launch took (ppp_rank_kernel_name, ppp_patch_graph_kernel_name)
const char *last_rank_kernel();
void note_rank_kernel(const char *name);
const char *last_patch_graph_kernel();
// geometry: how the per-patch kernel got its window's sizes, "cube" (compiled in) or "generic" (read from
// Geo); "none" for the other S5 kernels (ppp_patch_graph_kernel_geometry)
const char *last_patch_graph_geometry();
void note_patch_graph_kernel(const char *name, const char *geometry = "none");
hipError_t launch_consensus_part(const void *pred, int dtype, const uint8_t *ov, float *cons, const Geo &G,
                                 hipStream_t s);
hipError_t launch_rank(const void *pred, int dtype, const float *cons, const uint8_t *ov,
                       float *score, const ppp_box &sb, const Geo &G, hipStream_t s);
hipError_t launch_rank_v2(const void *pred, int dtype, const float *cons, const uint8_t *ov,
                          float *score, const ppp_box &sb, const Geo &G, hipStream_t s);
bool rank_vm_supported(const Geo &G);
size_t rank_vm_workspace_bytes(const ppp_box &sb, const Geo &G);
hipError_t launch_rank_vm(const void *pred, int dtype, const float *S, const uint8_t *ov, float *score,
                          const ppp_box &sb, void *work, const Geo &G, hipStream_t s);
bool rank_wg_supported(const Geo &G);
size_t rank_wg_workspace_bytes(const ppp_box &sb, const Geo &G);
// the launcher's plan for this box, without a launch: out = tile z, y, x; z step; tiles; splits and order
// slots per XCD; 1 for XCD ranges of equal weight.  resident_per_cu / cus_per_xcd <= 0: ask the device
void rank_wg_plan(const ppp_box &sb, const Geo &G, int resident_per_cu, int cus_per_xcd, int32_t out[8]);
// what that plan assumed of a CU: out = the thickness that sizes the kernel's LDS arrays, workgroups per CU,
// LDS bytes per workgroup, CUs per XCD
void rank_wg_plan_residency(const ppp_box &sb, const Geo &G, int resident_per_cu, int cus_per_xcd, int32_t out[4]);
#ifdef PPP_RW_STAMPS
size_t rank_wg_stamps_offset(const ppp_box &sb, const Geo &G);   // where the stamps lie in that workspace
#endif
hipError_t launch_rank_wg(const void *pred, int dtype, const float *S, const uint8_t *ov, float *score,
                          const ppp_box &sb, void *work, const Geo &G, hipStream_t s);
// ... with M / info / valid of the score box made by launch_pred_prepass (pre_work: its workspace); `work` holds
// rank_wg_prepared_workspace_bytes
size_t rank_wg_prepared_workspace_bytes(const Geo &G);
hipError_t launch_rank_wg_prepared(const float *S, float *score, const ppp_box &sb, void *pre_work, void *work,
                                   const Geo &G, hipStream_t s);
hipError_t launch_rank_valid(const void *pred, int dtype, const uint8_t *ov, uint8_t *valid, const Geo &G, hipStream_t s);
// one read of the prediction for the clean flag, S2's masks and the cover's per-voxel patch bits (ppp_prepass.hip)
struct PrepassWork {
    uint32_t *M, *info;       // as rank_wg_kernel reads them (ppp_rank_masks.hpp)
    uint8_t *valid;           // [V]
    uint32_t *bits_vol;       // [V][ceil(C / 32)]
    int32_t *unclean;         // the bits of ppp_pred_check
};
bool pred_prepass_supported(const Geo &G);
PrepassWork pred_prepass_layout(Carver &c, const ppp_box &sb, const Geo &G);
size_t pred_prepass_workspace_bytes(const ppp_box &sb, const Geo &G);
hipError_t launch_pred_prepass(const void *pred, int dtype, const uint8_t *ov, float fc_thresh, float *score,
                               const ppp_box &sb, void *work, const Geo &G, hipStream_t s);
hipError_t launch_patch_bits_from_table(const uint32_t *bits_vol, const uint32_t *centres, uint64_t n, uint32_t *bits,
                                        const Geo &G, hipStream_t s);
hipError_t launch_patch_graph(const void *pred, int dtype, const float *cons,
                              const uint32_t *pairs, const uint32_t *order, uint64_t n,
                              float *aff, const Geo &G, hipStream_t s);
int patch_graph_pa_chunk(const Geo &G, bool small = false);
hipError_t launch_patch_graph_pa(const void *pred, int dtype, const float *S, const uint32_t *rows,
                                 const uint32_t *order, const long long *group_start,
                                 const long long *chunk_offsets, int n_groups, long long n_blocks,
                                 int chunk, float *aff, const long long *drop_off,
                                 const unsigned long long *drops, const long long *bits_centres, int n_bits,
                                 const uint32_t *bits, const Geo &G, hipStream_t s);
hipError_t launch_patch_fg_bits(const void *pred, int dtype, const long long *centres, long long n,
                                uint32_t *table, const Geo &G, hipStream_t s);
long long patch_graph_lcg_words(const Geo &G, int dz, int dy, int dx);
// bits [first_bit, first_bit + n_bits) of a patch's bit words as one value: the per-patch kernel's own function, on the host
unsigned long long patch_plane_bits(const uint32_t *words, int n_words, int first_bit, int n_bits);
hipError_t launch_patch_graph_lcg(const void *pred, int dtype, const uint32_t *rows, const uint32_t *order,
                                  const long long *lcg_pos, long long n, const long long *drop_off,
                                  unsigned long long *drops, const Geo &G, hipStream_t s);
hipError_t launch_label(const uint32_t *pairs, const float *aff, uint64_t n,
                        const uint32_t *nodes, uint64_t n_nodes, uint32_t *node_key, void *work,
                        const Geo &G, hipStream_t s);
hipError_t launch_pairs_count(const int32_t *pts, int64_t n, const int *box, int l1max,
                              int64_t *counts, hipStream_t s, const int64_t *subset = nullptr,
                              int64_t m = 0, bool slices = false);
hipError_t launch_pairs_subset(const int32_t *pts, int64_t n, const int *box, int l1max,
                               const int64_t *subset, int64_t m, const int64_t *local_off,
                               const int64_t *gid_off, int64_t n_local_rows, int64_t n_rows_total,
                               int include_single, uint32_t *rows, long long *gid, hipStream_t s);
size_t label_workspace_bytes(const Geo &G);
hipError_t launch_label_begin(const uint32_t *nodes, uint64_t n_nodes, void *work, const Geo &G,
                              hipStream_t s);
hipError_t launch_label_add(const uint32_t *pairs, const float *aff, const long long *gid,
                            long long gid0, uint64_t n, void *work, const Geo &G, hipStream_t s);
hipError_t launch_label_union_edges(const long long *ea, const long long *eb, uint64_t n,
                                    void *work, const Geo &G, hipStream_t s);
hipError_t launch_label_finish(const uint32_t *nodes, uint64_t n_nodes, long long *key64,
                               uint32_t *key32, void *work, const Geo &G, hipStream_t s);
hipError_t launch_pairs_fill(const int32_t *pts, int64_t n, const int *box, int l1max,
                             const int64_t *offsets, int64_t n_pair_rows, int include_single,
                             uint32_t *rows, hipStream_t s, bool slices = false);
hipError_t launch_pair_group_keys(const uint32_t *rows, uint64_t n, int64_t *keys, const Geo &G,
                                  hipStream_t s);
hipError_t launch_pair_keys(const uint32_t *rows, uint64_t n, int64_t *keys, const Geo &G,
                            hipStream_t s);
// the reference's NumPy-semantics stages (cuda=False), ppp_numpy_path.hip
hipError_t launch_np_consensus(const void *pred, int dtype, const uint8_t *fg, int16_t *cons, const Geo &G,
                               double th, hipStream_t s);
hipError_t launch_np_rank(const void *pred, int dtype, const uint8_t *fg, const int16_t *cons, int32_t *score,
                          const Geo &G, double th, hipStream_t s);
hipError_t launch_np_graph(const void *pred, int dtype, const uint8_t *mask, const int16_t *cons,
                           const int32_t *rows, uint64_t n, long long *weight, int32_t *count, const Geo &G,
                           double th, hipStream_t s);
hipError_t launch_paint_rows(const void *rows, int dtype, const uint32_t *nodes, const uint32_t *labels,
                             uint64_t n, uint32_t *inst, const Geo &G, hipStream_t s);
hipError_t launch_paint(const void *pred, int dtype, const uint32_t *nodes,
                        const uint32_t *labels, uint64_t n, uint32_t *inst, const Geo &G,
                        hipStream_t s);
// no_overlap_per_channel: sizes + overlap pairs, paint by channel (ppp_pack_channels.hip)
size_t pack_scan_workspace_bytes(const Geo &G, const ppp_box &own);
hipError_t run_pack_scan_count(const void *pred, int dtype, const uint32_t *nodes, const uint32_t *labels, uint64_t n_nodes,
                               uint32_t n_labels, const ppp_box &own, unsigned long long *sizes, long long *n_pairs,
                               void *work, const Geo &G, hipStream_t s);
hipError_t run_pack_scan_fill(const void *pred, int dtype, const ppp_box &own, unsigned long long *pairs, long long n_pairs,
                              void *work, const Geo &G, hipStream_t s);
hipError_t launch_paint_channels(const void *pred, int dtype, const uint32_t *nodes, const uint32_t *labels, uint64_t n,
                                 const uint32_t *chan, uint32_t n_labels, uint32_t n_channels, uint32_t *out,
                                 const Geo &G, hipStream_t s);
hipError_t launch_cons_to_voxel_major(const float *compact, float *S, const Geo &G,
                                      hipStream_t s);
hipError_t launch_cons_planes_to_rows(const float *planes, const ppp_box &pb, float *S, const Geo &G,
                                      hipStream_t s);
hipError_t launch_cons_to_reference(const float *compact, float *ref, const Geo &G,
                                    hipStream_t s);
hipError_t launch_patch_bits(const void *pred, int dtype, const uint32_t *centres, uint64_t n,
                             float thresh, uint32_t *bits, const Geo &G, hipStream_t s);
hipError_t launch_patch_bits_volume(const void *pred, int dtype, float thresh, uint32_t *bits_vol,
                                    const Geo &G, hipStream_t s);
hipError_t launch_synth(const int32_t *labels, void *pred, int dtype, uint32_t seed, float hi,
                        float lo, float noise, unsigned long long voxel_offset, const Geo &G,
                        hipStream_t s);

hipError_t launch_pred_check(const void *pred, int dtype, long long n, const Geo &G, int *unclean, hipStream_t s);
hipError_t launch_counter_calibration(const void *src, int dtype, long long n_read, float *dst, long long n_write,
                                      hipStream_t s);
hipError_t launch_synth_box(const int32_t *labels, const int *lb, void *pred, int dtype, uint32_t seed,
                            float hi, float lo, float noise, const int *gdim, const Geo &G, hipStream_t s);

hipError_t launch_decode_tail(const float *X, long long B, int F, int S, const float *W1, float b1,
                              const float *W2, float b2, const float *W3, float b3, const long long *dst,
                              void *pred, int dtype, const Geo &G, hipStream_t s);

// the same tail with patch b stored as a row, rows[dst[b]][0 .. C), instead of a column of the block
hipError_t launch_decode_tail_rows(const float *X, long long B, int F, int S, const float *W1, float b1,
                                   const float *W2, float b2, const float *W3, float b3, const long long *dst,
                                   void *rows, int dtype, hipStream_t s);

// a prediction kept as rows of the mask voxels (ppp_rows.hip): index, expand into a box, compact from a box
size_t rows_index_bytes(long long V);
hipError_t run_rows_index_build(const uint8_t *mask, long long V, void *index, long long *n_rows, hipStream_t s);
hipError_t launch_rows_move(bool expand, void *rows, int elem_bytes, int C, const void *index, int Z, int Y, int X,
                            const ppp_box &bx, void *box, hipStream_t s);

size_t cover_workspace_bytes(long long n, const Geo &G);
hipError_t run_cover_pass(uint8_t *mask, const uint32_t *bits, long long bits_vox, const long long *lin,
                          long long n, int pix_th, int32_t *state, int32_t *cleared, void *work,
                          const Geo &G, hipStream_t s, int *rounds, uint32_t *mark_bits = nullptr);
// `mark_close_neighboorhood`: the mark volume (bits, [Z*Y][row words] like the running mask) and its rebuild
// from a list of selected centres; `select_patches_overlap_neighborhood`: rounds of 6-neighbour dilation
size_t cover_mark_bits_bytes(const Geo &G);
hipError_t run_cover_marks_from_selected(const long long *lin, const uint8_t *sel, long long n, uint32_t *mark_bits,
                                         const Geo &G, hipStream_t s);
size_t mask_dilate_workspace_bytes(const Geo &G);
hipError_t run_mask_dilate(const uint8_t *in, uint8_t *out, int iterations, int use_z, void *work, const Geo &G,
                           hipStream_t s);

// x and y passes of the rounds' neighbourhood minimum (radius p - 1) on caller-owned volumes of 4- or 8-byte elements
hipError_t run_minfilter_xy(const void *in, void *scratch, void *out, int elem_bytes, const Geo &G, hipStream_t s);

size_t rank_order_workspace_bytes(const Geo &G);
hipError_t run_rank_order(const float *score, const uint8_t *fg, long long *lin, float *out_score,
                          long long *n_out, void *work, const Geo &G, hipStream_t s);
size_t mws_edges_workspace_bytes(long long n_rows, long long n_nodes, const Geo &G);
hipError_t run_mws_edges(const uint32_t *rows, const float *aff, long long n_rows, const uint32_t *nodes,
                         long long n_nodes, int32_t *out_u, int32_t *out_v, long long *n_edges, void *work,
                         const Geo &G, hipStream_t s);

size_t thin_workspace_bytes(long long n, const Geo &G);
hipError_t run_thin_cover(const uint8_t *mask, const uint32_t *bits, const long long *lin, long long n,
                          uint8_t *keep, void *work, const Geo &G, hipStream_t s, int *rounds,
                          const long long *slice_interior = nullptr);
hipError_t launch_label_slice_renumber(const uint32_t *nodes, uint64_t n, int32_t *labels, int32_t *slice_min,
                                       int32_t *slice_max, const Geo &G, hipStream_t s);

hipError_t cover_open(const uint8_t *mask, const long long *lin, const int32_t *rankid, long long n,
                      const int32_t *state, int32_t *cleared, void *work, const Geo &G, hipStream_t s);
hipError_t cover_step_count(const uint32_t *bits, int pix_th, int32_t *state, void *work,
                            const Geo &G, hipStream_t s);
hipError_t cover_step_select(const uint32_t *bits, int pix_th, int32_t *state, int32_t *cleared, void *work,
                             int gZ, const Geo &G, hipStream_t s);
// set-cover thinning sharded over ranks by z (round 6)
size_t thin_shard_workspace_bytes(const Geo &G);
hipError_t thin_open(const uint8_t *mask, const long long *lin, const int32_t *gidx, long long n, int32_t *state,
                     int32_t *sel_count, int32_t *cleared, void *work, const Geo &G, hipStream_t s);
hipError_t thin_step_count(const uint32_t *bits, int32_t *state, void *work, const Geo &G, hipStream_t s);
hipError_t thin_step_select(const uint32_t *bits, int32_t *state, int32_t *sel_count, int32_t *cleared, void *work,
                            int gZ, const Geo &G, hipStream_t s);
// the steps both share, on a sharded cover's (K = int32_t ranks) or thinning's (K = long long keys) workspace;
// round_zone: import = keys / mask / clean are read into the zone of local slices [z_lo, z_hi), else written from it
template <typename K> hipError_t round_step_filter(void *work, const Geo &G, hipStream_t s);
template <typename K> hipError_t round_alive(void *work, const Geo &G, int32_t *alive, hipStream_t s);
template <typename K> hipError_t round_close(uint8_t *mask, void *work, const Geo &G, hipStream_t s);
template <typename K>
hipError_t round_zone(bool import, void *work, int z_lo, int z_hi, int own_lo, int own_hi, K *keys, uint8_t *mask,
                      uint8_t *clean, const Geo &G, hipStream_t s);

// post-steps of the label driver (ppp_postprocess.hip)
size_t post_compact_workspace_bytes(uint32_t max_id);
hipError_t run_post_compact(uint32_t *ids, long long n, uint32_t max_id, long long compsize, int relabel,
                            uint32_t start, long long *n_kept, void *work, hipStream_t s);
size_t post_dilate_workspace_bytes(long long V);
hipError_t run_post_dilate(const uint32_t *in, uint32_t *out, int Z, int Y, int X, int *rounds, void *work, hipStream_t s);
size_t post_clean_mask_workspace_bytes(long long V);
hipError_t run_post_clean_mask(const uint8_t *mask, uint8_t *out, int Z, int Y, int X, uint32_t structure,
                               long long size, long long *n_found, long long *n_kept, void *work, hipStream_t s);

// exact squared Euclidean distance transform (ppp_edt.hip): out[v] = min(min over feature voxels w of
// |v - w|^2, cap), cap = 0: no cap, 0xFFFFFFFF where there is neither feature nor cap
struct EdtWork {
    uint32_t *tmp;       // [V]: the volume between the y and the z pass
};
EdtWork edt_layout(Carver &c, long long V);
size_t post_edt_workspace_bytes(long long V);
hipError_t launch_edt_sq(const uint8_t *feature, uint32_t *out, int Z, int Y, int X, uint32_t cap, const EdtWork &W,
                         hipStream_t s);
hipError_t run_post_edt_sq(const uint8_t *feature, uint32_t *out, int Z, int Y, int X, uint32_t cap, void *work,
                           hipStream_t s);
// postprocess_fg (util/postprocess.py:122-199) in one call (ppp_postprocess.hip); stats[4]: found, small, removed, kept
size_t post_fg_filter_workspace_bytes(long long V);
hipError_t run_post_fg_filter(const uint8_t *mask, uint8_t *fg, uint32_t *inst, int Z, int Y, int X, long long compsize,
                              uint32_t min_d2, long long *stats, void *work, hipStream_t s);

// evaluate_patch as one streaming reduction (ppp_eval.hip): counts [1 + 2T] are ADDED to, maps [T][tz][Y][X] or null
constexpr int kEvalT = 4;        // thresholds served by one pass over the prediction
constexpr int kEvalMaxT = 32;    // thresholds per call
size_t eval_patch_workspace_bytes(long long n_tile_voxels);
hipError_t run_eval_patch(const void *pred, int dtype, const int32_t *labels, int L, int Z, int Y, int X, int pz, int py,
                          int px, int z0, int tz, const float *th, int T, long long *counts, int32_t *inter, int32_t *uni,
                          void *work, hipStream_t s);

// the patch mosaic of visualize_patches (ppp_mosaic.hip): every element of `out` is written; no workspace
constexpr int kMosaicMaxPx = 63;     // four LDS tiles of 128 voxels x (px | 1) 2-byte elements in 64 KiB
bool patch_mosaic_supported(int tz, int Y, int X, int pz, int py, int px, const char **why);
hipError_t run_patch_mosaic(const void *in, int dtype, const uint8_t *sel, int S, void *out, int tz, int Y, int X, int pz,
                            int py, int px, hipStream_t s);

// 3-d thinning of the foreground (ppp_skeleton.hip)
size_t skeleton_workspace_bytes(int Z, int Y, int X);
hipError_t run_skeletonize_3d(const uint8_t *mask, uint8_t *out, int Z, int Y, int X, long long *n_kept, int *stats,
                              void *work, hipStream_t s);
// the same thinning of every instance of an id map in one pass (the kernels instantiated with labels)
size_t skeleton_labels_workspace_bytes(int Z, int Y, int X);
hipError_t run_skeletonize_labels(const uint32_t *labels, uint32_t *out, int Z, int Y, int X, long long *n_kept, int *stats,
                                  void *work, hipStream_t s);

// the contingency table of two label stacks (ppp_overlap.hip); streams = La*Lb + La + Lb
int overlap_table_entries();
void overlap_last_stats(long long *out /* [3] */);
uint32_t overlap_slot_host(uint32_t a, uint32_t b);
size_t label_overlap_workspace_bytes(long long V, long long streams);
hipError_t run_label_overlap(const uint32_t *a, int La, const uint32_t *b, int Lb, long long V, uint32_t *rows,
                             long long *counts, long long cap, long long *n_rows, void *work, hipStream_t s);

// the ground-truth patch affinities of a label volume as an array (ppp_gt_affs.hip): every element of `out` is
// written; no workspace, no synchronisation.  plan out[5]: tile z, y, x; staged in LDS; edge ranges per tile
void gt_affs_dense_plan(int B, int L, int E, const int *halo, const int *box, int32_t out[5]);
hipError_t run_gt_affs_dense(const int32_t *labels, int B, int L, int Z, int Y, int X, const int32_t *nhood, int E,
                             const int *halo, const int *box, void *out, int dtype, int single, hipStream_t s);
hipError_t run_gt_affs_samples(const int32_t *labels, int B, int L, int Z, int Y, int X, const int32_t *samples,
                               long long N, const int32_t *nhood, int E, const int *ps, const int *ctr, void *out,
                               int dtype, hipStream_t s);

// the fused patch loss from the labels (ppp_patch_loss.hip): masked BCE with logits against the predicate of
// gt_affs_dense, forward (loss, state = (s, sum w), optional counts[3]) and backward (every element of `grad`
// is written).  Tiles come from gt_affs_dense_plan.  Workspace: one double per workgroup and sum (box != NULL:
// the dense form; NULL: the sampled form with N rows).  No synchronisation.
size_t patch_loss_workspace_bytes(int B, int L, int E, const int *halo, const int *box, long long N);
hipError_t run_patch_loss_dense(bool fwd, const void *logits, int dtype, const int32_t *labels, int B, int L, int Z, int Y,
                                int X, const int32_t *nhood, int E, const int *halo, const int *box, const float *weight,
                                double num_channels, float *loss, double *state, long long *counts, const float *grad_out,
                                void *grad, void *work, hipStream_t s);
hipError_t run_patch_loss_samples(bool fwd, const void *logits, int dtype, const int32_t *labels, int B, int L, int Z, int Y,
                                  int X, const int32_t *samples, long long N, const int32_t *nhood, int E, const int *ps,
                                  const int *ctr, float *loss, double *state, const float *grad_out, void *grad, void *work,
                                  hipStream_t s);

// one stored chunk, still Blosc-shuffled, to its place in a device tensor (ppp_chunk.hip).  The caller has
// clipped the selection to the chunk: [clo, chi) in chunk coordinates, not empty, and `dst` points at the
// destination element of chunk coordinate clo.  nblocks / waves_per_block are the launcher's.
struct ChunkGeo {
    const uint8_t *src;
    long long nbytes, blocksize;
    int shuffle;                // enum ppp_shuffle
    int cs[4];                  // chunk shape, leading axes of size 1 for fewer than 4
    int clo[4], chi[4];
    long long dstride[3];       // destination element strides of axes 0 .. 2 (axis 3: 1)
    void *dst;
    int fkind;                  // PPP_F16 / PPP_F32: the flags' element type; -1: no flags
    int *flags;
    long long nblocks;
    int waves_per_block;
    int small;                  // the chunk-linear index of every piece fits 31 bits
};
hipError_t launch_chunk_scatter(ChunkGeo g, int typesize, hipStream_t s);

}  // namespace ppp
