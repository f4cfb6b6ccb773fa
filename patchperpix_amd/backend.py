"""ctypes binding of libppp_mi355x.so (include/ppp_mi355x.h).

This module replaces the reference's device shim ``PatchPerPix/vote_instances/cuda_code.py``
(pycuda JIT + managed memory) for this package: device buffers are torch-ROCm tensors
(PyTorch is only the buffer / stream carrier), every computation happens inside the
hand-written HIP kernels of the shared library.  There is NO fallback: if the library is
missing, or no GPU is present, calls raise.
"""
import ctypes
import os

import numpy as np

from . import build as _build

F32, F16, BF16 = 0, 1, 2
BG_INV_TH, BG_HALF_TH, BG_LESS_THAN_TH = 0, 1, 2
VAL_COUNT, VAL_PROB_PRODUCT, VAL_NORM_PROB_PRODUCT = 0, 1, 2
CONS_COMPACT, CONS_REFERENCE, CONS_VOXEL_MAJOR = 0, 1, 2
ABI_VERSION = 5
NONE_KEY = 0xFFFFFFFF
NONE_KEY64 = 1 << 62      # PPP_LABEL_NONE_KEY (streaming labels, int64 keys)
PAIR_KEY_FAR = 0x7FFFFFFFFFFFFFFF   # PPP_PAIR_KEY_FAR


class Box(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("z0", "y0", "x0", "z1", "y1", "x1")]

    def shape(self):
        return (self.z1 - self.z0, self.y1 - self.y0, self.x1 - self.x0)


class Params(ctypes.Structure):
    _fields_ = [("abi_version", ctypes.c_int32),
                ("Z", ctypes.c_int32), ("Y", ctypes.c_int32), ("X", ctypes.c_int32),
                ("pz", ctypes.c_int32), ("py", ctypes.c_int32), ("px", ctypes.c_int32),
                ("th", ctypes.c_double), ("thi", ctypes.c_double),
                ("bg_rule", ctypes.c_int32), ("value_rule", ctypes.c_int32),
                ("use_overlap", ctypes.c_int32), ("normalise", ctypes.c_int32),
                ("norm_rank", ctypes.c_int32), ("count_pos_neg", ctypes.c_int32),
                ("norm_aff", ctypes.c_int32), ("cons_layout", ctypes.c_int32),
                ("cons_box", Box),
                ("origin_z", ctypes.c_int32), ("origin_y", ctypes.c_int32),
                ("origin_x", ctypes.c_int32), ("ring_z", ctypes.c_int32),
                # 1: ppp_pred_check found the buffer passed as `pred` clean (S1's short classification);
                # 2 (this layer only; the library reads "not 1"): checked, not clean; 0: not checked
                ("pred_clean", ctypes.c_int32),
                # tile of centres per workgroup of the ranking kernel: 0 = the library's rule,
                # 1 / 2 / 3 = 8 x 8 x 16 / 8 x 16 x 16 / 16 x 8 x 16 (same scores; tiling.assemble times them)
                ("rank_tile", ctypes.c_int32)]

    @property
    def shape(self):
        return (self.Z, self.Y, self.X)

    @property
    def patchshape(self):
        return (self.pz, self.py, self.px)

    def copy(self):
        q = Params()
        ctypes.memmove(ctypes.byref(q), ctypes.byref(self), ctypes.sizeof(Params))
        return q


_LIB = None
_SIGNATURES = {
    # name: (restype, argtypes)
    "ppp_abi_version": (ctypes.c_int, []),
    "ppp_pred_check": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                      ctypes.POINTER(Params), ctypes.c_void_p]),
    # one read of the prediction for the clean flag, S2's masks and the cover's patch bits (ppp_prepass.hip)
    "ppp_pred_prepass_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(Box), ctypes.POINTER(Params)]),
    "ppp_pred_prepass_layout": (ctypes.c_int, [ctypes.POINTER(Box), ctypes.POINTER(Params),
                                               ctypes.POINTER(ctypes.c_int64)]),
    "ppp_pred_prepass": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_double,
                                        ctypes.c_void_p, ctypes.POINTER(Box), ctypes.c_void_p,
                                        ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_rank_prepared_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(Params)]),
    "ppp_rank_patches_vm_prepared": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Box),
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Params),
                                                    ctypes.c_void_p]),
    "ppp_patch_bits_from_table": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                 ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_last_error": (ctypes.c_char_p, []),
    "ppp_consensus_kernel_name": (ctypes.c_char_p, []),
    "ppp_consensus_short_form": (ctypes.c_int, []),
    "ppp_rank_kernel_name": (ctypes.c_char_p, []),
    "ppp_patch_graph_kernel_name": (ctypes.c_char_p, []),
    "ppp_patch_graph_kernel_geometry": (ctypes.c_char_p, []),
    "ppp_reload_env": (None, []),
    "ppp_np_vote_planes": (ctypes.c_int64, [ctypes.POINTER(Params)]),
    "ppp_np_consensus": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_np_rank_patches": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_np_patch_graph": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_paint_patch_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER(Params),
                                            ctypes.c_void_p]),
    "ppp_counter_calibration": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                               ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "ppp_consensus_writes_voxel_major": (ctypes.c_int, [ctypes.POINTER(Params)]),
    "ppp_device_count": (ctypes.c_int, []),
    "ppp_pred_dtype_supported": (ctypes.c_int, [ctypes.c_int]),
    "ppp_minfilter_xy": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                        ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_cons_planes": (ctypes.c_int64, [ctypes.POINTER(Params)]),
    "ppp_cons_elems": (ctypes.c_int64, [ctypes.POINTER(Params)]),
    "ppp_consensus": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_consensus_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_consensus_part": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.POINTER(Params), ctypes.POINTER(Box),
                                          ctypes.c_void_p]),
    "ppp_consensus_sparse_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(Params), ctypes.POINTER(Box)]),
    "ppp_consensus_sparse": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.POINTER(Params), ctypes.POINTER(Box),
                                            ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "ppp_consensus_last_items": (None, [ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                        ctypes.POINTER(ctypes.c_int)]),
    "ppp_cons_planes_to_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Box), ctypes.c_void_p,
                                               ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_rank_patches": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.POINTER(Box), ctypes.POINTER(Params),
                                        ctypes.c_void_p]),
    "ppp_rank_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(Box), ctypes.POINTER(Params)]),
    "ppp_rank_wg_plan": (ctypes.c_int, [ctypes.POINTER(Box), ctypes.POINTER(Params), ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_int32)]),
    "ppp_rank_wg_plan_residency": (ctypes.c_int, [ctypes.POINTER(Box), ctypes.POINTER(Params), ctypes.c_int,
                                                  ctypes.c_int, ctypes.POINTER(ctypes.c_int32)]),
    "ppp_rank_patches_vm": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Box),
                                           ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_patch_graph": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                       ctypes.c_void_p, ctypes.POINTER(Params),
                                       ctypes.c_void_p]),
    "ppp_patch_graph_by_patch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                                                ctypes.c_void_p, ctypes.POINTER(Params),
                                                ctypes.c_void_p]),
    "ppp_patch_graph_by_patch_chunk_small": (ctypes.c_int32, [ctypes.POINTER(Params)]),
    "ppp_patch_graph_by_patch_chunked": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                        ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                                                        ctypes.c_int32, ctypes.c_void_p,
                                                        ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_patch_graph_lcg_words": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                   ctypes.POINTER(Params)]),
    "ppp_patch_plane_bits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
    "ppp_patch_graph_lcg": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_patch_graph_by_patch_lcg": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                                                    ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_patch_fg_bits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                         ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_patch_graph_by_patch_bits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                                                     ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                     ctypes.c_void_p, ctypes.c_int32,
                                                     ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_label_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(Params)]),
    "ppp_label_components": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                            ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.POINTER(Params),
                                            ctypes.c_void_p]),
    "ppp_label_begin": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                       ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_label_add": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_int64, ctypes.c_uint64, ctypes.c_void_p,
                                     ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_label_union_edges": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.c_void_p, ctypes.POINTER(Params),
                                             ctypes.c_void_p]),
    "ppp_label_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_patch_pairs_count_subset": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                                    ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                    ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_patch_pairs_fill_subset": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                                   ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                                   ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_patch_pairs_count": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                             ctypes.c_void_p, ctypes.POINTER(Params),
                                             ctypes.c_void_p]),
    "ppp_patch_pairs_fill": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                            ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                            ctypes.c_void_p, ctypes.POINTER(Params),
                                            ctypes.c_void_p]),
    "ppp_pair_sort_keys": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                          ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_paint_instances": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                           ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_cons_to_reference": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_cons_to_voxel_major": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_patch_bits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                      ctypes.c_uint64, ctypes.c_double, ctypes.c_void_p,
                                      ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_patch_bits_volume": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_double,
                                             ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_pair_group_keys": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                           ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_patch_graph_by_patch_chunk": (ctypes.c_int32, [ctypes.POINTER(Params)]),
    "ppp_cover_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.POINTER(Params)]),
    "ppp_cover_pass": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Params),
                                      ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]),
    "ppp_cover_pass_voxel_bits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                 ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.POINTER(Params), ctypes.c_void_p,
                                                 ctypes.POINTER(ctypes.c_int32)]),
    "ppp_cover_pass_marked": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.POINTER(Params), ctypes.c_void_p,
                                             ctypes.POINTER(ctypes.c_int32)]),
    "ppp_cover_pass_marked_voxel_bits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                        ctypes.c_void_p, ctypes.POINTER(Params),
                                                        ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]),
    "ppp_cover_mark_bits_bytes": (ctypes.c_int64, [ctypes.POINTER(Params)]),
    "ppp_cover_marks_from_selected": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                     ctypes.c_void_p, ctypes.POINTER(Params),
                                                     ctypes.c_void_p]),
    "ppp_mask_dilate_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(Params)]),
    "ppp_mask_dilate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                       ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_host_mws_sorted": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                             ctypes.c_int64, ctypes.c_void_p]),
    "ppp_host_mws_sorted_stats": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                   ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "ppp_host_mws_sorted_classes": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                     ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "ppp_rank_order_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(Params)]),
    "ppp_rank_order": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64),
                                      ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_mws_edges_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64,
                                                       ctypes.POINTER(Params)]),
    "ppp_mws_edges": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                     ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64),
                                     ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_thin_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.POINTER(Params)]),
    "ppp_thin_cover": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.POINTER(Params), ctypes.c_void_p,
                                      ctypes.POINTER(ctypes.c_int32)]),
    "ppp_cover_open": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_cover_step": (ctypes.c_int, [ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_int32, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_cover_alive": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p,
                                       ctypes.POINTER(ctypes.c_int32)]),
    "ppp_cover_close": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Params),
                                       ctypes.c_void_p]),
    "ppp_cover_zone": (ctypes.c_int, [ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                      ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_thin_shard_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(Params)]),
    "ppp_thin_open": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_thin_step": (ctypes.c_int, [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(Params),
                                     ctypes.c_void_p]),
    "ppp_thin_alive": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p,
                                      ctypes.POINTER(ctypes.c_int32)]),
    "ppp_thin_close": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_thin_zone": (ctypes.c_int, [ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                     ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_synth_pred": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                      ctypes.c_uint32, ctypes.c_float, ctypes.c_float,
                                      ctypes.c_float, ctypes.c_uint64, ctypes.POINTER(Params),
                                      ctypes.c_void_p]),
    "ppp_synth_pred_box": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                          ctypes.c_uint32, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                          ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_decode_tail": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                       ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_float,
                                       ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_int, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_decode_tail_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                            ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_float,
                                            ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_int, ctypes.c_int32, ctypes.c_void_p]),
    "ppp_rows_index_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "ppp_rows_index_build": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                            ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]),
    "ppp_rows_expand": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_void_p,
                                       ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(Box),
                                       ctypes.c_void_p, ctypes.c_void_p]),
    "ppp_rows_compact": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.POINTER(Box),
                                        ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                        ctypes.c_void_p, ctypes.c_void_p]),
    "ppp_host_mws":(ctypes.c_int64, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "ppp_host_rank_order": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p]),
    "ppp_host_cover_pass": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                             ctypes.c_double, ctypes.c_void_p,
                                             ctypes.POINTER(ctypes.c_int64),
                                             ctypes.POINTER(ctypes.c_int32)]),
    "ppp_host_cover_pass_marked": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                                    ctypes.c_double, ctypes.c_void_p,
                                                    ctypes.POINTER(ctypes.c_int64),
                                                    ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p]),
    "ppp_host_thin_cover": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                             ctypes.c_void_p]),
    "ppp_host_skeletonize_3d": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "ppp_host_skel_rule_mismatches": (ctypes.c_int64, [ctypes.c_uint32, ctypes.c_uint32]),
    "ppp_host_patch_pairs": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                              ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                              ctypes.c_void_p]),
    # a stack of independent 2-d images (the *_slices entry points, vote_instances/batch2d.py)
    "ppp_patch_pairs_count_slices": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                                    ctypes.c_void_p, ctypes.POINTER(Params),
                                                    ctypes.c_void_p]),
    "ppp_patch_pairs_fill_slices": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                                   ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                                   ctypes.c_void_p, ctypes.POINTER(Params),
                                                   ctypes.c_void_p]),
    "ppp_patch_graph_slices": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                              ctypes.c_void_p, ctypes.POINTER(Params),
                                              ctypes.c_void_p]),
    "ppp_patch_graph_lcg_slices": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                  ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_patch_graph_by_patch_lcg_slices": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                           ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                                                           ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                                           ctypes.c_void_p, ctypes.POINTER(Params),
                                                           ctypes.c_void_p]),
    "ppp_thin_cover_slices": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p,
                                             ctypes.POINTER(ctypes.c_int32)]),
    "ppp_label_slice_renumber": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(Params),
                                                ctypes.c_void_p]),
    # whole-volume post-steps of the label driver (postprocess.py)
    "ppp_post_compact_ids_workspace_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_uint32]),
    "ppp_post_compact_ids": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_int64,
                                            ctypes.c_int32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int64),
                                            ctypes.c_void_p, ctypes.c_void_p]),
    "ppp_post_dilate_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "ppp_post_dilate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                       ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p,
                                       ctypes.c_void_p]),
    "ppp_post_clean_mask_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "ppp_post_clean_mask": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                           ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64,
                                           ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                           ctypes.c_void_p, ctypes.c_void_p]),
    # postprocess_fg: exact squared distance transform and the component filter (ppp_edt.hip, ppp_postprocess.hip)
    "ppp_post_edt_sq_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "ppp_post_edt_sq": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                       ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]),
    "ppp_post_fg_filter_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "ppp_post_fg_filter": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                          ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32,
                                          ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p, ctypes.c_void_p]),
    # evaluate_patch as one streaming reduction (ppp_eval.hip)
    "ppp_eval_patch_thresholds_per_pass": (ctypes.c_int32, []),
    "ppp_eval_patch_max_thresholds": (ctypes.c_int32, []),
    "ppp_eval_patch_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]),
    "ppp_eval_patch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                      ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32,
                                      ctypes.c_int32, ctypes.POINTER(ctypes.c_float), ctypes.c_int32, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    # 3-d thinning of the foreground on the device (ppp_skeleton.hip)
    "ppp_skeletonize_3d_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "ppp_skeletonize_3d": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                          ctypes.c_int32, ctypes.POINTER(ctypes.c_int64),
                                          ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p, ctypes.c_void_p]),
    "ppp_skeletonize_labels_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "ppp_skeletonize_labels": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                              ctypes.c_int32, ctypes.POINTER(ctypes.c_int64),
                                              ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p, ctypes.c_void_p]),
    # the contingency table of two label stacks (ppp_overlap.hip)
    "ppp_label_overlap_table_entries": (ctypes.c_int32, []),
    "ppp_label_overlap_slot": (ctypes.c_uint32, [ctypes.c_uint32, ctypes.c_uint32]),
    "ppp_label_overlap_last_stats": (None, [ctypes.POINTER(ctypes.c_int64)]),
    "ppp_label_overlap_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                           ctypes.c_int32, ctypes.c_int32]),
    "ppp_label_overlap": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                         ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
                                         ctypes.c_void_p, ctypes.c_void_p]),
    # the patch mosaic of visualize_patches (ppp_mosaic.hip)
    "ppp_patch_mosaic": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                        ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                        ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p]),
    # the ground-truth patch affinities as an array (ppp_gt_affs.hip)
    "ppp_gt_affs_dense_plan": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                              ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                              ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.c_int32,
                                              ctypes.POINTER(ctypes.c_int32)]),
    "ppp_gt_affs_dense": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                         ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                         ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p, ctypes.c_int, ctypes.c_int32,
                                         ctypes.c_void_p]),
    "ppp_gt_affs_samples": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                           ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32,
                                           ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p,
                                           ctypes.c_int, ctypes.c_void_p]),
    # the fused patch loss from the labels (ppp_patch_loss.hip)
    "ppp_patch_loss_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                                        ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                                        ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.c_int64]),
    "ppp_patch_loss_dense_fwd": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                                ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p, ctypes.c_int32,
                                                ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                                ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "ppp_patch_loss_dense_bwd": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                                ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p, ctypes.c_int32,
                                                ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p]),
    "ppp_patch_loss_samples_fwd": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                                  ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p, ctypes.c_int64,
                                                  ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                                  ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p]),
    "ppp_patch_loss_samples_bwd": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                                  ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p, ctypes.c_int64,
                                                  ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                                  ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p]),
    # no_overlap_per_channel without the loop over components (ppp_pack_channels.hip, ppp_host_pack.cpp)
    "ppp_pack_scan_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(Params), ctypes.POINTER(Box)]),
    "ppp_pack_scan_count": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(Box), ctypes.c_void_p,
                                           ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p, ctypes.POINTER(Params),
                                           ctypes.c_void_p]),
    "ppp_pack_scan_fill": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Box), ctypes.c_void_p,
                                          ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_paint_instances_channels": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                                    ctypes.c_void_p, ctypes.POINTER(Params), ctypes.c_void_p]),
    "ppp_host_pack_channels": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]),
    # a stored zarr chunk, still Blosc-shuffled, to its place in a device tensor (ppp_chunk.hip)
    "ppp_chunk_scatter": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                         ctypes.c_int32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                         ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p,
                                         ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
}
ERR_UNSUPPORTED = -4      # PPP_ERR_UNSUPPORTED
SHUFFLE_NONE, SHUFFLE_BYTE, SHUFFLE_BIT = 0, 1, 2


def library_path():
    return _build.LIB


def lib():
    """Load libppp_mi355x.so; raise (never fall back) if it has not been built."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise RuntimeError(
                "HIP library %s is missing -- build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` "
                "(patchperpix_amd has no CPU fallback)" % path)
        # torch first: it brings its own libamdhip64, and a second HIP runtime loaded BEFORE it
        # (through this library) leaves the process without a visible device
        _torch()
        L = ctypes.CDLL(path)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the ABI is incomplete
            fn.restype = res
            fn.argtypes = args
        if L.ppp_abi_version() != ABI_VERSION:
            raise RuntimeError("libppp_mi355x.so ABI %d != %d" % (L.ppp_abi_version(), ABI_VERSION))
        _LIB = L
    return _LIB


def check(rc):
    if rc != 0:
        raise RuntimeError("libppp_mi355x: %s (code %d)" % (lib().ppp_last_error().decode(), rc))


def device_count():
    return lib().ppp_device_count()


# ----------------------------------------------------------------------------------------
# parameters from the reference's kwargs (utilVoteInstances.py:340-449)
# ----------------------------------------------------------------------------------------
def make_params(shape_zyx, patchshape, cons_box=None, cons_layout=CONS_COMPACT,
                origin=(0, 0, 0), **kw):
    """Translate the reference's keyword flags into ppp_params.

    Mirrors loadKernelFromFile's TH/THI substitution and setKernelBuildOptions' -D flags,
    including its defaults (vi_bg_use_inv_th defaults to True when absent) and its error
    for an undefined background rule."""
    th = float(kw["patch_threshold"])
    P = Params()
    P.abi_version = ABI_VERSION
    P.Z, P.Y, P.X = [int(s) for s in shape_zyx]
    P.pz, P.py, P.px = [int(p) for p in patchshape]
    P.th = th
    P.thi = th if th < 0.5 else 1.0 - th
    if kw.get("vi_bg_use_inv_th", True):
        P.bg_rule = BG_LESS_THAN_TH if th < 0.5 else BG_INV_TH
    elif kw.get("vi_bg_use_half_th", False):
        P.bg_rule = BG_HALF_TH
    elif kw.get("vi_bg_use_less_than_th", False):
        P.bg_rule = BG_LESS_THAN_TH
    else:
        raise RuntimeError("how is bg defined for vote instances?")
    P.use_overlap = 1 if kw.get("overlapping_inst", False) else 0
    if kw.get("consensus_norm_prob_product", True):
        P.value_rule = VAL_NORM_PROB_PRODUCT
    elif kw.get("consensus_prob_product", True):
        P.value_rule = VAL_PROB_PRODUCT
    else:
        assert \
            not kw.get("consensus_norm_aff", True) and \
            not kw.get("consensus_interleaved_cnt", True), \
            "no normalizing for accumulate consensus counter available"
        P.value_rule = VAL_COUNT
    P.normalise = 1 if kw.get("consensus_norm_aff", True) else 0
    P.norm_rank = 1 if kw.get("rank_norm_patch_score", True) else 0
    P.count_pos_neg = 1 if kw.get("rank_int_counter", False) else 0
    P.norm_aff = 1 if kw.get("patch_graph_norm_aff", True) else 0
    P.cons_layout = cons_layout
    if cons_box is None:
        cons_box = (0, 0, 0, P.Z, P.Y, P.X)
    P.cons_box = Box(*[int(v) for v in cons_box])
    P.origin_z, P.origin_y, P.origin_x = [int(v) for v in origin]
    return P


def params_from_kwargs(shape_zyx, patchshape, kwargs):
    """make_params for a reference-style kwargs dict (which may carry this package's own
    ``cons_box`` / ``cons_layout`` entries next to the reference's flags)."""
    kw = {k: v for k, v in kwargs.items() if k not in ("cons_box", "cons_layout", "origin")}
    return make_params(shape_zyx, patchshape, cons_box=kwargs.get("cons_box"),
                       cons_layout=kwargs.get("cons_layout", CONS_COMPACT),
                       origin=kwargs.get("origin", (0, 0, 0)), **kw)


# ----------------------------------------------------------------------------------------
# torch plumbing
# ----------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _dev_ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device tensors must be contiguous and on the GPU"
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(_torch().cuda.current_stream().cuda_stream)


def _workspace(nbytes, device):
    """The d_work buffer of an entry point, `nbytes` being the answer of its ppp_*_workspace_bytes
    query: a negative answer is the query's error (ppp_last_error says which)."""
    check(min(int(nbytes), 0))
    return _torch().empty(int(nbytes), dtype=_torch().uint8, device=device)


# Optional per-kernel timing with HIP events on the stream the kernels are launched on
# (bench.py switches it on): EVENTS = {} collects name -> [(start, stop), ...].
EVENTS = None


class _timed:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if EVENTS is not None:
            torch = _torch()
            self.a = torch.cuda.Event(enable_timing=True)
            self.b = torch.cuda.Event(enable_timing=True)
            self.a.record(torch.cuda.current_stream())

    def __exit__(self, *exc):
        if EVENTS is not None:
            self.b.record(_torch().cuda.current_stream())
            EVENTS.setdefault(self.name, []).append((self.a, self.b))


HOST_TIMES = None   # name -> [seconds, ...] wall time of host stages (bench.py switches on)


class host_timer:
    """Wall-clock timer for a host stage (synchronises the device first when enabled, so a
    stage is not charged for kernels still running from the previous one)."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if HOST_TIMES is not None:
            import time
            _torch().cuda.synchronize()
            self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        if HOST_TIMES is not None:
            import time
            _torch().cuda.synchronize()
            HOST_TIMES.setdefault(self.name, []).append(time.perf_counter() - self.t0)


NOTES = {}
LAST_PLAN = None    # the memory plan of the last to_instance_seg call that made one (vote_instances.py)
PRED_UPLOADS = 0    # to_device_pred calls whose input was NOT on the device: host -> device copies of a prediction


def note(key, value):
    """Record a workload statistic (number of selected patches, pairs, ...) or a name."""
    NOTES[key] = value if isinstance(value, str) else int(value)


def note_add(key, value):
    NOTES[key] = NOTES.get(key, 0) + int(value)


def event_times_ms():
    """name -> list of elapsed ms (call after a synchronize)."""
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in (EVENTS or {}).items()}


def pred_dtype_code(t):
    torch = _torch()
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float16:
        return F16
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError("pred must be float32, float16 or bfloat16, got %s" % t.dtype)


def counter_calibration(src, n_read, dst, n_write):
    """ppp_counter_calibration: read n_read elements of `src` (float16 / float32 device tensor),
    write n_write floats to `dst` (float32 device tensor).  Returns the true (read, write) bytes."""
    check(lib().ppp_counter_calibration(_dev_ptr(src), pred_dtype_code(src), int(n_read), _dev_ptr(dst),
                                        int(n_write), _stream()))
    return int(n_read) * src.element_size(), int(n_write) * 4


_HOST_ALLOCATOR = None


def tune_host_allocator(cli=False):
    """Host allocator of a long-running service: the pipeline's host arrays (masks, instance map:
    a few MB each at 140^3, several dozen per call) would otherwise be mmap'ed, first-touched and
    unmapped again on every call by glibc (~5 ms per step of page faults at 140^3).  Same effect
    as MALLOC_TRIM_THRESHOLD_ / MALLOC_MMAP_THRESHOLD_ in the environment.

    The thresholds are process-wide and keep freed host memory from going back to the OS, so they
    are set only for a process that IS one of the drivers (`cli=True`: run_ppp / vote_instances /
    stitch_patch_graph run as a program, bench.py) -- unless PPP_MALLOPT=0 (or the older
    PPP_BENCH_MALLOPT=0) -- or, for an application that calls main() as a library function, when
    it opts in with PPP_MALLOPT=1.  Returns what was done (each mallopt call reported on its own:
    many glibc builds refuse an M_MMAP_THRESHOLD above 32 MiB)."""
    global _HOST_ALLOCATOR
    if _HOST_ALLOCATOR is not None:
        return _HOST_ALLOCATOR
    want = os.environ.get("PPP_MALLOPT", os.environ.get("PPP_BENCH_MALLOPT"))
    if want == "0" or (not cli and want != "1"):
        if cli or want == "0":
            _HOST_ALLOCATOR = "off"
        return _HOST_ALLOCATOR or "untouched (library call; PPP_MALLOPT=1 opts in)"
    try:
        libc = ctypes.CDLL("libc.so.6")
        trim = bool(libc.mallopt(-1, 1 << 30))             # M_TRIM_THRESHOLD
        mmap = bool(libc.mallopt(-3, 1 << 30))             # M_MMAP_THRESHOLD
        if not mmap:
            mmap32 = bool(libc.mallopt(-3, 32 << 20))      # the largest value older glibc accepts
        _HOST_ALLOCATOR = "trim threshold 1 GiB: %s; mmap threshold 1 GiB: %s%s" % (
            "set" if trim else "refused", "set" if mmap else "refused",
            "" if mmap else (", 32 MiB: %s" % ("set" if mmap32 else "refused")))
    except OSError:
        _HOST_ALLOCATOR = "no libc"
    return _HOST_ALLOCATOR


def reload_env():
    """The library reads its PPP_* development switches once; after changing one in a running
    process (tests that compare kernel variants) this makes it look again."""
    lib().ppp_reload_env()


def to_device_pred(pred, device="cuda", keep_f16=True):
    """Host ndarray / tensor -> contiguous device tensor (f16 and bf16 stay as they are: widening
    is exact and happens in registers; a contiguous tensor already on `device` is returned itself).
    NOTES["pred_dtype"] names the element type the kernels are given."""
    global PRED_UPLOADS
    torch = _torch()
    if isinstance(pred, np.ndarray):
        if pred.dtype not in (np.float32, np.float16):
            pred = pred.astype(np.float32)
        pred = torch.from_numpy(np.ascontiguousarray(pred))
    if not pred.is_cuda:
        PRED_UPLOADS += 1
    if pred.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        pred = pred.float()
    if pred.dtype == torch.float16 and not keep_f16:
        pred = pred.float()
    pred = pred.to(device).contiguous()
    note("pred_dtype", str(pred.dtype).replace("torch.", ""))
    return pred


def chunk_scatter_rc(src, typesize, blocksize, shuffle, chunk_shape, origin, ranges, out, flags=None):
    """ppp_chunk_scatter, its return code as it is.  src: uint8 device tensor, the decompressed, still
    shuffled bytes of one chunk; shuffle: None / "byte" / "bit"; chunk_shape, origin, ranges ((start, stop)
    per axis): the chunk, the array coordinate of its first element and the selection; out: the contiguous
    device tensor of the selection's un-squeezed shape; flags: int32[3] device tensor {any < 0, any > 1,
    any NaN} the call only ever sets (float16 / float32 `out`), or None."""
    torch = _torch()
    n = len(chunk_shape)
    if not (len(origin) == len(ranges) == n == out.dim()) or tuple(out.shape) != tuple(b - a for a, b in ranges):
        raise ValueError("chunk_scatter: `out` must have the selection's un-squeezed shape")
    if out.element_size() != int(typesize) and int(typesize) in (1, 2, 4):
        raise ValueError("chunk_scatter: elements of %d bytes into a %s tensor" % (typesize, out.dtype))
    if src.dtype != torch.uint8:
        raise TypeError("chunk_scatter: `src` holds bytes (uint8)")
    fdt = -1
    if flags is not None:
        if out.dtype not in (torch.float16, torch.float32) or flags.dtype != torch.int32 or flags.numel() != 3:
            raise TypeError("chunk_scatter: flags are int32[3], for a float16 / float32 destination")
        fdt = pred_dtype_code(out)
    i64 = lambda seq: (ctypes.c_int64 * n)(*[int(v) for v in seq])
    return lib().ppp_chunk_scatter(_dev_ptr(src), int(src.numel()), int(typesize), int(blocksize),
                                   {None: SHUFFLE_NONE, "byte": SHUFFLE_BYTE, "bit": SHUFFLE_BIT}[shuffle], n,
                                   i64(chunk_shape), i64(origin), i64([a for a, _ in ranges]), i64([b for _, b in ranges]),
                                   _dev_ptr(out), fdt, _dev_ptr(flags), _stream())


def chunk_scatter(src, typesize, blocksize, shuffle, chunk_shape, origin, ranges, out, flags=None):
    """`chunk_scatter_rc`; False when the library does not serve the chunk's form (PPP_ERR_UNSUPPORTED: the
    caller un-shuffles on the host), True when the kernel was launched; every other code raises."""
    rc = chunk_scatter_rc(src, typesize, blocksize, shuffle, chunk_shape, origin, ranges, out, flags)
    if rc == ERR_UNSUPPORTED:
        return False
    check(rc)
    return True


# ----------------------------------------------------------------------------------------
# device stages
# ----------------------------------------------------------------------------------------
_CHECK_FLAG = {}


def pred_check(pred, P):
    """ppp_pred_check over the whole (contiguous) prediction tensor: 1 when every value lies in [0, 1]
    and none sits between the two class tests of P (with the shipped rule: none equals the threshold),
    2 otherwise -- the value of ppp_params.pred_clean for calls on THIS tensor while it is unchanged.
    One streaming read (196 GB at 512^3 / 9^3: 50 ms per volume) and one device -> host copy of the
    flag.  PPP_S1_CLEAN=0: never asked (returns 2)."""
    torch = _torch()
    if os.environ.get("PPP_S1_CLEAN", "1") == "0" or not torch.is_tensor(pred) or not pred.is_cuda \
            or not pred.is_contiguous():
        return 2
    key = str(pred.device)
    if key not in _CHECK_FLAG:
        _CHECK_FLAG[key] = torch.zeros((1,), dtype=torch.int32, device=pred.device)
    flag = _CHECK_FLAG[key]
    with _timed("pred_check"):
        check(lib().ppp_pred_check(_dev_ptr(pred), pred_dtype_code(pred), int(pred.numel()), _dev_ptr(flag),
                                   ctypes.byref(P), _stream()))
    bad = int(flag.item())
    note("pred_unclean_bits", bad)
    return 1 if bad == 0 else 2


class PredPrepass:
    """What ppp_pred_prepass made of ONE prediction tensor in its single read (valid while the tensor, the
    thresholds and the overlap mask stay what they were): `work` is the library's workspace (S2's masks, pair
    counts and `valid` for `score_box`, handed to rank_patches as `prepared`), `bits_vol` the int32 (V, words)
    view of the per-voxel patch bits for `fc_threshold` inside it, `clean` the value of ppp_params.pred_clean."""
    __slots__ = ("work", "score_box", "bits_vol", "offsets", "clean", "unclean_bits", "fc_threshold")


def pred_prepass(pred, overlap, fc_threshold, P, score, score_box=None):
    """ppp_pred_prepass: the clean flag, S2's pre-pass for `score_box` (its border / background scores go into
    `score`, float32 (Z, Y, X)) and the cover's per-voxel patch bits from one read of `pred`.  Returns a
    PredPrepass, or None where the library does not serve the geometry or PPP_PRED_PREPASS=0 asks for the
    separate launches -- the caller then keeps pred_check / rank_patches / patch_bits as they are."""
    torch = _torch()
    if os.environ.get("PPP_PRED_PREPASS", "1") == "0" or not torch.is_tensor(pred) or not pred.is_cuda \
            or not pred.is_contiguous():
        return None
    sb = (0, 0, 0) + tuple(int(v) for v in P.shape) if score_box is None else tuple(int(v) for v in score_box)
    box = ctypes.byref(Box(*sb))
    nbytes = int(lib().ppp_pred_prepass_workspace_bytes(box, ctypes.byref(P)))
    if nbytes == 0:
        return None
    pre = PredPrepass()
    pre.work = _workspace(nbytes, pred.device)
    off = (ctypes.c_int64 * 5)()
    check(lib().ppp_pred_prepass_layout(box, ctypes.byref(P), off))
    with _timed("pred_prepass"):
        check(lib().ppp_pred_prepass(_dev_ptr(pred), pred_dtype_code(pred), _dev_ptr(overlap), float(fc_threshold),
                                     _dev_ptr(score), box, _dev_ptr(pre.work), ctypes.byref(P), _stream()))
    V = int(P.Z) * int(P.Y) * int(P.X)
    words = (P.pz * P.py * P.px + 31) // 32
    pre.score_box, pre.offsets, pre.fc_threshold = sb, tuple(int(o) for o in off), float(fc_threshold)
    pre.bits_vol = pre.work[off[3]:off[3] + V * words * 4].view(torch.int32).view(V, words)
    pre.unclean_bits = int(pre.work[off[4]:off[4] + 4].view(torch.int32).item())
    note("pred_unclean_bits", pre.unclean_bits)
    # (PPP_S1_CLEAN=0: S1 is never told, as pred_check never asks)
    pre.clean = 2 if os.environ.get("PPP_S1_CLEAN", "1") == "0" or pre.unclean_bits else 1
    return pre


def patch_bits_from_table(bits_vol, centres, P):
    """ppp_patch_bits_from_table: the rows of `centres` (int32 [n, 3] on the device) out of a per-voxel
    table (PredPrepass.bits_vol): patch_bits without another look at the prediction."""
    torch = _torch()
    n = int(centres.shape[0])
    bits = torch.empty((n, int(bits_vol.shape[1])), dtype=torch.int32, device=bits_vol.device)
    with _timed("patch_bits"):
        check(lib().ppp_patch_bits_from_table(_dev_ptr(bits_vol), _dev_ptr(centres.contiguous()), n, _dev_ptr(bits),
                                              ctypes.byref(P), _stream()))
    return bits


def with_pred_clean(pred, P):
    """P with pred_clean decided (a copy when it was not): callers that pass the same tensor to many
    S1 launches (tiling.assemble: once per frame) decide once; a direct call decides per call."""
    if P.pred_clean != 0:
        return P
    Q = P.copy()
    Q.pred_clean = pred_check(pred, P)
    return Q


# S1 on sparse foreground (ppp_consensus_sparse): PPP_S1_SPARSE = 0 (the dense launch), 1 (always the
# item lists) or auto (the lists below the measured break-even share of active items).  A caller's
# `_s1_sparse` kwarg (tiling.assemble, vote_instances.to_instance_seg) overrides the environment
# for the duration of its call.
S1_SPARSE_DEFAULT = "0"
_S1_SPARSE = None
_S1_WORK = {}


class s1_sparse_scope:
    """`with s1_sparse_scope(v)`: v None = the environment decides, "auto", True / False"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        global _S1_SPARSE
        self.old = _S1_SPARSE
        if self.value is not None:
            _S1_SPARSE = self.value

    def __exit__(self, *exc):
        global _S1_SPARSE
        _S1_SPARSE = self.old


def s1_sparse_mode():
    """None (dense entry points), 0 (auto) or 1 (lists): the `mode` of ppp_consensus_sparse"""
    v = _S1_SPARSE if _S1_SPARSE is not None else os.environ.get("PPP_S1_SPARSE", S1_SPARSE_DEFAULT)
    if v is True or v == 1 or v == "1":
        return 1
    if v == "auto":
        return 0
    if v is False or v == 0 or v == "0":
        return None
    raise ValueError("PPP_S1_SPARSE / _s1_sparse must be 0, 1 or auto, got %r" % (v,))


def consensus_last_items():
    """(items, active items, took_lists) of the last ppp_consensus_sparse call"""
    t, a, k = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0)
    lib().ppp_consensus_last_items(ctypes.byref(t), ctypes.byref(a), ctypes.byref(k))
    return int(t.value), int(a.value), int(k.value)


def _consensus_sparse(pred, overlap, cons, cnt, P, part, open_rows):
    """The sparse entry when the mode asks for it and the packed kernel serves P; False when the
    caller is to make its dense call."""
    mode = s1_sparse_mode()
    if mode is None:
        return False
    L = lib()
    pb = ctypes.byref(part) if part is not None else None
    need = int(L.ppp_consensus_sparse_workspace_bytes(ctypes.byref(P), pb))
    if need <= 0:
        return False        # (v2 / gather / 25-wide kernels, reference layout: the dense path)
    key = str(pred.device)
    work = _S1_WORK.get(key)
    if work is None or work.numel() < need:
        work = _S1_WORK[key] = _workspace(need, pred.device)
    check(L.ppp_consensus_sparse(_dev_ptr(pred), pred_dtype_code(pred), _dev_ptr(overlap), _dev_ptr(cons),
                                 _dev_ptr(cnt), ctypes.byref(P), pb, 1 if open_rows else 0, _dev_ptr(work),
                                 mode, _stream()))
    total, active, took = consensus_last_items()
    note_add("s1_items", total)
    note_add("s1_active_items", active)
    note_add("s1_list_launches", took)
    return True


def s1_items_host(valid, patchshape, part=None):
    """NumPy restatement of the item criterion of ppp_consensus_sparse (csrc/ppp_consensus_sparse.hip).

    valid  bool (Z, Y, X): pred[mid] > TH and not overlapped;  part: the compute box (z0, y0, x0, z1,
    y1, x1), None = the whole volume.  An item is (run, offset row): a run is 64 base voxels of the
    compute box (one line, or two lines flattened over y * x when the box's x extent is >= 64 and no
    multiple of 64) times two slices; the rows are (0, dy >= 0), then (dz >= 1, every dy).
    Returns (active bool [n_runs, n_rows], runs, rows): runs[i] = list of (z, y, x0, n) line segments
    of base voxels, rows[r] = (dz, dy).  Active = some valid base voxel u of the run has a valid
    partner u + (dz, dy, dx) inside the volume, |dx| <= px - 1 (dx > 0 only in row (0, 0))."""
    valid = np.asarray(valid, dtype=bool)
    Z, Y, X = valid.shape
    pz, py, px = [int(p) for p in patchshape]
    cz0, cy0, cx0, cz1, cy1, cx1 = [int(v) for v in (part if part is not None else (0, 0, 0, Z, Y, X))]
    cZ, cY, cX = cz1 - cz0, cy1 - cy0, cx1 - cx0
    flat = cX >= 64 and cX % 64 != 0 and py >= 3 and cY > 1
    rows = [(0, dy) for dy in range(py)] + \
        [(dz, dy) for dz in range(1, pz) for dy in range(-(py - 1), py)]
    # partners along x: any valid voxel at x + dx, dx in [-(px-1), px-1] / in [1, px-1]
    pad = np.zeros((Z, Y, X + 2 * (px - 1)), dtype=bool)
    pad[:, :, px - 1:px - 1 + X] = valid
    dil_all = np.zeros_like(valid)
    dil_pos = np.zeros_like(valid)
    for dx in range(-(px - 1), px):
        sh = pad[:, :, px - 1 + dx:px - 1 + dx + X]
        dil_all |= sh
        if dx > 0:
            dil_pos |= sh
    rpl = (cX * cY + 63) // 64 if flat else (cX + 63) // 64
    n_runs = rpl * (1 if flat else cY) * ((cZ + 1) // 2)
    runs = []
    active = np.zeros((n_runs, len(rows)), dtype=bool)
    for run in range(n_runs):
        xr, r2 = run % rpl, run // rpl
        if flat:
            f0 = xr * 64
            uy, uz, ux0 = cy0 + f0 // cX, cz0 + 2 * r2, cx0 + f0 % cX
            nA = min(64, cX - f0 % cX)
            segs = [(uy, ux0, nA)]
            if nA < 64 and uy + 1 < cy1:
                segs.append((uy + 1, cx0, 64 - nA))
        else:
            uy, uz, ux0 = cy0 + r2 % cY, cz0 + 2 * (r2 // cY), cx0 + xr * 64
            segs = [(uy, ux0, min(64, cx1 - ux0))]
        lines = [(uz + s, y, x0, n) for s in (0, 1) if uz + s < cz1 for (y, x0, n) in segs]
        runs.append(lines)
        for (z, y, x0, n) in lines:
            U = valid[z, y, x0:x0 + n]
            if not U.any():
                continue
            for r, (dz, dy) in enumerate(rows):
                zw, yw = z + dz, y + dy
                if active[run, r] or zw >= Z or yw < 0 or yw >= Y:
                    continue
                D = (dil_pos if r == 0 else dil_all)[zw, yw, x0:x0 + n]
                active[run, r] = bool((U & D).any())
    return active, runs, rows


def consensus(pred, overlap, P, want_count=False, out=None, open_rows=False):
    """S1.  Returns cons (and count) as device float32 tensors shaped
    [planes, bz, by, bx] (compact), [bz, by, bx, W] (voxel-major) or [NSZ, NSY, NSX, Z, Y, X]
    (reference layout).  out: a flat float32 device tensor to carve the result from (the tiled
    path keeps ONE buffer for all its tiles: tens of GB allocated and freed per tile fragment the
    caching allocator until a tile that fits on paper no longer does)."""
    torch = _torch()
    L = lib()
    P = with_pred_clean(pred, P)
    if P.cons_layout == CONS_REFERENCE:
        shape = (2 * P.pz if P.pz > 1 else 1, 2 * P.py, 2 * P.px, P.Z, P.Y, P.X)
    elif P.cons_layout == CONS_VOXEL_MAJOR:
        shape = P.cons_box.shape() + (int(L.ppp_cons_planes(ctypes.byref(P))),)
    else:
        shape = (int(L.ppp_cons_planes(ctypes.byref(P))),) + P.cons_box.shape()
    n_el = int(np.prod(shape))
    if out is not None and out.numel() >= n_el:
        cons = out[:n_el].view(shape)
    else:
        cons = _big_empty(shape, pred.device)
    cnt = torch.empty(shape, dtype=torch.float32, device=pred.device) if want_count else None
    note_add("s1_base_voxels", int(np.prod(P.cons_box.shape())))
    note_add("s1_output_bytes", 4 * n_el)
    with _timed("consensus"):
        if _consensus_sparse(pred, overlap, cons, cnt, P, None,
                             open_rows and P.cons_layout == CONS_VOXEL_MAJOR and cnt is None):
            pass
        elif open_rows and P.cons_layout == CONS_VOXEL_MAJOR and cnt is None:
            # rows for the library's own consumers: no zeroing of entries they never read
            check(L.ppp_consensus_rows(_dev_ptr(pred), pred_dtype_code(pred), _dev_ptr(overlap),
                                       _dev_ptr(cons), ctypes.byref(P), _stream()))
        else:
            check(L.ppp_consensus(_dev_ptr(pred), pred_dtype_code(pred), _dev_ptr(overlap),
                                  _dev_ptr(cons), _dev_ptr(cnt), ctypes.byref(P), _stream()))
    note("s1_kernel", L.ppp_consensus_kernel_name().decode())
    note("s1_short_form", int(L.ppp_consensus_short_form()))
    return (cons, cnt) if want_count else cons


def _big_empty(shape, device):
    """float32 device buffer of tens of GB.  A block of the right size is normally waiting in
    torch's cache from the previous slab / step (a fresh hipMalloc costs ~25 ms per GB); only
    when the allocator really runs dry are the cached blocks handed back first."""
    torch = _torch()
    try:
        return torch.empty(shape, dtype=torch.float32, device=device)
    except torch.OutOfMemoryError:
        torch.cuda.empty_cache()
        return torch.empty(shape, dtype=torch.float32, device=device)


def rank_patches(pred, cons, overlap, P, score_box=None, out=None, prepared=None):
    """S2.  Returns the (Z, Y, X) float32 score volume on the device.  With a VOXEL_MAJOR
    consensus (P.cons_layout) the row-stationary kernel runs (ppp_rank_patches_vm).  prepared: the
    PredPrepass of this tensor and score box, whose pass wrote the border and background scores into
    `out` -- the kernel then starts from its masks (ppp_rank_patches_vm_prepared)."""
    torch = _torch()
    if prepared is not None:
        sb = (0, 0, 0) + tuple(int(v) for v in P.shape) if score_box is None else tuple(int(v) for v in score_box)
        assert out is not None and P.cons_layout == CONS_VOXEL_MAJOR and prepared.score_box == sb, \
            "a prepared ranking call takes the score volume and the box of its pre-pass"
        work = _workspace(lib().ppp_rank_prepared_workspace_bytes(ctypes.byref(P)), pred.device)
        cb = P.cons_box
        rad = (P.pz // 2, P.py // 2, P.px // 2)
        lo3 = [max(sb[a] - rad[a], (cb.z0, cb.y0, cb.x0)[a]) for a in range(3)]
        hi3 = [min(sb[3 + a] + rad[a], (cb.z1, cb.y1, cb.x1)[a]) for a in range(3)]
        note_add("s2_base_voxels", int(np.prod([max(0, h - l) for l, h in zip(lo3, hi3)])))
        with _timed("rank_patches"):
            check(lib().ppp_rank_patches_vm_prepared(_dev_ptr(cons), _dev_ptr(out), ctypes.byref(Box(*sb)),
                                                     _dev_ptr(prepared.work), _dev_ptr(work), ctypes.byref(P),
                                                     _stream()))
        return out
    if out is None:
        out = torch.zeros(P.shape, dtype=torch.float32, device=pred.device)
    box = None if score_box is None else ctypes.byref(Box(*[int(v) for v in score_box]))
    if P.cons_layout == CONS_VOXEL_MAJOR:
        nbytes = int(lib().ppp_rank_workspace_bytes(box, ctypes.byref(P)))
        if nbytes == 0:
            raise RuntimeError("libppp_mi355x: no voxel-major ranking kernel for this configuration")
        work = _workspace(nbytes, pred.device)
        # voxels whose consensus row the launch reads: the score box grown by the patch radius
        sb = (0, 0, 0) + tuple(P.shape) if score_box is None else tuple(int(v) for v in score_box)
        cb = P.cons_box
        rad = (P.pz // 2, P.py // 2, P.px // 2)
        lo3 = [max(sb[a] - rad[a], (cb.z0, cb.y0, cb.x0)[a]) for a in range(3)]
        hi3 = [min(sb[3 + a] + rad[a], (cb.z1, cb.y1, cb.x1)[a]) for a in range(3)]
        note_add("s2_base_voxels", int(np.prod([max(0, h - l) for l, h in zip(lo3, hi3)])))
        with _timed("rank_patches"):
            check(lib().ppp_rank_patches_vm(_dev_ptr(pred), pred_dtype_code(pred), _dev_ptr(cons),
                                            _dev_ptr(overlap), _dev_ptr(out), box, _dev_ptr(work),
                                            ctypes.byref(P), _stream()))
        return out
    with _timed("rank_patches"):
        check(lib().ppp_rank_patches(_dev_ptr(pred), pred_dtype_code(pred), _dev_ptr(cons),
                                     _dev_ptr(overlap), _dev_ptr(out), box, ctypes.byref(P),
                                     _stream()))
    return out


def rank_wg_plan(P, score_box=None, resident_per_cu=0, cus_per_xcd=0):
    """How ppp_rank_patches_vm would launch the workgroup-per-tile ranking kernel for this box, without
    launching (ppp_rank_wg_plan): tile, z step, tiles, splits and order slots per XCD, range kind.  With
    resident_per_cu and cus_per_xcd given no device is asked."""
    box = None if score_box is None else ctypes.byref(Box(*[int(v) for v in score_box]))
    out = (ctypes.c_int32 * 8)()
    check(lib().ppp_rank_wg_plan(box, ctypes.byref(P), int(resident_per_cu), int(cus_per_xcd), out))
    return dict(tile=(out[0], out[1], out[2]), tz_step=out[3], tiles=out[4], splits=out[5], slots=out[6],
                ranges="weight" if out[7] else "count")


def rank_wg_plan_residency(P, score_box=None, resident_per_cu=0, cus_per_xcd=0):
    """What that plan assumed of a CU (ppp_rank_wg_plan_residency): the thickness that sizes the LDS arrays of the
    kernel it launches, the workgroups per CU, the LDS bytes per workgroup, the CUs per XCD."""
    box = None if score_box is None else ctypes.byref(Box(*[int(v) for v in score_box]))
    out = (ctypes.c_int32 * 4)()
    check(lib().ppp_rank_wg_plan_residency(box, ctypes.byref(P), int(resident_per_cu), int(cus_per_xcd), out))
    return dict(lds_tz=out[0], resident=out[1], lds_bytes=out[2], cus_per_xcd=out[3])


def rank_vm_available(P):
    """True when ppp_rank_patches_vm handles this configuration (cubic 3/5/7/9 patches, float
    accumulation) and PPP_RANK does not ask for the gather kernel."""
    if os.environ.get("PPP_RANK", "vm") != "vm":
        return False
    Pv = P.copy()
    Pv.cons_layout = CONS_VOXEL_MAJOR
    # (the question is about the configuration, not a tile; with ring_z set -- "from a RING of rows?", which
    # only the workgroup-per-tile kernel reads -- the box is as thick as a ring may hold)
    Pv.cons_box = Box(0, 0, 0, P.Z, P.Y, P.X)
    if P.ring_z and P.ring_z < P.Z:
        # (a ring holds fewer slices than the volume: ask about centres whose rows fit into it)
        Pv.cons_box = Box(0, 0, 0, P.ring_z, P.Y, P.X)
        sb = Box(0, 0, 0, max(1, P.ring_z - P.pz // 2), P.Y, P.X)
        return int(lib().ppp_rank_workspace_bytes(ctypes.byref(sb), ctypes.byref(Pv))) > 0
    return int(lib().ppp_rank_workspace_bytes(None, ctypes.byref(Pv))) > 0


def pair_order(pairs, P):
    """Processing order for ppp_patch_graph: rows grouped by patch offset d = B - A, and by
    position of A inside a group.  pairs: device int32 [N, 6]; returns device int32 [N]."""
    torch = _torch()
    n = int(pairs.shape[0])
    keys = torch.empty((n,), dtype=torch.int64, device=pairs.device)
    check(lib().ppp_pair_sort_keys(_dev_ptr(pairs), n, _dev_ptr(keys), ctypes.byref(P), _stream()))
    return torch.argsort(keys).to(torch.int32)


def patch_graph_prepare(pred, pairs, Pv, ahead=False):
    """The part of S5 (patch_graph_by_patch) that needs no consensus: the rows grouped by patch A
    (inside a group by patch offset, so neighbouring lanes do similar work), the plan of the thinning
    masks and their buffers.  (`ahead` is accepted and ignored: rounds 4-5 ran the masks of tile t + 1
    on a side stream beside tile t's per-patch kernel; with a wave per pair the masks of a 512^3 step
    take 0.14 s and running them beside that kernel only slowed it -- 6.24 s in line, 6.70 s beside,
    DESIGN.md section 4 -- so the side stream is gone.)
    Pv: parameters of the FRAME `pred` and the rows live in (consensus box and ring do not matter)."""
    import types
    torch = _torch()
    n = int(pairs.shape[0])
    job = types.SimpleNamespace(n=n, n_live=0, plan=None, bufs=[None, None], masks_done=set(),
                                bits_centres=None, bits=None)
    job.aff = torch.zeros((n,), dtype=torch.float32, device=pred.device)
    if n == 0:
        return job
    with host_timer("s5e_group_sort"):
        keys = torch.empty((n,), dtype=torch.int64, device=pairs.device)
        check(lib().ppp_pair_group_keys(_dev_ptr(pairs), n, _dev_ptr(keys), ctypes.byref(Pv), _stream()))
        keys, order = torch.sort(keys)
        # rows that cannot share a stored consensus offset keep the zero aff was created with
        n_live = int(torch.searchsorted(keys, torch.tensor([PAIR_KEY_FAR], dtype=torch.int64,
                                                           device=keys.device)).item())
        note_add("s5_rows_dispatched", n_live)
        job.n_live = n_live
        if n_live == 0:
            return job
        keys, order = keys[:n_live], order[:n_live]
    dkey = keys & 0x1FFFF                         # patch offset B - A
    keys >>= 18                                   # linear index of patch A
    _, counts = torch.unique_consecutive(keys, return_counts=True)
    del keys
    zero = torch.zeros((1,), dtype=torch.int64, device=pred.device)
    job.group_start = torch.cat([zero, torch.cumsum(counts, 0)])
    chunk = int(lib().ppp_patch_graph_by_patch_chunk(ctypes.byref(Pv)))
    if chunk <= 0:
        raise RuntimeError("libppp_mi355x: no per-patch kernel for this patch shape")
    # few rows per patch (thinned covers): one- or two-wave workgroups
    small = int(lib().ppp_patch_graph_by_patch_chunk_small(ctypes.byref(Pv)))
    mode = os.environ.get("PPP_PA_CHUNK", "auto")
    if mode == "small" or (mode == "auto" and n_live <= 1.5 * small * int(counts.shape[0])):
        chunk = small
    job.chunk = chunk
    job.chunk_offsets = torch.cat([zero, torch.cumsum((counts + chunk - 1) // chunk, 0)])
    job.n_groups = int(counts.shape[0])
    job.order32 = order.to(torch.int32)
    oom = getattr(torch, "OutOfMemoryError", None) or torch.cuda.OutOfMemoryError
    # the foreground bits of every patch of the dispatched rows, once per patch (PPP_PA_BITS=0: built
    # inside the per-patch kernel, for every row; so they are when memory runs out in here)
    if os.environ.get("PPP_PA_BITS", "1") != "0":
        try:
            job.bits_centres, job.bits = patch_fg_bits(pred, pairs[order], Pv)
        except oom:
            job.bits_centres = job.bits = None
            torch.cuda.empty_cache()
    del order
    # thinning masks beforehand: the groups are cut into batches whose masks fit the budget (one
    # buffer, filled and read batch after batch; a second buffer when a batch's masks are made
    # beside the per-patch kernel of the batch before)
    # The plan's temporaries (about eight int64 per dispatched row) and the mask buffers are not
    # part of the tile planner's budget: the mask budget is capped by what is free right now, and
    # running out of memory anywhere in here falls back to the generator inside the kernel.
    plan = drops = None
    try:
        plan = _lcg_plan(dkey, job.group_start, Pv)
        if plan is not None:
            drops = torch.empty((plan["buffer_words"],), dtype=torch.int64, device=pred.device)
    except oom:
        plan = drops = None                       # the kernel runs the generator itself
        torch.cuda.empty_cache()
    del dkey
    job.plan = plan
    job.cuts = plan["group_cuts"] if plan is not None else [0, job.n_groups]
    co_host = job.chunk_offsets[torch.tensor(job.cuts, dtype=torch.int64, device=pred.device)].cpu().tolist()
    job.co_host = dict(zip(job.cuts, co_host))    # blocks before each cut: ONE copy for all batches
    job.bufs = [drops, drops]
    return job


def patch_fg_bits(pred, rows, Pv):
    """The foreground bits of every patch that occurs in `rows` (device int32 [n, 6]: centre of A,
    centre of B), once per patch (ppp_patch_fg_bits).  Returns (centres: int64 [m] ascending linear
    voxel indices in the frame of `pred`, bits: int32 [m, ceil(C / 32)])."""
    torch = _torch()
    rows = rows.to(torch.int64)
    lin = torch.cat([(rows[:, 0] * Pv.Y + rows[:, 1]) * Pv.X + rows[:, 2],
                     (rows[:, 3] * Pv.Y + rows[:, 4]) * Pv.X + rows[:, 5]])
    del rows
    centres = torch.unique(lin)                   # (sorted)
    del lin
    words = (Pv.pz * Pv.py * Pv.px + 31) // 32
    bits = torch.empty((int(centres.shape[0]), words), dtype=torch.int32, device=pred.device)
    with _timed("patch_graph_bits"):
        check(lib().ppp_patch_fg_bits(_dev_ptr(pred), pred_dtype_code(pred), _dev_ptr(centres),
                                      int(centres.shape[0]), _dev_ptr(bits), ctypes.byref(Pv), _stream()))
    return centres, bits


def _pa_masks(job, pred, pairs, Pv, b, slices=False):
    """the thinning masks of batch b into the buffer (filled and read batch after batch)"""
    n_b = len(job.cuts) - 1
    if job.plan is None or b >= n_b or b in job.masks_done:
        return
    lo, hi = job.plan["pos_cuts"][b], job.plan["pos_cuts"][b + 1]
    if hi > lo:
        fn = lib().ppp_patch_graph_lcg_slices if slices else lib().ppp_patch_graph_lcg
        with _timed("patch_graph_lcg"):
            check(fn(
                _dev_ptr(pred), pred_dtype_code(pred), _dev_ptr(pairs), _dev_ptr(job.order32),
                _dev_ptr(job.plan["pos"][lo:hi]), hi - lo, _dev_ptr(job.plan["drop_off"]),
                _dev_ptr(job.bufs[b % 2]), ctypes.byref(Pv), _stream()))
    job.masks_done.add(b)


def patch_graph_by_patch(pred, cons_vm, pairs, Pv, job=None, slices=False):
    """S5 with one workgroup per patch A (ppp_patch_graph_by_patch).  job: what patch_graph_prepare
    made for these rows (None: made here).  slices: the z axis is a stack of independent 2-d images
    (every image's own LCG seeds, ppp_patch_graph_by_patch_lcg_slices)."""
    if job is None:
        job = patch_graph_prepare(pred, pairs, Pv)
    aff = job.aff
    if job.n == 0 or job.n_live == 0:
        return aff
    plan, cuts = job.plan, job.cuts
    n_b = len(cuts) - 1
    for b in range(n_b):
        g0, g1 = cuts[b], cuts[b + 1]
        if plan is not None:
            _pa_masks(job, pred, pairs, Pv, b, slices)
        co = job.chunk_offsets[g0:g1 + 1]
        n_blocks = int(job.co_host[g1] - job.co_host[g0])
        with _timed("patch_graph"):
            check(lib().ppp_patch_graph_by_patch_bits(
                _dev_ptr(pred), pred_dtype_code(pred), _dev_ptr(cons_vm), _dev_ptr(pairs),
                _dev_ptr(job.order32), _dev_ptr(job.group_start[g0:g1 + 1].contiguous()),
                _dev_ptr((co - co[0]).contiguous()), g1 - g0, n_blocks, job.chunk, _dev_ptr(aff),
                _dev_ptr(plan["drop_off"]) if plan is not None else None,
                _dev_ptr(job.bufs[b % 2]) if plan is not None else None,
                _dev_ptr(job.bits_centres), 0 if job.bits is None else int(job.bits_centres.shape[0]),
                _dev_ptr(job.bits), 1 if slices else 0, ctypes.byref(Pv), _stream()))
    return aff


def lcg_words(dz, dy, dx, P):
    """uint64 words of precomputed thinning masks for a pair with patch offset (dz, dy, dx)
    (ppp_patch_graph_lcg_words as array arithmetic, for the patch widths whose kernel reads masks --
    the library returns 0 for the others; any integer arrays or scalars)."""
    nz, ny, nx = P.pz - abs(dz), P.py - abs(dy), P.px - abs(dx)
    rpc = 64 // P.px
    nch = (P.px + rpc - 1) // rpc
    inter = (nz > 0) & (ny > 0) & (nx > 0)
    return nz * ny * nx * nz * nch * inter


def _lcg_plan(dkey, group_start, Pv):
    """Which dispatched pair rows get their thinning decisions made beforehand (ppp_patch_graph_lcg):
    those whose windows intersect.  The groups (patches A) are cut into batches whose masks fit
    PPP_PA_LCG_BYTES (default 4 GiB -- a tile of the thinned 512^3 / 9^3 cover needs 1.9 GB; 0 = the
    per-patch kernel runs the generator itself; so it does for patch widths whose kernel does not
    read masks: ppp_patch_graph_lcg_words is 0 then), at most PPP_PA_LCG_BATCHES (64) of them: rows
    of later groups keep the generator.  dkey: offset code of the dispatched rows
    (ppp_pair_group_keys), group_start: int64 [groups + 1].  Returns None or a dict:
      group_cuts  [batches + 1] group indices, pos_cuts [batches + 1] cuts of `pos`,
      pos         int64 positions of the served rows, batch after batch, sorted by offset inside
      drop_off    int64 per dispatched row: word offset inside its batch's masks, -1 = none
      buffer_words  words of the largest batch"""
    torch = _torch()
    budget = int(os.environ.get("PPP_PA_LCG_BYTES", str(4 << 30)))
    if dkey.is_cuda:
        # never more than a quarter of what is free (+ what torch's allocator holds unused), after
        # the plan's own temporaries: ~8 int64 per dispatched row
        free = torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
        budget = min(budget, max(0, int(0.25 * (free - 64 * int(dkey.shape[0])))))
    budget //= 8
    max_batches = int(os.environ.get("PPP_PA_LCG_BATCHES", "64"))
    if budget <= 0 or int(lib().ppp_patch_graph_lcg_words(0, 0, 0, ctypes.byref(Pv))) <= 0:
        return None
    wx, wy = 4 * Pv.px + 1, 4 * Pv.py + 1
    dx = dkey % wx - 2 * Pv.px
    dy = (dkey // wx) % wy - 2 * Pv.py
    dz = dkey // (wx * wy) - 2 * Pv.pz
    words = lcg_words(dz, dy, dx, Pv)
    del dx, dy, dz
    ends = torch.cumsum(words, 0)
    total = int(ends[-1].item())
    if total == 0:
        return None
    n_groups = int(group_start.shape[0]) - 1
    zero = torch.zeros((1,), dtype=torch.int64, device=dkey.device)
    ends0 = torch.cat([zero, ends])                       # words before row i
    g_end = ends0[group_start[1:]]                        # words up to the end of group g
    g_words = g_end - ends0[group_start[:-1]]
    # windows of (budget - largest group) words: a batch = the groups that END in one window, so
    # it holds at most a window plus the part of its first group before the window
    window = budget - int(g_words.max().item())
    if window <= 0:
        return None
    batch_of_group = torch.clamp(g_end - 1, min=0) // window
    n_batches = int(batch_of_group[-1].item()) + 1
    n_served_batches = min(n_batches, max_batches)
    # (a group larger than the window leaves windows in which no group ends: number the batches
    # by the windows that do hold a group end, so that none is empty and PPP_PA_LCG_BATCHES counts
    # batches with work)
    _, batch_of_group = torch.unique_consecutive(batch_of_group, return_inverse=True)
    n_batches = int(batch_of_group[-1].item()) + 1
    n_served_batches = min(n_batches, max_batches)
    firsts = torch.searchsorted(batch_of_group, torch.arange(n_served_batches + 1, device=dkey.device))
    group_cuts = [int(v) for v in firsts.tolist()]
    if n_served_batches < n_batches:                      # the rest: one more launch, no masks
        group_cuts_all = group_cuts + [n_groups]
    else:
        group_cuts[-1] = n_groups
        group_cuts_all = group_cuts
    row_cuts = group_start[torch.tensor(group_cuts, device=dkey.device)]
    base = ends0[row_cuts]                                # words before each served batch (+ end)
    n_rows = int(dkey.shape[0])
    batch_of_row = torch.clamp(torch.searchsorted(row_cuts, torch.arange(n_rows, device=dkey.device),
                                                  right=True) - 1, max=n_served_batches)
    served = (words > 0) & (batch_of_row < n_served_batches)
    drop_off = torch.where(served, ends - words - base[torch.clamp(batch_of_row, max=n_served_batches - 1)],
                           torch.full_like(ends, -1))
    pos = torch.nonzero(served).reshape(-1)
    # batch after batch; inside a batch the lanes of a wave = rows of (nearly) the same offset
    pos = pos[torch.argsort(batch_of_row[pos] * (1 << 17) + dkey[pos])]
    pos_cuts = torch.searchsorted(batch_of_row[pos].contiguous(),
                                  torch.arange(n_served_batches + 1, device=dkey.device)).tolist()
    buffer_words = int((base[1:] - base[:-1]).max().item())
    note_add("s5_rows_lcg_beforehand", int(pos.shape[0]))
    note_add("s5_lcg_batches", n_served_batches)
    return dict(group_cuts=group_cuts_all, pos_cuts=[int(v) for v in pos_cuts] + [int(pos.shape[0])] *
                (len(group_cuts_all) - len(group_cuts)), pos=pos.contiguous(),
                drop_off=drop_off.contiguous(), buffer_words=max(buffer_words, 1))


def patch_graph_auto(pred, cons_compact, pairs, P, job=None, slices=False):
    """S5 from a COMPACT consensus: re-layout to voxel-major, then the workgroup-per-patch
    kernel (consensus rows staged once per patch in LDS; 0.3 TB instead of 5.4 TB of HBM reads
    on the 140^3 benchmark).  PPP_PATCH_GRAPH=pairs selects the pair-per-lane gather kernel
    with offset-grouped lanes (same bits), which is also what patch shapes without a per-patch
    specialisation use."""
    if P.cons_layout == CONS_VOXEL_MAJOR:
        vm, Pv = cons_compact, P          # already re-laid out (kept from the ranking stage)
    elif getattr(cons_compact, "_ppp_vm", None) is not None:
        vm, Pv = cons_compact._ppp_vm     # the ranking stage of the stage pipeline left it here
        cons_compact._ppp_vm = None
    else:
        vm, Pv = cons_to_voxel_major(cons_compact, P)
    if os.environ.get("PPP_PATCH_GRAPH", "patch") != "pairs" and \
            int(lib().ppp_patch_graph_by_patch_chunk(ctypes.byref(Pv))) > 0 and \
            max(P.pz, P.py) <= P.px:
        return patch_graph_by_patch(pred, vm, pairs, Pv, job=job, slices=slices)
    return patch_graph(pred, vm, pairs, Pv, order=pair_order(pairs, Pv), slices=slices)


def device_patch_pairs(sorted_zyx, P, max_ps_dist=2, include_single=True, slices=False):
    """Pair rows on the device from the x-sorted selected list (device int32 [n, 3]).
    Returns device int32 [rows, 6] (uint32 bit patterns) or None when there are no rows.
    slices: the z axis is a stack of independent 2-d images, the list is sorted by (z, x) and
    partners are searched in the same slice only (ppp_patch_pairs_*_slices)."""
    torch = _torch()
    n = int(sorted_zyx.shape[0])
    counts = torch.zeros((max(n, 1),), dtype=torch.int64, device=sorted_zyx.device)
    count_fn = lib().ppp_patch_pairs_count_slices if slices else lib().ppp_patch_pairs_count
    fill_fn = lib().ppp_patch_pairs_fill_slices if slices else lib().ppp_patch_pairs_fill
    with _timed("patch_pairs"):
        check(count_fn(_dev_ptr(sorted_zyx), n, int(max_ps_dist),
                       _dev_ptr(counts), ctypes.byref(P), _stream()))
        ends = torch.cumsum(counts, 0)
        n_rows = int(ends[n - 1].item()) if n else 0
        total = n_rows + (n if include_single else 0)
        if total == 0:
            return None
        offsets = (ends - counts).contiguous()
        rows = torch.empty((total, 6), dtype=torch.int32, device=sorted_zyx.device)
        check(fill_fn(_dev_ptr(sorted_zyx), n, int(max_ps_dist),
                      _dev_ptr(offsets), n_rows, 1 if include_single else 0,
                      _dev_ptr(rows), ctypes.byref(P), _stream()))
    return rows


def pair_counts_subset(sorted_zyx, subset, P, max_ps_dist=2):
    """Number of partners j > i of the patches listed in `subset` (device int64 indices into the
    x-sorted list).  Returns device int64 [n], zero outside the subset."""
    torch = _torch()
    n = int(sorted_zyx.shape[0])
    counts = torch.zeros((max(n, 1),), dtype=torch.int64, device=sorted_zyx.device)
    m = int(subset.numel())
    if n and m:
        with _timed("patch_pairs"):
            check(lib().ppp_patch_pairs_count_subset(_dev_ptr(sorted_zyx), n, int(max_ps_dist),
                                                     _dev_ptr(subset), m, _dev_ptr(counts),
                                                     ctypes.byref(P), _stream()))
    return counts[:n]


def pairs_subset(sorted_zyx, subset, counts, goffsets, n_rows_total, P, max_ps_dist=2,
                 include_single=True):
    """Pair rows of the patches in `subset` (device int64 [m], ascending) written compactly, in
    the canonical order, with their GLOBAL row ids: rows int32 [r (+ m), 6], ids int64 [r (+ m)].
    counts / goffsets: device int64 [n] (partners per patch, exclusive scan over all patches)."""
    torch = _torch()
    n, m = int(sorted_zyx.shape[0]), int(subset.numel())
    if m == 0:
        return None, None
    local_counts = counts[subset]
    ends = torch.cumsum(local_counts, 0)
    n_local = int(ends[-1].item())
    total = n_local + (m if include_single else 0)
    if total == 0:
        return None, None
    local_off = (ends - local_counts).contiguous()
    rows = torch.empty((total, 6), dtype=torch.int32, device=sorted_zyx.device)
    gid = torch.empty((total,), dtype=torch.int64, device=sorted_zyx.device)
    with _timed("patch_pairs"):
        check(lib().ppp_patch_pairs_fill_subset(
            _dev_ptr(sorted_zyx), n, int(max_ps_dist), _dev_ptr(subset.contiguous()), m,
            _dev_ptr(local_off), _dev_ptr(goffsets.contiguous()), n_local, int(n_rows_total),
            1 if include_single else 0, _dev_ptr(rows), _dev_ptr(gid), ctypes.byref(P), _stream()))
    return rows, gid


class LabelState:
    """Streaming union-find over the selected patches (ppp_label_begin / _add / _finish).
    The workspace is a torch tensor, so the node entries of its four volumes (parent u32,
    has-positive-edge u32, firstpos u64, key u64, all indexed by linear voxel index) can be
    read and written with torch indexing when ranks merge their forests."""

    def __init__(self, nodes, P):
        torch = _torch()
        self.torch, self.P, self.nodes = torch, P, nodes.contiguous()
        self.n = int(nodes.shape[0])
        V = int(P.Z) * int(P.Y) * int(P.X)
        self.V = V
        self.work = _workspace(lib().ppp_label_workspace_bytes(ctypes.byref(P)), nodes.device)
        self.parent = self.work[:4 * V].view(torch.int32)
        self.haspos = self.work[4 * V:8 * V].view(torch.int32)
        self.firstpos = self.work[8 * V:16 * V].view(torch.int64)
        n64 = nodes.to(torch.int64)
        self.lin = (n64[:, 0] * int(P.Y) + n64[:, 1]) * int(P.X) + n64[:, 2]
        with _timed("label_components"):
            check(lib().ppp_label_begin(_dev_ptr(self.nodes), self.n, _dev_ptr(self.work),
                                        ctypes.byref(P), _stream()))

    def add(self, rows, aff, gid=None, first_id=0):
        n = int(rows.shape[0])
        if n == 0:
            return
        with _timed("label_components"):
            check(lib().ppp_label_add(_dev_ptr(rows), _dev_ptr(aff), _dev_ptr(gid), int(first_id), n,
                                      _dev_ptr(self.work), ctypes.byref(self.P), _stream()))

    def export(self):
        """(parent, firstpos, haspos) of the nodes: int64 [n] linear voxel index of the node's
        parent, int64 [n], int32 [n]."""
        return (self.parent[self.lin].to(self.torch.int64) & 0xFFFFFFFF,
                self.firstpos[self.lin].clone(), self.haspos[self.lin].clone())

    def merge(self, parents, firstpos, haspos):
        """parents: int64 [k, n] forests of k ranks (this rank's included or not); firstpos /
        haspos: the element-wise MIN / MAX over all ranks."""
        for row in parents.reshape(-1, self.n):
            with _timed("label_components"):
                check(lib().ppp_label_union_edges(_dev_ptr(self.lin.contiguous()),
                                                  _dev_ptr(row.contiguous()), self.n,
                                                  _dev_ptr(self.work), ctypes.byref(self.P), _stream()))
        self.firstpos[self.lin] = firstpos
        self.haspos[self.lin] = haspos.to(self.torch.int32)

    def finish(self):
        """int64 [n]: order key of the node's component, NONE_KEY64 = not in a component."""
        keys = self.torch.empty((self.n,), dtype=self.torch.int64, device=self.nodes.device)
        if self.n:
            with _timed("label_components"):
                check(lib().ppp_label_finish(_dev_ptr(self.nodes), self.n, _dev_ptr(keys),
                                             _dev_ptr(self.work), ctypes.byref(self.P), _stream()))
        return keys


def patch_graph(pred, cons, pairs, P, order=None, slices=False):
    """S5.  pairs: device uint32-as-int32 [N, 6]; order: optional device int32 permutation
    (see pair_order); returns float32 [N].  slices: every image of a stack of 2-d images seeds
    its pairs' LCG with its own coordinates (ppp_patch_graph_slices)."""
    torch = _torch()
    n = int(pairs.shape[0])
    aff = torch.zeros((n,), dtype=torch.float32, device=pred.device)
    fn = lib().ppp_patch_graph_slices if slices else lib().ppp_patch_graph
    with _timed("patch_graph"):
        check(fn(_dev_ptr(pred), pred_dtype_code(pred), _dev_ptr(cons), _dev_ptr(pairs), _dev_ptr(order), n,
                 _dev_ptr(aff), ctypes.byref(P), _stream()))
    return aff


def label_components(pairs, aff, nodes, P):
    """S6 (components).  nodes: device int32 [K, 3]; returns int64 [K] order keys
    (NONE_KEY = not in a component)."""
    torch = _torch()
    n = 0 if pairs is None else int(pairs.shape[0])
    k = int(nodes.shape[0])
    keys = torch.empty((k,), dtype=torch.int32, device=nodes.device)
    work = _workspace(lib().ppp_label_workspace_bytes(ctypes.byref(P)), nodes.device)
    with _timed("label_components"):
        check(lib().ppp_label_components(_dev_ptr(pairs), _dev_ptr(aff), n, _dev_ptr(nodes), k,
                                         _dev_ptr(keys), _dev_ptr(work), ctypes.byref(P),
                                         _stream()))
    return keys.to(torch.int64) & 0xFFFFFFFF


def label_slice_renumber(nodes, labels, P):
    """Ids per slice of a stack of independent 2-d images (ppp_label_slice_renumber).  nodes int32
    [K, 3] device, labels int32 [K] device: ranks over the stack ascending by (slice, order key),
    renumbered in place from 1 in every slice.  Returns the largest id of every slice (int32 [Z])."""
    torch = _torch()
    slice_min = torch.empty((int(P.Z),), dtype=torch.int32, device=nodes.device)
    slice_max = torch.empty((int(P.Z),), dtype=torch.int32, device=nodes.device)
    with _timed("label_slice_renumber"):
        check(lib().ppp_label_slice_renumber(_dev_ptr(nodes.contiguous()), int(nodes.shape[0]),
                                             _dev_ptr(labels), _dev_ptr(slice_min), _dev_ptr(slice_max),
                                             ctypes.byref(P), _stream()))
    return slice_max


def paint_instances(pred, nodes, labels, instances, P):
    """S6 (paint).  nodes int32 [K, 3], labels int32 [K], instances int32 (Z, Y, X) in place."""
    with _timed("paint_instances"):
        check(lib().ppp_paint_instances(_dev_ptr(pred), pred_dtype_code(pred), _dev_ptr(nodes),
                                        _dev_ptr(labels), int(nodes.shape[0]),
                                        _dev_ptr(instances), ctypes.byref(P), _stream()))
    return instances


# ---- no_overlap_per_channel: sizes + overlap pairs, the greedy walk, the paint by channel ----------
PACK_MIN_VOXELS = 2000      # graph_to_labeling.py:98


def pack_scan(pred, nodes, labels, n_labels, P, own=None, sizes=None):
    """Sizes and overlap pairs of the components (ppp_pack_scan_count / _fill).  nodes int32 [K, 3] and
    labels int32 [K] (1 .. n_labels) in the frame of P; own = (z0, y0, x0, z1, y1, x1) of the frame's
    voxels to count (None: all).  Returns (sizes int64 [n_labels + 1] on the device, slot 0 unused --
    `sizes` given: added to in place -- and pair keys int64 [n], (b << 32) | a with a < b, one per
    pair and shared voxel: not yet unique)."""
    torch = _torch()
    dev = pred.device
    if sizes is None:
        sizes = torch.zeros((int(n_labels) + 1,), dtype=torch.int64, device=dev)
    box = Box(*[int(v) for v in own]) if own is not None else Box(0, 0, 0, P.Z, P.Y, P.X)
    work = _workspace(lib().ppp_pack_scan_workspace_bytes(ctypes.byref(P), ctypes.byref(box)), dev)
    n_pairs = ctypes.c_int64(0)
    with _timed("pack_scan"):
        check(lib().ppp_pack_scan_count(_dev_ptr(pred), pred_dtype_code(pred), _dev_ptr(nodes), _dev_ptr(labels),
                                        int(nodes.shape[0]), int(n_labels), ctypes.byref(box), _dev_ptr(sizes),
                                        ctypes.byref(n_pairs), _dev_ptr(work), ctypes.byref(P), _stream()))
        pairs = torch.empty((int(n_pairs.value),), dtype=torch.int64, device=dev)
        check(lib().ppp_pack_scan_fill(_dev_ptr(pred), pred_dtype_code(pred), ctypes.byref(box), _dev_ptr(pairs),
                                       int(n_pairs.value), _dev_ptr(work), ctypes.byref(P), _stream()))
    return sizes, pairs


def host_pack_channels(sizes, pairs, min_voxels=PACK_MIN_VOXELS):
    """ppp_host_pack_channels.  sizes: voxels of component k (label k + 1), host array [K]; pairs: host
    array of keys (b << 32) | a of overlapping labels a < b.  Returns (chan int32 [K], n_channels)."""
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    pairs = np.ascontiguousarray(pairs).astype(np.uint64, copy=False)
    chan = np.zeros(len(sizes), dtype=np.int32)
    n_ch = ctypes.c_int32(0)
    if lib().ppp_host_pack_channels(len(sizes), _np_ptr(sizes), _np_ptr(pairs), len(pairs), int(min_voxels),
                                    _np_ptr(chan), ctypes.byref(n_ch)) < 0:
        raise RuntimeError("libppp_mi355x: ppp_host_pack_channels: bad arguments")
    return chan, int(n_ch.value)


def paint_instances_channels(pred, nodes, labels, chan, n_channels, out, P):
    """S6 (paint by channel).  chan int32 [n_labels + 1] on the device (slot 0 unused): label l goes to
    out[chan[l]]; out int32 (n_channels, Z, Y, X) in place, the largest label of a channel wins."""
    with _timed("paint_instances"):
        check(lib().ppp_paint_instances_channels(_dev_ptr(pred), pred_dtype_code(pred), _dev_ptr(nodes),
                                                 _dev_ptr(labels), int(nodes.shape[0]), _dev_ptr(chan),
                                                 int(chan.numel()) - 1, int(n_channels), _dev_ptr(out),
                                                 ctypes.byref(P), _stream()))
    return out


def pack_channels(sizes, pairs):
    """sizes (device, [n_labels + 1]) and pair keys (device, any order, repeats allowed) -> (chan int32
    [n_labels + 1] on the device, slot 0 unused, and the channel count): unique, then the host walk."""
    torch = _torch()
    uniq = torch.unique(pairs) if pairs.numel() else pairs
    chan, n_ch = host_pack_channels(sizes[1:].cpu().numpy(), uniq.cpu().numpy())
    chan_dev = torch.from_numpy(np.concatenate([np.zeros(1, np.int32), chan])).to(sizes.device)
    return chan_dev, n_ch


# ---- the reference's NumPy-semantics stages (cuda=False) -------------------------------------------
def np_consensus(pred, foreground, P):
    """create_consensus_array (consensus_array.py:18-68) on the device: int16 votes
    [planes, Z, Y, X] (plane 0 = zero offset, plane q = COMPACT plane q - 1)."""
    torch = _torch()
    planes = int(lib().ppp_np_vote_planes(ctypes.byref(P)))
    votes = torch.empty((planes, P.Z, P.Y, P.X), dtype=torch.int16, device=pred.device)
    with _timed("np_consensus"):
        check(lib().ppp_np_consensus(_dev_ptr(pred), pred_dtype_code(pred), _dev_ptr(foreground), _dev_ptr(votes),
                                     ctypes.byref(P), _stream()))
    return votes


def np_rank_patches(pred, foreground, votes, P):
    """rank_patches (ranked_patches.py:76-105) on the device: int32 scores (Z, Y, X)."""
    torch = _torch()
    score = torch.empty((P.Z, P.Y, P.X), dtype=torch.int32, device=pred.device)
    with _timed("np_rank_patches"):
        check(lib().ppp_np_rank_patches(_dev_ptr(pred), pred_dtype_code(pred), _dev_ptr(foreground), _dev_ptr(votes),
                                        _dev_ptr(score), ctypes.byref(P), _stream()))
    return score


def np_patch_graph(pred, mask, votes, rows, P):
    """computePatchGraph's NumPy branch (aff_patch_graph.py:209-282) for candidate rows int32 [n, 6]:
    (weight int64 [n], count int32 [n])."""
    torch = _torch()
    n = int(rows.shape[0])
    weight = torch.zeros((n,), dtype=torch.int64, device=pred.device)
    count = torch.zeros((n,), dtype=torch.int32, device=pred.device)
    if n:
        with _timed("np_patch_graph"):
            check(lib().ppp_np_patch_graph(_dev_ptr(pred), pred_dtype_code(pred), _dev_ptr(mask), _dev_ptr(votes),
                                           _dev_ptr(rows), n, _dev_ptr(weight), _dev_ptr(count), ctypes.byref(P),
                                           _stream()))
    return weight, count


def paint_patch_rows(rows, nodes, labels, instances, P):
    """S6 (paint) from a patch table: rows float16 / bfloat16 / float32 [K, C] (row k = pred[:, node k]),
    nodes int32 [K, 3], labels int32 [K], instances int32 (Z, Y, X) in place."""
    assert rows.is_contiguous() and rows.shape[0] == nodes.shape[0]
    with _timed("paint_instances"):
        check(lib().ppp_paint_patch_rows(_dev_ptr(rows), pred_dtype_code(rows), _dev_ptr(nodes),
                                         _dev_ptr(labels), int(nodes.shape[0]),
                                         _dev_ptr(instances), ctypes.byref(P), _stream()))
    return instances


def direct_voxel_major(P):
    """S1 can write the voxel-major layout itself for these parameters."""
    Pv = P.copy()
    Pv.cons_layout = CONS_VOXEL_MAJOR
    return os.environ.get("PPP_S1_DIRECT_VM", "1") != "0" and \
        lib().ppp_consensus_writes_voxel_major(ctypes.byref(Pv)) == 1


def consensus_voxel_major(pred, overlap, P, out=None, open_rows=False):
    """S1 straight into the symmetric voxel-major layout when the library can do that for these
    parameters (ppp_consensus_writes_voxel_major), else COMPACT + ppp_cons_to_voxel_major.
    Returns (tensor [bz, by, bx, W], params with cons_layout = VOXEL_MAJOR).  out: see consensus."""
    Pv = P.copy()
    Pv.cons_layout = CONS_VOXEL_MAJOR
    if direct_voxel_major(P):
        return consensus(pred, overlap, Pv, out=out, open_rows=open_rows), Pv
    Pc = P.copy()
    Pc.cons_layout = CONS_COMPACT
    cons = consensus(pred, overlap, Pc)
    return cons_to_voxel_major(cons, Pc)


def consensus_part(pred, overlap, P, part, out):
    """S1 for the base voxels of `part` (z0, y0, x0, z1, y1, x1; inside P.cons_box) written into
    `out`, a buffer indexed by the whole P.cons_box (COMPACT planes or open VOXEL_MAJOR rows)."""
    b = Box(*[int(v) for v in part])
    note_add("s1_base_voxels", int(np.prod(b.shape())))
    P = with_pred_clean(pred, P)
    with _timed("consensus"):
        if not _consensus_sparse(pred, overlap, out, None, P, b, True):
            check(lib().ppp_consensus_part(_dev_ptr(pred), pred_dtype_code(pred), _dev_ptr(overlap), _dev_ptr(out),
                                           ctypes.byref(P), ctypes.byref(b), _stream()))
    note("s1_kernel", lib().ppp_consensus_kernel_name().decode())
    note("s1_short_form", int(lib().ppp_consensus_short_form()))


def cons_planes_to_rows(planes, planes_box, P, out=None):
    """VOXEL_MAJOR rows of P.cons_box cut from COMPACT planes indexed by `planes_box`
    (ppp_cons_planes_to_rows).  Returns (tensor [bz, by, bx, W], params with VOXEL_MAJOR)."""
    Pv = P.copy()
    Pv.cons_layout = CONS_VOXEL_MAJOR
    W = (2 * P.pz - 1) * (2 * P.py - 1) * (2 * P.px - 1)
    shape = Pv.cons_box.shape() + (W,)
    n_el = int(np.prod(shape))
    rows = out[:n_el].view(shape) if out is not None and out.numel() >= n_el else _big_empty(shape, planes.device)
    b = Box(*[int(v) for v in planes_box])
    with _timed("cons_planes_to_rows"):
        check(lib().ppp_cons_planes_to_rows(_dev_ptr(planes), ctypes.byref(b), _dev_ptr(rows), ctypes.byref(Pv),
                                            _stream()))
    return rows, Pv


def cons_to_reference(cons_compact, P):
    torch = _torch()
    shape = (2 * P.pz if P.pz > 1 else 1, 2 * P.py, 2 * P.px, P.Z, P.Y, P.X)
    ref = torch.empty(shape, dtype=torch.float32, device=cons_compact.device)
    check(lib().ppp_cons_to_reference(_dev_ptr(cons_compact), _dev_ptr(ref), ctypes.byref(P),
                                      _stream()))
    return ref


def cons_to_voxel_major(cons_compact, P):
    """Re-layout for ppp_patch_graph.  Returns (tensor [bz, by, bx, W], params with
    cons_layout = VOXEL_MAJOR)."""
    torch = _torch()
    W = (2 * P.pz - 1) * (2 * P.py - 1) * (2 * P.px - 1)
    vm = _big_empty(P.cons_box.shape() + (W,), cons_compact.device)
    Pc = P.copy()
    Pc.cons_layout = CONS_COMPACT
    with _timed("cons_to_voxel_major"):
        check(lib().ppp_cons_to_voxel_major(_dev_ptr(cons_compact), _dev_ptr(vm), ctypes.byref(Pc),
                                            _stream()))
    Pv = P.copy()
    Pv.cons_layout = CONS_VOXEL_MAJOR
    return vm, Pv


def patch_bits(pred, centres, thresh, P, scratch=None):
    """Bit r of row k = (pred[r][centre k] > float32(thresh)).  centres int32 [n, 3] on the
    device; returns int32 [n, ceil(C/32)] on the device.  scratch: a flat int32 device buffer the
    dense path may carve its per-voxel table and the result from (the caller's idle consensus
    pool: the two are 23 GB at 512^3 / 9^3)."""
    torch = _torch()
    n = int(centres.shape[0])
    words = (P.pz * P.py * P.px + 31) // 32
    V = int(P.Z) * int(P.Y) * int(P.X)
    dense = n * 16 >= V and os.environ.get("PPP_PATCH_BITS", "auto") != "sparse"
    vol = None
    if dense:
        # many centres (the cover candidates): one coalesced pass over the prediction for all
        # voxels, then a row gather -- instead of one cache line per (centre, channel)
        if scratch is not None and scratch.numel() >= V * words:
            vol = scratch[:V * words].view(V, words)
            scratch = scratch[V * words:]
        else:
            scratch = None
            try:
                vol = torch.empty((V, words), dtype=torch.int32, device=pred.device)
            except RuntimeError:          # no room for the per-voxel table: per-centre gathers
                dense = False
    if dense:
        with _timed("patch_bits"):
            check(lib().ppp_patch_bits_volume(_dev_ptr(pred), pred_dtype_code(pred), float(thresh),
                                              _dev_ptr(vol), ctypes.byref(P), _stream()))
            c = centres.to(torch.int64)
            lin = (c[:, 0] * int(P.Y) + c[:, 1]) * int(P.X) + c[:, 2]
            del c
            if scratch is not None and scratch.numel() >= n * words:
                bits = torch.index_select(vol, 0, lin, out=scratch[:n * words].view(n, words))
            else:
                bits = vol[lin]
        del vol
        return bits
    bits = torch.empty((n, words), dtype=torch.int32, device=pred.device)
    with _timed("patch_bits"):
        check(lib().ppp_patch_bits(_dev_ptr(pred), pred_dtype_code(pred), _dev_ptr(centres), n,
                                   float(thresh), _dev_ptr(bits), ctypes.byref(P), _stream()))
    return bits


def cover_pass_device(mask, bits, lin, state, pix_th, P, bits_first_voxel=None, mark_bits=None):
    """One pass of the greedy cover on the device (foreground_cover.py:111-180 without the stop
    rule, see ppp_cover_pass).  mask uint8 (Z,Y,X) is cleared in place; state int32 [n]
    (0 = takes part; ends 1 selected / 2 not) is updated in place.  bits: int32 [n, words] in
    list order, or -- bits_first_voxel given -- a table with a row per voxel whose first row
    belongs to that linear voxel index (ppp_cover_pass_voxel_bits).  mark_bits (cover_mark_bits):
    the pass with `mark_close_neighboorhood`, marks read and written in place
    (ppp_cover_pass_marked[_voxel_bits]).
    Returns (cleared int32 [n], rounds)."""
    torch = _torch()
    n = int(state.numel())
    cleared = torch.empty(n, dtype=torch.int32, device=mask.device)
    work = _workspace(lib().ppp_cover_workspace_bytes(n, ctypes.byref(P)), mask.device)
    rounds = ctypes.c_int32(0)
    with _timed("cover"):
        if mark_bits is not None and bits_first_voxel is None:
            check(lib().ppp_cover_pass_marked(_dev_ptr(mask), _dev_ptr(bits), _dev_ptr(lin), n, int(pix_th),
                                              _dev_ptr(state), _dev_ptr(cleared), _dev_ptr(mark_bits),
                                              _dev_ptr(work), ctypes.byref(P), _stream(), ctypes.byref(rounds)))
        elif mark_bits is not None:
            check(lib().ppp_cover_pass_marked_voxel_bits(_dev_ptr(mask), _dev_ptr(bits), int(bits_first_voxel),
                                                         _dev_ptr(lin), n, int(pix_th), _dev_ptr(state),
                                                         _dev_ptr(cleared), _dev_ptr(mark_bits), _dev_ptr(work),
                                                         ctypes.byref(P), _stream(), ctypes.byref(rounds)))
        elif bits_first_voxel is None:
            check(lib().ppp_cover_pass(_dev_ptr(mask), _dev_ptr(bits), _dev_ptr(lin), n, int(pix_th),
                                       _dev_ptr(state), _dev_ptr(cleared), _dev_ptr(work),
                                       ctypes.byref(P), _stream(), ctypes.byref(rounds)))
        else:
            check(lib().ppp_cover_pass_voxel_bits(_dev_ptr(mask), _dev_ptr(bits), int(bits_first_voxel),
                                                  _dev_ptr(lin), n, int(pix_th), _dev_ptr(state),
                                                  _dev_ptr(cleared), _dev_ptr(work), ctypes.byref(P),
                                                  _stream(), ctypes.byref(rounds)))
    return cleared, int(rounds.value)


def cover_mark_bits(P, device):
    """An empty mark volume of `mark_close_neighboorhood` (int32 words, ppp_cover_mark_bits_bytes)."""
    torch = _torch()
    nbytes = int(lib().ppp_cover_mark_bits_bytes(ctypes.byref(P)))
    if nbytes < 0:
        raise RuntimeError("ppp_cover_mark_bits_bytes: invalid parameters")
    return torch.zeros(nbytes // 4, dtype=torch.int32, device=device)


def cover_marks_from_selected(lin, selected, mark_bits, P):
    """Rebuild mark_bits from the centres lin int64 [n] with selected bool / uint8 [n] set (None: all);
    foreground_cover.py:162-168 for each of them (ppp_cover_marks_from_selected)."""
    torch = _torch()
    lin = lin.contiguous()
    sel = None if selected is None else selected.to(torch.uint8).contiguous()
    with _timed("cover"):
        check(lib().ppp_cover_marks_from_selected(_dev_ptr(lin), None if sel is None else _dev_ptr(sel),
                                                  int(lin.numel()), _dev_ptr(mark_bits), ctypes.byref(P),
                                                  _stream()))
    return mark_bits


def mask_dilate(mask, iterations, P, use_z=True):
    """scipy.ndimage.binary_dilation(mask != 0, iterations=iterations) on the device, uint8 0 / 1 out;
    use_z=False: every slice on its own (ppp_mask_dilate; foreground_cover.py:57-60)."""
    torch = _torch()
    mask = mask.contiguous()
    if mask.dtype != torch.uint8:
        mask = (mask != 0).to(torch.uint8)
    out = torch.empty_like(mask)
    work = _workspace(lib().ppp_mask_dilate_workspace_bytes(ctypes.byref(P)), mask.device)
    with _timed("cover"):
        check(lib().ppp_mask_dilate(_dev_ptr(mask), _dev_ptr(out), int(iterations), 1 if use_z else 0,
                                    _dev_ptr(work), ctypes.byref(P), _stream()))
    return out


def thin_cover_device(mask, bits, lin, P, slice_interior=None):
    """Set-cover thinning on the device (ppp_thin_cover; foreground_cover.py:183-256).
    mask uint8 (Z,Y,X) device tensor = mask_to_cover (not modified), bits int32 [n, words] /
    lin int64 [n]: the selected patches in list order.  Returns keep, bool [n] device tensor.
    slice_interior (int64 [Z] host array): the z axis is a stack of independent 2-d images whose
    interiors hold that many set voxels -- the loop's stop rule per slice (ppp_thin_cover_slices)."""
    torch = _torch()
    n = int(lin.numel())
    keep = torch.zeros(max(n, 1), dtype=torch.uint8, device=mask.device)
    if n == 0:
        return keep[:0].bool()
    work = _workspace(lib().ppp_thin_workspace_bytes(n, ctypes.byref(P)), mask.device)
    rounds = ctypes.c_int32(0)
    with _timed("thin_cover"):
        if slice_interior is None:
            check(lib().ppp_thin_cover(_dev_ptr(mask), _dev_ptr(bits.contiguous()), _dev_ptr(lin.contiguous()),
                                       n, _dev_ptr(keep), _dev_ptr(work), ctypes.byref(P), _stream(),
                                       ctypes.byref(rounds)))
        else:
            si = np.ascontiguousarray(slice_interior, dtype=np.int64)
            assert si.shape == (int(P.Z),)
            check(lib().ppp_thin_cover_slices(_dev_ptr(mask), _dev_ptr(bits.contiguous()),
                                              _dev_ptr(lin.contiguous()), n, _dev_ptr(keep), _dev_ptr(work),
                                              _np_ptr(si), ctypes.byref(P), _stream(), ctypes.byref(rounds)))
    note("thin_rounds", rounds.value)
    return keep[:n].bool()


class _RoundShard:
    """What one rank's share of the cover rounds and of the thinning rounds have in common: the steps of a
    round, the zones and the end, over the entry points ppp_<ENTRY>_step / _alive / _zone / _close."""
    COUNT, FILTER, SELECT = 0, 1, 2
    ENTRY = TIMER = None

    def __init__(self, mask, lin_local, bits, P, global_z, work_bytes):
        self.P, self.mask, self.bits = P, mask, bits
        self.lin = lin_local.contiguous()
        self.n = int(lin_local.numel())
        self.gz = int(global_z)
        self.work = _workspace(work_bytes, mask.device)

    def _entry(self, name):
        return getattr(lib(), "ppp_%s_%s" % (self.ENTRY, name))

    def step(self, what, *args):
        """what: COUNT / FILTER / SELECT; args: the subclass's (_step_lists)"""
        with _timed(self.TIMER):
            check(self._entry("step")(int(what), _dev_ptr(self.bits), *self._step_lists(*args), _dev_ptr(self.work),
                                      self.gz, ctypes.byref(self.P), _stream()))

    def alive(self):
        a = ctypes.c_int32(0)
        check(self._entry("alive")(_dev_ptr(self.work), ctypes.byref(self.P), _stream(), ctypes.byref(a)))
        return a.value != 0

    def zone(self, imp, z_lo, z_hi, own, key=None, mask=None, clean=None, rank=None):
        """key (int32 ranks in the cover, int64 keys in the thinning) or mask + clean: the buffers of the local
        slices [z_lo, z_hi), written (imp false; key "not mine" outside the own slices `own`) or read.
        rank: the cover's earlier name of `key`, still accepted."""
        key = rank if key is None else key
        with _timed(self.TIMER):
            check(self._entry("zone")(1 if imp else 0, _dev_ptr(self.work), int(z_lo), int(z_hi), int(own[0]),
                                      int(own[1]), _dev_ptr(key), _dev_ptr(mask), _dev_ptr(clean),
                                      ctypes.byref(self.P), _stream()))

    def close(self):
        with _timed(self.TIMER):
            check(self._entry("close")(_dev_ptr(self.mask), _dev_ptr(self.work), ctypes.byref(self.P), _stream()))


class CoverShard(_RoundShard):
    """One rank's share of the greedy cover rounds (ppp_cover_open / _step / _zone / _close):
    local mask uint8 (Zl, Y, X) device tensor (own slices + halo), the own ranked patches (local
    linear indices, global ranks, local bit table), local params with origin_z = first slice."""
    ENTRY, TIMER = "cover", "cover"

    def __init__(self, mask, lin_local, rank_id, bits, P, global_z):
        super().__init__(mask, lin_local, bits, P, global_z,
                         lib().ppp_cover_workspace_bytes(int(lin_local.numel()), ctypes.byref(P)))
        self.rank_id = rank_id.contiguous()
        self.state = self.cleared = None

    def open(self, state):
        """state int32 [n]: 0 takes part, 1 selected in an earlier pass, 2 never."""
        torch = _torch()
        self.state = state.contiguous()
        self.cleared = torch.empty(max(self.n, 1), dtype=torch.int32, device=self.mask.device)
        with _timed("cover"):
            check(lib().ppp_cover_open(_dev_ptr(self.mask), _dev_ptr(self.lin), _dev_ptr(self.rank_id),
                                       self.n, _dev_ptr(self.state), _dev_ptr(self.cleared),
                                       _dev_ptr(self.work), ctypes.byref(self.P), _stream()))

    def _step_lists(self, pix_th=0):
        return int(pix_th), _dev_ptr(self.state), _dev_ptr(self.cleared)


class ThinShard(_RoundShard):
    """One rank's share of the set-cover thinning rounds (ppp_thin_open / _step / _zone / _close; round 6):
    local mask uint8 (Zl, Y, X) device tensor (own slices + halo), the own selected patches (local linear
    indices, positions in the global selected list, local bit table), local params with origin_z = first
    slice.  After the rounds: state (1 = kept), count (voxels covered when kept), cleared (interior ones)."""
    ENTRY, TIMER = "thin", "thin_cover"

    def __init__(self, mask, lin_local, index_global, bits, P, global_z):
        torch = _torch()
        super().__init__(mask, lin_local, bits, P, global_z, lib().ppp_thin_shard_workspace_bytes(ctypes.byref(P)))
        self.index = index_global.to(torch.int32).contiguous()
        dev = mask.device
        self.state = torch.empty(max(self.n, 1), dtype=torch.int32, device=dev)
        self.count = torch.empty(max(self.n, 1), dtype=torch.int32, device=dev)
        self.cleared = torch.empty(max(self.n, 1), dtype=torch.int32, device=dev)
        with _timed("thin_cover"):
            check(lib().ppp_thin_open(_dev_ptr(self.mask), _dev_ptr(self.lin), _dev_ptr(self.index), self.n,
                                      _dev_ptr(self.state), _dev_ptr(self.count), _dev_ptr(self.cleared),
                                      _dev_ptr(self.work), ctypes.byref(self.P), _stream()))

    def _step_lists(self):
        return _dev_ptr(self.state), _dev_ptr(self.count), _dev_ptr(self.cleared)


def synth_pred(labels, P, seed=0, hi=0.95, lo=0.05, noise=0.04, f16=True, voxel_offset=0):
    """Procedural prediction volume on the device (bench / tests).  voxel_offset: linear index
    of local voxel 0 in the global volume when `labels` is a z-slab of a larger volume."""
    torch = _torch()
    C = P.pz * P.py * P.px
    pred = torch.empty((C,) + P.shape, dtype=torch.float16 if f16 else torch.float32,
                       device=labels.device)
    check(lib().ppp_synth_pred(_dev_ptr(labels), _dev_ptr(pred), F16 if f16 else F32,
                               int(seed) & 0xFFFFFFFF, hi, lo, noise, int(voxel_offset),
                               ctypes.byref(P), _stream()))
    return pred


def decode_tail(x, w1, b1, w2, b2, w3, b3, dst, pred, patchshape):
    """ppp_decode_tail: x float32 [n, 64, 4, 4, 4] (decoder features), dst int64 [n] voxel indices,
    pred (C, ...) float16 / float32 device block -- written in place at pred[:, dst].  The kernel
    trusts every extent it is given, so the arguments are checked here first (shapes, dtypes and
    devices only: no device synchronisation; the VALUES of dst, each in [0, voxels of pred), stay
    the caller's promise): a mismatch raises ValueError before the library is touched."""
    torch = _torch()
    patchshape = tuple(int(p) for p in patchshape)
    if x.dim() < 1 or pred.dim() < 1:
        raise ValueError("decode_tail: x and pred need a leading batch / channel dimension")
    n = int(x.shape[0])
    if patchshape == (7, 7, 7) and tuple(x.shape[1:]) != (64, 4, 4, 4):
        raise ValueError("decode_tail: 7^3 patches are decoded from features (n, 64, 4, 4, 4), got %s" %
                         (tuple(x.shape),))
    if int(dst.numel()) != n:
        raise ValueError("decode_tail: %d destination indices for %d patches" % (int(dst.numel()), n))
    if dst.is_floating_point() or dst.is_complex() or dst.dtype == torch.bool:
        raise ValueError("decode_tail: dst must hold integer voxel indices, got %s" % dst.dtype)
    if pred.dtype not in (torch.float16, torch.float32):
        raise ValueError("decode_tail: pred must be float16 or float32, got %s" % pred.dtype)
    if not pred.is_contiguous():
        raise ValueError("decode_tail: pred must be contiguous (it is written through its base pointer)")
    if int(pred.shape[0]) != int(np.prod(patchshape)):
        raise ValueError("decode_tail: pred has %d channels, patches of %s have %d" %
                         (int(pred.shape[0]), patchshape, int(np.prod(patchshape))))
    for name, w, count in (("w1", w1, int(x.shape[1]) * 27 if x.dim() > 1 else 27), ("w2", w2, 27), ("w3", w3, 27)):
        if int(w.numel()) != count:
            raise ValueError("decode_tail: %s has %d elements, expected %d" % (name, int(w.numel()), count))
    if len({t.device for t in (x, dst, pred, w1, w2, w3)}) != 1:
        raise ValueError("decode_tail: x, dst, pred and the weights must be on one device, got %s" %
                         sorted({str(t.device) for t in (x, dst, pred, w1, w2, w3)}))
    if n == 0:
        return pred
    P = Params()
    P.abi_version = ABI_VERSION
    vol = [int(v) for v in pred.shape[1:]]
    while len(vol) < 3:
        vol = [1] + vol
    P.Z, P.Y, P.X = vol
    P.pz, P.py, P.px = patchshape
    P.th = P.thi = 0.5
    P.bg_rule, P.value_rule = BG_LESS_THAN_TH, VAL_COUNT
    P.cons_box = Box(0, 0, 0, P.Z, P.Y, P.X)
    f32 = lambda t: t.detach().to(torch.float32).contiguous()
    x, w1, w2, w3 = f32(x), f32(w1).reshape(-1), f32(w2).reshape(-1), f32(w3).reshape(-1)
    check(lib().ppp_decode_tail(_dev_ptr(x), n, int(x.shape[1]), int(x.shape[2]), _dev_ptr(w1), float(b1),
                                _dev_ptr(w2), float(b2), _dev_ptr(w3), float(b3),
                                _dev_ptr(dst.to(torch.int64).contiguous()), _dev_ptr(pred),
                                pred_dtype_code(pred), ctypes.byref(P), _stream()))
    return pred


def decode_tail_rows(x, w1, b1, w2, b2, w3, b3, dst, rows):
    """ppp_decode_tail_rows: decode_tail with patch k written as the row rows[dst[k]] of a
    contiguous [n_rows, 343] float16 / float32 table (the VALUES of dst, each in [0, n_rows), stay
    the caller's promise)."""
    torch = _torch()
    n = int(x.shape[0])
    if tuple(x.shape[1:]) != (64, 4, 4, 4):
        raise ValueError("decode_tail_rows: features must be (n, 64, 4, 4, 4), got %s" % (tuple(x.shape),))
    if int(dst.numel()) != n or dst.dtype != torch.int64:
        raise ValueError("decode_tail_rows: dst must hold %d int64 row numbers" % n)
    if rows.dim() != 2 or int(rows.shape[1]) != 343 or not rows.is_contiguous() or \
            rows.dtype not in (torch.float16, torch.float32):
        raise ValueError("decode_tail_rows: rows must be a contiguous [n_rows, 343] float16 / float32 table")
    for name, w, count in (("w1", w1, 64 * 27), ("w2", w2, 27), ("w3", w3, 27)):
        if int(w.numel()) != count:
            raise ValueError("decode_tail_rows: %s has %d elements, expected %d" % (name, int(w.numel()), count))
    if len({t.device for t in (x, dst, rows, w1, w2, w3)}) != 1:
        raise ValueError("decode_tail_rows: x, dst, rows and the weights must be on one device")
    if n == 0:
        return rows
    f32 = lambda t: t.detach().to(torch.float32).contiguous()
    x, w1, w2, w3 = f32(x), f32(w1).reshape(-1), f32(w2).reshape(-1), f32(w3).reshape(-1)
    check(lib().ppp_decode_tail_rows(_dev_ptr(x), n, 64, 4, _dev_ptr(w1), float(b1), _dev_ptr(w2), float(b2),
                                     _dev_ptr(w3), float(b3), _dev_ptr(dst.contiguous()), _dev_ptr(rows),
                                     pred_dtype_code(rows), 343, _stream()))
    return rows


def rows_index_build(mask):
    """ppp_rows_index_build: mask (Z, Y, X) device tensor, non-zero = has a row.  Returns (index,
    n_rows): the device index (uint8 tensor, layout private to the library) that gives any voxel's
    row number in O(1), and the number of rows.  Synchronises."""
    torch = _torch()
    if mask.dim() != 3 or not mask.is_cuda:
        raise ValueError("rows_index_build: mask must be a (Z, Y, X) device tensor")
    Z, Y, X = [int(v) for v in mask.shape]
    index = _workspace(lib().ppp_rows_index_bytes(Z, Y, X), mask.device)
    m = (mask != 0).to(torch.uint8).contiguous() if mask.dtype != torch.uint8 else mask.contiguous()
    n = ctypes.c_int64(0)
    check(lib().ppp_rows_index_build(_dev_ptr(m), Z, Y, X, _dev_ptr(index), ctypes.byref(n), _stream()))
    return index, int(n.value)


def _rows_args(who, rows, index, shape, box, pred_box):
    Z, Y, X = [int(v) for v in shape]
    z0, z1, y0, y1, x0, x1 = [int(v) for v in box]
    if rows.dim() != 2 or not rows.is_contiguous() or not pred_box.is_contiguous():
        raise ValueError("%s: rows must be a contiguous [n_rows, C] table, the box contiguous" % who)
    C = int(rows.shape[1])
    if tuple(int(v) for v in pred_box.shape) != (C, z1 - z0, y1 - y0, x1 - x0) or pred_box.dtype != rows.dtype:
        raise ValueError("%s: the box tensor must be (%d, %d, %d, %d) of %s, got %s of %s" %
                         (who, C, z1 - z0, y1 - y0, x1 - x0, rows.dtype, tuple(pred_box.shape), pred_box.dtype))
    if int(index.numel()) != int(lib().ppp_rows_index_bytes(Z, Y, X)):
        raise ValueError("%s: the index was not built for a volume of %s" % (who, (Z, Y, X)))
    if len({rows.device, index.device, pred_box.device}) != 1:
        raise ValueError("%s: rows, index and box must be on one device" % who)
    return C, (Z, Y, X), Box(z0, y0, x0, z1, y1, x1)


def rows_expand(rows, index, shape, box, out=None):
    """ppp_rows_expand: the dense (C, bz, by, bx) prediction of `box` = (z0, z1, y0, y1, x0, x1) from the
    rows table [n_rows, C] (float32 / float16 / bfloat16, moved as bits) of the mask `index` was built
    from: a mask voxel gets its row, every other voxel zeros -- all written by the kernel.  The
    number of rows must be the index's (the caller's promise, as CompactPrediction keeps it)."""
    torch = _torch()
    z0, z1, y0, y1, x0, x1 = [int(v) for v in box]
    if out is None:
        out = torch.empty((int(rows.shape[1]), z1 - z0, y1 - y0, x1 - x0), dtype=rows.dtype, device=rows.device)
    C, (Z, Y, X), b = _rows_args("rows_expand", rows, index, shape, box, out)
    with _timed("rows_expand"):
        check(lib().ppp_rows_expand(_dev_ptr(rows), pred_dtype_code(rows), C, _dev_ptr(index), Z, Y, X, ctypes.byref(b),
                                    _dev_ptr(out), _stream()))
    return out


def rows_compact(pred_box, box, index, shape, rows):
    """ppp_rows_compact: the rows of the mask voxels of `box` written from its dense prediction
    (C, bz, by, bx); every other row of `rows` stays as it is."""
    C, (Z, Y, X), b = _rows_args("rows_compact", rows, index, shape, box, pred_box)
    check(lib().ppp_rows_compact(_dev_ptr(pred_box), pred_dtype_code(rows), C, ctypes.byref(b), _dev_ptr(index), Z, Y, X,
                                 _dev_ptr(rows), _stream()))
    return rows


def synth_pred_box(labels, label_box, box, gshape, patchshape, flags, seed=0, hi=0.95, lo=0.05,
                   noise=0.04, f16=True):
    """ppp_synth_pred for a box (z0, z1, y0, y1, x0, x1) of a volume of shape gshape.  labels:
    int32 device tensor over label_box (z0, z1, y0, y1, x0, x1), the box grown by the patch radius
    (clipped).  Returns (C, bz, by, bx)."""
    torch = _torch()
    z0, z1, y0, y1, x0, x1 = [int(v) for v in box]
    P = make_params((z1 - z0, y1 - y0, x1 - x0), patchshape, origin=(z0, y0, x0), **flags)
    C = P.pz * P.py * P.px
    pred = torch.empty((C,) + P.shape, dtype=torch.float16 if f16 else torch.float32, device=labels.device)
    lb = np.ascontiguousarray([label_box[0], label_box[2], label_box[4], label_box[1], label_box[3],
                               label_box[5]], dtype=np.int32)
    gd = np.ascontiguousarray(gshape, dtype=np.int32)
    check(lib().ppp_synth_pred_box(_dev_ptr(labels.contiguous()), _np_ptr(lb), _dev_ptr(pred),
                                   F16 if f16 else F32, int(seed) & 0xFFFFFFFF, hi, lo, noise,
                                   _np_ptr(gd), ctypes.byref(P), _stream()))
    return pred


# ----------------------------------------------------------------------------------------
# host stages (NumPy arrays in, NumPy arrays out)
# ----------------------------------------------------------------------------------------
def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _i32(seq):
    return np.ascontiguousarray(np.array(seq, dtype=np.int32))


def host_mws(pairs, aff, shape):
    """Mutex watershed on the patch graph (ppp_host_mws).  pairs uint32 [n, 6], aff float32 [n]
    (host arrays).  Returns (nodes int32 [k, 3], labels int64 [k], n_labels): the nodes that
    ended up in a component and their instance ids; n_labels = number of ids issued."""
    pairs = np.ascontiguousarray(np.asarray(pairs).reshape(-1, 6), dtype=np.uint32)
    aff = np.ascontiguousarray(aff, dtype=np.float32)
    n = len(aff)
    cap = min(2 * n, int(np.prod(shape))) + 1
    nodes = np.empty((cap, 3), dtype=np.int32)
    labels = np.empty((cap,), dtype=np.int32)
    n_labels = ctypes.c_int64(0)
    k = int(lib().ppp_host_mws(_np_ptr(pairs), _np_ptr(aff), n, _np_ptr(_i32(shape)), _np_ptr(nodes),
                               _np_ptr(labels), cap, ctypes.byref(n_labels)))
    if k < 0:
        raise RuntimeError("libppp_mi355x: ppp_host_mws: %s" %
                           ("node capacity too small" if k == -1 else "coordinate outside the volume"))
    keep = labels[:k] > 0
    return nodes[:k][keep], labels[:k][keep].astype(np.int64), int(n_labels.value)


def mws_labels_device(rows, aff, nodes, P):
    """Mutex watershed of the patch graph (graph_mws.py:7-85) with everything but the inherently
    sequential loop on the device: ppp_mws_edges filters the rows with aff != 0, puts them in
    networkx's edge order and sorts them stably by |aff| (descending); the edge list (8 bytes per
    edge) crosses to the host once and ppp_host_mws_sorted walks it.
    rows int32 [N, 6] / aff float32 [N] device tensors without repeated node pairs, nodes int32
    [K, 3] device.  Returns (labels int32 [K] device tensor, 0 = no component; ids issued)."""
    torch = _torch()
    n, k = int(rows.shape[0]), int(nodes.shape[0])
    labels = np.zeros((k,), dtype=np.int32)
    if n == 0 or k == 0:
        return torch.from_numpy(labels).to(nodes.device), 0
    eu_h, ev_h = mws_edges_device(rows, aff, nodes, P)
    ne = len(eu_h)
    with host_timer("s6b_mws_loop"):
        issued = int(lib().ppp_host_mws_sorted(_np_ptr(eu_h), _np_ptr(ev_h), ne, k, _np_ptr(labels)))
    note("mws_edges", ne)
    return torch.from_numpy(labels).to(nodes.device), issued


def mws_edges_device(rows, aff, nodes, P):
    """The edge list of the mutex watershed made on the device (ppp_mws_edges) and copied to the
    host: (eu, ev) int32 [n_edges] node numbers in the order the loop visits them, bit 31 of ev =
    attractive.  rows / aff / nodes: device tensors as for mws_labels_device (n, k > 0)."""
    torch = _torch()
    n, k = int(rows.shape[0]), int(nodes.shape[0])
    work = _workspace(lib().ppp_mws_edges_workspace_bytes(n, k, ctypes.byref(P)), rows.device)
    eu = torch.empty((n,), dtype=torch.int32, device=rows.device)
    ev = torch.empty((n,), dtype=torch.int32, device=rows.device)
    n_edges = ctypes.c_int64(0)
    with host_timer("s6a_mws_edges"):
        with _timed("mws_edges"):
            check(lib().ppp_mws_edges(_dev_ptr(rows), _dev_ptr(aff), n, _dev_ptr(nodes.contiguous()), k,
                                      _dev_ptr(eu), _dev_ptr(ev), ctypes.byref(n_edges), _dev_ptr(work),
                                      ctypes.byref(P), _stream()))
        ne = int(n_edges.value)
        eu_h = eu[:ne].cpu().numpy()
        ev_h = ev[:ne].cpu().numpy()
    return eu_h, ev_h


def host_rank_order(score, foreground, patchshape):
    score = np.ascontiguousarray(score, dtype=np.float32)
    fg = np.ascontiguousarray(foreground).astype(np.uint8)
    out = np.empty(score.size, dtype=np.int64)
    vol, ps = _i32(score.shape), _i32(patchshape)
    n = lib().ppp_host_rank_order(_np_ptr(score), _np_ptr(fg), _np_ptr(vol), _np_ptr(ps),
                                  _np_ptr(out))
    return out[:n].copy()


def padded_mask(mask):
    """uint8 0/1 copy of a (Z,Y,X) mask whose buffer has 8 spare bytes at the end, as the native
    cover functions require; returns (volume view, owner)."""
    flat = np.zeros(mask.size + 8, dtype=np.uint8)
    flat[:mask.size] = (np.asarray(mask).reshape(-1) != 0)
    return flat[:mask.size].reshape(mask.shape), flat


def rank_order_device(score, foreground, patchshape, to_host=True):
    """all_patches + rank_patches_by_score on the device (ppp_rank_order): interior foreground
    voxels in raster order, stably sorted by score descending (vote_instances.py:276,286-287,
    ranked_patches.py:21-30).  score: device float32 (Z,Y,X); foreground: host bool.
    Returns (lin int64, scores float32), NumPy arrays or (to_host=False) device tensors."""
    torch = _torch()
    Z, Y, X = [int(v) for v in score.shape]
    P = Params()
    P.abi_version = ABI_VERSION
    P.Z, P.Y, P.X = Z, Y, X
    P.pz, P.py, P.px = [int(p) for p in patchshape]
    P.th = P.thi = 0.5
    P.bg_rule, P.value_rule = BG_LESS_THAN_TH, VAL_COUNT
    P.cons_box = Box(0, 0, 0, Z, Y, X)
    if torch.is_tensor(foreground):
        fg = foreground.to(score.device)
        fg = (fg if fg.dtype == torch.uint8 else (fg != 0).to(torch.uint8)).contiguous().reshape(-1)
    else:
        fg = torch.from_numpy(np.ascontiguousarray(np.asarray(foreground) != 0).astype(np.uint8)
                              ).to(score.device).reshape(-1)
    V = Z * Y * X
    work = _workspace(lib().ppp_rank_order_workspace_bytes(ctypes.byref(P)), score.device)
    # the ranked list has at most one entry per interior voxel
    cap = max(1, (Z - 2 * (P.pz // 2)) * (Y - 2 * (P.py // 2)) * (X - 2 * (P.px // 2)))
    lin = torch.empty((min(cap, V),), dtype=torch.int64, device=score.device)
    sc = torch.empty((min(cap, V),), dtype=torch.float32, device=score.device)
    count = ctypes.c_int64(0)
    with _timed("rank_order"):
        check(lib().ppp_rank_order(_dev_ptr(score.contiguous()), _dev_ptr(fg), _dev_ptr(lin), _dev_ptr(sc),
                                   ctypes.byref(count), _dev_ptr(work), ctypes.byref(P), _stream()))
    n = int(count.value)
    lin, sc = lin[:n], sc[:n]
    if to_host:
        return lin.cpu().numpy(), sc.cpu().numpy()
    return lin, sc


# ----------------------------------------------------------------------------------------
# whole-volume post-steps of the label driver (ppp_postprocess.hip; callers: postprocess.py)
# ----------------------------------------------------------------------------------------
def post_compact_ids(ids, max_id, compsize=-1, relabel=True, start=1):
    """ppp_post_compact_ids, IN PLACE on a contiguous device tensor of 32-bit ids (int32 storage is
    read as uint32): ids of at most `compsize` voxels become 0, and with `relabel` the surviving
    ones become start, start + 1, ... in ascending order of the old id.  `max_id` bounds the ids of
    the map.  Returns the number of surviving ids."""
    assert ids.element_size() == 4 and not ids.is_floating_point(), "post_compact_ids needs 32-bit ids"
    n = int(ids.numel())
    work = _workspace(lib().ppp_post_compact_ids_workspace_bytes(n, int(max_id)), ids.device)
    kept = ctypes.c_int64(0)
    with _timed("post_compact_ids"):
        check(lib().ppp_post_compact_ids(_dev_ptr(ids), n, int(max_id), int(compsize), 1 if relabel else 0,
                                         int(start) & 0xFFFFFFFF, ctypes.byref(kept), _dev_ptr(work), _stream()))
    return int(kept.value)


def post_dilate(ids):
    """ppp_post_dilate on a contiguous (Z, Y, X) device tensor of 32-bit ids: the ascending in-place
    dilation loop of the reference in closed form.  Returns (new tensor, rounds)."""
    assert ids.element_size() == 4 and not ids.is_floating_point() and ids.dim() == 3, "post_dilate needs 32-bit ids, 3-d"
    Z, Y, X = [int(v) for v in ids.shape]
    work = _workspace(lib().ppp_post_dilate_workspace_bytes(Z, Y, X), ids.device)
    out = _torch().empty_like(ids)
    rounds = ctypes.c_int32(0)
    with _timed("post_dilate"):
        check(lib().ppp_post_dilate(_dev_ptr(ids), _dev_ptr(out), Z, Y, X, ctypes.byref(rounds), _dev_ptr(work),
                                    _stream()))
    return out, int(rounds.value)


def post_clean_mask(mask, structure_bits, size):
    """ppp_post_clean_mask on a contiguous (Z, Y, X) uint8 device tensor: the mask without its connected
    components (connectivity: the 27 structure bits) of at most `size` voxels.  Returns (uint8 tensor,
    components found, components kept)."""
    torch = _torch()
    assert mask.dtype == torch.uint8 and mask.dim() == 3, "post_clean_mask needs a uint8 (Z, Y, X) mask"
    Z, Y, X = [int(v) for v in mask.shape]
    work = _workspace(lib().ppp_post_clean_mask_workspace_bytes(Z, Y, X), mask.device)
    out = torch.empty_like(mask)
    found, kept = ctypes.c_int64(0), ctypes.c_int64(0)
    with _timed("post_clean_mask"):
        check(lib().ppp_post_clean_mask(_dev_ptr(mask), _dev_ptr(out), Z, Y, X, int(structure_bits), int(size),
                                        ctypes.byref(found), ctypes.byref(kept), _dev_ptr(work), _stream()))
    return out, int(found.value), int(kept.value)


def post_edt_sq(feature, cap=0):
    """ppp_post_edt_sq on a contiguous (Z, Y, X) uint8 device tensor: the exact squared Euclidean distance
    of every voxel to the nearest voxel with feature != 0, cut at `cap` (0: no cap; 0xFFFFFFFF where
    the volume holds no feature then).  Returns an int32 tensor whose bits are the uint32 values."""
    torch = _torch()
    assert feature.dtype == torch.uint8 and feature.dim() == 3, "post_edt_sq needs a uint8 (Z, Y, X) volume"
    assert 0 <= int(cap) <= 0xFFFFFFFF, "cap is an unsigned 32-bit value"
    Z, Y, X = [int(v) for v in feature.shape]
    work = _workspace(lib().ppp_post_edt_sq_workspace_bytes(Z, Y, X), feature.device)
    out = torch.empty((Z, Y, X), dtype=torch.int32, device=feature.device)
    with _timed("post_edt_sq"):
        check(lib().ppp_post_edt_sq(_dev_ptr(feature), _dev_ptr(out), Z, Y, X, int(cap), _dev_ptr(work), _stream()))
    return out


def post_fg_filter(mask, compsize, min_d2, want_instances=False):
    """ppp_post_fg_filter on a contiguous (Z, Y, X) uint8 device tensor: the mask without its 26-connected
    components of at most `compsize` voxels that have no voxel at a squared distance < `min_d2` from a
    larger component (min_d2 = 0: all of them go).  Returns (uint8 tensor, int32 tensor with the bits of the
    uint32 component numbers -- scipy.ndimage.label's of the result -- or None, (found, small, removed,
    kept))."""
    torch = _torch()
    assert mask.dtype == torch.uint8 and mask.dim() == 3, "post_fg_filter needs a uint8 (Z, Y, X) mask"
    assert 0 <= int(min_d2) <= 0xFFFFFFFF, "min_d2 is an unsigned 32-bit value"
    Z, Y, X = [int(v) for v in mask.shape]
    work = _workspace(lib().ppp_post_fg_filter_workspace_bytes(Z, Y, X), mask.device)
    fg = torch.empty_like(mask)
    inst = torch.empty((Z, Y, X), dtype=torch.int32, device=mask.device) if want_instances else None
    stats = (ctypes.c_int64 * 4)()
    with _timed("post_fg_filter"):
        check(lib().ppp_post_fg_filter(_dev_ptr(mask), _dev_ptr(fg), None if inst is None else _dev_ptr(inst), Z, Y, X,
                                       int(compsize), int(min_d2), stats, _dev_ptr(work), _stream()))
    return fg, inst, tuple(int(v) for v in stats)


def eval_patch(pred_tile, labels, patchshape, z0, thresholds, counts, want_maps=False):
    """ppp_eval_patch on the slices z0 .. z0 + tz of a prediction: `pred_tile` a contiguous (C, tz, Y, X) device
    tensor (float32 / float16 / bfloat16), `labels` the contiguous int32 (L, Z, Y, X) device tensor of the WHOLE
    volume (values >= 0), `thresholds` floats already rounded to the element type, `counts` an int64 device
    tensor of 1 + 2 T entries that is ADDED to (num_gt, then num_pred and tp per threshold).  Returns
    (inter, union), int32 (T, tz, Y, X) device tensors, or (None, None) without `want_maps`.  Does not
    synchronise."""
    torch = _torch()
    assert pred_tile.dim() == 4 and labels.dim() == 4 and labels.dtype == torch.int32, \
        "eval_patch needs a (C, tz, Y, X) prediction and int32 (L, Z, Y, X) labels"
    C, tz, Y, X = [int(v) for v in pred_tile.shape]
    L, Z = int(labels.shape[0]), int(labels.shape[1])
    assert tuple(labels.shape[2:]) == (Y, X), "prediction and labels differ in (Y, X)"
    T = len(thresholds)
    assert counts.dtype == torch.int64 and counts.numel() == 1 + 2 * T, "counts holds 1 + 2 T int64 entries"
    vol, patch = (ctypes.c_int32 * 3)(Z, Y, X), (ctypes.c_int32 * 3)(*[int(p) for p in patchshape])
    th = (ctypes.c_float * max(T, 1))(*[float(t) for t in thresholds])
    work = _workspace(lib().ppp_eval_patch_workspace_bytes(vol, tz), pred_tile.device)
    inter = union = None
    if want_maps:
        inter = torch.empty((T, tz, Y, X), dtype=torch.int32, device=pred_tile.device)
        union = torch.empty_like(inter)
    with _timed("eval_patch"):
        check(lib().ppp_eval_patch(_dev_ptr(pred_tile), pred_dtype_code(pred_tile), C, _dev_ptr(labels), L, vol, patch,
                                   int(z0), tz, th, T, _dev_ptr(counts), _dev_ptr(inter), _dev_ptr(union),
                                   _dev_ptr(work), _stream()))
    return inter, union


def patch_mosaic(pred_tile, patchshape, selected=None, out=None):
    """ppp_patch_mosaic on one z-tile: `pred_tile` a contiguous (C, tz, Y, X) device tensor (float32 / float16 /
    bfloat16, C = pz py px), `selected` None or a contiguous uint8 (S, tz, Y, X) device tensor with S = 1 or 3
    (pz = 1 only).  Returns the mosaic, (tz, Y py, X px) of the same dtype, or (3, tz, Y py, X px) with
    `selected`; `out`, when given, is that tensor and EVERY element of it is written.  Does not synchronise."""
    torch = _torch()
    assert pred_tile.dim() == 4, "patch_mosaic needs a (C, tz, Y, X) prediction"
    C, tz, Y, X = [int(v) for v in pred_tile.shape]
    pz, py, px = [int(p) for p in patchshape]
    S = 0
    if selected is not None:
        assert selected.dtype == torch.uint8 and selected.dim() == 4 and tuple(selected.shape[1:]) == (tz, Y, X), \
            "selected is a uint8 (S, tz, Y, X) tensor"
        S = int(selected.shape[0])
    shape = (tz, Y * py, X * px) if S == 0 else (3, tz, Y * py, X * px)
    if out is None:
        out = torch.empty(shape, dtype=pred_tile.dtype, device=pred_tile.device)
    assert tuple(out.shape) == shape and out.dtype == pred_tile.dtype, "out must be %s of %s" % (shape, pred_tile.dtype)
    patch = (ctypes.c_int32 * 3)(pz, py, px)
    with _timed("patch_mosaic"):
        check(lib().ppp_patch_mosaic(_dev_ptr(pred_tile), pred_dtype_code(pred_tile), C, _dev_ptr(selected), S,
                                     _dev_ptr(out), tz, Y, X, patch, _stream()))
    return out


def _out_dtype_code(dtype):
    torch = _torch()
    codes = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}
    assert dtype in codes, "out_dtype must be float32, float16 or bfloat16, got %s" % dtype
    return codes[dtype]


def nhood_halo(nhood):
    """The per-axis minimum and maximum of a device `nhood` (E, 3), the `halo` of ppp_gt_affs_dense: computed
    ONCE per tensor (one device -> host read, kept on the tensor with the version it was made from)."""
    have = getattr(nhood, "_ppp_halo", None)
    if have is None or have[0] != nhood._version:
        lo, hi = nhood.amin(dim=0).tolist(), nhood.amax(dim=0).tolist()
        have = (nhood._version, (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]))
        nhood._ppp_halo = have
    return have[1]


def gt_affs_dense_plan(B, L, vol, E, halo, box, out_dtype=None, single=False):
    """ppp_gt_affs_dense_plan: (tile z, y, x, staged in LDS, edge ranges per tile) of a call with these sizes."""
    torch = _torch()
    plan = (ctypes.c_int32 * 5)()
    check(lib().ppp_gt_affs_dense_plan(int(B), int(L), (ctypes.c_int32 * 3)(*[int(v) for v in vol]), int(E),
                                       (ctypes.c_int32 * 6)(*[int(v) for v in halo]),
                                       (ctypes.c_int32 * 6)(*[int(v) for v in box]),
                                       _out_dtype_code(out_dtype or torch.float32), 1 if single else 0, plan))
    return tuple(int(v) for v in plan)


def gt_affs_dense(labels, nhood, box=None, out=None, out_dtype=None, single=False):
    """ppp_gt_affs_dense: the ground-truth affinities of `labels`, a contiguous int32 device tensor (B, L, Z, Y, X)
    -- (B, Z, Y, X) with `single`, the one-channel form whose value is the id squared (float32 only) -- for the
    offsets `nhood`, a contiguous int32 device tensor (E, 3).  `box` = (z0, z1, y0, y1, x0, x1): the voxels
    that are written (default: all).  Returns (B, E, z1-z0, y1-y0, x1-x0) of `out_dtype` (float32 / float16 /
    bfloat16, default float32); `out`, when given, is that tensor and EVERY element of it is written.  Does not
    synchronise (the halo of a `nhood` tensor is read back once, `nhood_halo`)."""
    torch = _torch()
    assert labels.dtype == torch.int32 and labels.dim() == (4 if single else 5), \
        "gt_affs_dense needs int32 labels (B, L, Z, Y, X), or (B, Z, Y, X) with single"
    assert nhood.dtype == torch.int32 and nhood.dim() == 2 and nhood.shape[1] == 3, "nhood is an int32 (E, 3) tensor"
    B, L = int(labels.shape[0]), (1 if single else int(labels.shape[1]))
    Z, Y, X = [int(v) for v in labels.shape[-3:]]
    E = int(nhood.shape[0])
    if box is None:
        box = (0, Z, 0, Y, 0, X)
    box = [int(v) for v in box]
    assert len(box) == 6, "box = (z0, z1, y0, y1, x0, x1)"
    if out_dtype is None:
        out_dtype = torch.float32 if out is None else out.dtype
    assert not single or out_dtype == torch.float32, "the one-channel form (id squared) is float32 only"
    shape = (B, E, box[1] - box[0], box[3] - box[2], box[5] - box[4])
    if out is None:
        assert min(shape) > 0, "box %s is empty" % (box,)
        out = torch.empty(shape, dtype=out_dtype, device=labels.device)
    assert tuple(out.shape) == shape and out.dtype == out_dtype, "out must be %s of %s" % (shape, out_dtype)
    halo = nhood_halo(nhood) if E > 0 else (0,) * 6
    with _timed("gt_affs_dense"):
        check(lib().ppp_gt_affs_dense(_dev_ptr(labels), B, L, (ctypes.c_int32 * 3)(Z, Y, X), _dev_ptr(nhood), E,
                                      (ctypes.c_int32 * 6)(*halo), (ctypes.c_int32 * 6)(*box), _dev_ptr(out),
                                      _out_dtype_code(out_dtype), 1 if single else 0, _stream()))
    return out


def gt_affs_samples(labels, samples, nhood, ps, ctr, out=None, out_dtype=None):
    """ppp_gt_affs_samples: `labels` a contiguous int32 device tensor (B, L, Z, Y, X), `samples` int32 (N, 4) rows
    (b, z, y, x), the corners of patches of `ps` = (pz, py, px) voxels, `nhood` int32 (E, 3) indices into the
    patch, `ctr` the centre's index.  Returns (N, E) of `out_dtype` (default float32), or `out`.  Voxels outside
    the volume read as 0; N = 0 gives an empty tensor.  Does not synchronise."""
    torch = _torch()
    assert labels.dtype == torch.int32 and labels.dim() == 5, "gt_affs_samples needs int32 labels (B, L, Z, Y, X)"
    assert samples.dtype == torch.int32 and samples.dim() == 2 and samples.shape[1] == 4, \
        "samples is an int32 (N, 4) tensor of rows (b, z, y, x)"
    assert nhood.dtype == torch.int32 and nhood.dim() == 2 and nhood.shape[1] == 3, "nhood is an int32 (E, 3) tensor"
    B, L, Z, Y, X = [int(v) for v in labels.shape]
    N, E = int(samples.shape[0]), int(nhood.shape[0])
    if out_dtype is None:
        out_dtype = torch.float32 if out is None else out.dtype
    if out is None:
        out = torch.empty((N, E), dtype=out_dtype, device=labels.device)
    assert tuple(out.shape) == (N, E) and out.dtype == out_dtype, "out must be %s of %s" % ((N, E), out_dtype)
    with _timed("gt_affs_samples"):
        check(lib().ppp_gt_affs_samples(_dev_ptr(labels), B, L, (ctypes.c_int32 * 3)(Z, Y, X),
                                        _dev_ptr(samples) if N else None, N, _dev_ptr(nhood), E,
                                        (ctypes.c_int32 * 3)(*[int(p) for p in ps]),
                                        (ctypes.c_int32 * 3)(*[int(c) for c in ctr]), _dev_ptr(out) if N else None,
                                        _out_dtype_code(out_dtype), _stream()))
    return out


def _patch_loss_dense_geometry(logits, labels, nhood, weight, box):
    torch = _torch()
    assert labels.dtype == torch.int32 and labels.dim() == 5, "patch_loss needs int32 labels (B, L, Z, Y, X)"
    assert nhood.dtype == torch.int32 and nhood.dim() == 2 and nhood.shape[1] == 3, "nhood is an int32 (E, 3) tensor"
    B, L, Z, Y, X = [int(v) for v in labels.shape]
    E = int(nhood.shape[0])
    box = [int(v) for v in (box if box is not None else (0, Z, 0, Y, 0, X))]
    assert len(box) == 6, "box = (z0, z1, y0, y1, x0, x1)"
    ext = (box[1] - box[0], box[3] - box[2], box[5] - box[4])
    assert tuple(logits.shape) == (B, E) + ext, "logits must be %s, got %s" % ((B, E) + ext, tuple(logits.shape))
    if weight is not None:
        assert weight.dtype == torch.float32 and tuple(weight.shape) == (B,) + ext, "weight must be float32 %s" % ((B,) + ext,)
    return B, L, (Z, Y, X), E, box


def patch_loss_workspace_bytes(B, L, vol, E, halo=None, box=None, dtype=None, N=0):
    """ppp_patch_loss_workspace_bytes: the dense form with `halo` and `box`, the sampled form (box None) with N."""
    torch = _torch()
    n = lib().ppp_patch_loss_workspace_bytes(int(B), int(L), (ctypes.c_int32 * 3)(*[int(v) for v in vol]), int(E),
                                             (ctypes.c_int32 * 6)(*[int(v) for v in halo]) if halo is not None else None,
                                             (ctypes.c_int32 * 6)(*[int(v) for v in box]) if box is not None else None,
                                             _out_dtype_code(dtype or torch.float32), int(N))
    check(min(int(n), 0))
    return int(n)


def patch_loss_dense_fwd(logits, labels, nhood, weight=None, box=None, num_channels=None, want_counts=False, work=None):
    """ppp_patch_loss_dense_fwd: the masked BCE-with-logits loss of `logits`, a contiguous device tensor
    (B, E, bZ, bY, bX) of float32 / float16 / bfloat16, against the ground-truth affinities of `labels`
    (int32 (B, L, Z, Y, X)) for the offsets `nhood` (int32 (E, 3)) on `box` (default: the volume), which are never
    stored.  `weight`: float32 (B, bZ, bY, bX) >= 0 or None; `num_channels`: the divisor's factor (default E).
    Returns (loss, state, counts): a float32 tensor of 1, the float64 (s, sum w) the backward takes, and the int64
    (x > 0, G, x > 0 and G) counts or None.  `work`: a uint8 tensor of patch_loss_workspace_bytes.  Does not
    synchronise."""
    torch = _torch()
    B, L, vol, E, box = _patch_loss_dense_geometry(logits, labels, nhood, weight, box)
    halo = nhood_halo(nhood)
    code = _out_dtype_code(logits.dtype)
    if work is None:
        work = _workspace(patch_loss_workspace_bytes(B, L, vol, E, halo, box, logits.dtype), logits.device)
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    state = torch.empty(2, dtype=torch.float64, device=logits.device)
    counts = torch.empty(3, dtype=torch.int64, device=logits.device) if want_counts else None
    with _timed("patch_loss_dense_fwd"):
        check(lib().ppp_patch_loss_dense_fwd(_dev_ptr(logits), code, _dev_ptr(labels), B, L, (ctypes.c_int32 * 3)(*vol),
                                             _dev_ptr(nhood), E, (ctypes.c_int32 * 6)(*halo), (ctypes.c_int32 * 6)(*box),
                                             _dev_ptr(weight), float(E if num_channels is None else num_channels),
                                             _dev_ptr(loss), _dev_ptr(state), _dev_ptr(counts), _dev_ptr(work), _stream()))
    return loss, state, counts


def patch_loss_dense_bwd(logits, labels, nhood, state, grad_out, weight=None, box=None, out=None):
    """ppp_patch_loss_dense_bwd: the gradient of patch_loss_dense_fwd's loss with respect to `logits`, times
    `grad_out` (a float32 device tensor of 1), rounded once into the logits' type.  `state` is the forward's.
    Returns a tensor like `logits`, or `out`; EVERY element is written.  Does not synchronise."""
    torch = _torch()
    B, L, vol, E, box = _patch_loss_dense_geometry(logits, labels, nhood, weight, box)
    if out is None:
        out = torch.empty(logits.shape, dtype=logits.dtype, device=logits.device)
    assert tuple(out.shape) == tuple(logits.shape) and out.dtype == logits.dtype, "out must be like the logits"
    assert state.dtype == torch.float64 and state.numel() == 2 and grad_out.dtype == torch.float32 and grad_out.numel() == 1, \
        "state is the forward's float64 (2,), grad_out a float32 tensor of one element"
    with _timed("patch_loss_dense_bwd"):
        check(lib().ppp_patch_loss_dense_bwd(_dev_ptr(logits), _out_dtype_code(logits.dtype), _dev_ptr(labels), B, L,
                                             (ctypes.c_int32 * 3)(*vol), _dev_ptr(nhood), E,
                                             (ctypes.c_int32 * 6)(*nhood_halo(nhood)), (ctypes.c_int32 * 6)(*box),
                                             _dev_ptr(weight), _dev_ptr(state), _dev_ptr(grad_out), _dev_ptr(out), _stream()))
    return out


def _patch_loss_samples_geometry(logits, labels, samples, nhood):
    torch = _torch()
    assert labels.dtype == torch.int32 and labels.dim() == 5, "patch_loss needs int32 labels (B, L, Z, Y, X)"
    assert samples.dtype == torch.int32 and samples.dim() == 2 and samples.shape[1] == 4, \
        "samples is an int32 (N, 4) tensor of rows (b, z, y, x)"
    assert nhood.dtype == torch.int32 and nhood.dim() == 2 and nhood.shape[1] == 3, "nhood is an int32 (E, 3) tensor"
    B, L, Z, Y, X = [int(v) for v in labels.shape]
    N, E = int(samples.shape[0]), int(nhood.shape[0])
    assert tuple(logits.shape) == (N, E), "logits must be %s, got %s" % ((N, E), tuple(logits.shape))
    return B, L, (Z, Y, X), N, E


def patch_loss_samples_fwd(logits, labels, samples, nhood, ps, ctr, work=None):
    """ppp_patch_loss_samples_fwd: the mean BCE-with-logits loss of `logits` (N, E) against the sampled ground-truth
    affinities (the arguments of gt_affs_samples).  Returns (loss, state); N = 0 gives loss 0 and launches
    nothing.  Does not synchronise."""
    torch = _torch()
    B, L, vol, N, E = _patch_loss_samples_geometry(logits, labels, samples, nhood)
    loss = torch.zeros(1, dtype=torch.float32, device=logits.device)
    state = torch.zeros(2, dtype=torch.float64, device=logits.device)
    if work is None and N:
        work = _workspace(patch_loss_workspace_bytes(B, L, vol, E, dtype=logits.dtype, N=N), logits.device)
    with _timed("patch_loss_samples_fwd"):
        check(lib().ppp_patch_loss_samples_fwd(_dev_ptr(logits) if N else None, _out_dtype_code(logits.dtype), _dev_ptr(labels),
                                               B, L, (ctypes.c_int32 * 3)(*vol), _dev_ptr(samples) if N else None, N,
                                               _dev_ptr(nhood), E, (ctypes.c_int32 * 3)(*[int(p) for p in ps]),
                                               (ctypes.c_int32 * 3)(*[int(c) for c in ctr]), _dev_ptr(loss), _dev_ptr(state),
                                               _dev_ptr(work) if N else None, _stream()))
    return loss, state


def patch_loss_samples_bwd(logits, labels, samples, nhood, ps, ctr, state, grad_out, out=None):
    """ppp_patch_loss_samples_bwd: the gradient of patch_loss_samples_fwd's loss times `grad_out` (float32, one
    element, on the device), like `logits`, or `out`.  Does not synchronise."""
    torch = _torch()
    B, L, vol, N, E = _patch_loss_samples_geometry(logits, labels, samples, nhood)
    if out is None:
        out = torch.empty(logits.shape, dtype=logits.dtype, device=logits.device)
    assert tuple(out.shape) == (N, E) and out.dtype == logits.dtype, "out must be like the logits"
    with _timed("patch_loss_samples_bwd"):
        check(lib().ppp_patch_loss_samples_bwd(_dev_ptr(logits) if N else None, _out_dtype_code(logits.dtype), _dev_ptr(labels),
                                               B, L, (ctypes.c_int32 * 3)(*vol), _dev_ptr(samples) if N else None, N,
                                               _dev_ptr(nhood), E, (ctypes.c_int32 * 3)(*[int(p) for p in ps]),
                                               (ctypes.c_int32 * 3)(*[int(c) for c in ctr]), _dev_ptr(state),
                                               _dev_ptr(grad_out), _dev_ptr(out) if N else None, _stream()))
    return out


def host_cover_pass(mask_running, overlap, patchshape, ranked_lin, ranked_score, bits, pix_th,
                    score_threshold, selected, remaining, marked=None):
    """In place on mask_running (uint8), selected (uint8) and -- mark_close_neighboorhood --
    marked (uint8 volume); returns (new `remaining`, stopped-by-score-threshold)."""
    vol, ps = _i32(mask_running.shape), _i32(patchshape)
    rem = ctypes.c_int64(int(remaining))
    stopped = ctypes.c_int32(0)
    thr = float("nan") if score_threshold is None else float(score_threshold)
    lib().ppp_host_cover_pass_marked(_np_ptr(mask_running), _np_ptr(overlap), _np_ptr(vol), _np_ptr(ps),
                                     _np_ptr(ranked_lin), _np_ptr(ranked_score), _np_ptr(bits),
                                     len(ranked_lin), int(pix_th), thr, _np_ptr(selected),
                                     ctypes.byref(rem), ctypes.byref(stopped),
                                     None if marked is None else _np_ptr(marked))
    return rem.value, bool(stopped.value)


def host_thin_cover(mask, patchshape, sel_lin, bits):
    vol, ps = _i32(mask.shape), _i32(patchshape)
    keep = np.zeros(len(sel_lin), dtype=np.uint8)
    lib().ppp_host_thin_cover(_np_ptr(mask), _np_ptr(vol), _np_ptr(ps), _np_ptr(sel_lin),
                              _np_ptr(bits), len(sel_lin), _np_ptr(keep))
    return keep.astype(bool)


def host_skeletonize_3d(mask):
    """3-d thinning of a (Z, Y, X) (or (Y, X)) mask: bool array of the skeleton
    (ppp_host_skeletonize_3d; Lee / Kashyap / Chu 1994, what skimage's skeletonize_3d implements)."""
    m = np.ascontiguousarray(np.asarray(mask) != 0).astype(np.uint8)
    shape = m.shape
    m3 = m.reshape((1,) * (3 - m.ndim) + shape)
    out = np.empty_like(m3)
    if lib().ppp_host_skeletonize_3d(_np_ptr(m3), _np_ptr(_i32(m3.shape)), _np_ptr(out)) < 0:
        raise RuntimeError("libppp_mi355x: ppp_host_skeletonize_3d: bad arguments")
    return out.reshape(shape).astype(bool)


def skeletonize_3d(mask):
    """ppp_skeletonize_3d: the thinning of host_skeletonize_3d on the device, the same result voxel for
    voxel.  `mask` is a (Z, Y, X) or (Y, X) NumPy array or device tensor, 0 / non-zero; the bool result
    is of the same kind and shape.  NOTES["skeleton_stats"] = (passes, sub-iterations, rounds)."""
    torch = _torch()
    is_tensor = torch.is_tensor(mask)
    if not torch.cuda.is_available():
        raise RuntimeError("libppp_mi355x: ppp_skeletonize_3d: no HIP device available (this library has no CPU path)")
    if is_tensor:
        assert mask.is_cuda, "skeletonize_3d takes a NumPy array or a DEVICE tensor"
        m = (mask != 0).to(torch.uint8).contiguous()
    else:
        m = torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0).astype(np.uint8)).cuda()
    shape = tuple(m.shape)
    assert 2 <= len(shape) <= 3, "skeletonize_3d needs a (Z, Y, X) or (Y, X) mask"
    Z, Y, X = (1,) * (3 - len(shape)) + shape
    if Z * Y * X == 0:
        out = m
    else:
        work = _workspace(lib().ppp_skeletonize_3d_workspace_bytes(Z, Y, X), m.device)
        kept = ctypes.c_int64(0)
        stats = (ctypes.c_int32 * 3)()
        with _timed("skeletonize_3d"):
            check(lib().ppp_skeletonize_3d(_dev_ptr(m), _dev_ptr(m), Z, Y, X, ctypes.byref(kept), stats,
                                           _dev_ptr(work), _stream()))
        NOTES["skeleton_stats"] = tuple(int(v) for v in stats)
        NOTES["skeleton_kept"] = int(kept.value)
        out = m
    return out.bool() if is_tensor else out.cpu().numpy().astype(bool)


def skeletonize_labels(ids):
    """ppp_skeletonize_labels: the 3-d skeleton of every instance of an id map in ONE device pass.  For
    every id L the voxels that keep L are host_skeletonize_3d(ids == L); every other voxel is 0.  `ids` is a
    (Z, Y, X) or (Y, X) NumPy array or device tensor of uint16 / uint32 / int32 ids (0: background; only
    equality of the 32 bits is used); the result is of the same kind, dtype and shape, the input is left
    as it was.  Parity with scikit-image's skeletonize_3d is unpinned, as for skeletonize_3d.
    NOTES["skeleton_stats"] = (passes, sub-iterations, rounds), NOTES["skeleton_kept"] = voxels kept."""
    torch = _torch()
    is_tensor = torch.is_tensor(ids)
    if not torch.cuda.is_available():
        raise RuntimeError("libppp_mi355x: ppp_skeletonize_labels: no HIP device available (this library has no CPU path)")
    if is_tensor:
        assert ids.is_cuda, "skeletonize_labels takes a NumPy array or a DEVICE tensor"
        name = str(ids.dtype).replace("torch.", "")
        assert name in ("uint16", "uint32", "int32"), "skeletonize_labels takes uint16 / uint32 / int32 ids"
        t = ids.to(torch.int32) if name == "uint16" else ids.contiguous().view(torch.int32).clone()
    else:
        a = np.asarray(ids)
        name = a.dtype.name
        assert name in ("uint16", "uint32", "int32"), "skeletonize_labels takes uint16 / uint32 / int32 ids"
        t = torch.from_numpy(np.ascontiguousarray(a).astype(np.uint32).view(np.int32)).cuda()
    shape = tuple(t.shape)
    assert 2 <= len(shape) <= 3, "skeletonize_labels needs a (Z, Y, X) or (Y, X) map"
    Z, Y, X = (1,) * (3 - len(shape)) + shape
    if Z * Y * X != 0:
        work = _workspace(lib().ppp_skeletonize_labels_workspace_bytes(Z, Y, X), t.device)
        kept = ctypes.c_int64(0)
        stats = (ctypes.c_int32 * 3)()
        with _timed("skeletonize_labels"):
            check(lib().ppp_skeletonize_labels(_dev_ptr(t), _dev_ptr(t), Z, Y, X, ctypes.byref(kept), stats,
                                               _dev_ptr(work), _stream()))
        NOTES["skeleton_stats"] = tuple(int(v) for v in stats)
        NOTES["skeleton_kept"] = int(kept.value)
    if is_tensor:
        return (t & 0xFFFF).to(torch.uint16) if name == "uint16" else t.view(ids.dtype)
    return t.cpu().numpy().view(np.uint32).astype(a.dtype)


def _overlap_stack(t, who):
    torch = _torch()
    assert torch.is_tensor(t) and t.is_cuda and t.dim() == 4, "label_overlap: %s must be a (L, Z, Y, X) device tensor" % who
    assert str(t.dtype) in ("torch.uint32", "torch.int32"), "label_overlap: %s must hold 32-bit ids (uint32, or int32 storage)" % who
    return t.contiguous().view(torch.int32)


def label_overlap_raw(a, b, cap, rows=None, counts=None, work=None):
    """ONE ppp_label_overlap call: `a` (La, Z, Y, X) and `b` (Lb, Z, Y, X) device tensors of 32-bit ids,
    `rows` int32 storage [cap, 2] and `counts` int64 [cap] device tensors (None with cap = 0: the size
    query), `work` the workspace (None: allocated here).  Returns n_rows; the rows are written when
    n_rows <= cap."""
    a, b = _overlap_stack(a, "a"), _overlap_stack(b, "b")
    assert tuple(a.shape[1:]) == tuple(b.shape[1:]), "label_overlap: the stacks differ in (Z, Y, X)"
    La, Z, Y, X = [int(v) for v in a.shape]
    Lb = int(b.shape[0])
    if work is None:
        work = _workspace(lib().ppp_label_overlap_workspace_bytes(La, Lb, Z, Y, X), a.device)
    n = ctypes.c_int64(0)
    with _timed("label_overlap"):
        check(lib().ppp_label_overlap(_dev_ptr(a), La, _dev_ptr(b), Lb, Z, Y, X, _dev_ptr(rows), _dev_ptr(counts),
                                      int(cap), ctypes.byref(n), _dev_ptr(work), _stream()))
    return int(n.value)


OVERLAP_WORK_SHARE = 0.25      # label_overlap: the workspace of one call stays within this share of the free device memory


def _overlap_once(a, b):
    """one volume (or chunk of one) through ppp_label_overlap, size query and retry included"""
    torch = _torch()
    La, Z, Y, X = [int(v) for v in a.shape]
    work = _workspace(lib().ppp_label_overlap_workspace_bytes(La, int(b.shape[0]), Z, Y, X), a.device)
    cap = 1 << 16
    while True:
        rows = torch.empty((cap, 2), dtype=torch.int32, device=a.device)
        counts = torch.empty((cap,), dtype=torch.int64, device=a.device)
        n = label_overlap_raw(a, b, cap, rows, counts, work)
        if n <= cap:
            break
        cap = n
    return np.ascontiguousarray(rows[:n].cpu().numpy()).view(np.uint32), counts[:n].cpu().numpy()


def label_overlap_last_stats():
    """ppp_label_overlap_last_stats: (partial counts written, table flushes inside the pass's loop, items that went
    past the table) of the last ppp_label_overlap call in this process."""
    st = (ctypes.c_int64 * 3)()
    lib().ppp_label_overlap_last_stats(st)
    return tuple(int(v) for v in st)


def label_overlap(a, b, work_bytes=None):
    """ppp_label_overlap: the contingency table of two stacks of label maps, device tensors (La, Z, Y, X) and
    (Lb, Z, Y, X) of 32-bit ids (uint32, or int32 storage read as uint32; 0 = background).  Returns
    (rows uint32 [n, 2], counts int64 [n]) as host NumPy arrays: rows (a, b) with a, b != 0 count the
    (channel pair, voxel) incidences, rows (a, 0) and (0, b) are the sizes of the ids; sorted by (a, b).
    Equal to evaluate_instances.overlap_counts_host, integer for integer.  A call runs with room for the rows
    of a typical map; one that needs more is repeated once with the size it reported.

    The entry point's workspace covers the worst case, 32 bytes per voxel and key stream.  Where that exceeds
    `work_bytes` (default: OVERLAP_WORK_SHARE of the free device memory) the flat volume is cut into chunks of
    voxels that fit, each chunk is one call, and the tables -- counts of disjoint sets of voxels -- are added
    on the host: the same rows."""
    torch = _torch()
    a, b = _overlap_stack(a, "a"), _overlap_stack(b, "b")
    assert tuple(a.shape[1:]) == tuple(b.shape[1:]), "label_overlap: the stacks differ in (Z, Y, X)"
    La, Lb = int(a.shape[0]), int(b.shape[0])
    V = int(a[0].numel())
    if V == 0:
        return np.zeros((0, 2), dtype=np.uint32), np.zeros(0, dtype=np.int64)
    if work_bytes is None:
        work_bytes = int(OVERLAP_WORK_SHARE * torch.cuda.mem_get_info(a.device)[0])
    need = int(lib().ppp_label_overlap_workspace_bytes(La, Lb, *[int(v) for v in a.shape[1:]]))
    check(min(need, 0))
    if need <= work_bytes:
        return _overlap_once(a, b)
    a, b = a.reshape(La, 1, 1, V), b.reshape(Lb, 1, 1, V)
    chunk = max(1, min(V, int(work_bytes) // (40 * (La * Lb + La + Lb))))      # (32 bytes; 8 for the sort's temporary storage, 256-byte slots)
    keys, counts = [], []
    for v0 in range(0, V, chunk):
        r, c = _overlap_once(a[..., v0:v0 + chunk].contiguous(), b[..., v0:v0 + chunk].contiguous())
        keys.append(r[:, 0].astype(np.uint64) << np.uint64(32) | r[:, 1].astype(np.uint64))
        counts.append(c)
    u, inverse = np.unique(np.concatenate(keys), return_inverse=True)
    total = np.zeros(len(u), dtype=np.int64)
    np.add.at(total, inverse.reshape(-1), np.concatenate(counts))
    rows = np.stack([(u >> np.uint64(32)).astype(np.uint32), (u & np.uint64(0xFFFFFFFF)).astype(np.uint32)], axis=1)
    return rows.reshape(-1, 2), total


def host_skel_rule_mismatches(first, count):
    """ppp_host_skel_rule_mismatches: neighbour patterns in [first, first + count) on which the rule the
    device kernels evaluate (csrc/ppp_skel_rule.hpp) and the host thinning's predicates disagree."""
    n = int(lib().ppp_host_skel_rule_mismatches(int(first), int(count)))
    if n < 0:
        raise ValueError("ppp_host_skel_rule_mismatches: the range leaves [0, 2^26]")
    return n


def host_patch_pairs(sel_zyx, patchshape, max_ps_dist=2, include_single=True):
    sel = np.ascontiguousarray(np.asarray(sel_zyx).reshape(-1, 3), dtype=np.int32)
    ps = _i32(patchshape)
    n = len(sel)
    sorted_zyx = np.empty((n, 3), dtype=np.int32)
    rows = lib().ppp_host_patch_pairs(_np_ptr(sel), n, _np_ptr(ps), int(max_ps_dist),
                                      1 if include_single else 0, _np_ptr(sorted_zyx), None)
    if rows == 0:
        return sorted_zyx, None
    pairs = np.empty((rows, 6), dtype=np.uint32)
    lib().ppp_host_patch_pairs(_np_ptr(sel), n, _np_ptr(ps), int(max_ps_dist),
                               1 if include_single else 0, _np_ptr(sorted_zyx), _np_ptr(pairs))
    return sorted_zyx, pairs
