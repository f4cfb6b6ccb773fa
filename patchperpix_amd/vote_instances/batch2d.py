"""A stack of independent 2-d images voted in one call
(``to_instance_seg(..., independent_slices=True)``).

The reference takes 2-d data with a z axis of 1 (utilVoteInstances.py:187); on a stack of slices
its pair enumeration links patches of neighbouring slices.  Here the z axis of a (C, N, Y, X)
prediction with 2-d patches (1, py, px) is a BATCH: slice k gets, bit for bit, what a call on
``pred[:, k:k+1]`` gives -- its ids numbered from 1 -- but every stage runs once for the stack.

Why that is the per-image result, stage by stage (pz = 1: no window, consensus offset or thinning
neighbourhood reaches another slice):
  S1 / S2   slice-local kernels; the ranked list is a stable sort of raster order by score, so each
            slice's subsequence is its own ranked list;
  S3        the device cover's rounds are slice-local; what is not is the loop's stop rule ("the
            interior is empty") -- applied per slice here, and a slice that is done takes no part in
            the later pixTh passes.  The score_threshold break is a cut of a list sorted by score,
            the same in every subsequence.  mark_close_neighboorhood (marks never leave the
            centre's slice) and select_patches_overlap_neighborhood (in-plane dilation) ride the same
            batched rounds (foreground_cover.cover_options_device, per_slice); the host loop, where
            it is asked for, runs per slice;
  S4        ppp_thin_cover_slices: the same rounds, the stop rule per slice;
  pairs     the selected list sorted by (z, x), partners in the same slice only
            (ppp_patch_pairs_*_slices): the rows of slice k in its own canonical order;
  S5        every image's own LCG seeds (ppp_patch_graph*_slices);
  S6        components: keys ranked by (slice, key), renumbered per slice on the device
            (ppp_label_slice_renumber); mutex watershed: the edge list is made once for the stack,
            the sequential loop walks each slice's edges (a subsequence in the same order).
A stack whose consensus does not fit in HBM is cut into chunks of whole slices (no halo:
tiling.plan_slice_chunks), each chunk one batch.
"""
import logging
import os

import numpy as np

from .. import backend
from .aff_patch_graph import PatchPairs
from .consensus_array import loadOrComputeConsensus
from .foreground_cover import (_bits_for, _pix_thresholds, cover_options_device, cover_sequential, marks_on_device,
                               never_selected)
from .ranked_patches import PatchList, loadOrComputePatchRanking

logger = logging.getLogger(__name__)

# flags whose per-image result a batch does not reproduce: refused, never ignored
UNSUPPORTED_FLAGS = ("debug", "isbiHack", "blockwise", "graphToInst", "skipConsensus", "skipRanking",
                     "termAfterThinCover", "termAfterPatchGraph", "save_consensus", "save_patch_graph",
                     "pad_with_ps", "one_instance_per_channel", "no_overlap_per_channel", "sparse_labels")
# inputs that hand in stored stages or lists of one image
UNSUPPORTED_INPUTS = ("aff_graph", "selected_patches", "selected_patch_pairs", "consensus", "ranked_patches")


def check_flags(patchshape, kwargs):
    """Raise for what a batched call cannot serve: 3-d patches (ValueError), and the flags whose
    per-image result it does not reproduce (NotImplementedError naming the flag)."""
    if int(patchshape[0]) != 1:
        raise ValueError("independent_slices needs 2-d patches (1, py, px), not %s" % (list(patchshape),))
    if not kwargs.get("cuda", False):
        raise NotImplementedError("cuda=False (the NumPy semantics) is not supported with independent_slices")
    for opt in UNSUPPORTED_FLAGS:
        if kwargs.get(opt, False):
            raise NotImplementedError("%s is not supported with independent_slices" % opt)
    for opt in UNSUPPORTED_INPUTS:
        if kwargs.get(opt) is not None:
            raise NotImplementedError("%s is not supported with independent_slices" % opt)
    if kwargs.get("sample", 1.0) < 1.0:
        raise NotImplementedError("sample < 1 is not supported with independent_slices")


def slice_bytes(shape_yx, patchshape):
    """HBM one slice of a batch holds at the peak: the compact consensus planes and their
    voxel-major copy (S5), plus ~70 bytes per pixel of ranked lists and cover / sort work space."""
    py, px = int(patchshape[1]), int(patchshape[2])
    planes = ((2 * py - 1) * (2 * px - 1) - 1) // 2
    row = (2 * py - 1) * (2 * px - 1)
    return int(shape_yx[0]) * int(shape_yx[1]) * (4 * (planes + row) + 70)


def to_instance_seg_slices(pred_affs, foreground, mask_to_cover, numinst, patchshape, **kwargs):
    """``to_instance_seg`` on a (C, N, Y, X) stack of N independent 2-d images (patches (1, py, px)).
    Returns (instances (N, Y, X), foreground uint8 (N, Y, X)), slice k equal to a call on slice k
    alone -- or, with ``return_intermediates``, a list of N (pairs, aff), slice-local z = 0, and
    (None, None) where that slice's own call returns early.  mask_to_cover is modified in place
    as the single call does (overlap voxels cleared)."""
    import torch
    from .. import tiling
    from .vote_instances import _skeletonize
    patchshape = np.array([int(p) for p in patchshape])
    check_flags(patchshape, kwargs)
    rad = patchshape // 2
    pred_affs = backend.to_device_pred(pred_affs)
    host = lambda a: a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)      # noqa: E731
    if torch.is_tensor(mask_to_cover):
        mask_to_cover = mask_to_cover.cpu().numpy().astype(bool)
    foreground, numinst = host(foreground), host(numinst)
    N, Y, X = [int(v) for v in foreground.shape]
    if tuple(pred_affs.shape[1:]) != (N, Y, X):
        raise ValueError("prediction %s and foreground %s differ in shape" % (tuple(pred_affs.shape), (N, Y, X)))
    id_dtype = np.dtype(kwargs.get("_instances_dtype") or np.uint16)
    want_inter = kwargs.get("return_intermediates", False)
    if kwargs.get("skeletonize_foreground"):
        # per image: a 3-d thinning of the stack is a different function
        mask_to_cover = np.concatenate([_skeletonize(mask_to_cover[k:k + 1], kwargs.get("skeletonize_backend"))
                                        for k in range(N)]) if N else mask_to_cover
    ov = numinst > 1
    mask_to_cover[ov] = 0                                             # vote_instances.py:226
    inner = (slice(None), slice(int(rad[1]), Y - int(rad[1])), slice(int(rad[2]), X - int(rad[2])))
    # the per-image early-outs ("no fg found", "no patches found"): those slices stay zero
    live = np.flatnonzero((np.count_nonzero(mask_to_cover[inner], axis=(1, 2)) > 0) &
                          (np.count_nonzero(foreground[inner], axis=(1, 2)) > 0))
    instances = np.zeros((N, Y, X), dtype=id_dtype)
    inter = [(None, None)] * N
    # chunks of whole slices whose working set fits next to what is already resident
    n_chunk = kwargs.get("_chunk_slices")
    if n_chunk is None:
        avail = torch.cuda.mem_get_info()[0] + (torch.cuda.memory_reserved() - torch.cuda.memory_allocated())
        per_slice = slice_bytes((Y, X), patchshape)
        n_chunk = tiling.plan_slice_chunks(len(live), per_slice, 0.8 * avail)
        if len(live) < N or n_chunk < len(live):
            # a chunk that is not the whole stack votes a copy of its slices' prediction
            copy = int(pred_affs.shape[0]) * Y * X * pred_affs.element_size()
            n_chunk = tiling.plan_slice_chunks(len(live), per_slice + copy, 0.8 * avail)
    chunks = [live[i:i + int(n_chunk)] for i in range(0, len(live), max(1, int(n_chunk)))]
    backend.note("batch2d_chunks", len(chunks))
    if not kwargs.get("save_no_intermediates", False):
        # the per-image files (selected_patch_pairs.npy, ranking.pickle, ...) have fixed names in the
        # result folder: one call per image overwrites them, a batch has no per-image form of them
        logger.warning("independent_slices: the intermediate files of save_no_intermediates=False are not "
                       "written for a batch of images")
    kw = dict(kwargs, save_no_intermediates=True)
    for ks in chunks:
        sl = torch.from_numpy(ks).to(pred_affs.device)
        pred = pred_affs.index_select(1, sl).contiguous() if len(ks) < N else pred_affs
        res = _vote_batch(pred, foreground[ks], mask_to_cover[ks], numinst[ks], patchshape, id_dtype, kw)
        if want_inter:
            for j, k in enumerate(ks):
                inter[k] = res[j]
        else:
            instances[ks] = res
    if want_inter:
        return inter
    return instances, foreground.astype(np.uint8)


def _vote_batch(pred, foreground, mask_to_cover, numinst, patchshape, id_dtype, kw):
    """S1 .. S6 for one batch of slices that all pass the early-outs: instances (n, Y, X), or the
    list of n per-slice (pairs, aff)."""
    import torch
    dev = pred.device
    shape = tuple(int(v) for v in foreground.shape)
    n, Y, X = shape
    rad = patchshape // 2
    radslice = (slice(0, n), slice(int(rad[1]), Y - int(rad[1])), slice(int(rad[2]), X - int(rad[2])))
    overlap_mask = 1 * (numinst > 1)
    neighshape = patchshape.copy()
    neighshape[1:] *= 2
    instances = np.zeros(shape, dtype=id_dtype)
    P = backend.params_from_kwargs(shape, patchshape, kw)
    with backend.host_timer("s1_consensus"):
        cons, _, _ = loadOrComputeConsensus(instances, patchshape, neighshape, None, pred, rad, foreground,
                                            None, overlap_mask, **kw)
    with backend.host_timer("s2_rank_and_sort"):
        ranked, scores_array = loadOrComputePatchRanking(
            pred_affs=pred, consensus_vote_array=cons, overlap_mask=overlap_mask, all_patches=None,
            patchshape=patchshape, neighshape=neighshape, rad=rad, _foreground=foreground, **kw)
    ranked = PatchList.from_any(ranked)
    if kw.get("skipSelection", False):
        sel = ranked
    else:
        with backend.host_timer("s3_cover"):
            sel = _cover(overlap_mask, mask_to_cover, patchshape, ranked, radslice, pred, scores_array, P, kw)
    if not kw.get("skipThinCover") and len(sel) > 0:
        with backend.host_timer("s4_thin"):
            sel = _thin(mask_to_cover, sel, radslice, pred, patchshape, P, kw)
    with backend.host_timer("pairs"):
        order = np.lexsort((sel.coords[:, 2], sel.coords[:, 0]))          # stable: by z, then x
        sorted_zyx = np.ascontiguousarray(sel.coords[order], dtype=np.int32)
        rows = backend.device_patch_pairs(
            torch.from_numpy(sorted_zyx).to(dev), P,
            max_ps_dist=kw.get("max_total_patch_distance_in_ps_multiples", 2),
            include_single=kw["includeSinglePatchCCS"], slices=True)
    if rows is None:
        return [(None, None)] * n if kw.get("return_intermediates") else instances
    pairs = PatchPairs(rows, sorted_zyx)
    pairs.unique_pairs = True
    with backend.host_timer("s5_patch_graph"):
        if P.cons_layout == backend.CONS_COMPACT:
            aff = backend.patch_graph_auto(pred, cons, rows, P, slices=True)
        else:
            aff = backend.patch_graph(pred, cons, rows, P, order=backend.pair_order(rows, P), slices=True)
    del cons
    backend.note("n_selected", len(sel))
    backend.note("n_pairs", len(pairs))
    if kw.get("return_intermediates"):
        return split_rows(pairs.numpy(), aff.cpu().numpy(), n)
    with backend.host_timer("s6_label_paint"):
        return _label_and_paint(pred, pairs, aff, instances, P, kw)


def split_rows(rows, aff, n):
    """The rows of a batch (uint32 [R, 6]) and their affinities as n per-slice (pairs, aff) with
    slice-local z = 0 -- (None, None) for a slice without rows."""
    out = []
    order = np.argsort(rows[:, 0], kind="stable")      # by slice, the slice's own order inside
    starts = np.searchsorted(rows[order, 0], np.arange(n + 1))
    for k in range(n):
        own = order[starts[k]:starts[k + 1]]
        if len(own) == 0:
            out.append((None, None))
            continue
        r = rows[own].copy()
        r[:, 0] = 0
        r[:, 3] = 0
        out.append((r, aff[own]))
    return out


def _cover(overlap_mask, mask_to_cover, patchshape, ranked, radslice, pred, scores_array, P, kw):
    """S3 of every slice: the selected patches, slice after slice, each slice in its own order."""
    import torch
    n, Y, X = mask_to_cover.shape
    mark = bool(kw.get("mark_close_neighboorhood", False))
    near_overlap = bool(kw.get("select_patches_overlap_neighborhood", False))
    if len(ranked) == 0:
        return ranked
    on_device = os.environ.get("PPP_COVER", "device") != "host" and int(patchshape[2]) <= 32
    if on_device and (mark or near_overlap) and marks_on_device(mask_to_cover.shape, kw):
        # marks stay in their slice and p_z - 1 = 0: one batched cover serves them; the stop rule, the
        # score break, the ring's pixel threshold and its (in-plane) dilation are per slice
        dev = pred.device
        mask = torch.from_numpy(np.ascontiguousarray(mask_to_cover != 0).astype(np.uint8)).to(dev)
        ov = np.asarray(overlap_mask)
        overlap = torch.from_numpy(np.ascontiguousarray(ov != 0).astype(np.uint8)).to(dev) if ov.any() else None
        bits = backend.patch_bits(pred, torch.from_numpy(ranked.coords).to(dev), kw["fc_threshold"], P)
        order = cover_options_device(mask, overlap, bits, torch.from_numpy(ranked.lin(mask.shape)).to(dev),
                                     torch.from_numpy(np.ascontiguousarray(ranked.scores)).to(dev),
                                     _pix_thresholds(patchshape, kw), radslice, P, kw, per_slice=True)
        sel = ranked[order.cpu().numpy()]
        if near_overlap and len(sel):
            # the reference rebuilds the list from the score volume (foreground_cover.py:83-85)
            sel = PatchList(sel.coords, np.asarray(scores_array)[tuple(sel.coords.T)])
        return sel
    if not on_device or mark or near_overlap:
        # the sequential loop (and its marks) per slice, on the slice's subsequence of the ranked list
        parts = []
        z = ranked.coords[:, 0]
        one = (slice(0, 1),) + tuple(radslice[1:])
        for k in range(n):
            sub = ranked[np.flatnonzero(z == k)]
            local = PatchList(sub.coords - np.array([k, 0, 0], dtype=sub.coords.dtype), sub.scores)
            bits_of = lambda c, k=k: _bits_for(pred, c + np.array([k, 0, 0], dtype=c.dtype),   # noqa: E731
                                                kw["fc_threshold"], P)
            sc = scores_array[k:k + 1]
            sel, _ = cover_sequential(overlap_mask[k:k + 1], mask_to_cover[k:k + 1], patchshape, local, one,
                                      bits_of, sc, silent=True, **kw)
            parts.append(PatchList(sel.coords + np.array([k, 0, 0], dtype=sel.coords.dtype), sel.scores))
        return PatchList(np.concatenate([p.coords for p in parts]).reshape(-1, 3),
                         np.concatenate([p.scores for p in parts]))
    dev = pred.device
    mask = torch.from_numpy(np.ascontiguousarray(mask_to_cover != 0).astype(np.uint8)).to(dev)
    lin_h = ranked.lin(mask.shape)
    bits = backend.patch_bits(pred, torch.from_numpy(ranked.coords).to(dev), kw["fc_threshold"], P)
    never = torch.from_numpy(never_selected(overlap_mask, lin_h, ranked.scores,
                                            kw.get("score_threshold", False))).to(dev)
    lin = torch.from_numpy(lin_h).to(dev)
    selected = greedy_cover_slices(mask, bits, lin, never, _pix_thresholds(patchshape, kw), radslice, P)
    return ranked[np.flatnonzero(selected.cpu().numpy())]


def greedy_cover_slices(mask, bits, lin, never, pix_ths, radslice, P):
    """foreground_cover.greedy_cover_device with the loop's stop rule per slice: in every slice, the
    patches after the one that empties the slice's interior are dropped, and a slice that is done
    takes no part in the later passes.  Returns selected, bool [n] device (rank order)."""
    import torch
    n_sl, Y, X = [int(v) for v in mask.shape]
    plane = Y * X
    remaining = torch.count_nonzero(mask[tuple(radslice)], dim=(1, 2)).to(torch.int64)
    z_of = torch.div(lin, plane, rounding_mode="floor")
    selected = torch.zeros(int(lin.numel()), dtype=torch.bool, device=mask.device)
    total_rounds = 0
    for pix_th in pix_ths:
        done = remaining <= 0
        if bool(done.all().item()):
            break
        state = torch.where(selected, 1, torch.where(never | done[z_of], 2, 0)).to(torch.int32)
        cleared, rounds = backend.cover_pass_device(mask, bits, lin, state, pix_th, P)
        total_rounds += rounds
        idx = torch.nonzero((state == 1) & ~selected).flatten()          # rank order
        if idx.numel() == 0:
            continue
        zi = z_of[idx]
        o = torch.sort(zi, stable=True)[1]
        idx, zi = idx[o], zi[o]                                          # by slice, rank order inside
        c = cleared[idx].to(torch.int64)
        _, counts = torch.unique_consecutive(zi, return_counts=True)
        first = torch.repeat_interleave(torch.cumsum(counts, 0) - counts, counts)
        before = torch.cumsum(c, 0) - c                                  # cleared by earlier patches of the batch
        seg_before = before - before[first]                              # ... of the same slice
        keep = remaining[zi] - seg_before > 0                            # the slice's interior not empty yet
        selected[idx[keep]] = True
        remaining.index_add_(0, zi[keep], -c[keep])
    backend.note("cover_rounds", total_rounds)
    return selected


def _thin(mask_to_cover, sel, radslice, pred, patchshape, P, kw):
    """S4 of every slice (foreground_cover.thinOutForegroundCover with the stop rule per slice)."""
    import torch
    n = mask_to_cover.shape[0]
    mask = np.ascontiguousarray(mask_to_cover).astype(np.uint8)
    interior = np.count_nonzero(mask[tuple(radslice)], axis=(1, 2)).astype(np.int64)
    if os.environ.get("PPP_THIN", "device") != "host" and int(patchshape[2]) <= 32:
        dev = pred.device
        c = torch.from_numpy(np.ascontiguousarray(sel.coords, dtype=np.int32)).to(dev)
        bits_d = backend.patch_bits(pred, c, kw["fc_threshold"], P)
        keep = backend.thin_cover_device(torch.from_numpy((mask != 0).astype(np.uint8)).to(dev), bits_d,
                                         torch.from_numpy(sel.lin(mask.shape)).to(dev), P,
                                         slice_interior=interior).cpu().numpy()
    else:
        keep = np.zeros(len(sel), dtype=bool)
        for k in range(n):
            own = np.flatnonzero(sel.coords[:, 0] == k)
            if len(own) == 0:
                continue
            local = sel.coords[own] - np.array([k, 0, 0], dtype=sel.coords.dtype)
            bits = _bits_for(pred, sel.coords[own], kw["fc_threshold"], P)
            lin = (local[:, 1].astype(np.int64) * mask.shape[2] + local[:, 2])
            keep[own] = backend.host_thin_cover(mask[k:k + 1], patchshape, lin, bits) != 0
    return sel[np.flatnonzero(keep)]


def _label_and_paint(pred, pairs, aff, instances, P, kw):
    """S6: ids per slice (uint16 overflow checked per slice, as the single call does), painted."""
    import torch
    dev = pred.device
    nodes_h = pairs.nodes
    nodes = torch.from_numpy(nodes_h).to(dev)
    n = int(instances.shape[0])
    if kw["mws"]:
        labels = mws_labels_slices(pairs.rows_dev, aff, nodes, nodes_h[:, 0], n, P)
        top = np.zeros(n, dtype=np.int64)
        lab_h = labels.cpu().numpy()
        np.maximum.at(top, nodes_h[:, 0], lab_h)
    else:
        keys = backend.label_components(pairs.rows_dev, aff, nodes, P)
        valid = keys != backend.NONE_KEY
        comp = nodes[:, 0].to(torch.int64) * (1 << 32) + keys          # (slice, order key)
        labels = torch.zeros(int(nodes.shape[0]), dtype=torch.int32, device=dev)
        if bool(valid.any().item()):
            _, inv = torch.unique(comp[valid], return_inverse=True)
            labels[valid] = (inv + 1).to(torch.int32)
        top = backend.label_slice_renumber(nodes, labels, P).cpu().numpy()
    limit = np.iinfo(instances.dtype).max
    if len(top) and top.max() > limit:
        raise OverflowError("%d instances do not fit %s (slice %d)" % (top.max(), instances.dtype, int(np.argmax(top))))
    inst_dev = torch.zeros(tuple(instances.shape), dtype=torch.int32, device=dev)
    if int(nodes.shape[0]):
        backend.paint_instances(pred, nodes, labels, inst_dev, P)
    return inst_dev.cpu().numpy().astype(instances.dtype)


def mws_labels_slices(rows, aff, nodes, node_z, n_slices, P):
    """Mutex watershed per slice: the edge list made once for the stack (backend.mws_edges_device:
    networkx's edge order, stably sorted by |aff| -- each slice's edges are a subsequence in its own
    order), then the sequential loop over each slice's edges with the slice's node numbers.  nodes
    int32 [K, 3] device, sorted by slice; node_z host [K].  Returns int32 [K] device labels,
    numbered per slice."""
    torch = backend._torch()
    n, k = int(rows.shape[0]), int(nodes.shape[0])
    labels = np.zeros((k,), dtype=np.int32)
    if n and k:
        eu_h, ev_h = backend.mws_edges_device(rows, aff, nodes, P)
        node_starts = np.searchsorted(node_z, np.arange(n_slices + 1))
        # the edges grouped by slice, in their order inside each slice
        order = np.argsort(node_z[eu_h], kind="stable")
        edge_starts = np.searchsorted(node_z[eu_h][order], np.arange(n_slices + 1))
        eu_h, ev_h = eu_h[order], ev_h[order]
        with backend.host_timer("s6b_mws_loop"):
            for s in range(n_slices):
                a, b = int(node_starts[s]), int(node_starts[s + 1])
                e0, e1 = int(edge_starts[s]), int(edge_starts[s + 1])
                if b == a or e1 == e0:
                    continue
                eu_s = np.ascontiguousarray(eu_h[e0:e1] - a, dtype=np.int32)
                flag = ev_h[e0:e1] & np.int32(-0x80000000)
                ev_s = np.ascontiguousarray(((ev_h[e0:e1] & 0x7FFFFFFF) - a) | flag, dtype=np.int32)
                out = np.zeros((b - a,), dtype=np.int32)
                backend.lib().ppp_host_mws_sorted(backend._np_ptr(eu_s), backend._np_ptr(ev_s), e1 - e0, b - a,
                                                  backend._np_ptr(out))
                labels[a:b] = out
        backend.note("mws_edges", len(eu_h))
    return torch.from_numpy(labels).to(nodes.device)
