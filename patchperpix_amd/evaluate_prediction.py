"""The `evaluate_prediction` step (reference: PatchPerPix/evaluate/evaluate_prediction.py, called from
experiments/run_ppp.py:1300-1443): a checkpoint's dense prediction scored against the ground truth before
any instance is voted -- `evaluate_patch`, `evaluate_fg`, `evaluate_numinst`, under the reference's names and
kwargs.

evaluate_patch is the one that walks the whole (patch_channels, Z, Y, X) array.  The reference materialises
the ground-truth affinities as a second array of that shape and makes five or six passes per threshold; here
it is ONE streaming reduction on the device (`ppp_eval_patch`, csrc/ppp_eval.hip): the prediction is read in
z-chunks, each element once per four thresholds, the ground-truth affinity comes from the resident label
volume on the fly.  `patch_counts_host` is the definition in NumPy and the path without a device.

Definitions.  pred (C, Z, Y, X), C = pz py px all odd, channel
e = ((dz + rz) py + (dy + ry)) px + (dx + rx); labels (L, Z, Y, X), integer, 0 <= label < 2^31.

  numinst[v] = #{c : labels[c, v] > 0},  ov[v] = numinst[v] > 1
  G[e, v]  = v + off(e) inside the volume and some c has labels[c, v] != 0 == ... == labels[c, v + off(e)]
  G'[e, v] = G[e, v] and not ov[v]          (only the CENTRE's overlap zeroes an entry)
  P_t[e, v] = (0 if ov[v] else pred[e, v]) > tau(t)

G equals the reference's util/train_util.py seg_to_affgraph_{3d,2d}_multi_torch (and, for L = 1, the `> 0` of
seg_to_affgraph_3d_torch), which the reference states to restate gunpowder's add_affinities -- the functions
evaluate_patch itself calls; gunpowder is not compared against directly.  tau is NumPy's comparison of an
array with a Python float: the float rounded to the array's dtype (float32 rounding for float32 and bfloat16,
float16 rounding for float16); NaN compares false; a threshold that is not finite after rounding raises
ValueError.  With a negative threshold the zeroed overlap voxels count as predicted, as in the reference.

The dispatch rule is the post-steps' (`postprocess.use_device`): the device when there is one and
PPP_POSTPROCESS is not "host".
"""
import logging
import os

import numpy as np

from .vote_instances import io_hdflike

logger = logging.getLogger(__name__)

DEFAULT_CHUNK_BYTES = 1 << 30     # `eval_chunk_bytes`: prediction bytes read, uploaded and reduced at a time
FULL_STRUCTURE = (1 << 27) - 1    # np.ones((3, 3, 3)) as ppp_post_clean_mask's structure bits


def use_device():
    from . import postprocess
    return postprocess.use_device()


def _is_tensor(a):
    return type(a).__module__.startswith("torch") and hasattr(a, "is_cuda")


def thresh_key(thresh):
    return str(round(thresh, 2)).replace(".", "_")


# ----------------------------------------------------------------------------------------
# arguments
# ----------------------------------------------------------------------------------------
def _np_dtype_of(pred):
    """the NumPy dtype whose rounding the comparison uses"""
    name = str(pred.dtype).replace("torch.", "")
    if name in ("float32", "bfloat16"):
        return np.float32
    if name == "float16":
        return np.float16
    raise TypeError("the prediction must be float32, float16 or bfloat16, got %s" % name)


def rounded_thresholds(thresholds, dtype):
    """tau(t) per threshold as Python floats: t rounded to `dtype`, ValueError when that is not finite"""
    out = []
    for t in thresholds:
        with np.errstate(over="ignore"):
            tau = float(np.asarray(float(t), dtype=np.float64).astype(dtype))
        if not np.isfinite(tau):
            raise ValueError("threshold %r is not finite as %s" % (t, np.dtype(dtype).name))
        out.append(tau)
    if not out:
        raise ValueError("no thresholds given")
    return out


def _check_patch(patchshape, C):
    ps = [int(p) for p in np.asarray(patchshape).reshape(-1)]
    if len(ps) == 2:
        ps = [1] + ps
    if len(ps) != 3 or any(p < 1 or p % 2 == 0 for p in ps):
        raise ValueError("patchshape %s: three odd positive sides are needed" % (list(patchshape),))
    if ps[0] * ps[1] * ps[2] != C:
        raise ValueError("the prediction has %d channels, the patch %s has %d elements" % (C, ps, ps[0] * ps[1] * ps[2]))
    return ps


def _check_labels(labels, spatial):
    """(L, Z, Y, X) int32, from an integer array with the leading channel axis and values in [0, 2^31)"""
    labels = labels.cpu().numpy() if _is_tensor(labels) else np.asarray(labels)
    if labels.ndim != 1 + len(spatial) or tuple(labels.shape[1:]) != tuple(spatial) or labels.shape[0] < 1:
        raise ValueError("labels of shape %s: (L,) + %s is needed, with the leading channel axis"
                         % (labels.shape, tuple(spatial)))
    if not (np.issubdtype(labels.dtype, np.integer) or labels.dtype == np.bool_):
        raise ValueError("labels must be integers, got %s" % labels.dtype)
    if labels.size and (int(labels.min()) < 0 or int(labels.max()) >= 1 << 31):
        raise ValueError("labels must lie in [0, 2^31)")
    labels = labels.reshape((labels.shape[0],) + (1,) * (3 - len(spatial)) + tuple(spatial))
    return np.ascontiguousarray(labels.astype(np.int32))


# ----------------------------------------------------------------------------------------
# array level
# ----------------------------------------------------------------------------------------
def patch_counts_host(pred, labels, patchshape, thresholds, want_maps=False, z0=0, counts=None):
    """The definition in NumPy.  `pred` (C, tz, Y, X) float32 / float16: the slices z0 .. z0 + tz of the
    prediction; `labels` (L, Z, Y, X), the whole volume.  Returns (counts, inter, union): counts int64
    [1 + 2 T] = num_gt, then (num_pred_t, tp_t) per threshold -- ADDED to `counts` when given; inter / union
    int32 (T, tz, Y, X) or None.  Loops over the channels: no (C, ...) ground-truth array is built."""
    pred = np.asarray(pred)
    if pred.ndim != 4:
        raise ValueError("the prediction must be (C, Z, Y, X), got shape %s" % (pred.shape,))
    C, tz, Y, X = pred.shape
    pz, py, px = _check_patch(patchshape, C)
    labels = np.asarray(labels)
    if labels.ndim != 4 or labels.shape[2:] != (Y, X) or z0 < 0 or z0 + tz > labels.shape[1]:
        raise ValueError("labels of shape %s do not hold the tile z0 = %d of a prediction of shape %s"
                         % (labels.shape, z0, pred.shape))
    labels = _check_labels(labels, labels.shape[1:])
    dtype = _np_dtype_of(pred)
    taus = [dtype(t) for t in rounded_thresholds(thresholds, dtype)]
    T, Z = len(taus), labels.shape[1]
    ov = (labels[:, z0:z0 + tz] > 0).sum(axis=0) > 1
    counts = np.zeros(1 + 2 * T, dtype=np.int64) if counts is None else counts
    inter = np.zeros((T, tz, Y, X), dtype=np.int32) if want_maps else None
    union = np.zeros((T, tz, Y, X), dtype=np.int32) if want_maps else None
    e = 0
    for dz in range(-(pz // 2), pz // 2 + 1):
        for dy in range(-(py // 2), py // 2 + 1):
            for dx in range(-(px // 2), px // 2 + 1):
                g = np.zeros((tz, Y, X), dtype=bool)
                # centre voxels of the tile whose neighbour lies inside the volume
                za, zb = max(z0, -dz), min(z0 + tz, Z - dz)
                ya, yb = max(0, -dy), min(Y, Y - dy)
                xa, xb = max(0, -dx), min(X, X - dx)
                if za < zb and ya < yb and xa < xb:
                    c = labels[:, za:zb, ya:yb, xa:xb]
                    o = labels[:, za + dz:zb + dz, ya + dy:yb + dy, xa + dx:xb + dx]
                    g[za - z0:zb - z0, ya:yb, xa:xb] = ((c != 0) & (c == o)).any(axis=0)
                g &= ~ov
                pe = pred[e].copy()
                pe[ov] = 0
                counts[0] += np.count_nonzero(g)
                for i, tau in enumerate(taus):
                    p = pe > tau
                    both = p & g
                    counts[1 + 2 * i] += np.count_nonzero(p)
                    counts[2 + 2 * i] += np.count_nonzero(both)
                    if want_maps:
                        inter[i] += both
                        union[i] += p | g
                e += 1
    return counts, inter, union


def _z_chunks(Z, slice_bytes, budget):
    tz = max(1, min(Z, int(budget) // max(int(slice_bytes), 1)))
    return [(z, min(tz, Z - z)) for z in range(0, Z, tz)]


def _reduce(read_tile, dtype_name, C, spatial, labels, patch, thresholds, want_maps, budget, device):
    """counts (NumPy int64) and the two maps (NumPy int32 (T, Z, Y, X) or None) of a prediction that
    `read_tile(z, tz)` hands out as (C, tz, Y, X) NumPy arrays or tensors, a z-chunk at a time."""
    Z, Y, X = spatial
    T = len(thresholds)
    elem = 4 if dtype_name == "float32" else 2
    chunks = _z_chunks(Z, C * Y * X * elem, budget)
    inter = np.empty((T, Z, Y, X), dtype=np.int32) if want_maps else None
    union = np.empty((T, Z, Y, X), dtype=np.int32) if want_maps else None
    if device:
        import torch
        from . import backend
        np_dtype = np.float16 if dtype_name == "float16" else np.float32
        taus = rounded_thresholds(thresholds, np_dtype)
        if T > backend.lib().ppp_eval_patch_max_thresholds():
            raise ValueError("at most %d thresholds per call" % backend.lib().ppp_eval_patch_max_thresholds())
        d_labels = torch.from_numpy(labels).cuda()
        d_counts = torch.zeros(1 + 2 * T, dtype=torch.int64, device="cuda")
        for z, tz in chunks:
            tile = read_tile(z, tz)
            tile = tile if _is_tensor(tile) else torch.from_numpy(np.ascontiguousarray(tile))
            tile = tile.cuda().contiguous()
            i_t, u_t = backend.eval_patch(tile, d_labels, patch, z, taus, d_counts, want_maps)
            if want_maps:
                inter[:, z:z + tz] = i_t.cpu().numpy()
                union[:, z:z + tz] = u_t.cpu().numpy()
        return d_counts.cpu().numpy(), inter, union
    counts = None
    for z, tz in chunks:
        tile = read_tile(z, tz)
        if _is_tensor(tile):
            tile = (tile.float() if dtype_name == "bfloat16" else tile).cpu().numpy()
        counts, i_t, u_t = patch_counts_host(tile, labels, patch, thresholds, want_maps, z0=z, counts=counts)
        if want_maps:
            inter[:, z:z + tz], union[:, z:z + tz] = i_t, u_t
    return counts, inter, union


def metrics_from_counts(counts, thresholds, inter=None, union=None, return_patches=False, store_iou=False):
    """evaluate_prediction.py:94-150 from the integer counts: the reference's arithmetic, literally, in
    float64 on the host.  The IOU results are NumPy's from the integer maps, so they equal the reference's
    bit for bit, the NaN of an empty selection included."""
    num_gt = int(counts[0])
    metrics = {}
    for i, thresh in enumerate(thresholds):
        num_pred, tp = int(counts[1 + 2 * i]), int(counts[2 + 2 * i])
        precision = tp / max(float(num_pred), 1)
        recall = tp / max(float(num_gt), 1)
        f1 = 2 * (precision * recall) / max((precision + recall), 1)
        entry = {"precision": precision, "recall": recall, "f1": f1}
        if return_patches:
            unionFG = union[i].astype(np.int64)
            unionFG[unionFG == 0] = 1
            IOU = inter[i].astype(np.int64) / unionFG
            if store_iou:
                entry["IOU"] = IOU
            else:
                with np.errstate(invalid="ignore"), _quiet_empty_mean():
                    entry["IOU_mean"] = np.mean(IOU[unionFG > 1])
        metrics[thresh_key(thresh)] = {"rsc_0": entry}
    return metrics


class _quiet_empty_mean:
    """np.mean of an empty selection is NaN, as in the reference; its RuntimeWarning is not news here"""

    def __enter__(self):
        import warnings
        self._cm = warnings.catch_warnings()
        self._cm.__enter__()
        warnings.simplefilter("ignore", RuntimeWarning)

    def __exit__(self, *exc):
        return self._cm.__exit__(*exc)


def patch_metrics(pred, labels, patchshape, thresholds, return_patches=False, store_iou=False,
                  eval_chunk_bytes=DEFAULT_CHUNK_BYTES):
    """evaluate_patch on arrays: `pred` (C, Z, Y, X), a NumPy array (float32 / float16) or a tensor (bfloat16
    too), `labels` (L, Z, Y, X).  The device when there is one, else `patch_counts_host`.  Returns the
    reference's metric dict {thresh_key: {"rsc_0": {precision, recall, f1[, IOU | IOU_mean]}}}."""
    if pred.ndim != 4:
        raise ValueError("the prediction must be (C, Z, Y, X), got shape %s" % (tuple(pred.shape),))
    C, Z, Y, X = [int(s) for s in pred.shape]
    patch = _check_patch(patchshape, C)
    lab = _check_labels(labels, (Z, Y, X))
    name = str(pred.dtype).replace("torch.", "")
    rounded_thresholds(thresholds, _np_dtype_of(pred))
    counts, inter, union = _reduce(lambda z, tz: pred[:, z:z + tz], name, C, (Z, Y, X), lab, patch,
                                   [float(t) for t in thresholds], bool(return_patches), eval_chunk_bytes, use_device())
    return metrics_from_counts(counts, thresholds, inter, union, return_patches, store_iou)


# ----------------------------------------------------------------------------------------
# file level: the reference's names and kwargs
# ----------------------------------------------------------------------------------------
def _read_labels(label_fn, key):
    if not label_fn.rstrip("/").endswith(("zarr", "hdf")):
        raise NotImplementedError(label_fn)
    with io_hdflike.open_container(label_fn, "r") as inf:
        return np.array(inf[key])


def _refuse_png(kwargs):
    if kwargs.get("save_as_png", False):
        raise NotImplementedError("save_as_png = true is not provided by this repository (there is no PNG writer); "
                                  "unset it")


def evaluate_patch(prediction_fn, label_fn, **kwargs):
    """evaluate_prediction.py:38-150.  kwargs: aff_key, sample_gt_key, patchshape, eval_patch_thresholds,
    return_patches, store_iou (the reference's), and `eval_chunk_bytes` (this project's: the prediction is read
    in z-chunks of at most that many bytes, default 1 GiB, each uploaded and reduced; the host never holds
    the whole prediction nor any ground-truth affinity array).  `overlapping_inst` is accepted and not
    needed: G is one definition for every L.

    Both containers follow the reference's HDF branch (`np.squeeze(np.array(...))`): its zarr branch cannot
    run as written -- it assigns into an array opened read-only and compares a zarr array with a float.
    So the unit axes of the dataset are dropped: (C, Y, X) is a 2-d prediction (Z = 1, pz = 1), (C, Z, Y, X)
    a 3-d one; the labels are (L,) + the prediction's spatial shape, and the IOU arrays have that spatial
    shape."""
    if not prediction_fn.rstrip("/").endswith(("zarr", "hdf")):
        raise NotImplementedError(prediction_fn)
    thresholds = [float(t) for t in kwargs["eval_patch_thresholds"]]
    want_maps = bool(kwargs.get("return_patches"))
    with io_hdflike.open_container(prediction_fn, "r") as inf:
        ds = inf[kwargs["aff_key"]]
        full = tuple(int(s) for s in ds.shape)
        axes = [a for a, s in enumerate(full) if s != 1]
        if len(axes) not in (3, 4):
            raise NotImplementedError("a prediction of shape %s is neither 2-d nor 3-d" % (full,))
        squeezed = tuple(full[a] for a in axes)
        C, spatial = squeezed[0], squeezed[1:]
        patch = _check_patch(kwargs["patchshape"], C)
        if len(spatial) == 2 and patch[0] != 1:
            raise ValueError("a 2-d prediction needs a patch with pz = 1")
        labels = _check_labels(_read_labels(label_fn, kwargs["sample_gt_key"]), spatial)
        name = np.dtype(ds.dtype).name
        rounded_thresholds(thresholds, _np_dtype_of(ds))
        vol = (1,) * (3 - len(spatial)) + spatial
        zaxis = axes[1] if len(spatial) == 3 else None

        def read_tile(z, tz):
            sel = [slice(None)] * len(full)
            if zaxis is not None:
                sel[zaxis] = slice(z, z + tz)
            return np.asarray(ds[tuple(sel)]).reshape((C, tz) + vol[1:])
        counts, inter, union = _reduce(read_tile, name, C, vol, labels, patch, thresholds, want_maps,
                                       kwargs.get("eval_chunk_bytes", DEFAULT_CHUNK_BYTES), use_device())
    if want_maps:
        inter, union = inter.reshape((-1,) + spatial), union.reshape((-1,) + spatial)
    metrics = metrics_from_counts(counts, thresholds, inter, union, want_maps, kwargs.get("store_iou"))
    logger.info("%s", {k: {kk: vv for kk, vv in v["rsc_0"].items() if kk != "IOU"} for k, v in metrics.items()})
    return metrics


def _skeleton(mask, device):
    from . import backend
    m = np.asarray(mask) != 0
    if m.ndim not in (2, 3):
        raise ValueError("the skeleton needs a 2-d or 3-d mask, got shape %s" % (m.shape,))
    return np.asarray(backend.skeletonize_3d(m) if device else backend.host_skeletonize_3d(m)).astype(bool)


def _skeleton_scores(gt_mask, pred_mask, device):
    """evaluate_prediction.py:201-223 / :318-337: (tp, precision, recall, f1, num_gt_skel, num_pred_skel)"""
    gt_mask, pred_mask = np.asarray(gt_mask) != 0, np.asarray(pred_mask) != 0
    gt_sk, pred_sk = _skeleton(gt_mask, device), _skeleton(pred_mask, device)
    tp = float(np.sum(np.logical_and(gt_sk, pred_mask)))
    if np.sum(pred_sk) > 0 and tp > 0:
        precision = tp / (tp + float(np.sum(np.logical_and(np.logical_not(gt_mask), pred_sk))))
        recall = tp / (tp + float(np.sum(np.logical_and(gt_sk, np.logical_not(pred_mask)))))
        f1 = 2 * (precision * recall) / (precision + recall)
    else:
        precision = recall = f1 = 0
    return tp, precision, recall, f1


def _plain_scores(num_gt, num_pred, tp):
    if num_pred > 0 and tp > 0:
        precision = tp / float(num_pred)
        recall = tp / float(num_gt)
        return precision, recall, 2 * (precision * recall) / (precision + recall)
    return 0, 0, 0


def remove_small_components_host(mask, compsize):
    """`ndimage.label(mask, np.ones((3, 3, 3)))`, `remove_small_components(.., compsize)`, `> 0`
    (evaluate_prediction.py:311-313): components of AT MOST compsize voxels go (`counts <= compsize`)."""
    from scipy import ndimage
    mask = np.asarray(mask)
    if mask.ndim != 3:
        raise ValueError("remove_small_comps > 0 needs a 3-d mask (the 3 x 3 x 3 structure), got shape %s" % (mask.shape,))
    lab, n = ndimage.label(mask, np.ones((3, 3, 3)))
    counts = np.bincount(lab.reshape(-1), minlength=n + 1)
    keep = counts > compsize
    keep[0] = False
    return keep[lab]


def evaluate_fg(prediction_fn, label_fn, **kwargs):
    """evaluate_prediction.py:258-371.  The foreground is `fg_key`, or the centre channel of `aff_key`;
    thresholded with NumPy on the host (one volume), then, with a device, filtered by `ppp_post_clean_mask`
    (26-connected) and counted with torch; `evaluate_skeleton_coverage` thins with `ppp_skeletonize_3d` --
    the library's own thinning, parity with scikit-image's skeletonize_3d unpinned, as for
    skeletonize_backend = "ppp".  Counts come back as Python ints."""
    _refuse_png(kwargs)
    if not prediction_fn.rstrip("/").endswith(("zarr", "hdf")):
        raise NotImplementedError(prediction_fn)
    with io_hdflike.open_container(prediction_fn, "r") as inf:
        if kwargs.get("fg_key") is None:
            mid = int(np.prod(kwargs["patchshape"]) / 2)
            pred = np.squeeze(np.array(inf[kwargs["aff_key"]][mid]))
        else:
            pred = np.squeeze(np.array(inf[kwargs["fg_key"]]))
    labels = _read_labels(label_fn, kwargs["sample_gt_key"])
    gt_mask = np.max(labels > 0, axis=0).astype(np.uint8)
    threshs = kwargs.get("eval_fg_thresholds", [0.9])
    rm_comps = sorted(kwargs.get("remove_small_comps") or [0])
    if any(r > 0 for r in rm_comps) and pred.ndim != 3:
        raise ValueError("remove_small_comps > 0 needs a 3-d foreground (the 3 x 3 x 3 structure), got shape %s"
                         % (pred.shape,))
    if gt_mask.shape != pred.shape:
        raise ValueError("ground truth %s and foreground %s differ in shape" % (gt_mask.shape, pred.shape))
    device = use_device()
    skeleton = bool(kwargs.get("evaluate_skeleton_coverage"))
    if device:
        import torch
        from . import backend
        d_gt = torch.from_numpy(gt_mask).cuda() != 0
    num_gt = int(np.sum(gt_mask))
    metrics = {}
    for thresh in threshs:
        metrics[thresh_key(thresh)] = {}
        pred_mask = pred > thresh
        d_mask = torch.from_numpy(pred_mask.astype(np.uint8)).cuda() if device else None
        for rm_comp in rm_comps:
            if rm_comp > 0:
                if device:
                    d_mask = backend.post_clean_mask(d_mask.contiguous(), FULL_STRUCTURE, int(rm_comp))[0]
                else:
                    pred_mask = remove_small_components_host(pred_mask, rm_comp)
            if device:
                num_pred = int((d_mask != 0).sum())
                tp = int(((d_mask != 0) & d_gt).sum())
                if skeleton:
                    pred_mask = d_mask.cpu().numpy() != 0
            else:
                num_pred = int(np.sum(pred_mask))
                tp = int(np.sum(np.logical_and(gt_mask, pred_mask)))
            if skeleton:
                tp, precision, recall, f1 = _skeleton_scores(gt_mask, pred_mask, device)
            else:
                precision, recall, f1 = _plain_scores(num_gt, num_pred, tp)
            metrics[thresh_key(thresh)]["rsc_" + str(int(rm_comp))] = {
                "num_gt": num_gt, "num_pred": num_pred, "num_tp": tp,
                "precision": precision, "recall": recall, "f1": f1}
    return metrics


def evaluate_numinst(prediction_fn, label_fn, **kwargs):
    """evaluate_prediction.py:153-255: `argmax` of the numinst probabilities, or the `numinst_threshs` ladder,
    `max_numinst` clipping, one entry per value of np.unique(gt_numinst).  The classification and the counts
    are NumPy on the host (one small volume per class); `evaluate_skeleton_coverage` thins on the device
    when there is one (unpinned against scikit-image, as in evaluate_fg)."""
    _refuse_png(kwargs)
    if not prediction_fn.rstrip("/").endswith(("zarr", "hdf")):
        raise NotImplementedError(prediction_fn)
    with io_hdflike.open_container(prediction_fn, "r") as inf:
        prob = np.squeeze(np.array(inf[kwargs.get("numinst_key", kwargs.get("fg_key"))]))
    labels = _read_labels(label_fn, kwargs["sample_gt_key"])
    gt_numinst = np.sum(labels > 0, axis=0).astype(np.uint8)
    if kwargs.get("numinst_threshs"):
        pred_numinst = np.zeros(prob.shape[1:], dtype=np.uint8)
        for i in range(len(kwargs["numinst_threshs"])):
            pred_numinst[prob[i + 1] > kwargs["numinst_threshs"][i]] = i + 1
    else:
        pred_numinst = np.argmax(prob, axis=0).astype(np.uint8)
    if kwargs.get("max_numinst") is not None:
        gt_numinst = np.clip(gt_numinst, 0, kwargs["max_numinst"])
        pred_numinst = np.clip(pred_numinst, 0, kwargs["max_numinst"])
    if gt_numinst.shape != pred_numinst.shape:
        raise ValueError("ground truth %s and numinst prediction %s differ in shape"
                         % (gt_numinst.shape, pred_numinst.shape))
    device = use_device()
    metrics = {}
    for i in np.unique(gt_numinst):
        gt_mask, pred_mask = gt_numinst == i, pred_numinst == i
        num_gt, num_pred = int(np.sum(gt_mask)), int(np.sum(pred_mask))
        if kwargs.get("evaluate_skeleton_coverage") and i > 0:
            tp, precision, recall, f1 = _skeleton_scores(gt_mask, pred_mask, device)
        else:
            tp = int(np.sum(np.logical_and(gt_mask, pred_mask)))
            precision, recall, f1 = _plain_scores(num_gt, num_pred, tp)
        metrics[str(int(i))] = {"num_gt": num_gt, "num_pred": num_pred, "num_tp": tp,
                                "precision": precision, "recall": recall, "f1": f1}
    return metrics


# ----------------------------------------------------------------------------------------
# the task (run_ppp.py:1300-1443)
# ----------------------------------------------------------------------------------------
def store_iou_datasets(pred_fn, patch_metric, thresholds):
    """run_ppp.py:1347-1366: `volumes/<thresh_key>/IOU` (float64) into the prediction file, an existing
    dataset replaced first."""
    with io_hdflike.open_container(pred_fn, "a") as outfl:
        for th in thresholds:
            key = "volumes/{}/IOU".format(thresh_key(th))
            iou = patch_metric[thresh_key(th)]["rsc_0"]["IOU"]
            if pred_fn.rstrip("/").endswith("hdf"):
                try:
                    del outfl[key]
                except KeyError:
                    pass
                outfl.create_dataset(key, data=iou, compression="gzip")
            else:
                outfl.create_dataset(key, data=iou, overwrite=True)


def evaluate_prediction_sample(config, sample, data, pred_folder, file_format, output_folder):
    """run_ppp.py:1300-1367: the three dicts merged in the reference's order with dict.update (a threshold key
    shared by fg and patch metrics keeps the patch entry, as there)."""
    logger.info("evaluating prediction %s", sample)
    pred_fn = os.path.join(pred_folder, sample + "." + file_format)
    if data.rstrip("/").endswith(("zarr", "hdf")):
        label_fn, sample_gt_key = data, sample + "/" + config["data"]["gt_key"]
    else:
        label_fn = os.path.join(data, sample + "." + config["data"]["input_format"])
        sample_gt_key = config["data"]["gt_key"]
    cfg = config["evaluation"]["prediction"]
    common = dict(cfg)
    for section in ("model", "prediction", "data"):
        for k, v in config.get(section, {}).items():
            if k in common:
                raise TypeError("evaluate_prediction got multiple values for keyword argument %r" % k)
            common[k] = v
    metric = {}
    if cfg.get("eval_numinst_prediction"):
        metric.update(evaluate_numinst(pred_fn, label_fn, sample_gt_key=sample_gt_key, output_folder=output_folder,
                                       numinst_threshs=config.get("vote_instances", {}).get("numinst_threshs"), **common))
    if cfg.get("eval_fg_prediction"):
        metric.update(evaluate_fg(pred_fn, label_fn, sample_gt_key=sample_gt_key, output_folder=output_folder, **common))
    if cfg.get("eval_patch_prediction"):
        patch_metric = evaluate_patch(pred_fn, label_fn, sample_gt_key=sample_gt_key, **common)
        metric.update(patch_metric)
        if cfg.get("store_iou"):
            if file_format not in ("zarr", "hdf"):
                raise RuntimeError("invalid file format")
            store_iou_datasets(pred_fn, patch_metric, cfg["eval_patch_thresholds"])
    return metric


def jsonable(metric):
    """a sample's metric dict for prediction_metrics.json: NumPy scalars as Python numbers, IOU arrays left out"""
    if isinstance(metric, dict):
        return {str(k): jsonable(v) for k, v in metric.items() if not (k == "IOU" and isinstance(v, np.ndarray))}
    if isinstance(metric, np.generic):
        return metric.item()
    return metric


def summarize(metric_dicts, samples, metric_name):
    """run_ppp.py:1400-1443: per `<thresh_key>_<rsc_key>` the mean of `metric_name` over the samples, logged
    with the best one.  Returns (metrics, ths).  Entries that are no dicts (evaluate_numinst's are one level
    flatter; the reference's loop fails on them) are passed over."""
    reordered = {}
    for sample_metric in metric_dicts:
        for th_key, v1 in sample_metric.items():
            for rsc_key, v2 in v1.items():
                if isinstance(v2, dict):
                    reordered.setdefault(th_key + "_" + rsc_key, []).append(v2)
    metrics, ths = [], []
    for th, dicts in reordered.items():
        values = []
        for metric_dict, sample in zip(dicts, samples):
            for k in metric_name.split("."):
                if isinstance(metric_dict, dict) and k in metric_dict:
                    metric_dict = metric_dict[k]
            if isinstance(metric_dict, dict):
                logger.info("%s sample has no overlap/check metric", sample)
            else:
                logger.info("%s sample %-19s: %.4f", metric_name, sample, float(metric_dict))
                values.append(float(metric_dict))
        with _quiet_empty_mean():
            metric = np.mean(values)
        metrics.append(metric)
        ths.append(th)
        logger.info("%s: %.4f (%s)", metric_name, metric, th)
    logger.info("%s", metrics)
    logger.info("%s", ths)
    if metrics:
        logger.info("best %s: %.4f (%s)", metric_name, np.max(metrics), ths[int(np.argmax(metrics))])
    return metrics, ths
