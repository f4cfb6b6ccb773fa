"""The `evaluate` step (reference: experiments/run_ppp.py:1193-1262 and :1447-1536): the voted instance map
scored against the ground-truth instances, under the name and kwargs of the reference's call site
(`evaluate_file`, run_ppp.py:1239-1262).

Parity with `evaluate-instance-segmentation` is UNPINNED because the package is absent: the reference does
not vendor it (its setup.py:28 names it as a dependency), so there is no program text to restate and nothing
to generate golden vectors from.  What this module computes is DEFINED here and in DESIGN.md §7.16, once in
NumPy (`overlap_counts_host` and the metric layer, all of it host code on integer rows), and the device path
(`ppp_label_overlap`, csrc/ppp_overlap.hip) is pinned to that definition integer for integer.

The heavy part of every metric is the contingency table of two label stacks.  For A (La, ...) and B (Lb, ...),
0 = background, `overlap_counts*` return rows (a, b) uint32 [n, 2] with counts int64 [n]:

  (a, b), a != 0 and b != 0 :  #{(i, j, v) : A[i][v] == a and B[j][v] == b}
  (a, 0)                    :  #{(i, v) : A[i][v] == a}              (the size of a)
  (0, b)                    :  #{(j, v) : B[j][v] == b}              (the size of b)

without zero counts, sorted ascending by (a, b).  Everything below is float64 arithmetic on the host from
these integers; a ratio with a zero denominator is 0.

Inputs.  `pred` and `gt` are integer arrays (Z, Y, X) or (L, Z, Y, X); a 3-d array is ONE channel, whatever
`overlapping_inst` says (2-d results with one instance per channel go in as (L, 1, Y, X)).  2-d data is given a
leading unit z.  Values outside [0, 2^32) and spatial shapes
that differ (whatever `keep_gt_shape` says) raise ValueError.

remove_small_components = n.  Predicted ids with at most n voxels, counted over all channels, are removed
before anything else (`ppp_post_compact_ids` without relabel on the device path, np.unique on the host).

Num GT, Num Pred: the numbers of distinct non-zero ids.  g runs over the gt ids, p over the predicted ids,
n_gp is the pair count of overlap(gt, pred), |g| and |p| the sizes.

localization_criterion = "iou":    score[g, p] = n_gp / (|g| + |p| - n_gp).
localization_criterion = "cldice" (3-d only; a unit z raises NotImplementedError): Sp is the per-instance
  skeleton of pred and Sg that of gt, channel by channel (`ppp_skeletonize_labels` on the device, the host
  loop `postprocess.skeletonize_instances` otherwise; the library's own thinning, itself unpinned against
  scikit-image).  clPrec[g, p] = |Sp_p & g| / |Sp_p| from overlap(gt, Sp), clRec[g, p] = |Sg_g & p| / |Sg_g|
  from overlap(Sg, pred), score = 2 clPrec clRec / (clPrec + clRec).  The thinning keeps at least one voxel
  of every instance; that is asserted.

Thresholds th = 0.1 ... 0.9, keys confusion_matrix.th_0_1 ... th_0_9 (`evaluate_prediction.thresh_key`).
Candidate pairs: score > th.
  assignment_strategy = "greedy": candidates in descending score, ties by ascending (g, p); a pair is taken
    when both ids are still free.
  "hungarian", or use_linear_sum_assignment = True: scipy.optimize.linear_sum_assignment maximising the
    summed score over the candidate matrix, non-candidates weighted 0; assigned non-candidates are dropped.
  AP_TP = pairs taken, AP_FP = Num Pred - TP, AP_FN = Num GT - TP, precision = TP / (TP + FP),
  recall = TP / (TP + FN), fscore = 2 TP / (2 TP + FP + FN), AP = TP / (TP + FP + FN).
confusion_matrix.avFscore and .avAP: the means of fscore and AP over the nine thresholds.

evaluate_false_labels.  prec, rec = clPrec, clRec under cldice; n_gp / |p| and n_gp / |g| under iou.
  false_merge = sum over p of max(0, #{g : rec[g, p] > th} - 1),
  false_split = sum over g of max(0, #{p : prec[g, p] > th} - 1), per threshold.

general.avg_gt_skel_coverage (cldice only).  Every p is assigned to argmax_g clPrec[g, p] when that maximum
  is > 0, ties to the lowest g; cov[g] = min(1, sum over the p assigned to g of clRec[g, p]); the metric is
  the mean of cov over all gt ids.  It is the SUM of the parts, not the size of their union: predicted
  channels that overlap can cover a skeleton voxel twice, which is why cov is capped at 1.
general.avg_f1_cov_score = 0.5 avFscore + 0.5 avg_gt_skel_coverage.
avg_tp_skel_coverage (multi-threshold, cldice only): per threshold the mean of cov[g] over the gt ids that
  are TP at that threshold; 0 with none.

The dispatch rule is the post-steps' (`postprocess.use_device`).  The table costs La Lb + La + Lb key streams per
voxel on either path (and B is read once per channel of A on the device): maps with hundreds of channels a side
are slow, and beyond 65535 streams the device entry point refuses; there is no switch to the host for them."""
import logging
import os
import re

import numpy as np

from .evaluate_prediction import thresh_key
from .vote_instances import io_hdflike

logger = logging.getLogger(__name__)

THRESHOLDS = tuple(round(0.1 * k, 1) for k in range(1, 10))
GENERAL_METRICS = ("avg_gt_skel_coverage", "avg_f1_cov_score")
MULTI_THRESH_METRICS = ("avg_tp_skel_coverage",)


def use_device():
    from . import postprocess
    return postprocess.use_device()


def _is_tensor(a):
    return type(a).__module__.startswith("torch") and hasattr(a, "is_cuda")


# ----------------------------------------------------------------------------------------
# the contingency table
# ----------------------------------------------------------------------------------------
def _stack_u32(x, who):
    """an integer array with the leading channel axis as contiguous uint32, its values checked"""
    x = np.asarray(x)
    if x.ndim < 1 or x.shape[0] < 1:
        raise ValueError("%s needs the leading channel axis with at least one channel, got shape %s" % (who, x.shape))
    if not (np.issubdtype(x.dtype, np.integer) or x.dtype == np.bool_):
        raise ValueError("%s must hold integers, got %s" % (who, x.dtype))
    if x.size and (int(x.min()) < 0 or int(x.max()) >= 1 << 32):
        raise ValueError("%s: ids must lie in [0, 2^32)" % who)
    return np.ascontiguousarray(x.astype(np.uint32, copy=False))


def overlap_counts_host(a, b):
    """The definition in NumPy: `a` (La, ...) and `b` (Lb, ...) integer arrays of equal spatial shape.  Returns
    (rows uint32 [n, 2], counts int64 [n]); see the module docstring."""
    a, b = _stack_u32(a, "a"), _stack_u32(b, "b")
    if a.shape[1:] != b.shape[1:]:
        raise ValueError("the stacks differ in spatial shape: %s and %s" % (a.shape[1:], b.shape[1:]))
    A, B = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    keys, counts = [], []

    def add(k):
        u, c = np.unique(k, return_counts=True)
        keys.append(u)
        counts.append(c.astype(np.int64))
    add(A[A != 0].astype(np.uint64) << np.uint64(32))
    add(B[B != 0].astype(np.uint64))
    for i in range(A.shape[0]):
        for j in range(B.shape[0]):
            m = (A[i] != 0) & (B[j] != 0)
            add((A[i][m].astype(np.uint64) << np.uint64(32)) | B[j][m].astype(np.uint64))
    u, inverse = np.unique(np.concatenate(keys), return_inverse=True)
    total = np.zeros(len(u), dtype=np.int64)
    np.add.at(total, inverse.reshape(-1), np.concatenate(counts))
    rows = np.stack([(u >> np.uint64(32)).astype(np.uint32), (u & np.uint64(0xFFFFFFFF)).astype(np.uint32)], axis=1)
    return rows.reshape(-1, 2), total


def overlap_counts_device(a, b):
    """`overlap_counts_host` from the device (backend.label_overlap = ppp_label_overlap): NumPy arrays or
    device tensors in, the same host arrays out."""
    import torch
    from . import backend

    def up(x, who):
        if _is_tensor(x):
            return x.reshape(x.shape[0], 1, 1, -1)
        x = _stack_u32(x, who)
        return torch.from_numpy(x.view(np.int32)).cuda().reshape(x.shape[0], 1, 1, -1)
    ta, tb = up(a, "a"), up(b, "b")
    if ta.shape[1:] != tb.shape[1:]:
        raise ValueError("the stacks differ in spatial shape")
    return backend.label_overlap(ta, tb)


def overlap_counts(a, b):
    """the contingency table by the dispatch rule"""
    if use_device() and int(np.prod(np.shape(a)[1:])) < 1 << 31:
        return overlap_counts_device(a, b)
    if _is_tensor(a):
        a = a.cpu().numpy().view(np.uint32)
    if _is_tensor(b):
        b = b.cpu().numpy().view(np.uint32)
    return overlap_counts_host(a, b)


class _Table:
    """rows of overlap(A, B) as ids, sizes and the dense pair matrix n[a, b]"""

    def __init__(self, rows, counts):
        rows, counts = np.asarray(rows).reshape(-1, 2), np.asarray(counts, dtype=np.int64)
        ma, mb = rows[:, 1] == 0, rows[:, 0] == 0
        self.a_ids, self.a_size = rows[ma, 0], counts[ma]
        self.b_ids, self.b_size = rows[mb, 1], counts[mb]
        pair = ~(ma | mb)
        self.n = np.zeros((len(self.a_ids), len(self.b_ids)), dtype=np.int64)
        self.n[np.searchsorted(self.a_ids, rows[pair, 0]), np.searchsorted(self.b_ids, rows[pair, 1])] = counts[pair]


def _ratio(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    den = np.broadcast_to(den, num.shape)
    out = np.zeros(num.shape, dtype=np.float64)
    np.divide(num, den, out=out, where=den != 0)
    return out


# ----------------------------------------------------------------------------------------
# the metric layer
# ----------------------------------------------------------------------------------------
def _prepare(x, who):
    x = x.cpu().numpy() if _is_tensor(x) else np.asarray(x)
    if x.ndim == 2:
        x = x[None, None]
    elif x.ndim == 3:
        x = x[None]
    elif x.ndim != 4:
        raise ValueError("%s of shape %s: (Z, Y, X) or (L, Z, Y, X) is needed" % (who, x.shape))
    return _stack_u32(x, who)


def _skeletons(stack):
    """the per-instance skeleton of every channel, by the dispatch rule"""
    from . import postprocess
    return np.stack([np.asarray(postprocess.instance_skeletons(ch)[0]) for ch in stack])


def _assign(score, th, hungarian):
    """the (g, p) index pairs taken at threshold th"""
    cand = score > th
    if not cand.any():
        return []
    if hungarian:
        from scipy.optimize import linear_sum_assignment
        gi, pi = linear_sum_assignment(np.where(cand, score, 0.0), maximize=True)
        return [(int(g), int(p)) for g, p in zip(gi, pi) if cand[g, p]]
    gi, pi = np.nonzero(cand)
    order = np.lexsort((pi, gi, -score[gi, pi]))
    g_free, p_free = np.ones(score.shape[0], dtype=bool), np.ones(score.shape[1], dtype=bool)
    taken = []
    for k in order:
        g, p = int(gi[k]), int(pi[k])
        if g_free[g] and p_free[p]:
            g_free[g] = p_free[p] = False
            taken.append((g, p))
    return taken


def _refuse(kwargs, add_general_metrics, add_multi_thresh_metrics):
    for name in ("visualize", "partly", "foreground_only", "unique_false_labels"):
        if kwargs.get(name):
            raise NotImplementedError("%s = True is not provided by this repository; unset it" % name)
    if kwargs.get("filterSz"):
        raise NotImplementedError("filterSz = %r is not provided by this repository; unset it" % (kwargs["filterSz"],))
    if kwargs.get("evaluate_skeleton_coverage"):
        raise NotImplementedError("evaluate_skeleton_coverage is not provided by this repository; unset it")
    for name in add_general_metrics or []:
        if name not in GENERAL_METRICS:
            raise NotImplementedError("add_general_metrics: %r is not provided (known: %s)" % (name, ", ".join(GENERAL_METRICS)))
    for name in add_multi_thresh_metrics or []:
        if name not in MULTI_THRESH_METRICS:
            raise NotImplementedError("add_multi_thresh_metrics: %r is not provided (known: %s)"
                                      % (name, ", ".join(MULTI_THRESH_METRICS)))
    known = ("visualize", "partly", "foreground_only", "unique_false_labels", "filterSz", "evaluate_skeleton_coverage",
             "debug", "visualize_type")
    for name in kwargs:
        if name not in known:
            raise TypeError("evaluate_instances: unexpected keyword argument %r" % name)


def evaluate_volumes(pred, gt, overlapping_inst=False, use_linear_sum_assignment=False, localization_criterion="iou",
                     assignment_strategy="hungarian", remove_small_components=None, keep_gt_shape=False,
                     evaluate_false_labels=False, add_general_metrics=(), add_multi_thresh_metrics=(), metric=None,
                     **kwargs):
    """The nested metric dict of a predicted and a ground-truth instance map (module docstring): plain Python
    ints and floats under "general" and "confusion_matrix"."""
    _refuse(kwargs, add_general_metrics, add_multi_thresh_metrics)
    if localization_criterion not in ("iou", "cldice"):
        raise NotImplementedError("localization_criterion = %r is not provided (iou, cldice)" % (localization_criterion,))
    if assignment_strategy not in ("greedy", "hungarian"):
        raise NotImplementedError("assignment_strategy = %r is not provided (greedy, hungarian)" % (assignment_strategy,))
    cldice = localization_criterion == "cldice"
    wanted = list(add_general_metrics or []) + list(add_multi_thresh_metrics or [])
    if wanted and not cldice:
        raise NotImplementedError("%s needs localization_criterion = \"cldice\"" % wanted[0])
    pred, gt = _prepare(pred, "pred"), _prepare(gt, "gt")
    if pred.shape[1:] != gt.shape[1:]:
        raise ValueError("prediction %s and ground truth %s differ in spatial shape" % (pred.shape[1:], gt.shape[1:]))
    if cldice and pred.shape[1] == 1:
        raise NotImplementedError("localization_criterion = \"cldice\" needs 3-d data (the thinning is 3-d)")
    if remove_small_components is not None:
        from . import postprocess
        if use_device() and pred.size < 1 << 31:
            pred = np.asarray(postprocess.remove_small_components_device(pred, remove_small_components))
        else:
            pred = postprocess.remove_small_components(pred, remove_small_components)

    if cldice:
        t_prec = _Table(*overlap_counts(gt, _skeletons(pred)))      # n[g, p] = |Sp_p & g|, b_size = |Sp_p|
        t_rec = _Table(*overlap_counts(_skeletons(gt), pred))       # n[g, p] = |Sg_g & p|, a_size = |Sg_g|
        assert np.array_equal(t_prec.a_ids, t_rec.a_ids) and np.array_equal(t_prec.b_ids, t_rec.b_ids), \
            "an instance lost its skeleton: the thinning keeps at least one voxel"
        prec = _ratio(t_prec.n, t_prec.b_size[None, :])
        rec = _ratio(t_rec.n, t_rec.a_size[:, None])
        score = _ratio(2.0 * prec * rec, prec + rec)
        num_gt, num_pred = len(t_rec.a_ids), len(t_rec.b_ids)
    else:
        t = _Table(*overlap_counts(gt, pred))
        score = _ratio(t.n, t.a_size[:, None] + t.b_size[None, :] - t.n)
        prec, rec = _ratio(t.n, t.b_size[None, :]), _ratio(t.n, t.a_size[:, None])
        num_gt, num_pred = len(t.a_ids), len(t.b_ids)

    cov = None
    if cldice:
        cov = np.zeros(num_gt, dtype=np.float64)
        if num_gt and num_pred:
            best = np.argmax(prec, axis=0)                           # (the first maximum: the lowest g)
            for p in range(num_pred):
                if prec[best[p], p] > 0:
                    cov[best[p]] += rec[best[p], p]
            cov = np.minimum(cov, 1.0)

    hungarian = bool(use_linear_sum_assignment) or assignment_strategy == "hungarian"
    cm = {}
    fscores, aps = [], []
    for th in THRESHOLDS:
        taken = _assign(score, th, hungarian)
        tp = len(taken)
        fp, fn = num_pred - tp, num_gt - tp
        entry = {"AP_TP": tp, "AP_FP": fp, "AP_FN": fn,
                 "precision": float(_ratio(tp, tp + fp)), "recall": float(_ratio(tp, tp + fn)),
                 "fscore": float(_ratio(2 * tp, 2 * tp + fp + fn)), "AP": float(_ratio(tp, tp + fp + fn))}
        if evaluate_false_labels:
            entry["false_merge"] = int(np.maximum((rec > th).sum(axis=0) - 1, 0).sum())
            entry["false_split"] = int(np.maximum((prec > th).sum(axis=1) - 1, 0).sum())
        if "avg_tp_skel_coverage" in (add_multi_thresh_metrics or []):
            entry["avg_tp_skel_coverage"] = float(np.mean([cov[g] for g, _ in taken])) if taken else 0.0
        fscores.append(entry["fscore"])
        aps.append(entry["AP"])
        cm["th_" + thresh_key(th)] = entry
    cm["avFscore"] = float(np.mean(fscores))
    cm["avAP"] = float(np.mean(aps))
    general = {"Num GT": int(num_gt), "Num Pred": int(num_pred)}
    if any(m in GENERAL_METRICS for m in (add_general_metrics or [])):
        coverage = float(np.mean(cov)) if num_gt else 0.0
        general["avg_gt_skel_coverage"] = coverage
        if "avg_f1_cov_score" in add_general_metrics:
            general["avg_f1_cov_score"] = 0.5 * cm["avFscore"] + 0.5 * coverage
    return {"general": general, "confusion_matrix": cm}


# ----------------------------------------------------------------------------------------
# the result file
# ----------------------------------------------------------------------------------------
_BARE_KEY = re.compile(r"^[A-Za-z0-9_-]+$")


def _toml_key(k):
    k = str(k)
    return k if _BARE_KEY.match(k) else '"%s"' % k.replace("\\", "\\\\").replace('"', '\\"')


def _toml_value(v):
    if isinstance(v, (bool, np.bool_)):
        return "true" if v else "false"
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    if isinstance(v, (float, np.floating)):
        return repr(float(v))
    if isinstance(v, str):
        return '"%s"' % v.replace("\\", "\\\\").replace('"', '\\"').replace("\n", "\\n")
    raise TypeError("no TOML form for %r" % (v,))


def toml_dumps(d, _path=()):
    """A nested dict of str / int / float / bool as TOML: the values of a table first, then its sub-tables
    under their dotted headers; floats by repr, so they read back bit for bit."""
    lines = []
    if _path:
        lines.append("[%s]" % ".".join(_toml_key(k) for k in _path))
    for k, v in d.items():
        if not isinstance(v, dict):
            lines.append("%s = %s" % (_toml_key(k), _toml_value(v)))
    out = "\n".join(lines) + ("\n" if lines else "")
    for k, v in d.items():
        if isinstance(v, dict):
            out += ("\n" if out else "") + toml_dumps(v, _path + (k,))
    return out


def _read_dataset(fn, key):
    if not fn.rstrip("/").endswith(("zarr", "hdf")):
        raise NotImplementedError("%s: .hdf and .zarr are read" % fn)
    with io_hdflike.open_container(fn, "r") as inf:
        return np.array(inf[key])


def evaluate_file(res_file, gt_file, res_key=None, gt_key=None, out_dir=None, suffix="", from_scratch=False,
                  overlapping_inst=False, use_linear_sum_assignment=False, localization_criterion="iou",
                  assignment_strategy="hungarian", remove_small_components=None, keep_gt_shape=False,
                  evaluate_false_labels=False, add_general_metrics=[], add_multi_thresh_metrics=[], metric=None,
                  **kwargs):
    """`evaluate_volumes` of ``res_file[res_key]`` against ``gt_file[gt_key]`` (``.hdf`` / ``.zarr``).  The dict is
    written to ``<out_dir>/<sample><suffix>.toml`` (`toml_dumps`; out_dir defaults to the result file's folder) and
    returned; with ``from_scratch = False`` and that file present it is read back instead of computed.  Kwargs
    this project does not serve are refused by name (module docstring); ``debug`` is accepted and ignored."""
    from .run_ppp import load_config
    _refuse(kwargs, add_general_metrics, add_multi_thresh_metrics)
    sample = os.path.splitext(os.path.basename(res_file.rstrip("/")))[0]
    out_dir = os.path.dirname(os.path.abspath(res_file.rstrip("/"))) if out_dir is None else out_dir
    out_fn = os.path.join(out_dir, sample + suffix + ".toml")
    if not from_scratch and os.path.exists(out_fn):
        logger.info("%s exists: read back (from_scratch = false)", out_fn)
        return load_config([out_fn])
    metrics = evaluate_volumes(_read_dataset(res_file, res_key), _read_dataset(gt_file, gt_key),
                               overlapping_inst=overlapping_inst, use_linear_sum_assignment=use_linear_sum_assignment,
                               localization_criterion=localization_criterion, assignment_strategy=assignment_strategy,
                               remove_small_components=remove_small_components, keep_gt_shape=keep_gt_shape,
                               evaluate_false_labels=evaluate_false_labels, add_general_metrics=add_general_metrics,
                               add_multi_thresh_metrics=add_multi_thresh_metrics, metric=metric, **kwargs)
    os.makedirs(out_dir, exist_ok=True)
    with open(out_fn, "w") as f:
        f.write(toml_dumps(metrics))
    return metrics


def lookup(metrics, dotted):
    """the value under a dotted key, e.g. confusion_matrix.th_0_5.fscore"""
    for k in dotted.split("."):
        metrics = metrics[k]
    return metrics
