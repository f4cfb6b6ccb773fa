#!/usr/bin/env python3
"""tests/golden/eval_prediction/*.npz (a folder of their own: tests/conftest.py takes every *.npz directly under
tests/golden that it does not know by prefix for a vote_instances golden): the reference's own `evaluate_patch`,
`evaluate_fg` and `evaluate_numinst` (PatchPerPix/evaluate/evaluate_prediction.py, imported in place) on small
inputs.  Stubs stand in for zarr, h5py (a dict of arrays behind `File`), skimage, matplotlib, joblib, neurolight,
colorcet and nrrd; `gunpowder.add_affinities.seg_to_affgraph*`, which evaluate_patch calls, is served by the
reference's own restatement of it, util/train_util.py:523-695 (`seg_to_affgraph_*_torch`, on the CPU) -- gunpowder
itself is not on the development container.  `PatchPerPix.util.remove_small_components` is the reference's
util/postprocess.py function, loaded in place.  Every sample is read as `.hdf`: the zarr branch of evaluate_patch
cannot run as written.  Development container only.

  python tests/golden/gen_golden_eval_prediction.py

A file holds the datasets of the prediction file (`pred/<key>`) and of the label file (`gt/<key>`), and `runs`: a
JSON list of {"fn", "kwargs", "metrics"} with the metrics' scalars; a stored IOU array is the entry
`IOU/<run index>/<thresh_key>`.  The generator asserts that each case exercises what it is for (see `check_patch`,
`fg_case`, `numinst_case`) and that this project's host definition gives the same metrics."""
import contextlib
import importlib.util
import io
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "eval_prediction")
REF = "/root/reference/PatchPerPix"

STORE = {}          # "file name" -> {key: array}: what the stubbed h5py.File hands out


class FileStub:
    def __init__(self, fn, mode="r"):
        self.sets = STORE[fn]

    def __enter__(self):
        return self.sets

    def __exit__(self, *exc):
        return False


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    import torch
    for name in ("colorcet", "skimage", "skimage.morphology", "skimage.io", "zarr", "h5py", "nrrd", "joblib",
                 "matplotlib", "matplotlib.pyplot", "gunpowder", "gunpowder.add_affinities", "neurolight",
                 "neurolight.gunpowder", "PatchPerPix", "PatchPerPix.util"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["skimage.morphology"].skeletonize_3d = None
    sys.modules["skimage"].io = sys.modules["skimage.io"]
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["joblib"].Parallel = sys.modules["joblib"].delayed = None
    sys.modules["h5py"].File = FileStub
    sys.modules["neurolight"].gunpowder = sys.modules["neurolight.gunpowder"]
    gp = sys.modules["gunpowder"]
    gp.add_affinities = sys.modules["gunpowder.add_affinities"]
    tu = _load("ppp_ref_train_util", os.path.join(REF, "util", "train_util.py"))

    def serve(fn):
        def call(seg, nhood):
            seg = torch.from_numpy(np.ascontiguousarray(seg).astype(np.int64))[None]
            return fn(seg, np.asarray(nhood), "cpu")[0].numpy()
        return call
    gp.add_affinities.seg_to_affgraph = serve(tu.seg_to_affgraph_3d_torch)
    gp.add_affinities.seg_to_affgraph_2d = serve(tu.seg_to_affgraph_2d_torch)
    gp.add_affinities.seg_to_affgraph_3d_multi = serve(tu.seg_to_affgraph_3d_multi_torch)
    gp.add_affinities.seg_to_affgraph_2d_multi = serve(tu.seg_to_affgraph_2d_multi_torch)
    post = _load("ppp_ref_postprocess", os.path.join(REF, "util", "postprocess.py"))
    sys.modules["PatchPerPix.util"].remove_small_components = post.remove_small_components
    return _load("ppp_ref_evaluate_prediction", os.path.join(REF, "evaluate", "evaluate_prediction.py"))


def scalars(metrics):
    """the metrics as JSON-able numbers, IOU arrays taken out: (dict, {thresh_key: IOU})"""
    ious = {}

    def walk(d, top=None):
        out = {}
        for k, v in d.items():
            if isinstance(v, dict):
                out[k] = walk(v, top if top is not None else k)
            elif isinstance(v, np.ndarray):
                assert k == "IOU" and v.dtype == np.float64
                ious[top] = v
            else:
                out[k] = v.item() if isinstance(v, np.generic) else v
        return out
    return walk(metrics), ious


def run(ref, fn, sample, kwargs):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(invalid="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            return getattr(ref, fn)(sample + ".hdf", sample + "_gt.hdf", **kwargs)


# ----------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------
def make_labels(rng, L, spatial, n_inst):
    """random boxes, each put into the first channel in which it covers no earlier instance; L > 1: the
    later channels receive the boxes that overlap, so overlap voxels exist.  One channel may stay empty."""
    labels = np.zeros((L,) + spatial, dtype=np.int32)
    for lbl in range(1, n_inst + 1):
        lo = [int(rng.integers(0, max(1, s - 2))) for s in spatial]
        hi = [min(s, a + int(rng.integers(2, 5))) for a, s in zip(lo, spatial)]
        box = tuple(slice(a, b) for a, b in zip(lo, hi))
        for c in range(L):
            if not labels[c][box].any():
                labels[c][box] = 7 * lbl + 1          # (< 1000: the single-channel torch form multiplies labels)
                break
    return labels


def make_pred(rng, G, dtype, ov):
    pred = np.where(G, rng.uniform(0.1, 1.0, G.shape), rng.uniform(0.0, 1.0, G.shape) ** 3).astype(dtype)
    tau = dtype(0.3)
    assert float(tau) > 0.3                            # float32 and float16 both round 0.3 up
    clean = np.argwhere(np.broadcast_to(~ov, G.shape))
    for idx in clean[rng.choice(len(clean), size=12, replace=False)]:
        pred[tuple(idx)] = tau
    return pred


def nhood_of(patch, ndim):
    r = [p // 2 for p in patch]
    if ndim == 2:
        return [[i, j] for i in range(-r[1], r[1] + 1) for j in range(-r[2], r[2] + 1)]
    return [[z, y, x] for z in range(-r[0], r[0] + 1) for y in range(-r[1], r[1] + 1) for x in range(-r[2], r[2] + 1)]


def check_patch(name, pred, labels4, patch, thresholds):
    """what a patch case is for -- by this project's host definition, which `main` holds to the reference"""
    sys.path.insert(0, ROOT)
    from patchperpix_amd import evaluate_prediction as ev
    pred4 = pred.reshape((pred.shape[0],) + labels4.shape[1:])
    counts, inter, union = ev.patch_counts_host(pred4, labels4, patch, thresholds, want_maps=True)
    num_gt = int(counts[0])
    assert num_gt > 0, name
    for i in range(len(thresholds)):
        num_pred, tp = int(counts[1 + 2 * i]), int(counts[2 + 2 * i])
        assert num_pred > 0 and 0 < tp < min(num_gt, num_pred), (name, thresholds[i], num_gt, num_pred, tp)
        assert (union[i] > 1).any(), name
    tau = pred.dtype.type(0.3)
    assert (pred == tau).any(), name
    L = labels4.shape[0]
    if L > 1:
        numinst = (labels4 > 0).sum(axis=0)
        assert (numinst > 1).any(), name
        r = [p // 2 for p in patch]
        found = False
        for z, y, x in np.argwhere(numinst > 1):
            for c in range(L):
                lbl = labels4[c, z, y, x]
                if lbl == 0:
                    continue
                z0, y0, x0 = max(z - r[0], 0), max(y - r[1], 0), max(x - r[2], 0)
                win = (slice(z0, z + r[0] + 1), slice(y0, y + r[1] + 1), slice(x0, x + r[2] + 1))
                found |= bool(((labels4[c][win] == lbl) & (numinst[win] == 1)).any())
        assert found, (name, "no overlap voxel is the in-patch neighbour of a clean centre of its label")
    return ev


def patch_case(ref, name, spatial, patch, L, dtype, seed, n_inst):
    rng = np.random.default_rng(seed)
    ndim = len(spatial)
    labels = make_labels(rng, L, spatial, n_inst)
    nhood = np.array(nhood_of(patch, ndim))
    aff = sys.modules["gunpowder.add_affinities"]
    if L > 1:
        G = (aff.seg_to_affgraph_3d_multi if ndim == 3 else aff.seg_to_affgraph_2d_multi)(labels, nhood) > 0
    else:
        G = (aff.seg_to_affgraph if ndim == 3 else aff.seg_to_affgraph_2d)(labels[0], nhood) > 0
    ov = (labels > 0).sum(axis=0) > 1
    pred = make_pred(rng, G, dtype, ov)
    stored_pred = pred if ndim == 3 else pred[:, None]            # a 2-d prediction is stored (C, 1, Y, X)
    thresholds = [0.3, 0.5, 0.9]
    labels4 = labels.reshape((L,) + (1,) * (3 - ndim) + spatial)
    ev = check_patch(name, pred, labels4, patch, thresholds)
    STORE[name + ".hdf"] = {"volumes/pred_affs": stored_pred}
    STORE[name + "_gt.hdf"] = {"volumes/gt_instances": labels}
    base = dict(aff_key="volumes/pred_affs", sample_gt_key="volumes/gt_instances", patchshape=list(patch),
                eval_patch_thresholds=thresholds, overlapping_inst=L > 1)
    runs, arrays = [], {}
    for k, extra in enumerate((dict(), dict(return_patches=True, store_iou=False),
                               dict(return_patches=True, store_iou=True))):
        kwargs = dict(base, **extra)
        metrics, ious = scalars(run(ref, "evaluate_patch", name, kwargs))
        for th_key, iou in ious.items():
            arrays["IOU/%d/%s" % (k, th_key)] = iou
        runs.append({"fn": "evaluate_patch", "kwargs": kwargs, "metrics": metrics})
        # this project's host definition gives the same (the tests say it again, without the reference)
        mine = ev.patch_metrics(pred.reshape((pred.shape[0],) + labels4.shape[1:]), labels4, patch, thresholds,
                                extra.get("return_patches", False), extra.get("store_iou", False))
        mine_s, mine_i = scalars(mine)
        assert json.dumps(mine_s, sort_keys=True) == json.dumps(metrics, sort_keys=True), (name, mine_s, metrics)
        assert all(np.array_equal(mine_i[t].reshape(ious[t].shape), ious[t]) for t in ious), name
    # the centre channel as the foreground (fg_key None), without and with small components removed
    if ndim == 3:
        for rsc in (None, [0, 2]):
            kwargs = dict(base, eval_fg_thresholds=[0.5], remove_small_comps=rsc)
            metrics, _ = scalars(run(ref, "evaluate_fg", name, kwargs))
            runs.append({"fn": "evaluate_fg", "kwargs": kwargs, "metrics": metrics})
    save(name, {"pred/volumes/pred_affs": stored_pred, "gt/volumes/gt_instances": labels}, runs, arrays)


def fg_case(ref, name, seed):
    """isolated components of 1, 3, 4, 10 and 11 voxels next to two large ones, with remove_small_comps =
    [0, 3, 10]: components of AT MOST that many voxels go (`counts <= compsize`), which the counts below pin."""
    rng = np.random.default_rng(seed)
    spatial = (8, 12, 26)
    mask = np.zeros(spatial, dtype=bool)
    mask[0:3, 0:4, 0:4] = True                 # 48
    mask[5:8, 7:12, 0:3] = True                # 45
    sizes = {}
    for i, n in enumerate((1, 3, 4, 10, 11)):
        x0 = 6 + 4 * i
        vox = [(z, 1 + y, x0 + x) for z in (4, 5) for y in range(3) for x in range(2)][:n]
        if n == 3:
            vox = [(4, 1, x0), (5, 2, x0 + 1), (4, 3, x0)]       # diagonal steps only: one component under 26 neighbours
        for v in vox:
            mask[v] = True
        sizes[n] = len(vox)
    assert list(sizes.values()) == [1, 3, 4, 10, 11]
    pred = np.where(mask, rng.uniform(0.91, 1.0, spatial), rng.uniform(0.0, 0.5, spatial)).astype(np.float32)
    pred[0:3, 0:4, 0:2] = 0.7                  # between the two thresholds
    labels = np.zeros((2,) + spatial, dtype=np.int32)
    labels[0, 0:3, 0:5, 0:5] = 5
    labels[0, 5:8, 6:12, 0:3] = 9
    labels[1, 4:6, 1:4, 14:24] = 12
    labels[1, 2:4, 3:6, 3:6] = 20              # overlaps label 5 of channel 0
    STORE[name + ".hdf"] = {"volumes/pred_fgbg": pred}
    STORE[name + "_gt.hdf"] = {"volumes/gt_instances": labels}
    runs = []
    for kwargs in (dict(eval_fg_thresholds=[0.5, 0.9], remove_small_comps=[10, 0, 3]), dict(remove_small_comps=[]),
                   dict(eval_fg_thresholds=[0.9], remove_small_comps=[3])):
        kwargs = dict(kwargs, fg_key="volumes/pred_fgbg", sample_gt_key="volumes/gt_instances", patchshape=[3, 3, 3])
        metrics, _ = scalars(run(ref, "evaluate_fg", name, kwargs))
        runs.append({"fn": "evaluate_fg", "kwargs": kwargs, "metrics": metrics})
    m = runs[0]["metrics"]["0_5"]
    total = int(mask.sum())
    assert m["rsc_0"]["num_pred"] == total
    assert m["rsc_3"]["num_pred"] == total - 1 - 3, "a component of exactly 3 voxels goes at remove_small_comps = 3"
    assert m["rsc_10"]["num_pred"] == total - 1 - 3 - 4 - 10, "and one of exactly 10 at 10; 4 and 11 stay until then"
    assert runs[0]["metrics"]["0_9"]["rsc_0"]["num_pred"] == total - 24
    assert 0 < m["rsc_0"]["num_tp"] < min(m["rsc_0"]["num_gt"], m["rsc_0"]["num_pred"])
    save(name, {"pred/volumes/pred_fgbg": pred, "gt/volumes/gt_instances": labels}, runs, {})


def numinst_case(ref, name, seed):
    rng = np.random.default_rng(seed)
    spatial = (5, 9, 11)
    labels = make_labels(rng, 3, spatial, 9)
    gt = (labels > 0).sum(axis=0)
    assert set(np.unique(gt)) >= {0, 1, 2}
    prob = rng.uniform(0.0, 0.3, (4,) + spatial).astype(np.float32)
    noisy = np.where(rng.uniform(size=spatial) < 0.8, gt, rng.integers(0, 4, spatial))
    np.put_along_axis(prob, noisy[None], rng.uniform(0.35, 1.0, (1,) + spatial).astype(np.float32), axis=0)
    STORE[name + ".hdf"] = {"volumes/pred_numinst": prob}
    STORE[name + "_gt.hdf"] = {"volumes/gt_instances": labels}
    runs = []
    for extra in (dict(), dict(numinst_threshs=[0.4, 0.6]), dict(max_numinst=1),
                  dict(numinst_threshs=[0.4, 0.6, 0.5], max_numinst=2)):
        kwargs = dict(extra, numinst_key="volumes/pred_numinst", sample_gt_key="volumes/gt_instances")
        metrics, _ = scalars(run(ref, "evaluate_numinst", name, kwargs))
        assert all(0 < metrics[k]["num_tp"] < min(metrics[k]["num_gt"], metrics[k]["num_pred"]) for k in ("0", "1")), \
            (name, metrics)
        runs.append({"fn": "evaluate_numinst", "kwargs": kwargs, "metrics": metrics})
    assert sorted(runs[2]["metrics"]) == ["0", "1"] and len(runs[0]["metrics"]) >= 3
    # the two-step ladder never predicts 3: the reference's `else` branch (no prediction, zeros) is in the golden
    assert any(v["num_pred"] == 0 and v["precision"] == 0 for v in runs[1]["metrics"].values())
    save(name, {"pred/volumes/pred_numinst": prob, "gt/volumes/gt_instances": labels}, runs, {})


def save(name, datasets, runs, arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, runs=json.dumps(runs), **datasets, **arrays)
    print("%-14s %6d bytes  %s" % (name, os.path.getsize(path), [r["fn"] for r in runs]))


def main():
    ref = load_reference()
    os.makedirs(OUT, exist_ok=True)
    patch_case(ref, "patch_3d_L3", (5, 6, 8), (3, 3, 3), 3, np.float32, seed=11, n_inst=9)
    patch_case(ref, "patch_3d_L1", (6, 5, 7), (5, 3, 3), 1, np.float16, seed=12, n_inst=5)
    patch_case(ref, "patch_2d_L2", (9, 12), (1, 5, 5), 2, np.float32, seed=13, n_inst=6)
    fg_case(ref, "fg_rsc", seed=14)
    numinst_case(ref, "numinst", seed=15)


if __name__ == "__main__":
    main()
