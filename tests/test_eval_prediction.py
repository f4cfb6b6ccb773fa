"""The host side of `evaluate_prediction` (reference: PatchPerPix/evaluate/evaluate_prediction.py,
experiments/run_ppp.py:1300-1443): `patch_counts_host` and the three file-level functions against the
reference's own results (tests/golden/eval_prediction/*.npz, written by gen_golden_eval_prediction.py), the
refusals, the z-chunked reading and the task in run_ppp.  Integers and stored IOU arrays are compared with
array_equal, floats with ==; PPP_POSTPROCESS=host keeps the device out of it."""
import glob
import json
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from patchperpix_amd import evaluate_prediction as ev
from patchperpix_amd import minihdf5, minizarr, run_ppp

EV_DIR = os.path.join(GOLDEN_DIR, "eval_prediction")
GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(EV_DIR, "*.npz")))
PATCH_GOLDENS = [g for g in GOLDENS if g.startswith("patch_")]


@pytest.fixture(autouse=True)
def _host_path(monkeypatch):
    monkeypatch.setenv("PPP_POSTPROCESS", "host")


# ---------------------------------------------------------------------------------------------
# inputs shared with tests/test_eval_prediction_gpu.py
# ---------------------------------------------------------------------------------------------
def golden(name):
    """(prediction datasets, label datasets, runs, {(run index, thresh_key): IOU})"""
    z = np.load(os.path.join(EV_DIR, name + ".npz"))
    pred = {k[5:]: z[k] for k in z.files if k.startswith("pred/")}
    gt = {k[3:]: z[k] for k in z.files if k.startswith("gt/")}
    ious = {(int(k.split("/")[1]), k.split("/")[2]): z[k] for k in z.files if k.startswith("IOU/")}
    return pred, gt, json.loads(str(z["runs"])), ious


def write_container(path, datasets):
    """the datasets as a zarr store or an HDF5 file, by the name's ending"""
    if path.endswith(".zarr"):
        root = minizarr.open(path, "w")
        for key, data in datasets.items():
            root.create_dataset(key, data=data, chunks=data.shape)
    else:
        with minihdf5.File(path, "w") as f:
            for key, data in datasets.items():
                f.create_dataset(key, data=data, compression="gzip")
    return path


def write_sample(folder, name, fmt="zarr"):
    """the golden's two files in `folder`; returns (prediction file, label file, runs, ious)"""
    pred, gt, runs, ious = golden(name)
    return (write_container(os.path.join(str(folder), name + "." + fmt), pred),
            write_container(os.path.join(str(folder), name + "_gt." + fmt), gt), runs, ious)


def same(got, want):
    """a metric dict against the golden's scalars: ints equal, floats ==, NaN where NaN"""
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k, w in want.items():
        g = got[k]
        if isinstance(w, dict):
            same(g, w)
        elif isinstance(w, float) and math.isnan(w):
            assert math.isnan(g), (k, g)
        else:
            assert g == w and isinstance(g, (int, float, np.integer, np.floating)), (k, g, w)


def check_run(fn, pred_fn, label_fn, k, run, ious):
    got = getattr(ev, fn)(pred_fn, label_fn, **run["kwargs"])
    for th_key, entry in got.items():
        iou = entry.get("rsc_0", {}).pop("IOU", None) if isinstance(entry.get("rsc_0"), dict) else None
        assert (iou is not None) == ((k, th_key) in ious), (k, th_key)
        if iou is not None:
            assert iou.dtype == np.float64 and iou.shape == ious[(k, th_key)].shape
            assert np.array_equal(iou, ious[(k, th_key)])
    same(got, run["metrics"])
    return got


def patch_arrays(name):
    """(pred (C, Z, Y, X), labels (L, Z, Y, X), patch, thresholds) of a patch golden"""
    pred, gt, runs, _ = golden(name)
    p, lab = pred["volumes/pred_affs"], gt["volumes/gt_instances"]
    kw = runs[0]["kwargs"]
    if p.shape[1] == 1 and lab.ndim == 3:
        lab = lab[:, None]
    return p, lab, kw["patchshape"], kw["eval_patch_thresholds"]


# ---------------------------------------------------------------------------------------------
def test_the_goldens_are_there():
    assert GOLDENS == ["fg_rsc", "numinst", "patch_2d_L2", "patch_3d_L1", "patch_3d_L3"]


@pytest.mark.parametrize("name", PATCH_GOLDENS)
def test_patch_counts_host_equals_the_reference(name):
    pred, labels, patch, ths = patch_arrays(name)
    _, _, runs, ious = golden(name)
    counts, inter, union = ev.patch_counts_host(pred, labels, patch, ths, want_maps=True)
    assert counts.dtype == np.int64 and inter.dtype == np.int32 and inter.shape == (len(ths),) + pred.shape[1:]
    for k in range(3):
        kw = runs[k]["kwargs"]
        got = ev.metrics_from_counts(counts, ths, inter, union, kw.get("return_patches"), kw.get("store_iou"))
        for th in ths:
            iou = got[ev.thresh_key(th)]["rsc_0"].pop("IOU", None)
            if kw.get("store_iou"):
                assert np.array_equal(iou.reshape(ious[(k, ev.thresh_key(th))].shape), ious[(k, ev.thresh_key(th))])
        same(got, runs[k]["metrics"])
    # without the maps the counts are the same
    assert np.array_equal(ev.patch_counts_host(pred, labels, patch, ths)[0], counts)


@pytest.mark.parametrize("fmt", ["zarr", "hdf"])
@pytest.mark.parametrize("name", GOLDENS)
def test_file_level_functions_equal_the_reference(tmp_path, name, fmt):
    pred_fn, label_fn, runs, ious = write_sample(tmp_path, name, fmt)
    for k, run in enumerate(runs):
        check_run(run["fn"], pred_fn, label_fn, k, run, ious)


def test_tau_is_the_threshold_rounded_to_the_element_type():
    """pred == tau(0.3) > 0.3: NumPy compares in the array's dtype, so the element is NOT above the threshold"""
    for dtype in (np.float32, np.float16):
        tau = dtype(0.3)
        assert float(tau) > 0.3 and ev.rounded_thresholds([0.3], dtype) == [float(tau)]
        pred = np.full((1, 1, 1, 2), tau, dtype=dtype)
        pred[0, 0, 0, 1] = np.nextafter(tau, dtype(1))
        counts, _, _ = ev.patch_counts_host(pred, np.ones((1, 1, 1, 2), np.int32), (1, 1, 1), [0.3])
        assert list(counts) == [2, 1, 1] and list((pred > 0.3).reshape(-1)) == [False, True]


def test_a_negative_threshold_counts_the_zeroed_overlap_voxels():
    labels = np.zeros((2, 1, 1, 3), np.int32)
    labels[0, 0, 0, :2] = 4
    labels[1, 0, 0, 1:] = 6                           # voxel 1 overlaps
    pred = np.full((3, 1, 1, 3), np.nan, dtype=np.float32)      # NaN compares false; the overlap's is zeroed first
    counts, inter, union = ev.patch_counts_host(pred, labels, (1, 1, 3), [-0.5, 0.5], want_maps=True)
    # G': centre 0 -> itself and its right neighbour (the overlap voxel counts as a neighbour); centre 2 -> itself
    # and its left neighbour; the overlap centre has none
    assert list(counts) == [4, 3, 0, 0, 0]
    assert inter[0, 0, 0].tolist() == [0, 0, 0] and union[0, 0, 0].tolist() == [2, 3, 2]


@pytest.mark.parametrize("what", ["no channel axis", "negative", "too large", "even patch", "channels", "nan threshold",
                                  "inf threshold", "f16 overflow", "float labels"])
def test_refusals(what):
    pred = np.zeros((27, 2, 3, 4), np.float32)
    labels = np.ones((1, 2, 3, 4), np.int64)
    patch, ths = (3, 3, 3), [0.5]
    if what == "no channel axis":
        labels = labels[0]
    elif what == "negative":
        labels[0, 0, 0, 0] = -1
    elif what == "too large":
        labels[0, 0, 0, 0] = 1 << 31
    elif what == "even patch":
        pred, patch = np.zeros((18, 2, 3, 4), np.float32), (2, 3, 3)
    elif what == "channels":
        patch = (3, 3, 5)
    elif what == "nan threshold":
        ths = [float("nan")]
    elif what == "inf threshold":
        ths = [float("inf")]
    elif what == "f16 overflow":
        pred, ths = pred.astype(np.float16), [70000.0]          # finite as a float, inf as float16
    elif what == "float labels":
        labels = labels.astype(np.float32)
    with pytest.raises(ValueError):
        ev.patch_metrics(pred, labels, patch, ths)


def test_save_as_png_is_refused_not_ignored(tmp_path):
    pred_fn, label_fn, runs, _ = write_sample(tmp_path, "fg_rsc")
    with pytest.raises(NotImplementedError, match="save_as_png"):
        ev.evaluate_fg(pred_fn, label_fn, save_as_png=True, output_folder=str(tmp_path), **runs[0]["kwargs"])
    pred_fn, label_fn, runs, _ = write_sample(tmp_path, "numinst")
    with pytest.raises(NotImplementedError, match="save_as_png"):
        ev.evaluate_numinst(pred_fn, label_fn, save_as_png=True, output_folder=str(tmp_path), **runs[0]["kwargs"])


def test_file_level_labels_need_the_channel_axis(tmp_path):
    pred, gt, runs, _ = golden("patch_3d_L1")
    pred_fn = write_container(str(tmp_path / "s.zarr"), pred)
    label_fn = write_container(str(tmp_path / "s_gt.zarr"), {k: v[0] for k, v in gt.items()})
    with pytest.raises(ValueError, match="channel axis"):
        ev.evaluate_patch(pred_fn, label_fn, **runs[0]["kwargs"])


def test_small_components_need_a_3d_foreground(tmp_path):
    pred_fn = write_container(str(tmp_path / "s.zarr"), {"fg": np.ones((1, 4, 5), np.float32)})
    label_fn = write_container(str(tmp_path / "s_gt.zarr"), {"gt": np.ones((1, 4, 5), np.int32)})
    kw = dict(fg_key="fg", sample_gt_key="gt", patchshape=[1, 3, 3])
    assert ev.evaluate_fg(pred_fn, label_fn, **kw)["0_9"]["rsc_0"]["num_tp"] == 20
    with pytest.raises(ValueError, match="3-d"):
        ev.evaluate_fg(pred_fn, label_fn, remove_small_comps=[2], **kw)


@pytest.mark.parametrize("name", ["patch_3d_L3", "patch_2d_L2"])
def test_chunked_reading_equals_one_chunk(tmp_path, name, monkeypatch):
    pred_fn, label_fn, runs, ious = write_sample(tmp_path, name)
    pred, _, _, _ = patch_arrays(name)
    calls = []
    real = ev.patch_counts_host

    def spy(tile, *a, **k):
        calls.append(tile.shape[1])
        return real(tile, *a, **k)
    monkeypatch.setattr(ev, "patch_counts_host", spy)
    budget = pred[:, :2].nbytes if pred.shape[1] > 1 else 1        # two slices at a time: 2 + 2 + 1 of the 3-d case
    run = dict(runs[2], kwargs=dict(runs[2]["kwargs"], eval_chunk_bytes=budget))
    check_run("evaluate_patch", pred_fn, label_fn, 2, run, ious)
    if pred.shape[1] > 1:
        assert calls == [2, 2, 1], calls
    else:
        assert calls == [1]
    # a budget below one slice still moves one slice at a time
    del calls[:]
    check_run("evaluate_patch", pred_fn, label_fn, 2, dict(run, kwargs=dict(run["kwargs"], eval_chunk_bytes=1)), ious)
    assert calls == [1] * pred.shape[1]


def test_skeleton_coverage_uses_the_host_thinning(tmp_path):
    """not golden (scikit-image is absent where the goldens are made): the reference's formulas over
    backend.host_skeletonize_3d"""
    from patchperpix_amd import backend
    pred_fn, label_fn, runs, _ = write_sample(tmp_path, "fg_rsc")
    pred, gt, _, _ = golden("fg_rsc")
    kw = dict(runs[0]["kwargs"], evaluate_skeleton_coverage=True, remove_small_comps=[0], eval_fg_thresholds=[0.5])
    got = ev.evaluate_fg(pred_fn, label_fn, **kw)["0_5"]["rsc_0"]
    gt_mask = (gt["volumes/gt_instances"] > 0).any(axis=0)
    pm = pred["volumes/pred_fgbg"] > 0.5
    gs, ps = backend.host_skeletonize_3d(gt_mask), backend.host_skeletonize_3d(pm)
    tp = float((gs & pm).sum())
    assert tp > 0 and ps.sum() > 0
    precision, recall = tp / (tp + float((~gt_mask & ps).sum())), tp / (tp + float((gs & ~pm).sum()))
    assert got == {"num_gt": int(gt_mask.sum()), "num_pred": int(pm.sum()), "num_tp": tp, "precision": precision,
                   "recall": recall, "f1": 2 * (precision * recall) / (precision + recall)}
    # evaluate_numinst: class 0 plain, the others by the skeleton formulas
    pred_fn, label_fn, runs, _ = write_sample(tmp_path, "numinst")
    plain = ev.evaluate_numinst(pred_fn, label_fn, **runs[0]["kwargs"])
    skel = ev.evaluate_numinst(pred_fn, label_fn, evaluate_skeleton_coverage=True, **runs[0]["kwargs"])
    assert skel["0"] == plain["0"] and skel["1"]["num_gt"] == plain["1"]["num_gt"]
    assert isinstance(skel["1"]["num_tp"], float) and skel["1"]["num_tp"] <= plain["1"]["num_tp"]


# ---------------------------------------------------------------------------------------------
# the task
# ---------------------------------------------------------------------------------------------
CONFIG = """
[data]
test_data = %r
gt_key = "volumes/gt_instances"
input_format = %r
[model]
patchshape = %s
[prediction]
output_format = %r
aff_key = "volumes/pred_affs"
[evaluation]
metric = "f1"
[evaluation.prediction]
eval_patch_prediction = true
eval_fg_prediction = %s
eval_patch_thresholds = [0.3, 0.5, 0.9]
eval_fg_thresholds = [0.5]
return_patches = true
store_iou = %s
"""


def _task(tmp_path, fmt, gt_in_one_file, eval_fg, store_iou, name="patch_3d_L3"):
    pred, gt, runs, ious = golden(name)
    folder, gt_folder, out = tmp_path / "pred", tmp_path / "gt", tmp_path / "out"
    folder.mkdir()
    gt_folder.mkdir()
    pred_fn = write_container(str(folder / ("sample_a." + fmt)), pred)
    write_container(str(folder / ("sample_b." + fmt)), {k: v[..., ::-1].copy() for k, v in pred.items()})
    if gt_in_one_file:
        data = write_container(str(gt_folder / ("all." + fmt)), {s + "/" + k: v for s in ("sample_a", "sample_b")
                                                                 for k, v in gt.items()})
    else:
        data = str(gt_folder)
        for s in ("sample_a", "sample_b"):
            write_container(str(gt_folder / (s + "." + fmt)), gt)
    cfg = tmp_path / "config.toml"
    cfg.write_text(CONFIG % (data, fmt, runs[0]["kwargs"]["patchshape"], fmt, str(eval_fg).lower(), str(store_iou).lower()))
    argv = ["--config", str(cfg), "--do", "evaluate_prediction", "--pred-folder", str(folder), "--output-folder", str(out)]
    return argv, pred_fn, out, runs, ious


@pytest.mark.parametrize("fmt,gt_in_one_file", [("zarr", True), ("hdf", False)])
def test_run_ppp_evaluate_prediction_task(tmp_path, fmt, gt_in_one_file):
    argv, pred_fn, out, runs, ious = _task(tmp_path, fmt, gt_in_one_file, eval_fg=False, store_iou=True)
    run_ppp.main(argv + ["--sample", "sample_a"])
    with open(str(out / "prediction_metrics.json")) as f:
        got = json.load(f)
    assert sorted(got) == ["sample_a"], "--sample was ignored"
    same(got["sample_a"], runs[2]["metrics"])                   # (the IOU arrays are left out of the file)
    opener = (lambda p: minizarr.open(p, "r")) if fmt == "zarr" else (lambda p: minihdf5.File(p, "r"))
    f = opener(pred_fn)
    for th_key in ("0_3", "0_5", "0_9"):
        iou = np.asarray(f["volumes/%s/IOU" % th_key])
        assert iou.dtype == np.float64 and np.array_equal(iou, ious[(2, th_key)])
    if fmt == "hdf":
        f.close()
    # a second run replaces the datasets; both samples; (metrics, ths) as the reference returns them
    from patchperpix_amd.run_ppp import evaluate_prediction, load_config
    import argparse
    args = argparse.Namespace(pred_folder=argv[5], output_folder=argv[7], sample=None)
    metrics, ths = evaluate_prediction(args, load_config([argv[1]]))
    assert ths == ["0_3_rsc_0", "0_5_rsc_0", "0_9_rsc_0"] and len(metrics) == 3
    with open(str(out / "prediction_metrics.json")) as f:
        got = json.load(f)
    assert sorted(got) == ["sample_a", "sample_b"]
    for m, th_key in zip(metrics, ("0_3", "0_5", "0_9")):
        assert m == np.mean([got[s][th_key]["rsc_0"]["f1"] for s in ("sample_a", "sample_b")])


def test_a_threshold_key_shared_by_fg_and_patch_keeps_the_patch_entry(tmp_path):
    argv, _, out, runs, _ = _task(tmp_path, "zarr", True, eval_fg=True, store_iou=False)
    run_ppp.main(argv + ["--sample", "sample_a"])
    with open(str(out / "prediction_metrics.json")) as f:
        got = json.load(f)["sample_a"]
    same(got, runs[1]["metrics"])                               # "0_5" is the patch entry: no num_gt / num_pred in it


def test_the_cli_choice_exists():
    with pytest.raises(SystemExit):
        run_ppp.main(["--config", "x", "--do", "evaluate_something", "--pred-folder", "a", "--output-folder", "b"])
