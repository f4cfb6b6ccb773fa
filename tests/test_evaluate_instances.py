"""CPU: the `evaluate` step (patchperpix_amd/evaluate_instances.py).  The contingency table's NumPy definition
against a literal triple loop, the metric layer against answers worked out by hand in the comments, the TOML
file and the `--do evaluate` task.  Parity with the reference's evaluation package is unpinned (it is not
vendored); what is pinned here is this project's own definition, DESIGN.md §7.16."""
import itertools
import os

import numpy as np
import pytest

from patchperpix_amd import evaluate_instances as ei
from patchperpix_amd import minihdf5, minizarr, run_ppp

THS = ["th_0_%d" % k for k in range(1, 10)]


@pytest.fixture(autouse=True)
def _host(monkeypatch):
    monkeypatch.setenv("PPP_POSTPROCESS", "host")


# ---------------------------------------------------------------------------------------------
# overlap_counts_host against a literal triple loop
# ---------------------------------------------------------------------------------------------
def triple_loop(a, b):
    table = {}
    A, B = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    for v in range(A.shape[1]):
        for i in range(A.shape[0]):
            if A[i, v]:
                table[(int(A[i, v]), 0)] = table.get((int(A[i, v]), 0), 0) + 1
        for j in range(B.shape[0]):
            if B[j, v]:
                table[(0, int(B[j, v]))] = table.get((0, int(B[j, v])), 0) + 1
        for i in range(A.shape[0]):
            for j in range(B.shape[0]):
                if A[i, v] and B[j, v]:
                    k = (int(A[i, v]), int(B[j, v]))
                    table[k] = table.get(k, 0) + 1
    keys = sorted(table)
    return np.array(keys, dtype=np.uint32).reshape(-1, 2), np.array([table[k] for k in keys], dtype=np.int64)


@pytest.mark.parametrize("channels", [(1, 1), (3, 2), (2, 3)])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 5), (3, 4, 7)])
def test_overlap_counts_host_against_triple_loop(shape, channels):
    rng = np.random.default_rng(sum(shape) + 10 * channels[0])
    ids = np.array([0, 0, 1, 2, 3, 2 ** 31, 0xFFFFFFFF], dtype=np.uint32)
    a = ids[rng.integers(0, len(ids), (channels[0],) + shape)]
    b = ids[rng.integers(0, len(ids), (channels[1],) + shape)]
    if a.size > 3:
        a.reshape(-1)[:2] = (2 ** 31, 0xFFFFFFFF)                 # both big ids are present
        b.reshape(-1)[:2] = (0xFFFFFFFF, 0xFFFFFFFF)
    rows, counts = ei.overlap_counts_host(a, b)
    want_rows, want_counts = triple_loop(a, b)
    assert rows.dtype == np.uint32 and counts.dtype == np.int64
    assert np.array_equal(rows, want_rows) and np.array_equal(counts, want_counts)
    keys = [tuple(r) for r in rows.tolist()]
    assert keys == sorted(keys) and (counts > 0).all()
    # marginals: the sizes of the ids, counted over all channels
    for r, c in zip(rows, counts):
        if r[1] == 0:
            assert c == int((a == r[0]).sum())
        if r[0] == 0:
            assert c == int((b == r[1]).sum())
    if a.size > 3:
        assert (0xFFFFFFFF, 0xFFFFFFFF) in keys and (2 ** 31, 0xFFFFFFFF) in keys


def test_overlap_counts_host_all_background_side():
    a = np.zeros((2, 2, 3, 5), dtype=np.uint32)
    b = np.arange(30, dtype=np.uint32).reshape(1, 2, 3, 5) % 4              # 1: 8 voxels (1, 5 .. 29), 2 and 3: 7 each
    rows, counts = ei.overlap_counts_host(a, b)
    assert rows.tolist() == [[0, 1], [0, 2], [0, 3]] and counts.tolist() == [8, 7, 7]
    rows, counts = ei.overlap_counts_host(b, a)
    assert rows.tolist() == [[1, 0], [2, 0], [3, 0]] and counts.tolist() == [8, 7, 7]
    rows, counts = ei.overlap_counts_host(a, a[:1])
    assert rows.shape == (0, 2) and counts.shape == (0,)


def test_overlap_counts_refuses_bad_values():
    ok = np.ones((1, 2, 2, 2), dtype=np.int64)
    with pytest.raises(ValueError, match=r"\[0, 2\^32\)"):
        ei.overlap_counts_host(ok * -1, ok)
    with pytest.raises(ValueError, match=r"\[0, 2\^32\)"):
        ei.overlap_counts_host(ok, ok * 2 ** 32)
    with pytest.raises(ValueError, match="integers"):
        ei.overlap_counts_host(ok.astype(np.float32), ok)
    with pytest.raises(ValueError, match="spatial shape"):
        ei.overlap_counts_host(ok, np.ones((1, 2, 2, 3), dtype=np.int64))


# ---------------------------------------------------------------------------------------------
# metric cases worked out by hand
# ---------------------------------------------------------------------------------------------
def boxes(shape, *items):
    m = np.zeros(shape, dtype=np.uint32)
    for label, sl in items:
        m[sl] = label
    return m


def test_identical_maps():
    gt = boxes((4, 8, 8), (3, np.s_[:, :4, :]), (2 ** 31 + 9, np.s_[:, 5:, 2:]))
    for criterion, strategy in itertools.product(("iou", "cldice"), ("greedy", "hungarian")):
        d = ei.evaluate_volumes(gt, gt, localization_criterion=criterion, assignment_strategy=strategy,
                                evaluate_false_labels=True)
        assert d["general"] == {"Num GT": 2, "Num Pred": 2}
        for th in THS:
            e = d["confusion_matrix"][th]
            assert (e["AP_TP"], e["AP_FP"], e["AP_FN"]) == (2, 0, 0)
            assert e["precision"] == e["recall"] == e["fscore"] == e["AP"] == 1.0
            assert e["false_merge"] == 0 and e["false_split"] == 0
        assert d["confusion_matrix"]["avFscore"] == 1.0 and d["confusion_matrix"]["avAP"] == 1.0


def test_one_gt_box_cut_into_two_halves():
    # gt 1: 4 x 4 x 8 = 128 voxels.  The predicted halves 5 and 6 hold 64 voxels of it each and 32 voxels outside
    # it (two more rows): |p| = 96, iou = 64 / (128 + 96 - 64) = 0.4, precision n / |p| = 2 / 3, recall 0.5.
    gt = boxes((4, 8, 8), (1, np.s_[:, 2:6, :]))
    pred = boxes((4, 8, 8), (5, np.s_[:, 0:6, :4]), (6, np.s_[:, 2:8, 4:]))
    for strategy in ("greedy", "hungarian"):
        d = ei.evaluate_volumes(pred, gt, assignment_strategy=strategy, evaluate_false_labels=True)
        assert d["general"] == {"Num GT": 1, "Num Pred": 2}
        for k, th in enumerate(THS, start=1):
            e = d["confusion_matrix"][th]
            # 0.4 > th up to th = 0.3: one of the halves takes the box; from 0.4 on (0.4 > 0.4 is false) none does
            want = (1, 1, 0) if k <= 3 else (0, 2, 1)
            assert (e["AP_TP"], e["AP_FP"], e["AP_FN"]) == want, th
            assert e["fscore"] == (2 / 3 if k <= 3 else 0.0) and e["AP"] == (0.5 if k <= 3 else 0.0)
            assert e["precision"] == (0.5 if k <= 3 else 0.0) and e["recall"] == (1.0 if k <= 3 else 0.0)
            # both halves have precision 2 / 3 > th up to th = 0.6: the box counts as split once
            assert e["false_split"] == (1 if k <= 6 else 0), th
            assert e["false_merge"] == 0
        assert d["confusion_matrix"]["avFscore"] == pytest.approx(3 * (2 / 3) / 9, abs=1e-15)


def test_two_gt_boxes_under_one_predicted_id():
    gt = boxes((4, 8, 8), (1, np.s_[:, :4, :]), (2, np.s_[:, 4:, :]))
    pred = boxes((4, 8, 8), (9, np.s_[:, :, :]))
    d = ei.evaluate_volumes(pred, gt, evaluate_false_labels=True)
    # recall n / |g| = 1 for both boxes at every threshold: one merge; iou = 128 / 256 = 0.5
    for k, th in enumerate(THS, start=1):
        e = d["confusion_matrix"][th]
        assert e["false_merge"] == 1 and e["false_split"] == 0
        assert (e["AP_TP"], e["AP_FP"], e["AP_FN"]) == ((1, 0, 1) if k <= 4 else (0, 1, 2))


def test_greedy_and_hungarian_differ_on_the_2x2_matrix():
    # flat volume of 100 voxels, two channels each side: g1 = [0, 100), g2 = [0, 33), p1 = [0, 60), p2 = [45, 100)
    #   iou(g1, p1) = 60 / 100 = 0.6     iou(g1, p2) = 55 / 100 = 0.55
    #   iou(g2, p1) = 33 / 60 = 0.55     iou(g2, p2) = 0
    # th = 0.5: greedy takes (g1, p1) first and nothing is left; the assignment takes 0.55 + 0.55 > 0.6.
    gt = np.zeros((2, 1, 1, 100), dtype=np.uint32)
    pred = np.zeros((2, 1, 1, 100), dtype=np.uint32)
    gt[0, ..., :] = 1
    gt[1, ..., :33] = 2
    pred[0, ..., :60] = 1
    pred[1, ..., 45:] = 2
    greedy = ei.evaluate_volumes(pred, gt, assignment_strategy="greedy")["confusion_matrix"]
    hungarian = ei.evaluate_volumes(pred, gt, assignment_strategy="hungarian")["confusion_matrix"]
    by_switch = ei.evaluate_volumes(pred, gt, assignment_strategy="greedy", use_linear_sum_assignment=True)["confusion_matrix"]
    assert greedy["th_0_5"]["AP_TP"] == 1 and hungarian["th_0_5"]["AP_TP"] == 2 and by_switch == hungarian
    assert greedy["th_0_6"]["AP_TP"] == 0 and hungarian["th_0_6"]["AP_TP"] == 0      # 0.6 > 0.6 is false
    assert hungarian["th_0_5"]["fscore"] == 1.0 and greedy["th_0_5"]["fscore"] == 0.5


def test_remove_small_components_at_the_boundary():
    gt = boxes((2, 4, 8), (1, np.s_[:, :, :]))
    pred = boxes((2, 4, 8), (7, np.s_[0, 0, :4]), (8, np.s_[1, 1, :5]))       # 4 and 5 voxels
    assert ei.evaluate_volumes(pred, gt)["general"]["Num Pred"] == 2
    assert ei.evaluate_volumes(pred, gt, remove_small_components=3)["general"]["Num Pred"] == 2
    assert ei.evaluate_volumes(pred, gt, remove_small_components=4)["general"]["Num Pred"] == 1     # a size equal to n goes
    assert ei.evaluate_volumes(pred, gt, remove_small_components=5)["general"]["Num Pred"] == 0
    # the voxels of all channels count: 4 + 1
    two = np.stack([pred, boxes((2, 4, 8), (7, np.s_[1, 3, 7:]))])
    assert ei.evaluate_volumes(two, gt, remove_small_components=4)["general"]["Num Pred"] == 2


@pytest.mark.parametrize("criterion", ["iou", "cldice"])
def test_empty_sides(criterion):
    some = boxes((4, 6, 6), (1, np.s_[:, :3, :]))
    none = np.zeros_like(some)
    extra = dict(add_general_metrics=["avg_f1_cov_score"], add_multi_thresh_metrics=["avg_tp_skel_coverage"]) \
        if criterion == "cldice" else {}
    for pred, gt, want in ((none, none, (0, 0, 0)), (none, some, (0, 0, 1)), (some, none, (0, 1, 0))):
        d = ei.evaluate_volumes(pred, gt, localization_criterion=criterion, evaluate_false_labels=True, **extra)
        assert d["general"]["Num GT"] == want[2] and d["general"]["Num Pred"] == want[1]
        for th in THS:
            e = d["confusion_matrix"][th]
            assert (e["AP_TP"], e["AP_FP"], e["AP_FN"]) == want
            assert e["precision"] == e["recall"] == e["fscore"] == e["AP"] == 0.0
        assert d["confusion_matrix"]["avFscore"] == 0.0
        if extra:
            assert d["general"]["avg_gt_skel_coverage"] == 0.0 and d["general"]["avg_f1_cov_score"] == 0.0


def test_inputs_are_checked():
    ok = np.ones((2, 3, 4), dtype=np.int32)
    with pytest.raises(ValueError, match="spatial shape"):
        ei.evaluate_volumes(ok, np.ones((2, 3, 5), dtype=np.int32), keep_gt_shape=True)
    with pytest.raises(ValueError, match=r"\[0, 2\^32\)"):
        ei.evaluate_volumes(-ok, ok)
    with pytest.raises(NotImplementedError, match="3-d"):
        ei.evaluate_volumes(ok[0], ok[0], localization_criterion="cldice")
    d = ei.evaluate_volumes(ok[0], ok[0])                                     # 2-d: a leading unit z
    assert d["general"] == {"Num GT": 1, "Num Pred": 1}


def test_a_3d_array_is_one_channel_whatever_overlapping_inst_says():
    gt = boxes((4, 8, 8), (1, np.s_[:, :4, :]), (2, np.s_[:, 4:, :]))
    pred = boxes((4, 8, 8), (5, np.s_[:, :5, :]), (6, np.s_[:, 5:, :]))
    want = ei.evaluate_volumes(pred, gt)
    assert ei.evaluate_volumes(pred, gt, overlapping_inst=True) == want
    assert ei.evaluate_volumes(pred[None], gt, overlapping_inst=True) == want       # (L, Z, Y, X) against (Z, Y, X)
    # 2-d results with one instance per channel go in with their unit z
    d = ei.evaluate_volumes(pred[:, None], gt[:1], overlapping_inst=True)
    assert d["general"] == {"Num GT": 2, "Num Pred": 2}


# ---------------------------------------------------------------------------------------------
# cldice against the skeletons made directly with the host thinning
# ---------------------------------------------------------------------------------------------
def tubes():
    gt = np.zeros((12, 16, 30), dtype=np.uint32)
    gt[2:5, 2:5, 2:28] = 1
    gt[7:10, 9:12, 2:28] = 2
    pred = np.zeros_like(gt)
    pred[2:5, 3:6, 2:28] = 11            # tube 1 shifted by one row
    pred[7:10, 9:12, 6:30] = 12          # tube 2 shifted along its axis
    return gt, pred


def test_cldice_equals_the_definition_on_host_skeletons():
    from patchperpix_amd import postprocess
    gt, pred = tubes()
    sg, sp = postprocess.skeletonize_instances(gt), postprocess.skeletonize_instances(pred)
    g_ids, p_ids = [1, 2], [11, 12]
    prec = np.array([[((sp == p) & (gt == g)).sum() / (sp == p).sum() for p in p_ids] for g in g_ids])
    rec = np.array([[((sg == g) & (pred == p)).sum() / (sg == g).sum() for p in p_ids] for g in g_ids])
    with np.errstate(invalid="ignore"):
        score = np.where(prec + rec > 0, 2 * prec * rec / (prec + rec), 0.0)
    assert score[0, 1] == 0 and score[1, 0] == 0 and 0 < score[1, 1] < 1      # the case has something to say
    cov = np.minimum([rec[0, 0] if prec[0, 0] > 0 else 0.0, rec[1, 1] if prec[1, 1] > 0 else 0.0], 1.0)
    d = ei.evaluate_volumes(pred, gt, localization_criterion="cldice", assignment_strategy="greedy",
                            evaluate_false_labels=True, add_general_metrics=["avg_gt_skel_coverage", "avg_f1_cov_score"],
                            add_multi_thresh_metrics=["avg_tp_skel_coverage"])
    fscores = []
    for k, th in enumerate(THS, start=1):
        t = k / 10
        e = d["confusion_matrix"][th]
        matched = [g for g in range(2) if score[g, g] > t]
        tp = len(matched)
        assert (e["AP_TP"], e["AP_FP"], e["AP_FN"]) == (tp, 2 - tp, 2 - tp), th
        assert e["false_merge"] == 0 and e["false_split"] == 0
        assert e["avg_tp_skel_coverage"] == (float(np.mean(cov[matched])) if matched else 0.0)
        fscores.append(tp / 2)
    assert d["confusion_matrix"]["avFscore"] == float(np.mean(fscores))
    assert d["general"]["avg_gt_skel_coverage"] == float(np.mean(cov))
    assert d["general"]["avg_f1_cov_score"] == 0.5 * float(np.mean(fscores)) + 0.5 * float(np.mean(cov))
    assert d == ei.evaluate_volumes(pred, gt, localization_criterion="cldice", assignment_strategy="hungarian",
                                    evaluate_false_labels=True,
                                    add_general_metrics=["avg_gt_skel_coverage", "avg_f1_cov_score"],
                                    add_multi_thresh_metrics=["avg_tp_skel_coverage"])


# ---------------------------------------------------------------------------------------------
# invariance
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("criterion", ["iou", "cldice"])
def test_dict_is_invariant_under_id_permutation_and_channel_split(criterion):
    from patchperpix_amd import synth
    gt = synth.cell_labels((8, 12, 14), cell=5, seed=1).astype(np.uint32)
    pred = synth.cell_labels((8, 12, 14), cell=4, seed=2).astype(np.uint32)
    kw = dict(localization_criterion=criterion, assignment_strategy="greedy", evaluate_false_labels=True)
    if criterion == "cldice":
        kw.update(add_general_metrics=["avg_f1_cov_score"], add_multi_thresh_metrics=["avg_tp_skel_coverage"])
    base = ei.evaluate_volumes(pred, gt, **kw)
    assert base["general"]["Num GT"] > 3 and 0 < base["confusion_matrix"]["avFscore"] < 1
    rng = np.random.default_rng(0)

    def permuted(m):
        ids = np.unique(m[m != 0])
        new = rng.permutation(ids.astype(np.uint64) * 65537 % (2 ** 32 - 5) + 1).astype(np.uint32)
        assert len(np.unique(new)) == len(ids)
        table = dict(zip(ids.tolist(), new.tolist()))
        return np.vectorize(lambda v: table.get(v, 0), otypes=[np.uint32])(m)
    assert ei.evaluate_volumes(permuted(pred), gt, **kw) == base
    assert ei.evaluate_volumes(pred, permuted(gt), **kw) == base
    # a map without overlaps split into two channels by id
    ids = np.unique(pred[pred != 0])
    first = np.isin(pred, ids[::2])
    split = np.stack([np.where(first, pred, 0), np.where(first, 0, pred)]).astype(np.uint32)
    assert ei.evaluate_volumes(split, gt, **kw) == base
    ids = np.unique(gt[gt != 0])
    first = np.isin(gt, ids[::3])
    assert ei.evaluate_volumes(pred, np.stack([np.where(first, gt, 0), np.where(first, 0, gt)]), **kw) == base


# ---------------------------------------------------------------------------------------------
# files and the task
# ---------------------------------------------------------------------------------------------
def test_toml_round_trip(tmp_path):
    d = {"general": {"Num GT": 3, "a-b_c": True, "name": 'q"uo\\te'},
         "confusion_matrix": {"avFscore": 0.1 + 0.2, "th_0_1": {"AP_TP": 0, "fscore": 1e-300, "x": -0.0},
                              "th_0_2": {"deeper": {"v": 2.5}}}}
    fn = tmp_path / "d.toml"
    fn.write_text(ei.toml_dumps(d))
    assert run_ppp.load_config([str(fn)]) == d
    with pytest.raises(TypeError):
        ei.toml_dumps({"a": [1, 2]})


def _write_hdf(fn, key, array):
    with minihdf5.File(str(fn), "w") as f:
        f.create_dataset(key, data=array, dtype=array.dtype, compression="gzip")


def test_evaluate_file_reads_back_unless_from_scratch(tmp_path):
    gt, pred = tubes()
    _write_hdf(tmp_path / "s1.hdf", "vote_instances", pred)
    _write_hdf(tmp_path / "gt.hdf", "volumes/gt", gt)
    kw = dict(res_key="vote_instances", gt_key="volumes/gt", out_dir=str(tmp_path / "out"), suffix="_x")
    first = ei.evaluate_file(str(tmp_path / "s1.hdf"), str(tmp_path / "gt.hdf"), **kw)
    assert first == ei.evaluate_volumes(pred, gt)
    assert os.listdir(str(tmp_path / "out")) == ["s1_x.toml"]
    _write_hdf(tmp_path / "s1.hdf", "garbage", np.zeros((1,), dtype=np.uint8))     # res_key is gone
    assert ei.evaluate_file(str(tmp_path / "s1.hdf"), str(tmp_path / "gt.hdf"), **kw) == first
    with pytest.raises(KeyError):
        ei.evaluate_file(str(tmp_path / "s1.hdf"), str(tmp_path / "gt.hdf"), from_scratch=True, **kw)


@pytest.mark.parametrize("kwargs, name", [
    (dict(visualize=True), "visualize"), (dict(partly=True), "partly"), (dict(foreground_only=True), "foreground_only"),
    (dict(filterSz=5), "filterSz"), (dict(unique_false_labels=True), "unique_false_labels"),
    (dict(add_general_metrics=["avg_f1_cov_score", "nope_general"]), "nope_general"),
    (dict(add_multi_thresh_metrics=["nope_multi"]), "nope_multi"),
    (dict(localization_criterion="euclid"), "euclid"), (dict(assignment_strategy="random"), "random"),
    (dict(add_general_metrics=["avg_gt_skel_coverage"], localization_criterion="iou"), "avg_gt_skel_coverage"),
])
def test_unserved_kwargs_are_refused_by_name(tmp_path, kwargs, name):
    gt, pred = tubes()
    _write_hdf(tmp_path / "s.hdf", "k", pred)
    _write_hdf(tmp_path / "gt.hdf", "k", gt)
    kw = dict(dict(localization_criterion="cldice"), **kwargs)
    with pytest.raises(NotImplementedError, match=name):
        ei.evaluate_file(str(tmp_path / "s.hdf"), str(tmp_path / "gt.hdf"), res_key="k", gt_key="k", **kw)
    with pytest.raises(NotImplementedError, match=name):
        ei.evaluate_volumes(pred, gt, **kw)
    assert not os.path.exists(str(tmp_path / "s.toml"))


def test_debug_and_falsy_switches_are_accepted():
    gt, pred = tubes()
    want = ei.evaluate_volumes(pred, gt)
    assert ei.evaluate_volumes(pred, gt, debug=True, visualize=False, partly=False, foreground_only=False, filterSz=None,
                               unique_false_labels=False, visualize_type="nuclei") == want
    with pytest.raises(TypeError, match="no_such_switch"):
        ei.evaluate_volumes(pred, gt, no_such_switch=1)


CONFIG = """
[general]
debug = false
[data]
test_data = "%s"
gt_key = "gt"
input_format = "%s"
[vote_instances]
output_format = "%s"
one_instance_per_channel = false
[evaluation]
res_key = "vote_instances"
metric = "confusion_matrix.avFscore"
localization_criterion = "iou"
assignment_strategy = "greedy"
evaluate_false_labels = true
remove_small_components = 2
summary = ["general.Num GT", "confusion_matrix.avFscore", "confusion_matrix.th_0_5.AP_TP", "confusion_matrix.th_0_5.false_split"]
%s
"""


def _write(fn, fmt, key, array):
    if fmt == "hdf":
        _write_hdf(fn, key, array)
    else:
        minizarr.open(str(fn), "a").create_dataset(key, data=array, chunks=array.shape)


@pytest.mark.parametrize("layout", ["one_file", "folder"])
@pytest.mark.parametrize("fmt", ["hdf", "zarr"])
def test_run_ppp_evaluate(tmp_path, fmt, layout, caplog):
    gt, pred = tubes()
    samples = {"sample_a": (pred, gt), "sample_b": (pred[:, ::-1].copy(), gt)}
    out = tmp_path / "out"
    out.mkdir()
    if layout == "one_file":
        data = tmp_path / ("val." + fmt)
    else:
        data = tmp_path / "val"
        data.mkdir()
    for name, (p, g) in samples.items():
        _write(out / (name + "." + fmt), fmt, "vote_instances", p)
        if layout == "one_file":
            if fmt == "hdf":
                mode = "a" if data.exists() else "w"
                with minihdf5.File(str(data), mode) as f:
                    f.create_dataset(name + "/gt", data=g, dtype=g.dtype, compression="gzip")
            else:
                minizarr.open(str(data), "a").create_dataset(name + "/gt", data=g, chunks=g.shape)
        else:
            _write(data / (name + "." + fmt), fmt, "gt", g)
    cfg = tmp_path / "config.toml"
    cfg.write_text(CONFIG % (data, fmt, fmt, ""))
    argv = ["-c", str(cfg), "--do", "evaluate", "--pred-folder", str(tmp_path), "--output-folder", str(out)]
    with caplog.at_level("INFO"):
        run_ppp.main(argv)
    want = {name: ei.evaluate_volumes(p, g, assignment_strategy="greedy", evaluate_false_labels=True,
                                      remove_small_components=2) for name, (p, g) in samples.items()}
    assert want["sample_a"] != want["sample_b"]
    for name in samples:
        assert run_ppp.load_config([str(out / (name + ".toml"))]) == want[name]
        assert "confusion_matrix.avFscore sample %-19s: %.4f" % (name, want[name]["confusion_matrix"]["avFscore"]) in caplog.text
    lines = (out / "summary.csv").read_text().splitlines()
    assert lines[0] == "sample,general.Num GT,confusion_matrix.avFscore,confusion_matrix.th_0_5.AP_TP,confusion_matrix.th_0_5.false_split"
    assert len(lines) == 3
    for line, name in zip(lines[1:], sorted(samples)):
        cells = line.split(",")
        d = want[name]
        assert cells[0] == name and int(cells[1]) == d["general"]["Num GT"] == 2
        assert float(cells[2]) == d["confusion_matrix"]["avFscore"]
        assert int(cells[3]) == d["confusion_matrix"]["th_0_5"]["AP_TP"]
        assert int(cells[4]) == d["confusion_matrix"]["th_0_5"]["false_split"]


def test_run_ppp_evaluate_returns_the_mean_and_refuses_skeleton_coverage(tmp_path):
    import argparse
    gt, pred = tubes()
    out = tmp_path / "out"
    out.mkdir()
    _write_hdf(out / "a.hdf", "vote_instances", pred)
    _write_hdf(out / "b.hdf", "vote_instances", gt)
    with minihdf5.File(str(tmp_path / "val.hdf"), "w") as f:
        f.create_dataset("a/gt", data=gt, dtype=gt.dtype, compression="gzip")
        f.create_dataset("b/gt", data=gt, dtype=gt.dtype, compression="gzip")
    cfg = tmp_path / "config.toml"
    cfg.write_text(CONFIG % (tmp_path / "val.hdf", "hdf", "hdf", ""))
    args = argparse.Namespace(output_folder=str(out), pred_folder=str(tmp_path), sample=None)
    mean = run_ppp.evaluate(args, run_ppp.load_config([str(cfg)]))
    a = ei.evaluate_volumes(pred, gt, assignment_strategy="greedy", remove_small_components=2)["confusion_matrix"]["avFscore"]
    assert mean == (a + 1.0) / 2
    args.sample = "b"
    assert run_ppp.evaluate(args, run_ppp.load_config([str(cfg)])) == 1.0
    for key in ("evaluate_skeleton_coverage", "print_f_factor_perc_gt_0_8"):
        cfg.write_text(CONFIG % (tmp_path / "val.hdf", "hdf", "hdf", key + " = true"))
        with pytest.raises(NotImplementedError, match=key):
            run_ppp.evaluate(args, run_ppp.load_config([str(cfg)]))
    cfg.write_text(CONFIG % (tmp_path / "val.hdf", "hdf", "hdf", ""))
    config = run_ppp.load_config([str(cfg)])
    config["data"]["add_partly_val"] = True
    with pytest.raises(NotImplementedError, match="add_partly_val"):
        run_ppp.evaluate(args, config)


def test_run_ppp_evaluate_takes_the_per_channel_gt_key(tmp_path):
    """[data] one_instance_per_channel_gt replaces the gt key when one_instance_per_channel is set, and only then"""
    import argparse
    gt, pred = tubes()
    out = tmp_path / "out"
    out.mkdir()
    _write_hdf(out / "a.hdf", "vote_instances", pred[None])
    with minihdf5.File(str(tmp_path / "val.hdf"), "w") as f:
        f.create_dataset("a/gt", data=gt, dtype=gt.dtype, compression="gzip")
        f.create_dataset("per_channel", data=pred[None], dtype=pred.dtype, compression="gzip")
    cfg = tmp_path / "config.toml"
    cfg.write_text(CONFIG % (tmp_path / "val.hdf", "hdf", "hdf", "from_scratch = true"))
    args = argparse.Namespace(output_folder=str(out), pred_folder=str(tmp_path), sample=None)
    config = run_ppp.load_config([str(cfg)])
    config["data"]["one_instance_per_channel_gt"] = "per_channel"
    plain = run_ppp.evaluate(args, config)
    assert plain < 1.0                                   # scored against a/gt
    config["vote_instances"]["one_instance_per_channel"] = True
    assert run_ppp.evaluate(args, config) == 1.0         # scored against per_channel, which is the prediction
