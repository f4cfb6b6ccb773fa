"""GPU: the `validate` task (patchperpix_amd.validate) end to end -- the sweep against separate `label` +
`evaluate` runs file for file, one load per sample (the session's counters and the container's own reads), the
three residency branches, `vote_from_code` with the rows decoded once, the command line and ``prediction_only``.
Integers and files throughout: every comparison is equality, there is no tolerance anywhere."""
import argparse
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, REPO
from patchperpix_amd import minizarr, run_ppp, synth, validate as val
from patchperpix_amd.vote_instances import utilVoteInstances as util
from test_cli_gpu import _load_result
from test_compact_gpu import p7_case  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

SHAPE, PS, MARGIN, SPECK = (22, 24, 26), (5, 5, 5), 4, 5
THRESHS = [[0.9, 0.1], [0.334, 0.334]]
BASE = os.path.join(GOLDEN_DIR, "label_config_flylight_zarr.toml")

EXTRA = """
[general]
overwrite = false
[data]
val_data = "{val}"
test_data = "{val}"
gt_key = "gt"
input_format = "zarr"
[vote_instances]
only_bb = true
ignore_small_comps = {speck}
skeletonize_foreground = false
[evaluation]
res_key = "vote_instances"
metric = "confusion_matrix.avFscore"
localization_criterion = "iou"
[validation]
checkpoints = [100]
params_zip = ["patch_threshold", "fc_threshold"]
patch_threshold = [0.5, 0.8]
fc_threshold = [0.5, 0.8]
params_product = ["mws", "numinst_threshs"]
mws = [false, true]
numinst_threshs = [[0.9, 0.1], [0.334, 0.334]]
"""


def make_sample(seed):
    """labels and the overlap field of synth.make_case, cut back to a background margin wider than the patch
    radius, plus one speck of 2 voxels in the margin; the prediction is that of the cut labels"""
    c = synth.make_case(SHAPE, PS, seed=seed, kind="cells", cell=[7, 7, 7], overlap_frac=0.05)
    inner = tuple(slice(MARGIN, s - MARGIN) for s in SHAPE)
    lab = np.zeros(SHAPE, dtype=np.int64)
    lab[inner] = c["labels"][inner]
    lab[1, 1, 1:3] = 70000                                       # the speck
    numinst = np.where(lab != 0, np.maximum(c["numinst"], 1), 0).astype(np.uint8)
    numinst[1, 1, 1:3] = 1
    pred16 = synth.pred_from_labels(lab, PS, seed=seed).astype(np.float16)
    prob = np.zeros((3,) + SHAPE, dtype=np.float16)              # channel k = P(k instances)
    prob[0][numinst == 0] = 0.97
    prob[1][numinst == 1] = 0.95
    prob[1][numinst == 2] = 0.6                                  # 2 under [0.9, 0.1], 1 under [0.334, 0.334]
    prob[2][numinst == 2] = 0.3
    return lab, pred16, prob


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    root = tmp_path_factory.mktemp("validate")
    pred_dir = root / "pred"
    names = ["vs_a", "vs_b"]
    gt = minizarr.open(str(root / "val.zarr"), "w")
    for name, seed in zip(names, (81, 82)):
        lab, pred16, prob = make_sample(seed)
        fields = [util.numinst_from_prob(prob, numinst_threshs=t) for t in THRESHS]
        assert not np.array_equal(fields[0], fields[1]) and np.array_equal(fields[0] > 0, fields[1] > 0)
        fg = fields[0] > 0
        nz = np.nonzero(fg & (lab != 70000))
        assert all(int(nz[i].min()) > PS[i] // 2 and int(nz[i].max()) < SHAPE[i] - 1 - PS[i] // 2 for i in range(3))
        assert int((lab == 70000).sum()) == 2 < SPECK and fg[1, 1, 1]
        zf = minizarr.open(str(pred_dir / (name + ".zarr")), "w")
        zf.create_dataset("volumes/pred_affs", data=pred16, chunks=(pred16.shape[0], 12, 12, 13))
        zf.create_dataset("volumes/pred_numinst", data=prob, chunks=(3, 12, 12, 13))
        gt.create_dataset(name + "/gt", data=lab.astype(np.uint32), chunks=SHAPE)
        gt.create_dataset(name + "/gt_channels", data=lab.astype(np.uint32)[None], chunks=(1,) + SHAPE)
    extra = root / "extra.toml"
    extra.write_text(EXTRA.format(val=str(root / "val.zarr"), speck=SPECK))
    config = run_ppp.load_config([BASE, str(extra)])
    return dict(root=root, pred=str(pred_dir), names=names, config=config, configs=[BASE, str(extra)],
                sets=val.param_sets_of(config))


class Reads:
    """the reads of ``volumes/pred_affs`` that reach the store (minizarr.Array._read), by sample"""

    def __init__(self, mp):
        self.by_sample = {}
        real = minizarr.Array._read

        def counted(arr, ranges, out):
            if arr.path.rstrip("/").endswith("pred_affs"):
                store = os.path.dirname(os.path.dirname(arr.path.rstrip("/")))
                sample = os.path.splitext(os.path.basename(store))[0]
                self.by_sample[sample] = self.by_sample.get(sample, 0) + 1
            return real(arr, ranges, out)
        mp.setenv("PPP_ZARR", "mini")
        mp.setattr(minizarr.Array, "_read", counted)


def record_sessions(mp):
    sessions, base = [], val.SampleSession

    class Recorded(base):
        def __init__(self, *args):
            base.__init__(self, *args)
            sessions.append(self)
    mp.setattr(val, "SampleSession", Recorded)
    return sessions


def run_sweep(world, out, mode, **kw):
    with pytest.MonkeyPatch.context() as mp:
        if mode is None:
            mp.delenv("PPP_VALIDATE_RESIDENT", raising=False)
        else:
            mp.setenv("PPP_VALIDATE_RESIDENT", mode)
        reads, sessions = Reads(mp), record_sessions(mp)
        best = val.validate_checkpoints(copy.deepcopy(world["config"]), world["pred"], str(out), **kw)
    return dict(out=out, best=best, reads=reads.by_sample, sessions=sessions)


@pytest.fixture(scope="module")
def sweep(world):
    return run_sweep(world, world["root"] / "sweep", "device")


@pytest.fixture(scope="module")
def separate(world):
    """every set as `label` + `evaluate` of its own, into a fresh folder: (folders, metrics, reads)"""
    folders, metrics = [], []
    with pytest.MonkeyPatch.context() as mp:
        reads = Reads(mp)
        for k, s in enumerate(world["sets"]):
            config = copy.deepcopy(world["config"])
            config["vote_instances"].update(copy.deepcopy(s))
            folder = world["root"] / ("separate_%d" % k)
            args = argparse.Namespace(pred_folder=world["pred"], output_folder=str(folder), sample=None, checkpoint=None)
            run_ppp.label(args, config)
            metrics.append(run_ppp.evaluate(args, config))
            folders.append(str(folder))
    return folders, metrics, reads.by_sample


def set_folder(out, kind, s, checkpoint=100):
    return os.path.join(str(out), kind, str(checkpoint), *val.params_str(s))


def same_results(a_folder, b_folder, names):
    for name in names:
        a, b = _load_result(a_folder, name), _load_result(b_folder, name)
        assert set(a) == set(b) and "vote_instances" in a
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (a_folder, name, k)


# ---- 1 ----------------------------------------------------------------------------------------------
def test_sweep_equals_separate_runs(world, sweep, separate):
    folders, metrics, _ = separate
    sets, names = world["sets"], world["names"]
    assert len(sets) == 8
    for s, folder in zip(sets, folders):
        same_results(set_folder(sweep["out"], "instanced", s), folder, names)
        for name in names:
            got = run_ppp.load_config([os.path.join(set_folder(sweep["out"], "evaluated", s), name + ".toml")])
            assert got == run_ppp.load_config([os.path.join(folder, name + ".toml")])
    results = json.load(open(os.path.join(str(sweep["out"]), "results.json")))
    assert [r["metric"] for r in results] == [str(m) for m in metrics]
    assert [r["params"] for r in results] == [dict(s, filterSz=None, res_key="vote_instances") for s in sets]
    assert sweep["best"] == (100, dict(sets[int(np.argmax(metrics))], filterSz=None, res_key="vote_instances"))
    # not vacuous: the sets give different maps, instances exist, the speck and everything outside the box is empty
    for name in names:
        maps = [_load_result(f, name)["vote_instances"] for f in folders]
        assert sum(not np.array_equal(maps[0], m) for m in maps[1:]) >= 1
        assert all(m.max() > 1 for m in maps) and all(m[..., 1, 1, 1:3].max() == 0 for m in maps)
    assert 0.0 < max(metrics) <= 1.0


# ---- 2 ----------------------------------------------------------------------------------------------
def test_each_sample_is_loaded_once(world, sweep, separate):
    names = world["names"]
    assert sweep["reads"] == {n: 1 for n in names}
    assert [s.sample for s in sweep["sessions"]] == names
    for s in sweep["sessions"]:
        assert s.reads["volumes/pred_affs"] == 1 and s.reads["volumes/pred_numinst"] == 1
        assert s.sets_voted == 8 and s.h2d_copies == 1            # the upload of the first set; crops are device copies
    assert separate[2] == {n: 8 for n in names}                    # K calls of `label`: K reads


@pytest.mark.parametrize("mode", ["host", "off"])
def test_residency_branches_write_the_same_files(world, sweep, mode):
    run = run_sweep(world, world["root"] / ("sweep_" + mode), mode)
    assert run["best"] == sweep["best"]
    for s in world["sets"]:
        same_results(set_folder(run["out"], "instanced", s), set_folder(sweep["out"], "instanced", s), world["names"])
    assert open(os.path.join(str(run["out"]), "results.json")).read() == \
        open(os.path.join(str(sweep["out"]), "results.json")).read()
    if mode == "host":
        assert run["reads"] == {n: 1 for n in world["names"]}
        assert [s.h2d_copies for s in run["sessions"]] == [8, 8]   # the crop of every set crosses the bus
    else:
        assert run["reads"] == {n: 8 for n in world["names"]}
        assert all(s.reads == {} and s.h2d_copies == 8 for s in run["sessions"])   # what `label` does, 8 times


def test_existing_results_are_kept_and_complete_samples_not_opened(world, sweep):
    """the sweep again into its own folder: nothing is opened, nothing is read, the same answer"""
    stamp = os.path.getmtime(os.path.join(set_folder(sweep["out"], "instanced", world["sets"][0]), "vs_a.hdf"))
    again = run_sweep(world, sweep["out"], "device")
    assert again["sessions"] == [] and again["reads"] == {} and again["best"] == sweep["best"]
    assert os.path.getmtime(os.path.join(set_folder(sweep["out"], "instanced", world["sets"][0]), "vs_a.hdf")) == stamp


@pytest.mark.parametrize("stream", [True, False], ids=["streamed", "resident"])
def test_foreground_from_the_centre_channel(world, tmp_path, stream):
    """no numinst key: the foreground is the centre channel of the affinities.  Streamed, the session never holds
    the array (no read of it through the caching reader, the channel comes from the open dataset); resident, it is
    read once and the reader keeps the centre channel only.  Result files equal those of `label`."""
    config = copy.deepcopy(world["config"])
    del config["prediction"]["numinst_key"]
    config["validation"] = dict(checkpoints=[100], params_zip=["patch_threshold", "fc_threshold"], patch_threshold=[0.5, 0.8],
                                fc_threshold=[0.5, 0.8], params_product=["mws"], mws=[False, True])
    swept = copy.deepcopy(config)
    swept["vote_instances"]["stream_prediction"] = stream
    kept = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PPP_VALIDATE_RESIDENT", "device")
        reads, sessions = Reads(mp), record_sessions(mp)
        base_close = val.SampleSession.close
        mp.setattr(val.SampleSession, "close", lambda self: kept.append(dict(self.reader.cache)) or base_close(self))
        val.validate_checkpoints(swept, world["pred"], str(tmp_path / "out"), sample="vs_a")
    (session,) = sessions
    assert session.sets_voted == 4
    if stream:
        assert "volumes/pred_affs" not in session.reads and "volumes/pred_affs" not in kept[0]
        assert reads.by_sample["vs_a"] > 4                  # tiles and the centre channel, read from the store per set
    else:
        assert session.reads == {"volumes/pred_affs": 1} and reads.by_sample == {"vs_a": 1}
        assert session.h2d_copies == 1
        assert isinstance(kept[0]["volumes/pred_affs"], val._OneChannel)
    maps = []
    for k, s in enumerate(val.param_sets_of(config)):
        one = copy.deepcopy(config)
        one["vote_instances"].update(s, stream_prediction=False)
        folder = tmp_path / ("label_%d" % k)
        run_ppp.label(argparse.Namespace(pred_folder=world["pred"], output_folder=str(folder), sample="vs_a", checkpoint=None), one)
        same_results(set_folder(tmp_path / "out", "instanced", s), str(folder), ["vs_a"])
        maps.append(_load_result(str(folder), "vs_a")["vote_instances"])
    assert all(m.max() > 1 for m in maps) and any(not np.array_equal(maps[0], m) for m in maps[1:])


# ---- 3 ----------------------------------------------------------------------------------------------
def test_vote_from_code_decodes_once_per_sample(tmp_path, p7_case, monkeypatch):  # noqa: F811
    import torch
    from patchperpix_amd import decode as dec
    from test_decode import AE_SHIPPED, _reference_named_state
    c = p7_case
    fg, shape = c["fg"], c["shape"]
    ckpt = tmp_path / "model.pt"
    torch.save({"model_state_dict": {k: v.detach().cpu() for k, v in _reference_named_state(c["d"]).items()}}, ckpt)
    prob = np.zeros((3,) + shape, dtype=np.float16)
    prob[0][~fg] = 0.97
    prob[1][fg] = 0.95
    pred_dir = tmp_path / "pred"
    zf = minizarr.open(str(pred_dir / "sampleC.zarr"), "w")
    zf.create_dataset("volumes/pred_numinst", data=prob, chunks=(3, 12, 12, 13))
    zf.create_dataset("volumes/pred_code", data=c["code"].cpu().numpy(), chunks=(176, 11, 12, 13))
    minizarr.open(str(tmp_path / "val.zarr"), "w").create_dataset("sampleC/gt", data=fg.astype(np.uint32), chunks=shape)
    ae = dict(AE_SHIPPED)
    ae.pop("input_shape_squeezed")
    lines = ["[model]", "patchshape = [7, 7, 7]", "overlapping_inst = false", "code_units = 176", "[model.autoencoder]"]
    lines += ["%s = %s" % (k, ('"%s"' % v) if isinstance(v, str) else str(v).replace("(", "[").replace(")", "]"))
              for k, v in ae.items()]
    lines += ["[prediction]", 'code_key = "volumes/pred_code"', "decode_batch_size = 2048",
              "[vote_instances]", "vote_from_code = true",
              "[data]", 'val_data = "%s"' % (tmp_path / "val.zarr"), 'gt_key = "gt"', 'input_format = "zarr"',
              "[evaluation]", 'res_key = "vote_instances"', 'metric = "confusion_matrix.avFscore"',
              "[validation]", "checkpoints = [7]", 'params_product = ["mws"]', "mws = [false, true]"]
    common = tmp_path / "common.toml"
    common.write_text("\n".join(lines) + "\n")
    calls = []
    real = dec.decode_rows
    monkeypatch.setattr(dec, "decode_rows", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.delenv("PPP_VALIDATE_RESIDENT", raising=False)
    run_ppp.main(["--config", BASE, "--config", str(common), "--do", "validate", "--checkpoint", str(ckpt),
                  "--pred-folder", str(pred_dir), "--output-folder", str(tmp_path / "val")])
    assert calls == [1]
    maps = []
    for mws in (False, True):
        one = tmp_path / ("mws_%s.toml" % mws)
        one.write_text("[vote_instances]\nmws = %s\n" % str(mws).lower())
        out = tmp_path / ("label_%s" % mws)
        run_ppp.main(["--config", BASE, "--config", str(common), "--config", str(one), "--do", "label",
                      "--checkpoint", str(ckpt), "--pred-folder", str(pred_dir), "--output-folder", str(out)])
        same_results(str(tmp_path / "val" / "instanced" / "7" / ("mws_%s" % mws)), str(out), ["sampleC"])
        maps.append(_load_result(str(out), "sampleC")["vote_instances"])
    assert calls == [1, 1, 1] and maps[0].max() > 0
    assert len(json.load(open(str(tmp_path / "val" / "results.json")))) == 2


# ---- 4 ----------------------------------------------------------------------------------------------
def _cli(world, out, *more):
    argv = [sys.executable, "-m", "patchperpix_amd.run_ppp"]
    for c in world["configs"]:
        argv += ["--config", c]
    argv += ["--do", "validate", "--pred-folder", world["pred"], "--output-folder", str(out), "--sample", "vs_a"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("PPP_VALIDATE_RESIDENT", None)
    done = subprocess.run(argv + list(more), cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert done.returncode == 0, done.stdout.decode()[-3000:]


def _leaf_folders(root):
    return sorted(os.path.relpath(r, str(root)) for r, d, _ in os.walk(str(root)) if not d)


def test_cli_val_id_runs_one_set(world, sweep, tmp_path):
    sets = world["sets"]
    _cli(world, tmp_path / "one", "--val-id", "3")
    want = os.path.join("100", *val.params_str(sets[3]))
    assert _leaf_folders(tmp_path / "one" / "instanced") == [want] == _leaf_folders(tmp_path / "one" / "evaluated")
    results = json.load(open(str(tmp_path / "one" / "results.json")))
    assert len(results) == 1 and results[0]["params"] == dict(sets[3], filterSz=None, res_key="vote_instances")
    same_results(set_folder(tmp_path / "one", "instanced", sets[3]), set_folder(sweep["out"], "instanced", sets[3]), ["vs_a"])


def test_cli_without_val_id_runs_all_sets(world, sweep, tmp_path):
    sets = world["sets"]
    _cli(world, tmp_path / "all")
    want = sorted(os.path.join("100", *val.params_str(s)) for s in sets)
    assert _leaf_folders(tmp_path / "all" / "instanced") == want == _leaf_folders(tmp_path / "all" / "evaluated")
    results = json.load(open(str(tmp_path / "all" / "results.json")))
    assert [r["params"] for r in results] == [dict(s, filterSz=None, res_key="vote_instances") for s in sets]
    for s in sets:
        same_results(set_folder(tmp_path / "all", "instanced", s), set_folder(sweep["out"], "instanced", s), ["vs_a"])


# ---- 5 ----------------------------------------------------------------------------------------------
def test_prediction_only_votes_nothing(world, tmp_path, monkeypatch):
    config = copy.deepcopy(world["config"])
    config["validation"]["checkpoints"] = [100, 200]
    config["data"]["gt_key"] = "gt_channels"                      # (the prediction is scored against (L, Z, Y, X) labels)
    config["evaluation"].update(prediction_only=True, metric="f1",
                                prediction=dict(eval_numinst_prediction=True))
    pred = tmp_path / "pred"
    pred.mkdir()
    for c in (100, 200):
        os.symlink(world["pred"], str(pred / str(c)))
    calls = []
    real = run_ppp.evaluate_prediction
    monkeypatch.setattr(run_ppp, "evaluate_prediction", lambda args, cfg: calls.append(args.pred_folder) or real(args, cfg))
    sessions = record_sessions(monkeypatch)
    assert val.validate_checkpoints(config, str(pred), str(tmp_path / "out")) == (None, None)
    assert calls == [str(pred / "100"), str(pred / "200")] and sessions == []
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["evaluated"]
    for c in ("100", "200"):
        got = json.load(open(str(tmp_path / "out" / "evaluated" / c / "prediction_metrics.json")))
        assert sorted(got) == world["names"]
