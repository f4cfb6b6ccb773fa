"""The host side of the `postprocess` task (reference: PatchPerPix/util/postprocess.py:77-119, called from
experiments/run_ppp.py:2230-2259): one 3-d skeleton per instance (postprocess.skeletonize_instances, the
DEFINITION of the device pass of tests/test_skeleton_labels_gpu.py), the NRRD writer, the datasets
`postprocess_instances` writes and the task in run_ppp.  Native host functions only; every comparison is
np.array_equal on integers.  Parity with scikit-image's skeletonize_3d stays unpinned (tests/test_skeleton.py)."""
import gzip
import os

import numpy as np
import pytest

from patchperpix_amd import backend, minihdf5, mininrrd, postprocess, run_ppp, synth


def literal_loop(inst):
    """postprocess.py:110-112 with the library's thinning: one whole-volume thinning per instance"""
    out = np.zeros_like(inst)
    for lbl in np.unique(inst):
        if lbl != 0:
            out[backend.host_skeletonize_3d(inst == lbl)] = lbl
    return out


def _maps():
    rng = np.random.default_rng(5)
    flat = np.zeros((5, 12, 14), np.uint16)          # instances of ONE slice in a volume of several
    flat[2, 2:9, 3:11] = 4
    flat[4, 1:6, 1:9] = 9
    flat[0:2, 8:12, 0:14] = 70
    far = np.zeros((6, 10, 30), np.uint32)           # one instance of two far components, one in between
    far[1:5, 1:5, 1:6] = 3
    far[2:6, 5:10, 22:30] = 3
    far[0:6, 2:8, 10:16] = 2 ** 31 + 5
    return {"cells": synth.cell_labels((8, 12, 20), cell=5).astype(np.uint32),
            "noise": rng.integers(0, 4, (6, 9, 11)).astype(np.int32),
            "flat": flat, "far": far,
            "tubes": synth.tube_labels((14, 16, 18), n_tubes=3, radius=2, seed=1).astype(np.uint16),
            "slice": synth.cell_labels((1, 20, 24), cell=5).astype(np.uint16)[0]}


MAPS = _maps()


@pytest.mark.parametrize("name", sorted(MAPS))
def test_skeletonize_instances_is_the_literal_loop_and_the_crop_changes_nothing(name):
    inst = MAPS[name]
    want = literal_loop(inst)
    whole = postprocess.skeletonize_instances(inst, crop=False)
    boxed = postprocess.skeletonize_instances(inst)
    assert whole.dtype == inst.dtype and whole.shape == inst.shape
    assert np.array_equal(whole, want)
    assert boxed.dtype == inst.dtype and np.array_equal(boxed, want)
    assert np.array_equal(np.unique(want), np.unique(inst)), "an instance lost its skeleton"


def test_touching_instances_are_not_thinned_as_one_mask():
    inst = synth.cell_labels((8, 12, 20), cell=5).astype(np.uint32)
    got = postprocess.skeletonize_instances(inst)
    assert not np.array_equal(got != 0, backend.host_skeletonize_3d(inst != 0))
    for lbl in np.unique(inst):
        if lbl != 0:
            assert np.array_equal(got == lbl, backend.host_skeletonize_3d(inst == lbl))


def test_device_function_raises_without_a_device(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no HIP device"):
        backend.skeletonize_labels(MAPS["cells"])


# ---------------------------------------------------------------------------------------------
# mininrrd
# ---------------------------------------------------------------------------------------------
def test_nrrd_header_and_payload(tmp_path):
    rng = np.random.default_rng(0)
    mask = rng.random((3, 5, 7)) < 0.3
    fn = str(tmp_path / "m.nrrd")
    mininrrd.write(fn, mask)
    raw = open(fn, "rb").read()
    head, payload = raw.split(b"\n\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "NRRD0004"
    fields = dict(line.split(": ", 1) for line in lines[1:])
    assert fields == {"type": "uint8", "dimension": "3", "sizes": "7 5 3", "encoding": "gzip"}   # X Y Z
    # the bytes pynrrd writes for mask.transpose(2, 1, 0) in Fortran order = the C-order (Z, Y, X) mask
    assert gzip.decompress(payload) == mask.astype(np.uint8).tobytes()
    assert gzip.decompress(payload) == mask.astype(np.uint8).transpose(2, 1, 0).tobytes(order="F")
    got_fields, got = mininrrd.read(fn)
    assert got_fields["sizes"] == "7 5 3" and got.dtype == np.uint8 and np.array_equal(got, mask.astype(np.uint8))
    with pytest.raises(ValueError):
        mininrrd.write(fn, mask[0])


# ---------------------------------------------------------------------------------------------
# postprocess_instances (host) and the task
# ---------------------------------------------------------------------------------------------
RES_KEY = "vote_instances"


def _result_map():
    """instances of 40 - 125 voxels, three small ones (<= 6 voxels) and ids that are not consecutive"""
    inst = np.zeros((8, 14, 22), np.uint16)
    inst[:, :, :] = synth.cell_labels(inst.shape, cell=5)
    inst[0, 0, 0:3] = 60001
    inst[7, 13, 16:22] = 60002
    inst[3, 0, 0] = 60003
    return inst


def _write(folder, name, inst):
    fn = os.path.join(str(folder), name + ".hdf")
    with minihdf5.File(fn, "w") as f:
        f.create_dataset(RES_KEY, data=inst, compression="gzip")
    return fn


def _read(fn, key):
    with minihdf5.File(fn, "r") as f:
        ds = f[key]
        return np.asarray(ds), ds.dtype, ds.attrs.get("skeletonize_instances")


def test_postprocess_instances_on_the_host(tmp_path, monkeypatch):
    monkeypatch.setenv("PPP_POSTPROCESS", "host")
    inst = _result_map()
    fn = _write(tmp_path, "sample_a", inst)
    out = tmp_path / "out"
    kw = dict(res_key=RES_KEY, remove_small_comps=6, export_skeleton_nrrds=True, export_skeleton_labels=True)
    postprocess.postprocess_instances([fn], str(out), **kw)
    want = postprocess.relabel(postprocess.remove_small_components(inst, 6))
    assert want.max() < inst.max() and len(np.unique(want)) == len(np.unique(inst)) - 3
    got, dtype, by = _read(fn, RES_KEY + "_rm_6")
    assert dtype == np.uint16 and np.array_equal(got, want) and by == "ppp_host_skeletonize_3d"
    assert np.array_equal(_read(fn, RES_KEY)[0], inst), "the input dataset was changed"
    skel, sdtype, sby = _read(fn, RES_KEY + "_rm_6_skeleton")
    assert sdtype == np.uint16 and sby == "ppp_host_skeletonize_3d" and np.array_equal(skel, literal_loop(want))
    # one file per surviving id; their union is the skeleton map
    ids = [int(v) for v in np.unique(want) if v != 0]
    assert sorted(os.listdir(str(out))) == sorted("sample_a_%d.nrrd" % v for v in ids)
    union = np.zeros_like(want)
    for v in ids:
        fields, m = mininrrd.read(str(out / ("sample_a_%d.nrrd" % v)))
        assert fields["sizes"] == "22 14 8" and set(np.unique(m)) == {0, 1} and not union[m != 0].any()
        union[m != 0] = v
    assert np.array_equal(union, skel)

    # a second run replaces the dataset (another threshold writes another one next to it)
    with minihdf5.File(fn, "a") as f:
        f.create_dataset(RES_KEY + "_rm_6", data=np.zeros((2, 2), np.uint8))
    postprocess.postprocess_instances([fn], str(out), res_key=RES_KEY, remove_small_comps=6)
    got, dtype, _ = _read(fn, RES_KEY + "_rm_6")
    assert dtype == np.uint16 and np.array_equal(got, want)
    postprocess.postprocess_instances([fn], str(out), res_key=RES_KEY, remove_small_comps=3)
    assert np.array_equal(_read(fn, RES_KEY + "_rm_3")[0], postprocess.relabel(postprocess.remove_small_components(inst, 3)))


def test_dtype_rule_at_65535_ids(tmp_path, monkeypatch):
    """uint16 when the cleaned maximum is < 65535, else uint32 (postprocess.py:92-95): 65535 and 65534
    surviving instances of two voxels each"""
    monkeypatch.setenv("PPP_POSTPROCESS", "host")
    n = 65535
    flat = np.zeros(2 * n + 10, np.uint32)
    flat[:2 * n] = np.repeat(np.arange(n, dtype=np.uint32) * 3 + 7, 2)      # two voxels per id
    flat[2 * n:2 * n + 4] = 10 ** 6 + np.arange(4, dtype=np.uint32)         # single voxels: dropped
    inst = flat.reshape(2, 5, -1)
    fn = _write(tmp_path, "many", inst)
    postprocess.postprocess_instances([fn], str(tmp_path), res_key=RES_KEY, remove_small_comps=1)
    got, dtype, by = _read(fn, RES_KEY + "_rm_1")
    want = postprocess.relabel(postprocess.remove_small_components(inst, 1))
    assert int(want.max()) == 65535 and dtype == np.uint32 and np.array_equal(got, want) and by is None
    inst2 = inst.copy()
    inst2[inst2 == 7] = 0                                                    # one instance fewer: 65534
    fn2 = _write(tmp_path, "fewer", inst2)
    postprocess.postprocess_instances([fn2], str(tmp_path), res_key=RES_KEY, remove_small_comps=1)
    got2, dtype2, _ = _read(fn2, RES_KEY + "_rm_1")
    assert int(got2.max()) == 65534 and dtype2 == np.uint16
    assert np.array_equal(got2, postprocess.relabel(postprocess.remove_small_components(inst2, 1)))
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".nrrd")], "skeletons nobody asked for"


CONFIG = """
[vote_instances]
output_format = "hdf"
[evaluation]
res_key = "vote_instances"
[postprocessing]
process_instances = true
remove_small_comps = 6
export_skeleton_nrrds = true
%s
"""


def test_run_ppp_postprocess_task(tmp_path, monkeypatch):
    monkeypatch.setenv("PPP_POSTPROCESS", "host")
    inst = _result_map()
    folder = tmp_path / "inst"
    folder.mkdir()
    fn_a, fn_b = _write(folder, "sample_a", inst), _write(folder, "sample_b", inst[:, ::-1].copy())
    cfg = tmp_path / "config.toml"
    cfg.write_text(CONFIG % "")
    argv = ["--config", str(cfg), "--do", "postprocess", "--pred-folder", str(tmp_path), "--output-folder", str(folder)]
    run_ppp.main(argv + ["--sample", "sample_a"])
    want = postprocess.relabel(postprocess.remove_small_components(inst, 6))
    assert np.array_equal(_read(fn_a, RES_KEY + "_rm_6")[0], want)
    with minihdf5.File(fn_b, "r") as f:
        assert RES_KEY + "_rm_6" not in f, "--sample was ignored"
    with minihdf5.File(fn_a, "r") as f:
        assert RES_KEY + "_rm_6_skeleton" not in f, "export_skeleton_labels is off unless asked for"
    n_ids = len(np.unique(want)) - 1
    assert len([f for f in os.listdir(str(folder)) if f.startswith("sample_a_") and f.endswith(".nrrd")]) == n_ids
    run_ppp.main(argv)
    assert np.array_equal(_read(fn_b, RES_KEY + "_rm_6")[0],
                          postprocess.relabel(postprocess.remove_small_components(inst[:, ::-1], 6)))

    refused = tmp_path / "fg.toml"
    refused.write_text(CONFIG % "process_fg_prediction = true")
    with pytest.raises(NotImplementedError, match="process_fg_prediction"):
        run_ppp.main(["--config", str(refused), "--do", "postprocess", "--pred-folder", str(tmp_path),
                      "--output-folder", str(folder)])
