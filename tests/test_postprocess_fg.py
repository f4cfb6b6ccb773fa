"""The host side of `postprocess_fg` (reference: PatchPerPix/util/postprocess.py:122-199): the integer bound
`min_sq_distance`, `fg_filter` against the reference's own results (tests/golden/postprocess_fg/fg_*.npz, written by
gen_golden_postprocess_fg.py) and against a brute-force restatement of the definition, the two inputs the
reference leaves undefined, the uint16 wrap, the files `postprocess_fg` writes and the task in run_ppp.
Everything is an integer comparison; PPP_POSTPROCESS=host keeps the device out of it."""
import glob
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from patchperpix_amd import backend, minihdf5, mininrrd, minizarr, postprocess, run_ppp

FG_DIR = os.path.join(GOLDEN_DIR, "postprocess_fg")
GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(FG_DIR, "fg_*.npz")))


@pytest.fixture(autouse=True)
def _host_path(monkeypatch):
    monkeypatch.setenv("PPP_POSTPROCESS", "host")


# ---------------------------------------------------------------------------------------------
# inputs shared with tests/test_postprocess_fg_gpu.py
# ---------------------------------------------------------------------------------------------
def golden(name):
    z = np.load(os.path.join(FG_DIR, name + ".npz"))
    return z["pred"], json.loads(str(z["kwargs"])), z["fg"], z["instances"]


def random_cases(n=200, seed=7):
    """(mask, compsize, max_distance): seeded masks of 3 .. 13 voxels per axis, sparse to dense"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        shape = tuple(int(v) for v in rng.integers(3, 14, 3))
        mask = rng.random(shape) < rng.choice([0.03, 0.08, 0.15, 0.3])
        out.append((mask, int(rng.integers(0, 12)), float(rng.choice([0, 1, 1.5, 2, 2.5, 3, 4.2, 7.3, -1]))))
    return out


def lattice():
    """84 x 84 x 80 with every second voxel per axis set: 42 * 42 * 40 = 70560 isolated voxels"""
    m = np.zeros((84, 84, 80), dtype=bool)
    m[::2, ::2, ::2] = True
    return m


def brute_force(mask, compsize, max_distance):
    """The definition, restated without scipy: 26-connected components by flood fill, numbered by their
    smallest raster index; all-pairs integer squared distances.  Returns (fg, instances, stats)."""
    T = 0
    if max_distance > 0:
        while np.sqrt(np.float64(T)) < np.float64(max_distance):
            T += 1
    shape = mask.shape
    lab = np.zeros(shape, dtype=np.int64)
    comps = []
    for start in map(tuple, np.argwhere(mask)):          # (raster order: a new component's first voxel is its smallest)
        if lab[start]:
            continue
        comps.append([start])
        lab[start] = len(comps)
        todo = [start]
        while todo:
            z, y, x = todo.pop()
            for dz in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        w = (z + dz, y + dy, x + dx)
                        if all(0 <= w[a] < shape[a] for a in range(3)) and mask[w] and not lab[w]:
                            lab[w] = len(comps)
                            comps[-1].append(w)
                            todo.append(w)
    big = [np.array(c, dtype=np.int64) for c in comps if len(c) > compsize]
    big_vox = np.concatenate(big) if big else np.zeros((0, 3), dtype=np.int64)
    fg = np.zeros(shape, dtype=np.uint8)
    inst = np.zeros(shape, dtype=np.uint32)
    n_small = n_removed = n_kept = 0
    for c in comps:
        vox = np.array(c, dtype=np.int64)
        keep = True
        if len(c) <= compsize:
            n_small += 1
            keep = T > 0 and len(big_vox) > 0 and int(((vox[:, None] - big_vox[None]) ** 2).sum(-1).min()) < T
        if keep:
            n_kept += 1
            fg[tuple(vox.T)] = 1
            inst[tuple(vox.T)] = n_kept
        else:
            n_removed += 1
    return fg, inst, (len(comps), n_small, n_removed, n_kept)


# ---------------------------------------------------------------------------------------------
# the integer bound
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0, -1, -2.5, 1e-9, 1, 1.5, 2, 2.5, 3, np.sqrt(5.0), 7.3, 100])
def test_min_sq_distance_is_the_smallest_integer_whose_root_reaches_the_distance(m):
    T = postprocess.min_sq_distance(m)
    assert isinstance(T, int) and T >= 0
    if m <= 0:
        assert T == 0
        return
    assert np.sqrt(np.float64(T)) >= np.float64(m)
    assert T == 0 or np.sqrt(np.float64(T - 1)) < np.float64(m)


def test_min_sq_distance_values():
    got = [postprocess.min_sq_distance(m) for m in (1e-9, 1, 1.5, 2, 2.5, 3, np.sqrt(5.0), 7.3, 100)]
    assert got == [1, 1, 3, 4, 7, 9, 5, 54, 10000]


# ---------------------------------------------------------------------------------------------
# fg_filter
# ---------------------------------------------------------------------------------------------
def test_the_goldens_are_there():
    assert len(GOLDENS) >= 6


@pytest.mark.parametrize("name", GOLDENS)
def test_fg_filter_equals_the_reference(name):
    pred, kw, want_fg, want_inst = golden(name)
    mask = pred > kw["fg_threshold"]
    fg, inst, stats = postprocess.fg_filter(mask, kw["remove_small_comps"], kw["max_distance_to_fg"], kw["cc_instances"])
    assert fg.dtype == np.uint8 and np.array_equal(fg, want_fg)
    assert 0 < fg.sum() < mask.sum() and stats[2] > 0 and stats[3] == stats[0] - stats[2]
    if kw["cc_instances"]:
        assert inst.dtype == np.uint32 and np.array_equal(inst.astype(np.uint16), want_inst)
        assert int(inst.max()) == stats[3]
    else:
        assert inst is None


def test_fg_filter_equals_the_brute_force_definition():
    seen = set()
    for mask, compsize, dist in random_cases():
        want = brute_force(mask, compsize, dist)
        fg, inst, stats = postprocess.fg_filter(mask, compsize, dist, True)
        assert np.array_equal(fg, want[0]) and np.array_equal(inst, want[1]) and stats == want[2], (mask.shape, compsize, dist)
        seen.add((stats[2] > 0, stats[1] > stats[2]))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}   # removed some / kept some small


def test_nothing_to_remove_removes_nothing():
    """the reference raises IndexError here (it indexes with an empty float array)"""
    m = np.zeros((6, 8, 9), dtype=bool)
    m[1:4, 1:5, 1:5] = True                 # 48 voxels: big
    m[1, 1, 7] = True                       # d2 = 9 from the block: small, kept at max_distance 3.5 (T = 13)
    for dist, compsize in ((3.5, 5), (3.5, 0), (0, 0)):
        fg, inst, stats = postprocess.fg_filter(m, compsize, dist, True)
        assert np.array_equal(fg, m.astype(np.uint8)) and stats[2] == 0 and stats[3] == 2
        assert np.array_equal(np.unique(inst), [0, 1, 2]) and inst[1, 1, 7] == 2
    assert postprocess.fg_filter(m, 5, 3, False)[2] == (2, 1, 1, 1)     # T = 9: at the bound, removed


def test_no_big_component_removes_every_small_one():
    """scipy's transform of an all-ones array is an artefact; the minimum over an empty set is infinite"""
    m = np.zeros((5, 6, 7), dtype=bool)
    m[0, 0, 0] = m[2, 3, 4] = m[4, 5, 5:7] = True
    for dist in (2, 1000.0, 0):
        fg, inst, stats = postprocess.fg_filter(m, 2, dist, True)
        assert not fg.any() and not inst.any() and stats == (3, 3, 3, 0)
    fg, inst, stats = postprocess.fg_filter(np.zeros((3, 4, 5), dtype=bool), 2, 2, True)
    assert not fg.any() and not inst.any() and stats == (0, 0, 0, 0)


def test_fg_filter_wants_three_axes():
    with pytest.raises(ValueError, match="Z, Y, X"):
        postprocess.fg_filter(np.ones((4, 5), dtype=bool), 1, 1)


def test_more_than_65535_components_wrap_like_astype_uint16(tmp_path):
    m = lattice()
    fg, inst, stats = postprocess.fg_filter(m, 0, 2, True)
    assert stats == (70560, 0, 0, 70560) and np.array_equal(fg, m.astype(np.uint8))
    assert np.array_equal(inst[m], np.arange(1, 70561, dtype=np.uint32))     # raster order of the first voxels
    sample = str(tmp_path / "lattice.zarr")
    minizarr.open(sample, "w").create_dataset("volumes/pred_fgbg", data=m.astype(np.uint8), chunks=(42, 42, 80))
    postprocess.postprocess_fg([sample], str(tmp_path / "out"), fg_key="volumes/pred_fgbg", fg_threshold=0,
                               remove_small_comps=0, max_distance_to_fg=2, cc_instances=True)
    with minihdf5.File(str(tmp_path / "out" / "lattice.hdf"), "r") as f:
        got = np.asarray(f["volumes/instances"])
    assert got.dtype == np.uint16 and np.array_equal(got, inst.astype(np.uint16))
    assert got[m][65535] == 0 and got[m][65536] == 1 and got[m][65534] == 65535


# ---------------------------------------------------------------------------------------------
# the files
# ---------------------------------------------------------------------------------------------
def _write_zarr(folder, name, pred):
    fn = os.path.join(str(folder), name + ".zarr")
    minizarr.open(fn, "w").create_dataset("volumes/pred_fgbg", data=pred, chunks=pred.shape)
    return fn


def _read_hdf(fn):
    out = {}
    with minihdf5.File(fn, "r") as f:
        for key in f["volumes"].keys():
            ds = f["volumes/" + key]
            out[key] = (np.asarray(ds), ds.attrs.get("fg_filter"), ds.attrs.get("skeletonize_foreground"))
    return out


def _text(v):
    return v.decode() if isinstance(v, bytes) else v


def test_postprocess_fg_writes_the_reference_files(tmp_path):
    pred, kw, want_fg, want_inst = golden("fg_f32_d2p5")
    sample = _write_zarr(tmp_path, "sample_a", pred)
    out = tmp_path / "out"
    postprocess.postprocess_fg([sample], str(out), **dict(kw, export_skeleton_nrrds=True))
    assert sorted(os.listdir(str(out))) == ["sample_a.hdf", "sample_a.nrrd"]
    got = _read_hdf(str(out / "sample_a.hdf"))
    assert sorted(got) == ["fg", "instances"]
    fg, by, skel_by = got["fg"]
    assert fg.dtype == np.uint8 and np.array_equal(fg, want_fg)
    assert _text(by) == "scipy" and _text(skel_by) == "ppp_host_skeletonize_3d"
    assert got["instances"][0].dtype == np.uint16 and np.array_equal(got["instances"][0], want_inst)
    fields, payload = mininrrd.read(str(out / "sample_a.nrrd"))
    assert fields["sizes"] == "%d %d %d" % pred.shape[::-1]
    assert np.array_equal(payload, backend.host_skeletonize_3d(want_fg).astype(np.uint8)) and payload.any()

    # without cc_instances and the skeleton: one dataset, no .nrrd; the file is opened "w"
    postprocess.postprocess_fg([sample], str(out), **dict(kw, cc_instances=False))
    os.remove(str(out / "sample_a.nrrd"))
    postprocess.postprocess_fg([sample], str(out), **dict(kw, cc_instances=False))
    assert sorted(os.listdir(str(out))) == ["sample_a.hdf"]
    assert sorted(_read_hdf(str(out / "sample_a.hdf"))) == ["fg"]


def test_postprocess_fg_reads_hdf_samples_and_refuses_to_overwrite_them(tmp_path):
    pred, kw, want_fg, _ = golden("fg_u8_else")
    sample = str(tmp_path / "s.hdf")
    with minihdf5.File(sample, "w") as f:
        f.create_dataset("volumes/pred_fgbg", data=pred)
    with pytest.raises(ValueError, match="the sample itself"):
        postprocess.postprocess_fg([sample], str(tmp_path), **kw)
    with minihdf5.File(sample, "r") as f:
        assert np.array_equal(np.asarray(f["volumes/pred_fgbg"]), pred)
    postprocess.postprocess_fg([sample], str(tmp_path / "out"), **kw)
    assert np.array_equal(_read_hdf(str(tmp_path / "out" / "s.hdf"))["fg"][0], want_fg)


def test_postprocess_fg_wants_a_3d_dataset(tmp_path):
    sample = _write_zarr(tmp_path, "flat", np.ones((6, 7), np.float32))
    with pytest.raises(ValueError, match="3"):
        postprocess.postprocess_fg([sample], str(tmp_path / "out"), fg_key="volumes/pred_fgbg", fg_threshold=0.5,
                                   remove_small_comps=2)


CONFIG = """
[prediction]
output_format = "zarr"
fg_key = "volumes/pred_fgbg"
[postprocessing]
process_fg_prediction = true
fg_threshold = %r
remove_small_comps = %d
max_distance_to_fg = %r
cc_instances = true
"""


def test_run_ppp_postprocess_fg_task(tmp_path):
    pred, kw, want_fg, want_inst = golden("fg_f32_longx")
    folder = tmp_path / "pred"
    folder.mkdir()
    _write_zarr(folder, "sample_a", pred)
    _write_zarr(folder, "sample_b", pred[:, ::-1].copy())
    cfg = tmp_path / "config.toml"
    cfg.write_text(CONFIG % (kw["fg_threshold"], kw["remove_small_comps"], kw["max_distance_to_fg"]))
    out = tmp_path / "inst"
    argv = ["--config", str(cfg), "--do", "postprocess_fg", "--pred-folder", str(folder), "--output-folder", str(out)]
    run_ppp.main(argv + ["--sample", "sample_a"])
    assert sorted(os.listdir(str(out))) == ["sample_a.hdf"], "--sample was ignored"
    got = _read_hdf(str(out / "sample_a.hdf"))
    assert np.array_equal(got["fg"][0], want_fg) and np.array_equal(got["instances"][0], want_inst)
    run_ppp.main(argv)
    want_b = postprocess.fg_filter(pred[:, ::-1] > kw["fg_threshold"], kw["remove_small_comps"], kw["max_distance_to_fg"])[0]
    assert np.array_equal(_read_hdf(str(out / "sample_b.hdf"))["fg"][0], want_b)
    # the key stays refused under --do postprocess, and the refusal names the task that serves it
    with pytest.raises(NotImplementedError, match="process_fg_prediction.*postprocess_fg"):
        run_ppp.main(argv[:3] + ["postprocess"] + argv[4:])
