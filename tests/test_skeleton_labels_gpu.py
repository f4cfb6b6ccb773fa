"""GPU: the 3-d skeleton of every instance of an id map in one device pass (csrc/ppp_skeleton.hip with labels,
backend.skeletonize_labels, postprocess.skeletonize_instances_device) against the host loop that defines it --
one whole-volume backend.host_skeletonize_3d per instance (postprocess.skeletonize_instances, crop=False).  An
integer algorithm: every comparison is np.array_equal.  A build that thins `map != 0` as one mask fails every
case with touching instances."""
import ctypes
import functools
import os

import numpy as np
import pytest

from test_workspace_bounds import Guarded, guard  # noqa: F401  (guard: a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _device(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    monkeypatch.delenv("PPP_POSTPROCESS", raising=False)


# ---------------------------------------------------------------------------------------------
# id maps (made once, never changed) and the host loop's result for each
# ---------------------------------------------------------------------------------------------
def _two_blocks(seam):
    """two full blocks that meet between unpadded x = seam and seam + 1: at 31 the padded bits 32 | 33 --
    a word boundary of the bit image --, at 40 inside a word"""
    m = np.zeros((6, 10, 70), np.uint32)
    m[:, :, :seam + 1] = 11
    m[:, :, seam + 1:] = 12
    return m


def _far_components():
    m = np.zeros((7, 12, 70), np.uint32)
    m[1:6, 1:6, 1:9] = 5
    m[2:7, 6:12, 58:70] = 5                          # the same id again, far away
    m[0:7, 3:9, 20:40] = 6
    return m


def _big_ids():
    from patchperpix_amd import synth
    cells = synth.cell_labels((7, 11, 40), cell=5)
    ids = np.array([0, 7, 70000, 2 ** 31 + 5], np.uint32)
    return ids[np.where(cells == 0, 0, 1 + cells % 3)]


def _make(name):
    from patchperpix_amd import synth
    rng = np.random.default_rng(11)
    if name == "cells":                              # every voxel labelled, seams everywhere, x > one 64-lane run
        return synth.cell_labels((9, 14, 70), cell=5).astype(np.uint32)
    if name in ("blocks_31", "blocks_40"):
        return _two_blocks(int(name[-2:]))
    if name == "noise":                              # three interleaved noise instances: heavy on rounds
        return rng.integers(0, 4, (9, 12, 70)).astype(np.uint32)
    if name in ("tubes_0", "tubes_1"):               # crossing tubes
        return synth.tube_labels((24, 28, 66), n_tubes=3, radius=2, seed=int(name[-1])).astype(np.uint32)
    if name == "slice":                              # four border directions
        return synth.cell_labels((1, 40, 70), cell=5).astype(np.uint32)
    if name == "far":
        return _far_components()
    if name == "big_ids":
        return _big_ids()
    if name == "u16":
        return synth.cell_labels((6, 9, 33), cell=4).astype(np.uint16)
    if name == "i32":
        return synth.cell_labels((6, 9, 33), cell=4, seed=3).astype(np.int32)
    if name == "empty":
        return np.zeros((3, 4, 70), np.uint32)
    if name == "voxel":
        m = np.zeros((3, 4, 70), np.uint32)
        m[1, 2, 64] = 9
        return m
    if name == "row":
        m = np.full((1, 1, 40), 3, np.uint32)
        m[0, 0, 17:] = 4
        return m
    raise KeyError(name)


NAMES = ["cells", "blocks_31", "blocks_40", "noise", "tubes_0", "tubes_1", "slice", "far", "big_ids", "u16", "i32",
         "empty", "voxel", "row"]


@functools.lru_cache(maxsize=None)
def case(name):
    """(id map, the host loop's skeleton map), both read-only"""
    from patchperpix_amd import postprocess
    m = _make(name)
    want = postprocess.skeletonize_instances(m, crop=False)
    m.setflags(write=False)
    want.setflags(write=False)
    return m, want


def device(ids):
    from patchperpix_amd import backend
    backend.NOTES.pop("skeleton_stats", None)
    backend.NOTES.pop("skeleton_kept", None)
    got = backend.skeletonize_labels(ids)
    return got, backend.NOTES.get("skeleton_stats"), backend.NOTES.get("skeleton_kept")


@pytest.mark.parametrize("name", NAMES)
def test_device_pass_equals_the_host_loop(name):
    m, want = case(name)
    before = m.copy()
    got, stats, kept = device(m)
    assert isinstance(got, np.ndarray) and got.dtype == m.dtype and got.shape == m.shape
    assert np.array_equal(got, want)
    assert np.array_equal(m, before)
    if m.size:
        assert kept == int(np.count_nonzero(want)) and len(stats) == 3 and stats[0] >= 1
        assert stats[1] == stats[0] * (6 if m.shape[0] > 1 else 4)


def test_touching_instances_are_not_thinned_as_one_mask():
    """what separates the pass from the binary thinning of `map != 0` (the cases above compare with the host loop
    only): on touching instances the two differ"""
    from patchperpix_amd import backend
    for name in ("cells", "blocks_31", "blocks_40", "noise", "slice"):
        m, want = case(name)
        assert not np.array_equal(want != 0, backend.host_skeletonize_3d(m != 0)), name


def test_a_2d_map_is_a_single_slice():
    m, want = case("slice")
    got, _, _ = device(m[0])
    assert got.shape == m.shape[1:] and np.array_equal(got, want[0])


def test_one_id_is_the_binary_thinning_with_the_same_counts():
    """the kernels are the binary ones: a map with one id takes the same passes, sub-iterations and rounds"""
    from patchperpix_amd import backend, synth
    mask = synth.tube_labels((24, 28, 66), n_tubes=3, radius=2, seed=0) != 0
    mask[2:20, 3:20, 30:60] = True
    backend.NOTES.pop("skeleton_stats", None)
    binary = backend.skeletonize_3d(mask)
    binary_stats, binary_kept = backend.NOTES["skeleton_stats"], backend.NOTES["skeleton_kept"]
    for ident in (1, 2 ** 31 + 9):
        got, stats, kept = device(mask.astype(np.uint32) * np.uint32(ident))
        assert np.array_equal(got, binary.astype(np.uint32) * np.uint32(ident))
        assert stats == binary_stats and kept == binary_kept


def test_in_place_and_out_of_place_agree():
    import torch
    from patchperpix_amd import backend
    m, want = case("cells")
    Z, Y, X = m.shape
    src = torch.from_numpy(m.view(np.int32).copy()).cuda()
    out = torch.full_like(src, 9)
    work = backend._workspace(backend.lib().ppp_skeletonize_labels_workspace_bytes(Z, Y, X), src.device)
    kept, stats = ctypes.c_int64(0), (ctypes.c_int32 * 3)()

    def run(dst):
        backend.check(backend.lib().ppp_skeletonize_labels(backend._dev_ptr(src), backend._dev_ptr(dst), Z, Y, X,
                                                           ctypes.byref(kept), stats, backend._dev_ptr(work),
                                                           backend._stream()))
        return int(kept.value), tuple(stats)
    first = run(out)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want) and first[0] == np.count_nonzero(want)
    assert np.array_equal(src.cpu().numpy().view(np.uint32), m), "the id map was changed"
    assert run(src) == first                           # d_out == d_labels
    assert np.array_equal(src.cpu().numpy().view(np.uint32), want)


@pytest.mark.parametrize("name", ["big_ids", "u16", "i32"])
def test_device_tensor_in_device_tensor_out(name):
    import torch
    from patchperpix_amd import postprocess
    m, want = case(name)
    t = torch.from_numpy(m.copy()).cuda()
    got = postprocess.skeletonize_instances_device(t)
    assert torch.is_tensor(got) and got.is_cuda and got.dtype == t.dtype and tuple(got.shape) == m.shape
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(t.cpu().numpy(), m), "the input tensor was changed"


def test_other_integer_dtypes_go_as_uint32():
    from patchperpix_amd import postprocess
    m, want = case("cells")
    got = postprocess.skeletonize_instances_device(m.astype(np.int64))
    assert got.dtype == np.int64 and np.array_equal(got, want)
    with pytest.raises(ValueError):
        postprocess.skeletonize_instances_device(m.astype(np.int64) - 1)


def test_limits_match_the_binary_entry_point():
    from patchperpix_amd import backend
    q, qb = backend.lib().ppp_skeletonize_labels_workspace_bytes, backend.lib().ppp_skeletonize_3d_workspace_bytes
    for shape in ((65536, 1, 1), (1, 4 * 65535 + 1, 1), (2048, 1024, 1024), (0, 4, 4)):
        assert q(*shape) == qb(*shape) and q(*shape) < 0, shape
    assert q(9, 14, 70) > qb(9, 14, 70) > 0


# ---------------------------------------------------------------------------------------------
# workspace
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cells", "noise", "row"])
def test_stays_inside_its_workspace(name, guard):
    m, want = case(name)
    guarded = guard()
    got, _, _ = device(m)
    guarded.verify("skeletonize_labels")
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------
# the task
# ---------------------------------------------------------------------------------------------
def test_postprocess_instances_device_and_host_write_the_same(tmp_path, monkeypatch):
    from patchperpix_amd import backend, minihdf5, mininrrd, postprocess, synth
    inst = synth.cell_labels((8, 14, 70), cell=5).astype(np.uint16)
    inst[0, 0, 0:3] = 60001                            # removed: at most 6 voxels
    kw = dict(res_key="vote_instances", remove_small_comps=6, export_skeleton_nrrds=True, export_skeleton_labels=True)
    asked = []
    real = backend.skeletonize_labels
    monkeypatch.setattr(backend, "skeletonize_labels", lambda ids: asked.append(1) or real(ids))
    results = {}
    for mode in ("device", "host"):
        folder = tmp_path / mode
        folder.mkdir()
        fn = str(folder / "s.hdf")
        with minihdf5.File(fn, "w") as f:
            f.create_dataset("vote_instances", data=inst, compression="gzip")
        if mode == "host":
            monkeypatch.setenv("PPP_POSTPROCESS", "host")
        postprocess.postprocess_instances([fn], str(folder), **kw)
        with minihdf5.File(fn, "r") as f:
            data = {k: (np.asarray(f[k]), f[k].dtype) for k in f.keys()}
            by = f["vote_instances_rm_6_skeleton"].attrs.get("skeletonize_instances")
        nrrds = {n: mininrrd.read(str(folder / n))[1] for n in sorted(os.listdir(str(folder))) if n.endswith(".nrrd")}
        results[mode] = (data, nrrds, by)
    assert len(asked) == 1, "PPP_POSTPROCESS=host reached the device, or the device pass ran per instance"
    (d_data, d_nrrds, d_by), (h_data, h_nrrds, h_by) = results["device"], results["host"]
    assert (d_by, h_by) == ("ppp_skeletonize_labels", "ppp_host_skeletonize_3d")
    assert sorted(d_data) == sorted(h_data) == ["vote_instances", "vote_instances_rm_6", "vote_instances_rm_6_skeleton"]
    for k in d_data:
        assert d_data[k][1] == h_data[k][1] and np.array_equal(d_data[k][0], h_data[k][0]), k
    assert sorted(d_nrrds) == sorted(h_nrrds) and len(d_nrrds) == len(np.unique(d_data["vote_instances_rm_6"][0])) - 1
    for n in d_nrrds:
        assert np.array_equal(d_nrrds[n], h_nrrds[n]), n
