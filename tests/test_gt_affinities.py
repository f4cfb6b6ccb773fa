"""CPU: the NumPy definitions of the ground-truth patch affinities (patchperpix_amd/train_util.py) against the
goldens the reference's own `seg_to_affgraph_*_torch*` functions made (tests/golden/gt_affinities, generator
tests/golden/gen_golden_gt_affinities.py), element for element, through the reference's names and directly;
the relations between the forms (sampled == dense at loc + psH, box == slice), the wrap of negative patch
indices, offsets longer than an axis, and the ValueError / NotImplementedError cases.  No device is used."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from patchperpix_amd import backend
from patchperpix_amd import train_util as tu

GT_DIR = os.path.join(GOLDEN_DIR, "gt_affinities")
DENSE = {"d3_multi": ("seg_to_affgraph_3d_multi_torch", 3), "d3_thin": ("seg_to_affgraph_3d_multi_torch", 3),
         "d3_offsets": ("seg_to_affgraph_3d_multi_torch", 3), "d2_multi": ("seg_to_affgraph_2d_multi_torch", 2),
         "d3_single": ("seg_to_affgraph_3d_torch", 3), "d2_single": ("seg_to_affgraph_2d_torch", 2)}
SAMPLED = {"s3_multi": 3, "s2_multi": 2}


def load(name):
    return np.load(os.path.join(GT_DIR, name + ".npz"))


def test_the_golden_folder_holds_the_cases_and_stays_small():
    files = sorted(glob.glob(os.path.join(GT_DIR, "*.npz")))
    assert sorted(os.path.splitext(os.path.basename(f))[0] for f in files) == sorted(list(DENSE) + list(SAMPLED))
    assert sum(os.path.getsize(f) for f in files) < 1000000


@pytest.mark.parametrize("name", sorted(DENSE))
def test_dense_definition_equals_the_golden(name):
    g = load(name)
    fn, ndim = DENSE[name]
    want = g["aff"].astype(np.float32)
    for seg in (g["seg"], torch.from_numpy(g["seg"]), g["seg"].astype(np.int64)):
        got = getattr(tu, fn)(seg, g["nhood"], "cpu")
        assert type(got) is type(seg)
        got = got.numpy() if isinstance(got, torch.Tensor) else got
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got, want)
    # a tensor nhood, as torch_model.py:190 makes it
    got = getattr(tu, fn)(torch.from_numpy(g["seg"]), torch.from_numpy(g["nhood"]), "cpu").numpy()
    assert np.array_equal(got, want)


def test_single_form_is_the_id_squared():
    g = load("d3_single")
    centre = int(np.where((g["nhood"] == 0).all(axis=1))[0][0])
    got = tu.seg_to_affgraph_3d_torch(g["seg"], g["nhood"])
    assert np.array_equal(got[:, centre], g["seg"].astype(np.float32) ** 2) and got.max() > 1


@pytest.mark.parametrize("name", sorted(SAMPLED))
def test_sampled_definition_equals_the_golden(name):
    g = load(name)
    d = "%dd" % SAMPLED[name]
    fn = getattr(tu, "seg_to_affgraph_%s_multi_torch_code" % d)
    fnb = getattr(tu, "seg_to_affgraph_%s_multi_torch_code_batch" % d)
    ps, psH = int(g["ps"]), int(g["psH"])
    for conv in (lambda a: a, torch.from_numpy):
        got = fn(conv(g["seg"]), g["nhood"], "cpu", ps, psH, conv(g["samples"]))
        assert np.array_equal(np.asarray(got), g["aff"]) and np.asarray(got).dtype == np.float32
        assert np.array_equal(np.asarray(fn(conv(g["seg"]), g["nhood"], "cpu", ps, psH, conv(g["samples"][:1]))), g["aff_n1"])
        got = fnb(conv(g["seg"]), g["nhood"], "cpu", ps, psH, conv(g["batch_rows"]), int(g["batch_b"]))
        assert np.array_equal(np.asarray(got), g["aff_batch"])


@pytest.mark.parametrize("name", sorted(SAMPLED))
def test_sampled_equals_dense_at_loc_plus_psH(name):
    g = load(name)
    ndim = SAMPLED[name]
    d = "%dd" % ndim
    psH = int(g["psH"])
    dense = getattr(tu, "seg_to_affgraph_%s_multi_torch" % d)(g["seg"], g["nhood"] - psH)
    rows = g["samples"]
    at = rows[:, 1:] + psH
    picked = dense[(rows[:, 0], slice(None)) + tuple(at[:, a] for a in range(ndim))]
    assert np.array_equal(picked, g["aff"])


def test_box_equals_the_slice_of_the_full_result():
    g = load("d3_multi")
    full = tu.seg_to_affgraph_3d_multi_torch(g["seg"], g["nhood"])
    for box in ((1, 5, 3, 8, 5, 20), (0, 6, 0, 9, 0, 21), (5, 6, 8, 9, 20, 21)):
        got = tu.seg_to_affgraph_3d_multi_torch(g["seg"], g["nhood"], box=box)
        assert np.array_equal(got, full[:, :, box[0]:box[1], box[2]:box[3], box[4]:box[5]])
    g = load("d2_multi")
    full = tu.seg_to_affgraph_2d_multi_torch(g["seg"], g["nhood"])
    got = tu.seg_to_affgraph_2d_multi_torch(g["seg"], g["nhood"], box=(3, 8, 1, 22))
    assert np.array_equal(got, full[:, :, 3:8, 1:22])
    g = load("d3_single")
    full = tu.seg_to_affgraph_3d_torch(g["seg"], g["nhood"])
    assert np.array_equal(tu.seg_to_affgraph_3d_torch(g["seg"], g["nhood"], box=(1, 3, 0, 5, 2, 7)), full[:, :, 1:3, :, 2:7])
    for bad in ((0, 7, 0, 9, 0, 21), (2, 2, 0, 9, 0, 21), (-1, 3, 0, 9, 0, 21), (0, 6, 0, 9)):
        with pytest.raises(ValueError):
            tu.seg_to_affgraph_3d_multi_torch(load("d3_multi")["seg"], load("d3_multi")["nhood"], box=bad)


def test_negative_patch_indices_wrap_in_the_sampled_forms():
    g = load("s3_multi")
    ps, psH = int(g["ps"]), int(g["psH"])
    nhood = g["nhood"].copy()
    nhood[nhood > psH] -= ps                     # 3, 4 -> -2, -1: torch indexes from the end
    assert (nhood < 0).any()
    got = tu.seg_to_affgraph_3d_multi_torch_code(g["seg"], nhood, "cpu", ps, psH, g["samples"])
    assert np.array_equal(got, g["aff"])


def test_offsets_longer_than_an_axis_give_zeros():
    g = load("d3_offsets")
    nhood = np.array([[7, 0, 0], [0, -10, 0], [0, 0, 22], [0, 0, -500], [2 ** 31 - 1, 0, 0], [0, 0, -2 ** 31], [0, 1, 0]])
    got = tu.seg_to_affgraph_3d_multi_torch(g["seg"], nhood)
    assert not got[:, :6].any() and got[:, 6].any()
    g = load("d3_single")
    got = tu.seg_to_affgraph_3d_torch(g["seg"], np.array([[4, 0, 0], [0, 0, -8], [0, 0, 0]]))
    assert not got[:, :2].any() and got[:, 2].any()


def test_check_raises_value_errors():
    g = load("s3_multi")
    ps, psH = int(g["ps"]), int(g["psH"])
    seg, nhood = g["seg"], g["nhood"]
    B, _, Z, Y, X = seg.shape
    for row in ([0, Z - ps + 1, 0, 0], [0, 0, 0, X - ps + 1], [0, 0, -1, 0], [B, 0, 0, 0], [-1, 0, 0, 0]):
        with pytest.raises(ValueError, match="leaves the volume"):
            tu.seg_to_affgraph_3d_multi_torch_code(seg, nhood, "cpu", ps, psH, np.array([row]))
        # check=False: the C entry point's rule, voxels outside the volume read as 0 -- no exception
        out = tu.seg_to_affgraph_3d_multi_torch_code(seg, nhood, "cpu", ps, psH, np.array([row]), check=False)
        assert out.shape == (1, len(nhood))
    with pytest.raises(ValueError, match="leaves the volume"):
        tu.seg_to_affgraph_3d_multi_torch_code_batch(seg, nhood, "cpu", ps, psH, np.array([[0, 0, 0]]), B)
    big = seg.astype(np.int64)
    big[0, 0, 0, 0, 0] = 2 ** 31
    with pytest.raises(ValueError, match="fit int32"):
        tu.seg_to_affgraph_3d_multi_torch(big, nhood - psH)
    with pytest.raises(ValueError, match="fit int32"):
        tu.seg_to_affgraph_3d_multi_torch_code(torch.from_numpy(big), nhood, "cpu", ps, psH, g["samples"])
    one = load("d3_single")
    ok = one["seg"].copy()
    ok[0, 0, 0, 0] = -tu.MAX_SINGLE_ID
    ok[0, 0, 0, 1] = tu.MAX_SINGLE_ID
    got = tu.seg_to_affgraph_3d_torch(ok, one["nhood"])
    assert got[0, 13, 0, 0, 0] == got[0, 13, 0, 0, 1] == np.float32(tu.MAX_SINGLE_ID ** 2)
    for v in (tu.MAX_SINGLE_ID + 1, -tu.MAX_SINGLE_ID - 1):
        bad = one["seg"].copy()
        bad[1, 2, 3, 4] = v
        with pytest.raises(ValueError, match="46340"):
            tu.seg_to_affgraph_3d_torch(bad, one["nhood"])
    with pytest.raises(ValueError):
        tu.seg_to_affgraph_3d_multi_torch(seg.astype(np.float32), nhood)


def test_bool_and_small_integer_labels_are_accepted():
    g = load("d2_multi")
    fg = g["seg"] != 0
    want = tu.seg_to_affgraph_2d_multi_torch(fg.astype(np.int32), g["nhood"])
    for seg in (fg, fg.astype(np.uint8), torch.from_numpy(fg), fg.astype(np.int16)):
        assert np.array_equal(np.asarray(tu.seg_to_affgraph_2d_multi_torch(seg, g["nhood"])), want)


def test_one_channel_sampled_forms_are_not_implemented():
    g = load("s3_multi")
    with pytest.raises(NotImplementedError, match="cannot run"):
        tu.seg_to_affgraph_3d_torch_code(g["seg"][:, 0], g["nhood"], "cpu", 5, 2, g["samples"])
    with pytest.raises(NotImplementedError, match="cannot run"):
        tu.seg_to_affgraph_2d_torch_code(g["seg"][:, 0, 0], g["nhood"][:, 1:], "cpu", 5, 2, g["samples"][:, :3])


def test_no_samples_give_an_empty_result():
    g = load("s3_multi")
    for loc in (np.zeros((0, 4), dtype=np.int64), torch.zeros((0, 4), dtype=torch.int64), []):
        got = tu.seg_to_affgraph_3d_multi_torch_code(g["seg"], g["nhood"], "cpu", 5, 2, loc)
        assert tuple(got.shape) == (0, 125) and got.dtype == np.float32
    got = tu.seg_to_affgraph_2d_multi_torch_code_batch(torch.from_numpy(load("s2_multi")["seg"]), load("s2_multi")["nhood"],
                                                       "cpu", 7, 3, torch.zeros((0, 2), dtype=torch.int64), 1)
    assert tuple(got.shape) == (0, 49) and got.dtype == torch.float32


def test_out_dtype_on_the_host_path():
    g = load("d2_multi")
    want = g["aff"]
    got = tu.seg_to_affgraph_2d_multi_torch(torch.from_numpy(g["seg"]), g["nhood"], out_dtype=torch.bfloat16)
    assert got.dtype == torch.bfloat16 and np.array_equal(got.float().numpy(), want)
    got = tu.seg_to_affgraph_2d_multi_torch(g["seg"], g["nhood"], out_dtype=np.float16)
    assert got.dtype == np.float16 and np.array_equal(got, want)


def test_entry_points_check_their_arguments_before_any_device():
    """argument checks come before the device is asked for: the documented codes without a GPU too"""
    L = backend.lib()
    i3 = lambda *v: (ctypes.c_int32 * 3)(*v)
    i6 = lambda *v: (ctypes.c_int32 * 6)(*v)
    buf = np.zeros(64, dtype=np.int32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    halo, box, vol = i6(-1, 1, -1, 1, -1, 1), i6(0, 4, 0, 5, 0, 6), i3(4, 5, 6)
    dense = lambda **k: L.ppp_gt_affs_dense(p, k.get("B", 1), k.get("L", 1), k.get("vol", vol), p, k.get("E", 27),
                                            k.get("halo", halo), k.get("box", box), k.get("out", p), k.get("dt", 0),
                                            k.get("single", 0), None)
    INVALID, UNSUPPORTED = -1, -4
    # (every call below ends at a check: none may reach a launch, the pointers are host memory)
    assert dense(E=0) == INVALID and dense(E=65536) == UNSUPPORTED
    assert dense(vol=i3(2048, 1024, 1024), box=i6(0, 1, 0, 1, 0, 1)) == UNSUPPORTED
    assert dense(box=i6(0, 0, 0, 5, 0, 6)) == INVALID and dense(box=i6(0, 5, 0, 5, 0, 6)) == INVALID
    assert dense(box=i6(-1, 4, 0, 5, 0, 6)) == INVALID
    assert dense(B=0) == INVALID and dense(L=0) == INVALID and dense(dt=3) == INVALID
    assert dense(single=1, dt=1) == INVALID and dense(single=1, L=2) == INVALID
    assert dense(halo=i6(1, -1, 0, 0, 0, 0)) == INVALID and dense(out=None) == INVALID
    samples = lambda **k: L.ppp_gt_affs_samples(p, 1, 1, vol, p, k.get("N", 3), p, k.get("E", 27), k.get("ps", i3(3, 3, 3)),
                                                k.get("ctr", i3(1, 1, 1)), p, 0, None)
    assert samples(N=0) == 0, "N = 0 is a no-op that succeeds, device or not"
    assert samples(N=-1) == INVALID and samples(E=0) == INVALID and samples(E=65536) == UNSUPPORTED
    assert samples(ctr=i3(1, 3, 1)) == INVALID and samples(ps=i3(0, 3, 3)) == INVALID
    plan = (ctypes.c_int32 * 5)()
    assert L.ppp_gt_affs_dense_plan(1, 3, i3(140, 140, 140), 343, i6(-3, 3, -3, 3, -3, 3), i6(0, 140, 0, 140, 0, 140), 0, 0,
                                    plan) == 0
    assert list(plan)[:4] == [4, 8, 32, 1]
    # a halo as long as an axis does not fit the LDS tile: direct loads
    assert backend.gt_affs_dense_plan(1, 1, (6, 9, 21), 131, (-6, 6, -9, 9, -21, 21), (0, 6, 0, 9, 0, 21))[3] == 0
