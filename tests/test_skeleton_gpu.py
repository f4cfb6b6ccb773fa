"""GPU: the 3-d thinning on the device (csrc/ppp_skeleton.hip, backend.skeletonize_3d) against the host
function that defines it (backend.host_skeletonize_3d).  An integer algorithm: every comparison is
np.array_equal on the same mask.  Then the workspace under guard bands, the properties the reference
relies on, and the driver with skeletonize_backend="ppp_device"."""
import functools

import numpy as np
import pytest
from scipy import ndimage

from test_workspace_bounds import Guarded, guard  # noqa: F401  (guard: a fixture)

pytestmark = pytest.mark.gpu

BATCH = 16          # rounds per counter read-back (kBatch in csrc/ppp_skeleton.hip)
S26 = np.ones((3, 3, 3))


@pytest.fixture(autouse=True)
def _device(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    monkeypatch.delenv("PPP_SKELETONIZE", raising=False)


# ---------------------------------------------------------------------------------------------
# inputs (made once, never changed) and the host's result for each
# ---------------------------------------------------------------------------------------------
def _bar():
    m = np.zeros((12, 14, 40), bool)
    m[3:9, 4:10, 3:37] = True                        # 6 x 6 x 34
    return m


def _slice_with_holes():
    m = np.ones((1, 70, 70), bool)
    m[0, 3::7, 3::7] = False
    return m


def _cube():
    m = np.zeros((40, 40, 40), bool)
    m[4:36, 4:36, 4:36] = True
    return m


def _balls_and_tubes(seed):
    from patchperpix_amd import synth
    shape = (24 + seed, 28, 66)
    rng = np.random.default_rng(100 + seed)
    m = synth.tube_labels(shape, n_tubes=3, radius=2, seed=seed) != 0
    zz, yy, xx = np.mgrid[:shape[0], :shape[1], :shape[2]]
    for _ in range(4):
        c = rng.uniform(0, 1, 3) * np.asarray(shape)
        r = rng.uniform(3, 7)
        m |= (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r
    m &= rng.random(shape) >= 0.01                   # salt holes
    return m


def _noise():
    return np.random.default_rng(55).random((64, 64, 64)) < 0.55


def _all_but_a_corner(shape):
    m = np.ones(shape, bool)
    m[-1, -1, -1] = False
    return m


def _six_faces():
    """a cross of three slabs through the volume plus the eight corner voxels: foreground on every face"""
    m = np.zeros((9, 11, 37), bool)
    m[3:6, :, :] = True
    m[:, 4:7, :] = True
    m[:, :, 16:21] = True
    m[::8, ::10, ::36] = True
    return m


def _tubes_case():
    from patchperpix_amd import synth
    return synth.make_case((24, 40, 72), [3, 3, 3], seed=5, kind="tubes", n_tubes=3, radius=2.5)["foreground"]


def _single_voxel():
    m = np.zeros((5, 6, 7), bool)
    m[2, 3, 4] = True
    return m


INPUTS = {
    "bar": _bar,
    "full_3x5x70": lambda: np.ones((3, 5, 70), bool),
    "slice_with_holes": _slice_with_holes,
    "cube32": _cube,
    "plate_2x34x130": lambda: np.ones((2, 34, 130), bool),
    "noise64": _noise,
    "corner_5x7x33": lambda: _all_but_a_corner((5, 7, 33)),
    "corner_4x6x31": lambda: _all_but_a_corner((4, 6, 31)),
    "line_1x1x40": lambda: np.ones((1, 1, 40), bool),
    "tiny_1x3x3": lambda: np.ones((1, 3, 3), bool),
    "empty": lambda: np.zeros((4, 5, 6), bool),
    "single_voxel": _single_voxel,
    "tubes_smallest": _tubes_case,
    "six_faces": _six_faces,
}
INPUTS.update({"balls_tubes_%d" % s: functools.partial(_balls_and_tubes, s) for s in range(6)})


@functools.lru_cache(maxsize=None)
def case(name):
    """(mask, host skeleton), both read-only"""
    from patchperpix_amd import backend
    m = INPUTS[name]()
    want = backend.host_skeletonize_3d(m)
    m.setflags(write=False)
    want.setflags(write=False)
    return m, want


def device(mask):
    """(device skeleton, (passes, sub-iterations, rounds))"""
    from patchperpix_amd import backend
    backend.NOTES.pop("skeleton_stats", None)
    got = backend.skeletonize_3d(mask)
    return got, backend.NOTES.get("skeleton_stats")


def check(name):
    from patchperpix_amd import backend
    m, want = case(name)
    got, stats = device(m)
    assert isinstance(got, np.ndarray) and got.dtype == bool and got.shape == m.shape
    assert np.array_equal(got, want), "%s: %d voxels differ" % (name, int((got != want).sum()))
    assert backend.NOTES["skeleton_kept"] == int(want.sum())
    return want, stats


# ---------------------------------------------------------------------------------------------
# the seven inputs the round scheme was prototyped on
# ---------------------------------------------------------------------------------------------
def test_bar_becomes_a_line():
    want, stats = check("bar")
    assert want.sum() == 30 and stats[1] == 6 * stats[0]


def test_runs_that_cross_a_wave_along_x():
    check("full_3x5x70")
    want, (passes, subits, rounds) = check("plate_2x34x130")
    # a flat face costs about three rounds per voxel of its side: several batches and counter reads
    assert rounds > BATCH, "the plate did not run past one batch"


def test_cube_shrinks_over_many_passes():
    want, (passes, subits, rounds) = check("cube32")
    assert want.sum() <= 4 and passes >= 16 and subits == 6 * passes     # the unchanged counter across passes


def test_single_slice_peels_four_directions():
    want, (passes, subits, rounds) = check("slice_with_holes")
    assert subits == 4 * passes and want.sum() > 500


def test_noise_puts_many_ready_candidates_into_one_word():
    want, (passes, subits, rounds) = check("noise64")
    assert want.sum() > 20000 and rounds > subits


@pytest.mark.parametrize("seed", range(6))
def test_balls_and_tubes_with_salt_holes(seed):
    want, _ = check("balls_tubes_%d" % seed)
    assert 50 < want.sum() < case("balls_tubes_%d" % seed)[0].sum() / 3


# ---------------------------------------------------------------------------------------------
# edge cases
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["corner_5x7x33", "corner_4x6x31", "line_1x1x40", "tiny_1x3x3", "empty",
                                  "single_voxel", "tubes_smallest", "six_faces"])
def test_edge_cases(name):
    want, stats = check(name)
    if name == "empty":
        assert not want.any()
    if name == "single_voxel":
        assert want.sum() == 1
    if name == "tubes_smallest":
        assert want.any()


def test_input_kinds_and_result_kinds():
    import torch
    m, want = case("balls_tubes_0")
    # uint8 with values above 1, a non-contiguous view, a 2-d mask
    assert np.array_equal(device(m.astype(np.uint8) * 7)[0], want)
    wide = np.zeros(m.shape[:2] + (2 * m.shape[2],), bool)
    wide[:, :, ::2] = m
    view = wide[:, :, ::2]
    assert not view.flags.c_contiguous and np.array_equal(device(view)[0], want)
    flat, flat_want = case("slice_with_holes")
    got2d = device(flat[0])[0]
    assert got2d.shape == flat[0].shape and got2d.dtype == bool and np.array_equal(got2d, flat_want[0])
    # a device tensor in, a device tensor out; the caller's tensor is not changed
    for dt in (torch.bool, torch.uint8):
        t = torch.from_numpy(m.copy()).cuda().to(dt)
        before = t.clone()
        got = device(t)[0]
        assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.bool and tuple(got.shape) == m.shape
        assert np.array_equal(got.cpu().numpy(), want) and torch.equal(t, before)
    with pytest.raises(AssertionError):
        device(torch.from_numpy(m.copy()))            # a host tensor is neither


def test_in_place_and_out_of_place_agree():
    import ctypes
    import torch
    from patchperpix_amd import backend
    m, want = case("balls_tubes_1")
    Z, Y, X = m.shape
    src = torch.from_numpy(m.astype(np.uint8) * 3).cuda()
    out = torch.full_like(src, 9)
    work = backend._workspace(backend.lib().ppp_skeletonize_3d_workspace_bytes(Z, Y, X), src.device)
    kept, stats = ctypes.c_int64(0), (ctypes.c_int32 * 3)()

    def run(dst):
        backend.check(backend.lib().ppp_skeletonize_3d(backend._dev_ptr(src), backend._dev_ptr(dst), Z, Y, X,
                                                       ctypes.byref(kept), stats, backend._dev_ptr(work),
                                                       backend._stream()))
        return int(kept.value), tuple(stats)
    first = run(out)
    assert np.array_equal(out.cpu().numpy(), want.astype(np.uint8)) and first[0] == want.sum()
    assert np.array_equal(src.cpu().numpy(), m.astype(np.uint8) * 3), "the mask was changed"
    assert run(src) == first                           # d_out == d_mask
    assert np.array_equal(src.cpu().numpy(), want.astype(np.uint8))


# ---------------------------------------------------------------------------------------------
# workspace
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noise64", "plate_2x34x130"])
def test_stays_inside_its_workspace(name, guard):
    m, want = case(name)
    guarded = guard()
    got, _ = device(m)
    guarded.verify("skeletonize_3d")
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------
# properties (on the DEVICE result)
# ---------------------------------------------------------------------------------------------
def test_properties_of_a_smooth_random_mask():
    rng = np.random.default_rng(0)
    m = ndimage.gaussian_filter(rng.normal(size=(24, 28, 30)), 2.0) > 0.02
    s, _ = device(m)
    assert s.any() and not (s & ~m).any()                                  # a subset of the mask
    assert ndimage.label(s, S26)[1] == ndimage.label(m, S26)[1]            # the same 26-components
    again, stats = device(s)
    assert np.array_equal(again, s) and stats[0] == 1                      # idempotent: one pass, nothing goes


# ---------------------------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------------------------
def test_to_instance_seg_with_the_device_backend(monkeypatch):
    from conftest import Golden
    from patchperpix_amd import backend
    from patchperpix_amd.vote_instances import vote_instances as vi
    g = Golden("c3d_p3_thin_mws")
    kw = dict(g.kw, debug=False, isbiHack=False, save_no_intermediates=True, sample=1.0, result_folder="/tmp",
              affinities="x.zarr", skeletonize_foreground=True)
    kw.pop("skeletonize_backend", None)
    asked = []
    real = backend.skeletonize_3d
    monkeypatch.setattr(backend, "skeletonize_3d", lambda mask: asked.append(1) or real(mask))

    def run(**extra):
        vi.SKELETONIZE_SERVED_BY = None
        inst, fg = vi.to_instance_seg(g.pred.copy(), g.foreground.copy(), g.foreground.copy(), g.numinst.copy(),
                                      g.patchshape, **dict(kw, **extra))
        return inst, fg, vi.SKELETONIZE_SERVED_BY
    inst_d, fg_d, by_d = run(skeletonize_backend="ppp_device")
    assert by_d == "ppp_skeletonize_3d" and len(asked) == 1
    inst_h, fg_h, by_h = run(skeletonize_backend="ppp")
    assert by_h == "ppp_host_skeletonize_3d" and len(asked) == 1, "'ppp' reached the device"
    assert inst_d.dtype == inst_h.dtype and np.array_equal(inst_d, inst_h) and np.array_equal(fg_d, fg_h)
    assert inst_d.any()
    monkeypatch.setenv("PPP_SKELETONIZE", "ppp_device")
    inst_e, fg_e, by_e = run()
    assert by_e == "ppp_skeletonize_3d" and len(asked) == 2
    assert np.array_equal(inst_e, inst_d) and np.array_equal(fg_e, fg_d)
