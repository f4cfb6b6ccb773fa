"""GPU: `postprocess_fg` from the device -- the exact squared distance transform (csrc/ppp_edt.hip) against scipy's
distance_transform_edt squared and rounded, the component filter (ppp_post_fg_filter) against its host definition
postprocess.fg_filter, both workspaces under guard bands, and the files with the device on and off.  Integers
throughout: every comparison is np.array_equal."""
import os

import numpy as np
import pytest
from scipy import ndimage

from test_postprocess_fg import GOLDENS, _read_hdf, _write_zarr, golden, lattice, random_cases
from test_workspace_bounds import Guarded, guard  # noqa: F401  (guard: a fixture)

pytestmark = pytest.mark.gpu

INF = 0xFFFFFFFF


@pytest.fixture(autouse=True)
def _device_path(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    monkeypatch.delenv("PPP_POSTPROCESS", raising=False)


def pp():
    from patchperpix_amd import postprocess
    return postprocess


# ---------------------------------------------------------------------------------------------
# ppp_post_edt_sq
# ---------------------------------------------------------------------------------------------
# x of one lane row, below / at / above one 64-lane run, and several runs
SHAPES = [(1, 1, 70), (5, 1, 63), (1, 9, 64), (3, 70, 65), (7, 9, 130)]
CAPS = [0, 1, 2, 9, 10, 1000000]


def feature_sets(shape):
    rng = np.random.default_rng(sum(shape))
    Z, Y, X = shape
    corner = np.zeros(shape, dtype=np.uint8)
    corner[0, 0, 0] = 1                          # the largest distances: an uncapped window must not be cut
    runs = np.zeros(shape, dtype=np.uint8)
    for x in (63, 64, 127, 128):                 # one voxel on either side of every 64-run boundary
        if x < X:
            runs[Z // 2, Y // 2, x] = 1
    if not runs.any():
        runs[Z // 2, Y // 2, X - 1] = 1
    last_row = np.zeros(shape, dtype=np.uint8)   # every other line, and every other plane, holds no feature
    last_row[Z - 1, Y - 1, :] = rng.random(X) < 0.3
    last_row[Z - 1, Y - 1, X // 2] = 1
    sparse = (rng.random(shape) < 0.02).astype(np.uint8)
    sparse[Z - 1, Y - 1, X - 1] = 1
    return {"corner": corner, "runs": runs, "last_row": last_row, "sparse": sparse,
            "half": (rng.random(shape) < 0.5).astype(np.uint8), "all": np.ones(shape, dtype=np.uint8)}


def edt_sq(feature, cap):
    import torch
    from patchperpix_amd import backend
    out = backend.post_edt_sq(torch.from_numpy(feature).cuda(), cap)
    assert out.dtype == torch.int32 and tuple(out.shape) == feature.shape
    return out.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edt_sq_is_scipys_transform_squared(shape):
    for name, f in feature_sets(shape).items():
        assert f.any(), name
        exact = np.rint(ndimage.distance_transform_edt(f == 0) ** 2).astype(np.uint64)
        if name == "corner":
            assert int(exact.max()) == sum((n - 1) ** 2 for n in shape)
        for cap in CAPS:
            want = exact if cap == 0 else np.minimum(exact, cap)
            got = edt_sq(f, cap)
            assert np.array_equal(got, want.astype(np.uint32)), (name, cap, int((got != want).sum()))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edt_sq_without_a_feature_is_infinite(shape):
    f = np.zeros(shape, dtype=np.uint8)
    assert np.array_equal(edt_sq(f, 0), np.full(shape, INF, dtype=np.uint32))
    for cap in CAPS[1:] + [INF]:
        assert np.array_equal(edt_sq(f, cap), np.full(shape, cap, dtype=np.uint32))


def test_edt_sq_refuses_what_does_not_fit_32_bits():
    from patchperpix_amd import backend
    L = backend.lib()
    assert L.ppp_post_edt_sq_workspace_bytes(1, 1, 65535) > 0           # 65535^2 + 2 = 2^32 - 131069
    assert L.ppp_post_edt_sq_workspace_bytes(1, 1, 65536) == -4         # PPP_ERR_UNSUPPORTED
    # 2^32 - 1 - 65535^2 = 131070 = 362^2 + 26: Z = 5 stays one below the bound, Z = 6 passes it
    assert L.ppp_post_fg_filter_workspace_bytes(6, 362, 65535) == -4
    assert L.ppp_post_fg_filter_workspace_bytes(5, 362, 65535) > 0
    assert L.ppp_post_fg_filter_workspace_bytes(2048, 1024, 1024) == -4  # 2^31 voxels
    assert L.ppp_post_edt_sq_workspace_bytes(0, 4, 4) == -1             # PPP_ERR_INVALID_ARG


# ---------------------------------------------------------------------------------------------
# ppp_post_fg_filter
# ---------------------------------------------------------------------------------------------
def both(mask, compsize, dist, want_inst=True):
    want = pp().fg_filter(mask, compsize, dist, want_inst)
    got = pp().fg_filter_device(mask, compsize, dist, want_inst)
    assert got[0].dtype == np.uint8 and got[0].shape == mask.shape and np.array_equal(got[0], want[0])
    if want_inst:
        assert got[1].dtype == np.uint32 and np.array_equal(got[1], want[1])
    else:
        assert got[1] is None and want[1] is None
    assert got[2] == want[2]
    return got


@pytest.mark.parametrize("name", GOLDENS)
def test_fg_filter_device_equals_the_reference(name):
    pred, kw, want_fg, want_inst = golden(name)
    fg, inst, stats = both(pred > kw["fg_threshold"], kw["remove_small_comps"], kw["max_distance_to_fg"], kw["cc_instances"])
    assert np.array_equal(fg, want_fg) and stats[2] > 0
    if kw["cc_instances"]:
        assert np.array_equal(inst.astype(np.uint16), want_inst)


def test_fg_filter_device_on_random_masks():
    removed = kept_small = 0
    for mask, compsize, dist in random_cases():
        if mask.any():
            stats = both(mask, compsize, dist)[2]
            removed += stats[2]
            kept_small += stats[1] - stats[2]
    assert removed > 100 and kept_small > 100


def test_fg_filter_device_numbers_70560_components_in_raster_order():
    m = lattice()
    fg, inst, stats = both(m, 0, 2)
    assert stats == (70560, 0, 0, 70560)
    assert np.array_equal(inst[m], np.arange(1, 70561, dtype=np.uint32))
    assert both(m, 1, 2)[2] == (70560, 70560, 70560, 0)          # no big component: all removed
    assert both(m, 1, 0)[2] == (70560, 70560, 70560, 0)


def straddling_mask():
    """(6, 20, 140): a rod x = 0 .. 135 in row (0, 0) is the big component; two-voxel components across the
    64-lane run boundaries 63|64 and 127|128, and one behind the rod's end, at the squared distances 4, 8, 9
    and 5, 10 and 6 from it -- the values next to T = 4, 7, 9 (max_distance_to_fg 2, 2.5, 3) that a separate
    component can have: d2 <= 3 touches the rod, 7 is no sum of three squares."""
    m = np.zeros((6, 20, 140), dtype=bool)
    m[0, 0, 0:136] = True
    for z, y in ((2, 0), (2, 2), (0, 3)):
        m[z, y, 63:65] = True
    for z, y in ((2, 1), (1, 3)):
        m[z, y, 127:129] = True
    m[1, 1, 137:139] = True
    return m


def test_fg_filter_device_at_the_bound_across_lane_runs():
    m = straddling_mask()
    labels, n = ndimage.label(m, np.ones((3, 3, 3)))
    assert n == 7
    d2 = np.rint(ndimage.distance_transform_edt(labels != 1) ** 2).astype(np.int64)
    mind2 = sorted(int(d2[labels == k].min()) for k in range(2, n + 1))
    assert mind2 == [4, 5, 6, 8, 9, 10]
    for dist, T in ((2, 4), (2.5, 7), (3, 9), (3.2, 11)):
        assert pp().min_sq_distance(dist) == T
        fg, inst, stats = both(m, 5, dist)
        assert stats == (7, 6, sum(v >= T for v in mind2), 1 + sum(v < T for v in mind2))
        for k in range(2, n + 1):
            assert bool(fg[labels == k].all()) == (int(d2[labels == k].min()) < T) and fg[labels == k].min() == fg[labels == k].max()
    both(m, 5, 0)
    both(m, 1, 2.5)              # everything is big
    both(m, 200, 2.5)            # nothing is


def test_fg_filter_device_leaves_the_host_its_cases(monkeypatch, caplog):
    import logging
    from patchperpix_amd import backend
    monkeypatch.setattr(backend, "post_fg_filter", lambda *a, **k: pytest.fail("the device was asked"))
    with caplog.at_level(logging.DEBUG, logger="patchperpix_amd.postprocess"):
        fg, inst, stats = pp().fg_filter_device(np.zeros((0, 4, 5), dtype=bool), 2, 2, True)
        assert fg.shape == (0, 4, 5) and stats == (0, 0, 0, 0)
        with pytest.raises(ValueError):
            pp().fg_filter_device(np.ones((4, 5), dtype=bool), 2, 2)
    assert "on the host" in caplog.text


# ---------------------------------------------------------------------------------------------
# workspaces
# ---------------------------------------------------------------------------------------------
def test_edt_sq_stays_inside_its_workspace(guard):
    f = (np.random.default_rng(3).random((7, 13, 70)) < 0.01).astype(np.uint8)
    f[3, 3, 3] = 1
    want = {cap: edt_sq(f, cap) for cap in (0, 10)}
    guarded = guard()
    got = {cap: edt_sq(f, cap) for cap in (0, 10)}
    guarded.verify("post_edt_sq")
    exact = np.rint(ndimage.distance_transform_edt(f == 0) ** 2).astype(np.uint32)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[0], exact)
    assert np.array_equal(got[10], want[10]) and np.array_equal(got[10], np.minimum(exact, 10))


def test_fg_filter_stays_inside_its_workspace(guard):
    mask = np.random.default_rng(8).random((7, 13, 70)) < 0.12
    want = pp().fg_filter_device(mask, 6, 2.5, True)
    guarded = guard()
    got = pp().fg_filter_device(mask, 6, 2.5, True)
    guarded.verify("post_fg_filter")
    host = pp().fg_filter(mask, 6, 2.5, True)
    assert 0 < host[2][2] < host[2][1]
    for a, b, c in zip(got[:2], want[:2], host[:2]):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert got[2] == want[2] == host[2]


# ---------------------------------------------------------------------------------------------
# the files
# ---------------------------------------------------------------------------------------------
def test_postprocess_fg_writes_the_same_files_either_way(tmp_path, monkeypatch):
    from patchperpix_amd import backend, mininrrd
    pred, kw, want_fg, want_inst = golden("fg_f32_longx")
    sample = _write_zarr(tmp_path, "sample_a", pred)
    kw = dict(kw, export_skeleton_nrrds=True)
    asked = []
    real = backend.post_fg_filter
    monkeypatch.setattr(backend, "post_fg_filter", lambda *a, **k: asked.append(1) or real(*a, **k))
    pp().postprocess_fg([sample], str(tmp_path / "device"), **kw)
    assert len(asked) == 1
    monkeypatch.setenv("PPP_POSTPROCESS", "host")
    pp().postprocess_fg([sample], str(tmp_path / "host"), **kw)
    assert len(asked) == 1, "PPP_POSTPROCESS=host reached the device"
    assert sorted(os.listdir(str(tmp_path / "device"))) == sorted(os.listdir(str(tmp_path / "host"))) == ["sample_a.hdf", "sample_a.nrrd"]
    dev, host = _read_hdf(str(tmp_path / "device" / "sample_a.hdf")), _read_hdf(str(tmp_path / "host" / "sample_a.hdf"))
    assert sorted(dev) == sorted(host) == ["fg", "instances"]
    for key in dev:
        assert dev[key][0].dtype == host[key][0].dtype and np.array_equal(dev[key][0], host[key][0]), key
    assert np.array_equal(dev["fg"][0], want_fg) and np.array_equal(dev["instances"][0], want_inst)
    by = [v.decode() if isinstance(v, bytes) else v for v in (dev["fg"][1], host["fg"][1], dev["fg"][2], host["fg"][2])]
    assert by == ["ppp_post_fg_filter", "scipy", "ppp_skeletonize_3d", "ppp_host_skeletonize_3d"]
    skel_d, skel_h = mininrrd.read(str(tmp_path / "device" / "sample_a.nrrd")), mininrrd.read(str(tmp_path / "host" / "sample_a.nrrd"))
    assert skel_d[0] == skel_h[0] and np.array_equal(skel_d[1], skel_h[1]) and skel_d[1].any()
