"""GPU: the post-steps of the label driver from the device (csrc/ppp_postprocess.hip) against the host
functions they replace -- exact, these are integer steps.  Dilation: postprocess.dilate_instances;
compaction: postprocess.remove_small_components / relabel; clean_mask: the scipy form behind
PPP_POSTPROCESS=host.  Then the three workspaces under guard bands and the two drivers with the
device on and off."""
import logging

import numpy as np
import pytest
from scipy import ndimage

from test_postprocess_rule import random_maps, staircases, stitched_map
from test_workspace_bounds import Guarded, guard  # noqa: F401  (guard: a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _device_path(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    monkeypatch.delenv("PPP_POSTPROCESS", raising=False)


def pp():
    from patchperpix_amd import postprocess
    return postprocess


def voronoi(shape, n, seed, holes=0.0, dtype=np.uint32):
    """touching instances: nearest of n seeded centres; a fraction `holes` of the voxels background"""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(0, s, n) for s in shape], axis=1)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).reshape(-1, 1, 3)
    best = np.empty(len(grid), dtype=np.int64)
    for a in range(0, len(grid), 4096):
        best[a:a + 4096] = np.argmin(((grid[a:a + 4096] - pts[None]) ** 2).sum(-1), axis=1)
    m = (best + 1).astype(dtype).reshape(shape)
    if holes:
        m[rng.random(shape) < holes] = 0
    return m


# ---------------------------------------------------------------------------------------------
# dilation
# ---------------------------------------------------------------------------------------------
def dilate_both(m):
    from patchperpix_amd import backend
    backend.NOTES.pop("post_dilate_rounds", None)
    got = pp().dilate_instances_device(m)
    want = pp().dilate_instances(m)
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want)
    return backend.NOTES.get("post_dilate_rounds")


def test_dilate_random_maps():
    for m in random_maps():
        assert dilate_both(m) >= 1


def test_dilate_staircases_run_the_later_rounds():
    for m in staircases():
        assert dilate_both(m) >= 2


def test_dilate_voronoi_with_holes():
    m = voronoi((40, 40, 40), 150, 5, holes=0.1)
    assert len(np.unique(m)) > 140
    assert dilate_both(m) >= 2


@pytest.mark.parametrize("shape", [(3, 5, 65), (2, 3, 130), (1, 70, 70)])
def test_dilate_rows_that_cross_a_wave(shape):
    dilate_both(voronoi(shape, 12, 7, holes=0.15))
    # and runs longer than a wave along x, one id per row
    m = np.zeros(shape, dtype=np.uint32)
    m[:] = (np.arange(shape[1], dtype=np.uint32)[::-1] + 1)[None, :, None]
    m[..., shape[2] // 2] = 0
    dilate_both(m)


def test_dilate_compares_ids_unsigned():
    m = np.zeros((3, 6, 9), dtype=np.uint32)
    m[:, :, 0:3] = 70001
    m[:, :, 3:6] = 2 ** 31 + 5
    m[:, :, 6:9] = 400123
    m[1, 2, 4] = 3
    dilate_both(m)
    dilate_both(m[:, :, ::-1].copy())


def test_dilate_empty_map_and_corner_voxel():
    dilate_both(np.zeros((4, 5, 6), dtype=np.uint32))
    m = np.zeros((4, 5, 6), dtype=np.uint32)
    m[0, 0, 0] = 9
    dilate_both(m)
    m[3, 4, 5] = 2
    dilate_both(m)


def test_dilate_dtypes_tensors_and_host_cases(caplog):
    import torch
    m = voronoi((6, 9, 11), 9, 3, holes=0.2)
    for dt in (np.uint16, np.int32):
        dilate_both(m.astype(dt))
    want = pp().dilate_instances(m.astype(np.int32))
    t = torch.from_numpy(m.astype(np.int32)).cuda()
    got = pp().dilate_instances_device(t)
    assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(t.cpu().numpy(), m.astype(np.int32))
    # the host function serves iterations != 1 and other dtypes, with a debug line, never an error
    with caplog.at_level(logging.DEBUG, logger="patchperpix_amd.postprocess"):
        assert np.array_equal(pp().dilate_instances_device(m, iterations=2), pp().dilate_instances(m, iterations=2))
        assert np.array_equal(pp().dilate_instances_device(m.astype(np.int64)), pp().dilate_instances(m.astype(np.int64)))
    assert sum("on the host" in r.getMessage() for r in caplog.records) == 2


# ---------------------------------------------------------------------------------------------
# compaction
# ---------------------------------------------------------------------------------------------
def compact_both(m, compsize=None, relabel=False, start=None):
    P = pp()
    want, got = m, m
    if compsize is not None:
        want, got = P.remove_small_components(want, compsize), P.remove_small_components_device(got, compsize)
        assert got.dtype == want.dtype and np.array_equal(got, want)
    if relabel:
        want, got = P.relabel(want, start), P.relabel_device(got, start)
        assert got.dtype == want.dtype and np.array_equal(got, want)
    return got


def test_compact_the_stitched_map():
    m = stitched_map()
    got = compact_both(m, compsize=2, relabel=True)
    assert set(np.unique(got)) == {0, 1, 2}
    assert np.array_equal(pp().compact(m, 2), got)              # both steps in one pass
    compact_both(m, compsize=2)                                 # removal without relabel
    compact_both(m, compsize=-1, relabel=True)                  # nothing removed
    compact_both(m, relabel=True, start=5)
    compact_both(m, compsize=16, relabel=True)                  # exactly compsize voxels: removed
    assert compact_both(m, compsize=15, relabel=True).max() == 2


def test_compact_sizes_at_the_threshold():
    m = np.zeros((3, 7, 10), dtype=np.uint32)
    flat = m.reshape(-1)
    flat[0:6] = 11          # compsize voxels: removed
    flat[20:27] = 4         # compsize + 1: kept
    flat[100:101] = 9
    flat[150:156] = 7
    flat[156:163] = 8
    got = compact_both(m, compsize=6, relabel=True)
    assert sorted(np.unique(got)) == [0, 1, 2] and got.reshape(-1)[20] == 1 and got.reshape(-1)[156] == 2


def test_compact_long_runs_and_one_wave():
    m = np.zeros((4, 40, 67), dtype=np.uint32)
    flat = m.reshape(-1)
    flat[333:1333] = 77                 # one id as a run of 1 000 voxels over several x rows
    flat[2000:2040] = 5                 # an id whose voxels all sit in one wave's span
    flat[2040:2041] = 6
    flat[5000:9000:3] = 12              # no runs at all
    flat[-2:] = 3                       # the tail of the vectors
    for cs in (1, 39, 40, 999, 1000):
        compact_both(m, compsize=cs, relabel=True)
    want = np.bincount(flat)[[77, 5, 6, 12, 3]]
    assert list(want) == [1000, 40, 1, 1334, 2]


@pytest.mark.parametrize("x", [1, 3, 67])
def test_compact_x_extents_and_misaligned_maps(x):
    import torch
    rng = np.random.default_rng(x)
    m = np.repeat(rng.integers(0, 9, (5, 6, (x + 2) // 3)), 3, axis=2)[:, :, :x].astype(np.uint32)
    for cs in (0, 2, 7):
        compact_both(m, compsize=cs, relabel=True, start=3)
    # a tensor that starts 4, 8 and 12 bytes behind a 16-byte boundary (the head of the 16-byte loads)
    from patchperpix_amd import backend
    for off in (1, 2, 3):
        buf = torch.zeros(m.size + 8, dtype=torch.int32, device="cuda")
        view = buf[off:off + m.size]
        view.copy_(torch.from_numpy(m.view(np.int32).reshape(-1)))
        kept = backend.post_compact_ids(view, int(m.max()), compsize=2, relabel=True, start=1)
        want = pp().relabel(pp().remove_small_components(m, 2))
        assert np.array_equal(view.cpu().numpy().view(np.uint32).reshape(m.shape), want)
        assert kept == len(np.unique(want)) - 1
        assert int(buf[:off].abs().sum()) == 0 and int(buf[off + m.size:].abs().sum()) == 0


def test_compact_dtypes_and_tensors():
    import torch
    m = voronoi((5, 12, 13), 30, 11, holes=0.3)
    for dt in (np.uint16, np.int32):
        compact_both(m.astype(dt), compsize=20, relabel=True)
    # uint16 wraps the way the host's assignment does
    compact_both(m.astype(np.uint16), relabel=True, start=65530)
    t = torch.from_numpy(m.astype(np.int32)).cuda()
    got = pp().relabel_device(pp().remove_small_components_device(t, 20))
    assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy(), pp().relabel(pp().remove_small_components(m.astype(np.int32), 20)))
    assert np.array_equal(t.cpu().numpy(), m.astype(np.int32)), "the caller's tensor was changed"
    for dt in (np.uint16, np.uint32):
        t = torch.from_numpy(m.astype(dt)).cuda()
        got = pp().relabel_device(t, 7)
        assert got.is_cuda and got.dtype == t.dtype and np.array_equal(got.cpu().numpy(), pp().relabel(m.astype(dt), 7))
        got = pp().dilate_instances_device(t)
        assert got.is_cuda and got.dtype == t.dtype and np.array_equal(got.cpu().numpy(), pp().dilate_instances(m.astype(dt)))


def test_compact_ids_beyond_the_table_go_to_the_host(caplog, monkeypatch):
    from patchperpix_amd import backend
    m = stitched_map()
    m[0, 0, 0:3] = 2 ** 28 + 17
    m[0, 5, 0:5] = 2 ** 31 + 2
    monkeypatch.setattr(backend, "post_compact_ids", lambda *a, **k: pytest.fail("the device was asked"))
    with caplog.at_level(logging.DEBUG, logger="patchperpix_amd.postprocess"):
        compact_both(m, compsize=3, relabel=True)
        compact_both(np.where(m > 0, -1, 0).astype(np.int32), relabel=True)      # a negative id
        compact_both(m.astype(np.int64), compsize=3)
    assert sum("on the host" in r.getMessage() for r in caplog.records) == 4


def test_compact_entry_point_refuses_an_id_above_max_id():
    import torch
    from patchperpix_amd import backend
    t = torch.tensor([0, 3, 3, 9, 9, 9, 2, 2], dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="max_id"):
        backend.post_compact_ids(t, 8)
    assert t.tolist() == [0, 3, 3, 9, 9, 9, 2, 2]


# ---------------------------------------------------------------------------------------------
# clean_mask
# ---------------------------------------------------------------------------------------------
STRUCTURES = [np.ones([3] * 3), ndimage.generate_binary_structure(3, 1), ndimage.generate_binary_structure(3, 2)]


def clean_both(mask, structure, size, caplog, monkeypatch):
    from patchperpix_amd import backend
    from patchperpix_amd.vote_instances import stitch_patch_graph as spg
    calls = []
    real = backend.post_clean_mask
    monkeypatch.setattr(backend, "post_clean_mask", lambda *a: calls.append(1) or real(*a))
    with caplog.at_level(logging.INFO, logger=spg.logger.name):
        caplog.clear()
        got = spg.clean_mask(mask, structure, size)
        line_dev = [r.getMessage() for r in caplog.records if "small components" in r.getMessage()]
        monkeypatch.setenv("PPP_POSTPROCESS", "host")
        caplog.clear()
        want = spg.clean_mask(mask, structure, size)
        line_host = [r.getMessage() for r in caplog.records if "small components" in r.getMessage()]
        monkeypatch.delenv("PPP_POSTPROCESS")
    assert len(calls) == 1, "the device path did not run exactly once"
    assert got.dtype == want.dtype == bool and got.shape == want.shape and np.array_equal(got, want)
    assert len(line_dev) == 1 and line_dev == line_host           # the logged count of removed components
    return got


def serpentine(n):
    """a one-voxel-thick path that fills an n^3 box: one component under every structure"""
    m = np.zeros((n, n, n), dtype=bool)
    m[::2, ::2, :] = True                                        # lines along x in every other row / slice
    for z in range(0, n, 2):
        for k, y in enumerate(range(0, n - 2, 2)):
            m[z, y + 1, (n - 1) if k % 2 == 0 else 0] = True    # joined end to end within the slice
    last_y = (n - 1) // 2 * 2
    end_x = (n - 1) if ((last_y // 2) % 2 == 0) else 0
    for k, z in enumerate(range(0, n - 2, 2)):
        # a slice's path runs from (0, 0) to (last_y, end_x), the next slice's the other way round
        if k % 2 == 0:
            m[z + 1, last_y, end_x] = True
        else:
            m[z + 1, 0, 0] = True
    return m


@pytest.mark.parametrize("s", range(3))
def test_clean_mask_blobs_and_structures(s, caplog, monkeypatch):
    rng = np.random.default_rng(31 + s)
    mask = rng.random((9, 14, 21)) < 0.22
    for size in (0, 1, 3, 10):
        clean_both(mask, STRUCTURES[s], size, caplog, monkeypatch)
    clean_both(ndimage.binary_dilation(mask).astype(np.uint8) * 7, STRUCTURES[s], 40, caplog, monkeypatch)


def test_clean_mask_corner_contact(caplog, monkeypatch):
    m = np.zeros((6, 6, 6), dtype=bool)
    m[0:3, 0:3, 0:3] = True
    m[3:5, 3:5, 3:5] = True                                      # touches the first blob across one corner
    joined = clean_both(m, STRUCTURES[0], 27, caplog, monkeypatch)
    assert joined.sum() == 35                                    # one component of 35 voxels at 26
    apart = clean_both(m, STRUCTURES[1], 26, caplog, monkeypatch)
    assert apart.sum() == 27                                     # 27 + 8 at 6: the small one goes
    assert clean_both(m, STRUCTURES[2], 26, caplog, monkeypatch).sum() == 27
    assert clean_both(m, STRUCTURES[1], 27, caplog, monkeypatch).sum() == 0      # exactly `size`: removed


def test_clean_mask_serpentine(caplog, monkeypatch):
    m = serpentine(17)
    n = int(m.sum())
    for st in STRUCTURES:
        assert ndimage.label(m, st)[1] == 1
        assert clean_both(m, st, n - 1, caplog, monkeypatch).sum() == n          # size + 1 voxels: kept
        assert clean_both(m, st, n, caplog, monkeypatch).sum() == 0              # size voxels: removed


def test_clean_mask_empty_full_and_flat(caplog, monkeypatch):
    clean_both(np.zeros((5, 6, 7), dtype=bool), STRUCTURES[0], 3, caplog, monkeypatch)
    assert clean_both(np.ones((5, 6, 7), dtype=bool), STRUCTURES[0], 209, caplog, monkeypatch).all()
    assert not clean_both(np.ones((5, 6, 7), dtype=bool), STRUCTURES[1], 210, caplog, monkeypatch).any()
    rng = np.random.default_rng(5)
    flat = rng.random((1, 33, 70)) < 0.4
    for st in STRUCTURES:
        clean_both(flat, st, 4, caplog, monkeypatch)
    clean_both(flat[0], np.ones((3, 3)), 4, caplog, monkeypatch)                 # a 2-d mask, as the 2-d driver passes


# ---------------------------------------------------------------------------------------------
# workspaces
# ---------------------------------------------------------------------------------------------
def test_compact_stays_inside_its_workspace(guard):
    m = voronoi((7, 13, 19), 40, 2, holes=0.2)
    want = pp().compact(m, 30)
    guarded = guard()
    got = pp().compact(m, 30)
    guarded.verify("post_compact_ids")
    assert np.array_equal(got, want) and np.array_equal(got, pp().relabel(pp().remove_small_components(m, 30)))


def test_dilate_stays_inside_its_workspace(guard):
    m = voronoi((7, 13, 19), 40, 2, holes=0.2)
    want = pp().dilate_instances_device(m)
    guarded = guard()
    got = pp().dilate_instances_device(m)
    guarded.verify("post_dilate")
    assert np.array_equal(got, want) and np.array_equal(got, pp().dilate_instances(m))


def test_clean_mask_stays_inside_its_workspace(guard):
    from patchperpix_amd.vote_instances import stitch_patch_graph as spg
    mask = np.random.default_rng(8).random((7, 13, 19)) < 0.25
    want = spg.clean_mask(mask, np.ones([3] * 3), 3)
    guarded = guard()
    got = spg.clean_mask(mask, np.ones([3] * 3), 3)
    guarded.verify("post_clean_mask")
    labeled, n = ndimage.label(mask, np.ones([3] * 3))
    assert np.array_equal(got, want) and np.array_equal(got, (np.bincount(labeled.ravel()) > 3)[labeled] & mask)


# ---------------------------------------------------------------------------------------------
# drivers
# ---------------------------------------------------------------------------------------------
FIVE = ["vote_instances", "vote_foreground", "vote_instances_masked", "vote_instances_dil_1",
        "vote_instances_masked_dil_1"]


def _both_ways(run, monkeypatch):
    """run() with the device post-steps and with PPP_POSTPROCESS=host: the same five datasets"""
    from patchperpix_amd import backend
    from patchperpix_amd.vote_instances import vote_instances as vi
    asked = []
    for name in ("post_compact_ids", "post_dilate", "post_clean_mask"):
        real = getattr(backend, name)
        monkeypatch.setattr(backend, name, lambda *a, _r=real, _n=name, **k: asked.append(_n) or _r(*a, **k))
    results = []
    for mode in (None, "host"):
        if mode:
            monkeypatch.setenv("PPP_POSTPROCESS", mode)
        written = {}
        monkeypatch.setattr(vi, "write_result", lambda fn, ds, _w=written: _w.update(ds))
        n_before = len(asked)
        inst = run(mode or "device")
        results.append((inst, written))
        if mode:
            assert len(asked) == n_before, "PPP_POSTPROCESS=host reached the device"
    assert set(asked) == {"post_compact_ids", "post_dilate", "post_clean_mask"}
    (inst_d, dev), (inst_h, host) = results
    assert sorted(dev) == sorted(FIVE) and sorted(host) == sorted(FIVE)
    assert inst_d.dtype == inst_h.dtype and np.array_equal(inst_d, inst_h)
    for key in FIVE:
        assert dev[key].dtype == host[key].dtype == np.uint16 and np.array_equal(dev[key], host[key]), key
    assert len(np.unique(dev["vote_instances"])) >= 3
    assert np.count_nonzero(dev["vote_instances_dil_1"]) > np.count_nonzero(dev["vote_instances"])
    return dev


def test_stitch_main_writes_the_same_datasets_either_way(tmp_path, monkeypatch):
    from patchperpix_amd import synth, tiling
    from tests_flags import FLYLIGHT
    c = synth.make_case((12, 24, 24), (3, 3, 3), seed=5, cell=[6, 10, 10])
    pred = c["pred"].copy()
    pred[:, 11, 1, 1] = 0.0
    pred[13, 11, 1, 1] = 0.9                    # a one-voxel foreground component for clean_mask to drop
    np.save(tmp_path / "p.npy", pred)
    kw = dict(FLYLIGHT, overlapping_inst=False, patchshape=[3, 3, 3], ignore_small_comps=2, remove_small_comps=3,
              dilate_instances=True, only_bb=True)
    kw.pop("result_folder")

    def run(mode):
        return tiling.stitch_main(str(tmp_path / "p.npy"), result_folder=str(tmp_path / mode), **kw)
    _both_ways(run, monkeypatch)


def test_blockwise_reference_writes_the_same_datasets_either_way(tmp_path, monkeypatch):
    import json
    import os
    from conftest import GOLDEN_DIR
    from patchperpix_amd import minizarr
    from patchperpix_amd.vote_instances import stitch_patch_graph as spg
    z = np.load(os.path.join(GOLDEN_DIR, "bw_p3_cc_overlap.npz"))
    kw = json.loads(str(z["flags"]))
    kw.setdefault("max_total_patch_distance_in_ps_multiples", 2)
    kw.update(ignore_small_comps=2, remove_small_comps=3, dilate_instances=True, only_bb=True)
    pred_file = str(tmp_path / "sample.zarr")
    pred16 = z["pred_f16"]
    minizarr.open(pred_file, "w").create_dataset("volumes/pred_affs", data=pred16, chunks=(pred16.shape[0], 8, 8, 8))

    def run(mode):
        return spg.main(pred_file, result_folder=str(tmp_path / mode), blockwise_semantics="reference", **kw)
    _both_ways(run, monkeypatch)
