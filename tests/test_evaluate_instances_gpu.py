"""GPU: the contingency table of two label stacks from the device (csrc/ppp_overlap.hip, backend.label_overlap)
against its NumPy definition evaluate_instances.overlap_counts_host, and the `evaluate` step's files with the
device on and off.  Integers throughout: every comparison is np.array_equal, there is no tolerance anywhere."""
import ctypes
import functools
import os

import numpy as np
import pytest

from test_workspace_bounds import Guarded, guard  # noqa: F401  (guard: a fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 63), (1, 1, 64), (1, 1, 65), (3, 5, 67), (2, 7, 130), (5, 9, 257)]
CHANNELS = [(1, 1), (3, 2), (2, 3)]


@pytest.fixture(autouse=True)
def _device(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    monkeypatch.delenv("PPP_POSTPROCESS", raising=False)


def ei():
    from patchperpix_amd import evaluate_instances
    return evaluate_instances


def device_table(a, b):
    """backend.label_overlap on NumPy stacks (L, Z, Y, X)"""
    import torch
    from patchperpix_amd import backend
    ta = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()
    tb = torch.from_numpy(np.ascontiguousarray(b, dtype=np.uint32).view(np.int32)).cuda()
    return backend.label_overlap(ta, tb)


def same(got, want):
    assert got[0].dtype == np.uint32 and got[1].dtype == np.int64 and got[0].shape == (len(got[1]), 2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def runs_stack(rng, L, shape, n_ids, mean_run):
    """L channels of piecewise-constant ids along the flat volume: runs of geometric length over n_ids ids and
    background, so that channels overlap and runs cross row ends"""
    V = int(np.prod(shape))
    out = np.zeros((L, V), np.uint32)
    for c in range(L):
        v = 0
        while v < V:
            n = int(rng.geometric(1.0 / mean_run))
            out[c, v:v + n] = rng.integers(0, n_ids + 1)
            v += n
    return out.reshape((L,) + tuple(shape))


# ---------------------------------------------------------------------------------------------
# shapes around the lane vector and the 64-lane run, rows that start off 16 bytes, several channels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", CHANNELS, ids=lambda c: "%dx%d" % c)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_overlap_matches_host_definition(shape, channels):
    rng = np.random.default_rng(sum(shape) * 7 + channels[0])
    for mean_run in (1.5, 9.0, 300.0):
        a = runs_stack(rng, channels[0], shape, 5, mean_run)
        b = runs_stack(rng, channels[1], shape, 4, mean_run)
        same(device_table(a, b), ei().overlap_counts_host(a, b))


# ---------------------------------------------------------------------------------------------
# runs
# ---------------------------------------------------------------------------------------------
def _run_cases():
    shape = (3, 6, 70)
    V = int(np.prod(shape))
    lin = np.arange(V).reshape(shape)
    one = np.full(shape, 9, np.uint32)
    alternating = (1 + lin % 2).astype(np.uint32)                    # no run longer than 1
    rows = np.zeros(shape, np.uint32)                                # id k ends row y and starts row y + 1
    flat = rows.reshape(-1)
    for k, start in enumerate(range(35, V - 70, 70)):
        flat[start:start + 70] = k + 1
    changing = (1 + (lin // 3) % 5).astype(np.uint32)
    return {"one_id": (one, one), "alternating": (alternating, alternating[..., ::-1].copy()),
            "across_rows": (rows, one), "one_side_changes": (one, changing), "other_side_changes": (changing, one),
            "alternating_vs_one": (alternating, one)}


@pytest.mark.parametrize("name", sorted(_run_cases()))
def test_overlap_runs(name):
    a, b = _run_cases()[name]
    same(device_table(a[None], b[None]), ei().overlap_counts_host(a[None], b[None]))


# ---------------------------------------------------------------------------------------------
# table pressure: every voxel its own pair
# ---------------------------------------------------------------------------------------------
def table_entries():
    from patchperpix_amd import backend
    return int(backend.lib().ppp_label_overlap_table_entries())


@pytest.mark.parametrize("factor", [1, 2])
def test_overlap_every_voxel_its_own_pair(factor):
    entries = table_entries()
    assert entries == 2048              # the LDS table of csrc/ppp_overlap.hip: 2048 slots per workgroup
    V = factor * entries + 37           # just above the capacity of one table, and of two
    ids = (np.arange(V, dtype=np.uint32) + 1).reshape(1, 1, 1, V)
    rows, counts = device_table(ids, ids)
    same((rows, counts), ei().overlap_counts_host(ids, ids))
    assert len(counts) == 3 * V and (counts == 1).all()
    from patchperpix_amd import backend
    partials, flushes, spilled = backend.label_overlap_last_stats()
    assert partials == 3 * V and spilled > 0 and flushes == 0      # one step per workgroup: past the table, no look


@functools.lru_cache(maxsize=None)
def flush_case():
    """2.2 M voxels, the smallest size class at which a workgroup has a second step (more than 2048 steps of 1024
    voxels), ids changing every second voxel: 1536 new keys per step, so the look after the first step finds the
    table past half full and flushes it inside the loop"""
    V = 2200 * 1000
    lin = np.arange(V, dtype=np.uint32)
    a = (lin // 2 + 1).reshape(1, 10, 220, 1000)
    b = ((lin + 1) // 2 + 5).reshape(1, 10, 220, 1000)
    return a, b, ei().overlap_counts_host(a, b)


def test_overlap_flushes_the_table_inside_the_loop():
    from patchperpix_amd import backend
    a, b, want = flush_case()
    got = device_table(a, b)
    partials, flushes, spilled = backend.label_overlap_last_stats()
    same(got, want)
    # 2149 steps in 1075 workgroups of two: every workgroup with a second step flushed after its first
    assert flushes >= 1074 and partials > len(want[1])
    again = device_table(a, b)
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()


def test_overlap_every_voxel_its_own_pair_with_channels():
    V = table_entries() + 5
    lin = np.arange(V, dtype=np.uint32)
    a = np.stack([lin + 1, lin + 1 + V]).reshape(2, 1, 1, V)
    b = np.stack([lin + 7, 3 * lin + 1, lin[::-1] + 1]).reshape(3, 1, 1, V)
    same(device_table(a, b), ei().overlap_counts_host(a, b))


# ---------------------------------------------------------------------------------------------
# ids
# ---------------------------------------------------------------------------------------------
def test_overlap_big_ids():
    ids = np.array([0, 1, 2 ** 31, 2 ** 31 + 1, 0xFFFFFFFF, 0xFFFFFFFE], np.uint32)
    rng = np.random.default_rng(5)
    a = ids[rng.integers(0, len(ids), (2, 3, 5, 67))]
    b = ids[rng.integers(0, len(ids), (2, 3, 5, 67))]
    got = device_table(a, b)
    same(got, ei().overlap_counts_host(a, b))
    assert [0xFFFFFFFF, 0xFFFFFFFF] in got[0].tolist() and [2 ** 31, 0] in got[0].tolist()


def colliding_keys(n):
    """n keys (a, b) with the home slot of (1, 1) under overlap_slot of csrc/ppp_overlap.hip, read through
    ppp_label_overlap_slot"""
    from patchperpix_amd import backend
    slot = backend.lib().ppp_label_overlap_slot
    home, keys, a = slot(1, 1), [], 1
    while len(keys) < n:
        b = 1 + len(keys) % 3
        if slot(a, b) == home:
            keys.append((a, b))
        a += 1
    # the Python restatement of the hash agrees with the library's
    entries = table_entries()
    for ka, kb in keys:
        assert ((ka * 0x9E3779B1 + kb * 0x85EBCA77) & 0xFFFFFFFF) >> (32 - entries.bit_length() + 1) == home
    return keys


def test_overlap_keys_that_collide_in_the_table():
    keys = colliding_keys(100)          # more than the 64 slots a probe walks: some keys go to the list directly
    rng = np.random.default_rng(2)
    pick = rng.integers(0, len(keys), 900)
    a = np.repeat(np.array([keys[k][0] for k in pick], np.uint32), 3).reshape(1, 3, 9, 100)
    b = np.repeat(np.array([keys[k][1] for k in pick], np.uint32), 3).reshape(1, 3, 9, 100)
    same(device_table(a, b), ei().overlap_counts_host(a, b))


# ---------------------------------------------------------------------------------------------
# the cap protocol, outputs and workspace under guard bands
# ---------------------------------------------------------------------------------------------
FILL = 0xA5


def test_overlap_cap_protocol(guard):
    import torch
    from patchperpix_amd import backend
    rng = np.random.default_rng(9)
    a = runs_stack(rng, 2, (3, 5, 67), 5, 4.0)
    b = runs_stack(rng, 2, (3, 5, 67), 4, 4.0)
    want = ei().overlap_counts_host(a, b)
    n = len(want[1])
    ta = torch.from_numpy(a.view(np.int32)).cuda()
    tb = torch.from_numpy(b.view(np.int32)).cuda()
    g = guard()
    assert backend.label_overlap_raw(ta, tb, 0) == n                     # the size query: NULL outputs
    for cap in (n - 1, n):
        rows = g(cap * 8, ta.device)
        counts = g(cap * 8, ta.device)
        got = backend.label_overlap_raw(ta, tb, cap, rows.view(torch.int32).reshape(cap, 2), counts.view(torch.int64))
        assert got == n
        torch.cuda.synchronize()
        if cap < n:                                                      # nothing is written
            assert bool((rows == FILL).all()) and bool((counts == FILL).all())
        else:
            same((rows.cpu().numpy().view(np.uint32).reshape(n, 2), counts.cpu().numpy().view(np.int64)), want)
    g.verify("label_overlap_raw", "test_overlap_cap_protocol")


def test_overlap_argument_errors():
    import torch
    from patchperpix_amd import backend
    L = backend.lib()
    t = torch.zeros((1, 2, 3, 4), dtype=torch.int32, device="cuda")
    work = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    n = ctypes.c_int64(-7)
    p, w = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(work.data_ptr())

    def call(La=1, Lb=1, Z=2, Y=3, X=4, a=p, b=p, cap=0, n_rows=ctypes.byref(n), d_work=w):
        return L.ppp_label_overlap(a, La, b, Lb, Z, Y, X, None, None, cap, n_rows, d_work, None)
    assert call() == 0 and n.value == 0                                  # all background: no rows
    assert call(La=0) == -1 and call(Lb=0) == -1 and call(La=-3) == -1   # PPP_ERR_INVALID_ARG
    assert b"channel" in L.ppp_last_error()
    assert call(Z=0) == -1 and call(cap=-1) == -1 and call(cap=5) == -1  # (cap > 0 with NULL outputs)
    assert call(a=None) == -1 and call(d_work=None) == -1 and call(n_rows=None) == -1
    assert call(a=ctypes.c_void_p(t.data_ptr() + 2)) == -1               # misaligned
    assert call(Z=2048, Y=1024, X=1024) == -4                            # PPP_ERR_UNSUPPORTED: 2^31 voxels
    assert L.ppp_label_overlap_workspace_bytes(1, 1, 2048, 1024, 1024) == -4
    assert L.ppp_label_overlap_workspace_bytes(1, 1, 2047, 1024, 1024) > 0
    assert L.ppp_label_overlap_workspace_bytes(0, 1, 4, 4, 4) == -1
    assert L.ppp_label_overlap_workspace_bytes(300, 300, 4, 4, 4) == -4 and call(La=300, Lb=300) == -4
    assert L.ppp_label_overlap_workspace_bytes(1, 1, 2, 3, 4) <= 1 << 20  # (the calls above had room)


def test_overlap_is_deterministic():
    rng = np.random.default_rng(21)
    a = runs_stack(rng, 2, (5, 9, 257), 40, 2.0)
    b = runs_stack(rng, 2, (5, 9, 257), 40, 2.0)
    first = device_table(a, b)
    second = device_table(a, b)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    same(first, ei().overlap_counts_host(a, b))


def test_overlap_in_chunks_when_the_workspace_is_bounded(monkeypatch):
    """backend.label_overlap cuts the volume where the worst-case workspace exceeds its budget: the same rows"""
    import torch
    from patchperpix_amd import backend
    rng = np.random.default_rng(13)
    a, b = runs_stack(rng, 2, (3, 5, 67), 6, 3.0), runs_stack(rng, 1, (3, 5, 67), 6, 3.0)
    ta, tb = torch.from_numpy(a.view(np.int32)).cuda(), torch.from_numpy(b.view(np.int32)).cuda()
    calls = []
    real = backend.label_overlap_raw
    monkeypatch.setattr(backend, "label_overlap_raw", lambda *args: calls.append(int(args[0].shape[-1])) or real(*args))
    want = ei().overlap_counts_host(a, b)
    same(backend.label_overlap(ta, tb), want)
    assert calls == [67]
    del calls[:]
    same(backend.label_overlap(ta, tb, work_bytes=200 * 40 * 5), want)      # 200 voxels of 5 streams per call
    assert calls == [200] * 5 + [5]


def test_overlap_counts_dispatches_to_the_device(monkeypatch):
    from patchperpix_amd import backend
    calls = []
    real = backend.label_overlap
    monkeypatch.setattr(backend, "label_overlap", lambda a, b: calls.append(1) or real(a, b))
    rng = np.random.default_rng(4)
    a, b = runs_stack(rng, 1, (2, 7, 130), 5, 6.0), runs_stack(rng, 2, (2, 7, 130), 5, 6.0)
    same(ei().overlap_counts(a, b), ei().overlap_counts_host(a, b))
    assert calls == [1]
    monkeypatch.setenv("PPP_POSTPROCESS", "host")
    same(ei().overlap_counts(a, b), ei().overlap_counts_host(a, b))
    assert calls == [1]


# ---------------------------------------------------------------------------------------------
# file level, the device on and off
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tubes_case():
    """(gt, pred, pred2): a 24 x 40 x 40 volume of about six tubes; pred is gt with one tube split, two merged
    and one shifted; pred2 the same as two overlapping channels"""
    from patchperpix_amd import synth
    gt = synth.make_case((24, 40, 40), (1, 1, 1), seed=3, kind="tubes", n_tubes=6, radius=2.0)["labels"].astype(np.uint32)
    ids = [int(i) for i in np.unique(gt) if i]
    assert len(ids) >= 5
    pred = gt.copy()
    zz = np.arange(24)[:, None, None]
    pred[(gt == ids[0]) & (zz >= 12)] = 101                              # split
    pred[gt == ids[2]] = ids[1]                                          # merged
    shifted = np.zeros_like(gt)
    shifted[:, 2:, :] = np.where(gt == ids[3], ids[3], 0)[:, :-2, :]
    pred[gt == ids[3]] = 0
    pred[(shifted != 0) & (pred == 0)] = ids[3]                          # shifted
    second = np.zeros_like(pred)
    second[:, :, 1:] = np.where(pred == ids[1], 202, 0)[:, :, :-1]       # a copy of the merged one, overlapping it
    return gt, pred, np.stack([pred, second])


def _write(path, key, array):
    from patchperpix_amd import minihdf5
    with minihdf5.File(path, "w") as f:
        f.create_dataset(key, data=array, dtype=array.dtype, compression="gzip")


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("strategy", ["greedy", "hungarian"])
@pytest.mark.parametrize("criterion", ["iou", "cldice"])
def test_evaluate_file_device_equals_host(tmp_path, monkeypatch, criterion, strategy, channels):
    from patchperpix_amd import backend
    gt, pred, pred2 = tubes_case()
    res = pred if channels == 1 else pred2
    _write(str(tmp_path / "s.hdf"), "vote_instances", res)
    _write(str(tmp_path / "gt.hdf"), "volumes/gt_instances", gt)
    kw = dict(res_key="vote_instances", gt_key="volumes/gt_instances", localization_criterion=criterion,
              assignment_strategy=strategy, evaluate_false_labels=True, remove_small_components=3, from_scratch=True)
    if criterion == "cldice":
        kw.update(add_general_metrics=["avg_gt_skel_coverage", "avg_f1_cov_score"],
                  add_multi_thresh_metrics=["avg_tp_skel_coverage"])
    calls = []
    real = backend.label_overlap
    monkeypatch.setattr(backend, "label_overlap", lambda a, b: calls.append(1) or real(a, b))
    dev = ei().evaluate_file(str(tmp_path / "s.hdf"), str(tmp_path / "gt.hdf"), out_dir=str(tmp_path / "dev"), **kw)
    assert len(calls) == (2 if criterion == "cldice" else 1)
    monkeypatch.setenv("PPP_POSTPROCESS", "host")
    host = ei().evaluate_file(str(tmp_path / "s.hdf"), str(tmp_path / "gt.hdf"), out_dir=str(tmp_path / "host"), **kw)
    assert len(calls) == (2 if criterion == "cldice" else 1)
    assert dev == host
    assert open(str(tmp_path / "dev" / "s.toml")).read() == open(str(tmp_path / "host" / "s.toml")).read()
    assert dev["general"]["Num GT"] >= 5 and dev["general"]["Num Pred"] == dev["general"]["Num GT"] + channels - 1
    th = dev["confusion_matrix"]["th_0_5"]
    # one prediction covers two gt tubes: one of them stays unmatched unless the second channel's copy takes it
    assert 0 < th["AP_TP"] < dev["general"]["Num GT"] + channels - 1 and th["false_merge"] >= 1
