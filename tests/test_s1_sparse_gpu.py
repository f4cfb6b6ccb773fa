"""S1 on sparse foreground (ppp_consensus_sparse: item pre-pass, the packed kernel over the active
items, zero stores for the others) against the dense launch, bit for bit.

Every comparison runs both paths over a buffer prefilled with the same 0xFF pattern and compares the
WHOLE buffers as uint32: an entry one path writes and the other leaves shows up as a mismatch."""
import ctypes
import json
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from tests_flags import FLYLIGHT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert backend.device_count() >= 1
    return torch


def _poisoned(torch, n):
    return torch.full((int(n),), -1, dtype=torch.int32, device="cuda")       # 0xFFFFFFFF


def _s1(torch, pred, ov, P, mode, n_el, part=None, open_rows=False, want_count=False, cons=None):
    """One S1 call over poisoned buffers.  mode None: the dense entry points; 0 / 1: the sparse entry.
    Returns (cons int32 [n_el], count int32 [n_el] or None, (items, active, took_lists) or None)."""
    from patchperpix_amd import backend
    L = backend.lib()
    if cons is None:
        cons = _poisoned(torch, n_el)
    cnt = _poisoned(torch, n_el) if want_count else None
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())     # noqa: E731
    ovp = ptr(ov) if P.use_overlap else None
    box = backend.Box(*[int(v) for v in part]) if part is not None else None
    bref = ctypes.byref(box) if box is not None else None
    dt = backend.pred_dtype_code(pred)
    stream = backend._stream()
    items = None
    if mode is None:
        if part is not None:
            backend.check(L.ppp_consensus_part(ptr(pred), dt, ovp, ptr(cons), ctypes.byref(P), bref, stream))
        elif open_rows:
            backend.check(L.ppp_consensus_rows(ptr(pred), dt, ovp, ptr(cons), ctypes.byref(P), stream))
        else:
            backend.check(L.ppp_consensus(ptr(pred), dt, ovp, ptr(cons), ptr(cnt), ctypes.byref(P), stream))
    else:
        need = int(L.ppp_consensus_sparse_workspace_bytes(ctypes.byref(P), bref))
        assert need > 0
        work = torch.empty((need,), dtype=torch.uint8, device="cuda")
        backend.check(L.ppp_consensus_sparse(ptr(pred), dt, ovp, ptr(cons), ptr(cnt), ctypes.byref(P), bref,
                                             1 if open_rows else 0, ptr(work), mode, stream))
        items = backend.consensus_last_items()
    torch.cuda.synchronize()
    return cons, cnt, items


def _same(torch, a, b, what):
    assert a.dtype == torch.int32 and b.dtype == torch.int32
    if not torch.equal(a, b):
        bad = torch.nonzero(a != b).flatten()
        raise AssertionError("%s: %d of %d words differ, first at %d: %08x vs %08x" % (
            what, bad.numel(), a.numel(), int(bad[0]), int(a[bad[0]]) & 0xFFFFFFFF, int(b[bad[0]]) & 0xFFFFFFFF))


def _tube_case(shape, ps, seed, n_tubes, overlap=True):
    from patchperpix_amd import synth
    return synth.make_case(shape, list(ps), seed=seed, kind="tubes", n_tubes=n_tubes, radius=2.0,
                           overlap_frac=0.03 if overlap else 0.0)


def _valid(case, P):
    mid = case["pred"].shape[0] // 2
    v = case["pred"][mid] > np.float32(P.th)
    if P.use_overlap:
        v = v & ~(case["numinst"] > 1)
    return v


def _params(backend, shape, ps, layout, use_overlap, box=None, **extra):
    P = backend.make_params(shape, list(ps), cons_box=box, cons_layout=layout,
                            **dict(FLYLIGHT, overlapping_inst=bool(use_overlap)))
    for k, v in extra.items():
        setattr(P, k, v)
    return P


def _n_el(backend, P, ring=0):
    n = int(backend.lib().ppp_cons_elems(ctypes.byref(P)))
    if ring:
        n = n // (P.cons_box.z1 - P.cons_box.z0) * ring
    return n


@pytest.mark.parametrize("use_overlap", [True, False])
@pytest.mark.parametrize("f16", [True, False])
@pytest.mark.parametrize("X", [128, 96])
@pytest.mark.parametrize("px", [3, 5, 7, 9])
def test_lists_equal_dense_bit_for_bit(px, X, f16, use_overlap, torch_cuda):
    """px in {3, 5, 7, 9} x f16 / f32 x X = 128 (one line per run) / 96 (two lines flattened, a short
    last run) x overlap on / off, odd Z (the last slice pair half empty): closed voxel-major rows
    (ppp_consensus), open rows (ppp_consensus_rows), COMPACT planes with counts, a proper sub-box as
    `part` (COMPACT and open rows), a ring written by parts, and a part without foreground."""
    from patchperpix_amd import backend
    from oracle import ppp_oracle as orc
    torch = torch_cuda
    ps = (px, px, px)
    shape = (px + 4 if px < 9 else 11, 21, X)
    assert shape[0] % 2 == 1
    case = _tube_case(shape, ps, seed=px + X, n_tubes=3, overlap=use_overlap)
    # a slab without foreground (the empty part below)
    for k in ("labels",):
        case[k][:, :5, :] = 0
    from patchperpix_amd import synth
    case["pred"] = synth.pred_from_labels(case["labels"], list(ps), seed=px + X)
    case["foreground"] = case["labels"] != 0
    case["numinst"][~case["foreground"]] = 0
    pred = torch.from_numpy(case["pred"].astype(np.float16) if f16 else case["pred"]).cuda()
    ov = torch.from_numpy((case["numinst"] > 1).astype(np.uint8)).cuda()
    VM, CP = backend.CONS_VOXEL_MAJOR, backend.CONS_COMPACT

    def both(P, what, **kw):
        P = backend.with_pred_clean(pred, P)
        assert P.pred_clean == 1
        n = _n_el(backend, P, ring=P.ring_z)
        d = _s1(torch, pred, ov, P, None, n, **kw)
        s = _s1(torch, pred, ov, P, 1, n, **kw)
        _same(torch, d[0], s[0], what)
        if d[1] is not None:
            _same(torch, d[1], s[1], what + " (counts)")
        assert s[2][2] == 1 and backend.lib().ppp_consensus_kernel_name() == b"consensus_v3_kernel<lists>"
        return d, s

    # whole box: closed rows, open rows, planes + counts
    d, s = both(_params(backend, shape, ps, VM, use_overlap), "closed rows")
    assert not bool((s[0] == -1).any())                 # closed rows: fully overwritten
    both(_params(backend, shape, ps, VM, use_overlap), "open rows", open_rows=True)
    Pc = _params(backend, shape, ps, CP, use_overlap)
    d, s = both(Pc, "planes + counts", want_count=True)
    assert not bool((s[0] == -1).any()) and not bool((s[1] == -1).any())
    total, active, took = s[2]
    act, runs, rows = backend.s1_items_host(_valid(case, Pc), ps)
    assert (total, active) == (act.size, int(act.sum())) and 0 < active < total
    if px <= 7 and not f16:
        want = orc.positive_planes(orc.consensus_planes(case["pred"], 1 * (case["numinst"] > 1), list(ps),
                                                        **dict(FLYLIGHT, overlapping_inst=bool(use_overlap))), list(ps))
        got = s[0].cpu().numpy().view(np.uint32).reshape(want.shape)
        assert np.array_equal(got, np.ascontiguousarray(want).view(np.uint32))
    # a proper sub-box of a proper cons_box
    box = (1, 2, 3, shape[0] - 1, shape[1] - 1, shape[2] - 2)
    part = (2, 4, 9, shape[0] - 1, shape[1] - 3, shape[2] - 10)
    for layout in (CP, VM):
        d, s = both(_params(backend, shape, ps, layout, use_overlap, box=box), "part, layout %d" % layout, part=part)
        act, _, _ = backend.s1_items_host(_valid(case, Pc), ps, part=part)
        assert s[2][:2] == (act.size, int(act.sum()))
    # a part that holds no foreground at all: zero active items, only zero stores
    empty = (0, 0, 0, shape[0], 3, shape[2])
    d, s = both(_params(backend, shape, ps, CP, use_overlap), "empty part", part=empty)
    assert s[2][1] == 0 and s[2][0] > 0
    # rows in a ring, written by two parts (the ring wraps inside the second)
    ring = shape[0] + 1
    Pr = backend.with_pred_clean(pred, _params(backend, shape, ps, VM, use_overlap, ring_z=ring, origin_z=3))
    n = _n_el(backend, Pr, ring=ring)
    bufs = []
    for mode in (None, 1):
        buf = _poisoned(torch, n)
        for part in ((0, 0, 0, 4, shape[1], shape[2]), (4, 0, 0, shape[0], shape[1], shape[2])):
            _s1(torch, pred, ov, Pr, mode, n, part=part, cons=buf)
        bufs.append(buf)
    _same(torch, bufs[0], bufs[1], "ring by parts")


@pytest.mark.parametrize("px,X", [(5, 96), (7, 128)])
def test_values_outside_the_unit_interval_take_the_exact_path(px, X, torch_cuda):
    """non-CLEAN input (a value above 1, a negative one, an infinity at a background centre): the
    general kernel and its exact path, lists against dense and against the oracle"""
    from patchperpix_amd import backend
    from oracle import ppp_oracle as orc
    torch = torch_cuda
    ps, shape = (px, px, px), (9, 21, X)
    case = _tube_case(shape, ps, seed=31 + px, n_tubes=3)
    fgz, fgy, fgx = np.nonzero(case["foreground"][px // 2:-(px // 2), px // 2:-(px // 2), px // 2:-(px // 2)])
    k = len(fgz) // 2
    z, y, x = fgz[k] + px // 2, fgy[k] + px // 2, fgx[k] + px // 2
    case["pred"][3, z, y, x] = 1.5
    case["pred"][7, z, y, x + 1] = -0.25
    pred = torch.from_numpy(case["pred"]).cuda()
    ov = torch.from_numpy((case["numinst"] > 1).astype(np.uint8)).cuda()
    P = backend.with_pred_clean(pred, _params(backend, shape, ps, backend.CONS_COMPACT, True))
    assert P.pred_clean == 2
    n = _n_el(backend, P)
    d = _s1(torch, pred, ov, P, None, n, want_count=True)
    s = _s1(torch, pred, ov, P, 1, n, want_count=True)
    _same(torch, d[0], s[0], "planes")
    _same(torch, d[1], s[1], "counts")
    want = orc.positive_planes(orc.consensus_planes(case["pred"], 1 * (case["numinst"] > 1), list(ps),
                                                    **dict(FLYLIGHT, overlapping_inst=True)), list(ps))
    assert np.array_equal(s[0].cpu().numpy().view(np.uint32).reshape(want.shape),
                          np.ascontiguousarray(want).view(np.uint32))


def test_all_foreground_has_no_inactive_item_and_auto_stays_dense(torch_cuda):
    """An all-foreground volume.  Over the whole volume the only inactive items are those whose
    partners all lie beyond the volume's faces (the criterion asks for w inside the volume): the counts
    equal the restatement's.  Over a part whose every partner row is inside the volume EVERY item is
    active: the inactive list is empty and no zero launch is made.  Auto mode makes today's launch."""
    from patchperpix_amd import backend, synth
    torch = torch_cuda
    ps, shape = (5, 5, 5), (13, 24, 96)
    lab = np.ones(shape, dtype=np.int64)
    pred = torch.from_numpy(synth.pred_from_labels(lab, list(ps), seed=2).astype(np.float16)).cuda()
    P = backend.with_pred_clean(pred, _params(backend, shape, ps, backend.CONS_VOXEL_MAJOR, False))
    n = _n_el(backend, P)
    valid = np.ones(shape, dtype=bool)
    # whole volume, closed rows
    d = _s1(torch, pred, None, P, None, n)
    assert backend.lib().ppp_consensus_kernel_name() == b"consensus_v3_kernel"
    s = _s1(torch, pred, None, P, 1, n)
    act, _, _ = backend.s1_items_host(valid, ps)
    assert s[2] == (act.size, int(act.sum()), 1) and s[2][1] > 0.7 * s[2][0]
    _same(torch, d[0], s[0], "all foreground, lists")
    a = _s1(torch, pred, None, P, 0, n)                          # auto: today's launch
    assert a[2] == (act.size, int(act.sum()), 0)
    assert backend.lib().ppp_consensus_kernel_name() == b"consensus_v3_kernel"
    _same(torch, d[0], a[0], "all foreground, auto")
    # a part whose partners (dz <= 4, |dy| <= 4) all lie inside the volume: zero inactive items
    part = (0, 4, 0, 9, 20, 96)
    act, _, _ = backend.s1_items_host(valid, ps, part=part)
    assert act.all()
    d = _s1(torch, pred, None, P, None, n, part=part)
    s = _s1(torch, pred, None, P, 1, n, part=part)               # an empty inactive list: no zero launch
    assert s[2] == (act.size, act.size, 1)
    _same(torch, d[0], s[0], "all foreground part, lists")
    a = _s1(torch, pred, None, P, 0, n, part=part)
    assert a[2] == (act.size, act.size, 0)
    assert backend.lib().ppp_consensus_kernel_name() == b"consensus_v3_kernel"
    _same(torch, d[0], a[0], "all foreground part, auto")


def test_errors_match_the_dense_entry_points(torch_cuda):
    from patchperpix_amd import backend
    torch = torch_cuda
    L = backend.lib()
    ps, shape = (5, 5, 5), (7, 20, 64)
    kw = dict(FLYLIGHT)
    # parameters the packed kernel does not serve: no work space, the dense path stays
    P = backend.make_params(shape, list(ps), **dict(kw, patch_threshold=0.6))
    assert L.ppp_consensus_sparse_workspace_bytes(ctypes.byref(P), None) == 0
    P = backend.make_params(shape, list(ps), cons_layout=backend.CONS_REFERENCE, **kw)
    assert L.ppp_consensus_sparse_workspace_bytes(ctypes.byref(P), None) == 0
    P = backend.make_params(shape, list(ps), **kw)
    assert L.ppp_consensus_sparse_workspace_bytes(ctypes.byref(P), None) > 0
    bad = backend.Box(0, 0, 0, 8, 20, 64)
    assert L.ppp_consensus_sparse_workspace_bytes(ctypes.byref(P), ctypes.byref(bad)) == 0
    buf = torch.zeros((16,), dtype=torch.float32, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    assert L.ppp_consensus_sparse(p, 0, None, p, None, ctypes.byref(P), ctypes.byref(bad), 0, p, 1, None) != 0
    assert b"sub-box" in L.ppp_last_error()
    assert L.ppp_consensus_sparse(p, 0, None, p, None, ctypes.byref(P), None, 0, None, 1, None) != 0
    assert L.ppp_consensus_sparse(p, 0, None, p, None, ctypes.byref(P), None, 0, p, 2, None) != 0


def test_backend_takes_the_sparse_entry_from_the_environment(torch_cuda, monkeypatch):
    """PPP_S1_SPARSE = 0 / 1 / auto through backend.consensus, consensus_voxel_major and
    consensus_part: same output, and the item counts in the notes"""
    from patchperpix_amd import backend
    torch = torch_cuda
    ps, shape = (7, 7, 7), (13, 40, 96)
    case = _tube_case(shape, ps, seed=4, n_tubes=3)
    pred = torch.from_numpy(case["pred"].astype(np.float16)).cuda()
    ov = torch.from_numpy((case["numinst"] > 1).astype(np.uint8)).cuda()
    P = _params(backend, shape, ps, backend.CONS_COMPACT, True)
    act, _, _ = backend.s1_items_host(_valid(case, P), ps)
    out = {}
    for mode in ("0", "1", "auto"):
        monkeypatch.setenv("PPP_S1_SPARSE", mode)
        backend.reload_env()
        for k in ("s1_items", "s1_active_items", "s1_list_launches"):
            backend.NOTES.pop(k, None)
        cons, cnt = backend.consensus(pred, ov, P, want_count=True)
        notes = (backend.NOTES.get("s1_items"), backend.NOTES.get("s1_active_items"))
        assert notes == ((None, None) if mode == "0" else (act.size, int(act.sum())))
        rows, Pv = backend.consensus_voxel_major(pred, ov, P, open_rows=False)
        part = (2, 3, 5, 11, 30, 90)
        pool = _poisoned(torch, rows.numel()).view(torch.float32)
        backend.consensus_part(pred, ov, Pv, part, pool)
        out[mode] = [t.view(torch.int32).flatten() for t in (cons, cnt, rows, pool)]
        if mode == "1":
            assert backend.NOTES.get("s1_list_launches") == 3
    for mode in ("1", "auto"):
        for a, b, what in zip(out["0"], out[mode], ("planes", "counts", "rows", "part")):
            _same(torch, a, b, "PPP_S1_SPARSE=%s %s" % (mode, what))
    monkeypatch.setenv("PPP_S1_SPARSE", "maybe")
    with pytest.raises(ValueError):
        backend.consensus(pred, ov, P)


@pytest.mark.parametrize("name", ["t96_p9", "t70x140_p7"])
def test_tubes_end_to_end_against_the_oracle(name, torch_cuda):
    """to_instance_seg on tubes under the shipped flylight flags equals the oracle's instance map id
    for id (tests/golden/scale_tubes_<name>.npz, tests/golden/gen_scale_tubes_fixture.py): S1 over
    the item lists and with the dense launch, untiled and cut into 2 x 2 x 2 tiles."""
    from patchperpix_amd import backend, synth
    from patchperpix_amd.flags import FLYLIGHT as SHIPPED
    from patchperpix_amd.vote_instances import vote_instances as vi
    torch = torch_cuda
    z = np.load(os.path.join(GOLDEN_DIR, "scale_tubes_%s.npz" % name))
    shape, ps = tuple(int(v) for v in z["shape"]), [int(v) for v in z["patchshape"]]
    case = synth.make_case(shape, ps, **json.loads(str(z["synth_kwargs"])))
    pred16 = case["pred"].astype(np.float16)
    assert zlib.crc32(np.ascontiguousarray(pred16).tobytes()) == int(z["pred_f16_crc32"])       # same input
    kw = dict(SHIPPED, **json.loads(str(z["flags"])))
    run = dict(kw, save_no_intermediates=True, sample=1.0, result_folder="/tmp", affinities="x.zarr")
    pred = torch.from_numpy(pred16).cuda()
    fg = case["foreground"]
    want = z["instances"]
    assert len(np.unique(want)) - 1 == int(z["n_instances"]) > 5
    for sparse in (True, False):
        for grid in (dict(_n_slabs=1), dict(_n_slabs=2, _yx_tiles=(2, 2))):
            for k in ("s1_items", "s1_active_items", "s1_list_launches"):
                backend.NOTES.pop(k, None)
            inst, fgo = vi.to_instance_seg(pred, fg.copy(), fg.copy(), case["numinst"].copy(), ps,
                                           **dict(run, _s1_sparse=sparse, **grid))
            assert np.array_equal(inst, want), (sparse, grid)
            if sparse:
                assert backend.NOTES["s1_list_launches"] >= 1
                assert 0 < backend.NOTES["s1_active_items"] < 0.5 * backend.NOTES["s1_items"]
            else:
                assert "s1_items" not in backend.NOTES
