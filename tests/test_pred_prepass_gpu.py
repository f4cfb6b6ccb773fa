"""GPU: ppp_pred_prepass (csrc/ppp_prepass.hip) -- one read of the prediction for the clean flag, S2's masks and
the cover's per-voxel patch bits -- against the separate entries it stands for, byte for byte on the same input:

  M, info, valid   the first three arrays of ppp_rank_patches_vm's workspace after its own pre-pass (both
                   workspaces begin with the same description, ppp_rank_masks.hpp, and start from zero bytes)
  score            after the pre-pass alone: written exactly at the border, background and nP == 0 centres (a NumPy
                   restatement of that set), and there equal to ppp_rank_patches_vm's result; after
                   ppp_rank_patches_vm_prepared: the whole volume equal to ppp_rank_patches_vm's
  bits_vol         ppp_patch_bits_volume for fc_threshold
  unclean          the bits of ppp_pred_check

on the smallest volumes that cross a wave (X = 70: 64 lanes + a ragged mask row of 6 centres after four full rows
of 16) or are one mask row plus one centre (X = 17), barely taller than the patch (Z = p + 1), in the three element
types, with fc_threshold != patch_threshold and the shipped pair, a non-zero overlap mask, both border scores, and
values planted at the first and the last element of the tensor: each threshold itself, and 1.5, -0.1, NaN, inf in
turn.  Then the gather kernel against ppp_patch_bits, and a geometry the pass does not compile in."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PATCHES = (5, 7, 9)
DTYPES = ("float16", "bfloat16", "float32")
UNCLEAN = (1.5, -0.1, float("nan"), float("inf"))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert backend.device_count() >= 1
    return torch


def _shapes(p):
    return ((p + 1, p + 2, 70), (11, 9, 17))


def _flags(th, norm_rank):
    from tests_flags import FLYLIGHT
    return dict(FLYLIGHT, patch_threshold=th, overlapping_inst=True, rank_norm_patch_score=norm_rank)


_BASE = {}


def _base(torch, p, shape):
    """per (patch, volume), made once and left unchanged: a float32 prediction of synthetic cells with every value
    strictly inside (0, 1) and away from 0.4 / 0.5 / 0.6, an overlap mask with set voxels, and voxel-major rows
    for the ranking calls to read (both arms read the same rows: their content does not matter to the comparison,
    S1's result for the unplanted prediction is as good as any)"""
    key = (p, shape)
    if key not in _BASE:
        from patchperpix_amd import backend, synth
        ps = (p, p, p)
        c = synth.make_case(shape, ps, seed=170 + p, cell=[2 * p, 2 * p, 2 * p], overlap_frac=0.05)
        rng = np.random.default_rng(p * 1000 + shape[2])
        pred = np.where(c["pred"] > 0.5, rng.uniform(0.65, 0.97, c["pred"].shape), rng.uniform(0.03, 0.35, c["pred"].shape))
        # (some partners between the two fc / patch thresholds of the unequal case, on either side of 0.5)
        mid_band = rng.random(c["pred"].shape) < 0.1
        pred = np.where(mid_band, rng.choice(np.array([0.43, 0.47, 0.53, 0.57]), c["pred"].shape), pred).astype(np.float32)
        ov = (rng.random(shape) < 0.08).astype(np.uint8)
        assert ov.any()
        P = backend.make_params(shape, ps, **_flags(0.5, True))
        pred_d = torch.from_numpy(pred).cuda()
        rows, _ = backend.consensus_voxel_major(pred_d, torch.from_numpy(ov).cuda(), P)
        _BASE[key] = (pred, ov, rows)
    return _BASE[key]


def _to_dtype(torch, a32, dtype):
    return torch.from_numpy(a32).to(getattr(torch, dtype)).cuda().contiguous()


def _plant(torch, pred_d, first, last):
    flat = pred_d.view(-1)
    flat[0] = first
    flat[-1] = last


def _separate(torch, pred_d, ov_d, rows, P, Pv, fc):
    """today's launches: (M | info | valid bytes, final score, bits_vol, unclean bits)"""
    from patchperpix_amd import backend
    L = backend.lib()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    backend.check(L.ppp_pred_check(pred_d.data_ptr(), backend.pred_dtype_code(pred_d), pred_d.numel(), flag.data_ptr(),
                                   ctypes.byref(P), None))
    work = torch.zeros(int(L.ppp_rank_workspace_bytes(None, ctypes.byref(Pv))), dtype=torch.uint8, device="cuda")
    score = torch.zeros(tuple(P.shape), dtype=torch.float32, device="cuda")
    backend.check(L.ppp_rank_patches_vm(pred_d.data_ptr(), backend.pred_dtype_code(pred_d), rows.data_ptr(), ov_d.data_ptr(),
                                        score.data_ptr(), None, work.data_ptr(), ctypes.byref(Pv), None))
    assert backend.lib().ppp_rank_kernel_name() == b"rank_wg_kernel"
    V = int(np.prod(P.shape))
    words = (P.pz * P.py * P.px + 31) // 32
    bits = torch.zeros((V, words), dtype=torch.int32, device="cuda")
    backend.check(L.ppp_patch_bits_volume(pred_d.data_ptr(), backend.pred_dtype_code(pred_d), float(fc), bits.data_ptr(),
                                          ctypes.byref(P), None))
    torch.cuda.synchronize()
    return work, score, bits, int(flag.item())


def _written_set(pred_d, ov, P, th):
    """NumPy: the centres whose score needs no consensus -- not interior, or not foreground, or without a first
    pixel (no partner that is valid -- foreground, not overlap -- and above the threshold)"""
    pred = pred_d.float().cpu().numpy().astype(np.float64)
    p = int(P.pz)
    r = p // 2
    Z, Y, X = pred.shape[1:]
    mid = (p ** 3) // 2
    fg = pred[mid] > th
    valid = fg & (ov == 0)
    interior = np.zeros((Z, Y, X), bool)
    interior[r:Z - r, r:Y - r, r:X - r] = True
    n_first = np.zeros((Z, Y, X), np.int64)
    pad = np.pad(valid, r)
    ch = 0
    for dz in range(p):
        for dy in range(p):
            for dx in range(p):
                n_first += (pred[ch] > th) & pad[dz:dz + Z, dy:dy + Y, dx:dx + X]
                ch += 1
    return ~interior | ~fg | (n_first == 0), interior


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", PATCHES)
@pytest.mark.parametrize("which", (0, 1))
def test_prepass_equals_the_separate_launches(which, p, dtype, torch_cuda):
    from patchperpix_amd import backend
    torch = torch_cuda
    L = backend.lib()
    shape = _shapes(p)[which]
    ps = (p, p, p)
    pred32, ov, rows = _base(torch, p, shape)
    ov_d = torch.from_numpy(ov).cuda()
    turn = PATCHES.index(p) * 6 + DTYPES.index(dtype) * 2 + which          # which unclean value this case plants
    for ti, (fc, th, norm_rank) in enumerate(((0.4, 0.6, turn % 2 == 0), (0.5, 0.5, turn % 2 == 1))):
        P = backend.make_params(shape, ps, **_flags(th, norm_rank))
        Pv = P.copy()
        Pv.cons_layout = backend.CONS_VOXEL_MAJOR
        nbytes = int(L.ppp_pred_prepass_workspace_bytes(None, ctypes.byref(P)))
        assert nbytes > 0
        off = (ctypes.c_int64 * 5)()
        backend.check(L.ppp_pred_prepass_layout(None, ctypes.byref(P), off))
        assert off[0] == 0 and list(off) == sorted(off) and off[4] + 4 <= nbytes
        bad = UNCLEAN[(turn + ti) % len(UNCLEAN)]
        for first, last in ((th, fc), (fc, th), (bad, bad)):
            pred_d = _to_dtype(torch, pred32, dtype)
            _plant(torch, pred_d, first, last)
            work0, score0, bits0, unclean0 = _separate(torch, pred_d, ov_d, rows, P, Pv, fc)
            if first == bad:
                assert unclean0 & 1, (bad, unclean0)          # (the planted value is what the case says it is)
            # ---- the fused pass, on a score volume of sentinels: what it writes, and where
            work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            score = torch.full(tuple(shape), 123.0, dtype=torch.float32, device="cuda")
            backend.check(L.ppp_pred_prepass(pred_d.data_ptr(), backend.pred_dtype_code(pred_d), ov_d.data_ptr(), float(fc),
                                             score.data_ptr(), None, work.data_ptr(), ctypes.byref(P), None))
            torch.cuda.synchronize()
            tag = (shape, dtype, fc, th, first, last)
            assert torch.equal(work[:off[3]], work0[:off[3]]), ("M / info / valid", tag)
            V = int(np.prod(shape))
            got_bits = work[off[3]:off[3] + bits0.numel() * 4].view(torch.int32).view(V, -1)
            assert torch.equal(got_bits, bits0), ("bits_vol", tag)
            assert int(work[off[4]:off[4] + 4].view(torch.int32).item()) == unclean0, ("unclean", tag)
            written, interior = _written_set(pred_d, ov, P, th)
            s = score.cpu().numpy()
            assert np.array_equal(s != 123.0, written), ("which scores the pass writes", tag)
            assert np.array_equal(s[written].view(np.uint32), score0.cpu().numpy()[written].view(np.uint32)), ("scores", tag)
            assert np.all(s[~interior] == (-1.0 if norm_rank else -9999999.0))
            # ---- the ranking call that starts from these masks: the whole score volume
            score = torch.zeros(tuple(shape), dtype=torch.float32, device="cuda")
            backend.check(L.ppp_pred_prepass(pred_d.data_ptr(), backend.pred_dtype_code(pred_d), ov_d.data_ptr(), float(fc),
                                             score.data_ptr(), None, work.data_ptr(), ctypes.byref(P), None))
            own = torch.zeros(int(L.ppp_rank_prepared_workspace_bytes(ctypes.byref(Pv))), dtype=torch.uint8, device="cuda")
            backend.check(L.ppp_rank_patches_vm_prepared(rows.data_ptr(), score.data_ptr(), None, work.data_ptr(), own.data_ptr(),
                                                         ctypes.byref(Pv), None))
            torch.cuda.synchronize()
            assert torch.equal(score.view(torch.int32), score0.view(torch.int32)), ("prepared ranking", tag)


def test_prepass_on_an_inner_score_box(torch_cuda):
    """a score box inside the volume (what a tile of centres is): masks and pair counts of ITS centres, in ITS
    layout; valid and bits_vol stay those of the whole volume"""
    from patchperpix_amd import backend
    torch = torch_cuda
    L = backend.lib()
    p, shape = 7, (8, 9, 70)
    pred32, ov, rows = _base(torch, p, shape)
    ov_d = torch.from_numpy(ov).cuda()
    pred_d = _to_dtype(torch, pred32, "float16")
    P = backend.make_params(shape, (p, p, p), **_flags(0.5, True))
    Pv = P.copy()
    Pv.cons_layout = backend.CONS_VOXEL_MAJOR
    box = backend.Box(2, 1, 5, 7, 8, 59)
    work0 = torch.zeros(int(L.ppp_rank_workspace_bytes(ctypes.byref(box), ctypes.byref(Pv))), dtype=torch.uint8, device="cuda")
    score0 = torch.zeros(shape, dtype=torch.float32, device="cuda")
    backend.check(L.ppp_rank_patches_vm(pred_d.data_ptr(), backend.F16, rows.data_ptr(), ov_d.data_ptr(), score0.data_ptr(),
                                        ctypes.byref(box), work0.data_ptr(), ctypes.byref(Pv), None))
    off = (ctypes.c_int64 * 5)()
    backend.check(L.ppp_pred_prepass_layout(ctypes.byref(box), ctypes.byref(P), off))
    work = torch.zeros(int(L.ppp_pred_prepass_workspace_bytes(ctypes.byref(box), ctypes.byref(P))), dtype=torch.uint8, device="cuda")
    score = torch.zeros(shape, dtype=torch.float32, device="cuda")
    backend.check(L.ppp_pred_prepass(pred_d.data_ptr(), backend.F16, ov_d.data_ptr(), 0.5, score.data_ptr(), ctypes.byref(box),
                                     work.data_ptr(), ctypes.byref(P), None))
    own = torch.zeros(int(L.ppp_rank_prepared_workspace_bytes(ctypes.byref(Pv))), dtype=torch.uint8, device="cuda")
    backend.check(L.ppp_rank_patches_vm_prepared(rows.data_ptr(), score.data_ptr(), ctypes.byref(box), work.data_ptr(),
                                                 own.data_ptr(), ctypes.byref(Pv), None))
    torch.cuda.synchronize()
    assert torch.equal(work[:off[3]], work0[:off[3]])
    assert torch.equal(score.view(torch.int32), score0.view(torch.int32))


@pytest.mark.parametrize("p", PATCHES)
def test_gather_from_the_table_equals_patch_bits(p, torch_cuda):
    """patch_bits_from_table against patch_bits_kernel on a centre list with repeats, the first and the last voxel"""
    from patchperpix_amd import backend
    torch = torch_cuda
    L = backend.lib()
    shape = _shapes(p)[0]
    pred32, ov, _ = _base(torch, p, shape)
    pred_d = _to_dtype(torch, pred32, "bfloat16")
    P = backend.make_params(shape, (p, p, p), **_flags(0.6, True))
    rng = np.random.default_rng(p)
    cen = np.stack([rng.integers(0, s, 300) for s in shape], 1).astype(np.int32)
    cen[0] = (0, 0, 0)
    cen[1] = [s - 1 for s in shape]
    cen[2:40] = cen[40:78]                     # repeats
    cen[-1] = cen[1]
    cen_d = torch.from_numpy(cen).cuda()
    want = torch.zeros((len(cen), (p ** 3 + 31) // 32), dtype=torch.int32, device="cuda")
    backend.check(L.ppp_patch_bits(pred_d.data_ptr(), backend.BF16, cen_d.data_ptr(), len(cen), 0.4, want.data_ptr(),
                                   ctypes.byref(P), None))
    pre = backend.pred_prepass(pred_d, torch.from_numpy(ov).cuda(), 0.4, P, torch.zeros(shape, dtype=torch.float32, device="cuda"))
    assert pre is not None and pre.clean == 1 and pre.unclean_bits == 0
    got = backend.patch_bits_from_table(pre.bits_vol, cen_d, P)
    assert torch.equal(got, want)
    assert backend.patch_bits_from_table(pre.bits_vol, cen_d[:0], P).shape == (0, want.shape[1])


def test_other_geometries_keep_the_separate_kernels(torch_cuda):
    """3 x 5 x 7 is not compiled in: the size query says 0, the pass refuses, backend.pred_prepass returns None --
    and the kernels of before serve it: flag, patch bits of the volume, scores (the gather kernel) as the oracle's"""
    from oracle import ppp_oracle as orc
    from patchperpix_amd import backend, synth
    from tests_flags import FLYLIGHT
    torch = torch_cuda
    L = backend.lib()
    ps, shape = (3, 5, 7), (9, 12, 21)
    c = synth.make_case(shape, ps, seed=5, cell=[6, 10, 14], overlap_frac=0.05)
    pred = c["pred"].astype(np.float32)
    ov = (c["numinst"] > 1).astype(np.uint8)
    kw = dict(FLYLIGHT, overlapping_inst=True)
    P = backend.make_params(shape, ps, **kw)
    assert int(L.ppp_pred_prepass_workspace_bytes(None, ctypes.byref(P))) == 0
    pred_d, ov_d = torch.from_numpy(pred).cuda(), torch.from_numpy(ov).cuda()
    score = torch.zeros(shape, dtype=torch.float32, device="cuda")
    assert L.ppp_pred_prepass(pred_d.data_ptr(), backend.F32, ov_d.data_ptr(), 0.5, score.data_ptr(), None, score.data_ptr(),
                              ctypes.byref(P), None) != 0
    assert b"ppp_pred_prepass" in L.ppp_last_error()
    assert backend.pred_prepass(pred_d, ov_d, 0.5, P, score) is None
    assert backend.pred_check(pred_d, P) == 1
    cons = backend.consensus(pred_d, ov_d, P)
    got = backend.rank_patches(pred_d, cons, ov_d, P).cpu().numpy()
    want = orc.rank(pred, orc.consensus(pred, 1 * (ov > 0), ps, **kw), 1 * (ov > 0), ps, **kw)
    assert np.array_equal(np.asarray(want, np.float32).view(np.uint32), got.view(np.uint32))
    cen = torch.tensor([[0, 0, 0], [8, 11, 20], [4, 6, 10]], dtype=torch.int32, device="cuda")
    bits = backend.patch_bits(pred_d, cen, 0.5, P).cpu().numpy().view(np.uint32)
    words = (105 + 31) // 32
    for k, (z, y, x) in enumerate(cen.cpu().numpy()):
        on = pred[:, z, y, x] > np.float32(0.5)
        assert np.array_equal(np.packbits(on, bitorder="little"), bits[k].view(np.uint8)[:(105 + 7) // 8]), k
    assert bits.shape == (3, words)
