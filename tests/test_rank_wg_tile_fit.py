"""GPU (MI355X): the launch plan of the workgroup ranking kernel (ppp_rank_wg.hip) -- tiles of a run-time
thickness in z, XCD ranges of equal weight, the pre-pass with the cubic window compiled in -- forced through the
launcher's development switches (PPP_RANK_WG_TZ, PPP_RANK_WG_XCD, PPP_RANK_WG_SPLIT), because a
volume a test can afford is far below the size at which the rule chooses them.  Scores are compared as uint32 bit
patterns with the gather kernel on compact planes (the one pinned to the goldens and the oracle): no tolerance,
for the whole volume and for an inner score box inside a consensus box.  The rule itself is asked through
ppp_rank_wg_plan, without a launch."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCHES = ("PPP_RANK_WG_TILE", "PPP_RANK_WG_SPLIT", "PPP_RANK_WG_TZ", "PPP_RANK_WG_XCD", "PPP_RANK_ORDER",
            "PPP_RANK_TILE_MAJOR", "PPP_RANK_WG")
CASES = {"p7": ((7, 7, 7), (40, 37, 45), 12), "p5": ((5, 5, 5), (38, 41, 43), 9), "p9": ((9, 9, 9), (41, 36, 44), 13)}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert backend.device_count() >= 1
    return torch


def _build(torch, name, empty_upper_y=False):
    """ragged volume with overlap voxels; the gather kernel's scores for the whole volume; the inputs of the
    workgroup kernel for the whole volume and for an inner score box inside a consensus box.
    empty_upper_y: everything from y = 12 on is background -- only the first y-slab of tiles has weight"""
    from patchperpix_amd import backend, synth
    from tests_flags import FLYLIGHT
    ps, shape, cell = CASES[name]
    c = synth.make_case(shape, ps, seed=97, cell=[cell] * 3, overlap_frac=0.03)
    p = c["pred"].astype(np.float16)
    if empty_upper_y:
        p[:, :, 12:, :] = 0
    kw = dict(FLYLIGHT)
    P = backend.make_params(shape, ps, **kw)
    pred = torch.from_numpy(p).cuda()
    ov = torch.from_numpy((c["numinst"] > 1).astype(np.uint8)).cuda()
    cons = backend.consensus(pred, ov, P)
    want = backend.rank_patches(pred, cons, ov, P).cpu().numpy()
    assert (want > 0).sum() > (20 if empty_upper_y else 100)
    vm, Pv = backend.cons_to_voxel_major(cons, P)
    del cons
    r = ps[0] // 2
    sb = (r + 2, r + 1, r + 3, shape[0] - r - 3, shape[1] - r - 2, shape[2] - r - 5)
    box = (sb[0] - r, sb[1] - r, sb[2] - r, sb[3] + r, sb[4] + r, sb[5] + r)
    Pt = backend.make_params(shape, ps, cons_box=box, **kw)
    vm_t, Pvt = backend.cons_to_voxel_major(backend.consensus(pred, ov, Pt), Pt)
    return dict(pred=pred, ov=ov, want=want, vm=vm, Pv=Pv, vm_t=vm_t, Pvt=Pvt, sb=sb, shape=shape)


@pytest.fixture(scope="module")
def case7(torch_cuda):
    return _build(torch_cuda, "p7")


@pytest.fixture(scope="module")
def case7_uneven(torch_cuda):
    return _build(torch_cuda, "p7", empty_upper_y=True)


@pytest.fixture(scope="module", params=["p5", "p9"])
def case59(request, torch_cuda):
    return _build(torch_cuda, request.param)


class _Env:
    """the launcher's switches set for one block, every other one of them cleared"""

    def __init__(self, monkeypatch, **env):
        self.mp, self.env = monkeypatch, env

    def __enter__(self):
        from patchperpix_amd import backend
        for k in SWITCHES:
            self.mp.delenv(k, raising=False)
        for k, v in self.env.items():
            self.mp.setenv(k, v)
        backend.reload_env()

    def __exit__(self, *exc):
        from patchperpix_amd import backend
        self.mp.undo()
        backend.reload_env()


def _check_bits(case):
    from patchperpix_amd import backend
    got = backend.rank_patches(case["pred"], case["vm"], case["ov"], case["Pv"]).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), case["want"].view(np.uint32))
    sb = case["sb"]
    got_t = backend.rank_patches(case["pred"], case["vm_t"], case["ov"], case["Pvt"], score_box=sb).cpu().numpy()
    sl = tuple(slice(sb[i], sb[i + 3]) for i in range(3))
    assert np.array_equal(got_t[sl].view(np.uint32), case["want"][sl].view(np.uint32))


# z step 13 leaves a last tile one slice thick (thinner than the radius), 16 a ragged last tile of 8
@pytest.mark.parametrize("split", ["0", "2"])
@pytest.mark.parametrize("ranges", ["count", "weight"])
@pytest.mark.parametrize("tz", ["9", "10", "13", "16"])
def test_forced_z_step(case7, tz, ranges, split, monkeypatch):
    from patchperpix_amd import backend
    with _Env(monkeypatch, PPP_RANK_WG_TZ=tz, PPP_RANK_WG_XCD=ranges, PPP_RANK_WG_SPLIT=split):
        plan = backend.rank_wg_plan(case7["Pv"])
        t = int(tz)
        assert plan["tile"] == (16, 16, 16) and plan["tz_step"] == t and plan["ranges"] == ranges
        assert plan["tiles"] == -(-40 // t) * 3 * 3 and plan["splits"] == int(split)
        _check_bits(case7)


# only the first y-slab of the y-major tile sequence has weight: the weight cuts all fall into it and the last
# range would take every tile behind them -- more than an XCD's slots hold, so the clamp moves the cuts back
@pytest.mark.parametrize("env", [dict(PPP_RANK_WG_TZ="10", PPP_RANK_WG_SPLIT="0"),
                                 dict(PPP_RANK_WG_TZ="10", PPP_RANK_WG_SPLIT="2"),
                                 dict(PPP_RANK_WG_TILE="8x8x16", PPP_RANK_WG_SPLIT="0"),
                                 dict(PPP_RANK_WG_TILE="8x8x16", PPP_RANK_WG_SPLIT="3")],
                         ids=["tz10", "tz10-split2", "8x8x16", "8x8x16-split3"])
def test_uneven_weights_clamp_ranges(case7_uneven, env, monkeypatch):
    from patchperpix_amd import backend
    with _Env(monkeypatch, PPP_RANK_WG_XCD="weight", **env):
        plan = backend.rank_wg_plan(case7_uneven["Pv"])
        per_xcd = -(-plan["tiles"] // 8)
        assert plan["ranges"] == "weight" and plan["slots"] == per_xcd + plan["splits"] + (per_xcd + 3) // 4
        # (a third of the tiles have weight: eight equal ranges of them leave more than `slots` to the last)
        assert plan["tiles"] - plan["tiles"] // 3 > plan["slots"]
        _check_bits(case7_uneven)


def test_other_sizes_same_bits(case59, monkeypatch):
    """5^3 and 9^3 did not get the new launch paths: their default launches, and the ranges by weight that the
    switch gives any size, against the gather kernel"""
    from patchperpix_amd import backend
    with _Env(monkeypatch):
        plan = backend.rank_wg_plan(case59["Pv"])
        assert plan["tile"] == (8, 8, 16) and plan["tz_step"] == 8 and plan["ranges"] == "count" and plan["splits"] == 0
        _check_bits(case59)
    with _Env(monkeypatch, PPP_RANK_WG_TZ="10"):      # (7^3 only: ignored here)
        assert backend.rank_wg_plan(case59["Pv"]) == plan
    with _Env(monkeypatch, PPP_RANK_WG_XCD="weight", PPP_RANK_WG_SPLIT="1"):
        _check_bits(case59)


def _run_vm(torch, case):
    """one ppp_rank_patches_vm call on a zeroed workspace of the test's own: the scores and the whole workspace
    (masks M, info, validity, tile weights and order) as the call left them"""
    from patchperpix_amd import backend
    L = backend.lib()
    Pv = case["Pv"]
    nbytes = int(L.ppp_rank_workspace_bytes(None, ctypes.byref(Pv)))
    work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.zeros(case["shape"], dtype=torch.float32, device="cuda")
    backend.check(L.ppp_rank_patches_vm(backend._dev_ptr(case["pred"]), backend.pred_dtype_code(case["pred"]),
                                        backend._dev_ptr(case["vm"]), backend._dev_ptr(case["ov"]), backend._dev_ptr(out),
                                        None, backend._dev_ptr(work), ctypes.byref(Pv), backend._stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32), work.cpu().numpy()


def test_prepass_cube_scores_and_workspace(torch_cuda, case7, case59, monkeypatch):
    """the raw call with no switch set, on a workspace of the test's own: the final scores -- which hold the
    pre-pass's (border, background, no first pixel) -- are the gather kernel's, and the pre-pass with the window
    compiled in left its masks and info in the workspace"""
    for case in (case7, case59):
        with _Env(monkeypatch):
            score, work = _run_vm(torch_cuda, case)
        assert np.count_nonzero(work) > 1000
        assert np.array_equal(score, case["want"].view(np.uint32))


# ---- the rule, without a launch -------------------------------------------------------------------------------
def _plan_params(shape, ps):
    from patchperpix_amd import backend
    from tests_flags import FLYLIGHT
    P = backend.make_params(shape, ps, **dict(FLYLIGHT))
    Pv = P.copy()
    Pv.cons_layout = backend.CONS_VOXEL_MAJOR
    return Pv


def _todays_plan(shape, p, resident, cus):
    """the launcher's choice before the tile fit, restated: 8 x 16 x 16 from 1 024 such tiles on (never at 9^3),
    else 8 x 8 x 16; the tiles beyond the last full round split when their halves fit it"""
    cdiv = lambda a, b: -(-a // b)
    big = cdiv(shape[0], 8) * cdiv(shape[1], 16) * cdiv(shape[2], 16) >= 1024 and p != 9
    ty = 16 if big else 8
    tiles = cdiv(shape[0], 8) * cdiv(shape[1], ty) * cdiv(shape[2], 16)
    per_xcd, slots, splits = cdiv(tiles, 8), resident * cus, 0
    if big and per_xcd > slots and 2 * (per_xcd % slots) <= slots:
        splits = per_xcd % slots
    return dict(tile=(8, ty, 16), tz_step=8, tiles=tiles, splits=splits, slots=per_xcd + splits, ranges="count")


def test_plan_rule(torch_cuda, monkeypatch):
    from patchperpix_amd import backend
    with _Env(monkeypatch):
        # the default benchmark's launch: 183 tiles of 8 x 16 x 16 per XCD for 160 slots -- one round and a tail;
        # z step 10 is the thinnest tile whose 142 per XCD fit (9 gives 162)
        plan = backend.rank_wg_plan(_plan_params((140, 140, 140), (7, 7, 7)), None, 5, 32)
        assert plan["tile"] == (16, 16, 16) and plan["tz_step"] == 10 and plan["tiles"] == 14 * 9 * 9 and plan["splits"] == 0
        # (ranges of equal weight, which may grow by a quarter beyond the 142 tiles of an equal count)
        assert plan["ranges"] == "weight" and plan["slots"] == 142 + 36
        # four workgroups per CU: 128 slots -- 183 is still between one and two rounds, and z step 12 (122) fits
        assert backend.rank_wg_plan(_plan_params((140, 140, 140), (7, 7, 7)), None, 4, 32)["tz_step"] == 12
        # launches that are not between one and two rounds, and other sizes: today's plan
        for shape, p in (((112, 176, 176), 9), ((64, 64, 64), 7), ((200, 200, 200), 7), ((140, 140, 140), 5),
                         ((96, 128, 128), 7)):
            assert backend.rank_wg_plan(_plan_params(shape, (p, p, p)), None, 5, 32) == _todays_plan(shape, p, 5, 32), (shape, p)
    # the switches and the caller's tile win over the rule
    with _Env(monkeypatch, PPP_RANK_WG_SPLIT="23"):
        assert backend.rank_wg_plan(_plan_params((140, 140, 140), (7, 7, 7)), None, 5, 32) == \
            dict(tile=(8, 16, 16), tz_step=8, tiles=1458, splits=23, slots=183 + 23, ranges="count")
    with _Env(monkeypatch, PPP_RANK_WG_TILE="8x16x16"):
        assert backend.rank_wg_plan(_plan_params((140, 140, 140), (7, 7, 7)), None, 5, 32)["tile"] == (8, 16, 16)
    with _Env(monkeypatch):
        Pv = _plan_params((140, 140, 140), (7, 7, 7))
        Pv.rank_tile = 2
        assert backend.rank_wg_plan(Pv, None, 5, 32) == dict(tile=(8, 16, 16), tz_step=8, tiles=1458, splits=0, slots=183, ranges="count")
