"""The 7^3 ranking kernel of run-time tile thickness (ppp_rank_wg.hip) with its LDS arrays sized by the thickness
the launch uses.

GPU: scores as uint32 bit patterns against the one-wave kernel of ppp_rank_vm.hip (PPP_RANK_WG=0), no tolerance,
under every forced z step whose LDS size or carve-up differs (PPP_RANK_WG_TZ = 8, 9, 10, 11, 12, 16), on volumes
whose y / x extents of 17 and 33 leave a ragged tile of one line, with a background slab (empty tiles, inactive
centres), for the whole volume (z extent 24 / 27: not a multiple of most steps) and for score boxes 7 and 13 slices
thick (one z-tile; two z-tiles with a ragged second one).  5^3 and 9^3 keep their launches.

CPU: the plan (ppp_rank_wg_plan / ppp_rank_wg_plan_residency with a residency and the CUs of an XCD given: no
device is asked) for 5, 6 and 7 workgroups per CU at 140^3, 96^3 and 64^3."""
import numpy as np
import pytest

SWITCHES = ("PPP_RANK_WG_TILE", "PPP_RANK_WG_SPLIT", "PPP_RANK_WG_TZ", "PPP_RANK_WG_XCD", "PPP_RANK_ORDER",
            "PPP_RANK_TILE_MAJOR", "PPP_RANK_WG")
# (z, y, x): y / x extents of 33 and 17 -- 16 + 1 and 2 x 16 + 1 lines
VOLUMES = {"y33x17": (24, 33, 17), "y17x33": (27, 17, 33)}
LDS_PER_CU = 160 * 1024


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


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert backend.device_count() >= 1
    return torch


def _build(torch, shape, ps, cell, monkeypatch_cls):
    """synthetic cells with a background slab over the upper third in y; the voxel-major consensus of the whole
    volume; the one-wave kernel's scores for the whole volume (computed once, read-only afterwards)"""
    from patchperpix_amd import backend, synth
    from tests_flags import FLYLIGHT
    c = synth.make_case(shape, ps, seed=31, cell=[cell] * 3, overlap_frac=0.03)
    p = c["pred"].astype(np.float16)
    p[:, :, shape[1] - shape[1] // 3:, :4] = 0      # (background: x < 4 of the upper third in y)
    p[:, : shape[0] // 4, : shape[1] // 2, :] = 0   # (... and the lower half in y of the first quarter in z)
    P = backend.make_params(shape, ps, **dict(FLYLIGHT))
    pred = torch.from_numpy(p).cuda()
    ov = torch.from_numpy((c["numinst"] > 1).astype(np.uint8)).cuda()
    vm, Pv = backend.cons_to_voxel_major(backend.consensus(pred, ov, P), P)
    mp = monkeypatch_cls()
    with _Env(mp, PPP_RANK_WG="0"):
        want = backend.rank_patches(pred, vm, ov, Pv).cpu().numpy()
        assert backend.lib().ppp_rank_kernel_name().decode() == "rank_vm_kernel"
    want.setflags(write=False)
    assert (want > 0).sum() > 100
    return dict(pred=pred, ov=ov, vm=vm, Pv=Pv, want=want, shape=shape)


@pytest.fixture(scope="module", params=sorted(VOLUMES))
def case7(request, torch_cuda):
    return _build(torch_cuda, VOLUMES[request.param], (7, 7, 7), 9, pytest.MonkeyPatch)


@pytest.fixture(scope="module", params=[5, 9])
def case59(request, torch_cuda):
    p = request.param
    return _build(torch_cuda, (24, 33, 40), (p, p, p), 9, pytest.MonkeyPatch)


def _bits_equal(case, score_box=None):
    from patchperpix_amd import backend
    got = backend.rank_patches(case["pred"], case["vm"], case["ov"], case["Pv"], score_box=score_box).cpu().numpy()
    assert backend.lib().ppp_rank_kernel_name().decode() == "rank_wg_kernel"
    sl = tuple(slice(None) for _ in range(3)) if score_box is None else tuple(slice(score_box[i], score_box[i + 3]) for i in range(3))
    assert np.array_equal(got[sl].view(np.uint32), case["want"][sl].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("tz", [8, 9, 10, 11, 12, 16])
def test_forced_z_step_bits(case7, tz, monkeypatch):
    from patchperpix_amd import backend
    Z, Y, X = case7["shape"]
    with _Env(monkeypatch, PPP_RANK_WG_TZ=str(tz)):
        plan = backend.rank_wg_plan(case7["Pv"])
        res = backend.rank_wg_plan_residency(case7["Pv"])
        assert plan["tz_step"] == tz and plan["tiles"] == -(-Z // tz) * -(-Y // 16) * -(-X // 16)
        # the LDS arrays are sized by the smallest of 8 / 10 / 12 / 16 that holds the step, and the device holds
        # what the plan says it holds
        assert res["lds_tz"] == min(t for t in (8, 10, 12, 16) if t >= tz)
        assert 1 <= res["resident"] <= LDS_PER_CU // res["lds_bytes"]
        _bits_equal(case7)                                   # z extent 24 / 27: ragged last z-tile for most steps
        _bits_equal(case7, (3, 0, 0, 10, Y, X))              # 7 slices: one z-tile, thinner than every step
        _bits_equal(case7, (4, 2, 1, 17, Y - 1, X))          # 13 slices: two z-tiles with a ragged second one (one at 16)


@pytest.mark.gpu
def test_forced_z_step_with_ranges_by_weight_and_splits(case7, monkeypatch):
    with _Env(monkeypatch, PPP_RANK_WG_TZ="9", PPP_RANK_WG_XCD="weight", PPP_RANK_WG_SPLIT="2"):
        _bits_equal(case7)


@pytest.mark.gpu
def test_other_sizes_keep_their_launch(case59, monkeypatch):
    from patchperpix_amd import backend
    with _Env(monkeypatch):
        plan = backend.rank_wg_plan(case59["Pv"])
        res = backend.rank_wg_plan_residency(case59["Pv"])
        assert plan["tile"] == (8, 8, 16) and plan["tz_step"] == 8 and res["lds_tz"] == 8
        _bits_equal(case59)
    with _Env(monkeypatch, PPP_RANK_WG_TZ="10"):            # (7^3 only: ignored here)
        assert backend.rank_wg_plan(case59["Pv"]) == plan
        assert backend.rank_wg_plan_residency(case59["Pv"]) == res


# ---- the plan, without a device ----------------------------------------------------------------------------------
def _plan_params(shape, p):
    from patchperpix_amd import backend
    from tests_flags import FLYLIGHT
    P = backend.make_params(shape, (p, p, p), **dict(FLYLIGHT))
    Pv = P.copy()
    Pv.cons_layout = backend.CONS_VOXEL_MAJOR
    return Pv


def _cdiv(a, b):
    return -(-a // b)


def _lds_floor(tz):
    """what the 7^3 kernel of tiles tz x 16 x 16 keeps in LDS, from its arrays: the row image of 13^3 floats, the
    coefficient table of 256 x 8 B, per slice of the tile 256 float accumulators and 256 activity bits, one validity
    bit per voxel of the tile grown by the radius -- a lower bound (padding and alignment come on top)"""
    return 4 * 13 ** 3 + 2048 + tz * (1024 + 32) + (tz + 6) * 22 * 22 // 8


@pytest.fixture
def no_switches(monkeypatch):
    from patchperpix_amd import backend
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    backend.reload_env()
    yield
    monkeypatch.undo()
    backend.reload_env()


@pytest.mark.parametrize("resident", [5, 6, 7])
@pytest.mark.parametrize("n", [140, 96, 64])
def test_plan_by_residency(no_switches, n, resident):
    from patchperpix_amd import backend
    cus = 32
    Pv = _plan_params((n, n, n), 7)
    plan = backend.rank_wg_plan(Pv, None, resident, cus)
    res = backend.rank_wg_plan_residency(Pv, None, resident, cus)
    assert res["cus_per_xcd"] == cus and 1 <= res["resident"] <= resident
    assert res["lds_bytes"] * res["resident"] <= LDS_PER_CU
    # the rule: a launch that 8 x 16 x 16 tiles put between one and two rounds of `resident` workgroups per CU takes
    # the smallest z step in 8 .. 16 whose tiles fit one round of the workgroups a CU holds AT THAT THICKNESS
    per0 = _cdiv(_cdiv(n, 8) * _cdiv(n, 16) * _cdiv(n, 16), 8)
    big = _cdiv(n, 8) * _cdiv(n, 16) * _cdiv(n, 16) >= 1024
    between = big and resident * cus < per0 < 2 * resident * cus
    if between:
        assert plan["tile"] == (16, 16, 16) and plan["splits"] == 0 and plan["ranges"] == "weight"
        t = plan["tz_step"]
        assert 8 <= t <= 16 and res["lds_tz"] == min(z for z in (8, 10, 12, 16) if z >= t)
        assert _lds_floor(res["lds_tz"]) <= res["lds_bytes"] <= _lds_floor(res["lds_tz"]) + 256
        per = _cdiv(plan["tiles"], 8)
        assert plan["tiles"] == _cdiv(n, t) * _cdiv(n, 16) ** 2 and per <= res["resident"] * cus      # fits one round
        # ... and no thinner tile does, under the residency its own LDS size allows
        for t2 in range(8, t):
            lds_tz2 = min(z for z in (8, 10, 12, 16) if z >= t2)
            slots2 = min(resident, LDS_PER_CU // _lds_floor(lds_tz2)) * cus
            assert _cdiv(_cdiv(n, t2) * _cdiv(n, 16) ** 2, 8) > slots2, t2
    else:
        # nothing to fit: today's plan exists as before (8 x 16 x 16 from 1 024 such tiles on, else 8 x 8 x 16)
        ty = 16 if big else 8
        assert plan["tile"] == (8, ty, 16) and plan["tz_step"] == 8 and plan["ranges"] == "count"
        assert plan["tiles"] == _cdiv(n, 8) * _cdiv(n, ty) * _cdiv(n, 16) and res["lds_tz"] == 8
        assert plan["slots"] == _cdiv(plan["tiles"], 8) + plan["splits"]


def test_plan_140_cases(no_switches):
    """the default benchmark's launch (140^3 centres): 183 tiles of 8 x 16 x 16 per XCD"""
    from patchperpix_amd import backend
    Pv = _plan_params((140, 140, 140), 7)
    # five per CU (160 slots): z step 10 (142 per XCD), LDS sized for 10 slices
    assert backend.rank_wg_plan(Pv, None, 5, 32)["tz_step"] == 10
    r = backend.rank_wg_plan_residency(Pv, None, 5, 32)
    assert r["lds_tz"] == 10 and r["resident"] == 5 and 22000 < r["lds_bytes"] <= LDS_PER_CU // 7
    # four per CU (128 slots): z step 12 (122 per XCD); LDS sized for 12 slices still holds six
    assert backend.rank_wg_plan(Pv, None, 4, 32)["tz_step"] == 12
    assert LDS_PER_CU // backend.rank_wg_plan_residency(Pv, None, 4, 32)["lds_bytes"] == 6
    # three per CU (96 slots): nothing up to z step 16 (92 per XCD) ... fits; two per CU: a plan exists all the same
    assert backend.rank_wg_plan(Pv, None, 3, 32)["tz_step"] == 16
    assert backend.rank_wg_plan(Pv, None, 2, 32)["tiles"] > 0
    # six and seven per CU hold all 183 tiles of 8 x 16 x 16 in one round: the launch is not between one and two rounds
    for resident in (6, 7):
        assert backend.rank_wg_plan(Pv, None, resident, 32)["tile"] == (8, 16, 16)
