"""The cubic instantiation of the per-patch S5 kernels (csrc/ppp_patch_graph_pa.hip, PaGeo: the
window's sizes compiled in for p^3 windows, p = 3, 5, 7, 9) against the run-time instantiation
(forced with PPP_PA_CUBE=0) and the oracle's patch graph: aff as uint32 bit patterns, all three
equal.  Which instantiation served a call is read from ppp_patch_graph_kernel_geometry.

Inputs: synthetic predictions from the package's generator with a cell as wide as the patch, on the
smallest volumes that hold the cases (16^3 for 3^3 and 5^3, 24^3 for 7^3, 28^3 for 9^3); hand-built
pair lists, one patch A per row count of ROW_COUNTS with partners drawn from the interior centres
with x >= A.x at most 2 (p - 1) away on every axis.  Asserted on the list before anything runs on
the GPU: a patch with more rows than the larger workgroup serves, pairs with intersecting windows
and pairs apart, a pair at the largest offset |d| = 2 p - 2.

Every width's consensus row ends in a partial staging trip for both workgroup sizes (125 = 64 + 61,
729 = 11 * 64 + 25, 2197 = 34 * 64 + 21 = 8 * 256 + 149, 4913 = 38 * 128 + 49 = 19 * 256 + 49): the
cubic kernel tests only that trip, so equality with the oracle covers the tail.

The calls go through backend.patch_graph_prepare / patch_graph_by_patch -- the path the pipeline
takes -- with its switches: both workgroup sizes (PPP_PA_CHUNK), the patches' foreground bits from
the table or built in the kernel (PPP_PA_BITS), thinning masks for every intersecting row, for none
(the kernel runs the generator) and for the first batch only (PPP_PA_LCG_BYTES /
PPP_PA_LCG_BATCHES: the rows beyond the mask budget run the generator)."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

ROW_COUNTS = (300, 70, 40, 10)
# patch shape, volume, seed
CUBES = {3: ((3, 3, 3), (16, 16, 16), 21), 5: ((5, 5, 5), (16, 16, 16), 22), 7: ((7, 7, 7), (24, 24, 24), 23),
         9: ((9, 9, 9), (28, 28, 28), 24)}
# windows a PX = 7 case serves that are no cube: they keep the run-time instantiation
OTHERS = {"p577": ((5, 7, 7), (14, 20, 22), 25), "p177": ((1, 7, 7), (3, 24, 28), 26)}
OTHER_ROW_COUNTS = (70, 20, 5)
SWITCHES = ("PPP_PA_CUBE", "PPP_PA_CHUNK", "PPP_PA_BITS", "PPP_PA_LCG_BYTES", "PPP_PA_LCG_BATCHES")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert backend.device_count() >= 1
    return torch


@contextlib.contextmanager
def _env(**kw):
    """development switches for the calls inside; unset again (and read again) afterwards"""
    from patchperpix_amd import backend
    before = {k: os.environ.pop(k, None) for k in SWITCHES}
    try:
        os.environ.update({k: str(v) for k, v in kw.items()})
        backend.reload_env()
        yield
    finally:
        for k, v in before.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        backend.reload_env()


def pair_rows(shape, ps, counts, rng):
    """[n, 6] int32: for every count one patch A with that many partners; the first A sits in the
    middle of the volume in z and y, so that offsets up to the largest occur on both sides"""
    rad = [p // 2 for p in ps]
    reach = [2 * (p - 1) for p in ps]
    zz, yy, xx = np.meshgrid(*[np.arange(rad[k], shape[k] - rad[k]) for k in range(3)], indexing="ij")
    centres = np.stack([zz.ravel(), yy.ravel(), xx.ravel()], axis=1)
    low = centres[centres[:, 2] < rad[2] + 2]
    mid = np.array([shape[0] // 2, shape[1] // 2, rad[2]])
    others = low[np.any(low != mid, axis=1)]
    A_all = np.concatenate([mid[None], others[rng.choice(len(others), size=len(counts) - 1, replace=False)]])
    rows = []
    for A, n in zip(A_all, counts):
        d = centres - A
        ok = (np.abs(d[:, 0]) <= reach[0]) & (np.abs(d[:, 1]) <= reach[1]) & (d[:, 2] >= 0) & \
            (d[:, 2] <= reach[2]) & np.any(d != 0, axis=1)
        cand = centres[ok]
        assert len(cand) >= n, (A, len(cand))
        B = cand[rng.choice(len(cand), size=n, replace=False)]
        rows.append(np.concatenate([np.broadcast_to(A, B.shape), B], axis=1))
    rows = np.concatenate(rows).astype(np.int32)
    return rows[rng.permutation(len(rows))]          # the caller's row order is arbitrary


def list_properties(rows, ps):
    """what the tests require of a pair list (host arithmetic only)"""
    d = rows[:, 3:] - rows[:, :3]
    inter = np.all(np.abs(d) < np.array(ps), axis=1)
    _, counts = np.unique(rows[:, :3], axis=0, return_counts=True)
    return dict(largest_group=int(counts.max()), intersecting=int(inter.sum()), apart=int((~inter).sum()),
                at_largest_offset=int(np.any(np.abs(d) == 2 * (np.array(ps) - 1), axis=1).sum()))


def mask_budget_for_first_group(rows, ps, P):
    """PPP_PA_LCG_BYTES with which the plan of backend._lcg_plan puts the first group (patches A in
    order of their linear index) into its first batch and the others behind it: the window of a
    batch is the budget less the largest group's words"""
    from patchperpix_amd import backend
    d = rows[:, 3:] - rows[:, :3]
    words = np.asarray(backend.lcg_words(d[:, 0], d[:, 1], d[:, 2], P)).astype(np.int64)
    lin = (rows[:, 0].astype(np.int64) * P.Y + rows[:, 1]) * P.X + rows[:, 2]
    groups = np.unique(lin)
    g_words = np.array([words[lin == g].sum() for g in groups])
    assert g_words[0] > 0 and g_words[1:].sum() > 0
    return 8 * int(g_words[0] + g_words.max())


class _Case:
    """prediction, consensus, pair rows and the oracle's aff of one patch shape: made once"""

    def __init__(self, torch, ps, shape, seed, counts):
        from oracle import ppp_oracle as orc
        from patchperpix_amd import backend, synth
        from tests_flags import FLYLIGHT
        self.ps, self.shape = ps, shape
        kw = dict(FLYLIGHT)
        rng = np.random.default_rng(seed)
        self.rows = rows = pair_rows(shape, ps, counts, rng)
        self.props = list_properties(rows, ps)
        pred = synth.make_case(shape, ps, seed=seed, cell=[max(p, 2) for p in ps], noise=0.3)["pred"]
        assert np.array_equal(pred.astype(np.float16).astype(np.float32), pred)    # float16 sees the same values
        self.P = P = backend.make_params(shape, ps, **kw)
        self.cut_bytes = mask_budget_for_first_group(rows, ps, P)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
        self.pred32, self.pred16 = dev(pred), dev(pred.astype(np.float16))
        self.rows_d = dev(rows)
        cons = backend.consensus(self.pred32, torch.zeros(shape, dtype=torch.uint8, device="cuda"), P)
        self.vm, self.Pv = backend.cons_to_voxel_major(cons, P)
        cons_ref = backend.cons_to_reference(cons, P).cpu().numpy()
        del cons
        self.want = orc.patch_graph(pred, cons_ref, rows.view(np.uint32), ps, **kw).view(np.uint32)
        del cons_ref

    def run(self, torch, pred, cube, chunk, table, masks):
        """(aff bits, geometry reported, job) of one pass through the per-patch path"""
        from patchperpix_amd import backend
        env = {"PPP_PA_CHUNK": chunk, "PPP_PA_BITS": "1" if table else "0"}
        if not cube:
            env["PPP_PA_CUBE"] = "0"
        if masks == "none":
            env["PPP_PA_LCG_BYTES"] = "0"
        elif masks == "cut":
            env.update(PPP_PA_LCG_BYTES=self.cut_bytes, PPP_PA_LCG_BATCHES=1)
        with _env(**env):
            job = backend.patch_graph_prepare(pred, self.rows_d, self.Pv)
            aff = backend.patch_graph_by_patch(pred, self.vm, self.rows_d, self.Pv, job=job)
            torch.cuda.synchronize()
            geometry = backend.lib().ppp_patch_graph_kernel_geometry().decode()
        return aff.cpu().numpy().view(np.uint32), geometry, job


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    _CASES.clear()


def _case(torch, key):
    if key not in _CASES:
        _CASES.clear()                                   # (one at a time: a 9^3 consensus is 0.4 GB)
        if key in CUBES:
            _CASES[key] = _Case(torch, *CUBES[key], ROW_COUNTS)
        else:
            _CASES[key] = _Case(torch, *OTHERS[key], OTHER_ROW_COUNTS)
    return _CASES[key]


def _check_plan(case, job, masks):
    """the thinning masks the pass was meant to run with"""
    if masks == "none":
        assert job.plan is None
        return
    served = int((job.plan["drop_off"] >= 0).sum().item())
    if masks == "all":
        assert served == case.props["intersecting"]
    else:
        assert 0 < served < case.props["intersecting"]   # the rest: the generator inside the kernel


@pytest.mark.parametrize("p", sorted(CUBES))
def test_pair_lists_hold_the_cases(p):
    """host arithmetic only: what the comparison below relies on"""
    ps, shape, seed = CUBES[p]
    props = list_properties(pair_rows(shape, ps, ROW_COUNTS, np.random.default_rng(seed)), ps)
    assert props["largest_group"] > 256                  # more rows than the larger workgroup serves
    assert props["intersecting"] >= 30 and props["apart"] >= 30
    assert props["at_largest_offset"] >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("p", sorted(CUBES))
def test_cubic_equals_generic_equals_oracle(p, torch_cuda):
    from patchperpix_amd import backend
    torch = torch_cuda
    case = _case(torch, p)
    props = case.props
    small = int(backend.lib().ppp_patch_graph_by_patch_chunk_small(ctypes.byref(case.Pv)))
    wide = int(backend.lib().ppp_patch_graph_by_patch_chunk(ctypes.byref(case.Pv)))
    assert 0 < small < wide < props["largest_group"]
    assert props["intersecting"] >= 30 and props["apart"] >= 30 and props["at_largest_offset"] >= 1
    assert np.count_nonzero(case.want) > 50
    passes = [(case.pred32, chunk, table, masks) for chunk in ("small", "big") for table in (True, False)
              for masks in ("all", "cut", "none")]
    passes += [(case.pred16, chunk, True, "all") for chunk in ("small", "big")]
    for pred, chunk, table, masks in passes:
        what = (p, str(pred.dtype), chunk, table, masks)
        got_c, geo_c, job = case.run(torch, pred, True, chunk, table, masks)
        assert geo_c == "cube", what
        assert job.chunk == (small if chunk == "small" else wide) and (job.bits is not None) == table, what
        _check_plan(case, job, masks)
        got_g, geo_g, _ = case.run(torch, pred, False, chunk, table, masks)
        assert geo_g == "generic", what
        bad = np.nonzero(got_c != case.want)[0]
        assert bad.size == 0, (what, "cubic differs from the oracle", bad[:8], case.rows[bad[:8]])
        bad = np.nonzero(got_g != case.want)[0]
        assert bad.size == 0, (what, "generic differs from the oracle", bad[:8], case.rows[bad[:8]])
        assert np.array_equal(got_c, got_g), what


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(OTHERS))
def test_other_windows_keep_the_generic_instantiation(key, torch_cuda):
    torch = torch_cuda
    case = _case(torch, key)
    assert case.props["intersecting"] >= 5 and case.props["apart"] >= 5
    assert np.count_nonzero(case.want) > 10
    for chunk in ("small", "big"):
        for table in (True, False):
            for masks in ("all", "none"):
                got, geometry, job = case.run(torch, case.pred32, True, chunk, table, masks)
                assert geometry == "generic", (key, chunk, table, masks)
                _check_plan(case, job, masks)
                assert np.array_equal(got, case.want), (key, chunk, table, masks)
