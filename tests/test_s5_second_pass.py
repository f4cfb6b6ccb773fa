"""(The file keeps the name it was planned under: the second pass of a wave over the rows 65.. of a
patch was measured slower and is not in the tree -- header of csrc/ppp_patch_graph_pa.hip.  What
it pins is what that work changed or could have broken.)

The per-patch S5 kernel (ppp_patch_graph_by_patch_lcg, csrc/ppp_patch_graph_pa.hip) on groups
whose row counts sit on both sides of what one wave and one workgroup serve: a patch with 1, 63,
64, 65, 127, 128, 129 and 200 pair rows, through the small (one- or two-wave) kernel and the
256-thread one -- a partly filled wave, a full one, rows that spill into a second wave or a
further workgroup.  At 7^3 the small kernel adds the staged values of a candidate row under a
lane mask (PA_EXEC_ADD): every row here goes through that form.  Every kernel runs twice:
with the patches' foreground bits built inside it (ppp_patch_graph_by_patch_lcg) and read from
the table made once per patch (ppp_patch_fg_bits + ppp_patch_graph_by_patch_bits); the table
itself is compared with the expression in NumPy for every interior centre of a volume.

Hand-built pair lists on small random volumes (about 70 % foreground): one patch A per row
count, partners = interior centres with x >= A.x at most 2 (p - 1) away on every axis, so
intersecting windows, windows apart and offsets next to PPP_PAIR_KEY_FAR all occur.  The groups,
chunks and thinning masks are made here, through the C ABI, the way backend.patch_graph_prepare
makes them: with masks for every intersecting row, for none (d_drop_off NULL: the kernel runs the
generator itself) and for a mask budget that ends in the middle of a group.

aff is compared as uint32 bit patterns with ppp_patch_graph (a lane per pair: independent code)
and with the oracle's ppp_oracle_patch_graph: tolerance 0."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROW_COUNTS = (1, 63, 64, 65, 127, 128, 129, 200)
# shape, patch shape, seed: the smallest volumes whose interior holds 200 partners with x >= A.x
# (9^3: 20 x 20 x 30 -- its interior of 12 x 12 x 22 centres holds them; a larger volume only makes the
# consensus handed to the oracle larger, 18^3 floats per voxel)
CASES = [((14, 14, 24), (5, 5, 5), 11), ((20, 20, 34), (7, 7, 7), 12), ((20, 20, 30), (9, 9, 9), 13)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert backend.device_count() >= 1
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pair_rows(shape, ps, rng):
    """[n, 6] int32: for every count in ROW_COUNTS one patch A with that many partners"""
    rad = [p // 2 for p in ps]
    reach = [2 * (p - 1) for p in ps]
    zz, yy, xx = np.meshgrid(*[np.arange(rad[k], shape[k] - rad[k]) for k in range(3)], indexing="ij")
    centres = np.stack([zz.ravel(), yy.ravel(), xx.ravel()], axis=1)
    # patches A: low x (room for partners with x >= A.x), anywhere in z and y -- the interior's
    # border included
    low = centres[centres[:, 2] < rad[2] + 3]
    A_all = low[rng.choice(len(low), size=len(ROW_COUNTS), replace=False)]
    rows = []
    for A, n in zip(A_all, ROW_COUNTS):
        d = centres - A
        ok = (np.abs(d[:, 0]) <= reach[0]) & (np.abs(d[:, 1]) <= reach[1]) & (d[:, 2] >= 0) & \
            (d[:, 2] <= reach[2]) & np.any(d != 0, axis=1)
        cand = centres[ok]
        assert len(cand) >= n, (A, len(cand))
        B = cand[rng.choice(len(cand), size=n, replace=False)]
        rows.append(np.concatenate([np.broadcast_to(A, B.shape), B], axis=1))
    rows = np.concatenate(rows).astype(np.int32)
    return rows[rng.permutation(len(rows))]          # the caller's row order is arbitrary


class _Case:
    """prediction, consensus, pair rows, groups and the two references of one patch shape: made
    once, shared by the tests"""

    def __init__(self, torch, shape, ps, seed):
        from oracle import ppp_oracle as orc
        from patchperpix_amd import backend
        from tests_flags import FLYLIGHT
        self.ps = ps
        rng = np.random.default_rng(seed)
        C = ps[0] * ps[1] * ps[2]
        # float16-representable values: the float16 and the float32 kernels see the same numbers
        pred = rng.random((C,) + shape, dtype=np.float32).astype(np.float16).astype(np.float32)
        pred[C // 2] = (rng.random(shape) < 0.7).astype(np.float32)      # the foreground channel
        kw = dict(FLYLIGHT)
        self.P = P = backend.make_params(shape, ps, **kw)
        self.pred32 = _dev(torch, pred)
        self.pred16 = _dev(torch, pred.astype(np.float16))
        cons = backend.consensus(self.pred32, torch.zeros(shape, dtype=torch.uint8, device="cuda"), P)
        self.vm, self.Pv = backend.cons_to_voxel_major(cons, P)
        rows = _pair_rows(shape, ps, rng)
        self.rows = rows
        self.rows_d = _dev(torch, rows)
        d = rows[:, 3:] - rows[:, :3]
        inter = np.all(np.abs(d) < np.array(ps), axis=1)
        assert inter.any() and (~inter).any()
        assert any(np.any(np.abs(d[:, k]) == 2 * (ps[k] - 1)) for k in range(3))   # next to KEY_FAR
        # reference 1: a lane per pair
        self.want = backend.patch_graph(self.pred32, cons, self.rows_d, P).cpu().numpy().view(np.uint32)
        # reference 2: the oracle, on the same consensus in the reference's layout
        cons_ref = backend.cons_to_reference(cons, P).cpu().numpy()
        del cons
        aff_o = orc.patch_graph(pred, cons_ref, rows.view(np.uint32), ps, **kw)
        del cons_ref
        self.want_oracle = aff_o.view(np.uint32)
        assert np.count_nonzero(self.want) > 50
        # the groups: rows sorted by (patch A, windows apart, offset)
        n = len(rows)
        keys = torch.empty((n,), dtype=torch.int64, device="cuda")
        backend.check(backend.lib().ppp_pair_group_keys(backend._dev_ptr(self.rows_d), n, backend._dev_ptr(keys),
                                                        ctypes.byref(self.Pv), backend._stream()))
        keys, order = torch.sort(keys)
        keys, order = keys.cpu().numpy(), order.cpu().numpy()
        assert keys[-1] != backend.PAIR_KEY_FAR                           # every row is dispatched
        _, counts = np.unique(keys >> 18, return_counts=True)
        assert sorted(counts.tolist()) == sorted(ROW_COUNTS)
        self.order = order.astype(np.int32)
        self.counts = counts
        self.group_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        ds = d[order]
        self.words = np.asarray(backend.lcg_words(ds[:, 0], ds[:, 1], ds[:, 2], P)).astype(np.int64)

    def run(self, torch, pred, chunk, masks, table):
        """aff bits of the per-patch kernel with `chunk` rows per workgroup.  masks: 'all', 'none'
        or 'cut' = the mask budget ends in the middle of the largest group.  table: the patches'
        foreground bits from ppp_patch_fg_bits instead of built inside the kernel"""
        from patchperpix_amd import backend
        L, ptr = backend.lib(), backend._dev_ptr
        n = len(self.rows)
        order_d = _dev(torch, self.order)
        gs_d = _dev(torch, self.group_start)
        blocks = (self.counts + chunk - 1) // chunk
        co_d = _dev(torch, np.concatenate([[0], np.cumsum(blocks)]).astype(np.int64))
        off_d = drops = None
        if masks != "none":
            served = self.words > 0
            if masks == "cut":
                # (inside a group the rows with intersecting windows come first)
                g = int(np.argmax(self.counts))
                g0, g1 = int(self.group_start[g]), int(self.group_start[g + 1])
                cut = g0 + int(served[g0:g1].sum()) // 2
                assert cut > g0 and served[cut - 1] and served[cut]
                served = served & (np.arange(n) < cut)
            w = np.where(served, self.words, 0)
            off = np.where(served, np.cumsum(w) - w, -1).astype(np.int64)
            pos = np.nonzero(served)[0].astype(np.int64)
            off_d, pos_d = _dev(torch, off), _dev(torch, pos)
            drops = torch.zeros((max(int(w.sum()), 1),), dtype=torch.int64, device="cuda")
            backend.check(L.ppp_patch_graph_lcg(
                ptr(pred), backend.pred_dtype_code(pred), ptr(self.rows_d), ptr(order_d), ptr(pos_d), len(pos),
                ptr(off_d), ptr(drops), ctypes.byref(self.Pv), backend._stream()))
        aff = torch.zeros((n,), dtype=torch.float32, device="cuda")
        if table:
            centres, bits = backend.patch_fg_bits(pred, self.rows_d, self.Pv)
            backend.check(L.ppp_patch_graph_by_patch_bits(
                ptr(pred), backend.pred_dtype_code(pred), ptr(self.vm), ptr(self.rows_d), ptr(order_d), ptr(gs_d),
                ptr(co_d), len(self.counts), int(blocks.sum()), chunk, ptr(aff), ptr(off_d), ptr(drops),
                ptr(centres), int(centres.shape[0]), ptr(bits), 0, ctypes.byref(self.Pv), backend._stream()))
        else:
            backend.check(L.ppp_patch_graph_by_patch_lcg(
                ptr(pred), backend.pred_dtype_code(pred), ptr(self.vm), ptr(self.rows_d), ptr(order_d), ptr(gs_d),
                ptr(co_d), len(self.counts), int(blocks.sum()), chunk, ptr(aff), ptr(off_d), ptr(drops),
                ctypes.byref(self.Pv), backend._stream()))
        torch.cuda.synchronize()
        return aff.cpu().numpy().view(np.uint32)


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    _CASES.clear()


@pytest.fixture
def case(request, torch_cuda):
    i = request.param
    if i not in _CASES:
        _CASES[i] = _Case(torch_cuda, *CASES[i])
    return _CASES[i]


@pytest.mark.parametrize("case", range(len(CASES)), indirect=True)
def test_references_agree(case):
    """the pair-per-lane kernel and the oracle, before either is used as a reference"""
    assert np.array_equal(case.want, case.want_oracle)


@pytest.mark.parametrize("masks", ["all", "none", "cut"])
@pytest.mark.parametrize("case", range(len(CASES)), indirect=True)
def test_row_counts_around_a_workgroup(case, masks, torch_cuda):
    from patchperpix_amd import backend
    small = int(backend.lib().ppp_patch_graph_by_patch_chunk_small(ctypes.byref(case.Pv)))
    wide = int(backend.lib().ppp_patch_graph_by_patch_chunk(ctypes.byref(case.Pv)))
    assert 0 < small < wide
    for chunk in (small, wide):
        for pred in (case.pred16, case.pred32):
            for table in (False, True):
                got = case.run(torch_cuda, pred, chunk, masks, table)
                bad = np.nonzero(got != case.want)[0]
                assert bad.size == 0, (chunk, str(pred.dtype), masks, table, bad[:8], case.rows[bad[:8]])
                assert np.array_equal(got, case.want_oracle)


@pytest.mark.parametrize("shape,ps,seed", CASES[:2])
def test_foreground_bits_table_equals_the_expression(shape, ps, seed, torch_cuda):
    """ppp_patch_fg_bits for EVERY interior centre of the volume (those on the interior's border
    included), a patch without a foreground pixel and one with all among them, against
    bit r = mid[u_r] > th and pred[r][c] > th in NumPy."""
    torch = torch_cuda
    from patchperpix_amd import backend
    from tests_flags import FLYLIGHT
    rng = np.random.default_rng(seed + 100)
    C = ps[0] * ps[1] * ps[2]
    rad = [p // 2 for p in ps]
    pred = rng.random((C,) + shape, dtype=np.float32).astype(np.float16).astype(np.float32)
    pred[C // 2] = (rng.random(shape) < 0.7).astype(np.float32)
    c_all = tuple(rad)                                               # a corner of the interior
    c_none = tuple(shape[k] - rad[k] - 1 for k in range(3))          # the opposite corner
    pred[(slice(None),) + c_all] = 1.0
    pred[(C // 2,) + tuple(slice(c_all[k] - rad[k], c_all[k] + rad[k] + 1) for k in range(3))] = 1.0
    pred[(slice(None),) + c_none] = 0.0
    P = backend.make_params(shape, ps, **dict(FLYLIGHT))
    inner = tuple(slice(rad[k], shape[k] - rad[k]) for k in range(3))
    n_in = [shape[k] - 2 * rad[k] for k in range(3)]
    zz, yy, xx = np.meshgrid(*[np.arange(rad[k], shape[k] - rad[k]) for k in range(3)], indexing="ij")
    lin = ((zz * shape[1] + yy) * shape[2] + xx).ravel().astype(np.int64)          # ascending
    words = (C + 31) // 32
    want = np.zeros((len(lin), words), dtype=np.uint32)
    th = float(P.th)
    for r in range(C):
        rz, ry, rx = r // (ps[1] * ps[2]), (r // ps[2]) % ps[1], r % ps[2]
        mid = pred[C // 2, rz:rz + n_in[0], ry:ry + n_in[1], rx:rx + n_in[2]]      # u_r = c + r - rad
        on = (mid.astype(np.float64) > th) & (pred[(r,) + inner].astype(np.float64) > th)
        want[:, r >> 5] |= on.ravel().astype(np.uint32) << np.uint32(r & 31)
    i_all, i_none = 0, len(lin) - 1
    assert want[i_none].sum() == 0 and sum(bin(int(w)).count("1") for w in want[i_all]) == C
    for dt in (np.float32, np.float16):
        pred_d, lin_d = _dev(torch, pred.astype(dt)), _dev(torch, lin)
        bits = torch.zeros((len(lin), words), dtype=torch.int32, device="cuda")
        backend.check(backend.lib().ppp_patch_fg_bits(
            backend._dev_ptr(pred_d), backend.pred_dtype_code(pred_d), backend._dev_ptr(lin_d), len(lin),
            backend._dev_ptr(bits), ctypes.byref(P), backend._stream()))
        torch.cuda.synchronize()
        got = bits.cpu().numpy().view(np.uint32)
        bad = np.nonzero(np.any(got != want, axis=1))[0]
        assert bad.size == 0, (str(dt), bad[:8], got[bad[:4]], want[bad[:4]])
