"""The sweeps of a greedy-cover / thinning round (csrc/ppp_cover.hip) on their own.

The neighbourhood minimum has a kernel with compile-time radii for the cubic 3^3 .. 9^3 patches (tiles of
48 x 40 or 64 x 30 chosen from the slice extent) and a run-time kernel for every other shape; the count and
select sweeps handle several voxels per thread.  None of that may change what a round computes:

  * ppp_minfilter_xy against a NumPy sliding minimum ("none" outside the slice), on the slice extents at
    which the tiling has an edge: a single voxel, a slice smaller than every tile, one row / column past a
    tile, a last tile narrower than the radius, the benchmark's 140 x 140;
  * ppp_cover_pass / ppp_thin_cover against the sequential host loops (selection, running mask, cleared
    voxels, kept set) and against the one-shard step model of tests/shard_lockstep.py (state, cleared counts,
    mask, and the NUMBER OF ROUNDS, rounded up to the batch the host synchronises after: a step whose
    semantics moved -- a patch selected a round late, a rejection delayed -- changes the round count long
    before it changes a result).
All comparisons are exact."""
import ctypes

import numpy as np
import pytest

import shard_lockstep as ls

COVER_BATCH = 8                     # rounds per host synchronisation (ppp_cover.hip)
NONE = {np.dtype(np.int32): 0x7F7F7F7F, np.dtype(np.int64): 0x7F7F7F7F7F7F7F7F}

FILTER_SHAPES = [(1, 1, 1), (2, 3, 5), (3, 33, 65), (2, 12, 140), (1, 140, 140)]
CUBIC = [(3, 3, 3), (5, 5, 5), (7, 7, 7), (9, 9, 9)]
FALLBACK = [(3, 5, 7), (1, 25, 25)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert backend.device_count() >= 1
    return torch


def sliding_min_xy(a, ry, rx):
    """minimum over [y - ry, y + ry] x [x - rx, x + rx] of every slice, "none" outside the slice"""
    Z, Y, X = a.shape
    p = np.full((Z, Y + 2 * ry, X + 2 * rx), NONE[a.dtype], dtype=a.dtype)
    p[:, ry:ry + Y, rx:rx + X] = a
    m = p[:, :, 0:X].copy()
    for d in range(1, 2 * rx + 1):
        np.minimum(m, p[:, :, d:d + X], out=m)
    out = m[:, 0:Y].copy()
    for d in range(1, 2 * ry + 1):
        np.minimum(out, m[:, d:d + Y], out=out)
    return out


def filter_inputs(shape, seed):
    """(name, volume): int32 ranks (a permutation, as the rank volume holds them) with 0 / 50 / 97 % "none",
    int64 keys above 2^32 ((count part) << 32 | index, as the key volume holds them) likewise, all "none" """
    rs = np.random.RandomState(seed)
    n = int(np.prod(shape))
    for dtype in (np.int32, np.int64):
        for frac in (0.0, 0.5, 0.97):
            if dtype == np.int32:
                v = rs.permutation(n).astype(np.int32)
            else:
                v = (rs.randint(1, 1 << 20, size=n).astype(np.int64) << 32) | rs.permutation(n).astype(np.int64)
                assert v.min() >= 1 << 32
            v[rs.rand(n) < frac] = NONE[np.dtype(dtype)]
            yield "%s %d%% none" % (np.dtype(dtype).name, round(100 * frac)), v.reshape(shape)
        yield "%s all none" % np.dtype(dtype).name, np.full(shape, NONE[np.dtype(dtype)], dtype=dtype)


def device_minfilter_xy(torch, backend, a, ps):
    P = backend.make_params(a.shape, ps, **dict(ls.FLAGS))
    d_in = torch.from_numpy(a).cuda()
    keep = d_in.clone()
    out = torch.full_like(d_in, -1)                     # (no voxel may stay unwritten)
    scratch = torch.full_like(d_in, -1)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    backend.check(backend.lib().ppp_minfilter_xy(ptr(d_in), ptr(out), ptr(scratch), a.itemsize, ctypes.byref(P),
                                                 backend._stream()))
    torch.cuda.synchronize()
    assert torch.equal(d_in, keep), "the filter wrote its input"
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("ps", CUBIC + FALLBACK, ids=lambda p: "p%dx%dx%d" % tuple(p))
@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=lambda s: "%dx%dx%d" % tuple(s))
def test_minfilter_xy_equals_sliding_minimum(shape, ps, torch_cuda):
    from patchperpix_amd import backend
    for name, a in filter_inputs(shape, seed=7 + shape[2]):
        want = sliding_min_xy(a, ps[1] - 1, ps[2] - 1)
        got = device_minfilter_xy(torch_cuda, backend, a, ps)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, "%s: %d voxels differ, first (z, y, x) = %s: %d, expected %d" % (
            name, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


# ---- whole passes: the rounds compute what they computed -------------------------------------------------
# (p3x5x7: a non-cubic window; p1x11x11: the recount's row-by-row branch, py > 9; both straddle a mask word)
ROUND_CASES = {"p5": ((20, 12, 33), (5, 5, 5)), "p7": ((21, 13, 70), (7, 7, 7)),
               "p3x5x7": ((12, 20, 40), (3, 5, 7)), "p1x11x11": ((3, 40, 70), (1, 11, 11))}
PIX_THS = [10, 0]
_MODEL = {}


def model_of(name):
    """the case and its one-shard model runs (CPU), made once"""
    if name not in _MODEL:
        shape, ps = ROUND_CASES[name]
        case = ls.Case(shape, ps, seed=3)
        side = ls.ModelSide()
        whole = (0, shape[0])
        _MODEL[name] = (case, ls.run_cover(case, whole, [side], PIX_THS)["passes"],
                        ls.run_thin(case, whole, [side])["passes"][0], case.bits(side).numpy())
    return _MODEL[name]


def batches(rounds):
    return (rounds + COVER_BATCH - 1) // COVER_BATCH * COVER_BATCH


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROUND_CASES))
def test_cover_passes_equal_host_loop_and_step_model(name, torch_cuda):
    from patchperpix_amd import backend
    torch = torch_cuda
    case, model_passes, _, bits_h = model_of(name)
    P = case.params()
    bits_d = case.bits(ls.DeviceSide())
    assert np.array_equal(bits_d.cpu().numpy(), bits_h)
    bits_u = np.ascontiguousarray(bits_h).view(np.uint32)
    lin_d = torch.from_numpy(case.lin).cuda()
    mask_d = torch.from_numpy(case.mask.copy()).cuda()
    zeros8 = np.zeros(case.shape, dtype=np.uint8)
    score = np.zeros(case.n, dtype=np.float32)
    # the host loop twice: as the reference runs it (it stops when the interior is empty), and without its
    # stop rule -- what one device pass computes
    run_stop, _o1 = backend.padded_mask(case.mask)
    run_free, _o2 = backend.padded_mask(case.mask)
    sel_stop = np.zeros(case.n, dtype=np.uint8)
    selected = np.zeros(case.n, dtype=bool)
    remaining = case.interior
    assert len(model_passes) == len(PIX_THS), "the first pass emptied the interior: the case is too easy"
    for p, pix_th in enumerate(PIX_THS):
        model = model_passes[p]
        state_d = torch.from_numpy(selected.astype(np.int32)).cuda()
        cleared_d, rounds = backend.cover_pass_device(mask_d, bits_d, lin_d, state_d, pix_th, P)
        state, cleared = state_d.cpu().numpy(), cleared_d.cpu().numpy()
        print("%s pix_th %d: %d rounds (model %d), %d selected" % (name, pix_th, rounds, model["rounds"],
                                                                   int((state == 1).sum())))
        # the step model
        assert np.array_equal(state, model["state"]), "pass %d: state" % p
        assert np.array_equal(cleared, model["cleared"]), "pass %d: cleared interior voxels" % p
        assert np.array_equal(mask_d.cpu().numpy(), model["mask"]), "pass %d: running mask" % p
        assert rounds == batches(model["rounds"]), "pass %d: %d rounds, the model needs %d" % (p, rounds, model["rounds"])
        assert model["rounds"] > COVER_BATCH
        # the sequential loop without the stop rule: same selection, same mask, same number of cleared voxels
        sel_free = selected.astype(np.uint8)
        big = 1 << 40
        left, _ = backend.host_cover_pass(run_free, zeros8, case.ps, case.lin, score, bits_u, pix_th, None, sel_free, big)
        assert np.array_equal(sel_free != 0, state == 1), "pass %d: selection of the host loop" % p
        assert np.array_equal(run_free, mask_d.cpu().numpy()), "pass %d: mask of the host loop" % p
        new = (state == 1) & ~selected
        assert big - left == int(cleared[new].sum())
        # the loop's stop rule on the device's counts (rank order) against the loop that applies it itself
        remaining_h, _ = backend.host_cover_pass(run_stop, zeros8, case.ps, case.lin, score, bits_u, pix_th, None,
                                                 sel_stop, remaining)
        idx = np.flatnonzero(new)
        left = remaining - np.cumsum(cleared[idx])
        done = np.flatnonzero(left <= 0)
        if len(done):
            idx, remaining = idx[:done[0] + 1], 0
        elif len(idx):
            remaining = int(left[-1])
        selected[idx] = True
        assert np.array_equal(selected, sel_stop != 0), "pass %d: selection after the stop rule" % p
        assert max(remaining_h, 0) == remaining
        assert np.array_equal(selected, model["selected"])
        if remaining == 0:
            break
        assert np.array_equal(run_stop, run_free)
    assert selected.sum() > 30


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROUND_CASES))
def test_thinning_equals_host_loop_and_step_model(name, torch_cuda):
    from patchperpix_amd import backend
    torch = torch_cuda
    case, _, model, bits_h = model_of(name)
    P = case.params()
    bits_d = case.bits(ls.DeviceSide())
    mask_d = torch.from_numpy(case.mask.copy()).cuda()
    keep = backend.thin_cover_device(mask_d, bits_d, torch.from_numpy(case.lin).cuda(), P).cpu().numpy()
    rounds = int(backend.NOTES["thin_rounds"])
    print("%s thinning: %d rounds (model %d), %d of %d kept" % (name, rounds, model["rounds"], int(keep.sum()), case.n))
    assert np.array_equal(mask_d.cpu().numpy(), case.mask), "the thinning wrote the caller's mask"
    want = backend.host_thin_cover(case.mask, case.ps, case.lin, np.ascontiguousarray(bits_h).view(np.uint32))
    assert np.array_equal(keep, want), "kept set of the host loop"
    assert 0 < keep.sum() < case.n
    # the step model: its kept patches in the order the loop picks them (count descending, index ascending),
    # cut where the interior is empty
    kept = np.flatnonzero(model["state"] == 1)
    order = kept[np.lexsort((kept, -model["count"][kept]))]
    left = case.interior - np.cumsum(model["cleared"][order])
    done = np.flatnonzero(left <= 0)
    chosen = np.zeros(case.n, dtype=bool)
    chosen[order[:done[0] + 1] if len(done) else order] = True
    if not len(done):
        chosen[0] = True                                  # every count 0 with voxels left: np.argmax picks patch 0
    assert np.array_equal(keep, chosen), "kept set of the step model"
    assert rounds == batches(model["rounds"]), "%d rounds, the model needs %d" % (rounds, model["rounds"])
    assert model["rounds"] > COVER_BATCH
