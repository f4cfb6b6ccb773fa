"""GPU: the greedy cover's two optional branches, `mark_close_neighboorhood` (reference
foreground_cover.py:141-143, 162-168) and `select_patches_overlap_neighborhood` (:53-85), on the device
-- equal to the sequential host loop and to the oracle: coordinates, order and scores."""
import numpy as np
import pytest

import cover_marks_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert backend.device_count() >= 1
    return torch


def _cover(case, option, where, monkeypatch, torch):
    """computeForegroundCover of the case under PPP_COVER=where -> (coords, scores, notes)."""
    from patchperpix_amd import backend
    from patchperpix_amd.vote_instances import foreground_cover as fc
    from patchperpix_amd.vote_instances.ranked_patches import PatchList
    monkeypatch.setenv("PPP_COVER", where)
    backend.NOTES.pop("cover_rounds", None)
    backend.NOTES.pop("cover_cut", None)
    pred = torch.from_numpy(case.pred).cuda()
    ranked = PatchList(case.ranked_coords.copy(), case.ranked_scores.copy())
    sel, n = fc.computeForegroundCover(case.overlap_mask.copy(), case.mask_to_cover.copy(), case.ps, ranked,
                                       case.radslice, pred, case.rad, None, case.scores.copy(), silent=True,
                                       **case.flags(option))
    assert n == len(sel)
    return np.asarray(sel.coords).reshape(-1, 3), np.asarray(sel.scores), dict(backend.NOTES)


def _same(got, want):
    assert np.array_equal(got[0], np.asarray(want[0]).reshape(-1, 3))
    assert np.array_equal(np.asarray(got[1], dtype=np.float32), np.asarray(want[1], dtype=np.float32))


@pytest.mark.parametrize("option", ["mark", "ring", "both"])
@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_device_cover_equals_the_host_loop_and_the_oracle(name, option, torch_cuda, monkeypatch):
    case = cases.synthetic(name)
    want = case.oracle_cover(option)
    assert len(want[0]) > 0
    dev = _cover(case, option, "device", monkeypatch, torch_cuda)
    assert dev[2].get("cover_rounds", 0) > 0            # the rounds ran on the device ...
    host = _cover(case, option, "host", monkeypatch, torch_cuda)
    assert "cover_rounds" not in host[2]                # ... and PPP_COVER=host is still the loop
    _same(dev, want)
    _same(host, want)
    if option != "ring":
        # the flag is not a no-op
        plain = case.oracle_cover(None)
        assert not np.array_equal(np.asarray(want[0]), np.asarray(plain[0]))


def test_short_axis_keeps_the_host_loop(torch_cuda, monkeypatch):
    """Y < 7: the mark box's slice wraps to the far end of the axis -- the sequential loop's business."""
    case = cases.synthetic("W")
    got = _cover(case, "mark", "device", monkeypatch, torch_cuda)
    assert "cover_rounds" not in got[2]
    _same(got, case.oracle_cover("mark"))
    # the ring alone has no marks to wrap: on the device
    got = _cover(case, "ring", "device", monkeypatch, torch_cuda)
    assert got[2].get("cover_rounds", 0) > 0
    _same(got, case.oracle_cover("ring"))


def test_stop_rule_cut_before_the_ring_cover(torch_cuda, monkeypatch):
    """cover_marks_cases.stop_rule: the device pass selects a patch behind the point at which the
    sequential loop ends; its marks must not reach the ring cover's candidate."""
    case = cases.stop_rule()
    want = case.oracle_cover("both")
    assert [tuple(c) for c in want[0]] == [(0, 2, 22), (0, 4, 8), (0, 4, 22)]
    dev = _cover(case, "both", "device", monkeypatch, torch_cuda)
    assert dev[2]["cover_cut"] == 1                     # the raw pass selected one patch more than survives
    _same(dev, want)
    _same(_cover(case, "both", "host", monkeypatch, torch_cuda), want)


# ---- the new entry points on their own -------------------------------------------------------

@pytest.mark.parametrize("use_z", [True, False])
@pytest.mark.parametrize("k", [2, 5])
def test_mask_dilate_equals_scipy(k, use_z, torch_cuda):
    import scipy.ndimage
    from patchperpix_amd import backend
    from tests_flags import FLYLIGHT
    torch = torch_cuda
    shape = (5, 9, 37)
    rng = np.random.default_rng(3)
    m = rng.random(shape) < 0.02
    m[0, 0, 0] = m[4, 8, 36] = m[2, 4, 31] = m[2, 4, 32] = True     # corners, a word boundary
    P = backend.make_params(shape, (3, 3, 3), **FLYLIGHT)
    got = backend.mask_dilate(torch.from_numpy(m.astype(np.uint8)).cuda(), k, P, use_z=use_z).cpu().numpy()
    if use_z:
        want = scipy.ndimage.binary_dilation(m, iterations=k)
    else:
        want = np.stack([scipy.ndimage.binary_dilation(s, iterations=k) for s in m])
    assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got.astype(bool), want)


def _unpack_marks(mark_bits, shape):
    Z, Y, X = shape
    words = mark_bits.cpu().numpy().view(np.uint32).reshape(Z * Y, (X + 31) // 32 + 1)
    bits = (words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(Z * Y, -1)[:, :X].reshape(shape).astype(bool), bits.reshape(Z * Y, -1)[:, X:]


def test_marks_from_selected_equals_numpy_slices(torch_cuda):
    from patchperpix_amd import backend
    from tests_flags import FLYLIGHT
    torch = torch_cuda
    shape = (3, 11, 70)
    centres = np.array([[0, 5, 5], [0, 1, 20], [0, 2, 40], [1, 5, 1], [1, 5, 2], [1, 9, 68], [1, 10, 69], [2, 3, 3],
                        [2, 4, 30], [2, 4, 33], [2, 7, 66], [0, 8, 35]], dtype=np.int64)
    picked = np.ones(len(centres), dtype=bool)
    picked[-1] = False
    want = np.zeros(shape, dtype=bool)
    for (z, y, x) in centres[picked]:
        want[z, y - 3:y + 4, x - 3:x + 4] = True          # (the reference's plain slices)
    assert not want[0, :, 17:24].any() and not want[1, :, :6].any() and want[1, 10, 69]
    P = backend.make_params(shape, (3, 3, 3), **FLYLIGHT)
    lin = torch.from_numpy((centres[:, 0] * shape[1] + centres[:, 1]) * shape[2] + centres[:, 2]).cuda()
    marks = backend.cover_mark_bits(P, lin.device)
    marks.fill_(-1)                                        # rebuilt from nothing
    backend.cover_marks_from_selected(lin, torch.from_numpy(picked).cuda(), marks, P)
    got, spare = _unpack_marks(marks, shape)
    assert np.array_equal(got, want) and not spare.any()
    backend.cover_marks_from_selected(lin, None, marks, P)
    want[0, 5:11, 32:39] = True
    assert np.array_equal(_unpack_marks(marks, shape)[0], want)


def test_marked_pass_on_its_own(torch_cuda):
    """ppp_cover_pass_marked against the host loop's marked pass: states and marks, list-order bits and
    the per-voxel bit table."""
    from patchperpix_amd import backend
    torch = torch_cuda
    case = cases.synthetic("A")
    kw = case.flags("mark")
    P = backend.make_params(case.shape, case.ps, **kw)
    n = len(case.ranked_coords)
    lin_h = np.ravel_multi_index(tuple(case.ranked_coords.T.astype(np.int64)), case.shape)
    pred = torch.from_numpy(case.pred).cuda()
    bits = backend.patch_bits(pred, torch.from_numpy(case.ranked_coords).cuda(), kw["fc_threshold"], P)
    # host: one pass, no stop (remaining never reaches 0)
    running, _owner = backend.padded_mask(case.mask_to_cover)
    marked_h = np.zeros(case.shape, dtype=np.uint8)
    sel_h = np.zeros(n, dtype=np.uint8)
    backend.host_cover_pass(running, (case.overlap_mask > 0).astype(np.uint8), case.ps, lin_h, case.ranked_scores,
                            bits.cpu().numpy().view(np.uint32), 0, None, sel_h, 1 << 40, marked=marked_h)
    never = torch.from_numpy(case.overlap_mask.reshape(-1)[lin_h] > 0).cuda()
    lin = torch.from_numpy(lin_h).cuda()
    V = int(np.prod(case.shape))
    table = torch.zeros((V, bits.shape[1]), dtype=torch.int32, device=lin.device)
    table[lin] = bits
    for b, first in ((bits, None), (table, 0)):
        mask = torch.from_numpy(case.mask_to_cover.astype(np.uint8)).cuda()
        marks = backend.cover_mark_bits(P, lin.device)
        state = torch.where(never, 2, 0).to(torch.int32)
        backend.cover_pass_device(mask, b, lin, state, 0, P, bits_first_voxel=first, mark_bits=marks)
        assert np.array_equal(state.cpu().numpy() == 1, sel_h.astype(bool))
        assert np.array_equal(_unpack_marks(marks, case.shape)[0], marked_h.astype(bool))
        assert np.array_equal(mask.cpu().numpy() != 0, running != 0)


# ---- through the drivers ---------------------------------------------------------------------

def _kw(base, **over):
    return dict(base, debug=False, isbiHack=False, save_no_intermediates=True, sample=1.0,
                result_folder="/tmp", affinities="x.zarr", **over)


def _forbid_the_host_loop(monkeypatch):
    from patchperpix_amd.vote_instances import batch2d
    from patchperpix_amd.vote_instances import foreground_cover as fc

    def refuse(*a, **k):
        raise AssertionError("the sequential host cover was called")
    monkeypatch.setattr(fc, "cover_sequential", refuse)
    monkeypatch.setattr(batch2d, "cover_sequential", refuse)


@pytest.mark.parametrize("name", ["A", "B"])
def test_tiled_assembly_keeps_the_cover_on_the_device(name, torch_cuda, monkeypatch):
    from patchperpix_amd.vote_instances import vote_instances as vi
    case = cases.synthetic(name)
    kw = _kw(case.flags("both"))
    _forbid_the_host_loop(monkeypatch)
    args = lambda: (case.pred.copy(), case.foreground.copy(), case.foreground.copy(), case.numinst.copy(), case.ps)  # noqa: E731
    want, want_fg = vi.to_instance_seg(*args(), **kw)
    assert want.any()
    grid = dict(_n_slabs=2 if case.shape[0] > 1 else 1, _yx_tiles=(2, 2))
    inst, fg = vi.to_instance_seg(*args(), **dict(kw, **grid))
    assert np.array_equal(inst, want) and np.array_equal(fg, want_fg)


def test_batch_of_slices_serves_marks_and_ring_per_slice(torch_cuda, monkeypatch):
    from patchperpix_amd import synth
    from patchperpix_amd.vote_instances import vote_instances as vi
    from tests_flags import FLYLIGHT
    ps = (1, 5, 5)
    parts = [synth.make_case((1, 60, 64), ps, seed=s, cell=[1, 11, 11], overlap_frac=0.03, kind="cells")
             for s in (72, 77, 78)]
    pred = np.concatenate([c["pred"] for c in parts], axis=1).astype(np.float32)
    fg = np.concatenate([c["foreground"] for c in parts])
    ni = np.concatenate([c["numinst"] for c in parts])
    kw = _kw(dict(FLYLIGHT, **cases.OPTIONS["both"]))
    _forbid_the_host_loop(monkeypatch)
    inst, fgo = vi.to_instance_seg(pred.copy(), fg.copy(), fg.copy(), ni.copy(), ps, independent_slices=True, **kw)
    assert all(inst[k].any() for k in range(3))
    for k in range(3):
        sl = slice(k, k + 1)
        i1, f1 = vi.to_instance_seg(np.ascontiguousarray(pred[:, sl]), fg[sl].copy(), fg[sl].copy(), ni[sl].copy(), ps, **kw)
        assert np.array_equal(inst[sl], i1), k
        assert np.array_equal(fgo[sl], f1), k
