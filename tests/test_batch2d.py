"""GPU: a stack of independent 2-d images voted in one call (``independent_slices=True``) equals,
slice by slice and bit for bit, one call per image -- instance ids, foreground and the per-slice
(pairs, aff) intermediates."""
import numpy as np
import pytest

from conftest import Golden, golden_names

pytestmark = pytest.mark.gpu

C2D = [n for n in golden_names() if n.startswith("c2d_")]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert backend.device_count() >= 1
    return torch


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _kw(base, **over):
    return dict(base, debug=False, isbiHack=False, save_no_intermediates=True, sample=1.0,
                result_folder="/tmp", affinities="x.zarr", **over)


def _vi():
    from patchperpix_amd.vote_instances import vote_instances as vi
    return vi


def _batched(pred, fg, mask, ni, ps, **kw):
    return _vi().to_instance_seg(pred.copy(), fg.copy(), mask.copy(), ni.copy(), ps, independent_slices=True, **kw)


def _one(pred, fg, mask, ni, ps, k, **kw):
    sl = slice(k, k + 1)
    return _vi().to_instance_seg(np.ascontiguousarray(pred[:, sl]), fg[sl].copy(), mask[sl].copy(),
                                 ni[sl].copy(), ps, **kw)


@pytest.mark.parametrize("name", C2D)
def test_golden_stack_equals_the_golden_per_slice(name, torch_cuda):
    """N = 5 copies of every 2-d golden case in one call: every slice is the reference's result.
    (Without the same-slice pair rule the identical neighbours would merge; with a z-dependent LCG
    seed slices 1..4 would get other affinities.)"""
    g = Golden(name)
    N = 5
    pred = np.concatenate([g.pred] * N, axis=1)
    fg = np.concatenate([g.foreground] * N)
    ni = np.concatenate([g.numinst] * N)
    kw = _kw(g.kw)
    inst, fgo = _batched(pred, fg, fg, ni, g.patchshape, **kw)
    assert inst.shape == fg.shape and inst.dtype == np.uint16
    for k in range(N):
        if g.has("instances"):
            assert np.array_equal(inst[k:k + 1], g["instances"]), k
            assert np.array_equal(fgo[k:k + 1], g["foreground_out"]), k
        else:
            assert not inst[k].any()
    res = _batched(pred, fg, fg, ni, g.patchshape, **dict(kw, return_intermediates=True))
    assert len(res) == N
    for k in range(N):
        if g.has("aff"):
            assert np.array_equal(res[k][0], g["pairs"]), k
            assert np.array_equal(_bits(res[k][1]), _bits(g["aff"])), k
        else:
            assert res[k] == (None, None)


def _mixed_stack(ps, Y=44, X=48):
    """Different random images, an empty slice, and a slice whose mask is empty but whose
    foreground is not."""
    from patchperpix_amd import synth
    cases = [synth.make_case((1, Y, X), ps, seed=s, cell=[1, 3 * ps[1], 3 * ps[2]], overlap_frac=0.02 * (s % 2))
             for s in (5, 6, 7, 8)]
    empty = synth.make_case((1, Y, X), ps, seed=9, kind="empty")
    order = [cases[0], empty, cases[1], cases[2], cases[3]]
    pred = np.concatenate([c["pred"] for c in order], axis=1).astype(np.float32)
    fg = np.concatenate([c["foreground"] for c in order])
    ni = np.concatenate([c["numinst"] for c in order])
    mask = fg.copy()
    mask[3] = False              # mask empty, foreground not: that slice's own call returns early
    return pred, fg, mask, ni


@pytest.mark.parametrize("mws", [False, True])
@pytest.mark.parametrize("sparse", [True, False])
@pytest.mark.parametrize("ps", [(1, 5, 5), (1, 9, 9)])
def test_mixed_stack_equals_per_slice_calls_and_the_oracle(mws, sparse, ps, torch_cuda):
    from oracle import ppp_oracle as orc
    from patchperpix_amd.flags import FLYLIGHT
    pred, fg, mask, ni = _mixed_stack(ps)
    kw = _kw(FLYLIGHT, mws=mws, select_patches_for_sparse_data=sparse)
    inst, fgo = _batched(pred, fg, mask, ni, ps, **kw)
    inter = _batched(pred, fg, mask, ni, ps, **dict(kw, return_intermediates=True))
    assert any(inst[k].any() for k in range(len(fg)))
    for k in range(len(fg)):
        i1, f1 = _one(pred, fg, mask, ni, ps, k, **kw)
        assert np.array_equal(inst[k:k + 1], i1), k
        assert np.array_equal(fgo[k:k + 1], f1), k
        p1 = _one(pred, fg, mask, ni, ps, k, **dict(kw, return_intermediates=True))
        if p1[0] is None:
            assert inter[k] == (None, None), k
        else:
            assert np.array_equal(inter[k][0], p1[0]), k
            assert np.array_equal(_bits(inter[k][1]), _bits(p1[1])), k
        sl = slice(k, k + 1)
        ref = orc.to_instance_seg(pred[:, sl], fg[sl].copy(), mask[sl].copy(), ni[sl].copy(), ps, **kw)
        assert np.array_equal(inst[k:k + 1], ref["instances"]), k
        if "pairs" in ref and inter[k][0] is not None:
            assert np.array_equal(inter[k][0], ref["pairs"]), k
            assert np.array_equal(_bits(inter[k][1]), _bits(ref["aff"])), k
    assert not inst[1].any() and not inst[3].any()
    assert inter[1] == (None, None) and inter[3] == (None, None)


def test_thinned_cover_with_components_at_7x7_patches(torch_cuda):
    """Patch shape (1, 7, 7) with the thinned cover (ppp_thin_cover_slices: its stop rule per slice)
    and connected components: pairs, affinities and ids of every slice are its own call's."""
    from patchperpix_amd.flags import FLYLIGHT_CC
    ps = (1, 7, 7)
    pred, fg, mask, ni = _mixed_stack(ps, Y=40, X=52)
    kw = _kw(FLYLIGHT_CC)                # (mws = false, skipThinCover = false)
    inter = _batched(pred, fg, mask, ni, ps, **dict(kw, return_intermediates=True))
    inst, _ = _batched(pred, fg, mask, ni, ps, **kw)
    for k in range(len(fg)):
        p1 = _one(pred, fg, mask, ni, ps, k, **dict(kw, return_intermediates=True))
        if p1[0] is None:
            assert inter[k] == (None, None)
            continue
        assert np.array_equal(inter[k][0], p1[0]), k
        assert np.array_equal(_bits(inter[k][1]), _bits(p1[1])), k
        assert np.array_equal(inst[k:k + 1], _one(pred, fg, mask, ni, ps, k, **kw)[0]), k


def test_chunks_of_whole_slices_give_the_same_result(torch_cuda, monkeypatch):
    from patchperpix_amd.flags import FLYLIGHT_CC
    from patchperpix_amd.vote_instances import batch2d
    ps = (1, 5, 5)
    pred, fg, mask, ni = _mixed_stack(ps)
    kw = _kw(FLYLIGHT_CC)
    whole, _ = _batched(pred, fg, mask, ni, ps, **kw)
    calls = []
    inner = batch2d._vote_batch
    monkeypatch.setattr(batch2d, "_vote_batch", lambda pred, fg, *a: calls.append(fg.shape[0]) or inner(pred, fg, *a))
    chunked, _ = _batched(pred, fg, mask, ni, ps, _chunk_slices=2, **kw)
    assert calls == [2, 1]          # the 3 slices that pass the early-outs, in chunks of 2
    assert np.array_equal(whole, chunked)


def test_pair_kernel_rows_split_by_slice_equal_the_per_slice_rows(torch_cuda):
    """ppp_patch_pairs_*_slices on a (z, x)-sorted list: the rows of slice k, in order, are the rows
    of slice k's own x-sorted list; no row links two slices (neighbouring slices hold the same
    centres, which the plain kernel pairs at dz = 1)."""
    torch = torch_cuda
    from patchperpix_amd import backend
    from patchperpix_amd.flags import FLYLIGHT
    rng = np.random.default_rng(3)
    N, Y, X, ps = 4, 60, 70, (1, 9, 9)
    base = np.stack([np.zeros(40, np.int32), rng.integers(4, Y - 4, 40), rng.integers(4, X - 4, 40)], 1).astype(np.int32)
    pts = np.concatenate([base + np.array([k, 0, 0], np.int32) for k in range(N)] +
                         [np.stack([np.full(15, 2), rng.integers(4, Y - 4, 15), rng.integers(4, X - 4, 15)], 1).astype(np.int32)])
    order = np.lexsort((pts[:, 2], pts[:, 0]))
    pts = np.ascontiguousarray(pts[order])
    P = backend.make_params((N, Y, X), ps, **FLYLIGHT)
    rows = backend.device_patch_pairs(torch.from_numpy(pts).cuda(), P, include_single=True, slices=True)
    rows = rows.cpu().numpy().view(np.uint32)
    assert (rows[:, 0] == rows[:, 3]).all()
    P1 = backend.make_params((1, Y, X), ps, **FLYLIGHT)
    for k in range(N):
        own = pts[pts[:, 0] == k] - np.array([k, 0, 0], np.int32)
        one = backend.device_patch_pairs(torch.from_numpy(np.ascontiguousarray(own)).cuda(), P1,
                                         include_single=True).cpu().numpy().view(np.uint32)
        got = rows[rows[:, 0] == k].copy()
        got[:, [0, 3]] = 0
        assert np.array_equal(got, one), k


def test_cli_label_with_batch_2d_writes_the_same_files(tmp_path, torch_cuda, monkeypatch):
    """run_ppp --do label with [vote_instances] batch_2d: 2-d samples of equal shape are voted in
    one call, a sample of another shape in a group of its own; every result file holds what the
    one-at-a-time run writes."""
    import os
    from conftest import GOLDEN_DIR
    from patchperpix_amd import run_ppp, synth
    from patchperpix_amd.vote_instances import vote_instances as vi_mod
    from test_cli_gpu import _load_result
    calls = []
    inner = vi_mod.to_instance_seg

    def recording(pred, *a, **k):
        calls.append((bool(k.get("independent_slices", False)), int(np.shape(pred)[1])))
        return inner(pred, *a, **k)
    monkeypatch.setattr(vi_mod, "to_instance_seg", recording)
    pred_dir = tmp_path / "pred"
    pred_dir.mkdir()
    shapes = {"s0": (40, 44), "s1": (40, 44), "s2": (36, 50), "s3": (40, 44)}
    for i, (name, (Y, X)) in enumerate(sorted(shapes.items())):
        c = synth.make_case((1, Y, X), (1, 5, 5), seed=80 + i, cell=[1, 9, 9])
        np.save(pred_dir / (name + ".npy"), c["pred"][:, 0])
    extra = tmp_path / "batch.toml"
    extra.write_text("[vote_instances]\nbatch_2d = 16\n")
    base = os.path.join(GOLDEN_DIR, "label_config.toml")
    ran = {}
    for out, cfgs in (("one", [base]), ("batch", [base, str(extra)])):
        argv = [a for c in cfgs for a in ("--config", c)]
        del calls[:]
        run_ppp.main(argv + ["--do", "label", "--pred-folder", str(pred_dir), "--output-folder", str(tmp_path / out)])
        ran[out] = list(calls)
    assert ran["one"] == [(False, 1)] * 4
    assert ran["batch"] == [(True, 3), (True, 1)]     # the (40, 44) group, then the other shape
    assert sorted(os.listdir(tmp_path / "one")) == sorted(os.listdir(tmp_path / "batch"))
    for name in shapes:
        a, b = _load_result(str(tmp_path / "one"), name), _load_result(str(tmp_path / "batch"), name)
        assert sorted(a) == sorted(b)
        for key in a:
            assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), (name, key)
        assert a["vote_instances"].max() > 1
