"""GPU (MI355X): every tile shape the launcher of the workgroup ranking kernel (ppp_rank_wg.hip) can
choose, for every patch size the kernel is built for -- the shapes are forced through the launcher's
development switches, because the volumes a test can afford are far below the 1 024 big tiles at which
the launcher picks 8 x 16 x 16 (and splits tiles) on its own.  Scores are compared as uint32 bit patterns
with the gather kernel on compact planes (the one pinned to the goldens and the oracle): no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (PPP_RANK_WG_TILE, PPP_RANK_WG_SPLIT): the three tile shapes whole, and with the heaviest tiles of every
# XCD's range split into halves (some / more than there are: every tile) -- the mixed launch
SHAPES = [("8x8x16", "0"), ("8x16x16", "0"), ("16x8x16", "0"), ("8x16x16", "1"), ("8x16x16", "3"),
          ("8x16x16", "999"), ("8x8x16", "2"), ("16x8x16", "2")]
CASES = [((7, 7, 7), (40, 37, 45), 12), ((5, 5, 5), (38, 41, 43), 9), ((9, 9, 9), (41, 36, 44), 13)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert backend.device_count() >= 1
    return torch


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "p%d" % c[0][0])
def case(request, torch_cuda):
    """ragged volume with overlap voxels; the gather kernel's scores for the whole volume; the inputs of
    the workgroup kernel for the whole volume and for an inner score box inside a consensus box"""
    torch = torch_cuda
    from patchperpix_amd import backend, synth
    from tests_flags import FLYLIGHT
    ps, shape, cell = request.param
    c = synth.make_case(shape, ps, seed=97, cell=[cell] * 3, overlap_frac=0.03)
    kw = dict(FLYLIGHT)
    P = backend.make_params(shape, ps, **kw)
    pred = torch.from_numpy(c["pred"].astype(np.float16)).cuda()
    ov = torch.from_numpy((c["numinst"] > 1).astype(np.uint8)).cuda()
    cons = backend.consensus(pred, ov, P)
    want = backend.rank_patches(pred, cons, ov, P).cpu().numpy()
    assert (want > 0).sum() > 100
    vm, Pv = backend.cons_to_voxel_major(cons, P)
    del cons
    r = ps[0] // 2
    sb = (r + 2, r + 1, r + 3, shape[0] - r - 3, shape[1] - r - 2, shape[2] - r - 5)
    box = (sb[0] - r, sb[1] - r, sb[2] - r, sb[3] + r, sb[4] + r, sb[5] + r)
    Pt = backend.make_params(shape, ps, cons_box=box, **kw)
    vm_t, Pvt = backend.cons_to_voxel_major(backend.consensus(pred, ov, Pt), Pt)
    return dict(pred=pred, ov=ov, want=want, vm=vm, Pv=Pv, vm_t=vm_t, Pvt=Pvt, sb=sb)


@pytest.mark.parametrize("tile,split", SHAPES, ids=["%s-split%s" % s for s in SHAPES])
def test_rank_wg_every_tile_shape(case, tile, split, monkeypatch):
    from patchperpix_amd import backend
    monkeypatch.setenv("PPP_RANK_WG_TILE", tile)
    monkeypatch.setenv("PPP_RANK_WG_SPLIT", split)
    backend.reload_env()
    try:
        got = backend.rank_patches(case["pred"], case["vm"], case["ov"], case["Pv"]).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), case["want"].view(np.uint32))
        sb = case["sb"]
        got_t = backend.rank_patches(case["pred"], case["vm_t"], case["ov"], case["Pvt"], score_box=sb).cpu().numpy()
        sl = tuple(slice(sb[i], sb[i + 3]) for i in range(3))
        assert np.array_equal(got_t[sl].view(np.uint32), case["want"][sl].view(np.uint32))
    finally:
        monkeypatch.undo()
        backend.reload_env()
