"""No stage writes outside the device workspace it asked for.

No entry point that takes a d_work pointer is told how large the buffer is: a launcher stays inside it
because its carve and its ppp_*_workspace_bytes query run the same layout function (csrc, `Carver`).
Here every workspace the package allocates (backend._workspace) gets a guard band in front and behind,
filled with 0xA5 like the workspace itself; after the run every band must be untouched, the results must
be those of the same call on plain buffers, and every stage the case is about must have asked for a
workspace.  The bands are memory the test owns: a stray write shows as a failed assertion, not a fault."""
import sys

import numpy as np
import pytest

from conftest import Golden

pytestmark = pytest.mark.gpu

FILL = 0xA5
LABELS = ("label_components", "LabelState.__init__")     # either serves the connected components


class Guarded:
    """Stands in for backend._workspace: [band | nbytes | band], all 0xA5, the middle handed out.
    A band is as large as the request (an array that the size query forgot altogether still lands
    in it), a multiple of 256 bytes (the workspace keeps its alignment), at least 4096 bytes."""

    def __init__(self, backend, torch):
        self.backend, self.torch, self.taken = backend, torch, []

    def __call__(self, nbytes, device):
        nbytes = int(nbytes)
        self.backend.check(min(nbytes, 0))
        band = max(4096, (nbytes + 255) // 256 * 256)
        buf = self.torch.full((band + nbytes + band,), FILL, dtype=self.torch.uint8, device=device)
        f = sys._getframe(1)
        who = f.f_code.co_name
        if who == "__init__":
            who = type(f.f_locals["self"]).__name__ + ".__init__"
        self.taken.append((buf, nbytes, band, who))
        return buf[band:band + nbytes]

    def verify(self, *stages):
        """every band intact; every stage (a caller's name, or a tuple of alternatives) asked"""
        self.torch.cuda.synchronize()
        assert self.taken
        for buf, nbytes, band, who in self.taken:
            for name, part in (("front", buf[:band]), ("back", buf[band + nbytes:])):
                bad = self.torch.nonzero(part != FILL).flatten()
                assert bad.numel() == 0, "%s wrote %d bytes into the %s band of its %d-byte workspace, first at %d" % (
                    who, bad.numel(), name, nbytes, int(bad[0]) - (band if name == "front" else 0))
        callers = {t[3] for t in self.taken}
        for s in stages:
            assert callers & set(s if isinstance(s, tuple) else (s,)), "%s asked for no workspace (%s did)" % (s, sorted(callers))


@pytest.fixture
def guard(monkeypatch):
    import torch
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"

    def install():
        g = Guarded(backend, torch)
        monkeypatch.setattr(backend, "_workspace", g)
        monkeypatch.setattr(backend, "_S1_WORK", {})      # (S1 keeps its workspace between calls)
        return g
    return install


def _fused(g):
    from patchperpix_amd.vote_instances import vote_instances as vi
    kw = dict(g.kw, debug=False, isbiHack=False, save_no_intermediates=True, sample=1.0, result_folder="/tmp",
              affinities="x.zarr")
    return vi.to_instance_seg(g.pred.copy(), g.foreground.copy(), g.foreground.copy(), g.numinst.copy(),
                              g.patchshape, **kw)


@pytest.mark.parametrize("name,stages", [
    # 3^3: S2's one-wave kernel; ranked list, cover passes, thinning, watershed edges
    ("c3d_p3_thin_mws", ("rank_patches", "rank_order_device", "cover_pass_device", "thin_cover_device", "mws_edges_device")),
    # 5^3: S2's workgroup kernel (its workspace carries the tile weights, the order and the dealing table)
    ("c3d_p5_thin_mws", ("rank_patches", "rank_order_device", "cover_pass_device", "thin_cover_device", "mws_edges_device")),
    # 2-d (pz = 1) layouts; connected components instead of the watershed
    ("c2d_p5_blobs", ("rank_patches", "rank_order_device", "cover_pass_device", LABELS)),
])
def test_fused_pipeline_stays_inside_its_workspaces(name, stages, guard):
    g = Golden(name)
    want_inst, want_fg = _fused(g)
    guarded = guard()
    inst, fg = _fused(g)
    guarded.verify(*stages)
    assert inst.dtype == want_inst.dtype and np.array_equal(inst, want_inst) and np.array_equal(fg, want_fg)
    assert np.array_equal(inst, g["instances"]) and inst.any()


def test_s1_item_lists_stay_inside_their_workspace(guard):
    import torch
    from patchperpix_amd import backend, synth
    from tests_flags import FLYLIGHT
    shape, ps = (12, 14, 18), (5, 5, 5)
    c = synth.make_case(shape, ps, seed=29, cell=[6, 6, 6], overlap_frac=0.02)
    P = backend.make_params(shape, ps, **dict(FLYLIGHT))
    pred = torch.from_numpy(c["pred"].astype(np.float16)).cuda()
    ov = torch.from_numpy((c["numinst"] > 1).astype(np.uint8)).cuda()
    with backend.s1_sparse_scope(0):
        dense = backend.consensus(pred, ov, P)
    with backend.s1_sparse_scope(1):
        plain = backend.consensus(pred, ov, P)
        guarded = guard()
        got = backend.consensus(pred, ov, P)
    guarded.verify("_consensus_sparse")
    assert backend.consensus_last_items()[2] == 1, "the item lists did not run"
    assert torch.equal(got.view(torch.int32), plain.view(torch.int32))
    assert torch.equal(got.view(torch.int32), dense.view(torch.int32)) and bool((dense != 0).any())


def test_cover_shard_stays_inside_its_workspace(guard, monkeypatch):
    from patchperpix_amd import backend, tiling
    g = Golden("c3d_p5_thin_mws")
    shape = tuple(g.foreground.shape)
    kw = dict(g.kw, debug=False, isbiHack=False, save_no_intermediates=True, sample=1.0, result_folder="/tmp",
              affinities="x.zarr")
    monkeypatch.setenv("PPP_COVER_SHARDED", "force")

    def run():
        return tiling.assemble(backend.to_device_pred(g.pred.copy()), 0, shape, g.foreground.copy(), g.foreground.copy(),
                               g.numinst.copy(), g.patchshape, [(0, shape[0])], **kw)
    want_inst, want_fg = run()
    guarded = guard()
    inst, fg = run()
    guarded.verify("CoverShard.__init__")
    assert np.array_equal(inst, want_inst) and np.array_equal(fg, want_fg)
    assert np.array_equal(inst, g["instances"]) and inst.any()


def test_thin_shard_stays_inside_its_workspace(guard):
    import torch
    from patchperpix_amd import backend, tiling
    g = Golden("c3d_p5_thin_mws")
    shape, ps = tuple(g.foreground.shape), g.patchshape
    Z, Y, X = shape
    flags = {k: v for k, v in g.kw.items() if k not in ("cons_box", "cons_layout", "origin")}
    P = backend.make_params(shape, ps, **flags)
    pred = backend.to_device_pred(g.pred.copy())
    # the patches the cover selected, in the order of its list
    coords = torch.from_numpy(np.ascontiguousarray(g["cover_coords"].astype(np.int32))).cuda()
    n = int(coords.shape[0])
    assert n > 10
    lin = ((coords[:, 0].to(torch.int64) * Y + coords[:, 1]) * X + coords[:, 2]).contiguous()
    bits = backend.patch_bits(pred, coords, g.kw["fc_threshold"], P)
    mask = g.foreground.copy().astype(bool)
    mask[g.numinst > 1] = False
    mask_d = torch.from_numpy(mask.astype(np.uint8)).cuda()
    rad = [p // 2 for p in ps]
    interior = int(mask[tuple(slice(r, s - r) for r, s in zip(rad, shape))].sum())

    def shard():
        keep, _ = tiling.sharded_thin_own(
            tiling.DeviceOps(), tiling.LocalComm(), shape, ps, (0, Z), [(0, Z)], mask_d.clone(), 0, interior, lin,
            torch.arange(n, dtype=torch.int64, device="cuda"), bits,
            lambda a, b: backend.make_params((b - a, Y, X), ps, origin=(a, 0, 0), **flags))
        return keep.cpu().numpy()
    want = np.flatnonzero(backend.thin_cover_device(mask_d, bits, lin, P).cpu().numpy())
    plain = shard()
    guarded = guard()
    got = shard()
    kept = np.flatnonzero(backend.thin_cover_device(mask_d, bits, lin, P).cpu().numpy())
    guarded.verify("ThinShard.__init__", "thin_cover_device")
    assert np.array_equal(got, plain) and np.array_equal(kept, want)
    assert np.array_equal(got, want) and 0 < len(want) <= n
