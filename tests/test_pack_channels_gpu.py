"""`no_overlap_per_channel` on the device: sizes and overlap pairs in one pass (ppp_pack_scan_count /
_fill), the channel walk on the host, one paint by channel -- equal to the oracle's paint_per_channel
on components given directly (more than one channel, up to seven components on a voxel, small
components painted over large ones, empty components), equal to the loop over components
(PPP_PACK_CHANNELS=loop) where a window is clipped by the volume border, additive over sub-boxes, and
end to end on crossing bars: stage path, loop, tiled assembly, provider and two ranks give the
oracle's map."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pack_channels_cases as pc
from conftest import REPO
from test_workspace_bounds import guard  # noqa: F401  (the guard-band fixture)

pytestmark = pytest.mark.gpu


def _on_device(pred, nodes, labels, dtype="float32"):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return (torch.from_numpy(np.ascontiguousarray(pred.astype(dtype))).cuda(), torch.from_numpy(nodes).cuda(),
            torch.from_numpy(labels).cuda())


def _params(shape, ps):
    from patchperpix_amd import backend
    from tests_flags import FLYLIGHT
    return backend.make_params(shape, ps, **dict(FLYLIGHT, patch_threshold=pc.TH))


@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("i", range(len(pc.DIRECT)))
def test_direct_cases_equal_the_oracle(i, dtype):
    import torch
    from patchperpix_amd import backend
    from patchperpix_amd.vote_instances import graph_to_labeling as g2l
    shape, ps = pc.DIRECT[i][:2]
    pred, ccs = pc.direct_case(i)
    want, masks = pc.direct_expected(i)
    nodes, labels = pc.nodes_and_labels(ccs)
    pred_d, nodes_d, labels_d = _on_device(pred, nodes, labels, dtype)
    P = _params(shape, ps)
    sizes, keys = backend.pack_scan(pred_d, nodes_d, labels_d, len(ccs), P)
    assert np.array_equal(sizes.cpu().numpy(), np.concatenate([[0], masks.reshape(len(masks), -1).sum(1)]))
    # one key per pair and shared voxel; their set is the set of overlapping pairs
    shared = masks.sum(0).astype(np.int64)
    assert keys.numel() == int((shared * (shared - 1) // 2).sum())
    assert np.array_equal(torch.unique(keys).cpu().numpy().astype(np.uint64), np.sort(pc.overlap_pairs(masks)))
    got = g2l.paint_channels(pred_d, nodes_d, labels_d, len(ccs), shape, P).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)


def test_border_nodes_equal_the_loop(monkeypatch):
    """windows clipped by the volume border (the reference's indexing fails there; the kernels clip):
    held equal to the loop over components"""
    from patchperpix_amd.vote_instances import graph_to_labeling as g2l
    shape, ps = pc.DIRECT[3][:2]
    Z, Y, X = shape
    pred, ccs = pc.direct_case(3)
    ccs = [list(cc) for cc in ccs]
    ccs[0] += [(0, 0, 0), (Z - 1, Y - 1, X - 1)]
    ccs[3] += [(0, 5, X - 1), (1, 0, 2)]
    ccs[5] += [(Z - 1, 3, 0), (0, 1, 1)]
    nodes, labels = pc.nodes_and_labels(ccs)
    pred_d, nodes_d, labels_d = _on_device(pred, nodes, labels)
    P = _params(shape, ps)
    got = g2l.paint_channels(pred_d, nodes_d, labels_d, len(ccs), shape, P).cpu().numpy()
    monkeypatch.setenv("PPP_PACK_CHANNELS", "loop")
    want = g2l.paint_channels(pred_d, nodes_d, labels_d, len(ccs), shape, P).cpu().numpy()
    assert want.shape[0] >= 2 and got.shape == want.shape and np.array_equal(got, want)
    # the border nodes took part: the corner voxels belong to a component
    assert want[:, 0, 0, 0].any() or want[:, Z - 1, Y - 1, X - 1].any()


@pytest.mark.parametrize("axis", [0, 2])
def test_half_boxes_sum_to_the_whole_box(axis):
    import torch
    from patchperpix_amd import backend
    shape, ps = pc.DIRECT[1][:2]
    pred, ccs = pc.direct_case(1)
    nodes, labels = pc.nodes_and_labels(ccs)
    pred_d, nodes_d, labels_d = _on_device(pred, nodes, labels)
    P = _params(shape, ps)
    sizes, keys = backend.pack_scan(pred_d, nodes_d, labels_d, len(ccs), P)
    cut = shape[axis] // 2 + 1
    lo, hi = [0, 0, 0], list(shape)
    hi[axis] = cut
    part = torch.zeros_like(sizes)
    _, k0 = backend.pack_scan(pred_d, nodes_d, labels_d, len(ccs), P, own=tuple(lo) + tuple(hi), sizes=part)
    lo[axis], hi[axis] = cut, shape[axis]
    _, k1 = backend.pack_scan(pred_d, nodes_d, labels_d, len(ccs), P, own=tuple(lo) + tuple(hi), sizes=part)
    assert sizes.sum() > 0 and torch.equal(part, sizes)
    assert k0.numel() > 0 and k1.numel() > 0 and k0.numel() + k1.numel() == keys.numel()
    assert torch.equal(torch.unique(torch.cat([k0, k1])), torch.unique(keys))
    # an empty box is a valid box
    empty, k2 = backend.pack_scan(pred_d, nodes_d, labels_d, len(ccs), P, own=(2, 2, 2, 2, 9, 9))
    assert k2.numel() == 0 and not empty.any()


def test_pass_stays_inside_its_workspace(guard):  # noqa: F811
    from patchperpix_amd import backend
    shape, ps = pc.DIRECT[3][:2]
    pred, ccs = pc.direct_case(3)
    want, masks = pc.direct_expected(3)
    nodes, labels = pc.nodes_and_labels(ccs)
    pred_d, nodes_d, labels_d = _on_device(pred, nodes, labels)
    P = _params(shape, ps)
    guarded = guard()
    sizes, keys = backend.pack_scan(pred_d, nodes_d, labels_d, len(ccs), P)
    part, _ = backend.pack_scan(pred_d, nodes_d, labels_d, len(ccs), P, own=(3, 2, 5, 11, 20, 21))
    guarded.verify("pack_scan")
    assert np.array_equal(sizes.cpu().numpy()[1:], masks.reshape(len(masks), -1).sum(1))
    assert np.array_equal(part.cpu().numpy()[1:], masks[:, 3:11, 2:20, 5:21].reshape(len(masks), -1).sum(1))


def _run(case, ps, kw, **extra):
    from patchperpix_amd.vote_instances import vote_instances as vi
    return vi.to_instance_seg(case["pred"].copy(), case["foreground"].copy(), case["foreground"].copy(),
                              case["numinst"].copy(), list(ps), **dict(kw, **extra))


@pytest.mark.parametrize("ps,flagset", [((5, 5, 5), "shipped"), ((5, 5, 5), "nothin_cc"), ((3, 3, 3), "shipped"),
                                        ((3, 3, 3), "nothin_cc")])
def test_crossing_bars_end_to_end(ps, flagset, monkeypatch):
    """overlap voxels are no patch centres, so the bars hold together only through patches that reach
    across the thin overlaps -- and overlap there: the map needs a second channel"""
    from patchperpix_amd import backend, tiling
    from test_tiling import ArrayProvider
    case, kw, want = pc.bars_expected(ps, flagset)
    shape = case["foreground"].shape
    stage, fg = _run(case, ps, kw, _n_slabs=1)
    assert stage.dtype == want.dtype and stage.shape == want.shape and np.array_equal(stage, want)
    assert np.array_equal(fg, case["foreground"].astype(np.uint8))
    tiled, fg_t = _run(case, ps, kw, _n_slabs=2, _yx_tiles=(2, 2))
    assert tiled.dtype == want.dtype and tiled.shape == want.shape and np.array_equal(tiled, want)
    assert np.array_equal(fg_t, fg) and backend.NOTES.get("pack_channels") == want.shape[0]
    if ps == (5, 5, 5) and flagset == "shipped":
        prov, _ = tiling.assemble(ArrayProvider(case["pred"], device="cuda"), 0, shape, case["foreground"].copy(),
                                  case["foreground"].copy(), case["numinst"].copy(), list(ps),
                                  tiling.plan_slabs(shape[0], 2), _yx_tiles=(2, 2), **kw)
        assert prov.shape == want.shape and np.array_equal(prov, want)
    monkeypatch.setenv("PPP_PACK_CHANNELS", "loop")
    loop, _ = _run(case, ps, kw, _n_slabs=1)
    assert loop.shape == want.shape and np.array_equal(loop, want)


WORKER = r"""
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, {repo!r}); sys.path.insert(0, os.path.join({repo!r}, "tests"))
from patchperpix_amd import tiling, backend, flags as flagsets
import pack_channels_cases as pc
torch.cuda.set_device(0)                      # both ranks on the one GPU of the box
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
ps = (5, 5, 5)
case = pc.bars_case(ps)
shape = case["foreground"].shape
kw = dict(flagsets.FLAG_SETS["shipped"], no_overlap_per_channel=True)
slabs = tiling.plan_slabs(shape[0], world)
mine = tiling.slabs_of_rank(slabs, rank, world)
lo, hi = tiling.local_range(mine, shape[0], ps)
for gather in (True, False):
    pred_local = torch.from_numpy(np.ascontiguousarray(case["pred"][:, lo:hi])).cuda()
    inst, fg = tiling.assemble(pred_local, lo, shape, case["foreground"].copy(), case["foreground"].copy(),
                               case["numinst"].copy(), list(ps), mine, comm=tiling.TorchDistComm(), _yx_tiles=(1, 2),
                               _gather_result=gather, **kw)
    np.save(os.path.join({out!r}, "inst_%d_rank%d.npy" % (gather, rank)), inst)
np.save(os.path.join({out!r}, "own_rank%d.npy" % rank), np.array([mine[0][0], mine[-1][1]]))
dist.destroy_process_group()
"""


def test_two_ranks_sharing_the_gpu(tmp_path):
    """sizes and pairs split over two ranks (each counts its own slab, cut in two tiles): summed and
    united, the same walk on both -- the gathered map, and each rank's own z-range of every channel"""
    from test_tiling import _free_port
    case, kw, want = pc.bars_expected((5, 5, 5), "shipped")
    script = tmp_path / "pack_worker.py"
    script.write_text(WORKER.format(repo=REPO, out=str(tmp_path)))
    port = _free_port()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, OMP_NUM_THREADS="1")
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                           "--master-addr", "127.0.0.1", "--master-port", port, str(script)], env=env, timeout=600)
    for r in range(2):
        whole = np.load(tmp_path / ("inst_1_rank%d.npy" % r))
        assert whole.dtype == want.dtype and whole.shape == want.shape and np.array_equal(whole, want), "rank %d differs" % r
        z0, z1 = np.load(tmp_path / ("own_rank%d.npy" % r))
        own = np.load(tmp_path / ("inst_0_rank%d.npy" % r))
        assert own.shape == want[:, z0:z1].shape and np.array_equal(own, want[:, z0:z1]), "own range of rank %d differs" % r
