"""GPU (MI355X): every consumer of the prediction after S2 against NumPy's compare -- the float32 value against
float32(threshold) -- on predictions that hold float32(t) and its neighbours (tests/threshold_cases.py), exactly:

  bits        ppp_patch_bits, ppp_patch_bits_volume, backend.patch_bits on both routes, the fused pre-pass's bits_vol
              and patch_bits_from_table against the packed model for fc_threshold; S5's patch_fg_bits on the same
              prediction against the DOUBLE-rule model for patch_threshold: both rules side by side
  cover       the device cover (rows in rank order, a bit row per voxel, the pix_th ladder, marks) and the device
              thinning behind vote_instances/foreground_cover.py against orc.foreground_cover / orc.thin_cover
  pack, paint pack_scan, paint_instances, paint_patch_rows (face nodes: clipped windows), paint_instances_channels
              against the explicit models for patch_threshold
  renumber    label_slice_renumber against NumPy
  end to end  vote_instances.to_instance_seg against orc.to_instance_seg

tests/test_threshold_rule.py (CPU) asserts that on these cells the double rule, and a compare in the storage type,
give other results: a kernel that took either would fail here."""
import ctypes

import numpy as np
import pytest

import threshold_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert backend.device_count() >= 1
    return torch


def _set_env(monkeypatch, env):
    from patchperpix_amd import backend
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    backend.reload_env()


_INPUTS = {}        # one entry: the device prediction of the last cell


def _inputs(torch, cell):
    """(pred on the device in the cell's type, the float32 host array it widens to, P)"""
    from patchperpix_amd import backend
    s, pair, dtype = cell
    b = tc.base_case(s)
    if cell not in _INPUTS:
        _INPUTS.clear()
        host = tc.prediction(s, pair, dtype)
        pred = torch.from_numpy(np.array(host)).cuda().to(getattr(torch, dtype)).contiguous()
        assert np.array_equal(pred.float().cpu().numpy().view(np.uint32), host.view(np.uint32))     # an exact narrowing
        _INPUTS[cell] = (pred, host)
    pred, host = _INPUTS[cell]
    return pred, host, backend.make_params(b["vol"], b["ps"], **tc.flags(pair))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.count_nonzero(got != want)
    assert bad == 0, "%s: %d of %d entries differ from the model" % (what, bad, got.size)


# ---- bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", tc.BITS_CELLS, ids=tc.cell_id)
def test_patch_bits_follow_numpys_compare(cell, torch_cuda, monkeypatch):
    from patchperpix_amd import backend
    torch, L = torch_cuda, backend.lib()
    s, (th, fc), dtype = cell
    pred, host, P = _inputs(torch, cell)
    b = tc.base_case(s)
    V, words = int(np.prod(b["vol"])), tc.words_of(b["ps"])
    cen = tc.centre_list(s, n=max(200, V // 8))
    assert len(cen) * 16 >= V                                  # backend.patch_bits takes its dense route by itself
    cen_d = torch.from_numpy(cen).cuda()
    want_vol = tc.packed_bits(host, fc)
    want = want_vol[(cen[:, 0].astype(np.int64) * b["vol"][1] + cen[:, 1]) * b["vol"][2] + cen[:, 2]]
    code = backend.pred_dtype_code(pred)
    # the wave per centre, and the thread per voxel
    got = torch.zeros((len(cen), words), dtype=torch.int32, device="cuda")
    backend.check(L.ppp_patch_bits(pred.data_ptr(), code, cen_d.data_ptr(), len(cen), float(fc), got.data_ptr(), ctypes.byref(P), None))
    _same(_u32(got), want, "ppp_patch_bits")
    vol = torch.zeros((V, words), dtype=torch.int32, device="cuda")
    backend.check(L.ppp_patch_bits_volume(pred.data_ptr(), code, float(fc), vol.data_ptr(), ctypes.byref(P), None))
    _same(_u32(vol), want_vol, "ppp_patch_bits_volume")
    # the wrapper on both of its routes, and the empty list
    for route in ("auto", "sparse"):
        monkeypatch.setenv("PPP_PATCH_BITS", route)
        _same(_u32(backend.patch_bits(pred, cen_d, fc, P)), want, "backend.patch_bits (%s)" % route)
        assert tuple(backend.patch_bits(pred, cen_d[:0], fc, P).shape) == (0, words)
    monkeypatch.delenv("PPP_PATCH_BITS")
    # the fused pre-pass (cubic 5 / 7 / 9): its per-voxel table and the gather out of it
    score = torch.zeros(b["vol"], dtype=torch.float32, device="cuda")
    ov_d = torch.from_numpy(b["overlap"].astype(np.uint8)).cuda()
    pre = backend.pred_prepass(pred, ov_d, fc, P, score)
    assert (pre is not None) == (s in ("p5", "p7", "p9"))
    if pre is not None:
        _same(_u32(pre.bits_vol), want_vol, "PredPrepass.bits_vol")
        _same(_u32(backend.patch_bits_from_table(pre.bits_vol, cen_d, P)), want, "patch_bits_from_table")
        assert tuple(backend.patch_bits_from_table(pre.bits_vol, cen_d[:0], P).shape) == (0, words)
    # S5's foreground bits of the same prediction: the double rule, with the mid-channel term, for patch_threshold
    inner = np.argwhere(tc.interior_mask(s))
    inner = inner[np.random.default_rng(len(inner)).permutation(len(inner))[:120]].astype(np.int32)
    rows = torch.from_numpy(np.concatenate([inner, np.roll(inner, 1, axis=0)], axis=1)).cuda()
    lin, bits = backend.patch_fg_bits(pred, rows, P)
    centres = np.stack(np.unravel_index(lin.cpu().numpy(), b["vol"]), axis=1)
    assert len(centres) == len(np.unique(inner, axis=0))
    _same(_u32(bits), tc.fg_bits(host, th, b["ps"], centres), "ppp_patch_fg_bits (double rule)")


# ---- cover and thinning --------------------------------------------------------------------------------------------
def _radslice(s):
    ps, vol, _, _ = tc.SHAPES[s]
    return tuple(slice(p // 2, v - p // 2) for p, v in zip(ps, vol))


@pytest.mark.parametrize("cell", tc.COVER_CELLS, ids=tc.cell_id)
def test_cover_and_thinning_follow_numpys_compare(cell, torch_cuda):
    from patchperpix_amd import backend
    from patchperpix_amd.vote_instances import foreground_cover as fcov
    from patchperpix_amd.vote_instances.ranked_patches import PatchList
    torch, L = torch_cuda, backend.lib()
    s, pair, dtype = cell
    fc = pair[1]
    pred, host, P = _inputs(torch, cell)
    b = tc.base_case(s)
    ps, vol = b["ps"], b["vol"]
    rc, rs = tc.ranked(s, pair, dtype)
    ranked = PatchList(rc.copy(), rs.copy())                   # (the shared arrays are read-only)
    mask = tc.mask_to_cover(s)
    radslice, rad = _radslice(s), np.array([p // 2 for p in ps])
    V, words = int(np.prod(vol)), tc.words_of(ps)
    bits_vol = torch.zeros((V, words), dtype=torch.int32, device="cuda")
    backend.check(L.ppp_patch_bits_volume(pred.data_ptr(), backend.pred_dtype_code(pred), float(fc), bits_vol.data_ptr(),
                                          ctypes.byref(P), None))
    lin_h = ranked.lin(vol)
    lin = torch.from_numpy(lin_h).cuda()
    never = torch.from_numpy(fcov.never_selected(b["overlap"], lin_h, rs, False)).cuda()
    for sparse in (True, False):
        kw = tc.flags(pair, select_patches_for_sparse_data=sparse)
        want = tc.cover(s, pair, dtype, sparse=sparse)
        assert sparse or len(fcov._pix_thresholds(ps, kw)) >= 2               # the ladder runs
        # rows in rank order
        sel, n = fcov.computeForegroundCover(b["overlap"], mask.copy(), ps, ranked, radslice, pred, rad, None, None, silent=True, **kw)
        _same(sel.coords, rc[want], "cover, rows in rank order, sparse=%s" % sparse)
        # a bit row per voxel
        m = torch.from_numpy(mask.astype(np.uint8)).cuda()
        chosen, _ = fcov.greedy_cover_device(m, bits_vol, lin, never, fcov._pix_thresholds(ps, kw), radslice, P, bits_first_voxel=0)
        _same(np.flatnonzero(chosen.cpu().numpy()), want, "cover, a bit row per voxel, sparse=%s" % sparse)
    # marks
    kw = tc.flags(pair, select_patches_for_sparse_data=True, mark_close_neighboorhood=True)
    assert fcov.marks_on_device(vol, kw)
    sel, _ = fcov.computeForegroundCover(b["overlap"], mask.copy(), ps, ranked, radslice, pred, rad, None, None, silent=True, **kw)
    _same(sel.coords, rc[tc.cover(s, pair, dtype, mark=True)], "cover with marks")
    # thinning of the (sparse) cover
    cover = PatchList(rc[tc.cover(s, pair, dtype)], rs[tc.cover(s, pair, dtype)])
    thin, _ = fcov.thinOutForegroundCover(mask.copy(), cover, radslice, pred, rad, ps, **tc.flags(pair))
    _same(thin.coords, cover.coords[tc.thinned(s, pair, dtype)], "thinning")


# ---- pack scan and the paints -----------------------------------------------------------------------------------------
def _components_on_device(torch, cell, extra=()):
    s, pair, dtype = cell
    ccs = [list(cc) for cc in tc.components(s, pair, dtype)]
    for node, label in extra:
        ccs[label - 1].append(node)
    nodes, labels = tc.nodes_and_labels(ccs)
    return ccs, nodes, torch.from_numpy(nodes).cuda(), torch.from_numpy(labels).cuda()


@pytest.mark.parametrize("cell", tc.PAINT_CELLS, ids=tc.cell_id)
def test_pack_scan_and_paints_follow_numpys_compare(cell, torch_cuda, monkeypatch):
    from patchperpix_amd import backend
    from patchperpix_amd.vote_instances import graph_to_labeling as g2l
    torch = torch_cuda
    s, (th, fc), dtype = cell
    pred, host, P = _inputs(torch, cell)
    b = tc.base_case(s)
    ps, vol = b["ps"], b["vol"]
    ccs, nodes, nodes_d, labels_d = _components_on_device(torch, cell)
    masks = tc.component_masks(ccs, host, ps, vol, th)
    # pack scan: sizes, one key per pair and shared voxel, their set
    want_sizes, want_keys = tc.pack_scan_model(masks)
    sizes, keys = backend.pack_scan(pred, nodes_d, labels_d, len(ccs), P)
    _same(sizes.cpu().numpy(), want_sizes, "pack_scan sizes")
    shared = masks.sum(0).astype(np.int64)
    assert keys.numel() == int((shared * (shared - 1) // 2).sum())
    _same(torch.unique(keys).cpu().numpy().astype(np.uint64), want_keys, "pack_scan pair keys")
    # the paint of one volume
    inst = torch.zeros(vol, dtype=torch.int32, device="cuda")
    backend.paint_instances(pred, nodes_d, labels_d, inst, P)
    _same(inst.cpu().numpy(), tc.paint_model(masks), "paint_instances")
    # the paint by channel, and the loop over components it stands for
    want = tc.channels_model(masks, backend.PACK_MIN_VOXELS)
    assert want.shape[0] >= 2
    for mode in ("pass", "loop"):
        monkeypatch.setenv("PPP_PACK_CHANNELS", mode)
        _same(g2l.paint_channels(pred, nodes_d, labels_d, len(ccs), vol, P).cpu().numpy(), want, "paint_channels (%s)" % mode)


@pytest.mark.parametrize("cell", tc.PAINT_CELLS, ids=tc.cell_id)
def test_paint_from_rows_follows_numpys_compare_at_the_faces(cell, torch_cuda):
    """rows in the cell's element type; nodes on all six faces: their windows are clipped, nothing wraps around"""
    from patchperpix_amd import backend
    torch = torch_cuda
    s, (th, fc), dtype = cell
    pred, host, P = _inputs(torch, cell)
    b = tc.base_case(s)
    ccs, nodes, nodes_d, labels_d = _components_on_device(torch, cell, extra=tc.face_nodes(s))
    idx = nodes_d.long()
    rows = pred[:, idx[:, 0], idx[:, 1], idx[:, 2]].t().contiguous()
    assert rows.dtype == getattr(torch, dtype) and tuple(rows.shape) == (len(nodes), int(np.prod(b["ps"])))
    inst = torch.zeros(b["vol"], dtype=torch.int32, device="cuda")
    backend.paint_patch_rows(rows, nodes_d, labels_d, inst, P)
    want = tc.paint_model(tc.component_masks(ccs, host, b["ps"], b["vol"], th))
    _same(inst.cpu().numpy(), want, "paint_patch_rows")
    inner = tc.paint_model(tc.component_masks(tc.components(s, (th, fc), dtype), host, b["ps"], b["vol"], th))
    assert (want != inner).any()                               # the face nodes painted something


# ---- ids per slice --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,K", [(1, 1000), (2, 257), (3, 5)])
def test_label_slice_renumber_equals_numpy(seed, K, torch_cuda):
    """ranks over the stack ascending by (slice, key); empty slices, a slice of unlabelled nodes only, unlabelled nodes"""
    from patchperpix_amd import backend
    torch = torch_cuda
    rng = np.random.default_rng(seed)
    Z, Y, X = 9, 30, 40
    P = backend.make_params((Z, Y, X), (1, 5, 5), **tc.flags((0.5, 0.5)))
    n_comp = rng.integers(1, 6, Z)
    n_comp[[1, 4, Z - 1]] = 0                                    # slices without a component
    first = np.concatenate([[1], 1 + np.cumsum(n_comp)])          # first rank of every slice
    live = np.flatnonzero(n_comp)
    z_more = rng.choice(live, K)
    z = np.concatenate([np.repeat(live, n_comp[live]), z_more])                        # every component has a node
    comp = np.concatenate([np.concatenate([np.arange(n_comp[k]) for k in live]), rng.integers(0, 1 << 30, K) % n_comp[z_more]])
    labels = (first[z] + comp).astype(np.int32)
    unl = rng.random(len(z)) < 0.2
    unl[:int(n_comp.sum())] = False
    labels[unl] = 0
    z = np.concatenate([z, np.full(3, 4)])                       # slice 4: unlabelled nodes only
    labels = np.concatenate([labels, np.zeros(3, np.int32)])
    order = rng.permutation(len(z))
    z, labels = z[order], labels[order]
    nodes = np.stack([z, rng.integers(0, Y, len(z)), rng.integers(0, X, len(z))], 1).astype(np.int32)
    want = np.where(labels > 0, labels - first[z] + 1, 0)
    nodes_d, labels_d = torch.from_numpy(nodes).cuda(), torch.from_numpy(labels.copy()).cuda()
    slice_max = backend.label_slice_renumber(nodes_d, labels_d, P)
    _same(labels_d.cpu().numpy(), want, "labels")
    _same(slice_max.cpu().numpy(), n_comp, "per-slice maxima")
    empty = backend.label_slice_renumber(nodes_d[:0], labels_d[:0], P)
    assert not empty.cpu().numpy().any()


# ---- end to end -------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _vote(torch, cell, mws, **extra):
    from patchperpix_amd.vote_instances import vote_instances as vi
    s, pair, dtype = cell
    b = tc.base_case(s)
    pred, _, _ = _inputs(torch, cell)
    return vi.to_instance_seg(pred, b["foreground"].copy(), b["foreground"].copy(), b["numinst"].copy(), list(b["ps"]),
                              **tc.flags(pair, mws=mws, **extra))


def _same_result(got, res, ref, what):
    inst, fg = got
    assert inst.dtype == ref["instances"].dtype, what
    _same(inst, ref["instances"], what + ": instances")
    _same(fg, ref["foreground"], what + ": foreground")
    assert tc.n_instances(inst) >= tc.MIN_INSTANCES, what
    _same(res[0], ref["pairs"], what + ": pair rows")
    _same(_bits(res[1]), _bits(ref["aff"]), what + ": affinities")


@pytest.mark.parametrize("cell", tc.E2E_CELLS, ids=tc.cell_id)
@pytest.mark.parametrize("mws", [False, True], ids=["cc", "mws"])
def test_end_to_end_equals_the_oracle(mws, cell, torch_cuda, monkeypatch):
    torch = torch_cuda
    ref = tc.e2e_expected(*cell, mws)
    runs = [{"PPP_PIPELINE": "fused"}, {"PPP_PIPELINE": "stages"}]
    if cell[0] == "p5":
        runs.insert(1, {"PPP_PIPELINE": "fused", "PPP_PRED_PREPASS": "0"})           # (the default: 1)
    for env in runs:
        monkeypatch.delenv("PPP_PRED_PREPASS", raising=False)
        _set_env(monkeypatch, env)
        _same_result(_vote(torch, cell, mws), _vote(torch, cell, mws, return_intermediates=True), ref, str(env))


def test_tiled_assembly_equals_the_oracle(torch_cuda):
    from patchperpix_amd import tiling
    torch = torch_cuda
    cell, mws = ("p5", (0.6, 0.3), "float32"), True
    s, pair, _ = cell
    b = tc.base_case(s)
    ref = tc.e2e_expected(*cell, mws)
    pred, _, _ = _inputs(torch, cell)

    def run(**extra):
        return tiling.assemble(pred, 0, b["vol"], b["foreground"].copy(), b["foreground"].copy(), b["numinst"].copy(), list(b["ps"]),
                               tiling.plan_slabs(b["vol"][0], 1), _yx_tiles=(2, 2), **tc.flags(pair, mws=mws, **extra))
    _same_result(run(), run(return_intermediates=True), ref, "tiling.assemble, 2 x 2 tiles")


@pytest.mark.parametrize("mws", [False, True], ids=["cc", "mws"])
def test_stack_of_slices_equals_the_oracle_per_slice(mws, torch_cuda):
    from patchperpix_amd.vote_instances import vote_instances as vi
    s, pair, _ = tc.STACK
    c = tc.stack_case()
    refs = tc.stack_expected(mws)

    def run(**extra):
        return vi.to_instance_seg(c["pred"].copy(), c["foreground"].copy(), c["foreground"].copy(), c["numinst"].copy(),
                                  list(tc.SHAPES[s][0]), independent_slices=True, **tc.flags(pair, mws=mws, **extra))
    inst, fg = run()
    res = run(return_intermediates=True)
    assert len(res) == len(refs) == 3
    for k, ref in enumerate(refs):
        _same_result((inst[k:k + 1], fg[k:k + 1]), res[k], ref, "slice %d" % k)
