"""GPU (MI355X): a device ``torch.bfloat16`` prediction through every entry that reads the prediction.

The inputs are the committed goldens' ``pred_f16`` rounded ONCE to bfloat16 by torch; the goldens'
recorded outputs do not apply to those values.  What is compared, always as bit patterns:
 (a) the CPU oracle run on the values widened to float32, and
 (b) the device run on the float32 tensor holding the same values.
bfloat16 widens to float32 exactly, so the tolerance is 0 ulp everywhere."""
import ctypes
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN_DIR, Golden

pytestmark = pytest.mark.gpu

# volume / patch: the smallest at which each kernel family is selected (tests/test_gpu_parity.py)
STAGE_GOLDENS = ["c3d_p3_cells", "c3d_p5_thin_mws", "c3d_p7_thin_mws", "c3d_p9_cells", "c2d_p25_cells",
                 "c2d_p5_th09_inv"]
RUN = dict(debug=False, isbiHack=False, save_no_intermediates=True, sample=1.0, result_folder="/tmp",
           affinities="x.zarr")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert backend.device_count() >= 1
    return torch


def _to_bf16(a):
    """host array -> CPU bfloat16 tensor (one rounding, torch's round-to-nearest-even)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Case:
    """a golden's fields with the prediction rounded to bfloat16: .bf (CPU bf16 tensor), .wide (the same
    values as a float32 ndarray)"""

    def __init__(self, name=None, synth_case=None, ps=None, kw=None):
        if name is not None:
            g = self.golden = Golden(name)
            self.bf = _to_bf16(g.z["pred_f16"])
            self.f16 = g.z["pred_f16"]
            self.foreground, self.numinst, self.ps, self.kw = g.foreground, g.numinst, g.patchshape, g.kw
        else:
            self.golden = None
            self.f16 = synth_case["pred"].astype(np.float16)
            self.bf = _to_bf16(self.f16)
            self.foreground, self.numinst, self.ps, self.kw = synth_case["foreground"], synth_case["numinst"], list(ps), kw
        self.wide = self.bf.float().numpy()
        self.overlap = 1 * (self.numinst > 1)


_CASES, _ORACLE = {}, {}


def _case(name):
    if name not in _CASES:
        if name == "aniso_p377":
            from patchperpix_amd import synth
            from tests_flags import FLYLIGHT
            ps = (3, 7, 7)
            _CASES[name] = Case(synth_case=synth.make_case((14, 18, 20), ps, seed=3, cell=[5, 8, 8], overlap_frac=0.02),
                                ps=ps, kw=dict(FLYLIGHT))
        else:
            _CASES[name] = Case(name)
    return _CASES[name]


def _oracle(name):
    """the oracle on the widened values: computed once per case, shared, never modified"""
    if name not in _ORACLE:
        from oracle import ppp_oracle as orc
        c = _case(name)
        _ORACLE[name] = orc.to_instance_seg(c.wide, c.foreground.copy(), c.foreground.copy(), c.numinst.copy(), c.ps, **c.kw)
    return _ORACLE[name]


def _stages(torch, pred, overlap, ps, kw, pairs, cross=True):
    """S1 / S2 / S5 through backend on the tensor `pred` as it is: consensus planes, scores, pair
    affinities from every S2 / S5 kernel that serves the shape (one key each), the S1 kernel's name.
    cross: the kernels of a stage agree with each other bit for bit -- on finite consensus values; with
    an infinite one a masked term is inf * 0 in one kernel and skipped in another, so the planted-values
    test compares kernel by kernel (bfloat16 against float32) instead."""
    from patchperpix_amd import backend
    P = backend.make_params(tuple(pred.shape[1:]), ps, **kw)
    ov = _dev(torch, (overlap > 0).astype(np.uint8)) if P.use_overlap else None
    cons = backend.consensus(pred, ov, P)
    out = dict(s1_kernel=backend.lib().ppp_consensus_kernel_name().decode(), cons=cons.cpu().numpy())
    out["score"] = backend.rank_patches(pred, cons, ov, P).cpu().numpy()
    if backend.rank_vm_available(P):
        vm0, Pv0 = backend.cons_to_voxel_major(cons, P)
        out["score_vm"] = backend.rank_patches(pred, vm0, ov, Pv0).cpu().numpy()
        assert not cross or np.array_equal(_bits(out["score"]), _bits(out["score_vm"]))
    if pairs is not None and len(pairs):
        pd = _dev(torch, np.ascontiguousarray(pairs, dtype=np.uint32).view(np.int32))
        out["aff"] = backend.patch_graph(pred, cons, pd, P).cpu().numpy()
        order = backend.pair_order(pd, P)
        vm, Pv = backend.cons_to_voxel_major(cons, P)
        out["aff_vm"] = backend.patch_graph(pred, vm, pd, Pv, order=order).cpu().numpy()
        assert not cross or np.array_equal(_bits(out["aff"]), _bits(out["aff_vm"]))
        if P.px in (3, 5, 7, 9) or (P.px == 25 and P.pz == 1):
            out["aff_pa"] = backend.patch_graph_by_patch(pred, vm, pd, Pv).cpu().numpy()
            assert not cross or np.array_equal(_bits(out["aff"]), _bits(out["aff_pa"]))
            os.environ["PPP_PA_LCG_BYTES"] = "65536"           # (the LCG masks cut into batches)
            try:
                out["aff_pa_batched"] = backend.patch_graph_by_patch(pred, vm, pd, Pv).cpu().numpy()
            finally:
                del os.environ["PPP_PA_LCG_BYTES"]
            assert not cross or np.array_equal(_bits(out["aff"]), _bits(out["aff_pa_batched"]))
    return out


def _vi():
    from patchperpix_amd.vote_instances import vote_instances as vi
    return vi


def _seg(c, pred, **extra):
    return _vi().to_instance_seg(pred, c.foreground.copy(), c.foreground.copy(), c.numinst.copy(), c.ps,
                                 **dict(c.kw, **RUN, **extra))


# ---- 1. stage by stage -----------------------------------------------------------------------
@pytest.mark.parametrize("name", STAGE_GOLDENS + ["aniso_p377"])
def test_stages_equal_the_oracle_and_the_float32_tensor(name, torch_cuda):
    from oracle import ppp_oracle as orc
    from patchperpix_amd import backend
    torch = torch_cuda
    c, ref = _case(name), _oracle(name)
    assert "aff" in ref and len(np.unique(ref["instances"])) > 2          # a non-trivial case ...
    # ... that the rounding changes: not the consensus of the float16 values (the golden's recorded one)
    pos = orc.positive_planes(ref["cons"], c.ps)
    if c.golden is None:
        assert not np.array_equal(_bits(orc.consensus(c.f16.astype(np.float32), c.overlap, c.ps, **c.kw)), _bits(ref["cons"]))
    elif c.golden.has("cons_pos"):
        assert not np.array_equal(_bits(pos), _bits(c.golden["cons_pos"]))
    else:
        assert hashlib.sha256(np.ascontiguousarray(pos).tobytes()).hexdigest() != str(c.golden["cons_pos_sha256"])
    got = _stages(torch, c.bf.cuda(), c.overlap, c.ps, c.kw, ref["pairs"])
    wide = _stages(torch, _dev(torch, c.wide), c.overlap, c.ps, c.kw, ref["pairs"])
    Ph = backend.make_params(tuple(c.bf.shape[1:]), c.ps, **c.kw)
    backend.consensus(_dev(torch, c.f16), _dev(torch, (c.overlap > 0).astype(np.uint8)) if Ph.use_overlap else None, Ph)
    half = backend.lib().ppp_consensus_kernel_name().decode()
    assert got["s1_kernel"] == half == wide["s1_kernel"]                  # the type moves no case to another family
    assert np.array_equal(_bits(got["cons"]), _bits(pos))
    assert np.array_equal(_bits(got["score"]), _bits(ref["scores"]))
    assert np.array_equal(_bits(got["aff"]), _bits(ref["aff"]))
    for k in ("cons", "score", "aff"):
        assert np.array_equal(_bits(got[k]), _bits(wide[k])), k
    # pair rows and the instance map: the oracle's, and the float32 tensor's
    pairs, aff = _seg(c, c.bf.cuda(), return_intermediates=True)
    assert np.array_equal(pairs, ref["pairs"]) and np.array_equal(_bits(aff), _bits(ref["aff"]))
    inst, _ = _seg(c, c.bf.cuda())
    assert np.array_equal(inst, ref["instances"])
    assert np.array_equal(inst, _seg(c, _dev(torch, c.wide))[0])


# ---- 2. special values -------------------------------------------------------------------------
# 2^-20 and 2^-133 do not survive a round trip through float16: a hidden conversion would show.
# Every value goes through the one rounding every input of this file goes through (torch, to nearest
# even).  All but one are bfloat16 values already; 0.501953125 = 0.5 + 2^-9 lies half way between 0.5 and
# its upper bfloat16 neighbour 0.50390625 = 0.5 + 2^-8 and rounds to 0.5 -- so that neighbour is planted too
# (0.498046875 = 0.5 - 2^-9 IS the lower neighbour: the spacing halves below 0.5).
SPECIAL = [0.5, 0.498046875, 0.501953125, 0.50390625, 0.0, 1.0, 1.0078125, -0.0, -0.25, 2.0 ** -20, 2.0 ** -133,
           float("inf")]
ROUNDS_TO = {0.501953125: 0.5}


def _planted(c, per_value=56):
    """a copy of the case's bf16 prediction with every SPECIAL value in `per_value` elements: the first
    8 of each at the centre channel of interior foreground voxels, the rest anywhere (seeded)"""
    import torch
    rng = np.random.default_rng(7)
    bf = c.bf.clone()
    C, shape = bf.shape[0], tuple(bf.shape[1:])
    rad = [p // 2 for p in c.ps]
    inner = np.zeros(shape, dtype=bool)
    inner[tuple(slice(r, s - r) for r, s in zip(rad, shape))] = True
    centres = np.flatnonzero((inner & (c.foreground > 0)).ravel())
    assert len(centres) >= 8 * len(SPECIAL)
    centres = rng.permutation(centres)
    V = int(np.prod(shape))
    flat = bf.view(C, V)
    anywhere = rng.permutation(C * V)[:len(SPECIAL) * (per_value - 8)].reshape(len(SPECIAL), -1)
    for i, v in enumerate(SPECIAL):
        val = torch.tensor(v, dtype=torch.float64).to(torch.bfloat16)
        assert float(val) == ROUNDS_TO.get(v, v)                          # exactly representable
        flat[C // 2, torch.from_numpy(centres[8 * i:8 * i + 8])] = val
        flat.view(-1)[torch.from_numpy(anywhere[i])] = val
    for v in SPECIAL:     # (later plantings may overwrite earlier ones: still at least 50 of each)
        same = (bf.view(torch.int16) == torch.tensor(v, dtype=torch.float64).to(torch.bfloat16).view(torch.int16)).sum()
        assert int(same) >= 50, v
    return bf


@pytest.mark.parametrize("name", ["c3d_p5_thin_mws", "c3d_p9_cells"])
def test_special_values_take_the_bits_of_the_float32_tensor(name, torch_cuda, monkeypatch):
    from patchperpix_amd import backend
    torch = torch_cuda
    c, ref = _case(name), _oracle(name)
    P = backend.make_params(tuple(c.bf.shape[1:]), c.ps, **c.kw)
    bad = _planted(c)
    bad_d, wide_d = bad.cuda(), bad.float().cuda()
    assert backend.pred_check(bad_d, P) == 2
    bits_bf = backend.NOTES["pred_unclean_bits"]
    assert backend.pred_check(wide_d, P) == 2
    assert bits_bf == backend.NOTES["pred_unclean_bits"] == 3
    got = _stages(torch, bad_d, c.overlap, c.ps, c.kw, ref["pairs"], cross=False)
    wide = _stages(torch, wide_d, c.overlap, c.ps, c.kw, ref["pairs"], cross=False)
    assert got["s1_kernel"] == wide["s1_kernel"] == "consensus_v3_kernel"
    assert set(got) == set(wide) and {"cons", "score", "score_vm", "aff", "aff_vm", "aff_pa"} <= set(got)
    for k in got:
        if k != "s1_kernel":
            assert np.array_equal(_bits(got[k]), _bits(wide[k])), k
    # the same bits from the kernels that test the values against the threshold one by one
    ct = _dev(torch, np.argwhere(c.foreground > 0).astype(np.int32))
    assert torch.equal(backend.patch_bits(bad_d, ct, 0.5, P), backend.patch_bits(wide_d, ct, 0.5, P))      # per voxel
    few = ct[::97].contiguous()
    assert torch.equal(backend.patch_bits(bad_d, few, 0.5, P), backend.patch_bits(wide_d, few, 0.5, P))    # per centre
    # the untouched copy is clean, and the short classification gives what the general kernel gives
    clean_d = c.bf.cuda()
    assert backend.pred_check(clean_d, P) == 1
    ov = _dev(torch, (c.overlap > 0).astype(np.uint8))
    short = backend.consensus(clean_d, ov, P).cpu().numpy()
    monkeypatch.setenv("PPP_S1_CLEAN", "0")
    backend.reload_env()
    general = backend.consensus(clean_d, ov, P).cpu().numpy()
    assert np.array_equal(_bits(short), _bits(general))


# ---- 3. ppp_pred_check on 1-d buffers: head / 16-byte body / tail --------------------------------
def test_pred_check_flags_every_position_of_short_buffers(torch_cuda):
    from patchperpix_amd import backend
    torch = torch_cuda
    L = backend.lib()
    P = backend.make_params((4, 4, 4), (3, 3, 3), patch_threshold=0.5)
    jobs = [(n, start, pos, bad) for n in range(1, 41) for start in range(8) for pos in range(n) for bad in (2.0, 0.5)]
    flags = {}
    for dtype, code in ((torch.bfloat16, backend.BF16), (torch.float32, backend.F32)):
        room = torch.full((64 + 16,), 0.25, dtype=dtype, device="cuda")
        es = room.element_size()
        first = ((-room.data_ptr()) % 16) // es                 # element index of a 16-byte boundary
        assert (room.data_ptr() + first * es) % 16 == 0
        out = torch.full((len(jobs),), -1, dtype=torch.int32, device="cuda")
        for j, (n, start, pos, bad) in enumerate(jobs):
            room[first + start + pos] = bad
            rc = L.ppp_pred_check(room.data_ptr() + (first + start) * es, code, n, out.data_ptr() + 4 * j,
                                  ctypes.byref(P), backend._stream())
            assert rc == 0, L.ppp_last_error()
            room[first + start + pos] = 0.25
        flags[dtype] = out.cpu().numpy()
    want = np.array([1 if bad == 2.0 else 2 for _, _, _, bad in jobs], dtype=np.int32)
    assert np.array_equal(flags[torch.float32], want)
    assert np.array_equal(flags[torch.bfloat16], flags[torch.float32])
    # ... and a buffer without a bad element is clean at every length and offset
    room = torch.full((80,), 0.25, dtype=torch.bfloat16, device="cuda")
    first = ((-room.data_ptr()) % 16) // 2
    out = torch.full((40 * 8,), -1, dtype=torch.int32, device="cuda")
    for n in range(1, 41):
        for start in range(8):
            assert L.ppp_pred_check(room.data_ptr() + 2 * (first + start), backend.BF16, n,
                                    out.data_ptr() + 4 * ((n - 1) * 8 + start), ctypes.byref(P), backend._stream()) == 0
    assert not out.cpu().numpy().any()


# ---- 4. to_instance_seg end to end --------------------------------------------------------------
@pytest.mark.parametrize("name", ["c3d_p5_thin_mws", "c3d_p7_thin_mws"])
@pytest.mark.parametrize("how", ["fused", "stages", "tiled", "cover_host", "thin_host"])
def test_end_to_end_equals_the_oracle(name, how, torch_cuda, monkeypatch):
    from patchperpix_amd import backend
    c, ref = _case(name), _oracle(name)
    env = {"stages": ("PPP_PIPELINE", "stages"), "cover_host": ("PPP_COVER", "host"), "thin_host": ("PPP_THIN", "host")}
    if how in env:
        monkeypatch.setenv(*env[how])
    extra = dict(_n_slabs=2, _yx_tiles=(2, 2)) if how == "tiled" else {}
    pred = c.bf.cuda()
    inst, fg = _seg(c, pred, **extra)
    assert backend.NOTES["pred_dtype"] == "bfloat16"
    assert inst.dtype == np.uint16 and np.array_equal(inst, ref["instances"])
    assert len(np.unique(inst)) > 2


def _scale_fixture(torch, name):
    """tests/golden/gen_bf16_fixture.py: the oracle's instance map of a shape that takes it minutes; the
    input regenerated on the device and checked by the CRC of its 16-bit patterns"""
    from patchperpix_amd import backend, flags as F, synth
    z = np.load(os.path.join(GOLDEN_DIR, "scale_bf16_%s.npz" % name))
    shape, ps = tuple(int(v) for v in z["shape"]), [int(v) for v in z["patchshape"]]
    kw = dict(F.FLYLIGHT_CC, _instances_dtype=np.uint32)
    lab = synth.cell_labels(shape, [int(z["cell"])] * 3, seed=int(z["seed"]))
    pred = backend.synth_pred(_dev(torch, lab.astype(np.int32)), backend.make_params(shape, ps, **kw),
                              seed=int(z["seed"]), f16=True).to(torch.bfloat16)
    assert zlib.crc32(pred.view(torch.int16).cpu().numpy().tobytes()) == int(z["pred_bf16_crc32"])    # same input
    assert int(z["n_instances"]) > 5
    return shape, ps, kw, lab != 0, pred, z["instances"]


def test_consensus_cache_equals_the_oracle(torch_cuda, monkeypatch):
    from patchperpix_amd import backend
    shape, ps, kw, fg, pred, want = _scale_fixture(torch_cuda, "cache_p5")
    monkeypatch.setenv("PPP_VM_POISON", "1")
    backend.NOTES.pop("cons_cache_gb", None)
    got = _vi().to_instance_seg(pred, fg.copy(), fg.copy(), fg.astype(np.uint8), ps,
                                **dict(kw, _cons_cache=True, _n_slabs=2, _yx_tiles=(2, 2)))[0]
    assert "cons_cache_gb" in backend.NOTES
    assert np.array_equal(got, want)


def test_ring_sweep_equals_the_oracle(torch_cuda, monkeypatch):
    from patchperpix_amd import backend
    shape, ps, kw, fg, pred, want = _scale_fixture(torch_cuda, "ring_p5")
    n = -(-shape[0] // 8)
    ring = -(-shape[0] // n) + 28
    monkeypatch.setenv("PPP_VM_POISON", "1")
    backend.NOTES.pop("ring_z", None)
    got = _vi().to_instance_seg(pred, fg.copy(), fg.copy(), fg.astype(np.uint8), ps,
                                **dict(kw, _cons_cache=False, _ring_z=ring, _n_slabs=n, _yx_tiles=(2, 2)))[0]
    assert backend.NOTES.get("ring_z") == ring
    assert np.array_equal(got, want)


def test_sparse_item_lists_on_tubes_equal_the_oracle(torch_cuda):
    from oracle import ppp_oracle as orc
    from patchperpix_amd import backend, synth
    from patchperpix_amd.flags import FLYLIGHT
    shape, ps = (13, 40, 96), [7, 7, 7]            # tests/test_s1_sparse_gpu.py, its smallest tubes case
    case = synth.make_case(shape, ps, seed=4, kind="tubes", n_tubes=3, radius=2.0, overlap_frac=0.03)
    c = Case(synth_case=case, ps=ps, kw=dict(FLYLIGHT))
    ref = orc.to_instance_seg(c.wide, c.foreground.copy(), c.foreground.copy(), c.numinst.copy(), ps, **c.kw)
    assert len(np.unique(ref["instances"])) > 2
    for k in ("s1_items", "s1_active_items", "s1_list_launches"):
        backend.NOTES.pop(k, None)
    inst, _ = _seg(c, c.bf.cuda(), _s1_sparse=True)
    assert backend.NOTES["s1_list_launches"] >= 1 and 0 < backend.NOTES["s1_active_items"] < backend.NOTES["s1_items"]
    assert np.array_equal(inst, ref["instances"])


# ---- 5. cuda=False: the NumPy semantics ----------------------------------------------------------
@pytest.mark.parametrize("name", ["c3d_p3_blobs", "c2d_p5_th09"])
def test_numpy_semantics_equal_their_oracle(name, torch_cuda):
    from oracle import ppp_oracle as orc
    from oracle import ppp_oracle_np as onp
    z = np.load(os.path.join(GOLDEN_DIR, "np_%s.npz" % name))
    bf = _to_bf16(z["pred_f16"])
    pred = bf.float().numpy()
    fg, numinst, ps = z["foreground"].astype(bool), z["numinst"], [int(p) for p in z["patchshape"]]
    kw = json.loads(str(z["flags"]))
    kw.setdefault("max_total_patch_distance_in_ps_multiples", 2)
    kw.update(save_no_intermediates=True, result_folder="/tmp")
    th = float(kw["patch_threshold"])
    overlap = 1 * (numinst > 1)
    mask = fg.copy()
    mask[overlap > 0] = 0
    # the oracle's stages in the order of tests/test_numpy_semantics.py::test_oracle_stages_match_the_reference
    votes = onp.consensus(pred, fg, ps, th)
    rc, rs = onp.ranked(*onp.rank(pred, fg, votes, ps, th))
    chosen = rc[orc.foreground_cover(rc, rs, overlap, mask, pred, ps, **kw)]
    if not kw.get("skipThinCover", False):
        chosen = chosen[orc.thin_cover(chosen, mask, pred, ps, **kw)]
    srt = chosen[np.argsort(chosen[:, 2], kind="stable")]
    rows, w = onp.patch_graph(pred, mask, overlap, votes, srt, ps, th, include_single=kw["includeSinglePatchCCS"])
    want = orc.label(rows.astype(np.uint32), w, pred, ps, fg.shape, keep_zero_edges=True, **kw)
    assert len(np.unique(want)) > 2
    inst, fgo = _vi().to_instance_seg(bf.cuda(), fg.copy(), fg.copy(), numinst.copy(), ps, **dict(kw, cuda=False))
    assert inst.dtype == np.uint16 and np.array_equal(inst, want)
    # (the device stages on their own: votes and ranks)
    from patchperpix_amd.vote_instances import numpy_semantics as ns
    fd = _dev(torch_cuda, fg.astype(np.uint8))
    v = ns.create_consensus_array(bf.cuda(), fd, ps, **kw)
    assert np.array_equal(v.cpu().numpy(), votes)
    ranked, _ = ns.rank_patches(bf.cuda(), fd, v, fg, ps, **kw)
    assert np.array_equal(ranked.coords, rc) and np.array_equal(ranked.scores.astype(np.int64), rs)


# ---- 6. independent_slices -------------------------------------------------------------------
def test_independent_slices_equal_the_single_calls(torch_cuda):
    from patchperpix_amd import synth
    from patchperpix_amd.flags import FLYLIGHT
    ps = (1, 5, 5)
    cases = [synth.make_case((1, 44, 48), ps, seed=s, cell=[1, 15, 15], overlap_frac=0.02 * (s % 2)) for s in (5, 6, 7)]
    bf = _to_bf16(np.concatenate([c["pred"] for c in cases], axis=1).astype(np.float16)).cuda()
    fg = np.concatenate([c["foreground"] for c in cases])
    ni = np.concatenate([c["numinst"] for c in cases])
    kw = dict(FLYLIGHT, **RUN)
    inst, fgo = _vi().to_instance_seg(bf, fg.copy(), fg.copy(), ni.copy(), ps, independent_slices=True, **kw)
    res = _vi().to_instance_seg(bf, fg.copy(), fg.copy(), ni.copy(), ps, independent_slices=True,
                                **dict(kw, return_intermediates=True))
    assert all(inst[k].any() for k in range(3))
    for k in range(3):
        sl = slice(k, k + 1)
        one = bf[:, sl].contiguous()
        i1, f1 = _vi().to_instance_seg(one, fg[sl].copy(), fg[sl].copy(), ni[sl].copy(), ps, **kw)
        assert np.array_equal(inst[sl], i1) and np.array_equal(fgo[sl], f1), k
        p1, a1 = _vi().to_instance_seg(one, fg[sl].copy(), fg[sl].copy(), ni[sl].copy(), ps,
                                       **dict(kw, return_intermediates=True))
        assert np.array_equal(res[k][0], p1) and np.array_equal(_bits(res[k][1]), _bits(a1)), k


# ---- 7. per-channel outputs ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c3d_p3_per_channel", "c3d_p3_packed_channels"])
def test_per_channel_outputs_equal_the_float32_tensor(name, torch_cuda):
    c = Case(name)
    assert c.kw.get("one_instance_per_channel") or c.kw.get("no_overlap_per_channel")
    got, fg_b = _seg(c, c.bf.cuda())
    want, fg_w = _seg(c, _dev(torch_cuda, c.wide))
    assert got.ndim == 4 and got.any() and len(np.unique(got)) > 2
    assert got.dtype == want.dtype and np.array_equal(got, want) and np.array_equal(fg_b, fg_w)


# ---- 8. direct calls ---------------------------------------------------------------------------
def test_paint_from_a_table_of_bf16_patch_rows(torch_cuda):
    from patchperpix_amd import backend
    torch = torch_cuda
    c, ref = _case("c3d_p5_thin_mws"), _oracle("c3d_p5_thin_mws")
    shape = tuple(c.bf.shape[1:])
    P = backend.make_params(shape, c.ps, **c.kw)
    nodes_h = np.unique(ref["pairs"].reshape(-1, 3).astype(np.int32), axis=0)
    assert len(nodes_h) > 20
    nodes = _dev(torch, nodes_h)
    labels = torch.arange(1, len(nodes_h) + 1, dtype=torch.int32, device="cuda")
    pred = c.bf.cuda()
    idx = nodes.long()
    rows = pred[:, idx[:, 0], idx[:, 1], idx[:, 2]].t().contiguous()
    assert rows.dtype == torch.bfloat16 and rows.shape == (len(nodes_h), pred.shape[0])
    out = {}
    for key, r in (("bf16", rows), ("f32", rows.float())):
        out[key] = backend.paint_patch_rows(r, nodes, labels, torch.zeros(shape, dtype=torch.int32, device="cuda"), P)
    direct = backend.paint_instances(pred, nodes, labels, torch.zeros(shape, dtype=torch.int32, device="cuda"), P)
    assert int(out["bf16"].max()) > 0
    assert torch.equal(out["bf16"], out["f32"]) and torch.equal(out["bf16"], direct)


def test_provider_of_bf16_boxes_through_the_tiled_assembly(torch_cuda):
    from patchperpix_amd import backend, tiling
    torch = torch_cuda
    name = "c3d_p5_thin_mws"
    c, ref = _case(name), _oracle(name)
    pred = c.bf.cuda()
    seen = []

    class Provider:
        def pred_box(self, box):
            z0, z1, y0, y1, x0, x1 = box
            t = pred[:, z0:z1, y0:y1, x0:x1].contiguous()
            seen.append(t.dtype)
            return t
    shape = tuple(pred.shape[1:])
    fg_d = _dev(torch, c.foreground.astype(np.uint8))
    inst, _ = tiling.assemble(Provider(), 0, shape, fg_d, fg_d.clone(), _dev(torch, c.numinst.astype(np.uint8)), c.ps,
                              tiling.plan_slabs(shape[0], 2), _yx_tiles=(2, 2), **dict(c.kw, **RUN))
    assert len(seen) >= 8 and set(seen) == {torch.bfloat16}
    assert np.array_equal(np.asarray(inst), ref["instances"])


# ---- 9. no copy ---------------------------------------------------------------------------------
def test_a_resident_bf16_tensor_is_passed_as_it_is(torch_cuda):
    from patchperpix_amd import backend
    c = _case("c3d_p5_thin_mws")
    t = c.bf.cuda()
    got = backend.to_device_pred(t)
    assert got.data_ptr() == t.data_ptr() and got.dtype == torch_cuda.bfloat16
    backend.NOTES.pop("pred_dtype", None)
    _seg(c, t)
    assert backend.NOTES["pred_dtype"] == "bfloat16"


# ---- 10. the C ABI says no where it must ---------------------------------------------------------
def test_writing_and_bench_entry_points_refuse_bf16_and_unknown_codes_stay_errors(torch_cuda):
    from patchperpix_amd import backend
    torch = torch_cuda
    L = backend.lib()
    P = backend.make_params((8, 8, 8), (7, 7, 7), patch_threshold=0.5)
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    INVALID = -1
    box = (ctypes.c_int32 * 6)(0, 0, 0, 8, 8, 8)
    dims = (ctypes.c_int32 * 3)(8, 8, 8)
    calls = {
        "ppp_synth_pred": lambda: L.ppp_synth_pred(p, p, backend.BF16, 0, 0.9, 0.1, 0.05, 0, ctypes.byref(P), None),
        "ppp_synth_pred_box": lambda: L.ppp_synth_pred_box(p, ctypes.addressof(box), p, backend.BF16, 0, 0.9, 0.1, 0.05,
                                                           ctypes.addressof(dims), ctypes.byref(P), None),
        "ppp_decode_tail": lambda: L.ppp_decode_tail(p, 1, 64, 4, p, 0.0, p, 0.0, p, 0.0, p, p, backend.BF16,
                                                     ctypes.byref(P), None),
        "ppp_counter_calibration": lambda: L.ppp_counter_calibration(p, backend.BF16, 16, p, 16, None),
    }
    for name, call in calls.items():
        assert call() == INVALID, name
        msg = L.ppp_last_error().decode()
        assert "bfloat16" in msg and "2" in msg and name in msg, msg
    assert not buf.any()
    for code in (3, -1):
        assert L.ppp_consensus(p, code, None, p, None, ctypes.byref(P), None) == INVALID
        assert ("bad pred dtype %d" % code) in L.ppp_last_error().decode()
        assert L.ppp_pred_check(p, code, 16, p, ctypes.byref(P), None) == INVALID
