"""GPU (MI355X): every S1 / S2 / S5 kernel family against the oracle across the flag space
(tests/flag_matrix_cases.py), bit for bit (uint32 patterns, 0 ulp), on predictions that hold the float
neighbours of both thresholds.  One parametrised test per stage; an id is family-shape-flags-dtype.

Every cell asserts which kernel served it (ppp_consensus_kernel_name / ppp_rank_kernel_name /
ppp_patch_graph_kernel_name).  Where a family cannot serve a flag set the cell asserts the refusal -- the documented
error or "no kernel" answer -- and, through the backend, which kernel served instead and that its result is the
oracle's.  S2 and S5 cells read the consensus of the default S1 dispatch after it was held to the oracle's."""
import ctypes

import numpy as np
import pytest

import flag_matrix_cases as fm

pytestmark = pytest.mark.gpu

ALL = list(fm.FLAG_SETS)
CUBIC = ("p3", "p5", "p7", "p9")
V3_SETS = [n for n in ALL if fm.v3_serves(n)]
TH05_SETS = [n for n in ALL if fm.th05_variant(n)]
INT_SETS = [n for n in ALL if fm.geo_flags(n)["count_pos_neg"]]

# float16 / bfloat16 rotate over the families: (float16 sets, bfloat16 sets), all non-default
ROTATION = [(("half03_prob", "less06_count"), ("inv07_prob_noov", "raw")),
            (("half09_count", "nonorm_s1"), ("less04_prob", "noov"))]
ROTATION_V3 = (("noov", "nonorm_s1"), ("raw", "nonorm_s5"))          # sets the packed S1 kernel serves

# family -> dict(env: development switches, cells: {shape: flag sets}, rot: shape of the float16 / bfloat16 cells)
S1 = {
    "gather": dict(env={"PPP_CONSENSUS_GENERIC": "1"}, cells={"p3": ALL}, rot="p3"),
    "gather11": dict(env={}, cells={"w11": ALL}, rot="w11"),
    "v2_line": dict(env={"PPP_S1_V3": "0", "PPP_S1_FLAT": "0"}, cells={s: ALL for s in CUBIC + ("p357",)}, rot="p5"),
    "v2_flat": dict(env={"PPP_S1_V3": "0", "PPP_S1_FLAT": "1"}, cells={s: ALL for s in CUBIC}, rot="p7"),
    "v2_general": dict(env={"PPP_S1_V3": "0", "PPP_S1_NO_TH05": "1"}, cells={"p5": TH05_SETS}, rot="p5", v3=True),
    "v3": dict(env={}, cells={s: ALL for s in CUBIC + ("p357",)}, rot="p3", v3=True),
    "v3_vm": dict(env={}, cells={"p5": ALL}, rot="p5", v3=True),
    "lists": dict(env={}, cells={"p5": ALL}, rot="p5", v3=True),
    "wide": dict(env={}, cells={"w25": ALL}, rot="w25"),
    # the packed kernel's one-line-per-run form (every matrix shape takes the flat form by the rule)
    "v3_line": dict(env={"PPP_S1_FLAT": "0"}, cells={s: ALL for s in CUBIC + ("p357",)}, rot="p7", v3=True),
}
S2 = {
    "rank_generic": dict(env={"PPP_RANK_GENERIC": "1"}, cells={"p3": ALL}, rot="p3"),
    "rank_generic11": dict(env={}, cells={"w11": ALL}, rot="w11"),
    "rank_v2": dict(env={}, cells={"p5": ALL, "p357": ALL}, rot="p5"),
    "rank_vm": dict(env={"PPP_RANK_WG": "0"}, cells={**{s: ALL for s in CUBIC}, "w25": ALL, "p357": ["default"]}, rot="p3"),
    "rank_wg": dict(env={}, cells={s: ALL for s in ("p5", "p7", "p9")}, rot="p5"),
}
S5 = {
    "pg_compact": dict(env={}, cells={"p3": ALL, "w11": ALL}, rot="p3"),
    "pg_vm": dict(env={"PPP_PATCH_GRAPH_GENERIC": "1"}, cells={"p5": ALL, "w25": ALL}, rot="p5"),
    "pg_vm2": dict(env={}, cells={"p3": ALL, "p7": ALL, "p357": ALL}, rot="p3"),
    "pa": dict(env={}, cells={**{s: ALL for s in CUBIC}, "w25": ALL}, rot="p3"),
    "pa_big": dict(env={"PPP_PA_CHUNK": "big"}, cells={"p5": ALL, "p7": ["default", "raw"], "p9": ["default", "raw"]}, rot="p5"),
    "pa_small": dict(env={"PPP_PA_CHUNK": "small"}, cells={"p7": ALL}, rot="p7"),          # 7^3: one wave per chunk
    "pa_nobits": dict(env={"PPP_PA_BITS": "0"}, cells={"p7": ALL}, rot="p7"),
    "pa_nolcg": dict(env={"PPP_PA_LCG_BYTES": "0"}, cells={"p5": ALL}, rot="p5"),
}


def _cells(families):
    out = []
    for i, (fam, d) in enumerate(families.items()):
        for shape, names in d["cells"].items():
            out += [(fam, shape, n, "float32") for n in names]
        f16, bf16 = ROTATION_V3 if d.get("v3") else ROTATION[i % 2]
        out += [(fam, d["rot"], n, "float16") for n in f16] + [(fam, d["rot"], n, "bfloat16") for n in bf16]
    # cells that share inputs and oracle outputs next to each other
    order = {n: k for k, n in enumerate(ALL)}
    out.sort(key=lambda c: (list(fm.SHAPES).index(c[1]), fm.DTYPES.index(c[3]), fm.s1_key(c[2]), order[c[2]]))
    return out


S1_CELLS, S2_CELLS, S5_CELLS = _cells(S1), _cells(S2), _cells(S5)
_id = "-".join


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert backend.device_count() >= 1
    return torch


def _hash(t):
    return fm.bits_hash(t.cpu().numpy())


def _set_env(monkeypatch, env):
    from patchperpix_amd import backend
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    backend.reload_env()


_INPUTS = {}        # one entry: the device inputs of the last (shape, prediction)


def _inputs(torch, shape, flag, dtype):
    """(pred, overlap or None, P) on the device for a cell; the overlap mask only where the flags read it"""
    from patchperpix_amd import backend
    b = fm.base_case(shape)
    key = (shape, dtype, tuple(float(v) for v in fm.pinned_values(flag, dtype)))
    if key not in _INPUTS:
        _INPUTS.clear()
        host = fm.prediction(shape, flag, dtype)
        pred = torch.from_numpy(np.array(host)).cuda().to(getattr(torch, dtype))
        assert np.array_equal(pred.float().cpu().numpy().view(np.uint32), host.view(np.uint32))     # an exact narrowing
        _INPUTS[key] = (pred, torch.from_numpy(np.array(b["overlap"])).cuda(),
                        torch.from_numpy(np.array(b["pairs"]).view(np.int32)).cuda())
    pred, ov, pairs = _INPUTS[key]
    P = backend.make_params(b["vol"], b["ps"], **fm.FLAG_SETS[flag])
    assert P.pred_clean == 0
    return pred, (ov if P.use_overlap else None), pairs, P


_CONS = {}          # one entry: the default dispatch's consensus of the last (shape, prediction, S1 flags), held to the oracle


def _consensus(torch, shape, flag, dtype):
    """(compact consensus, P, voxel-major rows, Pv): what S2 and S5 read.  From the library's default S1 dispatch,
    after its bits were compared with the oracle's (so that a wrong S1 fails here and not as an S2 / S5 mismatch)."""
    from patchperpix_amd import backend
    pred, ov, _, P = _inputs(torch, shape, flag, dtype)
    key = (shape, dtype, tuple(float(v) for v in fm.pinned_values(flag, dtype)), fm.s1_key(flag))
    if key not in _CONS:
        _CONS.clear()
        backend.reload_env()
        cons = backend.consensus(pred, ov, P)
        assert _hash(cons) == fm.oracle(shape, flag, dtype)["cons_hash"], "S1 (default dispatch) differs from the oracle"
        vm, _ = backend.cons_to_voxel_major(cons, P)
        _CONS[key] = (cons, vm)
    cons, vm = _CONS[key]
    Pv = P.copy()
    Pv.cons_layout = backend.CONS_VOXEL_MAJOR
    return cons, P, vm, Pv


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    assert got.shape == want.shape, what
    bad = np.count_nonzero(got != want)
    assert bad == 0, "%s: %d of %d entries differ from the oracle" % (what, bad, got.size)


def _same_cons(torch, cons, shape, flag, dtype, what):
    if _hash(cons) != fm.oracle(shape, flag, dtype)["cons_hash"]:
        _same_bits(cons.cpu().numpy(), fm.oracle_cons_planes(shape, flag, dtype), what)
        raise AssertionError(what + ": hash differs")


# ---- S1 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,shape,flag,dtype", S1_CELLS, ids=[_id(c) for c in S1_CELLS])
def test_s1_family_matches_oracle(fam, shape, flag, dtype, torch_cuda, monkeypatch):
    from patchperpix_amd import backend
    torch, L = torch_cuda, backend.lib()
    pred, ov, _, P = _inputs(torch, shape, flag, dtype)
    what = _id((fam, shape, flag, dtype))
    _set_env(monkeypatch, S1[fam]["env"])
    name = lambda: L.ppp_consensus_kernel_name().decode()      # noqa: E731
    Pv = P.copy()
    Pv.cons_layout = backend.CONS_VOXEL_MAJOR
    if fam in ("v3", "v3_line", "v3_vm", "lists"):
        assert L.ppp_consensus_writes_voxel_major(ctypes.byref(Pv)) == (1 if fm.v3_serves(flag) else 0)
    if fam in ("gather", "gather11", "v2_line", "v2_flat", "v2_general", "wide"):
        cons = backend.consensus(pred, ov, P)
        assert name() == {"gather": "consensus_gather_kernel", "gather11": "consensus_gather_kernel",
                          "wide": "consensus_wide_kernel"}.get(fam, "consensus_v2_kernel")
        _same_cons(torch, cons, shape, flag, dtype, what)
    elif fam in ("v3", "v3_line"):
        cons = backend.consensus(pred, ov, P)
        # refused: the general kernel of the line-run family serves, and is the oracle's too
        assert name() == ("consensus_v3_kernel" if fm.v3_serves(flag) else "consensus_v2_kernel")
        _same_cons(torch, cons, shape, flag, dtype, what)
    elif fam == "v3_vm":
        want = fm.voxel_major_from_planes(fm.oracle_cons_planes(shape, flag, dtype), fm.SHAPES[shape][0])
        if fm.v3_serves(flag):
            vm = backend.consensus(pred, ov, Pv)
            assert name() == "consensus_v3_kernel" and backend.direct_voxel_major(P)
        else:
            with pytest.raises(RuntimeError, match="writes VOXEL_MAJOR only with the packed kernel"):
                backend.consensus(pred, ov, Pv)
            assert not backend.direct_voxel_major(P)
            vm, Pv2 = backend.consensus_voxel_major(pred, ov, P)             # compact planes + re-layout
            assert name() == "consensus_v2_kernel" and Pv2.cons_layout == backend.CONS_VOXEL_MAJOR
        _same_bits(vm.cpu().numpy(), want, what)
    elif fam == "lists":
        need = int(L.ppp_consensus_sparse_workspace_bytes(ctypes.byref(P), None))
        with backend.s1_sparse_scope(True):
            cons = backend.consensus(pred, ov, P)
        if fm.v3_serves(flag):
            assert need > 0 and name() == "consensus_v3_kernel<lists>" and backend.consensus_last_items()[2] == 1
        else:
            assert need == 0 and name() == "consensus_v2_kernel"              # the dense call served
            out = torch.empty_like(cons)
            rc = L.ppp_consensus_sparse(backend._dev_ptr(pred), backend.pred_dtype_code(pred), backend._dev_ptr(ov),
                                        backend._dev_ptr(out), None, ctypes.byref(P), None, 0, None, 1, backend._stream())
            assert rc != 0 and b"serves the packed kernel only" in L.ppp_last_error()
        _same_cons(torch, cons, shape, flag, dtype, what)
    else:
        raise AssertionError(fam)


# ---- S2 -----------------------------------------------------------------------------------------------------------
S2_KERNEL = {"rank_generic": "rank_kernel", "rank_generic11": "rank_kernel", "rank_v2": "rank_v2_kernel",
             "rank_vm": "rank_vm_kernel", "rank_wg": "rank_wg_kernel"}


@pytest.mark.parametrize("fam,shape,flag,dtype", S2_CELLS, ids=[_id(c) for c in S2_CELLS])
def test_s2_family_matches_oracle(fam, shape, flag, dtype, torch_cuda, monkeypatch):
    from patchperpix_amd import backend
    torch, L = torch_cuda, backend.lib()
    pred, ov, _, _ = _inputs(torch, shape, flag, dtype)
    cons, P, vm, Pv = _consensus(torch, shape, flag, dtype)
    what = _id((fam, shape, flag, dtype))
    want = fm.oracle(shape, flag, dtype)["score"]
    _set_env(monkeypatch, S2[fam]["env"])
    name = lambda: L.ppp_rank_kernel_name().decode()           # noqa: E731
    g = fm.geo_flags(flag)
    if fam in ("rank_generic", "rank_generic11", "rank_v2"):
        score = backend.rank_patches(pred, cons, ov, P)
        assert name() == S2_KERNEL[fam]
        _same_bits(score.cpu().numpy(), want, what)
        return
    cubic = shape in CUBIC
    serves = not g["count_pos_neg"] and (cubic or shape == "w25")
    assert backend.rank_vm_available(P) == serves
    if not serves:
        # float accumulation of cubic (or 2-d) patches only: the documented answers, no numbers
        assert int(L.ppp_rank_workspace_bytes(None, ctypes.byref(Pv))) == 0
        with pytest.raises(RuntimeError, match="no voxel-major ranking kernel"):
            backend.rank_patches(pred, vm, ov, Pv)
        score = torch.zeros(P.shape, dtype=torch.float32, device="cuda")
        work = torch.zeros((64,), dtype=torch.uint8, device="cuda")
        rc = L.ppp_rank_patches_vm(backend._dev_ptr(pred), backend.pred_dtype_code(pred), backend._dev_ptr(vm),
                                   backend._dev_ptr(ov), backend._dev_ptr(score), None, backend._dev_ptr(work),
                                   ctypes.byref(Pv), backend._stream())
        assert rc != 0 and b"no count_pos_neg" in L.ppp_last_error()
        # ... and the gather form on the compact planes serves the set
        score = backend.rank_patches(pred, cons, ov, P)
        assert name() == ("rank_v2_kernel" if P.px in (3, 5, 7, 9) else "rank_kernel")
        _same_bits(score.cpu().numpy(), want, what + " (gather form)")
        return
    score = backend.rank_patches(pred, vm, ov, Pv)
    assert name() == S2_KERNEL[fam]
    _same_bits(score.cpu().numpy(), want, what)


# ---- S5 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,shape,flag,dtype", S5_CELLS, ids=[_id(c) for c in S5_CELLS])
def test_s5_family_matches_oracle(fam, shape, flag, dtype, torch_cuda, monkeypatch):
    from patchperpix_amd import backend
    torch, L = torch_cuda, backend.lib()
    pred, _, pairs, _ = _inputs(torch, shape, flag, dtype)
    cons, P, vm, Pv = _consensus(torch, shape, flag, dtype)
    what = _id((fam, shape, flag, dtype))
    want = fm.oracle(shape, flag, dtype)["aff"]
    _set_env(monkeypatch, S5[fam]["env"])
    name = lambda: L.ppp_patch_graph_kernel_name().decode()    # noqa: E731
    if fam == "pg_compact":
        aff = backend.patch_graph(pred, cons, pairs, P)                           # row order
        assert name() == "patch_graph_kernel"
    elif fam in ("pg_vm", "pg_vm2"):
        aff = backend.patch_graph(pred, vm, pairs, Pv, order=backend.pair_order(pairs, Pv))
        assert name() == ("patch_graph_vm2_kernel" if fam == "pg_vm2" else "patch_graph_vm_kernel")
    else:
        job = backend.patch_graph_prepare(pred, pairs, Pv)
        big, small = int(L.ppp_patch_graph_by_patch_chunk(ctypes.byref(Pv))), int(L.ppp_patch_graph_by_patch_chunk_small(ctypes.byref(Pv)))
        assert 0 < small < big and job.n_live < job.n == len(want)                # far rows are never dispatched
        if fam == "pa_big":
            assert job.chunk == big
        elif fam == "pa_small":
            assert job.chunk == small and (shape != "p7" or small == 64)         # 7^3: one wave
        # (the thinning masks are made beforehand for the 3-d widths only)
        assert (job.bits is None) == (fam == "pa_nobits") and (job.plan is None) == (fam == "pa_nolcg" or shape == "w25")
        aff = backend.patch_graph_by_patch(pred, vm, pairs, Pv, job=job)
        assert name() == ("patch_graph_pa_kernel<small>" if job.chunk == small else "patch_graph_pa_kernel")
    _same_bits(aff.cpu().numpy(), want, what)
