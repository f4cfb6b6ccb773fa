"""GPU (MI355X): the short classification of the packed S1 kernel (consensus_v3_kernel<..., CLEAN = true>, what
serves every prediction ppp_pred_check finds clean) against the oracle, bit for bit (uint32 patterns, 0 ulp), on
the clean variant of the flag matrix's inputs (tests/flag_matrix_cases.py): no value outside [0, 1], none equal to
the threshold, and both float neighbours of 0.5 on each side, 0, 1, the largest value below 1, the smallest
subnormal and the smallest normal pinned into every channel.  An id is family-shape-flags-dtype.

Every cell asserts that the check calls its prediction clean, which kernel served, that the short classification
really ran (ppp_consensus_short_form) and the oracle's bits.  The `general` family runs the general classification
(PPP_S1_CLEAN=0) on the same predictions: a difference between the two forms shows as a difference from the oracle.
Then the compute boxes that take each form by the rule instead of the switch, and ppp_pred_check's truth table."""
import ctypes

import numpy as np
import pytest

import flag_matrix_cases as fm

pytestmark = pytest.mark.gpu

SERVED = [n for n in fm.FLAG_SETS if fm.v3_serves(n)]
KEYS = [n for k, n in enumerate(SERVED) if fm.s1_key(n) not in [fm.s1_key(m) for m in SERVED[:k]]]    # one set per S1 key
FIVE = ("p3", "p5", "p7", "p9", "p357")
LINE = {"PPP_S1_FLAT": "0"}


def _grid(shapes, names, dtypes):
    return [(s, n, d) for s in shapes for n in names for d in dtypes]


_DENSE = _grid(FIVE, SERVED, ("float32",)) + _grid(FIVE, KEYS, ("float16", "bfloat16"))
_VM = _grid(("p3", "p5", "p7"), ("default",), fm.DTYPES) + _grid(("p5",), KEYS[1:], fm.DTYPES)
# family -> dict(env: development switches, cells, vm: voxel-major rows, lists: the item lists, short: the form expected)
FAMILIES = {
    "v3c_flat": dict(env={}, cells=_DENSE),
    "v3c_line": dict(env=LINE, cells=_DENSE),
    "v3c_vm_flat": dict(env={}, cells=_VM, vm=True),
    "v3c_vm_line": dict(env=LINE, cells=_VM, vm=True),
    "lists_c": dict(env={}, cells=_grid(FIVE, KEYS, fm.DTYPES), lists=True),
    "lists_c_vm": dict(env={}, cells=_grid(("p5",), KEYS, fm.DTYPES), lists=True, vm=True),
    # (the line form of the lists' instantiations: no volume of the matrix takes it without the switch)
    "lists_c_line": dict(env=LINE, cells=_grid(("p3", "p5", "p7", "p9"), ("default",), fm.DTYPES), lists=True),
    # the general classification on the clean prediction
    "general": dict(env={"PPP_S1_CLEAN": "0"}, cells=_grid(FIVE, ("default",), fm.DTYPES), short=0),
}


def _cells():
    out = [(fam, s, n, d) for fam, f in FAMILIES.items() for (s, n, d) in f["cells"]]
    # cells that share inputs and the oracle's planes next to each other
    out.sort(key=lambda c: (list(fm.SHAPES).index(c[1]), fm.DTYPES.index(c[3]), fm.s1_key(c[2]), SERVED.index(c[2])))
    return out


CELLS = _cells()
# compute boxes (shape, x extent): 64 -- the line form by the rule; 65 -- the flat form, a one-lane rest of the first line
PART_CELLS = [(s, n) for s in ("p5", "p7") for n in (64, 65)]
_id = "-".join


def part_box(shape, x_extent):
    """a proper sub-box in z and y (an odd number of slices: the last slice pair is half empty)"""
    _, (Z, Y, X), _, _ = fm.SHAPES[shape]
    box = (1, 2, 5, Z - 1 if Z % 2 else Z - 2, Y - 1, 5 + x_extent)
    assert (box[3] - box[0]) % 2 == 1 and box[5] <= X
    return box


def cell_form(cell):
    """(dtype, px, FLAT, lists, short form): the instantiation of consensus_v3_kernel a cell launches"""
    fam, shape, _, dtype = cell
    f = FAMILIES[fam]
    return (dtype, fm.SHAPES[shape][0][2], fm.v3_flat_form(shape, f["env"]), bool(f.get("lists")), f.get("short", 1) == 1)


def part_form(shape, x_extent):
    return ("float16", fm.SHAPES[shape][0][2], fm.v3_flat_form(shape, {}, part_box(shape, x_extent)), False, True)


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


def _to_device(torch, host, dtype):
    """The float32 array `host` as a device tensor of `dtype`, narrowed on the host (exact by construction; no
    device conversion that could flush a subnormal), and read back as bit patterns."""
    pat, _ = fm.dtype_patterns(host, dtype)
    ints = np.ascontiguousarray(pat).view(np.int32 if dtype == "float32" else np.int16)
    t = torch.from_numpy(ints.copy()).cuda().view(getattr(torch, dtype))
    assert np.array_equal(t.view(torch.int32 if dtype == "float32" else torch.int16).cpu().numpy(), ints)
    return t


_INPUTS = {}        # one entry: the device inputs of the last (shape, dtype)


def _inputs(torch, shape, flag, dtype):
    """(pred, overlap or None, P) on the device for a clean cell"""
    from patchperpix_amd import backend
    b = fm.base_case(shape)
    if (shape, dtype) not in _INPUTS:
        _INPUTS.clear()
        host = fm.prediction(shape, flag, dtype, fm.CLEAN)
        assert np.array_equal(host.view(np.uint32), fm.to_dtype(host, dtype).view(np.uint32))
        _INPUTS[(shape, dtype)] = (_to_device(torch, host, dtype), torch.from_numpy(np.array(b["overlap"])).cuda())
    pred, ov = _INPUTS[(shape, dtype)]
    P = backend.make_params(b["vol"], b["ps"], **fm.FLAG_SETS[flag])
    assert P.pred_clean == 0
    return pred, (ov if P.use_overlap else None), P


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    assert got.shape == want.shape, what
    bad = np.count_nonzero(got != want)
    assert bad == 0, "%s: %d of %d entries differ from the oracle" % (what, bad, got.size)


def _same_cons(cons, shape, flag, dtype, what):
    if fm.bits_hash(cons.cpu().numpy()) != fm.oracle(shape, flag, dtype, fm.CLEAN)["cons_hash"]:
        _same_bits(cons.cpu().numpy(), fm.oracle_cons_planes(shape, flag, dtype, fm.CLEAN), what)
        raise AssertionError(what + ": hash differs")


_ROWS = {}          # one entry: the oracle's voxel-major rows of the last (shape, dtype, S1 flags)


def _oracle_rows(shape, flag, dtype):
    key = (shape, dtype, fm.s1_key(flag))
    if key not in _ROWS:
        _ROWS.clear()
        _ROWS[key] = fm.voxel_major_from_planes(fm.oracle_cons_planes(shape, flag, dtype, fm.CLEAN), fm.SHAPES[shape][0])
    return _ROWS[key]


# ---- the clean cells --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,shape,flag,dtype", CELLS, ids=[_id(c) for c in CELLS])
def test_clean_prediction_matches_oracle(fam, shape, flag, dtype, torch_cuda, monkeypatch):
    from patchperpix_amd import backend
    torch, L = torch_cuda, backend.lib()
    f = FAMILIES[fam]
    pred, ov, P = _inputs(torch, shape, flag, dtype)
    what = _id((fam, shape, flag, dtype))
    assert backend.pred_check(pred, P) == 1                    # (before the switches: PPP_S1_CLEAN=0 asks nothing)
    _set_env(monkeypatch, f["env"])
    short = f.get("short", 1)
    if not short:
        # the caller KNOWS the prediction is clean; the library's switch takes the general classification all the same
        P.pred_clean = 1
    if f.get("vm"):
        P.cons_layout = backend.CONS_VOXEL_MAJOR
        assert L.ppp_consensus_writes_voxel_major(ctypes.byref(P)) == 1
    if f.get("lists"):
        assert int(L.ppp_consensus_sparse_workspace_bytes(ctypes.byref(P), None)) > 0
        with backend.s1_sparse_scope(True):
            cons = backend.consensus(pred, ov, P)              # (VOXEL_MAJOR: direct rows, closed)
        assert L.ppp_consensus_kernel_name().decode() == "consensus_v3_kernel<lists>"
        assert backend.consensus_last_items()[2] == 1
    else:
        cons = backend.consensus(pred, ov, P)
        assert L.ppp_consensus_kernel_name().decode() == "consensus_v3_kernel"
    assert L.ppp_consensus_short_form() == short and backend.NOTES["s1_short_form"] == short
    if f.get("vm"):
        _same_bits(cons.cpu().numpy(), _oracle_rows(shape, flag, dtype), what)
    else:
        _same_cons(cons, shape, flag, dtype, what)


# ---- compute boxes that take each form by the rule ------------------------------------------------------------------
@pytest.mark.parametrize("shape,x_extent", PART_CELLS, ids=["%s-x%d" % c for c in PART_CELLS])
def test_clean_part_takes_its_form_by_the_rule(shape, x_extent, torch_cuda):
    """ppp_consensus_part (float16, default flags, clean) over a box whose x extent is exactly 64 (one line per run,
    by the rule) or 65 (two lines flattened), into a poisoned buffer: the entries of the part's base voxels are the
    oracle's, every other entry keeps the poison."""
    from patchperpix_amd import backend
    torch, L = torch_cuda, backend.lib()
    backend.reload_env()
    pred, ov, P = _inputs(torch, shape, "default", "float16")
    box = part_box(shape, x_extent)
    assert fm.v3_flat_form(shape, {}, box) == (x_extent != 64)
    assert backend.pred_check(pred, P) == 1
    P.pred_clean = 1
    want = fm.oracle_cons_planes(shape, "default", "float16", fm.CLEAN).view(np.uint32)
    out = torch.full(want.shape, -1, dtype=torch.int32, device="cuda")                 # 0xFFFFFFFF
    part = backend.Box(*box)
    backend.check(L.ppp_consensus_part(backend._dev_ptr(pred), backend.pred_dtype_code(pred), backend._dev_ptr(ov),
                                       backend._dev_ptr(out), ctypes.byref(P), ctypes.byref(part), backend._stream()))
    assert L.ppp_consensus_kernel_name().decode() == "consensus_v3_kernel" and L.ppp_consensus_short_form() == 1
    got = out.cpu().numpy().view(np.uint32)
    inside = np.zeros(want.shape[1:], dtype=bool)
    inside[box[0]:box[3], box[1]:box[4], box[2]:box[5]] = True
    bad = np.count_nonzero(got[:, inside] != want[:, inside])
    assert bad == 0, "%d of %d entries of the part differ from the oracle" % (bad, want[:, inside].size)
    assert np.count_nonzero(want[:, inside]) >= 1000
    assert (got[:, ~inside] == 0xFFFFFFFF).all(), "an entry outside the part was written"


# ---- ppp_pred_check: a single planted value ----------------------------------------------------------------------
def _from_bits(u):
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


def _planted(dtype, half):
    """[(value as float32, the bits ppp_pred_check must return, or None: the model's)]"""
    up = lambda v: fm._step(np.float32(v), dtype, True)            # noqa: E731
    down = lambda v: fm._step(np.float32(v), dtype, False)         # noqa: E731
    sub, normal = fm.smallest(dtype)
    mid = 2 if half else 0              # bg 0.25: everything in [0.25, 0.5] votes nowhere
    out = [(np.float32(0.0), 0), (sub, 0), (normal, 0), (down(0.5), mid), (up(0.5), 0), (np.float32(0.5), 2),
           (down(1.0), 0), (np.float32(1.0), 0), (up(1.0), 1), (np.float32(2.0), 1), (np.float32(np.inf), 1),
           (np.float32(-0.0), 1), (-sub, 1), (np.float32(-1.0), 1), (np.float32(-np.inf), 1),
           (_from_bits(0x7FC00000), 3), (_from_bits(0xFFC00000), 3)]
    if half:
        out += [(np.float32(0.25), 2), (np.float32(0.375), 2), (down(0.25), 0), (up(0.25), 2)]
    return out


@pytest.mark.parametrize("dtype", fm.DTYPES)
def test_pred_check_truth_table(dtype, torch_cuda):
    """One value planted in an otherwise clean 1-d buffer of 64, through the raw entry point: the returned bits are
    the CPU model's (fm.is_clean) and the expected class of every planted value."""
    from patchperpix_amd import backend
    torch, L = torch_cuda, backend.lib()
    for name in ("default", "half05"):
        g = fm.geo_flags(name)
        assert (g["th"], g["bg"]) == (0.5, 0.25 if name == "half05" else 0.5)
        P = backend.make_params(fm.SHAPES["p3"][1], fm.SHAPES["p3"][0], **fm.FLAG_SETS[name])
        planted = _planted(dtype, name == "half05")
        # rows 67 apart: their starts take every alignment, so the head and tail loops of the check run too; the
        # check is given the first 64 values of a row (last row: nothing planted)
        host = np.full((len(planted) + 1, 67), 0.75, dtype=np.float32)
        for j, (v, _) in enumerate(planted):
            host[j, (7 * j + 3) % 64] = v
        assert np.array_equal(host.view(np.uint32), fm.to_dtype(host, dtype).view(np.uint32))     # all representable
        model = [fm.is_clean(row[:64], dtype, g["th"], g["bg"]) for row in host]
        for (v, want), m in zip(planted + [(None, 0)], model):
            assert m == want, (name, dtype, v, m, want)             # the model itself is the documented table
        buf = _to_device(torch, host, dtype)
        out = torch.full((len(host),), -1, dtype=torch.int32, device="cuda")
        es = buf.element_size()
        for j in range(len(host)):
            rc = L.ppp_pred_check(buf.data_ptr() + j * 67 * es, backend.pred_dtype_code(buf), 64, out.data_ptr() + 4 * j,
                                  ctypes.byref(P), backend._stream())
            assert rc == 0, L.ppp_last_error()
        got = out.cpu().numpy().tolist()
        assert got == model, (name, dtype, [(float(v), a, b) for (v, _), a, b in zip(planted, got, model) if a != b])
