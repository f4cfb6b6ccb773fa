"""GPU: `ppp_eval_patch` (csrc/ppp_eval.hip) against its host definition evaluate_prediction.patch_counts_host and
the reference's results (tests/golden/eval_prediction) -- shapes around the 64-lane run and the vector width, the
patch sizes in use, 1 .. 3 label channels with overlaps, the three element types, NaN / inf / values at the
threshold, the threshold passes, z-tiles accumulated into one set of counters, workspace and outputs under guard
bands, the argument errors -- and the file-level functions with the device on.  Integers throughout: every
comparison is np.array_equal."""
import ctypes
import math

import numpy as np
import pytest

from test_eval_prediction import GOLDENS, PATCH_GOLDENS, check_run, golden, patch_arrays, write_sample
from test_workspace_bounds import Guarded, guard  # noqa: F401  (guard: a fixture)

pytestmark = pytest.mark.gpu

THS = [0.3, 0.5, 0.9]


@pytest.fixture(autouse=True)
def _device_path(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    monkeypatch.delenv("PPP_POSTPROCESS", raising=False)


def ev():
    from patchperpix_amd import evaluate_prediction
    return evaluate_prediction


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def make_labels(rng, L, shape, empty_channel=False):
    """boxes of about a third of each extent, dealt to the channels in turn so that they overlap; with
    `empty_channel` the last channel stays all background"""
    labels = np.zeros((L,) + shape, dtype=np.int32)
    used = L - 1 if empty_channel and L > 1 else L
    for k in range(3 * used + 2):
        lo = [int(rng.integers(0, s)) for s in shape]
        box = tuple(slice(a, a + max(1, s // 3) + 1) for a, s in zip(lo, shape))
        labels[k % used][box] = 3 + k
    if used > 1:                                      # one overlap voxel whatever the boxes did
        labels[0].reshape(-1)[0], labels[1].reshape(-1)[0] = 101, 102
    return labels


def make_pred(rng, C, shape, special=True):
    """float32 values that bfloat16 and float16 hold exactly (0, or [2^-6, 1) with 7 mantissa bits); with
    `special`: NaN, +inf, -inf and values equal to the threshold 0.5 planted"""
    p = rng.uniform(2.0 ** -6, 1.0, (C,) + shape).astype(np.float32)
    p = (p.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    p[rng.random(p.shape) < 0.1] = 0.0
    if special:
        flat = p.reshape(-1)
        idx = rng.choice(flat.size, size=min(flat.size, 16), replace=False)
        for i, v in zip(idx, [np.nan, np.inf, -np.inf, 0.5] * 4):
            flat[i] = v
    return p


def as_tensor(p, dtype):
    import torch
    return torch.from_numpy(p).to({"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}[dtype])


def host_counts(p, labels, patch, ths, dtype, want_maps=True):
    """the definition on the values of `p` held as `dtype` (bfloat16: the float32 tensor of the same values)"""
    arr = p.astype(np.float16) if dtype == "float16" else as_tensor(p, dtype).float().numpy()
    return ev().patch_counts_host(arr, labels, patch, ths, want_maps)


def device_counts(p, labels, patch, ths, dtype, tile=None, want_maps=True):
    """ppp_eval_patch over the volume in z-tiles of `tile` slices (None: one call), one set of counters"""
    import torch
    from patchperpix_amd import backend
    t = as_tensor(p, dtype)
    taus = ev().rounded_thresholds(ths, np.float16 if dtype == "float16" else np.float32)
    Z = p.shape[1]
    d_labels = torch.from_numpy(labels).cuda()
    counts = torch.zeros(1 + 2 * len(ths), dtype=torch.int64, device="cuda")
    inter, union = [], []
    for z in range(0, Z, tile or Z):
        tz = min(tile or Z, Z - z)
        i_t, u_t = backend.eval_patch(t[:, z:z + tz].contiguous().cuda(), d_labels, patch, z, taus, counts, want_maps)
        assert (i_t is None) == (not want_maps) and (u_t is None) == (not want_maps)
        if want_maps:
            assert i_t.dtype == torch.int32 and tuple(i_t.shape) == (len(ths), tz) + p.shape[2:]
            inter.append(i_t.cpu().numpy())
            union.append(u_t.cpu().numpy())
    if want_maps:
        return counts.cpu().numpy(), np.concatenate(inter, axis=1), np.concatenate(union, axis=1)
    return counts.cpu().numpy(), None, None


def equal(got, want):
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    if want[1] is not None and got[1] is not None:
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


# ---------------------------------------------------------------------------------------------
# ppp_eval_patch against the host definition
# ---------------------------------------------------------------------------------------------
# x below, at and above one 64-lane run and across the vector-width remainders (voxel counts that are and are
# not multiples of 4 / 8); Z = 1 under pz = 3: every dz != 0 neighbour lies outside; (2, 2, 2): inside no radius
SHAPES = [(1, 1, 5), (1, 9, 63), (2, 3, 64), (3, 5, 65), (4, 6, 130), (2, 2, 2)]
DTYPES = ["float32", "float16", "bfloat16"]


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_counts_and_maps_equal_the_host_definition(shape, L):
    rng = np.random.default_rng(1000 * L + sum(shape))
    labels = make_labels(rng, L, shape, empty_channel=L == 3)
    assert L == 1 or ((labels > 0).sum(axis=0) > 1).any()
    p = make_pred(rng, 27, shape)
    results = {}
    for dtype in DTYPES:
        want = host_counts(p, labels, (3, 3, 3), THS, dtype)
        got = device_counts(p, labels, (3, 3, 3), THS, dtype)
        equal(got, want)
        results[dtype] = got
    # values that all three types hold exactly, and no such value between 0.3 and its two roundings
    for dtype in DTYPES[1:]:
        equal(results[dtype], results["float32"])


@pytest.mark.parametrize("shape,patch", [((4, 9, 66), (7, 7, 7)), ((2, 2, 2), (7, 7, 7)), ((1, 12, 40), (1, 5, 5)),
                                         ((1, 30, 70), (1, 25, 25))], ids=["7x7x7", "7x7x7-tiny", "1x5x5", "1x25x25"])
def test_patch_sizes(shape, patch):
    rng = np.random.default_rng(sum(shape) + patch[1])
    labels = make_labels(rng, 2, shape)
    p = make_pred(rng, patch[0] * patch[1] * patch[2], shape)
    for dtype in ("float16", "float32"):
        equal(device_counts(p, labels, patch, THS, dtype), host_counts(p, labels, patch, THS, dtype))


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_values_at_the_rounded_threshold(dtype):
    """pred == tau(0.3) > 0.3 is not above the threshold, the next value is; a negative threshold counts the
    zeroed overlap voxels"""
    np_dtype = np.dtype(dtype).type
    rng = np.random.default_rng(5)
    shape = (2, 3, 64)
    labels = make_labels(rng, 2, shape)
    p = rng.uniform(0.0, 1.0, (27,) + shape).astype(np_dtype)
    tau = np_dtype(0.3)
    flat = p.reshape(-1)
    flat[::7] = tau
    flat[3::7] = np.nextafter(tau, np_dtype(1))
    flat[5::7] = np.nextafter(tau, np_dtype(0))
    p = p.astype(np.float32)                           # (exact: as_tensor narrows it again)
    ths = [0.3, -0.25]
    want = host_counts(p, labels, (3, 3, 3), ths, dtype)
    assert want[0][1] > 0 and want[0][3] > want[0][1]
    equal(device_counts(p, labels, (3, 3, 3), ths, dtype), want)


def test_no_foreground_at_all():
    shape = (2, 3, 64)
    labels = np.zeros((2,) + shape, dtype=np.int32)
    p = np.zeros((27,) + shape, dtype=np.float32)
    got = device_counts(p, labels, (3, 3, 3), THS, "float32")
    assert not got[0].any() and not got[1].any() and not got[2].any()
    import torch
    m = ev().patch_metrics(torch.from_numpy(p).cuda(), labels, (3, 3, 3), THS, return_patches=True)
    for th in THS:
        e = m[ev().thresh_key(th)]["rsc_0"]
        assert e["precision"] == 0 and e["recall"] == 0 and e["f1"] == 0 and math.isnan(e["IOU_mean"])


def test_threshold_passes():
    """T = 1, the per-pass chunk, chunk + 1 (a pass boundary) and the maximum"""
    from patchperpix_amd import backend
    chunk, most = backend.lib().ppp_eval_patch_thresholds_per_pass(), backend.lib().ppp_eval_patch_max_thresholds()
    assert 1 < chunk < most
    rng = np.random.default_rng(9)
    shape = (2, 3, 64)
    labels = make_labels(rng, 2, shape)
    p = make_pred(rng, 27, shape)
    all_ths = [round(0.03 * (i + 1), 4) for i in range(most)]
    want = host_counts(p, labels, (3, 3, 3), all_ths, "float16")
    for T in (1, chunk, chunk + 1, most):
        got = device_counts(p, labels, (3, 3, 3), all_ths[:T], "float16")
        equal(got, (want[0][:1 + 2 * T], want[1][:T], want[2][:T]))


@pytest.mark.parametrize("shape", [(3, 5, 65), (4, 6, 130)], ids=lambda s: "x".join(map(str, s)))
def test_z_tiles_accumulate_into_one_set_of_counters(shape):
    rng = np.random.default_rng(sum(shape))
    labels = make_labels(rng, 3, shape)
    p = make_pred(rng, 27, shape)
    for dtype in ("float16", "float32"):
        whole = device_counts(p, labels, (3, 3, 3), THS, dtype)
        equal(whole, host_counts(p, labels, (3, 3, 3), THS, dtype))
        for tile in (1, 2):
            equal(device_counts(p, labels, (3, 3, 3), THS, dtype, tile=tile), whole)
            equal(device_counts(p, labels, (3, 3, 3), THS, dtype, tile=tile, want_maps=False), whole)


# ---------------------------------------------------------------------------------------------
# bounds and argument errors
# ---------------------------------------------------------------------------------------------
def _raw(pred, labels, vol, patch, z0, tz, ths, counts, inter, union, work, C=None, dtype=0):
    from patchperpix_amd import backend
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    th = (ctypes.c_float * max(len(ths), 1))(*ths)
    return backend.lib().ppp_eval_patch(ptr(pred), dtype, pred.shape[0] if C is None else C, ptr(labels), labels.shape[0],
                                        (ctypes.c_int32 * 3)(*vol), (ctypes.c_int32 * 3)(*patch), z0, tz, th, len(ths),
                                        ptr(counts), ptr(inter), ptr(union), ptr(work), backend._stream())


@pytest.mark.parametrize("shape,dtype", [((3, 5, 65), "float32"), ((4, 6, 130), "float16"), ((2, 3, 64), "bfloat16")])
def test_workspace_and_outputs_stay_inside_their_bounds(guard, shape, dtype):
    import torch
    from patchperpix_amd import backend
    g = guard()
    rng = np.random.default_rng(3)
    labels = make_labels(rng, 2, shape)
    p = make_pred(rng, 27, shape)
    want = host_counts(p, labels, (3, 3, 3), THS, dtype)
    T, n = len(THS), shape[0] * shape[1] * shape[2]
    BAND, FILL = 1024, -0x5A5A5A5B                                # int32 elements; 0xA5A5A5A5
    bufs = {name: torch.full((BAND + size + BAND,), FILL, dtype=dt, device="cuda")
            for name, size, dt in (("inter", T * n, torch.int32), ("union", T * n, torch.int32),
                                   ("counts", 1 + 2 * T, torch.int64))}
    mid = {k: b[BAND:b.numel() - BAND] for k, b in bufs.items()}
    mid["counts"].zero_()
    vol = (ctypes.c_int32 * 3)(*shape)
    work = backend._workspace(backend.lib().ppp_eval_patch_workspace_bytes(vol, shape[0]), "cuda")
    taus = ev().rounded_thresholds(THS, np.float16 if dtype == "float16" else np.float32)
    code = {"float32": 0, "float16": 1, "bfloat16": 2}[dtype]
    rc = _raw(as_tensor(p, dtype).cuda().contiguous(), torch.from_numpy(labels).cuda(), shape, (3, 3, 3), 0, shape[0],
              taus, mid["counts"], mid["inter"], mid["union"], work, dtype=code)
    assert rc == 0, backend.lib().ppp_last_error()
    g.verify("test_workspace_and_outputs_stay_inside_their_bounds")
    for name, b in bufs.items():
        assert bool((b[:BAND] == FILL).all()) and bool((b[-BAND:] == FILL).all()), name
    equal((mid["counts"].cpu().numpy(), mid["inter"].cpu().numpy().reshape(want[1].shape),
           mid["union"].cpu().numpy().reshape(want[2].shape)), want)


def test_argument_errors_return_their_codes_without_launching():
    import torch
    from patchperpix_amd import backend
    INVALID, UNSUPPORTED = -1, -4
    shape = (2, 3, 8)
    pred = torch.zeros((27,) + shape, device="cuda")
    labels = torch.zeros((1,) + shape, dtype=torch.int32, device="cuda")
    counts = torch.zeros(1 + 2 * 40, dtype=torch.int64, device="cuda")
    maps = torch.zeros(48, dtype=torch.int32, device="cuda")
    work = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    most = backend.lib().ppp_eval_patch_max_thresholds()
    ok = dict(vol=shape, patch=(3, 3, 3), z0=0, tz=2, ths=[0.5], inter=None, union=None, C=None, dtype=0)
    cases = [(dict(C=26), INVALID), (dict(patch=(3, 2, 3), C=18), INVALID), (dict(patch=(3, 3, 0), C=0), INVALID),
             (dict(ths=[]), INVALID), (dict(ths=[0.1] * (most + 1)), INVALID), (dict(z0=1), INVALID),
             (dict(tz=0), INVALID), (dict(z0=-1, tz=1), INVALID), (dict(ths=[float("inf")]), INVALID),
             (dict(ths=[float("nan")]), INVALID), (dict(inter=maps), INVALID), (dict(dtype=3), INVALID),
             (dict(vol=(2048, 1024, 1024)), UNSUPPORTED), (dict(patch=(41, 41, 41), C=68921), UNSUPPORTED)]
    for change, want in cases:
        kw = dict(ok, **change)
        rc = _raw(pred, labels, kw["vol"], kw["patch"], kw["z0"], kw["tz"], kw["ths"], counts, kw["inter"], kw["union"],
                  work, C=kw["C"], dtype=kw["dtype"])
        assert rc == want, (change, rc, backend.lib().ppp_last_error())
    torch.cuda.synchronize()
    assert not counts.any(), "a refused call launched"
    assert backend.lib().ppp_eval_patch_workspace_bytes((ctypes.c_int32 * 3)(2048, 1024, 1024), 1) == UNSUPPORTED
    # and the plain call is accepted
    assert _raw(pred, labels, shape, (3, 3, 3), 0, 2, [0.5], counts, None, None, work) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# the functions above the kernel, device on
# ---------------------------------------------------------------------------------------------
def _spy(monkeypatch, name):
    from patchperpix_amd import backend
    calls, real = [], getattr(backend, name)

    def wrapper(*a, **k):
        calls.append(name)
        return real(*a, **k)
    monkeypatch.setattr(backend, name, wrapper)
    return calls


@pytest.mark.parametrize("name", PATCH_GOLDENS)
def test_patch_metrics_equal_the_reference(name, monkeypatch):
    import torch
    calls = _spy(monkeypatch, "eval_patch")
    pred, labels, patch, ths = patch_arrays(name)
    _, _, runs, ious = golden(name)
    from test_eval_prediction import same
    for k in range(3):
        kw = runs[k]["kwargs"]
        got = ev().patch_metrics(torch.from_numpy(pred).cuda(), labels, patch, ths, kw.get("return_patches", False),
                                 kw.get("store_iou", False), eval_chunk_bytes=pred[:, :2].nbytes)
        for th in ths:
            iou = got[ev().thresh_key(th)]["rsc_0"].pop("IOU", None)
            if kw.get("store_iou"):
                assert np.array_equal(iou.reshape(ious[(k, ev().thresh_key(th))].shape), ious[(k, ev().thresh_key(th))])
        same(got, runs[k]["metrics"])
    assert len(calls) >= 3


@pytest.mark.parametrize("name", GOLDENS)
def test_file_level_functions_with_the_device_on(tmp_path, name, monkeypatch):
    """equal to the goldens, which the device-off run equals too (test_eval_prediction.py)"""
    patch_calls = _spy(monkeypatch, "eval_patch")
    clean_calls = _spy(monkeypatch, "post_clean_mask")
    pred_fn, label_fn, runs, ious = write_sample(tmp_path, name)
    for k, run in enumerate(runs):
        check_run(run["fn"], pred_fn, label_fn, k, run, ious)
    assert bool(patch_calls) == name.startswith("patch_")
    if name == "fg_rsc":
        assert clean_calls, "the component filter did not run on the device"


def test_skeleton_coverage_with_the_device_on(tmp_path, monkeypatch):
    """the reference's formulas over backend.host_skeletonize_3d, the device thinning being equal to it"""
    calls = _spy(monkeypatch, "skeletonize_3d")
    from test_eval_prediction import test_skeleton_coverage_uses_the_host_thinning as body
    body(tmp_path)
    assert calls, "the thinning did not run on the device"
