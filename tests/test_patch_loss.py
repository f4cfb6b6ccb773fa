"""CPU: the fused patch loss from the labels (patchperpix_amd/train_loss.py) without a device.  The NumPy float64
definitions and the CPU-tensor path (autograd included) against the goldens the reference's own
MaskedBCEWithLogitsLoss made on the reference's own targets (tests/golden/patch_loss, generator
tests/golden/gen_golden_patch_loss.py); the mask-channel rule, cnt == 0, N == 0, and the argument codes of the
five C entry points before any device is asked for."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from patchperpix_amd import backend
from patchperpix_amd import train_loss as tl

PL_DIR = os.path.join(GOLDEN_DIR, "patch_loss")
DENSE = {"d3_nomask": 3, "d3_cm1": 3, "d3_cm2": 3, "d3_zero": 3, "d3_box": 3, "d2_cm2": 2}


def load(name):
    g = np.load(os.path.join(PL_DIR, name + ".npz"))
    return {k: g[k] for k in g.files}


def close64(a, b):
    """1e-12 relative; for a gradient plus the reference's own cancellation error, one rounding of sigmoid(x) next
    to 1 at the scale of the largest gradient (gen_golden_patch_loss.close)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    floor = 2.0 ** -52 * np.abs(b).max() if b.ndim else 0.0
    return bool(np.all(np.abs(a - b) <= 1e-12 * np.abs(b) + floor))


def close32(a, b, E):
    """the float32 goldens against a float32 evaluation in another order: E + 32 roundings of the loss, 32 of an
    element of the gradient plus the subtraction's one rounding at the largest gradient's scale"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not b.ndim:
        return bool(abs(a - b) <= (E + 32) * 2.0 ** -24 * abs(b))
    return bool(np.all(np.abs(a - b) <= 32 * 2.0 ** -24 * np.abs(b) + 2.0 ** -23 * np.abs(b).max()))


def host_args(g, ndim):
    lift = lambda a: a.reshape(a.shape[:-ndim] + (1,) * (3 - ndim) + a.shape[-ndim:])
    nhood = g["nhood"] if ndim == 3 else np.concatenate([np.zeros_like(g["nhood"][:, :1]), g["nhood"]], axis=1)
    weight = None
    if "mask" in g:
        weight = lift(g["mask"][:, 0 if g["mask"].shape[1] == 1 else 1])
    box = None
    if "box" in g:
        box = tuple(int(v) for v in g["box"])
        box = box if ndim == 3 else (0, 1) + box
    return lift(g["logits"]), lift(g["seg"]), nhood, weight, box, (float(g["num_channels"]) if "num_channels" in g else None)


def test_the_golden_folder_holds_the_cases_and_stays_small():
    files = sorted(glob.glob(os.path.join(PL_DIR, "*.npz")))
    assert sorted(os.path.splitext(os.path.basename(f))[0] for f in files) == sorted(list(DENSE) + ["s3_n5"])
    assert sum(os.path.getsize(f) for f in files) < 300000
    assert set(int(load(n)["seg"].shape[1]) for n in DENSE) == {2}


@pytest.mark.parametrize("name", sorted(DENSE))
def test_host_definition_equals_the_golden(name):
    g = load(name)
    loss, grad = tl.patch_loss_host(*host_args(g, DENSE[name]))
    assert grad.dtype == np.float64 and grad.size == g["grad64"].size
    assert close64(loss, g["loss64"]) and close64(grad.reshape(g["grad64"].shape), g["grad64"])


def test_sampled_host_definition_equals_the_golden():
    g = load("s3_n5")
    assert len(g["samples"]) == 5 and len(np.unique(g["samples"], axis=0)) == 4, "a duplicate row"
    ps, psH = int(g["ps"]), int(g["psH"])
    loss, grad = tl.patch_loss_samples_host(g["logits"], g["seg"], g["samples"], g["nhood"], (ps,) * 3, (psH,) * 3)
    assert close64(loss, g["loss64"]) and close64(grad, g["grad64"])
    dup = np.where((g["samples"] == g["samples"][1]).all(axis=1))[0]
    assert len(dup) == 2 and not np.array_equal(grad[dup[0]], grad[dup[1]]), "each row has its own logits"


@pytest.mark.parametrize("name", sorted(DENSE))
@pytest.mark.parametrize("tag", ["64", "32"])
def test_cpu_tensor_path_equals_the_golden_with_autograd(name, tag):
    g = load(name)
    E = len(g["nhood"])
    dtype = torch.float64 if tag == "64" else torch.float32
    x = torch.tensor(g["logits"], dtype=dtype, requires_grad=True)
    kw = {}
    if "box" in g:
        kw["box"] = tuple(int(v) for v in g["box"])
    if "num_channels" in g:
        kw["num_channels"] = float(g["num_channels"])
    mask = torch.from_numpy(g["mask"]) if "mask" in g else None
    loss = tl.patch_bce_from_labels(x, torch.from_numpy(g["seg"]), g["nhood"], mask, **kw)
    assert loss.dim() == 0 and loss.dtype == dtype
    loss.backward()
    ok = close64 if tag == "64" else (lambda a, b: close32(a, b, E))
    assert ok(loss.item(), g["loss" + tag]) and ok(x.grad.numpy(), g["grad" + tag])
    # the module is the same function
    again = tl.PatchLossFromLabels(kw.get("num_channels"))(x.detach(), torch.from_numpy(g["seg"]), g["nhood"], mask,
                                                          box=kw.get("box"))
    assert again.item() == loss.item()


def test_cpu_tensor_sampled_path_equals_the_golden():
    g = load("s3_n5")
    ps, psH = int(g["ps"]), int(g["psH"])
    for shape in ((5, 27), (5, 1, 3, 3, 3)):
        x = torch.tensor(g["logits"].reshape(shape), dtype=torch.float64, requires_grad=True)
        loss = tl.patch_bce_from_label_samples(x, torch.from_numpy(g["seg"]), g["nhood"], ps, psH, torch.from_numpy(g["samples"]))
        loss.backward()
        assert close64(loss.item(), g["loss64"]) and close64(x.grad.numpy().reshape(5, 27), g["grad64"])
    with pytest.raises(ValueError, match="leaves the volume"):
        tl.patch_bce_from_label_samples(x, torch.from_numpy(g["seg"]), g["nhood"], ps, psH, np.array([[0, 3, 0, 0]] * 5))


def test_the_mask_channel_rule():
    g = load("d3_cm2")
    x, seg, m = torch.from_numpy(g["logits"]), torch.from_numpy(g["seg"]), torch.from_numpy(g["mask"])
    by = lambda mask: tl.patch_bce_from_labels(x, seg, g["nhood"], mask).item()
    assert by(m) == by(m[:, 1]) == by(m[:, 1:2]) != by(m[:, 0])           # Cm == 2: channel 1; Cm == 1: channel 0
    assert by(m) == by(m.bool()) == by(m.to(torch.uint8)) == by(m.double()), "any float / bool / integer mask"
    three = torch.cat([m, m[:, :1]], dim=1)
    assert by(three) == by(m[:, 1])
    with pytest.raises(ValueError):
        by(m[:, :, :2])
    with pytest.raises(ValueError, match="negative"):
        by(-m)


def test_a_count_of_zero_gives_zero_loss_and_zero_gradient():
    g = load("d3_zero")
    assert not g["mask"].any()
    logits = g["logits"].copy()
    logits[0, 0, 0, 0, :3] = [np.nan, np.inf, -np.inf]                     # no weight: whatever the logits hold
    loss, grad = tl.patch_loss_host(*((logits[...],) + host_args(g, 3)[1:]))
    assert loss == 0.0 and not grad.any()
    x = torch.tensor(logits, requires_grad=True)
    out = tl.patch_bce_from_labels(x, torch.from_numpy(g["seg"]), g["nhood"], torch.from_numpy(g["mask"]))
    out.backward()
    assert out.item() == 0.0 and not x.grad.numpy().any()
    # the same with a weight on other voxels only
    g = load("d3_cm1")
    hole = np.argwhere(g["mask"][:, 0] == 0)[0]
    logits = g["logits"].copy()
    logits[hole[0], :, hole[1], hole[2], hole[3]] = np.nan
    loss, grad = tl.patch_loss_host(*((logits,) + host_args(g, 3)[1:]))
    assert close64(loss, g["loss64"]) and close64(grad, g["grad64"])
    x = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    out = tl.patch_bce_from_labels(x, torch.from_numpy(g["seg"]), g["nhood"], torch.from_numpy(g["mask"]), num_channels=27.0)
    out.backward()
    assert close64(out.item(), g["loss64"]) and close64(x.grad.numpy(), g["grad64"])


def test_no_samples_give_zero():
    g = load("s3_n5")
    x = torch.zeros((0, 27), requires_grad=True)
    loss = tl.patch_bce_from_label_samples(x, torch.from_numpy(g["seg"]), g["nhood"], 3, 1, torch.zeros((0, 4), dtype=torch.int64))
    loss.backward()
    assert loss.item() == 0.0 and tuple(x.grad.shape) == (0, 27)
    assert tl.patch_loss_samples_host(np.zeros((0, 27)), g["seg"], np.zeros((0, 4), dtype=np.int64), g["nhood"], (3,) * 3,
                                      (1,) * 3)[0] == 0.0


def test_shapes_that_do_not_fit_raise():
    g = load("d3_box")
    x, seg = torch.from_numpy(g["logits"]), torch.from_numpy(g["seg"])
    with pytest.raises(ValueError, match="box="):
        tl.patch_bce_from_labels(x, seg, g["nhood"])
    with pytest.raises(ValueError):
        tl.patch_bce_from_labels(x, seg, g["nhood"], box=(0, 2, 0, 3, 1, 6, 0))
    with pytest.raises(ValueError):
        tl.patch_bce_from_labels(x, seg, g["nhood"], box=(0, 3, 0, 3, 1, 6))
    with pytest.raises(ValueError):
        tl.patch_bce_from_labels(x[:, :5], seg, g["nhood"], box=tuple(int(v) for v in g["box"]))
    with pytest.raises(ValueError):
        tl.patch_bce_from_labels(x, seg.float(), g["nhood"], box=tuple(int(v) for v in g["box"]))


def test_counts_on_the_cpu_path_are_the_integer_sums():
    g = load("d3_nomask")
    loss, counts = tl.patch_bce_from_labels(torch.from_numpy(g["logits"]), torch.from_numpy(g["seg"]), g["nhood"], want_counts=True)
    G = __import__("patchperpix_amd.train_util", fromlist=["x"]).gt_affs_dense_host(g["seg"], g["nhood"])
    assert counts.dtype == torch.int64 and np.array_equal(counts.numpy(), tl.patch_counts_host(g["logits"], G))
    assert counts[2] <= min(counts[0], counts[1]) and counts[1] == int(G.sum())


def test_entry_points_check_their_arguments_before_any_device():
    """argument checks come before the device is asked for: the documented codes without a GPU too"""
    L = backend.lib()
    i3 = lambda *v: (ctypes.c_int32 * 3)(*v)
    i6 = lambda *v: (ctypes.c_int32 * 6)(*v)
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    odd = ctypes.c_void_p(buf.ctypes.data + 2)
    halo, box, vol = i6(-1, 1, -1, 1, -1, 1), i6(0, 4, 0, 5, 0, 6), i3(4, 5, 6)
    INVALID, UNSUPPORTED = -1, -4
    # (every call below ends at a check: none may reach a launch, the pointers are host memory)
    fwd = lambda **k: L.ppp_patch_loss_dense_fwd(k.get("x", p), k.get("dt", 0), p, k.get("B", 1), k.get("L", 1), k.get("vol", vol),
                                                 p, k.get("E", 27), k.get("halo", halo), k.get("box", box), k.get("w", None),
                                                 k.get("nc", 27.0), k.get("loss", p), k.get("state", p), None,
                                                 k.get("work", p), None)
    bwd = lambda **k: L.ppp_patch_loss_dense_bwd(k.get("x", p), k.get("dt", 0), p, k.get("B", 1), k.get("L", 1), k.get("vol", vol),
                                                 p, k.get("E", 27), k.get("halo", halo), k.get("box", box), k.get("w", None),
                                                 k.get("state", p), k.get("go", p), k.get("grad", p), None)
    for f in (fwd, bwd):
        assert f(E=0) == INVALID and f(E=65536) == UNSUPPORTED
        assert f(vol=i3(2048, 1024, 1024), box=i6(0, 1, 0, 1, 0, 1)) == UNSUPPORTED
        assert f(box=i6(0, 0, 0, 5, 0, 6)) == INVALID and f(box=i6(0, 5, 0, 5, 0, 6)) == INVALID
        assert f(B=0) == INVALID and f(L=0) == INVALID and f(dt=3) == INVALID
        assert f(halo=i6(1, -1, 0, 0, 0, 0)) == INVALID and f(x=None) == INVALID and f(state=None) == INVALID
        assert f(x=odd) == INVALID and b"misaligned" in L.ppp_last_error()
        assert f(w=odd) == INVALID
    assert fwd(w=p, nc=0.0) == INVALID and fwd(w=p, nc=float("nan")) == INVALID and fwd(work=None) == INVALID
    assert bwd(go=None) == INVALID and bwd(grad=None) == INVALID
    sfwd = lambda **k: L.ppp_patch_loss_samples_fwd(k.get("x", p), k.get("dt", 0), p, 1, 1, vol, p, k.get("N", 3), p, k.get("E", 27),
                                                    k.get("ps", i3(3, 3, 3)), k.get("ctr", i3(1, 1, 1)), k.get("loss", p), p, p, None)
    sbwd = lambda **k: L.ppp_patch_loss_samples_bwd(k.get("x", p), k.get("dt", 0), p, 1, 1, vol, p, k.get("N", 3), p, k.get("E", 27),
                                                    k.get("ps", i3(3, 3, 3)), k.get("ctr", i3(1, 1, 1)), p, p, k.get("grad", p), None)
    for f in (sfwd, sbwd):
        assert f(N=0) == 0 and f(N=0, x=None) == 0, "N = 0 is a no-op that succeeds, device or not"
        assert f(N=-1) == INVALID and f(E=0) == INVALID and f(E=65536) == UNSUPPORTED and f(dt=7) == INVALID
        assert f(ctr=i3(1, 3, 1)) == INVALID and f(ps=i3(0, 3, 3)) == INVALID and f(x=None) == INVALID
    ws = L.ppp_patch_loss_workspace_bytes
    assert ws(1, 1, vol, 27, halo, box, 0, 0) > 0 and ws(1, 1, vol, 27, None, None, 0, 5) > 0
    assert ws(1, 1, vol, 0, halo, box, 0, 0) == INVALID and ws(1, 1, vol, 65536, None, None, 0, 5) == UNSUPPORTED
    assert ws(1, 1, vol, 27, None, None, 0, -1) == INVALID and ws(1, 1, vol, 27, halo, i6(0, 5, 0, 5, 0, 6), 0, 0) == INVALID
    # one double per workgroup and sum, in the Carver's 256-byte slots; the tiles are the planner's
    plan = backend.gt_affs_dense_plan(1, 3, (140, 140, 140), 343, (-3, 3) * 3, (0, 140) * 3)
    groups = plan[4] * int(np.prod([-(-140 // t) for t in plan[:3]]))
    assert backend.patch_loss_workspace_bytes(1, 3, (140,) * 3, 343, (-3, 3) * 3, (0, 140) * 3) == 2 * (-(-groups * 8 // 256) * 256)
