"""GPU: the fused patch loss from the labels (csrc/ppp_patch_loss.hip) through patchperpix_amd/train_loss.py and
backend.patch_loss_*.  The reference is `patch_loss_host` -- NumPy float64 -- on the exactly widened logits.

Tolerances (derived, not tuned; u = 2^-24):
  loss      |loss - loss64| <= (E + 32) u loss64, plus one float32 rounding of the result.  Every term is >= 0, so
            the sum's relative error is at most the E - 1 float32 additions of a voxel plus the element's own
            error, for which 32 u are allowed (exp, log1p, the formula; NumPy's float32 evaluation measured 4.7 u).
  gradient  float32: within 32 u relative of the float64 value, element by element.  float16 / bfloat16: one of the
            two neighbours, in that type, of a value within that distance.
            Below the smallest normal float32, 2^-126, the format itself keeps no relative accuracy, neither for
            sigmoid(-|x|) nor for the product: 2^-126 times max(1, s w grad_out) is allowed on top.
Worst values measured on an MI355X over this file's cases: loss 0.88 u (of an allowance of 2082, the 2049-edge case;
0.56 u of 60 otherwise), float32 gradient 5.2 u of 32; neither exceeds half its allowance.  Only the extreme-logit
case (|x| >= 88 under a scale of 2^40) uses the 2^-126 term."""
import numpy as np
import pytest

from test_patch_loss import DENSE, load
from test_patch_loss import test_entry_points_check_their_arguments_before_any_device as argument_codes

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -126


@pytest.fixture(autouse=True)
def _needs_gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"


def tl():
    from patchperpix_amd import train_loss
    return train_loss


def tu():
    from patchperpix_amd import train_util
    return train_util


def be():
    from patchperpix_amd import backend
    return backend


def dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def tdtype(name):
    import torch
    return {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}[name]


def bits(t):
    import torch
    a = t.detach().cpu().contiguous()
    return a.view({4: torch.int32, 2: torch.int16}[a.element_size()]).numpy()


def make_labels(rng, B, L, spatial, n=None):
    """boxes of about a third of each extent dealt to the channels in turn, so that they overlap; ids repeat
    across channels (the per-channel rule matters) and one id is negative"""
    seg = np.zeros((B, L) + spatial, dtype=np.int32)
    n = n or 4 * L + 3
    for b in range(B):
        for k in range(n):
            lo = [int(rng.integers(0, s)) for s in spatial]
            box = tuple(slice(a, a + max(1, s // 3) + 1) for a, s in zip(lo, spatial))
            seg[b, k % L][box] = 3 + k % 5
        seg[b, L - 1].reshape(-1)[: max(1, seg[b, L - 1].size // 7)] = -9
    return seg


def centred(r):
    g = np.meshgrid(np.arange(-r[0], r[0] + 1), np.arange(-r[1], r[1] + 1), np.arange(-r[2], r[2] + 1), indexing="ij")
    return np.stack([a.reshape(-1) for a in g], axis=1)


def halo_of(nhood):
    lo, hi = nhood.min(axis=0), nhood.max(axis=0)
    return (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2])


def plan_of(seg, nhood, dtype=None, box=None):
    vol = seg.shape[-3:]
    return be().gt_affs_dense_plan(seg.shape[0], seg.shape[1], vol, len(nhood), halo_of(nhood),
                                   box or (0, vol[0], 0, vol[1], 0, vol[2]), dtype)


def logits_for(rng, seg, nhood, box=None, dtype="float32", sigma=4.0):
    """N(0, sigma^2) logits of the box's shape, rounded into the element type: a CPU tensor"""
    import torch
    vol = seg.shape[-3:]
    box = box or (0, vol[0], 0, vol[1], 0, vol[2])
    ext = (box[1] - box[0], box[3] - box[2], box[5] - box[4])
    x = (sigma * rng.standard_normal((seg.shape[0], len(nhood)) + ext)).astype(np.float32)
    return torch.from_numpy(x).to(tdtype(dtype))


# ---- the tolerances of the module's docstring ----
def loss_ok(got, want, E):
    return abs(got - want) <= (E + 32) * U * abs(want) + U * abs(want)


def step16(t, up):
    """the neighbour above (below) each value of a float16 / bfloat16 CPU tensor"""
    import torch
    b = t.contiguous().view(torch.int16).to(torch.int32)
    order = torch.where(b >= 0, b, -(b & 0x7FFF)) + (1 if up else -1)
    b = torch.where(order >= 0, order, (-order) | 0x8000)
    b = torch.where(b >= 0x8000, b - 0x10000, b).to(torch.int16)
    return b.view(t.dtype)


def grad_ok(got, want64, scale=1.0):
    """`got` a CPU tensor of the element type, `want64` the float64 array, `scale` = max s w grad_out"""
    import torch
    want = torch.from_numpy(np.ascontiguousarray(want64))
    tol = 32 * U * want.abs() + TINY * max(1.0, float(scale))
    g = got.double()
    if got.dtype == torch.float32:
        bad = ~((g - want).abs() <= tol)
    else:
        lo, hi = (want - tol).to(got.dtype), (want + tol).to(got.dtype)         # round to nearest
        lo = torch.where(lo.double() > want - tol, step16(lo, False), lo)       # ... down to the neighbour below
        hi = torch.where(hi.double() < want + tol, step16(hi, True), hi)
        bad = ~((g >= lo.double()) & (g <= hi.double()))
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        print("first bad gradient at %d: got %r, want %r" % (i, float(g.reshape(-1)[i]), float(want.reshape(-1)[i])))
    return not bool(bad.any())


def worst(got, want64):
    """the largest relative error of a float32 gradient in u, over the elements that are normal numbers"""
    g, w = got.double().numpy(), np.asarray(want64)
    ok = np.abs(w) > TINY
    return float((np.abs(g - w)[ok] / np.abs(w)[ok]).max() / U) if ok.any() else 0.0


def fused(x, seg, nhood, w=None, box=None, nc=None, go=None, check=True, counts=False):
    """forward and backward through the public function: (loss, gradient on the CPU, counts)"""
    xd = x.cuda().requires_grad_(True)
    out = tl().patch_bce_from_labels(xd, dev(seg), nhood, None if w is None else dev(w), box=box, num_channels=nc,
                                     check=check, want_counts=counts)
    loss, cnt = out if counts else (out, None)
    assert loss.dim() == 0 and loss.is_cuda and str(loss.dtype) == "torch.float32"
    (loss if go is None else go * loss).backward()
    assert xd.grad.dtype == x.dtype and xd.grad.shape == x.shape
    return loss.item(), xd.grad.cpu(), cnt


def check_case(x, seg, nhood, w=None, box=None, nc=None, go=None, counts=False):
    E = len(nhood)
    loss, grad, cnt = fused(x, seg, nhood, w, box, nc, go, counts=counts)
    l64, g64 = tl().patch_loss_host(x.double().numpy(), seg, nhood, w, box, nc)
    s = 0.0 if not np.abs(g64).max() else (1.0 / (float(nc or E) * float(w.sum())) if w is not None else 1.0 / x.numel())
    scale = s * (go or 1.0) * (float(w.max()) if w is not None else 1.0)
    print("loss %.9g want %.9g: %.2f u of %d; gradient worst %.2f u" % (loss, l64, abs(loss - l64) / max(l64, 1e-300) / U,
                                                                        E + 33, worst(grad, g64 * (go or 1.0)) if x.dtype == tdtype("float32") else -1))
    assert loss_ok(loss, l64, E)
    assert grad_ok(grad, g64 * (go or 1.0), scale)
    if counts:
        G = tu().gt_affs_dense_host(seg, nhood, box)
        assert np.array_equal(cnt.cpu().numpy(), tl().patch_counts_host(x.float().numpy(), G))
    return loss, grad


# ---------------------------------------------------------------------------------------------
# the goldens through the public functions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("name", sorted(DENSE))
def test_dense_goldens_through_the_public_function(name, dtype):
    import torch
    g = load(name)
    x = torch.from_numpy(g["logits"]).to(tdtype(dtype))
    kw = {}
    if "box" in g:
        kw["box"] = tuple(int(v) for v in g["box"])
    if "num_channels" in g:
        kw["num_channels"] = float(g["num_channels"])
    xd = x.cuda().requires_grad_(True)
    loss = tl().patch_bce_from_labels(xd, dev(g["seg"]), g["nhood"], dev(g["mask"]) if "mask" in g else None, **kw)
    loss.backward()
    E = len(g["nhood"])
    if dtype == "float32":
        assert loss_ok(loss.item(), float(g["loss64"]), E)
        # the reference's own float64 gradient carries its subtraction's rounding at the largest gradient's scale
        gg, want = xd.grad.cpu().double().numpy(), g["grad64"]
        assert np.all(np.abs(gg - want) <= 32 * U * np.abs(want) + 2.0 ** -52 * np.abs(want).max() + TINY)
    # and the definition on the widened logits, in every type
    ndim = DENSE[name]
    lift = lambda a: a.reshape(a.shape[:-ndim] + (1,) * (3 - ndim) + a.shape[-ndim:])
    n3 = g["nhood"] if ndim == 3 else np.concatenate([np.zeros_like(g["nhood"][:, :1]), g["nhood"]], axis=1)
    w = lift(g["mask"][:, 0 if g["mask"].shape[1] == 1 else 1]) if "mask" in g else None
    box = kw.get("box")
    box = None if box is None else (box if ndim == 3 else (0, 1) + box)
    l64, g64 = tl().patch_loss_host(lift(x.double().numpy()), lift(g["seg"]), n3, w, box, kw.get("num_channels"))
    assert loss_ok(loss.item(), l64, E) and grad_ok(xd.grad.cpu(), g64.reshape(x.shape), 1.0)
    if name == "d3_zero":
        assert loss.item() == 0.0 and not bits(xd.grad).any()


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_sampled_golden_and_the_dense_result_at_the_centres(dtype):
    import torch
    g = load("s3_n5")
    ps, psH = int(g["ps"]), int(g["psH"])
    for rows in (g["samples"], g["samples"][:1], g["samples"][:0]):
        N = len(rows)
        x = torch.from_numpy(g["logits"][:N]).to(tdtype(dtype))
        xd = x.cuda().requires_grad_(True)
        loss = tl().patch_bce_from_label_samples(xd.reshape((N, 1, ps, ps, ps)), dev(g["seg"]), g["nhood"], ps, psH, dev(rows))
        loss.backward()
        l64, g64 = tl().patch_loss_samples_host(x.double().numpy(), g["seg"], rows, g["nhood"], (ps,) * 3, (psH,) * 3)
        assert loss.dim() == 0 and loss.is_cuda and tuple(xd.grad.shape) == (N, 27)
        assert loss_ok(loss.item(), l64, 27) and (N == 0 or grad_ok(xd.grad.cpu(), g64, 1.0))
        if N == 5 and dtype == "float32":
            assert loss_ok(loss.item(), float(g["loss64"]), 27)
            # each row is the dense result at its centre with the raster nhood moved to the centre
            for n, (b, z, y, x0) in enumerate(rows):
                at = (int(z) + psH, int(y) + psH, int(x0) + psH)
                box = (at[0], at[0] + 1, at[1], at[1] + 1, at[2], at[2] + 1)
                _, gd = tl().patch_loss_host(x[n].double().numpy().reshape(1, 27, 1, 1, 1), g["seg"][b:b + 1], g["nhood"] - psH, None, box)
                assert grad_ok(xd.grad[n].cpu() * 5, gd.reshape(27), 1.0)


# ---------------------------------------------------------------------------------------------
# seeded cases sized by the plan
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_every_axis_exceeds_the_tile_by_a_non_multiple(dtype):
    rng = np.random.default_rng(1)
    seg = make_labels(rng, 2, 2, (6, 19, 75))
    nhood = centred((1, 1, 1))
    assert plan_of(seg, nhood, tdtype(dtype))[:4] == (4, 8, 32, 1)
    w = rng.random((2, 6, 19, 75)).astype(np.float32)
    w[w < 0.3] = 0
    check_case(logits_for(rng, seg, nhood, dtype=dtype), seg, nhood, w, counts=True)
    check_case(logits_for(rng, seg, nhood, dtype=dtype), seg, nhood)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("box", [(1, 8, 2, 19, 3, 66), (1, 8, 2, 19, 3, 67)])
def test_boxes_of_63_and_64_voxels_in_x(box, dtype):
    """bX = 63: rows start at every phase of a 16-byte group (the piecewise loads and stores); bX = 64: the aligned kernel"""
    rng = np.random.default_rng(2)
    seg = make_labels(rng, 1, 2, (9, 21, 70))
    nhood = centred((1, 1, 1))
    ext = (box[1] - box[0], box[3] - box[2], box[5] - box[4])
    w = rng.random((1,) + ext).astype(np.float32)
    check_case(logits_for(rng, seg, nhood, box, dtype), seg, nhood, w, box=box, counts=True)


@pytest.mark.parametrize("staged", [1, 0])
@pytest.mark.parametrize("L", [1, 4, 5])
def test_channel_counts_around_the_register_channels_staged_and_direct(L, staged):
    """kRegCh = 4 channels of the centre stay in registers: one channel, exactly four, and a fifth that is read again;
    each with the labels staged in LDS and -- an offset as long as the x axis -- loaded directly"""
    rng = np.random.default_rng(3 + L)
    seg = make_labels(rng, 1, L, (8, 12, 40))
    nhood = centred((1, 2, 2)) if staged else np.concatenate([centred((1, 1, 1)), [[0, 0, 40], [0, 0, -39], [7, 11, 39]]])
    assert plan_of(seg, nhood)[3] == staged
    check_case(logits_for(rng, seg, nhood), seg, nhood, counts=True)


def test_an_offset_as_long_as_an_axis_takes_the_direct_path():
    rng = np.random.default_rng(9)
    seg = make_labels(rng, 1, 2, (6, 9, 21))
    nhood = np.concatenate([centred((1, 1, 1)), [[6, 0, 0], [0, -9, 0], [0, 0, 21], [0, 0, -20], [5, 8, 20]]])
    assert plan_of(seg, nhood)[3] == 0
    check_case(logits_for(rng, seg, nhood), seg, nhood, counts=True)


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_343_edges_in_blocks_of_64_and_a_remainder(dtype):
    rng = np.random.default_rng(10)
    seg = make_labels(rng, 1, 3, (8, 10, 40))
    nhood = centred((3, 3, 3))
    assert len(nhood) == 343 == 5 * 64 + 23
    w = rng.random((1, 8, 10, 40)).astype(np.float32)
    check_case(logits_for(rng, seg, nhood, dtype=dtype), seg, nhood, w, nc=343.0)


def test_one_edge():
    rng = np.random.default_rng(11)
    seg = make_labels(rng, 2, 1, (5, 9, 33))
    for nhood in (np.array([[0, 0, 1]]), np.array([[0, 0, 0]])):
        check_case(logits_for(rng, seg, nhood), seg, nhood, counts=True)


def test_two_dimensional_images():
    import torch
    rng = np.random.default_rng(12)
    seg = make_labels(rng, 2, 2, (1, 40, 70))
    n2 = centred((0, 2, 2))[:, 1:]
    x = logits_for(rng, seg, centred((0, 2, 2)))
    w = rng.random((2, 2, 40, 70)).astype(np.float32)
    xd = x[:, :, 0].cuda().requires_grad_(True)
    loss = tl().patch_bce_from_labels(xd, dev(seg[:, :, 0]), n2, dev(w))
    loss.backward()
    l64, g64 = tl().patch_loss_host(x.double().numpy(), seg, centred((0, 2, 2)), w[:, 1][:, None], None, 25.0)
    assert tuple(xd.grad.shape) == (2, 25, 40, 70)
    assert loss_ok(loss.item(), l64, 25) and grad_ok(xd.grad.cpu(), g64[:, :, 0], 1.0)
    assert isinstance(tl().PatchLossFromLabels(25.0)(xd.detach(), dev(seg[:, :, 0]), n2, dev(w)), torch.Tensor)


# ---------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------
def test_weights_none_fractional_zero_and_nan_logits_where_the_weight_is_zero():
    import torch
    rng = np.random.default_rng(13)
    seg = make_labels(rng, 2, 2, (5, 11, 48))
    nhood = centred((1, 1, 1))
    x = logits_for(rng, seg, nhood)
    frac = rng.random((2, 5, 11, 48)).astype(np.float32)
    check_case(x, seg, nhood)
    check_case(x, seg, nhood, frac, nc=3.5)
    loss, grad, _ = fused(x, seg, nhood, np.zeros_like(frac))
    assert loss == 0.0 and not bits(grad).any(), "cnt == 0: zero loss, zero gradient"
    # zero over whole 16-byte groups, NaN / inf logits there; `out=` under a sentinel: every element is written
    holes = frac.copy()
    holes[:, :, :, 8:24] = 0
    holes[0, 2, 3, 30] = 0                                             # and one lone voxel inside a live group
    bad = x.clone()
    bad[:, :, :, :, 8:24] = float("nan")
    bad[:, 5, :, :, 12:16] = float("inf")
    bad[0, :, 2, 3, 30] = float("nan")
    l64, g64 = tl().patch_loss_host(bad.double().numpy(), seg, nhood, holes)
    assert np.isfinite(l64)
    d_x, d_seg, d_w, d_n = bad.cuda(), dev(seg), dev(holes), dev(nhood.astype(np.int32))
    loss, state, _ = be().patch_loss_dense_fwd(d_x, d_seg, d_n, weight=d_w)
    out = torch.full_like(d_x, 12345.0)
    res = be().patch_loss_dense_bwd(d_x, d_seg, d_n, state, torch.ones(1, device="cuda"), weight=d_w, out=out)
    assert res is out and loss_ok(loss.item(), l64, 27) and np.isfinite(loss.item())
    got = out.cpu()
    assert not bool((got == 12345.0).any()) and bool(torch.isfinite(got).all())
    assert not bits(got[:, :, :, :, 8:24]).any() and not bits(got[0, :, 2, 3, 30]).any()
    assert grad_ok(got, g64, 1.0)
    with pytest.raises(ValueError, match="negative"):
        tl().patch_bce_from_labels(d_x, d_seg, nhood, -d_w)


def test_extreme_logits_keep_the_loss_finite_and_the_gradient_accurate():
    import torch
    rng = np.random.default_rng(14)
    seg = make_labels(rng, 1, 2, (4, 8, 32))
    nhood = centred((1, 1, 1))
    vals = np.array([0.0, -0.0, 100.0, -100.0, 1e4, -1e4, 30.0, -30.0, 17.0, -17.0, 88.0, -88.0], dtype=np.float32)
    x = torch.from_numpy(vals[rng.integers(0, len(vals), size=(1, 27, 4, 8, 32))])
    G = tu().gt_affs_dense_host(seg, nhood)
    for v in (100.0, -100.0, 30.0, -30.0):
        assert ((x.numpy() == v) & (G == 1)).any() and ((x.numpy() == v) & (G == 0)).any()
    loss, grad = check_case(x, seg, nhood, go=2.0 ** 40)
    assert np.isfinite(loss)
    # where sigmoid(x) - 1 would cancel: x = 30 with g = 1 is -exp(-30) to 32 u, not a multiple of 2^-24
    sel = torch.from_numpy((x.numpy() == 30.0) & (G == 1))
    want = -np.exp(-30.0) / (1 + np.exp(-30.0)) / x.numel() * 2.0 ** 40
    assert bool(((grad[sel].double() - want).abs() <= 32 * U * abs(want)).all())
    h = torch.tensor([65504.0, -65504.0, 0.0, 11.0, -11.0], dtype=torch.float16)[torch.from_numpy(rng.integers(0, 5, size=(1, 27, 4, 8, 32)))]
    loss, _ = check_case(h, seg, nhood, go=1024.0)
    assert np.isfinite(loss)


def test_a_grad_scaler_keeps_float16_gradients_out_of_the_subnormals():
    import torch
    rng = np.random.default_rng(15)
    seg = make_labels(rng, 2, 2, (6, 16, 64))
    nhood = centred((1, 1, 1))
    x = logits_for(rng, seg, nhood, dtype="float16")
    _, g64 = tl().patch_loss_host(x.double().numpy(), seg, nhood)
    loss, grad, _ = fused(x, seg, nhood, go=65536.0)
    want = g64 * 65536.0
    assert grad_ok(grad, want, 65536.0 / x.numel())
    normal = np.abs(want) >= 2.0 ** -14 * (1 + 2.0 ** -9)              # stays a normal float16 under the tolerance
    assert normal.mean() > 0.5 and not bool((grad.double().numpy()[normal] == 0).any())
    _, plain, _ = fused(x, seg, nhood)
    assert (plain.double().numpy()[normal] == 0).any() or (np.abs(g64[normal]) < 2.0 ** -14).any(), "the unscaled gradients are subnormal"


# ---------------------------------------------------------------------------------------------
# autograd, determinism, counters
# ---------------------------------------------------------------------------------------------
def test_autograd_leaf_upstream_op_retain_graph_and_check_false():
    import torch
    rng = np.random.default_rng(16)
    seg = make_labels(rng, 1, 2, (5, 9, 40))
    nhood = centred((1, 1, 1))
    x = logits_for(rng, seg, nhood)
    w = rng.random((1, 5, 9, 40)).astype(np.float32)
    l64, g64 = tl().patch_loss_host(x.double().numpy(), seg, nhood, w)
    d_seg, d_w = dev(seg), dev(w)
    leaf = x.cuda().requires_grad_(True)
    loss = tl().patch_bce_from_labels(leaf, d_seg, nhood, d_w)
    loss.backward(retain_graph=True)
    first = bits(leaf.grad).copy()
    assert grad_ok(leaf.grad.cpu(), g64, 1.0)
    leaf.grad = None
    loss.backward()
    assert np.array_equal(bits(leaf.grad), first), "two backward calls of one graph: equal bits"
    with pytest.raises(RuntimeError):
        g, = torch.autograd.grad(tl().patch_bce_from_labels(leaf, d_seg, nhood, d_w), leaf, create_graph=True)
        g.sum().backward()                                             # differentiable once
    a = (x / 2).cuda().requires_grad_(True)                            # pred = 2 a: exact in float32
    tl().patch_bce_from_labels(2 * a, d_seg, nhood, d_w).backward()
    assert grad_ok(a.grad.cpu(), 2 * g64, 2.0)
    # non-contiguous logits are made contiguous
    t = x.cuda().permute(0, 1, 2, 4, 3).contiguous().permute(0, 1, 2, 4, 3).requires_grad_(True)
    assert not t.is_contiguous()
    tl().patch_bce_from_labels(t, d_seg, nhood, d_w).backward()
    assert np.array_equal(bits(t.grad.contiguous()), first)
    # check=False: the same bits, int64 labels and a mask with two channels
    free = x.cuda().requires_grad_(True)
    mask2 = torch.stack([torch.zeros_like(d_w), d_w], dim=1)
    l2 = tl().patch_bce_from_labels(free, d_seg.long(), dev(nhood), mask2, check=False)
    l2.backward()
    assert l2.item() == loss.item() and np.array_equal(bits(free.grad), first)
    with pytest.raises(ValueError, match="fit int32"):
        big = d_seg.long().clone()
        big[0, 0, 0, 0, 0] = 2 ** 31
        tl().patch_bce_from_labels(free, big, nhood, d_w)


def test_two_runs_give_equal_bits():
    rng = np.random.default_rng(17)
    seg = make_labels(rng, 2, 3, (9, 20, 70))
    nhood = centred((2, 2, 2))
    x = logits_for(rng, seg, nhood)
    w = rng.random((2, 9, 20, 70)).astype(np.float32)
    runs = [fused(x, seg, nhood, w) for _ in range(2)]
    assert np.float32(runs[0][0]).tobytes() == np.float32(runs[1][0]).tobytes()
    assert np.array_equal(bits(runs[0][1]), bits(runs[1][1]))


def test_counters_on_labels_only_equal_the_target_sum():
    import torch
    rng = np.random.default_rng(18)
    seg = make_labels(rng, 2, 2, (7, 13, 50))
    nhood = centred((1, 2, 2))
    d_seg, d_n = dev(seg), dev(nhood.astype(np.int32))
    x = torch.zeros((2, len(nhood), 7, 13, 50), device="cuda")           # no logit is positive
    w = torch.zeros((2, 7, 13, 50), device="cuda")                       # and no voxel has weight: all are read
    _, counts = tl().patch_bce_from_labels(x, d_seg, d_n, w, want_counts=True)
    assert counts.dtype == torch.int64 and counts.tolist() == [0, int(be().gt_affs_dense(d_seg, d_n).sum().item()), 0]
    _, counts = tl().patch_bce_from_labels(x + 1, d_seg, d_n, w, want_counts=True)
    assert counts.tolist() == [x.numel(), counts[1].item(), counts[1].item()]


# ---------------------------------------------------------------------------------------------
# workspace, memory, offsets past 2^31, the ABI
# ---------------------------------------------------------------------------------------------
def test_the_workspace_is_not_left(monkeypatch):
    """tests/test_workspace_bounds.py's technique: a guard band in front of and behind the workspace, both untouched"""
    import torch
    FILL = 0xA5
    taken = []

    def guarded(nbytes, device):
        nbytes = int(nbytes)
        be().check(min(nbytes, 0))
        band = max(4096, (nbytes + 255) // 256 * 256)
        buf = torch.full((band + nbytes + band,), FILL, dtype=torch.uint8, device=device)
        taken.append((buf, nbytes, band))
        return buf[band:band + nbytes]

    rng = np.random.default_rng(19)
    seg = make_labels(rng, 2, 2, (6, 19, 75))
    nhood = centred((3, 3, 3))
    x = logits_for(rng, seg, nhood)
    w = rng.random((2, 6, 19, 75)).astype(np.float32)
    want = fused(x, seg, nhood, w)
    g = load("s3_n5")
    xs = torch.from_numpy(g["logits"]).cuda().requires_grad_(True)
    plain = tl().patch_bce_from_label_samples(xs, dev(g["seg"]), g["nhood"], 3, 1, dev(g["samples"])).item()
    monkeypatch.setattr(be(), "_workspace", guarded)
    got = fused(x, seg, nhood, w)
    sampled = tl().patch_bce_from_label_samples(xs, dev(g["seg"]), g["nhood"], 3, 1, dev(g["samples"]))
    sampled.backward()
    torch.cuda.synchronize()
    assert len(taken) == 2 and taken[0][1] == be().patch_loss_workspace_bytes(2, 2, (6, 19, 75), 343, halo_of(nhood), (0, 6, 0, 19, 0, 75))
    assert taken[1][1] == be().patch_loss_workspace_bytes(2, 2, (5, 6, 7), 27, N=5)
    for buf, nbytes, band in taken:
        assert bool((buf[:band] == FILL).all()) and bool((buf[band + nbytes:] == FILL).all())
    assert got[0] == want[0] and np.array_equal(bits(got[1]), bits(want[1])) and sampled.item() == plain


def test_peak_memory_is_the_gradient_and_the_workspace():
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(20)
    seg = make_labels(rng, 1, 3, (26, 46, 70))
    box = (3, 23, 3, 43, 3, 67)
    nhood = centred((3, 3, 3))
    d_seg, d_n = dev(seg), dev(nhood.astype(np.int32))
    x = (4 * torch.randn((1, 343, 20, 40, 64), device="cuda")).requires_grad_(True)
    mask = (torch.rand((1, 1, 20, 40, 64), device="cuda") < 0.7).float()
    nbytes = x.numel() * 4
    work = be().patch_loss_workspace_bytes(1, 3, (26, 46, 70), 343, halo_of(nhood), box)
    tl().patch_bce_from_labels(x[:, :, :1], d_seg, d_n, mask[:, :, :1], box=(3, 4, 3, 43, 3, 67)).backward()     # warm: caches, handles
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = tl().patch_bce_from_labels(x, d_seg, d_n, mask, box=box, check=False)
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("fused: %d bytes over the baseline; gradient %d + workspace %d" % (peak, nbytes, work))
    assert peak <= nbytes + work + 65536
    fused_grad, fused_loss = x.grad, loss.item()
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    target = tu().seg_to_affgraph_3d_multi_torch(d_seg, d_n, "cuda", check=False, box=box)
    loss = (F.binary_cross_entropy_with_logits(x, target, reduction="none") * mask).sum() / (343.0 * mask.sum())
    loss.backward()
    torch.cuda.synchronize()
    unfused = torch.cuda.max_memory_allocated() - base
    print("unfused: %d bytes over the baseline" % unfused)
    assert unfused >= 3 * nbytes, "the unfused path holds two more tensors of that size than the gradient"
    assert abs(loss.item() - fused_loss) <= (343 + 32) * 2 * U * fused_loss
    assert bool(((x.grad - fused_grad).abs() <= 64 * U * fused_grad.abs() + 2 * U * fused_grad.abs().max()).all())


def test_offsets_past_two_to_the_31():
    """E = 2049 edges of 2^20 voxels, float16: the first E whose B E bV passes 2^31 (the issue's 2200 reduced to it,
    to keep the test to seconds).  The loss against plain torch in float64 on the device, edge by edge; the
    gradient on a seeded sample of elements and the last one."""
    import torch
    vol = (16, 256, 256)
    V = vol[0] * vol[1] * vol[2]
    g = np.meshgrid(np.arange(-1, 2), np.arange(-13, 14), np.arange(-13, 14), indexing="ij")
    nhood = np.stack([a.reshape(-1) for a in g], axis=1)[:2049]
    E = len(nhood)
    assert E * V > 2 ** 31 and (E - 1) * V <= 2 ** 31
    z, y, x_ = torch.meshgrid(torch.arange(vol[0]), torch.arange(vol[1]), torch.arange(vol[2]), indexing="ij")
    cell = (z // 5) * 7919 + (y // 11) * 104729 + (x_ // 9) * 1299709
    seg = ((cell % 5 != 0) * (cell % 1000 + 1)).to(torch.int32).reshape((1, 1) + vol).cuda()
    assert plan_of(seg.cpu().numpy(), nhood, torch.float16)[3] == 1
    gen = torch.Generator(device="cuda").manual_seed(21)
    x = torch.empty((1, E) + vol, dtype=torch.float16, device="cuda")
    for e0 in range(0, E, 256):
        x[0, e0:e0 + 256] = (4 * torch.randn((min(256, E - e0),) + vol, generator=gen, device="cuda")).half()
    x.requires_grad_(True)
    loss = tl().patch_bce_from_labels(x, seg, nhood, check=False)
    (2.0 ** 24 * loss).backward()                                       # 1 / (E V) alone is below float16
    lab = seg[0, 0]
    total = torch.zeros((), dtype=torch.float64, device="cuda")
    for e, n in enumerate(nhood.tolist()):
        lo = [max(0, -d) for d in n]
        hi = [min(s, s - d) for s, d in zip(vol, n)]
        G = torch.zeros(vol, dtype=torch.float64, device="cuda")
        c = lab[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        o = lab[lo[0] + n[0]:hi[0] + n[0], lo[1] + n[1]:hi[1] + n[1], lo[2] + n[2]:hi[2] + n[2]]
        G[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = (c == o) & (c != 0)
        xe = x.detach()[0, e].double()
        total += (xe.clamp(min=0) - xe * G + torch.log1p(torch.exp(-xe.abs()))).sum()
    l64 = (total / (E * V)).item()
    print("loss %.9g want %.9g: %.2f u" % (loss.item(), l64, abs(loss.item() - l64) / l64 / U))
    assert loss_ok(loss.item(), l64, E)
    rng = np.random.default_rng(22)
    flat = np.concatenate([rng.integers(0, E * V, size=4096), [E * V - 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1]])
    idx = torch.from_numpy(flat).cuda()
    got = x.grad.reshape(-1)[idx].cpu()
    xs = x.detach().reshape(-1)[idx].double().cpu().numpy()
    e, v = flat // V, flat % V
    pos = np.stack(np.unravel_index(v, vol), axis=1)
    nb = pos + nhood[e]
    ok = ((nb >= 0) & (nb < np.array(vol))).all(axis=1)
    labs = lab.cpu().numpy()
    centre = labs[pos[:, 0], pos[:, 1], pos[:, 2]]
    other = np.where(ok, labs[tuple(np.clip(nb, 0, np.array(vol) - 1).T)], 0)
    Gs = (centre == other) & (centre != 0)
    assert 0.02 < Gs.mean() < 0.98
    _, slope = tl()._bce64(xs, Gs)
    assert grad_ok(got, slope * 2.0 ** 24 / (E * V), 2.0 ** 24 / (E * V))
    assert (bits(got) != 0).mean() > 0.5


def test_argument_codes_and_alignment_with_a_device():
    import torch
    argument_codes()
    lib = be().lib()
    for name in ("ppp_patch_loss_workspace_bytes", "ppp_patch_loss_dense_fwd", "ppp_patch_loss_dense_bwd",
                 "ppp_patch_loss_samples_fwd", "ppp_patch_loss_samples_bwd"):
        assert hasattr(lib, name)
    # an output pointer that is 4- but not 16-byte aligned takes the piecewise kernel and gives the same bits
    rng = np.random.default_rng(23)
    seg = make_labels(rng, 1, 2, (4, 8, 64))
    nhood = centred((1, 1, 1))
    x = logits_for(rng, seg, nhood).cuda()
    d_seg, d_n = dev(seg), dev(nhood.astype(np.int32))
    loss, state, _ = be().patch_loss_dense_fwd(x, d_seg, d_n)
    one = torch.ones(1, device="cuda")
    want = be().patch_loss_dense_bwd(x, d_seg, d_n, state, one)
    flat = torch.zeros(x.numel() + 1, device="cuda")
    shifted = flat[1:].view(x.shape)
    assert shifted.data_ptr() % 16 == 4
    be().patch_loss_dense_bwd(x, d_seg, d_n, state, one, out=shifted)
    assert np.array_equal(bits(shifted), bits(want)) and flat[0].item() == 0
    xs = flat[1:].view(x.shape).copy_(x)
    loss2, _, _ = be().patch_loss_dense_fwd(xs, d_seg, d_n)
    assert loss2.item() == loss.item()
