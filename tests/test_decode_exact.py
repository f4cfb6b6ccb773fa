"""The decoder's fused tail (csrc/ppp_decode.hip) and its dense head against float64 references
(tests/decode_ref.py): exact where float32 is exact, correctly rounded off ties otherwise."""
import copy
import functools

import numpy as np
import pytest
import torch

import decode_ref as ref
from patchperpix_amd import decode as dec
from test_decode import AE, AE_SHIPPED

SENTINEL = 7.0


def _bits16(a):
    return np.ascontiguousarray(a, dtype=np.float16).view(np.int16)


@functools.lru_cache(maxsize=None)
def _exact_case():
    """257 exact patches and their float64 result, made once; a test with B patches takes the
    first B.  Nothing may write into the returned tensors."""
    case = ref.exact_tail_case(np.random.default_rng(20240607), 257)
    want, _ = ref.tail64(*case)
    return case, want


def _shipped(seed, device="cpu"):
    torch.manual_seed(seed)
    return dec.PatchDecoder(dict(AE_SHIPPED)).to(device).eval()


# ------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------
def test_collapsed_algebra_equals_the_literal_layers():
    """Z[v][t] gathered through (o + t - 1) >> 1 over the in-range taps IS the convolution over
    the upsampled features, borders included: 1e-12 absolute in float64 on normal operands (the
    weights scaled by 1 / sqrt(fan-in), so that the outputs are O(1) and 1e-12 is thousands of
    float64 roundings)."""
    rng = np.random.default_rng(1)
    case = (rng.normal(size=(5, 64, 4, 4, 4)), rng.normal(size=(1, 64, 3, 3, 3)) / np.sqrt(1728.0), 0.3,
            rng.normal(size=(1, 1, 3, 3, 3)) / np.sqrt(27.0), -0.2,
            rng.normal(size=(1, 1, 3, 3, 3)) / np.sqrt(27.0), 0.1)
    want, _ = ref.tail64(*case)
    got = ref.tail64_collapsed(*case)
    assert got.shape == tuple(want.shape) == (5, 343)
    assert float(np.abs(want.numpy()).max()) > 0.1
    assert float(np.abs(got - want.numpy()).max()) <= 1e-12


def test_error_bound_encloses_the_float32_torch_tail():
    """The derived bound E of tail64 holds for a float32 evaluation we can run here (torch on the
    CPU, default-init shipped weights, 130 codes): |f32 - want| <= E everywhere (measured: the
    largest ratio is 0.0029), and at most 2 % of the float64 values lie within E of a float16
    rounding boundary (measured: 0.7 %) -- the cap on what the comparison on the device may leave
    out."""
    d = _shipped(11)
    g = torch.Generator(device="cpu").manual_seed(3)
    codes = torch.randn((130, 176), generator=g)
    with torch.no_grad():
        feats = d.head(codes)
        f32 = d.tail(feats).reshape(130, 343).double()
    want, E = ref.tail64(feats, *d.fused_tail_params())
    ratio = float(((f32 - want).abs() / E).max())
    excluded = float((ref.f16_tie_distance(want) <= E.numpy()).mean())
    print("cpu: max |f32 - want| / E = %.3g, share within E of a tie = %.4f" % (ratio, excluded))
    assert bool(((f32 - want).abs() <= E).all()), ratio
    assert excluded <= 0.02
    assert float(want.abs().max()) > 0


def test_exact_tail_case_holds_its_conditions():
    case, want = _exact_case()
    L = ref.tail_layers64(*case)
    assert float(L["A1"].max()) < 2 ** 24 and float(L["A2"].max()) < 2 ** 24
    assert float(L["A3"].max()) * 2 ** 9 < 2 ** 24
    for k, grid in (("y1", 1.0), ("y2", 1.0), ("y3", 2.0 ** -9)):          # all on the layer's grid
        assert bool((L[k] / grid == torch.round(L[k] / grid)).all())
    cut = float((L["s1"] < 0).double().mean())
    assert 0.25 <= cut <= 0.75, cut
    w = want.numpy()
    h = ref.to_f16(w).astype(np.float64)
    assert float((h != w).mean()) >= 0.10
    lo, hi = ref.f16_bracket(w)
    assert int(((lo != hi) & (w - lo.astype(np.float64) == hi.astype(np.float64) - w)).sum()) >= 1   # exact ties
    assert ref.f16_tie_distance(w).min() == 0.0
    # float32 evaluation, in torch's order here, is exact
    with torch.no_grad():
        y = torch.nn.functional.interpolate(case[0], scale_factor=2, mode="nearest")
        y = torch.relu(torch.nn.functional.conv3d(y, case[1], padding=1) + case[2])
        y = torch.nn.functional.conv3d(y, case[3], padding=1) + case[4]
        y = torch.nn.functional.conv3d(y, case[5], padding=1) + case[6]
    assert torch.equal(y[:, 0, :7, :7, :7].reshape(-1, 343).double(), want)


def _assert_dense_matrices_exact(d32):
    """Every W of d32's dense head against the W a float64 copy of the decoder builds on the CPU:
    the two plain-convolution units bit for bit; the unit with the upsampling in front, where an
    entry is the float32 sum of up to 8 weights (7 additions), within 7 u sum|w|, sum|w| being the
    same entry of the float64 construction with absolute weights.  Bias rows equal."""
    d64 = ref.double_copy(d32)
    dabs = ref.double_copy(d32)
    with torch.no_grad():
        for p in dabs.parameters():
            p.abs_()
    assert d32.enable_dense_head() and d64.enable_dense_head() and dabs.enable_dense_head()
    s32, s64, sabs = d32._dense["stages"], d64._dense["stages"], dabs._dense["stages"]
    assert len(s32) == len(s64) == 3
    for i, ((W, b, _), (W64, b64, _), (Wabs, _, _)) in enumerate(zip(s32, s64, sabs)):
        W, b = W.cpu(), b.cpu()
        assert W.dtype == torch.float32 and W64.dtype == torch.float64 and W.shape == W64.shape
        assert torch.equal(b, b64.float()), "bias row of unit %d" % i
        assert int((W64 != 0).sum()) > 0
        if i == 0:
            excess = float(((W.double() - W64).abs() - 7 * ref.U32 * Wabs).max())
            assert excess <= 0, "upsampled unit: |W - W64| exceeds 7 u sum|w| by %g" % excess
        else:
            bad = W.view(torch.int32) != W64.float().view(torch.int32)
            assert not bool(bad.any()), "unit %d: %d entries of W are not the weight itself, max |W - W64| = %g" % (
                i, int(bad.sum()), float((W.double() - W64).abs().max()))


@pytest.mark.parametrize("cfg", ["shipped", "small"])
def test_dense_head_matrices_hold_the_weights_themselves(cfg):
    torch.manual_seed(5)
    _assert_dense_matrices_exact(dec.PatchDecoder(dict(AE_SHIPPED if cfg == "shipped" else AE)).eval())


def test_decode_tail_checks_its_arguments(monkeypatch):
    """backend.decode_tail refuses, before it touches the library (CPU tensors do here), every
    argument the kernel would trust."""
    from patchperpix_amd import backend

    def no_lib():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(backend, "lib", no_lib)
    n, ps = 3, (7, 7, 7)
    ok = dict(x=torch.zeros(n, 64, 4, 4, 4), w1=torch.zeros(1, 64, 3, 3, 3), b1=0.0,
              w2=torch.zeros(1, 1, 3, 3, 3), b2=0.0, w3=torch.zeros(1, 1, 3, 3, 3), b3=0.0,
              dst=torch.arange(n), pred=torch.zeros(343, 2, 3, 4, dtype=torch.float16), patchshape=ps)
    bad = {
        "channels": dict(x=torch.zeros(n, 32, 4, 4, 4)),
        "grid": dict(x=torch.zeros(n, 64, 4, 4, 8)),
        "no grid": dict(x=torch.zeros(n, 64 * 64)),
        "fewer dst": dict(dst=torch.arange(n - 1)),
        "more dst": dict(dst=torch.arange(n + 1)),
        "strided pred": dict(pred=torch.zeros(343, 2, 3, 8, dtype=torch.float16)[..., ::2]),
        "transposed pred": dict(pred=torch.zeros(24, 343, dtype=torch.float16).t()),
        "float64 pred": dict(pred=torch.zeros(343, 2, 3, 4, dtype=torch.float64)),
        "bfloat16 pred": dict(pred=torch.zeros(343, 2, 3, 4, dtype=torch.bfloat16)),
        "channels of pred": dict(pred=torch.zeros(342, 2, 3, 4, dtype=torch.float16)),
        "voxel-major pred": dict(pred=torch.zeros(24, 343, dtype=torch.float16)),
        "w1": dict(w1=torch.zeros(1, 64, 3, 3)),
        "w2": dict(w2=torch.zeros(1, 1, 3, 3, 2)),
        "w3": dict(w3=torch.zeros(28)),
        "float dst": dict(dst=torch.arange(n).float()),
        "meta x": dict(x=torch.zeros(n, 64, 4, 4, 4, device="meta")),
        "meta dst": dict(dst=torch.arange(n, device="meta")),
        "meta pred": dict(pred=torch.zeros(343, 2, 3, 4, dtype=torch.float16, device="meta")),
    }
    for name, change in bad.items():
        with pytest.raises(ValueError):
            backend.decode_tail(**dict(ok, **change))
            pytest.fail("accepted: " + name)
    # the arguments the cases were derived from pass the checks: they reach the library
    with pytest.raises(AssertionError, match="the library was reached"):
        backend.decode_tail(**ok)


# ------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------
def _run_tail(case, B, dst, block):
    from patchperpix_amd import backend
    X, w1, b1, w2, b2, w3, b3 = case
    dev = block.device
    backend.decode_tail(X[:B].to(dev), w1.to(dev), b1, w2.to(dev), b2, w3.to(dev), b3, dst, block, (7, 7, 7))
    return block


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2, 5, 63, 64, 65, 129, 257])
def test_fused_tail_is_bit_exact_over_the_batch_edges(B):
    """exact_tail_case through the kernel at the batch sizes where its group / wave split takes
    another turn (fewer patches than waves; one short of, exactly and one more than a 64-patch
    group; a last group of one patch after 2 and 4 full ones): the scattered columns hold the
    float16 rounding of the float64 result BIT FOR BIT (-0 and ties count), the float32 block is
    the float16 block widened, and every other column of the sentinel-filled block is untouched.
    dst as int64, as int32 and as a strided int64 view: the same block."""
    case, want = _exact_case()
    shape = (5, 6, 7) if B <= 200 else (7, 8, 9)
    V = int(np.prod(shape))
    g = torch.Generator(device="cpu").manual_seed(100 + B)
    ends = [V - 1] if B == 1 else [0, V - 1]
    mid = (torch.randperm(V - 2, generator=g)[:B - len(ends)] + 1).tolist()
    dst = torch.tensor(sorted(ends + mid), dtype=torch.int64)
    assert dst.numel() == B and dst.unique().numel() == B
    want16 = _bits16(ref.to_f16(want[:B]).T)                             # (343, B)
    outside = torch.ones(V, dtype=torch.bool).index_fill(0, dst, False)
    d_dev = dst.cuda()
    two = torch.stack([d_dev, d_dev + 1], 1)
    blocks = []
    for dtype, dd in ((torch.float16, d_dev), (torch.float32, d_dev), (torch.float16, d_dev.to(torch.int32)),
                      (torch.float16, two[:, 0])):
        block = torch.full((343,) + shape, SENTINEL, dtype=dtype, device="cuda")
        blocks.append(_run_tail(case, B, dd, block).cpu().reshape(343, V))
    torch.cuda.synchronize()
    b16, b32, bi32, bstr = blocks
    got16 = b16[:, dst].numpy().view(np.int16)
    assert np.array_equal(got16, want16), "%d of %d values differ" % (int((got16 != want16).sum()), want16.size)
    assert bool((b16[:, outside] == SENTINEL).all()), "a write outside dst"
    assert torch.equal(b32, b16.float())
    assert torch.equal(bi32.view(torch.int16), b16.view(torch.int16))
    assert torch.equal(bstr.view(torch.int16), b16.view(torch.int16))


@pytest.mark.gpu
def test_fused_tail_rounds_realistic_weights_correctly():
    """Default-init shipped weights, 130 codes through the head on the device, the features copied
    to the CPU for tail64: every value the kernel writes is one of the two float16 neighbours of
    the float64 result, and THE correctly rounded one wherever that result is further from a
    float16 rounding boundary than the derived float32 bound E (at most 2 % of the values are not,
    the cap test_error_bound_encloses_the_float32_torch_tail puts on the reference alone).

    The default initialisation leaves the last bias in charge: every value of this case lies in
    [-0.1262, -0.1199].  So that values of both signs are held to the same standard, the same
    features go through a second time with that bias negated (values in [0.1271, 0.1333]); every
    assertion holds for each pass on its own, the one on the signs over the two."""
    from patchperpix_amd import backend
    d = _shipped(11, "cuda")
    g = torch.Generator(device="cpu").manual_seed(3)
    codes = torch.randn((130, 176), generator=g).cuda()
    with torch.no_grad():
        feats = d.head(codes).contiguous()
    w1, b1, w2, b2, w3, b3 = d.fused_tail_params()
    signs = set()
    for last_bias in (b3, -b3):
        tp = (w1, b1, w2, b2, w3, last_bias)
        block = torch.full((343, 1, 1, 130), SENTINEL, dtype=torch.float16, device="cuda")
        backend.decode_tail(feats, *tp, torch.arange(130, device="cuda"), block, (7, 7, 7))
        got = block.cpu().reshape(343, 130).t().numpy()                   # (130, 343) float16
        want, E = ref.tail64(feats.cpu(), *tp)
        w, E = want.numpy(), E.numpy()
        lo, hi = ref.f16_bracket(w)
        firm = ref.f16_tie_distance(w) > E
        excluded = 1.0 - float(firm.mean())
        r16 = ref.to_f16(w)
        wrong = _bits16(got) != _bits16(r16)
        print("gpu, last bias %+.4f: want in [%.4f, %.4f], share within E of a tie = %.4f, "
              "not the rounded float64 value: %d off ties, %d within E of one"
              % (last_bias, w.min(), w.max(), excluded, int(wrong[firm].sum()), int(wrong[~firm].sum())))
        assert float(np.abs(w).max()) > 0
        assert excluded <= 0.02
        near = (got == lo) | (got == hi)
        assert near.all(), "%d values are not a float16 neighbour of the float64 result" % int((~near).sum())
        assert not wrong[firm].any(), "%d values off ties are not correctly rounded" % int(wrong[firm].sum())
        signs |= set(np.sign(w).ravel().tolist())
    assert {-1.0, 1.0} <= signs


@pytest.mark.gpu
def test_fused_tail_scatters_past_32_bit_offsets():
    """A float16 block of (343, 100, 250, 252): V = 6.3 M voxels, 343 V = 2.16 G elements (past
    2^31) and 4.32 GB (past 2^32 bytes), filled with the sentinel.  70 exact patches go to both
    ends, the middle and random voxels; the columns are bit exact, and after the sentinel is
    written back into them the WHOLE block is the sentinel again: no stray write anywhere, a
    wrapped offset included.  Device memory: the 4.32 GB block plus one boolean temporary of 2.16
    GB, under 7 GB."""
    case, want = _exact_case()
    B, shape = 70, (100, 250, 252)
    V = int(np.prod(shape))
    assert 343 * V > 2 ** 31 and 2 * 343 * V > 2 ** 32
    g = torch.Generator(device="cpu").manual_seed(70)
    fixed = [0, 1, V // 2 - 1, V // 2, V - 2, V - 1]
    rand = torch.randint(2, V - 2, (B,), generator=g).unique()
    rand = rand[torch.randperm(rand.numel(), generator=g)[:B - len(fixed)]]
    dst = torch.tensor(sorted(fixed + rand.tolist()), dtype=torch.int64)
    assert dst.numel() == B and dst.unique().numel() == B
    block = torch.full((343,) + shape, SENTINEL, dtype=torch.float16, device="cuda")
    _run_tail(case, B, dst.cuda(), block)
    flat = block.reshape(343, V)
    got16 = flat[:, dst.cuda()].cpu().numpy().view(np.int16)
    want16 = _bits16(ref.to_f16(want[:B]).T)
    assert np.array_equal(got16, want16), "%d of %d values differ" % (int((got16 != want16).sum()), want16.size)
    flat[:, dst.cuda()] = SENTINEL
    assert bool((block == SENTINEL).all()), "a write outside dst"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["dense", "conv"])
def test_head_on_the_device_against_float64(mode):
    """The head on the device -- as the GEMMs decode_into enables by default, and as MIOpen
    convolutions -- against the float64 head on the CPU, by the project's own criterion
    (test_dense_head_equals_convolution_head): max|got - want| <= 1e-5 max|want|.  Measured
    max|got - want| / max|want| on an MI355X: 4.1e-7 dense, 4.0e-7 convolutions (on a CPU: 2.6e-7
    and 3.9e-7)."""
    d = _shipped(5, "cuda")
    x = torch.randn(9, d.code_units, generator=torch.Generator(device="cpu").manual_seed(5))
    want = ref.head64(d, x)
    if mode == "dense":
        assert d.enable_dense_head() and d._dense["n_stages"] == 1
    with torch.no_grad():
        got = d.head(x.cuda()).cpu().double()
    assert (getattr(d, "_dense", None) is not None) == (mode == "dense")
    assert got.shape == want.shape == (9, 64, 4, 4, 4)
    ratio = float((got - want).abs().max()) / float(want.abs().max())
    print("gpu head (%s): max|got - want| / max|want| = %.3g" % (mode, ratio))
    assert ratio <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["shipped", "small"])
def test_dense_head_matrices_on_the_device_hold_the_weights_themselves(cfg):
    torch.manual_seed(5)
    _assert_dense_matrices_exact(dec.PatchDecoder(dict(AE_SHIPPED if cfg == "shipped" else AE)).cuda().eval())


@pytest.mark.gpu
def test_dense_head_gemms_are_exact_on_integer_operands():
    """A shipped-shape head whose parameters are all in {-1, 0, 1} (weights 4 % dense, biases
    50 %) on integer codes in [-2, 2]: sum|terms| of every output of every layer is below 2^24
    (asserted on the float64 side), so float32 in any order is exact, and the dense head on the
    device equals the float64 convolution head BIT FOR BIT -- a reduced-precision GEMM mode or an
    inexact W would show.  (The convolution head is not held to this: a transform-based algorithm
    is legitimately inexact.)"""
    g = torch.Generator(device="cpu").manual_seed(17)
    d = _shipped(0)
    with torch.no_grad():
        for p in d.parameters():
            keep = torch.rand(p.shape, generator=g) < (0.04 if p.dim() > 1 else 0.5)
            sign = torch.randint(0, 2, p.shape, generator=g) * 2 - 1
            p.copy_((keep * sign).float())
    x = torch.randint(-2, 3, (9, d.code_units), generator=g).float()
    assert ref.head_abs_terms64(d, x) < 2 ** 24
    want = ref.head64(d, x)
    assert float(want.abs().max()) > 100 and float((want != 0).double().mean()) > 0.25
    d = d.cuda()
    assert d.enable_dense_head()
    with torch.no_grad():
        got = d.head(x.cuda()).cpu()
    assert got.dtype == torch.float32
    bad = got.view(torch.int32) != want.float().view(torch.int32)
    assert not bool(bad.any()), "%d of %d outputs differ, max |diff| = %g" % (
        int(bad.sum()), bad.numel(), float((got.double() - want).abs().max()))
