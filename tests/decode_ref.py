"""Plain float64 references of the decoder (helper of tests/test_decode_exact.py, not a test file).

Nothing here touches the project's kernels or its dense head: ``tail64`` is the last decoder stage
as the literal layers in float64 torch ops on the CPU, with a DERIVED forward-error bound for a
float32 evaluation of the same layers; ``tail64_collapsed`` is the algebra csrc/ppp_decode.hip
states in its header, in float64 NumPy; ``head64`` is the head of a float64 copy of a decoder;
``exact_tail_case`` makes operands on which float32 arithmetic in ANY order is exact, so that the
only rounding left in the kernel is the final round-to-nearest-even to float16.

float64 -> float16 goes through NumPy (``to_f16``), which rounds once; torch narrows a double to
float first and would round twice.
"""
import copy

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24                 # unit roundoff of float32


def gamma(n):
    """Higham's gamma_n for float32: n chained roundings grow a sum of |terms| by at most this."""
    return n * U32 / (1.0 - n * U32)


def _f64(t):
    if torch.is_tensor(t):
        return t.detach().to(device="cpu", dtype=torch.float64)
    return torch.as_tensor(np.asarray(t, dtype=np.float64))


def tail_layers64(X, w1, b1, w2, b2, w3, b3):
    """The three layers on the full 8^3 grid in float64, with what the error bound and the exact
    case need: pre-activation ``s1``, ``y1``, ``y2``, ``y3`` and ``A1``..``A3``, the sum of the
    absolute values of the terms (bias included) that make up every output."""
    X, w1, w2, w3 = _f64(X), _f64(w1).reshape(1, 64, 3, 3, 3), _f64(w2).reshape(1, 1, 3, 3, 3), \
        _f64(w3).reshape(1, 1, 3, 3, 3)
    b1, b2, b3 = float(b1), float(b2), float(b3)
    assert tuple(X.shape[1:]) == (64, 4, 4, 4)
    up = F.interpolate(X, scale_factor=2, mode="nearest")
    s1 = F.conv3d(up, w1, padding=1) + b1
    A1 = abs(b1) + F.conv3d(up.abs(), w1.abs(), padding=1)
    y1 = torch.relu(s1)
    y2 = F.conv3d(y1, w2, padding=1) + b2
    A2 = abs(b2) + F.conv3d(y1.abs(), w2.abs(), padding=1)
    y3 = F.conv3d(y2, w3, padding=1) + b3
    A3 = abs(b3) + F.conv3d(y2.abs(), w3.abs(), padding=1)
    return dict(s1=s1, y1=y1, y2=y2, y3=y3, A1=A1, A2=A2, A3=A3, w2=w2, w3=w3)


def tail64(X, w1, b1, w2, b2, w3, b3):
    """(want, E), both float64 (B, 343): the literal last stage -- nearest x2, conv3d padding 1 +
    b1, ReLU, two single-map conv3d padding 1 + bias, crop [:7, :7, :7] -- and a running forward
    error bound for the kernel's float32 evaluation of it.

    With u = 2^-24 and gamma(n) = n u / (1 - n u), a float32 sum of n-times-rounded terms is
    within gamma(n) * sum|terms| of the exact one, whatever the order (so also in whatever order
    the matrix instruction adds):
      layer 1: every product goes through at most 64 chained channel additions, 27 gather
               additions and the bias addition: E1 = gamma(92) * A1, A1 = |b1| + conv(|U|, |W1|);
      ReLU is 1-Lipschitz and exact: E1 passes through;
      layer 2: the input error propagates as P2 = conv(E1, |W2|); the layer's own 27 fused
               multiply-adds and the bias act on inputs up to |y1| + E1:
               E2 = P2 + gamma(28) * (A2 + P2), A2 = |b2| + conv(|y1|, |W2|);
      layer 3: the same with E2, W3, b3, y2.
    """
    L = tail_layers64(X, w1, b1, w2, b2, w3, b3)
    E1 = gamma(92) * L["A1"]
    P2 = F.conv3d(E1, L["w2"].abs(), padding=1)
    E2 = P2 + gamma(28) * (L["A2"] + P2)
    P3 = F.conv3d(E2, L["w3"].abs(), padding=1)
    E3 = P3 + gamma(28) * (L["A3"] + P3)
    n = L["y3"].shape[0]
    crop = lambda t: t[:, 0, :7, :7, :7].reshape(n, 343)
    return crop(L["y3"]), crop(E3)


def tail64_collapsed(X, w1, b1, w2, b2, w3, b3):
    """The kernel header's algebra in float64 NumPy, (B, 343):
    Z[v][t] = sum_c X[c][v] W1[c][t];  Y1[o] = relu(b1 + sum_t Z[(o + t - 1) >> 1][t]) over the
    taps that stay inside the 8^3 grid; then the two single-map convolutions and the crop."""
    X = _f64(X).numpy().reshape(-1, 64, 64)
    w1 = _f64(w1).numpy().reshape(64, 27)
    w2, w3 = _f64(w2).numpy().reshape(27), _f64(w3).numpy().reshape(27)
    n = X.shape[0]
    Z = np.einsum("bcv,ct->bvt", X, w1).reshape(n, 4, 4, 4, 27)
    o = np.arange(8)
    y1 = np.full((n, 8, 8, 8), float(b1))
    for t in range(27):
        iz, iy, ix = o + t // 9 - 1, o + (t // 3) % 3 - 1, o + t % 3 - 1
        mz, my, mx = (iz >= 0) & (iz < 8), (iy >= 0) & (iy < 8), (ix >= 0) & (ix < 8)
        y1[np.ix_(np.arange(n), o[mz], o[my], o[mx])] += \
            Z[np.ix_(np.arange(n), iz[mz] >> 1, iy[my] >> 1, ix[mx] >> 1)][..., t]
    y1 = np.maximum(y1, 0.0)

    def conv1(src, w, bias):
        out = np.full(src.shape, float(bias))
        for t in range(27):
            iz, iy, ix = o + t // 9 - 1, o + (t // 3) % 3 - 1, o + t % 3 - 1
            mz, my, mx = (iz >= 0) & (iz < 8), (iy >= 0) & (iy < 8), (ix >= 0) & (ix < 8)
            out[np.ix_(np.arange(n), o[mz], o[my], o[mx])] += \
                w[t] * src[np.ix_(np.arange(n), iz[mz], iy[my], ix[mx])]
        return out

    y3 = conv1(conv1(y1, w2, b2), w3, b3)
    return y3[:, :7, :7, :7].reshape(n, 343)


def to_f16(want):
    """float64 -> float16 NumPy array, rounded once to nearest-even."""
    w = want.numpy() if torch.is_tensor(want) else np.asarray(want)
    assert w.dtype == np.float64 and np.isfinite(w).all() and np.abs(w).max(initial=0.0) < 65504.0
    return w.astype(np.float16)


def f16_bracket(want):
    """(lo, hi) float16 arrays: the largest float16 <= want and the smallest float16 >= want
    (equal where want is representable)."""
    w = want.numpy() if torch.is_tensor(want) else np.asarray(want, dtype=np.float64)
    h = to_f16(w)
    hf = h.astype(np.float64)
    lo = np.where(hf <= w, h, np.nextafter(h, np.float16(-np.inf)))
    hi = np.where(hf >= w, h, np.nextafter(h, np.float16(np.inf)))
    assert (lo.astype(np.float64) <= w).all() and (w <= hi.astype(np.float64)).all()
    return lo.astype(np.float16), hi.astype(np.float16)


def f16_tie_distance(want):
    """float64 distance from want to the nearest boundary of float16 rounding: the midpoints
    between its rounded value and that value's two float16 neighbours.  A computed value closer
    to want than this rounds to the same float16 as want."""
    w = want.numpy() if torch.is_tensor(want) else np.asarray(want, dtype=np.float64)
    h = to_f16(w)
    hf = h.astype(np.float64)
    up = 0.5 * (hf + np.nextafter(h, np.float16(np.inf)).astype(np.float64))
    dn = 0.5 * (hf + np.nextafter(h, np.float16(-np.inf)).astype(np.float64))
    assert (dn <= w).all() and (w <= up).all()
    return np.minimum(up - w, w - dn)


def double_copy(decoder):
    """A float64 CPU copy of a PatchDecoder with no dense form."""
    d = copy.deepcopy(decoder).cpu().double().eval()
    d._dense = None
    return d


def head64(decoder, codes):
    """The decoder's head as its convolutions, in float64 on the CPU."""
    with torch.no_grad():
        return double_copy(decoder).head(_f64(codes))


def head_abs_terms64(decoder, codes):
    """The largest sum|terms| over every output of every convolution of the head: the head of a
    float64 copy with |weights|, |biases| and |codes| bounds it (|relu(s)| <= sum|terms of s|, by
    induction over the layers).  Below 2^24 with integer operands, float32 is exact in any order."""
    d = double_copy(decoder)
    worst = [0.0]
    hooks = []
    with torch.no_grad():
        for p in d.parameters():
            p.abs_()
        for m in d.modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.Conv3d)):
                hooks.append(m.register_forward_hook(
                    lambda mod, inp, out: worst.__setitem__(0, max(worst[0], float(out.max())))))
        d.head(_f64(codes).abs())
    for h in hooks:
        h.remove()
    return worst[0]


def exact_tail_case(rng, n):
    """(X, w1, b1, w2, b2, w3, b3) for n patches, float32 tensors / floats, exactly representable
    and small: X integers in [-3, 3], W1 and W2 integers in [-2, 2], W3 integers in [-1, 1] times
    2^-9, b1 = -5, b2 = 3, b3 = 0.25.  Every value of layers 1 and 2 is an integer and every value
    of layer 3 a multiple of 2^-9; sum|terms| of every output (in units of the layer's grid) is
    asserted below 2^24 -- at most 5 + 64*27*6 = 10373, then 3 + 27*2*10373 = 560145, then
    128 + 27*560145 = 15.1 M by construction -- so every partial sum in every order is a float32
    number: float32 evaluation is exact, and the only rounding is the last one, to float16."""
    X = torch.from_numpy(rng.integers(-3, 4, size=(n, 64, 4, 4, 4)).astype(np.float32))
    w1 = torch.from_numpy(rng.integers(-2, 3, size=(1, 64, 3, 3, 3)).astype(np.float32))
    w2 = torch.from_numpy(rng.integers(-2, 3, size=(1, 1, 3, 3, 3)).astype(np.float32))
    w3 = torch.from_numpy((rng.integers(-1, 2, size=(1, 1, 3, 3, 3)) * 2.0 ** -9).astype(np.float32))
    case = (X, w1, -5.0, w2, 3.0, w3, 0.25)
    L = tail_layers64(*case)
    assert float(L["A1"].max()) < 2 ** 24 and float(L["A2"].max()) < 2 ** 24 and \
        float(L["A3"].max()) * 2 ** 9 < 2 ** 24
    return case
