#!/usr/bin/env python3
"""tests/golden/patch_loss/*.npz (a folder of their own, as gt_affinities/ is): the reference's own
`MaskedBCEWithLogitsLoss` (experiments/flylight/setups/setup01/torch_loss.py:47-67) on the reference's own
`seg_to_affgraph_*_multi_torch*` targets (PatchPerPix/util/train_util.py), both imported in place with
`torchmetrics` and `gunpowder` stubbed, on small CPU tensors, in float64 and in float32, with autograd for the
gradient.  Development container only.

  python tests/golden/gen_golden_patch_loss.py

A file holds the inputs (`seg` int32, `nhood`, `logits` float32, and where the case has them `mask`, `box`,
`num_channels`, `samples`, `ps`, `psH`) and the reference's results `loss64`, `grad64`, `loss32`, `grad32`.  The
archives carry fixed time stamps.  The generator asserts that this project's `patch_loss_host` /
`patch_loss_samples_host` reproduce the float64 results to 1e-12 relative (the gradient: plus the reference's own
cancellation error, see `close`)."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "patch_loss")
REF = "/root/reference"

sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import gen_golden_gt_affinities as gg  # noqa: E402  (boxes, centred, raster and the fixed-stamp writer)


def load(name, path, stubs):
    for s in stubs:
        sys.modules.setdefault(s, types.ModuleType(s))
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_loss(ref_loss, target, logits, mask, num_channels, dtype):
    import torch
    fn = ref_loss.MaskedBCEWithLogitsLoss(reduction="none", num_channels=float(num_channels))
    x = torch.tensor(logits, dtype=dtype, requires_grad=True)
    m = None if mask is None else torch.tensor(mask, dtype=dtype)
    loss = fn(x, target.to(dtype), m)
    loss.backward()
    return loss.detach().numpy(), x.grad.numpy()


def close(a, b):
    """1e-12 relative, element by element.  The reference forms sigmoid(x) - g by SUBTRACTION: where sigmoid(x)
    rounds next to 1 its gradient carries that one rounding, 2^-53 of the largest gradient's scale, whatever the
    element's own size (measured here: up to 3e-11 of a gradient of 5e-9) -- so that much of the largest
    magnitude is allowed on top.  It is zero for a scalar loss."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    floor = 2.0 ** -52 * np.abs(b).max() if b.ndim else 0.0
    return bool(np.all(np.abs(a - b) <= 1e-12 * np.abs(b) + floor))


def dense_case(refs, name, seg, nhood, ndim, seed, mask=None, box=None, num_channels=None):
    import torch
    from patchperpix_amd import train_loss
    ref_tu, ref_loss = refs
    rng = np.random.default_rng(seed)
    fn = "seg_to_affgraph_%dd_multi_torch" % ndim
    target = getattr(ref_tu, fn)(torch.from_numpy(seg), nhood, "cpu")
    if box is not None:
        target = target[(slice(None), slice(None)) + tuple(slice(a, b) for a, b in zip(box[0::2], box[1::2]))]
    assert 0 < float(target.mean()) < 1, name
    logits = (4.0 * rng.standard_normal(target.shape)).astype(np.float32)
    nc = float(len(nhood) if num_channels is None else num_channels)
    arrays = dict(seg=seg, nhood=nhood, logits=logits)
    for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
        loss, grad = reference_loss(ref_loss, target, logits, mask, nc, dtype)
        arrays["loss" + tag], arrays["grad" + tag] = loss, grad
    # this project's definition: the mask's channel rule, 2-d lifted to 3-d
    weight = None
    if mask is not None:
        weight = mask[:, 0 if mask.shape[1] == 1 else 1]
        arrays["mask"] = mask
        arrays["num_channels"] = np.float64(nc)
    seg5, n3 = gg.lift(seg, nhood, ndim, False)
    box3 = None
    if box is not None:
        arrays["box"] = np.array(box, dtype=np.int64)
        box3 = tuple(box) if ndim == 3 else (0, 1) + tuple(box)
    lift = lambda a: a.reshape(a.shape[:-ndim] + (1,) * (3 - ndim) + a.shape[-ndim:])
    loss, grad = train_loss.patch_loss_host(lift(logits), seg5, n3, None if weight is None else lift(weight), box3, nc)
    assert close(loss, arrays["loss64"]) and close(grad.reshape(logits.shape), arrays["grad64"]), name
    gg.OUT = OUT
    gg.save(name, **arrays)
    return arrays


def main():
    refs = (load("ppp_ref_train_util", os.path.join(REF, "PatchPerPix", "util", "train_util.py"), ["gunpowder"]),
            load("ppp_ref_torch_loss", os.path.join(REF, "experiments", "flylight", "setups", "setup01", "torch_loss.py"),
                 ["torchmetrics"]))
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(201)
    spatial = (3, 4, 6)
    seg = np.stack([gg.boxes(rng, 2, spatial, 6, first_id=3 + 50 * b) for b in range(2)])
    assert ((seg != 0).sum(axis=1) > 1).any(), "no overlap voxel"
    nhood = np.array([[0, 0, 0], [0, 0, 1], [0, 0, -1], [0, 1, 0], [0, -1, 0], [1, 0, 0], [-1, 0, 0], [1, 1, -1], [0, 0, 2]])
    dense_case(refs, "d3_nomask", seg, nhood, 3, 1)
    frac = rng.random((2, 1) + spatial).astype(np.float32)
    frac[frac < 0.3] = 0
    dense_case(refs, "d3_cm1", seg, nhood, 3, 2, mask=frac, num_channels=27.0)
    two = np.stack([rng.random((2,) + spatial) < 0.5, rng.random((2,) + spatial) < 0.6], axis=1).astype(np.float32)
    assert not np.array_equal(two[:, 0], two[:, 1])
    dense_case(refs, "d3_cm2", seg, nhood, 3, 3, mask=two)
    got = dense_case(refs, "d3_zero", seg, nhood, 3, 4, mask=np.zeros((2, 1) + spatial, dtype=np.float32))
    assert float(got["loss64"]) == 0 and not got["grad64"].any()
    box = (1, 3, 0, 3, 1, 6)
    crop = tuple(slice(a, b) for a, b in zip(box[0::2], box[1::2]))
    dense_case(refs, "d3_box", seg, nhood, 3, 5, mask=frac[(slice(None), slice(None)) + crop], box=box)
    seg2 = np.stack([gg.boxes(rng, 2, (7, 9), 5, first_id=2 + 30 * b) for b in range(2)])
    m2 = np.stack([rng.random((2, 7, 9)) < 0.5, rng.random((2, 7, 9)) < 0.7], axis=1).astype(np.float32)
    dense_case(refs, "d2_cm2", seg2, gg.centred(1, 2), 2, 6, mask=m2)

    # sampled: N = 5 with a duplicate row
    import torch
    from patchperpix_amd import train_loss
    ps, psH = 3, 1
    segs = np.stack([gg.boxes(rng, 2, (5, 6, 7), 8, first_id=4 + 90 * b) for b in range(2)])
    rows = np.array([[0, 0, 0, 0], [1, 2, 3, 4], [0, 1, 2, 3], [1, 2, 3, 4], [1, 0, 1, 2]], dtype=np.int64)
    raster = gg.raster(ps, 3)
    target = refs[0].seg_to_affgraph_3d_multi_torch_code(torch.from_numpy(segs), raster, "cpu", ps, psH, rows)
    assert tuple(target.shape) == (5, 27) and 0 < float(target.mean()) < 1
    logits = (4.0 * np.random.default_rng(7).standard_normal(target.shape)).astype(np.float32)
    arrays = dict(seg=segs, nhood=raster, logits=logits, samples=rows, ps=np.int64(ps), psH=np.int64(psH))
    for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
        arrays["loss" + tag], arrays["grad" + tag] = reference_loss(refs[1], target, logits, None, 27.0, dtype)
    loss, grad = train_loss.patch_loss_samples_host(logits, segs, rows, raster, (ps,) * 3, (psH,) * 3)
    assert close(loss, arrays["loss64"]) and close(grad, arrays["grad64"])
    gg.OUT = OUT
    gg.save("s3_n5", **arrays)
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    assert total < 300000, total
    print("total %d bytes" % total)


if __name__ == "__main__":
    main()
