#!/usr/bin/env python3
"""Times the fused patch loss from the labels (csrc/ppp_patch_loss.hip through
`train_loss.patch_bce_from_labels`), forward + backward, against the unfused path of this project:
`train_util.seg_to_affgraph_3d_multi_torch(box=)` on the device, torch's `binary_cross_entropy_with_logits`,
the mask and autograd -- the reference's MaskedBCEWithLogitsLoss on a stored target.

Cases: `synth.tube_labels` at 140^3 with three seeds stacked to L = 3 and the centred 7^3 nhood; the whole
volume and the 134^3 box torch_model.py:432-441 crops to; float32 and bfloat16 logits; with and without a mask.

Before any time is printed the fused loss and gradient are compared with the definition evaluated in float64 on
the device (plain torch, in slabs of 49 edges, on the exactly widened logits) within the tolerances of
tests/test_patch_loss_gpu.py, and the unfused loss with the same value (in bfloat16 the unfused path rounds its
loss map and its sum into that type: 2^-6 there).

`ms`: forward + backward between HIP events, the median of --reps calls with minimum and maximum, the two paths
ALTERNATING in one process; `copy_ms`: a device-to-device copy of the logits' bytes in the same run, and the
ratios to it as they come out; `peak_mb`: what `torch.cuda.max_memory_allocated` rises by over the inputs.  The
run fails unless the slowest fused call of the 134^3 crop is faster than the fastest unfused one.

    python tools/time_patch_loss.py [--cases ...] [--reps 7] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ["%s_%s_%s" % (v, d, m) for v in ("full", "crop") for d in ("f32", "bf16") for m in ("mask", "nomask")]
U = 2.0 ** -24


def centred(r):
    g = np.meshgrid(*[np.arange(-a, a + 1) for a in r], indexing="ij")
    return np.stack([a.reshape(-1) for a in g], axis=1).astype(np.int32)


def tube_stack(shape=(140, 140, 140), L=3):
    from patchperpix_amd import synth
    return np.stack([synth.tube_labels(shape, n_tubes=14, radius=2.5, seed=s).astype(np.int32) for s in range(L)])[None]


def run_case(name, d_labels, d_nhood, box, dtype, masked, reps, warmup):
    import torch
    import torch.nn.functional as F
    from patchperpix_amd import train_loss, train_util
    E = int(d_nhood.shape[0])
    ext = (box[1] - box[0], box[3] - box[2], box[5] - box[4])
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = (4 * torch.randn((1, E) + ext, generator=gen, device="cuda")).to(dtype).requires_grad_(True)
    mask = (torch.rand((1, 1) + ext, generator=gen, device="cuda") < 0.7).float() if masked else None
    nbytes = x.numel() * x.element_size()

    def fused():
        x.grad = None
        loss = train_loss.patch_bce_from_labels(x, d_labels, d_nhood, mask, box=box, num_channels=float(E), check=False)
        loss.backward()
        return loss

    def unfused():
        x.grad = None
        target = train_util.seg_to_affgraph_3d_multi_torch(d_labels, d_nhood, "cuda", check=False, box=box, out_dtype=dtype)
        loss = F.binary_cross_entropy_with_logits(x, target, reduction="none")
        if mask is not None:
            loss = torch.sum(loss * mask[:, 0].unsqueeze(1)) / (torch.sum(mask[:, 0]) * float(E))
        else:
            loss = loss.mean()
        loss.backward()
        return loss

    def peak(fn):
        x.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn().item()
        torch.cuda.synchronize()
        return out, x.grad, (torch.cuda.max_memory_allocated() - base) / 1e6

    # ---- compare before any time is printed ----
    lf, gf, peak_f = peak(fused)
    lu, gu, peak_u = peak(unfused)
    # the definition in float64 on the device, in slabs of 49 edges, on the exactly widened logits
    target = train_util.seg_to_affgraph_3d_multi_torch(d_labels, d_nhood, "cuda", check=False, box=box, out_dtype=dtype)
    w = None if mask is None else mask[:, 0].unsqueeze(1).double()
    cnt = float(x.numel()) if mask is None else float(E) * float(mask[:, 0].double().sum())
    total, worst = torch.zeros((), dtype=torch.float64, device="cuda"), 0.0
    for e0 in range(0, E, 49):
        xs, g = x.detach()[:, e0:e0 + 49].double(), target[:, e0:e0 + 49] > 0
        t = torch.exp(-xs.abs())
        r = 1.0 / (1.0 + t)
        elem = torch.where(g, (-xs).clamp(min=0), xs.clamp(min=0)) + torch.log1p(t)
        slope = torch.where(g, -torch.where(xs >= 0, t * r, r), torch.where(xs >= 0, r, t * r))
        if w is not None:
            elem, slope = elem * w, slope * w
        total += elem.sum()
        want = slope / cnt
        # float32: 32 u relative; bfloat16: the two neighbours of such a value, one unit of its 8 bits
        tol = 32 * U * want.abs() + (2.0 ** -126 if dtype == torch.float32 else 2.0 ** -8 * want.abs() + 2.0 ** -133)
        worst = max(worst, ((gf[:, e0:e0 + 49].double() - want).abs() - tol).max().item())
        del xs, g, t, r, elem, slope, want, tol
    l64 = (total / cnt).item()
    assert abs(lf - l64) <= (E + 33) * U * l64, "%s: the fused loss %r is not the definition's %r" % (name, lf, l64)
    assert worst <= 0, "%s: the fused gradient leaves its tolerance by %r" % (name, worst)
    # the unfused path rounds its loss map and its sum into the logits' type
    assert abs(lu - l64) <= ((E + 33) * U if dtype == torch.float32 else 2.0 ** -6) * l64, \
        "%s: the unfused loss %r is not the definition's %r" % (name, lu, l64)
    del gf, gu, target
    x.grad = None

    # ---- time, alternating ----
    tf, tun, tc = [], [], []
    dst = torch.empty_like(x)
    for k in range(warmup + reps):
        for fn, into in ((fused, tf), (unfused, tun), (lambda: dst.copy_(x.detach()), tc)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if k >= warmup:
                into.append(e0.elapsed_time(e1))
    stat = lambda t: (statistics.median(t), min(t), max(t))
    f, u, c = stat(tf), stat(tun), stat(tc)
    res = {"case": name, "box": list(box), "E": E, "dtype": str(dtype)[6:], "mask": bool(masked), "logits_mb": round(nbytes / 1e6, 1),
           "loss": lf, "fused_ms": round(f[0], 3), "fused_ms_min_max": [round(f[1], 3), round(f[2], 3)],
           "unfused_ms": round(u[0], 3), "unfused_ms_min_max": [round(u[1], 3), round(u[2], 3)],
           "copy_ms": round(c[0], 3), "copy_ms_min_max": [round(c[1], 3), round(c[2], 3)],
           "fused_over_copy": round(f[0] / c[0], 2), "unfused_over_copy": round(u[0] / c[0], 2),
           "unfused_over_fused": round(u[0] / f[0], 2), "fused_peak_mb": round(peak_f, 1), "unfused_peak_mb": round(peak_u, 1)}
    print(json.dumps(res), flush=True)
    if name.startswith("crop"):
        assert f[2] < u[1], "%s: the fused path (slowest call %.3f ms) does not beat the unfused one (fastest %.3f ms)" % (
            name, f[2], u[1])
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=CASES, choices=CASES)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "time_patch_loss.py needs a GPU"
    d_labels = torch.from_numpy(tube_stack()).cuda()
    d_nhood = torch.from_numpy(centred((3, 3, 3))).cuda()
    rows = []
    for c in args.cases:
        v, d, m = c.split("_")
        box = (3, 137) * 3 if v == "crop" else (0, 140) * 3
        rows.append(run_case(c, d_labels, d_nhood, box, torch.float32 if d == "f32" else torch.bfloat16, m == "mask",
                             args.reps, args.warmup))
        torch.cuda.empty_cache()
    print("\n%-18s %9s %10s %16s %11s %16s %8s %7s %7s %6s %9s %9s" % (
        "case", "logits MB", "fused ms", "min .. max", "unfused ms", "min .. max", "copy ms", "f/copy", "u/copy", "u/f",
        "f peak MB", "u peak MB"))
    for r in rows:
        print("%-18s %9.1f %10.3f %7.3f .. %-6.3f %11.3f %7.3f .. %-6.3f %8.3f %7.2f %7.2f %6.2f %9.1f %9.1f" % (
            r["case"], r["logits_mb"], r["fused_ms"], r["fused_ms_min_max"][0], r["fused_ms_min_max"][1], r["unfused_ms"],
            r["unfused_ms_min_max"][0], r["unfused_ms_min_max"][1], r["copy_ms"], r["fused_over_copy"], r["unfused_over_copy"],
            r["unfused_over_fused"], r["fused_peak_mb"], r["unfused_peak_mb"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
