#!/usr/bin/env python3
"""Times the ground-truth patch affinities kernels (csrc/ppp_gt_affs.hip: `backend.gt_affs_dense`,
`backend.gt_affs_samples`) and asserts, BEFORE any time is printed, that every timed result equals the
definition written as plain torch operations on the device in this file (`plain_torch_dense`: per edge one
shifted compare, an `any` over the channels and one assignment).

Cases: `synth.tube_labels` at 140^3 with three seeds stacked to L = 3 and the centred 7^3 nhood -- dense float32
and float16, the whole volume and the box torch_model.py:432-441 crops to (the patch radius off every face);
a 2-d image of 696 x 520 with discs in two channels and a 25 x 25 nhood; the sampled form with N = 1024 rows at
foreground voxels, ps = 7, against the dense kernel plus a gather of those rows.

`device_ms`: the time between HIP events around the entry point, the median of --reps calls after --warmup
calls, with minimum and maximum; `copy_ms`: a device-to-device copy of the output's byte count in the same run
(`ratio_to_copy` = copy / kernel); `torch_ms`: `plain_torch_dense` in the same run, timed the same way.  The
run fails unless the slowest kernel call of a dense case is faster than the fastest plain-torch call.

    python tools/time_gt_affinities.py [--cases ...] [--reps 7] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ["tubes_f32", "tubes_f16", "tubes_crop_f32", "tubes_crop_f16", "image_2d", "sampled"]


def centred(r):
    g = np.meshgrid(*[np.arange(-a, a + 1) for a in r], indexing="ij")
    return np.stack([a.reshape(-1) for a in g], axis=1).astype(np.int32)


def tube_stack(shape=(140, 140, 140), L=3):
    from patchperpix_amd import synth
    return np.stack([synth.tube_labels(shape, n_tubes=14, radius=2.5, seed=s).astype(np.int32) for s in range(L)])[None]


def disc_image(shape=(696, 520), L=2, n=60, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    seg = np.zeros((L, 1) + shape, dtype=np.int32)
    for k in range(n):
        cy, cx, r = rng.integers(0, shape[0]), rng.integers(0, shape[1]), rng.integers(8, 26)
        seg[k % L, 0][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k + 1
    return seg[None]


def plain_torch_dense(labels, nhood, box, out_dtype):
    """The definition on the device with plain torch operations: `labels` (B, L, Z, Y, X), `nhood` a host (E, 3)
    array, `box` (z0, z1, y0, y1, x0, x1).  aff[b, e, v] = 1 iff v + n lies inside the volume and some channel
    holds the same non-zero id at v and at v + n."""
    import torch
    size = labels.shape[2:]
    lo0, hi0 = box[0::2], box[1::2]
    out = torch.zeros((labels.shape[0], len(nhood)) + tuple(b - a for a, b in zip(lo0, hi0)), dtype=out_dtype,
                      device=labels.device)
    for e, n in enumerate(nhood.tolist()):
        lo = [max(a, -d) for a, d in zip(lo0, n)]
        hi = [min(b, s - d) for b, s, d in zip(hi0, size, n)]
        if any(a >= b for a, b in zip(lo, hi)):
            continue
        c = labels[:, :, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        o = labels[:, :, lo[0] + n[0]:hi[0] + n[0], lo[1] + n[1]:hi[1] + n[1], lo[2] + n[2]:hi[2] + n[2]]
        out[:, e, lo[0] - lo0[0]:hi[0] - lo0[0], lo[1] - lo0[1]:hi[1] - lo0[1], lo[2] - lo0[2]:hi[2] - lo0[2]] = \
            ((c == o) & (c != 0)).any(dim=1)
    return out


def timed(fn, reps, warmup):
    """median, minimum, maximum of the device time of fn() in ms, between HIP events"""
    import torch
    times = []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def timed_entry(fn, name, reps, warmup):
    """the same of the backend's own HIP events around the entry point `name`"""
    import torch
    from patchperpix_amd import backend
    times = []
    for k in range(warmup + reps):
        backend.EVENTS = {}
        fn()
        torch.cuda.synchronize()
        ms = sum(backend.event_times_ms()[name])
        backend.EVENTS = None
        if k >= warmup:
            times.append(ms)
    return statistics.median(times), min(times), max(times)


def dense_case(name, labels, nhood, box, out_dtype, reps, warmup):
    import torch
    from patchperpix_amd import backend
    d_labels = torch.from_numpy(labels).cuda()
    d_nhood = torch.from_numpy(nhood).cuda()
    out = backend.gt_affs_dense(d_labels, d_nhood, box=box, out_dtype=out_dtype)
    ref = plain_torch_dense(d_labels, nhood, box, out_dtype)
    torch.cuda.synchronize()
    assert torch.equal(out, ref), "%s: the kernel and the plain torch definition differ" % name
    ones = float(out.float().mean())
    del ref
    k = timed_entry(lambda: backend.gt_affs_dense(d_labels, d_nhood, box=box, out=out), "gt_affs_dense", reps, warmup)
    dst = torch.empty_like(out)
    c = timed(lambda: dst.copy_(out), reps, warmup)
    del dst
    t = timed(lambda: plain_torch_dense(d_labels, nhood, box, out_dtype), reps, min(warmup, 1))
    nbytes = out.numel() * out.element_size()
    vol = labels.shape[2:]
    plan = backend.gt_affs_dense_plan(labels.shape[0], labels.shape[1], vol, len(nhood), backend.nhood_halo(d_nhood), box,
                                      out_dtype)
    res = {"case": name, "labels": list(labels.shape), "E": int(len(nhood)), "box": list(box), "dtype": str(out_dtype)[6:],
           "out_mb": round(nbytes / 1e6, 1), "ones": round(ones, 5), "tile": list(plan[:3]), "staged": plan[3],
           "edge_ranges": plan[4], "device_ms": round(k[0], 3), "device_ms_min_max": [round(k[1], 3), round(k[2], 3)],
           "gbps": round(nbytes / k[0] / 1e6, 1), "copy_ms": round(c[0], 3), "copy_ms_min_max": [round(c[1], 3), round(c[2], 3)],
           "ratio_to_copy": round(c[0] / k[0], 3), "torch_ms": round(t[0], 3),
           "torch_ms_min_max": [round(t[1], 3), round(t[2], 3)], "torch_over_kernel": round(t[0] / k[0], 1)}
    print(json.dumps(res), flush=True)
    assert k[2] < t[1], "%s: the kernel (slowest call %.3f ms) does not beat plain torch (fastest call %.3f ms)" % (name, k[2], t[1])
    return res


def sampled_case(reps, warmup, N=1024, ps=7):
    import torch
    from patchperpix_amd import backend
    labels = tube_stack()
    rng = np.random.default_rng(0)
    psH = ps // 2
    fg = np.argwhere((labels[0] != 0).any(axis=0)[psH:-psH, psH:-psH, psH:-psH])        # centres whose patch fits: corners
    rows = np.concatenate([np.zeros((N, 1), dtype=np.int64), fg[rng.integers(0, len(fg), N)]], axis=1).astype(np.int32)
    raster = (centred((psH,) * 3) + psH).astype(np.int32)
    d_labels, d_rows, d_raster = torch.from_numpy(labels).cuda(), torch.from_numpy(rows).cuda(), torch.from_numpy(raster).cuda()
    d_centred = torch.from_numpy(centred((psH,) * 3)).cuda()
    out = backend.gt_affs_samples(d_labels, d_rows, d_raster, (ps,) * 3, (psH,) * 3)
    at = (d_rows[:, 1:] + psH).long()

    def dense_and_gather():
        dense = backend.gt_affs_dense(d_labels, d_centred)
        return dense[0][:, at[:, 0], at[:, 1], at[:, 2]].t().contiguous()
    ref = dense_and_gather()
    torch.cuda.synchronize()
    assert torch.equal(out, ref), "sampled: the rows differ from the dense result at loc + psH"
    ones = float(out.mean())
    del ref
    k = timed_entry(lambda: backend.gt_affs_samples(d_labels, d_rows, d_raster, (ps,) * 3, (psH,) * 3, out=out),
                    "gt_affs_samples", reps, warmup)
    t = timed(dense_and_gather, reps, min(warmup, 1))
    res = {"case": "sampled", "labels": list(labels.shape), "N": N, "E": int(len(raster)), "ones": round(ones, 5),
           "device_ms": round(k[0], 4), "device_ms_min_max": [round(k[1], 4), round(k[2], 4)],
           "dense_plus_gather_ms": round(t[0], 3), "dense_plus_gather_ms_min_max": [round(t[1], 3), round(t[2], 3)]}
    print(json.dumps(res), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=CASES, choices=CASES)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "time_gt_affinities.py needs a GPU"
    rows, sampled = [], None
    tubes = tube_stack() if any(c.startswith("tubes") for c in args.cases) else None
    n7 = centred((3, 3, 3))
    for c in args.cases:
        if c.startswith("tubes"):
            dt = torch.float16 if c.endswith("f16") else torch.float32
            box = (3, 137) * 3 if "crop" in c else (0, 140) * 3
            rows.append(dense_case(c, tubes, n7, box, dt, args.reps, args.warmup))
        elif c == "image_2d":
            n25 = centred((0, 12, 12))
            rows.append(dense_case(c, disc_image(), n25, (0, 1, 0, 696, 0, 520), torch.float32, args.reps, args.warmup))
        else:
            sampled = sampled_case(args.reps, args.warmup)
        torch.cuda.empty_cache()
    if rows:
        print("\n%-15s %-8s %5s %9s %10s %16s %9s %9s %7s %10s %8s" % ("case", "dtype", "E", "out MB", "device ms", "min .. max",
                                                                      "GB/s", "copy ms", "ratio", "torch ms", "torch/k"))
        for r in rows:
            print("%-15s %-8s %5d %9.1f %10.3f %7.3f .. %-6.3f %9.1f %9.3f %7.3f %10.3f %8.1f" % (
                r["case"], r["dtype"], r["E"], r["out_mb"], r["device_ms"], r["device_ms_min_max"][0], r["device_ms_min_max"][1],
                r["gbps"], r["copy_ms"], r["ratio_to_copy"], r["torch_ms"], r["torch_over_kernel"]))
    if sampled:
        print("\nsampled: N = %d, E = %d: %.4f ms (%.4f .. %.4f); dense kernel + gather %.3f ms" % (
            sampled["N"], sampled["E"], sampled["device_ms"], sampled["device_ms_min_max"][0], sampled["device_ms_min_max"][1],
            sampled["dense_plus_gather_ms"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
