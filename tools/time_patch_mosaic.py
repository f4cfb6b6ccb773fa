#!/usr/bin/env python3
"""Times `ppp_patch_mosaic` (csrc/ppp_mosaic.hip: the patch mosaic of visualize_patches as one pass over the
prediction) against the host definition `visualize.patches.mosaic_host`, asserts that both give the same bits
BEFORE any time is printed, and prints one JSON line per case and a table at the end.

Cases: the shape of flylight140_p7 -- 343 x 140^3, float16 -- and a 2-d image, 625 x 1 x 696 x 520 (25 x 25
patches, float16).  The prediction is uniform noise made on the device.

`kernel_ms`: the time between HIP events around the entry point, the median of --reps calls after --warmup calls in
one process, with the spread (min .. max).  `gbps`: (input + output) bytes divided by that time -- the input
counted whole, although the channels with j == 0 or i == 0 are never read (`gbps_read` counts what is read).
`copy_ms` / `copy_gbps`: the yardstick, measured in the same run between the same events: a device-to-device
`Tensor.copy_` that moves the same number of bytes (half of them read, half written).  `host_s`: one call of
mosaic_host on the whole array.  `loop_s_est`: the reference-style loop over the voxels (one tile assignment
and, in 3-d, one np.max per voxel) timed on a crop of --loop-crop voxels per side and scaled by the voxel count:
an ESTIMATE.

    python tools/time_patch_mosaic.py [--cases p7 img2d] [--reps 7] [--warmup 2] [--loop-crop 32]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {                       # volume, patch
    "p7": ((140, 140, 140), (7, 7, 7)),
    "img2d": ((1, 696, 520), (1, 25, 25)),
}


def event_ms(fn, reps, warmup):
    import torch
    times = []
    for k in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(a.elapsed_time(b))
    return times


def voxel_loop(crop, patch):
    """the reference's loop (patches.py:35-45, 86-96) on a copy of `crop`: what it costs per voxel"""
    C, Z, Y, X = crop.shape
    pz, py, px = patch
    arr = crop.copy()
    out = np.zeros((Z, Y * py, X * px), dtype=arr.dtype)
    t0 = time.perf_counter()
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                p = arr[:, z, y, x].reshape(patch)
                p[:, 0, :] = 1
                p[:, :, 0] = 1
                out[z, y * py:(y + 1) * py, x * px:(x + 1) * px] = np.max(p, axis=0) if pz > 1 else p[0]
    return time.perf_counter() - t0, out


def time_case(name, reps, warmup, loop_crop):
    import torch
    from patchperpix_amd import backend
    from patchperpix_amd.visualize import patches
    assert torch.cuda.is_available(), "time_patch_mosaic.py needs a GPU"
    shape, patch = CASES[name]
    C = patch[0] * patch[1] * patch[2]
    torch.manual_seed(0)
    pred = torch.rand((C,) + shape, device="cuda", dtype=torch.float16)
    out = torch.empty((shape[0], shape[1] * patch[1], shape[2] * patch[2]), device="cuda", dtype=torch.float16)
    backend.patch_mosaic(pred, patch, out=out)
    torch.cuda.synchronize()
    host_in = pred.cpu().numpy()
    t0 = time.perf_counter()
    want = patches.mosaic_host(host_in, patch)
    t_host = time.perf_counter() - t0
    assert np.array_equal(out.cpu().numpy().view(np.uint16), want.view(np.uint16)), "device and host mosaics differ"
    t_kernel = event_ms(lambda: backend.patch_mosaic(pred, patch, out=out), reps, warmup)
    in_bytes, out_bytes = pred.numel() * 2, out.numel() * 2
    read_bytes = in_bytes // (patch[1] * patch[2]) * ((patch[1] - 1) * (patch[2] - 1))
    half = (in_bytes + out_bytes) // 2 // 16 * 16
    src = torch.empty(half, dtype=torch.uint8, device="cuda").random_(0, 255)
    dst = torch.empty_like(src)
    t_copy = event_ms(lambda: dst.copy_(src), reps, warmup)
    n = min(loop_crop, *[s for s in shape if s > 1])
    crop = host_in[:, :min(n, shape[0]), :n, :n]
    t_loop, loop_out = voxel_loop(crop, patch)
    assert np.array_equal(loop_out.view(np.uint16), patches.mosaic_host(crop, patch).view(np.uint16)), "the loop differs"
    med, med_c = statistics.median(t_kernel), statistics.median(t_copy)
    res = {"case": name, "pred_shape": [C] + list(shape), "dtype": "float16", "in_gb": round(in_bytes / 1e9, 3),
           "out_gb": round(out_bytes / 1e9, 3), "kernel_ms": round(med, 3),
           "kernel_ms_min_max": [round(min(t_kernel), 3), round(max(t_kernel), 3)],
           "gbps": round((in_bytes + out_bytes) / med / 1e6, 1), "gbps_read": round((read_bytes + out_bytes) / med / 1e6, 1),
           "copy_ms": round(med_c, 3), "copy_ms_min_max": [round(min(t_copy), 3), round(max(t_copy), 3)],
           "copy_gbps": round(2 * half / med_c / 1e6, 1), "host_s": round(t_host, 2),
           "loop_crop_voxels": int(np.prod(crop.shape[1:])), "loop_crop_s": round(t_loop, 2),
           "loop_s_est": round(t_loop * float(np.prod(shape)) / float(np.prod(crop.shape[1:])), 1)}
    print(json.dumps(res), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-crop", type=int, default=32)
    args = ap.parse_args(argv)
    rows = [time_case(c, args.reps, args.warmup, args.loop_crop) for c in args.cases]
    print("\n%-6s %-20s %7s %7s %10s %9s %9s %9s %10s %8s %12s" % (
        "case", "prediction", "in GB", "out GB", "kernel ms", "GB/s", "read GB/s", "copy ms", "copy GB/s", "host s", "loop s (est)"))
    for r in rows:
        print("%-6s %-20s %7.3f %7.3f %10.3f %9.1f %9.1f %9.3f %10.1f %8.2f %12.1f" % (
            r["case"], "x".join(map(str, r["pred_shape"])), r["in_gb"], r["out_gb"], r["kernel_ms"], r["gbps"],
            r["gbps_read"], r["copy_ms"], r["copy_gbps"], r["host_s"], r["loop_s_est"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
