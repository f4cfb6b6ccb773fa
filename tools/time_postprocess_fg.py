#!/usr/bin/env python3
"""Times `postprocess_fg`'s component filter from the device (postprocess.fg_filter_device: upload, the
kernels of csrc/ppp_edt.hip and csrc/ppp_postprocess.hip, download) against the host path on the same
mask (postprocess.fg_filter: ndimage.label, np.bincount, distance_transform_edt), asserts that both give
the same foreground, instances and counts, and prints one JSON line per case and a table at the end.

Input: a thresholded synthetic foreground prediction -- synth.tube_labels (thin tubes, a few percent
foreground) at 0.9, background at 0.1, and hashed speckles (one voxel in 400) at 0.8 that the threshold
0.5 turns into small components near to and far from the tubes -- at 140^3 and 512^3, with
remove_small_comps = 100 and max_distance_to_fg = 10, cc_instances on.

`device_s` is the wall time of the call on a NumPy mask, the best of --reps after a warm-up call;
`kernels_ms` the time between HIP events around the entry point in that call; `host_s` one host call.

    python tools/time_postprocess_fg.py [--sizes 140 512] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REMOVE_SMALL_COMPS = 100
MAX_DISTANCE_TO_FG = 10
FG_THRESHOLD = 0.5


def foreground(n, seed=0):
    from patchperpix_amd import synth
    tubes = synth.tube_labels((n, n, n), n_tubes=max(14, 14 * n // 140), radius=2.5, seed=seed) != 0
    pred = np.where(tubes, np.float32(0.9), np.float32(0.1))
    for z0 in range(0, n, 64):                      # (slabs: the hash works on uint64 temporaries)
        lin = np.arange(z0 * n * n, min(z0 + 64, n) * n * n, dtype=np.uint64) + np.uint64(seed * 0x9E3779B1)
        speckle = (synth.hash_u32(lin) % 400 == 0).reshape(-1, n, n)
        pred[z0:z0 + 64][speckle] = 0.8
    return pred


def time_size(n, reps):
    import torch
    from patchperpix_amd import backend, postprocess
    assert torch.cuda.is_available(), "time_postprocess_fg.py needs a GPU"
    mask = foreground(n) > FG_THRESHOLD
    args = (mask, REMOVE_SMALL_COMPS, MAX_DISTANCE_TO_FG, True)
    postprocess.fg_filter_device(*args)             # warm-up: library load, allocator, first launches
    best = kernels = dev = None
    for _ in range(reps):
        backend.EVENTS = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev = postprocess.fg_filter_device(*args)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if best is None or dt < best:
            best, kernels = dt, round(sum(sum(v) for v in backend.event_times_ms().values()), 3)
        backend.EVENTS = None
    t0 = time.perf_counter()
    host = postprocess.fg_filter(*args)
    t_host = time.perf_counter() - t0
    assert np.array_equal(dev[0], host[0]), "foreground differs"
    assert np.array_equal(dev[1], host[1]), "instances differ"
    assert dev[2] == host[2], "counts differ"
    found, small, removed, kept = dev[2]
    res = {"shape": [n, n, n], "foreground_voxels": int(mask.sum()), "components": found, "small": small,
           "removed": removed, "kept": kept, "min_d2": postprocess.min_sq_distance(MAX_DISTANCE_TO_FG),
           "device_s": round(best, 4), "kernels_ms": kernels, "host_s": round(t_host, 3)}
    print(json.dumps(res), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[140, 512])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args(argv)
    rows = [time_size(n, args.reps) for n in args.sizes]
    print("\n%-8s %12s %11s %9s %9s %10s %11s %9s %8s" % ("volume", "fg voxels", "components", "small", "removed",
                                                         "device_s", "kernels_ms", "host_s", "host/dev"))
    for r in rows:
        print("%-8s %12d %11d %9d %9d %10.4f %11.3f %9.3f %8.1f" % (
            "%d^3" % r["shape"][0], r["foreground_voxels"], r["components"], r["small"], r["removed"], r["device_s"],
            r["kernels_ms"], r["host_s"], r["host_s"] / r["device_s"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
