#!/usr/bin/env python3
"""Times the 3-d thinning behind `skeletonize_foreground` from the device (csrc/ppp_skeleton.hip,
backend.skeletonize_3d) against the host function that defines it (ppp_host_skeletonize_3d) on the same
mask, asserts that both give the same array, and prints one JSON line per case.

Cases:
  flylight140_p7   the foreground of bench.py's default workload (140^3, dense blobs: many rounds)
  tubes140 / tubes256 / tubes512
                   synth.tube_labels (the generator behind make_case(kind="tubes")) at N^3 with
                   radius 2.5 and 30 tubes at 140^3 (3.4 % foreground, the case of time_s1_sparse.py), the
                   tube count scaled with N^2 so that the foreground fraction stays (the flylight regime)

`device_s` is the wall time of backend.skeletonize_3d on a NumPy array (what a driver pays: upload,
kernels, counter read-backs, download), best of --reps after a warm-up; `entry_ms` the time between HIP
events around the entry point in that run; `host_s` one run of the host function.  `stats` = passes,
sub-iterations, rounds.  The host runs at 512^3 only when its 256^3 run took under five minutes;
otherwise `host_s_estimate` scales the 256^3 time with the voxel count -- an estimate, labelled as one.

    python tools/time_skeleton.py [--cases flylight140_p7 tubes140 tubes256 tubes512] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOST_LIMIT_S = 300.0


def flylight140():
    import torch
    import bench
    shape, ps, cell = bench.WORKLOADS["flylight140_p7"]
    return (bench.device_labels(torch, shape, cell, seed=0) != 0).cpu().numpy()


def tubes(n):
    from patchperpix_amd import synth
    n_tubes = max(1, int(round(30 * (n / 140.0) ** 2)))
    return synth.tube_labels((n, n, n), n_tubes=n_tubes, radius=2.5, seed=0) != 0


def best_of(fn, reps):
    import torch
    from patchperpix_amd import backend
    fn()                                    # warm-up: library load, allocator, first launches
    best, entry, out = None, None, None
    for _ in range(reps):
        backend.EVENTS = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if best is None or dt < best:
            best, entry = dt, round(sum(sum(v) for v in backend.event_times_ms().values()), 3)
        backend.EVENTS = None
    return out, best, entry


def run_case(name, mask, reps, host_256_s):
    from patchperpix_amd import backend
    res = {"case": name, "shape": list(mask.shape), "foreground": int(mask.sum()),
           "foreground_frac": round(float(mask.mean()), 4)}
    dev, t_dev, entry = best_of(lambda: backend.skeletonize_3d(mask), reps)
    res.update(device_s=round(t_dev, 4), entry_ms=entry, kept=int(dev.sum()),
               stats=list(backend.NOTES["skeleton_stats"]))
    host_s = None
    if mask.size <= 256 ** 3 or (host_256_s is not None and host_256_s < HOST_LIMIT_S):
        t0 = time.perf_counter()
        host = backend.host_skeletonize_3d(mask)
        host_s = time.perf_counter() - t0
        assert np.array_equal(dev, host), "%s: the device skeleton differs from the host's" % name
        res.update(host_s=round(host_s, 3), equal=True, host_over_device=round(host_s / t_dev, 1))
    elif host_256_s is not None:
        res["host_s_estimate"] = round(host_256_s * mask.size / 256 ** 3, 1)
        res["note"] = "host not run: estimate = its 256^3 time scaled with the voxel count"
    else:
        res["note"] = "host not run (no 256^3 host time in this call to decide by)"
    print(json.dumps(res), flush=True)
    return host_s


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["flylight140_p7", "tubes140", "tubes256", "tubes512"])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_skeleton.py needs a GPU: a timing without one says nothing")
    host_256_s = None
    for name in args.cases:
        mask = flylight140() if name == "flylight140_p7" else tubes(int(name.replace("tubes", "")))
        host_s = run_case(name, mask, args.reps, host_256_s)
        if name == "tubes256":
            host_256_s = host_s
    return 0


if __name__ == "__main__":
    sys.exit(main())
