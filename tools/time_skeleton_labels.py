#!/usr/bin/env python3
"""Times the 3-d skeleton of EVERY instance of an id map from the device -- one pass, whatever the number of
instances (csrc/ppp_skeleton.hip with labels, backend.skeletonize_labels) -- against the host loop that
defines it (postprocess.skeletonize_instances: one ppp_host_skeletonize_3d per instance), asserts that both
give the same map, and prints one JSON line per case.

Cases (N = the edge of the cube; the defaults are tubes140 and cells140):
  tubesN     synth.tube_labels((N, N, N), radius=2.5) with 30 tubes at 140^3, the count scaled with N^2 like
             tools/time_skeleton.py: thin instances, a few percent foreground (neurons; the flylight regime)
  cellsN     synth.cell_labels((N, N, N), cell=18): at 140^3 the instances of bench.py's flylight140_p7
             workload -- about 500 touching blobs, > 90 % foreground, seams everywhere

`device_s` is the wall time of backend.skeletonize_labels on a NumPy uint32 map (what the `postprocess` task
pays: upload, kernels, counter read-backs, download), best of --reps after a warm-up; `entry_ms` the time
between HIP events around the entry point in that run; `stats` = passes, sub-iterations, rounds.
`host_bbox_s` is one run of the host function as the task calls it (every instance thinned inside its
bounding box).  `host_loop_s_estimate` is the loop the reference's driver has -- one WHOLE-VOLUME thinning per
instance: --host-instances of them are timed (evenly spread over the ids) and the mean is scaled by the
instance count: an ESTIMATE, labelled as one.

    python tools/time_skeleton_labels.py [--cases tubes140 cells140 cells256 ...] [--reps 3] [--host-instances 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.time_skeleton import best_of  # noqa: E402


def make(name):
    from patchperpix_amd import synth
    kind, n = name.rstrip("0123456789"), name[len(name.rstrip("0123456789")):]
    if kind not in ("tubes", "cells") or not n:
        raise SystemExit("unknown case %r (tubesN or cellsN)" % name)
    n = int(n)
    if kind == "tubes":
        n_tubes = max(1, int(round(30 * (n / 140.0) ** 2)))
        return synth.tube_labels((n, n, n), n_tubes=n_tubes, radius=2.5, seed=0).astype(np.uint32)
    return synth.cell_labels((n, n, n), cell=18).astype(np.uint32)


def run_case(name, ids, reps, host_instances):
    from patchperpix_amd import backend, postprocess
    labels = np.unique(ids)
    labels = labels[labels != 0]
    res = {"case": name, "shape": list(ids.shape), "instances": int(len(labels)),
           "foreground_frac": round(float((ids != 0).mean()), 4)}
    dev, t_dev, entry = best_of(lambda: backend.skeletonize_labels(ids), reps)
    res.update(device_s=round(t_dev, 4), entry_ms=entry, kept=int(np.count_nonzero(dev)),
               stats=list(backend.NOTES["skeleton_stats"]))
    t0 = time.perf_counter()
    host = postprocess.skeletonize_instances(ids)
    t_host = time.perf_counter() - t0
    assert np.array_equal(dev, host), "%s: the device pass differs from the host loop" % name
    res.update(host_bbox_s=round(t_host, 3), equal=True, host_bbox_over_device=round(t_host / t_dev, 1))
    picked = labels[np.linspace(0, len(labels) - 1, min(host_instances, len(labels))).astype(int)]
    t0 = time.perf_counter()
    for lbl in picked:
        whole = backend.host_skeletonize_3d(ids == lbl)
        assert np.array_equal(whole, dev == lbl), "%s: instance %d differs" % (name, lbl)
    per = (time.perf_counter() - t0) / len(picked)
    res.update(host_loop_instances_timed=int(len(picked)), host_loop_s_per_instance=round(per, 3),
               host_loop_s_estimate=round(per * len(labels), 1),
               host_loop_estimate_over_device=round(per * len(labels) / t_dev, 1),
               note="host_loop_s_estimate = mean of the timed whole-volume thinnings x instances: an estimate")
    print(json.dumps(res), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["tubes140", "cells140"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-instances", type=int, default=4)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_skeleton_labels.py needs a GPU: a timing without one says nothing")
    for name in args.cases:
        run_case(name, make(name), args.reps, args.host_instances)
    return 0


if __name__ == "__main__":
    sys.exit(main())
