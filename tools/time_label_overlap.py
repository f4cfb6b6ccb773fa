#!/usr/bin/env python3
"""Times `ppp_label_overlap` (csrc/ppp_overlap.hip: the contingency table of two label stacks in one streaming
pass plus a rocPRIM sort / reduce-by-key of the partial counts) against the host definition
`evaluate_instances.overlap_counts_host`, asserts that both give the same rows and counts BEFORE any time is
printed, and prints one JSON line per case and a table at the end.

Cases: tube labels of `synth.tube_labels` (the generator behind synth.make_case(kind="tubes")) at 140^3 and at
512^3, gt = the generator's labels, pred = the VOTED map -- the synthetic prediction of these labels
(backend.synth_pred, float16) through vote_instances.to_instance_seg with the shipped flag set, patches of 7^3 at
140^3 and 5^3 at 512^3; made once per case and not part of any time -- and, at 140^3, the pair (Sg, pred) of the
cldice criterion, Sg the per-instance skeleton of gt.  `dense_140` (cell labels, every voxel foreground, short
runs) shows the pass away from tube-like input.  --pred displaced takes the labels displaced by (1, 2, 1) voxels
with other ids in place of the vote.

`device_ms`: the time between HIP events around the entry point (both synchronisations inside), the median of
--reps calls after --warmup calls, with the spread; `gbps`: (La + Lb) * 4 bytes per voxel divided by that time;
`copy_ms` / `copy_gbps`: a device-to-device copy of the same byte count in the same run; `host_s`: one call of
overlap_counts_host.

    python tools/time_label_overlap.py [--cases tubes_140 tubes_512 skel_140 dense_140] [--reps 7] [--warmup 2]
                                       [--pred voted|displaced]
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

CASES = {                       # volume, tubes (0: cell labels), skeleton of gt as the first stack, patch of the vote
    "tubes_140": ((140, 140, 140), 14, False, (7, 7, 7)),
    "tubes_512": ((512, 512, 512), 180, False, (5, 5, 5)),
    "skel_140": ((140, 140, 140), 14, True, (7, 7, 7)),
    "dense_140": ((140, 140, 140), 0, False, (7, 7, 7)),
}


def voted_map(gt, patch):
    """the instance map vote_instances makes of the synthetic prediction of `gt`"""
    import torch
    from patchperpix_amd import backend
    from patchperpix_amd.flags import FLYLIGHT
    from patchperpix_amd.vote_instances import vote_instances as vi
    kw = dict(FLYLIGHT)
    labels = torch.from_numpy(gt.astype(np.int32)).cuda()
    pred = backend.synth_pred(labels, backend.make_params(gt.shape, patch, **kw), seed=0, f16=True)
    fg = (labels != 0).to(torch.uint8)
    inst, _ = vi.to_instance_seg(pred, fg, fg.clone(), fg, list(patch), **kw)
    del pred
    torch.cuda.empty_cache()
    return np.ascontiguousarray(inst).astype(np.uint32)


def make_pair(shape, n_tubes, skeleton, patch, how):
    from patchperpix_amd import backend, synth
    if n_tubes:
        gt = synth.tube_labels(shape, n_tubes=n_tubes, radius=2.5, seed=0).astype(np.uint32)
    else:
        gt = synth.cell_labels(shape, 9, seed=0).astype(np.uint32)
    if how == "voted":
        pred = voted_map(gt, patch)
    else:
        pred = np.zeros_like(gt)
        pred[1:, 2:, 1:] = np.where(gt != 0, gt + 1000, 0)[:-1, :-2, :-1]
    if skeleton:
        gt = backend.skeletonize_labels(gt)
    return gt[None], pred[None]


def time_case(name, reps, warmup, how):
    import torch
    from patchperpix_amd import backend
    from patchperpix_amd import evaluate_instances as ei
    assert torch.cuda.is_available(), "time_label_overlap.py needs a GPU"
    shape, n_tubes, skeleton, patch = CASES[name]
    t0 = time.perf_counter()
    a, b = make_pair(shape, n_tubes, skeleton, patch, how)
    t_make = time.perf_counter() - t0
    ta = torch.from_numpy(a.view(np.int32)).cuda()
    tb = torch.from_numpy(b.view(np.int32)).cuda()
    times = []
    for k in range(warmup + reps):
        backend.EVENTS = {}
        rows, counts = backend.label_overlap(ta, tb)
        torch.cuda.synchronize()
        ms = sum(sum(v) for v in backend.event_times_ms().values())
        backend.EVENTS = None
        if k >= warmup:
            times.append(ms)
    t0 = time.perf_counter()
    h_rows, h_counts = ei.overlap_counts_host(a, b)
    t_host = time.perf_counter() - t0
    assert np.array_equal(rows, h_rows) and np.array_equal(counts, h_counts), "device and host tables differ"
    nbytes = (ta.numel() + tb.numel()) * 4
    src = torch.cat([ta.reshape(-1), tb.reshape(-1)])
    dst = torch.empty_like(src)
    copies = []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            copies.append(e0.elapsed_time(e1))
    med, cmed = statistics.median(times), statistics.median(copies)
    res = {"case": name, "shape": list(shape), "pred": how, "make_s": round(t_make, 1), "pred_ids": int(len(np.unique(b)) - 1),
           "fg_share": round(float((a != 0).mean()), 4), "rows": int(len(counts)),
           "read_mb": round(nbytes / 1e6, 1), "device_ms": round(med, 3),
           "device_ms_min_max": [round(min(times), 3), round(max(times), 3)], "gbps": round(nbytes / med / 1e6, 1),
           "copy_ms": round(cmed, 3), "copy_gbps": round(nbytes / cmed / 1e6, 1),
           "ratio_to_copy": round(cmed / med, 3), "host_s": round(t_host, 3)}
    print(json.dumps(res), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pred", default="voted", choices=["voted", "displaced"])
    args = ap.parse_args(argv)
    rows = [time_case(c, args.reps, args.warmup, args.pred) for c in args.cases]
    print("\n%-10s %-14s %8s %8s %10s %9s %9s %10s %8s %8s" % ("case", "volume", "fg", "rows", "device ms", "GB/s",
                                                              "copy ms", "copy GB/s", "ratio", "host s"))
    for r in rows:
        print("%-10s %-14s %8.4f %8d %10.3f %9.1f %9.3f %10.1f %8.3f %8.3f" % (
            r["case"], "x".join(map(str, r["shape"])), r["fg_share"], r["rows"], r["device_ms"], r["gbps"], r["copy_ms"],
            r["copy_gbps"], r["ratio_to_copy"], r["host_s"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
