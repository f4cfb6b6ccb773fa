#!/usr/bin/env python3
"""Times `ppp_eval_patch` (csrc/ppp_eval.hip: evaluate_patch as one streaming reduction over the dense
prediction) against the host definition `evaluate_prediction.patch_counts_host`, asserts that both give the same
counts and maps, and prints one JSON line per case and a table at the end.

Cases: the shape of flylight140_p7 -- 343 x 140^3, float16, 3 thresholds, L = 1 and L = 8 label channels, and
for the cost of the label loads the foreground of the L = 8 case in one channel and no foreground at all --
and a 2-d image, 625 x 1 x 696 x 520 (25 x 25 patches).  The prediction is uniform noise made on the device;
the labels are synth.tube_labels volumes (thin tubes, one volume per channel, so channels overlap).

`kernel_ms` / `kernel_maps_ms`: the time between HIP events around the entry point without / with the
inter / union maps, the median of --reps calls after --warmup calls in one process, with the spread (min .. max);
`gbps`: the prediction's bytes divided by that time.  `host_s`: one call of patch_counts_host on the first
--host-z slices of the volume (0: all of them), which is also what the device result is compared on, as a
z-tile of its own; `host_s_volume` scales it to the volume by the slice count.

    python tools/time_eval_patch.py [--cases p7_L1 p7_L8 ...] [--reps 7] [--warmup 2] [--host-z 16]
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

THRESHOLDS = [0.3, 0.5, 0.9]
CASES = {                       # volume, patch, label channels, tube volumes laid into them
    "p7_L1": ((140, 140, 140), (7, 7, 7), 1, 1),
    "p7_L8": ((140, 140, 140), (7, 7, 7), 8, 8),
    "p7_L1_dense": ((140, 140, 140), (7, 7, 7), 1, 8),      # the foreground of p7_L8 in ONE channel: the gather's cost
    "p7_L1_empty": ((140, 140, 140), (7, 7, 7), 1, 0),      # no foreground: no label load at all
    "img2d": ((1, 696, 520), (1, 25, 25), 1, 1),
}


def make_labels(shape, L, volumes):
    """`volumes` tube volumes with ids of their own, volume k laid into channel k % L where that is still empty"""
    from patchperpix_amd import synth
    vol = tuple(max(s, 8) for s in shape)
    out = np.zeros((L,) + shape, dtype=np.int32)
    for k in range(volumes):
        t = synth.tube_labels(vol, n_tubes=14, radius=2.5, seed=k)[:shape[0], :shape[1], :shape[2]]
        t = (t + 1000 * k * (t != 0)).astype(np.int32)
        out[k % L] = np.where(out[k % L] == 0, t, out[k % L])
    return out


def device_times(pred, d_labels, patch, taus, want_maps, reps, warmup):
    import torch
    from patchperpix_amd import backend
    times = []
    for k in range(warmup + reps):
        counts = torch.zeros(1 + 2 * len(taus), dtype=torch.int64, device="cuda")
        backend.EVENTS = {}
        res = backend.eval_patch(pred, d_labels, patch, 0, taus, counts, want_maps)
        torch.cuda.synchronize()
        ms = sum(sum(v) for v in backend.event_times_ms().values())
        backend.EVENTS = None
        if k >= warmup:
            times.append(ms)
    return times, counts, res


def time_case(name, reps, warmup, host_z):
    import torch
    from patchperpix_amd import backend
    from patchperpix_amd import evaluate_prediction as ev
    assert torch.cuda.is_available(), "time_eval_patch.py needs a GPU"
    shape, patch, L, volumes = CASES[name]
    C = patch[0] * patch[1] * patch[2]
    torch.manual_seed(0)
    pred = torch.rand((C,) + shape, device="cuda", dtype=torch.float16)
    labels = make_labels(shape, L, volumes)
    d_labels = torch.from_numpy(labels).cuda()
    taus = ev.rounded_thresholds(THRESHOLDS, np.float16)
    t_plain, counts, _ = device_times(pred, d_labels, patch, taus, False, reps, warmup)
    t_maps, counts_m, (inter, union) = device_times(pred, d_labels, patch, taus, True, reps, warmup)
    assert torch.equal(counts, counts_m), "counts with and without the maps differ"
    # the host definition on the first slices, against the device on the same z-tile
    nz = shape[0] if host_z <= 0 else min(host_z, shape[0])
    tile = pred[:, :nz].contiguous()
    d_counts = torch.zeros_like(counts)
    d_inter, d_union = backend.eval_patch(tile, d_labels, patch, 0, taus, d_counts, True)
    tile_host = tile.cpu().numpy()
    t0 = time.perf_counter()
    h_counts, h_inter, h_union = ev.patch_counts_host(tile_host, labels, patch, THRESHOLDS, want_maps=True)
    t_host = time.perf_counter() - t0
    assert np.array_equal(d_counts.cpu().numpy(), h_counts), "counts differ"
    assert np.array_equal(d_inter.cpu().numpy(), h_inter) and np.array_equal(d_union.cpu().numpy(), h_union), "maps differ"
    assert torch.equal(inter[:, :nz], d_inter) and torch.equal(union[:, :nz], d_union), "the z-tile differs from the volume"
    nbytes = pred.numel() * pred.element_size()
    med, med_m = statistics.median(t_plain), statistics.median(t_maps)
    numinst = (labels > 0).sum(axis=0)
    res = {"case": name, "pred_shape": [C] + list(shape), "dtype": "float16", "L": L, "thresholds": len(taus),
           "pred_gb": round(nbytes / 1e9, 3), "fg_share": round(float((numinst == 1).mean()), 4),
           "overlap_share": round(float((numinst > 1).mean()), 5), "num_gt": int(counts[0]),
           "kernel_ms": round(med, 3), "kernel_ms_min_max": [round(min(t_plain), 3), round(max(t_plain), 3)],
           "kernel_maps_ms": round(med_m, 3), "kernel_maps_ms_min_max": [round(min(t_maps), 3), round(max(t_maps), 3)],
           "gbps": round(nbytes / med / 1e6, 1), "gbps_maps": round(nbytes / med_m / 1e6, 1),
           "host_slices": nz, "host_s": round(t_host, 2), "host_s_volume": round(t_host * shape[0] / nz, 1)}
    print(json.dumps(res), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-z", type=int, default=16)
    args = ap.parse_args(argv)
    rows = [time_case(c, args.reps, args.warmup, args.host_z) for c in args.cases]
    print("\n%-12s %-22s %3s %9s %11s %9s %14s %10s %14s" % ("case", "prediction", "L", "pred GB", "kernel ms", "GB/s",
                                                           "with maps ms", "GB/s", "host s (volume)"))
    for r in rows:
        print("%-12s %-22s %3d %9.3f %11.3f %9.1f %14.3f %10.1f %14.1f" % (
            r["case"], "x".join(map(str, r["pred_shape"])), r["L"], r["pred_gb"], r["kernel_ms"], r["gbps"],
            r["kernel_maps_ms"], r["gbps_maps"], r["host_s_volume"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
