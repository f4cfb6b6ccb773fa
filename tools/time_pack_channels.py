#!/usr/bin/env python3
"""Times `no_overlap_per_channel` (graph_to_labeling.paint_channels): the device pass + host walk + paint
by channel against the loop over components (PPP_PACK_CHANNELS=loop) in the same process, on the same
nodes and labels, asserts that both give the same map, and prints one JSON line per case.

Cases:
  flylight140_p7   the labelling of bench.py's default workload (140^3 / 7^3, shipped flags)
  bars140          the crossing bars of tests/pack_channels_cases.py as a lattice in 140^3 / 5^3: 63 bars of
                   more than 2000 voxels whose patches overlap where they cross
  tiled140         flylight140_p7 through the tiled assembly (2 slabs x 2 x 2 tiles): the share of the
                   sizes-and-pairs pass (s6_pack_scan) in s6_label_paint

The nodes and labels are taken from one run of the stage path (the call of paint_channels is recorded).
`*_s` is the wall time of paint_channels from NumPy nodes / labels to the NumPy map (upload, kernels,
read-backs, host walk, download), best of --reps after a warm-up; `*_entry_ms` the time between HIP
events around the library's entry points in that run.

    python tools/time_pack_channels.py [--cases flylight140_p7 bars140 tiled140] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def flylight140():
    import torch
    import bench
    from patchperpix_amd import backend, flags
    shape, ps, cell = bench.WORKLOADS["flylight140_p7"]
    kw = dict(flags.FLYLIGHT, no_overlap_per_channel=True)
    P = backend.make_params(shape, ps, **kw)
    labels = bench.device_labels(torch, shape, cell, seed=0)
    pred = backend.synth_pred(labels, P, seed=0, f16=True)
    fg = (labels != 0).cpu().numpy()
    return pred, fg, fg.astype(np.uint8), ps, kw


def bars140():
    import torch
    import pack_channels_cases as pc
    from patchperpix_amd import flags
    n, ps = 140, (5, 5, 5)
    boxes = []
    for b in range(0, n - 19, 20):             # a layer: bars along x, and bars along y two voxels into them
        boxes += [(b + 3, b + 11, y + 4, y + 14, 0, n) for y in range(0, n - 27, 28)]
        boxes += [(b + 9, b + 17, 0, n, x + 8, x + 19) for x in range(0, n - 34, 35)]
    case = pc.bars_case(ps, (n, n, n), boxes)
    kw = dict(flags.FLYLIGHT, no_overlap_per_channel=True)
    return torch.from_numpy(case["pred"].astype(np.float16)).cuda(), case["foreground"], case["numinst"], ps, kw


def recorded_labelling(pred, fg, numinst, ps, kw):
    """the arguments of the stage path's paint_channels call, and the map it returned"""
    from patchperpix_amd.vote_instances import graph_to_labeling as g2l
    from patchperpix_amd.vote_instances import vote_instances as vi
    seen = {}
    plain = g2l.paint_channels

    def recorder(pred_affs, nodes_dev, labels_dev, n_comp, shape, P, **flags):
        seen.update(pred=pred_affs, nodes=nodes_dev.cpu().numpy(), labels=labels_dev.cpu().numpy(), n_comp=n_comp,
                    shape=shape, P=P)
        return plain(pred_affs, nodes_dev, labels_dev, n_comp, shape, P, **flags)
    g2l.paint_channels = recorder
    try:
        inst, _ = vi.to_instance_seg(pred, fg.copy(), fg.copy(), numinst.copy(), list(ps), **dict(kw, _n_slabs=1))
    finally:
        g2l.paint_channels = plain
    return seen, inst


def best_of(fn, reps):
    import torch
    from patchperpix_amd import backend
    fn()                                    # warm-up: allocator, first launches
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


def run_case(name, make, reps):
    import torch
    from patchperpix_amd.vote_instances import graph_to_labeling as g2l
    pred, fg, numinst, ps, kw = make()
    a, inst = recorded_labelling(pred, fg, numinst, ps, kw)

    def paint():
        nodes_dev, labels_dev = torch.from_numpy(a["nodes"]).cuda(), torch.from_numpy(a["labels"]).cuda()
        return g2l.paint_channels(a["pred"], nodes_dev, labels_dev, a["n_comp"], a["shape"], a["P"]).cpu().numpy()
    os.environ.pop("PPP_PACK_CHANNELS", None)
    new, t_new, e_new = best_of(paint, reps)
    os.environ["PPP_PACK_CHANNELS"] = "loop"
    try:
        loop, t_loop, e_loop = best_of(paint, reps)
    finally:
        os.environ.pop("PPP_PACK_CHANNELS", None)
    assert new.shape == loop.shape and np.array_equal(new, loop), "%s: the pass differs from the loop" % name
    assert np.array_equal(new.astype(inst.dtype), inst)
    print(json.dumps({"case": name, "shape": list(a["shape"]), "patchshape": list(ps), "nodes": int(len(a["nodes"])),
                      "instances": int(a["n_comp"]), "channels": int(new.shape[0]), "equal": True,
                      "pass_s": round(t_new, 4), "pass_entry_ms": e_new, "loop_s": round(t_loop, 4),
                      "loop_entry_ms": e_loop, "loop_over_pass": round(t_loop / t_new, 1)}), flush=True)


def run_tiled(reps):
    import torch
    from patchperpix_amd import backend
    from patchperpix_amd.vote_instances import vote_instances as vi
    pred, fg, numinst, ps, kw = flylight140()
    want, _ = vi.to_instance_seg(pred, fg.copy(), fg.copy(), numinst.copy(), list(ps), **dict(kw, _n_slabs=1))
    best = None
    for _ in range(reps + 1):               # (the first run is the warm-up)
        backend.HOST_TIMES = {}
        torch.cuda.synchronize()
        got, _ = vi.to_instance_seg(pred, fg.copy(), fg.copy(), numinst.copy(), list(ps),
                                    **dict(kw, _n_slabs=2, _yx_tiles=(2, 2)))
        t = {k: sum(v) for k, v in backend.HOST_TIMES.items()}
        backend.HOST_TIMES = None
        if best is None or t["s6_label_paint"] < best["s6_label_paint"]:
            best = t
    assert got.shape == want.shape and np.array_equal(got, want), "tiled140: the tiled map differs from the stage path's"
    print(json.dumps({"case": "tiled140", "tiles": [2, 2, 2], "channels": int(got.shape[0]), "equal": True,
                      "s6_label_paint_s": round(best["s6_label_paint"], 4), "s6_pack_scan_s": round(best["s6_pack_scan"], 4),
                      "pack_scan_share": round(best["s6_pack_scan"] / best["s6_label_paint"], 3)}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["flylight140_p7", "bars140", "tiled140"])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_pack_channels.py needs a GPU: a timing without one says nothing")
    for name in args.cases:
        if name == "tiled140":
            run_tiled(args.reps)
        else:
            run_case(name, {"flylight140_p7": flylight140, "bars140": bars140}[name], args.reps)
    return 0


if __name__ == "__main__":
    sys.exit(main())
