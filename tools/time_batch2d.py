#!/usr/bin/env python3
"""Times a stack of 2-d images voted one image per call (the loop) against one batched call
(``to_instance_seg(..., independent_slices=True)``), checks that both give the same instances,
and prints ms per image with the host stage times (backend.host_timer) of either way.

Workloads (bench.py's shapes, synthetic predictions made on the device by ppp_synth_pred):
  worm2d_p25     the 520 x 696 wormbodies image, 16 copies
  dec32x256_p25  32 slices of 256 x 256 (the shape of the decode workload; the prediction is
                 synthesised here, the decoder is not part of what is timed)

    python tools/time_batch2d.py [--workloads worm2d_p25 dec32x256_p25] [--reps 3] [--flags shipped]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (shape of the stack, patch shape, cell size, True: copies of one image, False: distinct slices)
    "worm2d_p25": ((16, 520, 696), (1, 25, 25), (1, 40, 40), True),
    "dec32x256_p25": ((32, 256, 256), (1, 25, 25), (1, 40, 40), False),
}


def make_stack(name):
    import torch
    from patchperpix_amd import backend, synth
    from patchperpix_amd.flags import FLYLIGHT
    shape, ps, cell, copies = WORKLOADS[name]
    lab = synth.cell_labels((1,) + shape[1:] if copies else shape, cell, seed=0)
    if copies:
        lab = np.repeat(lab, shape[0], axis=0)
    labels = torch.from_numpy(lab.astype(np.int32)).cuda()
    P = backend.make_params(shape, ps, **FLYLIGHT)
    pred = backend.synth_pred(labels, P, seed=0, f16=True)
    fg = lab != 0
    return pred, fg, ps


def timed(fn, reps):
    import torch
    from patchperpix_amd import backend
    fn()                                    # warm-up: library load, allocator, first launches
    best, stages = None, None
    for _ in range(reps):
        backend.HOST_TIMES = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if best is None or dt < best:
            best, stages = dt, {k: round(1e3 * sum(v), 2) for k, v in backend.HOST_TIMES.items()}
        backend.HOST_TIMES = None
    return out, best, stages


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--flags", default="shipped", help="patchperpix_amd.flags.FLAG_SETS key")
    args = ap.parse_args(argv)
    from patchperpix_amd.flags import FLAG_SETS
    from patchperpix_amd.vote_instances import vote_instances as vi
    kw = dict(FLAG_SETS[args.flags])
    for name in args.workloads:
        pred, fg, ps = make_stack(name)
        n = fg.shape[0]

        def loop():
            return np.concatenate([vi.to_instance_seg(pred[:, k:k + 1], fg[k:k + 1].copy(), fg[k:k + 1].copy(),
                                                      fg[k:k + 1].astype(np.uint8), ps, **kw)[0] for k in range(n)])

        def batch():
            return vi.to_instance_seg(pred, fg.copy(), fg.copy(), fg.astype(np.uint8), ps, independent_slices=True,
                                      **kw)[0]

        a, t_loop, s_loop = timed(loop, args.reps)
        b, t_batch, s_batch = timed(batch, args.reps)
        print(json.dumps({"workload": name, "images": n, "flags": args.flags, "equal": bool(np.array_equal(a, b)),
                          "ms_per_image_loop": round(1e3 * t_loop / n, 2),
                          "ms_per_image_batch": round(1e3 * t_batch / n, 2),
                          "speedup": round(t_loop / t_batch, 2),
                          "stages_ms_loop": s_loop, "stages_ms_batch": s_batch}), flush=True)
        if not np.array_equal(a, b):
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
