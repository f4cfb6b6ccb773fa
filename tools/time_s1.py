"""Time the scoring kernel S1 alone (kernel experiments; not the benchmark).

    python tools/time_s1.py [--case 140p7|slab9|...] [--reps N] [--dtype f16|bf16|f16,bf16]

Cases: 140p7 = the whole 140^3 / 7^3 benchmark volume; slab9 = 16 slices of base voxels of a
(48, 512, 512) / 9^3 volume (the slab shape of the north-star pass); slab7 likewise at 7^3.
PPP_LIB / PPP_S1_* select library and kernel variants.  Prints one JSON line.
--dtype: the element type of the prediction; bf16 = the float16 case rounded once to bfloat16 (other
values than the float16 run votes on: a timing, not a comparison of results).  Several types, comma
separated, are timed INTERLEAVED in one process (repeat r of every type before repeat r + 1), the
line then carries ms / min_ms / checksum per type."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    "140p7": ((140, 140, 140), (7, 7, 7), None, (20, 20, 20)),
    "slab9": ((48, 512, 512), (9, 9, 9), (16, 0, 0, 32, 512, 512), (24, 24, 24)),
    "slab7": ((44, 512, 512), (7, 7, 7), (14, 0, 0, 30, 512, 512), (20, 20, 20)),
    "96p5": ((96, 96, 96), (5, 5, 5), None, (12, 12, 12)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="140p7")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtype", default="f16")
    args = ap.parse_args()
    import torch
    import bench
    from patchperpix_amd import backend, flags
    shape, ps, box, cell = CASES[args.case]
    kw = dict(flags.FLYLIGHT)
    P = backend.make_params(shape, ps, **kw)
    labels = bench.device_labels(torch, shape, cell, seed=0)
    pred = backend.synth_pred(labels, P, seed=0, f16=True)
    ov = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    Pb = backend.make_params(shape, ps, cons_box=box, **kw)
    dtypes = args.dtype.split(",")
    preds = {}
    for d in dtypes:
        if d not in ("f16", "bf16"):
            raise SystemExit("--dtype: f16, bf16 or both, comma separated")
        preds[d] = pred if d == "f16" else pred.to(torch.bfloat16)
    times = {d: [] for d in dtypes}
    crc, kernel = {}, {}
    for r in range(args.reps + 1):
        for d in dtypes:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(torch.cuda.current_stream())
            cons = backend.consensus(preds[d], ov, Pb)
            b.record(torch.cuda.current_stream())
            torch.cuda.synchronize()
            if r:
                times[d].append(a.elapsed_time(b))
            else:
                crc[d] = int(cons.view(torch.int32).sum(dtype=torch.int64).item()) & 0xFFFFFFFF
                kernel[d] = backend.NOTES.get("s1_kernel")
            del cons
    out = {"case": args.case, "lib": os.path.basename(backend.library_path()),
           "env": {k: v for k, v in os.environ.items() if k.startswith("PPP_S1")}}
    if len(dtypes) == 1:
        t = times[dtypes[0]]
        out.update(ms=[round(v, 2) for v in t], min_ms=round(min(t), 2), checksum=crc[dtypes[0]])
        if dtypes[0] != "f16":
            out["dtype"] = dtypes[0]
    else:
        for d in dtypes:
            out[d] = {"ms": [round(v, 2) for v in times[d]], "min_ms": round(min(times[d]), 2),
                      "spread_ms": round(max(times[d]) - min(times[d]), 2), "checksum": crc[d], "kernel": kernel[d]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
