"""Time S1 on sparse foreground: the dense launch against the item lists (ppp_consensus_sparse).

    python tools/time_s1_sparse.py [--case t140p7|tile9|sweep|all] [--reps N] [--out FILE.json]

Cases: t140p7 = tubes in the 140^3 / 7^3 benchmark volume; tile9 = tubes in a 256 x 512 x 512 / 9^3
volume (one tile of the 512^3 plan; S1 over a 16-slice slab of it: the rows of a whole tile do not fit
next to the prediction); sweep = 140^3 / 7^3 with tube counts from 2 to 1500 (about 1 % to 60 % active
items) -- where lists and dense cost the same is the share auto mode switches at.

Per input: the active share (ppp_consensus_last_items), the dense launch and the lists launch (HIP
events around the whole call, warm, median of --reps >= 5 runs, with min / max), and the parts of the
lists launch timed on their own: the pre-pass (auto mode on an input it sends to the dense kernel
costs dense + pre-pass) and the zero stores (the lists with the active ones dropped: a part without
foreground).  Prints one JSON line per input; --out collects them."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, reps):
    ms = []
    for r in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(torch.cuda.current_stream())
        fn()
        b.record(torch.cuda.current_stream())
        torch.cuda.synchronize()
        if r:
            ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def measure(torch, name, shape, ps, n_tubes, box, reps, seed=0):
    from patchperpix_amd import backend, flags, synth
    kw = dict(flags.FLYLIGHT)
    lab = synth.tube_labels(shape, n_tubes=n_tubes, radius=2.5, seed=seed)
    P = backend.make_params(shape, ps, **kw)
    pred = backend.synth_pred(torch.from_numpy(lab.astype(np.int32)).cuda(), P, seed=seed, f16=True)
    ov = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    Pv = backend.make_params(shape, ps, cons_box=box, cons_layout=backend.CONS_VOXEL_MAJOR, **kw)
    Pv = backend.with_pred_clean(pred, Pv)
    L = backend.lib()
    n_el = int(L.ppp_cons_elems(ctypes.byref(Pv)))
    out = backend._big_empty((n_el,), pred.device)
    need = int(L.ppp_consensus_sparse_workspace_bytes(ctypes.byref(Pv), None))
    work = torch.empty((need,), dtype=torch.uint8, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    dt = backend.pred_dtype_code(pred)

    def dense():
        backend.check(L.ppp_consensus_rows(ptr(pred), dt, ptr(ov), ptr(out), ctypes.byref(Pv), backend._stream()))

    def lists(mode=1):
        backend.check(L.ppp_consensus_sparse(ptr(pred), dt, ptr(ov), ptr(out), None, ctypes.byref(Pv), None, 1, ptr(work),
                                             mode, backend._stream()))

    res = {"case": name, "shape": list(shape), "patchshape": list(ps), "n_tubes": n_tubes,
           "foreground": round(float((lab != 0).mean()), 4), "cons_box": list(box) if box else None}
    res["dense"] = timed(torch, dense, reps)
    crc_d = int(out.view(torch.int32).sum(dtype=torch.int64).item())
    res["lists"] = timed(torch, lists, reps)
    assert int(out.view(torch.int32).sum(dtype=torch.int64).item()) == crc_d
    total, active, took = backend.consensus_last_items()
    res.update(items=total, active_items=active, active_share=round(active / total, 4))
    # the parts.  Activity depends on the centre channel alone: with that channel all background no item
    # is active (pre-pass + the zero stores of every item); with it all foreground every item is, and
    # auto mode makes the dense launch -- what it costs over the plain dense call is the pre-pass
    mid = pred.shape[0] // 2
    keep = pred[mid].clone()

    def zeros_only():
        lists(1)

    def auto_dense():
        lists(0)

    dense_full = dense
    pred[mid] = 0.0
    z = timed(torch, zeros_only, reps)
    assert backend.consensus_last_items()[1] == 0
    res["prepass_and_all_zero_stores"] = z
    pred[mid] = 1.0
    ad, dfull = timed(torch, auto_dense, reps), timed(torch, dense_full, reps)
    assert backend.consensus_last_items()[2] == 0
    res["prepass_ms"] = round(ad["median_ms"] - dfull["median_ms"], 3)
    res["zero_stores_ms_for_this_input"] = round((z["median_ms"] - res["prepass_ms"]) * (1.0 - active / total), 3)
    res["speedup"] = round(res["dense"]["median_ms"] / res["lists"]["median_ms"], 3)
    res["ideal_speedup"] = round(total / max(active, 1), 3)
    res["fraction_of_ideal"] = round(res["speedup"] / res["ideal_speedup"], 3)
    res["dense_spread_ms"] = round(res["dense"]["max_ms"] - res["dense"]["min_ms"], 3)
    pred[mid] = keep
    del out, pred, keep, work
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="t140p7", choices=["t140p7", "tile9", "sweep", "all"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5, "median of at least five runs"
    import torch
    rows = []

    def run(*a, **k):
        r = measure(torch, *a, reps=args.reps, **k)
        rows.append(r)
        print(json.dumps(r), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump({"tool": "tools/time_s1_sparse.py", "reps": args.reps, "results": rows}, f, indent=1)

    if args.case in ("t140p7", "all"):
        run("t140p7", (140, 140, 140), (7, 7, 7), 30, None)
    if args.case in ("tile9", "all"):
        run("tile9", (256, 512, 512), (9, 9, 9), 120, (120, 0, 0, 136, 512, 512))
    if args.case in ("sweep", "all"):
        for n in (2, 10, 60, 150, 300, 500, 800, 1500):
            run("sweep140p7_%d" % n, (140, 140, 140), (7, 7, 7), n, None)


if __name__ == "__main__":
    main()
