"""When does every workgroup of a rank_wg_kernel launch start and end, and on which CU?  Needs the
diagnostic build of the library (PPP_EXTRA_FLAGS=-DPPP_RW_STAMPS, e.g. variants/libppp_rwstamps.so via
PPP_LIB): the kernel writes (start, end, HW_ID, tile) per workgroup into the tile-weight array of its
workspace, the times on the device-wide 100 MHz counter.  Prints a summary: distribution of the
workgroups' durations, of their start times, per XCD and per round, and the CU-milliseconds by the number
of workgroups resident on the CU; round 6, "why does a launch of 1 024 workgroups take 131 ms and one of
2 048 only 196"; round 7, the drain of the default benchmark's launch (--case 140p7).

    PPP_LIB=$PWD/variants/libppp_rwstamps.so python tools/s2_wg_times.py [--case wg1024|wg2048|wg4096|140p7]
    ... --dump raw.npy            keep the raw stamps;   --load raw.npy: analyse them again, no GPU"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = {"wg1024": ((24, 264, 264), (9, 9, 9), (24, 24, 24)), "wg2048": ((40, 264, 264), (9, 9, 9), (24, 24, 24)),
         "wg4096": ((72, 264, 264), (9, 9, 9), (24, 24, 24)),
         # the default benchmark's launch: 140^3 centres at 7^3 (1 458 tiles of 8 x 16 x 16)
         "140p7": ((140, 140, 140), (7, 7, 7), (18, 18, 18)),
         # the launch of the 512^3 step: 32 x 256 x 256 centres (2 048 tiles, none at a border of the rows)
         "ring2048": ((48, 272, 272), (9, 9, 9), (24, 24, 24), (8, 8, 8, 40, 264, 264))}
RW_ORDER_MAX = 16384


def run_launch(args, shape, ps, cell, sbox):
    """two launches of S2 on the case's volume; the stamps of the second and its time"""
    import numpy as np
    import torch
    import bench
    from patchperpix_amd import backend, flags
    kw = dict(flags.FLYLIGHT)
    P = backend.make_params(shape, ps, **kw)
    labels = bench.device_labels(torch, shape, cell, seed=0)
    pred = backend.synth_pred(labels, P, seed=0, f16=True)
    ov = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    vm, Pv = backend.consensus_voxel_major(pred, ov, P)
    L = backend.lib()
    box = ctypes.byref(backend.Box(*sbox)) if sbox else None
    nbytes = int(L.ppp_rank_workspace_bytes(box, ctypes.byref(Pv)))
    out = torch.zeros(shape, dtype=torch.float32, device="cuda")
    res = {"case": args.case, "lib": os.path.basename(backend.library_path())}
    for rep in range(2):
        work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        backend.check(L.ppp_rank_patches_vm(backend._dev_ptr(pred), backend.pred_dtype_code(pred), backend._dev_ptr(vm),
                                            backend._dev_ptr(ov), backend._dev_ptr(out), box, backend._dev_ptr(work),
                                            ctypes.byref(Pv), backend._stream()))
        b.record()
        torch.cuda.synchronize()
        res["launch_ms"] = round(a.elapsed_time(b), 2)
    # where the stamps lie in the workspace: the diagnostic build says (the tile-weight array of its layout)
    L.ppp_rank_wg_stamps_offset.restype = ctypes.c_int64
    off = int(L.ppp_rank_wg_stamps_offset(box, ctypes.byref(Pv)))
    assert off >= 0, "no stamps: the workgroup kernel does not serve this case"
    st = work[off: off + RW_ORDER_MAX * 4].cpu().numpy().view(np.uint32).reshape(-1, 4)
    return st, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="wg2048")
    ap.add_argument("--load", default=None, help="analyse a --dump of an earlier run instead of launching (with --launch-ms)")
    ap.add_argument("--launch-ms", type=float, default=0.0)
    ap.add_argument("--dump", default=None, help="write the raw stamps (block, start, end, HW_ID, tile | XCC << 24) as .npy")
    args = ap.parse_args()
    import numpy as np
    shape, ps, cell = CASES[args.case][:3]
    sbox = CASES[args.case][3] if len(CASES[args.case]) > 3 else None
    sb = sbox or ((0, 0, 0) + tuple(shape))
    sZ, sY, sX = sb[3] - sb[0], sb[4] - sb[1], sb[5] - sb[2]
    if args.load:
        # (a dump of an earlier run: the analysis alone, no GPU)
        st = np.load(args.load)[:, 1:].copy()
        res = {"case": args.case, "lib": "dump", "launch_ms": args.launch_ms}
    else:
        st, res = run_launch(args, shape, ps, cell, sbox)
    res["workgroups_launched"] = int(np.sum(st[:, 1] != 0))
    if args.dump:
        np.save(args.dump, np.concatenate([np.arange(len(st), dtype=np.uint32)[:, None], st], axis=1))
    st = st[(st[:, 1] != 0)]
    if len(st) == 0:
        print(json.dumps(dict(res, error="no stamps: not the -DPPP_RW_STAMPS build")))
        return
    # the stamps are the device-wide 100 MHz counter (wall_clock64), 10 ns a tick, low 32 bits: one zero for
    # the launch, its first start.  (The cycle counter the stamps used before round 7 is a clock per CU: the
    # first workgroups of a launch, which start together, differed by up to 19 ms on it -- the ramp that
    # profiles/r06_h* show at the start of a launch is that, not the dispatcher.)
    raw_s, raw_e = st[:, 0].astype(np.int64), st[:, 1].astype(np.int64)
    raw_e = np.where(raw_e < raw_s, raw_e + (1 << 32), raw_e)
    xcd = ((st[:, 3] >> 24) & 0xF).astype(np.int64)              # XCC_ID of the workgroup's XCD
    cluster = xcd
    halved = ((st[:, 3] >> 23) & 1).astype(bool)                 # the record is half a tile
    st[:, 3] &= 0x7FFFFF
    scale = 1e-5
    start, end = (raw_s - raw_s.min()) * scale, (raw_e - raw_s.min()) * scale
    res["xcd_clusters"] = int(len(np.unique(cluster)))
    res["kernel_span_ms"] = round(float(end.max()), 2)
    res["half_tiles"] = int(halved.sum())
    dur = end - start
    hw = st[:, 2]
    # HW_ID (gfx9): wave 3:0, simd 5:4, pipe 7:6, cu 11:8, sh 12, se 15:13 (, xcc via XCC_ID elsewhere)
    cu = ((hw >> 8) & 0xF) | (((hw >> 12) & 0x1) << 4) | (((hw >> 13) & 0x7) << 5)
    res.update(workgroups=int(len(st)),
               duration_ms={k: round(float(v), 2) for k, v in zip(("min", "p10", "median", "p90", "max"),
                                                                 np.percentile(dur, [0, 10, 50, 90, 100]))},
               start_ms={k: round(float(v), 2) for k, v in zip(("p10", "median", "p90", "max"), np.percentile(start, [10, 50, 90, 100]))},
               first_round=int(np.sum(start < 1.0)),
               workgroups_per_xcd=[int(np.sum(xcd == c)) for c in np.unique(xcd)],
               last_end_per_xcd_ms=[round(float(end[xcd == c].max()), 1) for c in np.unique(xcd)])
    first = start < 1.0
    res["first_round_duration_ms"] = {k: round(float(v), 2) for k, v in zip(("min", "median", "max"), np.percentile(dur[first], [0, 50, 100]))}
    if (~first).any():
        res["later_rounds_duration_ms"] = {k: round(float(v), 2) for k, v in zip(("min", "median", "max"), np.percentile(dur[~first], [0, 50, 100]))}
    # how busy the slots are over time: resident workgroups in 10 slices of the launch
    edges = np.linspace(0, end.max(), 11)
    res["resident_workgroups_over_time"] = [int(np.sum((start < hi) & (end > lo))) for lo, hi in zip(edges[:-1], edges[1:])]
    # CU-milliseconds by the number of workgroups resident on the CU (the kernel is built for four per CU and
    # runs 1.66 x / 1.25 x / 1.125 x slower per workgroup with one fewer than 2 / 3 / 4): a sweep over the
    # start / end events of every CU (XCD, HW_ID's CU)
    cu_ms = {}
    for key in set(zip(cluster.tolist(), cu.tolist())):
        m = (cluster == key[0]) & (cu == key[1])
        ev = sorted([(t, 1) for t in start[m]] + [(t, -1) for t in end[m]])
        n, last = 0, 0.0
        for t, d in ev:
            cu_ms[n] = cu_ms.get(n, 0.0) + (t - last)
            n, last = n + d, t
        cu_ms[0] = cu_ms.get(0, 0.0) + (end.max() - last)
    # when do the workgroups start and end: counts per twentieth of the launch
    e20 = np.linspace(0, end.max(), 21)
    res["starts_per_twentieth"] = np.histogram(start, e20)[0].tolist()
    res["ends_per_twentieth"] = np.histogram(end, e20)[0].tolist()
    res["first_start_per_cu_ms"] = {k: round(float(v), 2) for k, v in zip(("min", "median", "p90", "max"), np.percentile(
        [start[(cluster == c) & (cu == u)].min() for c, u in set(zip(cluster.tolist(), cu.tolist()))], [0, 50, 90, 100]))}
    res["cus_seen"] = len(set(zip(cluster.tolist(), cu.tolist())))
    res["cu_ms_by_resident_workgroups"] = {int(k): round(float(v), 1) for k, v in sorted(cu_ms.items())}
    # per CU id (within its shader engine): spread of the total busy time
    busy = {}
    for c, d in zip(cu.tolist(), dur.tolist()):
        busy[c] = busy.get(c, 0.0) + d
    v = np.array(list(busy.values()))
    res["per_cu_id_busy_ms"] = {"ids": len(busy), "min": round(float(v.min()), 1), "median": round(float(np.median(v)), 1), "max": round(float(v.max()), 1)}
    # duration against the tile's position in z (the tiles of a launch differ in where they sit)
    tiles = st[:, 3].astype(np.int64)
    tz = tiles // (tiles.max() // max(1, -(-sZ // 8)) + 1)
    res["median_duration_by_z_tile"] = {int(k): round(float(np.median(dur[tz == k])), 2) for k in np.unique(tz)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
