#!/usr/bin/env python3
"""Wall time of loading one flylight140_p7 prediction (343 x 140^3 float16, Blosc zstd with bit shuffle, eight
chunks, written by this project's writer) two ways, alternating in one process:

  (a) the host load: ``arr[...]`` (file read, codec, un-shuffle and scatter copy on 16 host threads), the logits
      test ``min < 0 and max > 1`` and the upload -- with each of those steps also run on its own over the chunks,
      on the same thread pool, which is the split DESIGN.md 7.17 lacks;
  (b) the device load: ``arr.read_device(..., flags=True)`` -- file read and codec on the host threads, host ->
      device copies and ppp_chunk_scatter issued by the caller -- with the codec stage and the copies also run on
      their own;
  (c) the kernel alone on one chunk, next to a device-to-device copy of the same byte count in the same run.

The two loads must give equal bits and equal logits decisions before any time is printed.  Medians and ranges
over --reps rounds.  The lower bound of (b) is the codec on the host threads plus the copies over the bus; the
last lines say how close (b) comes to that sum and whether its range lies below (a)'s.

  python tools/time_load.py [--work DIR] [--size 140] [--reps 3] [--keep]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_sample(work, size):
    import torch
    import bench
    from patchperpix_amd import backend, minizarr
    from patchperpix_amd.flags import FLYLIGHT
    shape, ps, cell = (size,) * 3, (7, 7, 7), (18, 18, 18)
    t0 = time.perf_counter()
    labels = bench.device_labels(torch, shape, cell, seed=0)
    P = backend.make_params(shape, ps, **FLYLIGHT)
    pred = backend.synth_pred(labels, P, seed=0, f16=True).cpu().numpy()
    del labels
    torch.cuda.empty_cache()
    half = (size + 1) // 2
    zf = minizarr.open(os.path.join(work, "sample.zarr"), "w")
    arr = zf.create("volumes/pred_affs", shape=pred.shape, chunks=(pred.shape[0], half, half, half), dtype=np.float16)
    # (the writer encodes chunk by chunk; here eight at a time)
    boxes = [(slice(None),) + tuple(slice(i * half, min(size, (i + 1) * half)) for i in idx) for idx in np.ndindex(2, 2, 2)]

    def put(sel):
        arr[sel] = pred[sel]
    with ThreadPoolExecutor(max_workers=8) as pool:
        list(pool.map(put, boxes))
    stored = sum(os.path.getsize(os.path.join(arr.path, f)) for f in os.listdir(arr.path))
    print("sample: %s float16 = %.2f GB, %.2f GB on disk, written in %.1f s" % (pred.shape, pred.nbytes / 1e9, stored / 1e9,
                                                                             time.perf_counter() - t0), flush=True)
    return pred


def pooled(fn, items):
    """fn over the items on the reader's thread pool; (results, wall seconds)"""
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        out = list(pool.map(fn, items))
    return out, time.perf_counter() - t0


def host_load(arr):
    """what loadAffinities and the upload do today: (tensor, logits decision, seconds)"""
    import torch
    from patchperpix_amd import backend
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a = arr[...]
    logits = bool(np.min(a) < 0 and np.max(a) > 1)
    t = backend.to_device_pred(a)
    torch.cuda.synchronize()
    return t, logits, time.perf_counter() - t0


def host_split(arr):
    """the steps of the host load, each over all chunks on the thread pool, then the test and the upload"""
    import torch
    from patchperpix_amd import minizarr
    idx = list(np.ndindex(*[-(-s // c) for s, c in zip(arr.shape, arr.chunks)]))
    t = {}
    raws, t["file read"] = pooled(arr.read_chunk_bytes, idx)
    shuffled, t["codec"] = pooled(lambda raw: minizarr.blosc_decode(raw, unshuffle=False), raws)
    plain, t["un-shuffle"] = pooled(lambda s: minizarr.unshuffle_blocks(s[0], s[1], s[2], s[3]), shuffled)
    del raws, shuffled
    out = np.empty(arr.shape, dtype=arr.dtype)
    ranges = [(0, s) for s in arr.shape]

    def scatter(k):
        src, dst = minizarr._clip(arr.chunks, [i * c for i, c in zip(idx[k], arr.chunks)], ranges)
        out[dst] = plain[k].view(arr.dtype).reshape(arr.chunks)[src]
    _, t["scatter copy"] = pooled(scatter, range(len(idx)))
    del plain
    t0 = time.perf_counter()
    bool(np.min(out) < 0 and np.max(out) > 1)
    t["min / max"] = time.perf_counter() - t0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev = torch.from_numpy(out).cuda()
    torch.cuda.synchronize()
    t["upload"] = time.perf_counter() - t0
    del dev
    return t


def device_load(arr):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t, (neg, gt1, nan) = arr.read_device((slice(None),) * arr.ndim, device="cuda", flags=True)
    torch.cuda.synchronize()
    return t, (not nan) and neg and gt1, time.perf_counter() - t0


def device_split(arr):
    """the stages of the device load on their own: file read + codec on the thread pool (into pageable buffers),
    the host -> device copies of all chunks from one pinned buffer, and the kernel over all chunks"""
    import torch
    from patchperpix_amd import backend
    idx = list(np.ndindex(*[-(-s // c) for s, c in zip(arr.shape, arr.chunks)]))
    t = {}
    shuffled, t["file read + codec (threads)"] = pooled(lambda i: arr.decode_chunk_shuffled(arr.read_chunk_bytes(i)), idx)
    nbytes = len(shuffled[0][0])
    pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    pinned.numpy()[:] = shuffled[0][0]
    dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.empty(arr.shape, dtype=torch.float16, device="cuda")
    flags = torch.zeros(3, dtype=torch.int32, device="cuda")
    ranges = [(0, s) for s in arr.shape]
    a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    torch.cuda.synchronize()
    a.record()
    for _ in idx:
        dev.copy_(pinned, non_blocking=True)
    b.record()
    for i, s in zip(idx, shuffled):
        backend.chunk_scatter(dev, s[1], s[2], s[3], arr.chunks, [k * ch for k, ch in zip(i, arr.chunks)], ranges, out, flags)
    c.record()
    torch.cuda.synchronize()
    t["host -> device copies"] = a.elapsed_time(b) / 1e3
    t["kernel"] = b.elapsed_time(c) / 1e3
    return t


def kernel_alone(arr, reps=10):
    """(c): ppp_chunk_scatter of one whole chunk with its flags, and a device-to-device copy of as many bytes"""
    import torch
    from patchperpix_amd import backend
    src, ts, bs, kind = arr.decode_chunk_shuffled(arr.read_chunk_bytes((0,) * arr.ndim))
    dev = torch.from_numpy(np.array(src)).cuda()
    out = torch.empty(arr.shape, dtype=torch.float16, device="cuda")
    flags = torch.zeros(3, dtype=torch.int32, device="cuda")
    other = torch.empty_like(dev)
    ranges = [(0, s) for s in arr.shape]
    kern, copy = [], []
    for r in range(reps + 2):
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        a.record()
        backend.chunk_scatter(dev, ts, bs, kind, arr.chunks, [0] * arr.ndim, ranges, out, flags)
        b.record()
        other.copy_(dev)
        c.record()
        torch.cuda.synchronize()
        if r >= 2:
            kern.append(a.elapsed_time(b) / 1e3)
            copy.append(b.elapsed_time(c) / 1e3)
    return len(src), kern, copy


def stat(values):
    return "%.3f s (%.3f .. %.3f)" % (float(np.median(values)), min(values), max(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default=None)
    ap.add_argument("--size", type=int, default=140)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--keep", action="store_true")
    args = ap.parse_args()
    import torch
    from patchperpix_amd import minizarr
    work = args.work or tempfile.mkdtemp(prefix="time_load_")
    os.makedirs(work, exist_ok=True)
    try:
        pred = write_sample(work, args.size)
        arr = minizarr.open(os.path.join(work, "sample.zarr"), "r")["volumes/pred_affs"]
        # equal bits and equal logits decisions, before any time
        th, lh, _ = host_load(arr)
        td, ld, _ = device_load(arr)
        assert th.dtype == td.dtype and th.shape == td.shape and torch.equal(th.view(torch.int16), td.view(torch.int16))
        assert np.array_equal(th.cpu().numpy().view(np.uint16), pred.view(np.uint16)) and lh == ld
        print("host load and device load: equal bits, logits decision %s both" % lh, flush=True)
        del th, td, pred
        host, dev, hsplit, dsplit = [], [], [], []
        for _ in range(args.reps):
            t, _, s = host_load(arr)
            del t
            host.append(s)
            hsplit.append(host_split(arr))
            t, _, s = device_load(arr)
            del t
            dev.append(s)
            dsplit.append(device_split(arr))
            torch.cuda.empty_cache()
        nbytes, kern, copy = kernel_alone(arr)
        print("(a) host load    %s" % stat(host))
        for k in hsplit[0]:
            print("      %-28s %s" % (k, stat([s[k] for s in hsplit])))
        print("(b) device load  %s" % stat(dev))
        for k in dsplit[0]:
            print("      %-28s %s" % (k, stat([s[k] for s in dsplit])))
        ms = lambda v: "%.3f ms (%.3f .. %.3f)" % (1e3 * float(np.median(v)), 1e3 * min(v), 1e3 * max(v))
        print("(c) kernel, one chunk of %.1f MB  %s = %.0f GB/s read + written;  device-to-device copy  %s = %.0f GB/s"
              % (nbytes / 1e6, ms(kern), 2e-9 * nbytes / np.median(kern), ms(copy), 2e-9 * nbytes / np.median(copy)))
        bound = [s["file read + codec (threads)"] + s["host -> device copies"] for s in dsplit]
        print("lower bound of (b), codec on the host threads + copies: %s;  (b) / bound = %.2f" % (stat(bound), np.median(dev) / np.median(bound)))
        print("device load range %s the host load's range: %s" % ("lies below" if max(dev) < min(host) else "does NOT lie below",
                                                                "a win" if max(dev) < min(host) else "not a win"))
        print(json.dumps({"host_load_s": [round(v, 3) for v in host], "device_load_s": [round(v, 3) for v in dev],
                          "host_split_s": {k: round(float(np.median([s[k] for s in hsplit])), 3) for k in hsplit[0]},
                          "device_split_s": {k: round(float(np.median([s[k] for s in dsplit])), 4) for k in dsplit[0]},
                          "kernel_chunk_ms": round(1e3 * float(np.median(kern)), 4), "d2d_copy_chunk_ms": round(1e3 * float(np.median(copy)), 4),
                          "chunk_bytes": nbytes}))
    finally:
        if not args.keep and args.work is None:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
