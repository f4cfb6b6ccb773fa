#!/usr/bin/env python3
"""Times the three whole-volume post-steps of the label driver -- clean_mask (ignore_small_comps),
remove_small_components + relabel (remove_small_comps), dilate_instances -- from the device
(csrc/ppp_postprocess.hip) against the host functions on the same map, asserts that both give the
same arrays, and prints one JSON line per case.

Cases:
  flylight140_p7   the instance map and foreground of bench.py's default workload (140^3, shipped
                   flags), host dilation included
  voronoi256 / voronoi512
                   N^3 maps of about 10 000 touching instances (nearest seed of a jittered 22^3 grid,
                   one cell in 9 dropped to background, speckles added to the foreground).  The host
                   dilation is NOT run above 140^3: one instance of its loop is timed and
                   `host_dilate_s_estimate` = per-instance seconds x instances -- an estimate; the
                   device map is compared with the host loop on a 140^3 crop.

`device_s` is the wall time of the postprocess.*_device call on NumPy arrays (what a driver pays:
upload, kernels, download); `kernels_ms` the time between HIP events around the entry point.

    python tools/time_postprocess.py [--cases flylight140_p7 voronoi256 voronoi512] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IGNORE_SMALL_COMPS = 200        # the shipped flylight configuration
REMOVE_SMALL_COMPS = 600
HOST_DILATE_MAX = 140 ** 3


def flylight140():
    import torch
    import bench
    from patchperpix_amd import backend, flags
    from patchperpix_amd.vote_instances import vote_instances as vi
    shape, ps, cell = bench.WORKLOADS["flylight140_p7"]
    kw = dict(flags.FLYLIGHT, _instances_dtype=np.uint32)
    P = backend.make_params(shape, ps, **kw)
    labels = bench.device_labels(torch, shape, cell, seed=0)
    pred = backend.synth_pred(labels, P, seed=0, f16=True)
    fg = (labels != 0).cpu().numpy()
    inst, _ = vi.to_instance_seg(pred, fg.copy(), fg.copy(), fg.astype(np.uint8), ps, **kw)
    return inst.astype(np.uint32), fg


def voronoi(n, grid=22, seed=0):
    """(uint32 map, bool foreground) made on the device, slab by slab"""
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    cell = n / grid
    pts = (torch.stack(torch.meshgrid(*[torch.arange(grid, device="cuda")] * 3, indexing="ij"), -1).float()
           + torch.rand((grid, grid, grid, 3), generator=gen, device="cuda")) * cell
    ids = (torch.arange(grid ** 3, device="cuda", dtype=torch.int64) + 1).reshape(grid, grid, grid)
    ids[(ids % 9) == 0] = 0
    out = torch.empty((n, n, n), dtype=torch.int32, device="cuda")
    ax = torch.arange(n, device="cuda")
    cy, cx = [(ax.float() / cell).long().clamp_(0, grid - 1)] * 2
    for z0 in range(0, n, 16):
        z = ax[z0:z0 + 16]
        cz = (z.float() / cell).long().clamp_(0, grid - 1)
        pos = torch.stack(torch.meshgrid(z.float(), ax.float(), ax.float(), indexing="ij"), -1)
        best = torch.full(pos.shape[:3], float("inf"), device="cuda")
        lab = torch.zeros(pos.shape[:3], dtype=torch.int64, device="cuda")
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    iz = (cz + dz).clamp_(0, grid - 1)[:, None, None]
                    iy = (cy + dy).clamp_(0, grid - 1)[None, :, None]
                    ix = (cx + dx).clamp_(0, grid - 1)[None, None, :]
                    d = ((pts[iz, iy, ix] - pos) ** 2).sum(-1)
                    closer = d < best
                    best = torch.where(closer, d, best)
                    lab = torch.where(closer, ids[iz, iy, ix].expand_as(lab), lab)
        out[z0:z0 + 16] = lab.to(torch.int32)
    inst = out.cpu().numpy().view(np.uint32)
    fg = inst != 0
    fg |= (torch.rand((n, n, n), generator=gen, device="cuda") < 0.002).cpu().numpy()
    return inst, fg


def best_of(fn, reps):
    import torch
    from patchperpix_amd import backend
    fn()                                    # warm-up: library load, allocator, first launches
    best, kernels, out = None, None, None
    for _ in range(reps):
        backend.EVENTS = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if best is None or dt < best:
            best, kernels = dt, round(sum(sum(v) for v in backend.event_times_ms().values()), 3)
        backend.EVENTS = None
    return out, best, kernels


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def run_case(name, inst, fg, reps):
    from scipy import ndimage
    from patchperpix_amd import backend, postprocess
    from patchperpix_amd.vote_instances import stitch_patch_graph as spg
    n_inst = len(np.unique(inst)) - 1
    res = {"case": name, "shape": list(inst.shape), "instances": int(n_inst)}
    ones = np.ones([3] * 3)

    # clean_mask
    (dev, found, kept), t_dev, k_dev = best_of(lambda: postprocess.clean_mask_device(fg, ones, IGNORE_SMALL_COMPS), reps)
    os.environ["PPP_POSTPROCESS"] = "host"
    host, t_host = once(lambda: spg.clean_mask(fg, ones, IGNORE_SMALL_COMPS))
    del os.environ["PPP_POSTPROCESS"]
    assert np.array_equal(dev, host), "clean_mask differs"
    res["clean_mask"] = {"device_s": round(t_dev, 4), "kernels_ms": k_dev, "host_s": round(t_host, 4),
                         "components": found, "removed": found - kept}

    # remove_small_components + relabel
    dev, t_dev, k_dev = best_of(lambda: postprocess._compact_device(inst, REMOVE_SMALL_COMPS, True, None), reps)
    host, t_host = once(lambda: postprocess.relabel(postprocess.remove_small_components(inst, REMOVE_SMALL_COMPS)))
    assert dev.dtype == host.dtype and np.array_equal(dev, host), "compaction differs"
    res["compact"] = {"device_s": round(t_dev, 4), "kernels_ms": k_dev, "host_s": round(t_host, 4),
                      "kept": int(dev.max())}

    # dilate_instances
    dev, t_dev, k_dev = best_of(lambda: postprocess.dilate_instances_device(inst), reps)
    res["dilate"] = {"device_s": round(t_dev, 4), "kernels_ms": k_dev, "rounds": backend.NOTES.get("post_dilate_rounds")}
    if inst.size <= HOST_DILATE_MAX:
        host, t_host = once(lambda: postprocess.dilate_instances(inst))
        assert np.array_equal(dev, host), "dilation differs"
        res["dilate"]["host_s"] = round(t_host, 3)
    else:
        lbl = int(inst[inst != 0][0])
        out = inst.copy()

        def one_instance():
            out[ndimage.binary_dilation(out == lbl, iterations=1)] = lbl
        _, t_one = once(one_instance)
        res["dilate"]["host_s_per_instance"] = round(t_one, 3)
        res["dilate"]["host_dilate_s_estimate"] = round(t_one * n_inst, 1)
        # the host loop on a 140^3 crop checks the full-size map: a voxel decided in round r depends on
        # ids within r voxels, so the crop's result holds `rounds` + 1 voxels inside its faces
        side, margin = 140, res["dilate"]["rounds"] + 1
        a = [(s_ - side) // 2 for s_ in inst.shape]
        crop = tuple(slice(a_, a_ + side) for a_ in a)
        inner = tuple(slice(margin, side - margin) for _ in a)
        host, t_host = once(lambda: postprocess.dilate_instances(inst[crop]))
        assert np.array_equal(dev[crop][inner], host[inner]), "dilation differs"
        res["dilate"]["host_s_crop140"] = round(t_host, 3)
    print(json.dumps(res), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["flylight140_p7", "voronoi256", "voronoi512"])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args(argv)
    for name in args.cases:
        inst, fg = flylight140() if name == "flylight140_p7" else voronoi(int(name.replace("voronoi", "")))
        run_case(name, inst, fg, args.reps)
    return 0


if __name__ == "__main__":
    sys.exit(main())
