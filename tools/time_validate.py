#!/usr/bin/env python3
"""Wall time of the `validate` sweep on one flylight140_p7 sample, three ways: PPP_VALIDATE_RESIDENT=device (the
sample stays in HBM), host (read once, the crop uploaded per set) and off (the baseline: 8 separate loads, what 8
`label` runs do).

The sample is bench.py's generator at 140^3 / 7^3 written as the prediction step writes it: a float16 zarr array
``volumes/pred_affs`` (Blosc zstd, bit shuffle) with a three-channel ``volumes/pred_numinst``.  The sweep is
``patch_threshold, fc_threshold = [0.5, 0.8]`` zipped, times ``mws = [false, true]``, times ``numinst_threshs =
[[0.9, 0.1], [0.334, 0.334]]``: 8 sets.  The result files of the three runs are compared before any time is
printed.  Per run: wall time and its split into load (container read + decompress + logits test), upload
(host -> device copies of the affinities), assembly, the rest of the vote (bounding box, post-steps, result
file) and scoring.

  python tools/time_validate.py [--work DIR] [--size 140] [--keep]
"""
import argparse
import copy
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("device", "host", "off")


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
    lab = labels.cpu().numpy().astype(np.uint32)
    del labels
    torch.cuda.empty_cache()
    rng = np.random.default_rng(0)
    numinst = (lab != 0).astype(np.uint8)
    numinst[(rng.uniform(size=shape) < 0.03) & (lab != 0)] = 2
    prob = np.zeros((3,) + shape, dtype=np.float16)
    prob[0][numinst == 0] = 0.97
    prob[1][numinst == 1] = 0.95
    prob[1][numinst == 2] = 0.6          # 2 under [0.9, 0.1], 1 under [0.334, 0.334]
    prob[2][numinst == 2] = 0.3
    half = (size + 1) // 2
    zf = minizarr.open(os.path.join(work, "pred", "sample.zarr"), "w")
    zf.create_dataset("volumes/pred_affs", data=pred, chunks=(pred.shape[0], half, half, half))
    zf.create_dataset("volumes/pred_numinst", data=prob, chunks=(3, half, half, half))
    minizarr.open(os.path.join(work, "val.zarr"), "w").create_dataset("sample/gt", data=lab, chunks=shape)
    stored = sum(os.path.getsize(os.path.join(r, f)) for r, _, fs in
                 os.walk(os.path.join(work, "pred", "sample.zarr", "volumes", "pred_affs")) for f in fs)
    print("sample: %s float16 = %.2f GB, %.2f GB on disk, written in %.1f s" % (pred.shape, pred.nbytes / 1e9, stored / 1e9,
                                                                             time.perf_counter() - t0), flush=True)


def make_config(work):
    from patchperpix_amd import run_ppp
    config = run_ppp.load_config([os.path.join(ROOT, "tests", "golden", "label_config_flylight_zarr.toml")])
    config["general"]["overwrite"] = False
    config["model"]["patchshape"] = [7, 7, 7]
    config["vote_instances"].update(only_bb=True, skeletonize_foreground=False)
    config["data"] = dict(val_data=os.path.join(work, "val.zarr"), gt_key="gt", input_format="zarr")
    config["evaluation"] = dict(res_key="vote_instances", metric="confusion_matrix.avFscore", localization_criterion="iou")
    config["validation"] = dict(checkpoints=[1], params_zip=["patch_threshold", "fc_threshold"], patch_threshold=[0.5, 0.8],
                                fc_threshold=[0.5, 0.8], params_product=["mws", "numinst_threshs"], mws=[False, True],
                                numinst_threshs=[[0.9, 0.1], [0.334, 0.334]])
    return config


class Clock:
    """inclusive wall time of wrapped functions, the device drained at both ends"""

    def __init__(self):
        self.t, self.restore = {}, []

    def wrap(self, owner, name, key):
        import torch
        real = getattr(owner, name)

        def timed(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                return real(*a, **k)
            finally:
                torch.cuda.synchronize()
                self.t[key] = self.t.get(key, 0.0) + time.perf_counter() - t0
        setattr(owner, name, timed)
        self.restore.append((owner, name, real))

    def undo(self):
        for owner, name, real in reversed(self.restore):
            setattr(owner, name, real)


def run(mode, work, config):
    from patchperpix_amd import backend, tiling, validate
    from patchperpix_amd.vote_instances import utilVoteInstances as util
    os.environ["PPP_VALIDATE_RESIDENT"] = mode
    out = os.path.join(work, "out_" + mode)
    sessions, base = [], validate.SampleSession

    class Recorded(base):
        def __init__(self, *args):
            base.__init__(self, *args)
            sessions.append(self)
    clock = Clock()
    clock.wrap(util, "loadAffinities", "load")                     # off: the load of every `label`-like call
    clock.wrap(backend, "to_device_pred", "upload")                # every mode: whole array or crop
    clock.wrap(tiling, "to_instance_seg_tiled", "assembly")        # (includes the crop's upload)
    clock.wrap(tiling, "_stitch_vote", "vote")
    clock.wrap(validate, "score_set", "scoring")
    validate.SampleSession = Recorded
    t0 = time.perf_counter()
    try:
        best = validate.validate_checkpoints(copy.deepcopy(config), os.path.join(work, "pred"), out)
    finally:
        validate.SampleSession = base
        clock.undo()
    wall = time.perf_counter() - t0
    t = clock.t
    upload = t.get("upload", 0.0)
    crops = upload - sum(s.times["upload"] for s in sessions)      # the uploads made inside the assembly
    split = {"load": t.get("load", 0.0) + sum(s.times["load"] for s in sessions), "upload": upload,
             "assembly": t.get("assembly", 0.0) - crops,
             "box_post_steps_and_file": t.get("vote", 0.0) - t.get("assembly", 0.0), "scoring": t.get("scoring", 0.0)}
    return out, wall, split, best


def same_files(a, b):
    from patchperpix_amd.vote_instances import io_hdflike
    found = 0
    for root, _, files in os.walk(os.path.join(a, "instanced")):
        for fn in files:
            other = os.path.join(b, os.path.relpath(os.path.join(root, fn), a))
            with io_hdflike.open_container(os.path.join(root, fn), "r") as fa, io_hdflike.open_container(other, "r") as fb:
                assert sorted(fa.keys()) == sorted(fb.keys()), fn
                for k in fa.keys():
                    assert np.array_equal(np.array(fa[k]), np.array(fb[k])), (root, fn, k)
            found += 1
    assert found == 8, found
    assert open(os.path.join(a, "results.json")).read() == open(os.path.join(b, "results.json")).read()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default=None)
    ap.add_argument("--size", type=int, default=140)
    ap.add_argument("--keep", action="store_true")
    args = ap.parse_args()
    work = args.work or tempfile.mkdtemp(prefix="time_validate_")
    os.makedirs(work, exist_ok=True)
    try:
        write_sample(work, args.size)
        config = make_config(work)
        runs = {}
        for mode in reversed(MODES):        # (off first: the one-time costs of a process land in the longest run)
            runs[mode] = run(mode, work, config)
            print("ran %s: %.2f s" % (mode, runs[mode][1]), flush=True)
        for mode in MODES[1:]:
            same_files(runs["device"][0], runs[mode][0])
            assert runs[mode][3] == runs["device"][3]
        print("result files and results.json of the three runs are equal; best: %s" % (runs["device"][3],))
        for mode in MODES:
            _, wall, split, _ = runs[mode]
            print("%-6s wall %7.2f s   %s" % (mode, wall, "  ".join("%s %.2f" % kv for kv in split.items())))
        off, dev = runs["off"], runs["device"]
        once = (off[2]["load"] + off[2]["upload"]) / 8.0
        print("off - device = %.2f s;  7 x (read + decompress + upload) of the off run = %.2f s"
              % (off[1] - dev[1], 7.0 * once))
        print(json.dumps({m: {"wall_s": round(runs[m][1], 3), **{k: round(v, 3) for k, v in runs[m][2].items()}}
                          for m in MODES}))
    finally:
        if not args.keep and args.work is None:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
