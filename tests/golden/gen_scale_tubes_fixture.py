#!/usr/bin/env python3
"""Sparse-foreground fixtures of the ORACLE: thin tubes, a few percent foreground (the flylight
neurons the shipped configuration segments; the other scale_* fixtures are dense cells).

  python tests/golden/gen_scale_tubes_fixture.py [name ...]

Runs oracle/ppp_oracle.to_instance_seg with the SHIPPED flylight flags on
synth.make_case(kind="tubes") at the shapes below and writes tests/golden/scale_tubes_<name>.npz: the
instance map, the seed and the generator's parameters.  tests/test_s1_sparse_gpu.py regenerates the
input from the seed (checked by CRC) and compares the HIP path id for id, with S1 over item lists
and with the dense launch.  About a minute per case on 8 cores.
"""
import json
import os
import sys
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

CASES = {
    # (shape, patchshape, n_tubes, radius, seed)
    "t96_p9": ((96, 96, 96), (9, 9, 9), 14, 2.5, 0),
    "t70x140_p7": ((70, 140, 140), (7, 7, 7), 15, 2.5, 0),
}


def main(names):
    from oracle import ppp_oracle as orc
    from patchperpix_amd import synth
    from patchperpix_amd.flags import FLYLIGHT
    for name in names:
        shape, ps, n_tubes, radius, seed = CASES[name]
        kw = dict(FLYLIGHT)
        case = synth.make_case(shape, list(ps), seed=seed, kind="tubes", n_tubes=n_tubes, radius=radius)
        fg = case["foreground"]
        t0 = time.perf_counter()
        out = orc.to_instance_seg(case["pred"], fg.copy(), fg.copy(), case["numinst"], list(ps), **kw)
        dt = time.perf_counter() - t0
        inst = out["instances"]
        np.savez_compressed(
            os.path.join(HERE, "scale_tubes_%s.npz" % name),
            shape=np.array(shape), patchshape=np.array(ps), seed=np.array(seed),
            synth_kwargs=json.dumps(dict(kind="tubes", n_tubes=n_tubes, radius=radius, seed=seed)),
            flags=json.dumps({k: v for k, v in kw.items() if isinstance(v, (bool, int, float, str))}),
            pred_f16_crc32=np.array(zlib.crc32(np.ascontiguousarray(case["pred"].astype(np.float16)).tobytes())),
            instances=inst, n_instances=np.array(len(np.unique(inst)) - 1), oracle_seconds=np.array(dt))
        print(name, "%.0f s" % dt, "instances", len(np.unique(inst)) - 1, "of", n_tubes, "tubes; foreground",
              round(float(fg.mean()), 4), inst.dtype)


if __name__ == "__main__":
    main(sys.argv[1:] or list(CASES))
