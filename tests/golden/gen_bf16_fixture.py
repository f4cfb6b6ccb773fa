#!/usr/bin/env python3
"""Fixtures of the ORACLE for the bfloat16 end-to-end tests whose shapes take the oracle minutes: the
smallest 5^3 shapes of the consensus-cache and the ring tests (tests/test_gpu_parity.py).

  python tests/golden/gen_bf16_fixture.py [name ...]

The input is synth.pred_from_labels rounded to float16 (what ppp_synth_pred writes) and then once to
bfloat16 by torch; the oracle runs on those values widened to float32.  Writes
tests/golden/scale_bf16_<name>.npz: the instance map and the CRC of the input's 16-bit patterns.
tests/test_bf16_gpu.py regenerates the input on the device (checked by the CRC) and compares the tiled
HIP path id for id.  One to two minutes per case on 8 cores.
"""
import os
import sys
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

CASES = {
    # (shape, patchshape, cell, seed): test_consensus_cache_equals_recomputation / test_ring_sweep_equals_plain_tiles
    "cache_p5": ((40, 44, 48), (5, 5, 5), 12, 6),
    "ring_p5": ((50, 44, 48), (5, 5, 5), 12, 7),
}


def main(names):
    import torch
    from oracle import ppp_oracle as orc
    from patchperpix_amd import synth
    from patchperpix_amd.flags import FLYLIGHT_CC
    for name in names:
        shape, ps, cell, seed = CASES[name]
        kw = dict(FLYLIGHT_CC, _instances_dtype=np.uint32)
        lab = synth.cell_labels(shape, [cell] * 3, seed=seed)
        pred16 = synth.pred_from_labels(lab, list(ps), seed=seed).astype(np.float16)
        bf = torch.from_numpy(pred16).to(torch.bfloat16)
        fg = lab != 0
        t0 = time.perf_counter()
        out = orc.to_instance_seg(bf.float().numpy(), fg.copy(), fg.copy(), fg.astype(np.uint8), list(ps), **kw)
        dt = time.perf_counter() - t0
        inst = out["instances"]
        np.savez_compressed(
            os.path.join(HERE, "scale_bf16_%s.npz" % name),
            shape=np.array(shape), patchshape=np.array(ps), cell=np.array(cell), seed=np.array(seed),
            pred_bf16_crc32=np.array(zlib.crc32(bf.view(torch.int16).numpy().tobytes())),
            instances=inst, n_instances=np.array(len(np.unique(inst)) - 1), oracle_seconds=np.array(dt))
        print(name, "%.0f s" % dt, "instances", len(np.unique(inst)) - 1, inst.dtype)


if __name__ == "__main__":
    main(sys.argv[1:] or list(CASES))
