#!/usr/bin/env python3
"""ppp+dec on a volume whose dense prediction is NOT kept: decode.DecodeProvider (every tile's halo
decoded again) against decode.decode_rows + compact.CompactPrediction (every foreground voxel decoded
once into rows, the tiles expanded from them), on the same code, foreground and decoder, through the
same tiled assembly -- tiles forced to 2 x 2 x 2 -- with the instance maps asserted equal.

Default: 256^3 at 7^3, foreground = synth.tube_labels (a few percent), a random decoder of the
shipped shape with its logits spread and centred (as tests/test_decode.py does).  One JSON line:
wall time of each way (decode + vote), `voxels_decoded` of each, rows bytes against dense float16
bytes.  The acceptance is the counter and the equality; the time is recorded, not gated.

    python tools/time_compact_decode.py [--side 256] [--tubes 100] [--batch 4096]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AE_SHIPPED = dict(activation="relu", num_fmaps=[64, 128], downsample_factors=[[2, 2, 2], [2, 2, 2]],
                  upsampling="resize_conv", kernel_size=3, num_repetitions=2, padding="same",
                  code_fmaps=22, code_units=176, input_shape_squeezed=(7, 7, 7))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--tubes", type=int, default=100)
    ap.add_argument("--batch", type=int, default=4096)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_compact_decode.py needs a GPU: a timing without one says nothing")
    from patchperpix_amd import decode as dec, flags, synth, tiling
    n = args.side
    shape, ps = (n, n, n), [7, 7, 7]
    fg = synth.tube_labels(shape, n_tubes=args.tubes, radius=2.5, seed=0) != 0
    torch.manual_seed(0)
    d = dec.PatchDecoder(dict(AE_SHIPPED)).cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(0)
    code = torch.randn((176,) + shape, generator=g, device="cuda", dtype=torch.float16)
    # random weights: spread and centre the logits so that both classes occur (probe on a corner)
    k = min(n, 64)
    probe = dec.decode_rows(d, code[:, :k, :k, :k].contiguous(), fg[:k, :k, :k], batch_size=args.batch).rows
    with torch.no_grad():
        scale = 8.0 / float(probe.std())
        d.up_conv[-1][-1].weight.mul_(scale)
        d.up_conv[-1][-1].bias.mul_(scale).sub_(float(probe.median()) * scale)
    del probe
    kw = dict(flags.FLYLIGHT, overlapping_inst=False)
    numinst = fg.astype(np.uint8)
    slabs = tiling.plan_slabs(n, 2)

    def vote(provider):
        inst, _ = tiling.assemble(provider, 0, shape, fg.copy(), fg.copy(), numinst, ps, slabs, _yx_tiles=(2, 2),
                                  _instances_dtype=np.uint32, **kw)
        return inst

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prov = dec.DecodeProvider(d, code, fg, batch_size=args.batch, expit=True)
    a = vote(prov)
    torch.cuda.synchronize()
    t_prov = time.perf_counter() - t0
    t0 = time.perf_counter()
    cp = dec.decode_rows(d, code, fg, batch_size=args.batch, out_dtype=torch.float16, expit=True)
    torch.cuda.synchronize()
    t_dec = time.perf_counter() - t0
    b = vote(cp)
    torch.cuda.synchronize()
    t_rows = time.perf_counter() - t0
    assert np.array_equal(a, b), "the instance maps differ"
    assert cp.voxels_decoded == int(fg.sum())
    print(json.dumps({"shape": list(shape), "patchshape": ps, "tiles": [2, 2, 2], "foreground": round(float(fg.mean()), 4),
                      "instances": int(len(np.unique(a)) - 1), "equal": True,
                      "provider_s": round(t_prov, 2), "provider_voxels_decoded": int(prov.voxels_decoded),
                      "rows_s": round(t_rows, 2), "rows_decode_s": round(t_dec, 2),
                      "rows_voxels_decoded": int(cp.voxels_decoded),
                      "decoded_ratio": round(prov.voxels_decoded / max(1, cp.voxels_decoded), 2),
                      "rows_gb": round(cp.nbytes / 1e9, 3), "dense_f16_gb": round(2e-9 * cp.C * float(np.prod(shape)), 3)}),
          flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
