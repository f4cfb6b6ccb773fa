"""Time the greedy cover with `mark_close_neighboorhood` / `select_patches_overlap_neighborhood`
(reference foreground_cover.py:53-85, 141-168): the device form (ppp_cover_pass_marked, ppp_mask_dilate;
foreground_cover.cover_options_device) against the sequential host loop (PPP_COVER=host), each flag
alone and both together, results asserted equal.

    python tools/time_cover_marks.py [--case 140p7 | 2d_p25 | all] [--repeat N]

Cases: synth.make_case cells at 140^3 / 7^3 and at 696 x 520 / (1, 25, 25).  Prints one JSON line per
case and option: ms of the device form (best of N after a warm-up) and of the host loop (one run), the
number of selected patches and of parallel rounds.  Both times are whole computeForegroundCover calls:
the device side includes packing the patch bits of the ranked list and the copy of the selected list
to the host, the host side the per-chunk transfer of the patch bits."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {
    "140p7": ((140, 140, 140), (7, 7, 7), [18, 18, 18]),
    "2d_p25": ((1, 696, 520), (1, 25, 25), [1, 40, 40]),
}
OPTIONS = {
    "mark": dict(mark_close_neighboorhood=True),
    "ring": dict(select_patches_overlap_neighborhood=True),
    "both": dict(mark_close_neighboorhood=True, select_patches_overlap_neighborhood=True),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", default="all", choices=sorted(CASES) + ["all"])
    ap.add_argument("--repeat", type=int, default=2)
    args = ap.parse_args()
    import torch
    from patchperpix_amd import backend, synth
    from patchperpix_amd.flags import FLYLIGHT_NOTHIN_CC as FLYLIGHT
    from patchperpix_amd.vote_instances import foreground_cover as fc
    from patchperpix_amd.vote_instances.ranked_patches import PatchList

    for name in (sorted(CASES) if args.case == "all" else [args.case]):
        shape, ps, cell = CASES[name]
        case = synth.make_case(shape, ps, seed=11, cell=cell, overlap_frac=0.03, kind="cells")
        P = backend.make_params(shape, ps, **FLYLIGHT)
        pred = torch.from_numpy(case["pred"]).cuda()
        overlap = 1 * (case["numinst"] > 1)
        ov = torch.from_numpy(overlap.astype(np.uint8)).cuda()
        cons = backend.consensus(pred, ov, P)
        score = backend.rank_patches(pred, cons, ov, P)
        del cons
        lin, s = backend.rank_order_device(score, case["foreground"], ps)
        ranked = PatchList(np.stack(np.unravel_index(lin, shape), axis=1).astype(np.int32), s)
        scores = score.cpu().numpy()
        mask = case["foreground"].copy()
        mask[overlap > 0] = 0
        rad = [p // 2 for p in ps]
        radslice = tuple(slice(rad[i], shape[i] - rad[i]) for i in range(3))

        def run(kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sel, _ = fc.computeForegroundCover(overlap.copy(), mask.copy(), ps, ranked, radslice, pred, rad, None,
                                               scores, silent=True, **kw)
            torch.cuda.synchronize()
            return sel, (time.perf_counter() - t0) * 1e3

        for option, flags in OPTIONS.items():
            kw = dict(FLYLIGHT, **flags)
            os.environ["PPP_COVER"] = "device"
            backend.NOTES.pop("cover_rounds", None)
            dev, _ = run(kw)                                    # warm-up
            assert backend.NOTES.get("cover_rounds", 0) > 0, "the device form did not run"
            dev_ms = min(run(kw)[1] for _ in range(max(1, args.repeat)))
            rounds = backend.NOTES["cover_rounds"]
            os.environ["PPP_COVER"] = "host"
            host, host_ms = run(kw)
            assert np.array_equal(dev.coords, host.coords), "device and host loop select different patches"
            assert np.array_equal(dev.scores, host.scores)
            print(json.dumps(dict(case=name, shape=shape, patchshape=ps, option=option, ranked=len(ranked),
                                  selected=len(dev), rounds=rounds, device_ms=round(dev_ms, 2),
                                  host_ms=round(host_ms, 2))), flush=True)
        os.environ.pop("PPP_COVER", None)
        del pred, ov, score


if __name__ == "__main__":
    main()
