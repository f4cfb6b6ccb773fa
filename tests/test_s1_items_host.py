"""The item criterion of S1 on sparse foreground (backend.s1_items_host, the NumPy restatement of
csrc/ppp_consensus_sparse.hip) against the oracle: an item the criterion calls inactive has only
zero consensus entries."""
import numpy as np

from tests_flags import FLYLIGHT

SHAPE, PS = (24, 40, 72), [5, 5, 5]


def tube_case():
    from patchperpix_amd import synth
    return synth.make_case(SHAPE, PS, seed=5, kind="tubes", n_tubes=3, radius=2.5, overlap_frac=0.03)


def test_inactive_items_are_all_zero_in_the_oracle():
    from oracle import ppp_oracle as orc
    from patchperpix_amd import backend
    case = tube_case()
    kw = dict(FLYLIGHT, overlapping_inst=True)
    ov = case["numinst"] > 1
    assert ov.any()
    th = np.float32(kw["patch_threshold"])
    mid = case["pred"].shape[0] // 2
    valid = (case["pred"][mid] > th) & ~ov
    active, runs, rows = backend.s1_items_host(valid, PS)
    assert len(runs) == ((SHAPE[1] * SHAPE[2] + 63) // 64) * (SHAPE[0] // 2) and len(rows) == 4 * 9 + 5
    share = float(active.mean())
    print("active share", share, "of", active.size, "items")
    assert share < 0.5                                   # (a condition on the input)
    assert active.any()
    cons = orc.consensus_planes(case["pred"], 1 * ov, PS, **kw)
    planes = orc.positive_planes(cons, PS)               # [L - 1, Z, Y, X], L = (dz * wy + dy) * wx + dx
    wx = 2 * PS[2] - 1
    wy = 2 * PS[1] - 1
    n_zero_items = 0
    for run, lines in enumerate(runs):
        for r, (dz, dy) in enumerate(rows):
            if active[run, r]:
                continue
            for dx in range(-(PS[2] - 1), PS[2]):
                L = (dz * wy + dy) * wx + dx
                if L <= 0:
                    continue
                for (z, y, x0, n) in lines:
                    assert not planes[L - 1, z, y, x0:x0 + n].any(), (run, (dz, dy, dx))
            n_zero_items += 1
    assert n_zero_items == int((~active).sum())
    # and the criterion is not vacuous: the active items hold every nonzero entry, and most of them
    # hold one
    n_hit = 0
    for run, lines in enumerate(runs):
        for r, (dz, dy) in enumerate(rows):
            if not active[run, r]:
                continue
            Ls = [(dz * wy + dy) * wx + dx for dx in range(-(PS[2] - 1), PS[2])]
            n_hit += any(planes[L - 1, z, y, x0:x0 + n].any() for L in Ls if L > 0 for (z, y, x0, n) in lines)
    assert n_hit > 0.5 * int(active.sum())


def test_items_of_a_part_and_of_plain_runs():
    """run numbering of a sub-box: one line per run when its x extent is a multiple of 64 (or < 64)"""
    from patchperpix_amd import backend
    valid = np.zeros((6, 10, 140), dtype=bool)
    valid[2, 4, 70] = True
    active, runs, rows = backend.s1_items_host(valid, [3, 3, 3], part=(1, 2, 4, 6, 9, 132))
    assert len(runs) == 2 * 7 * 3 and len(rows) == 2 * 5 + 3
    # the only valid voxel has no partner: nothing is active
    assert not active.any()
    valid[3, 5, 72] = True                               # partner at d = (1, 1, 2)
    active, runs, rows = backend.s1_items_host(valid, [3, 3, 3], part=(1, 2, 4, 6, 9, 132))
    hit = np.argwhere(active)
    assert len(hit) == 1
    run, r = hit[0]
    assert rows[r] == (1, 1) and (2, 4, 68, 64) in runs[run]
