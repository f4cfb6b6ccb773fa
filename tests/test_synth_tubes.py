"""synth.make_case(kind="tubes"): the sparse-foreground generator (thin tubes, a few percent
foreground -- the flylight neurons; every other kind is >= 90 % foreground)."""
import hashlib

import numpy as np
import pytest

from patchperpix_amd import synth

# the two parameter sets of the end-to-end fixtures (tests/golden/gen_scale_tubes_fixture.py)
SETS = [((96, 96, 96), (9, 9, 9), 14), ((70, 140, 140), (7, 7, 7), 15)]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_tubes_are_deterministic_per_seed():
    a = synth.make_case((24, 40, 72), [5, 5, 5], seed=5, kind="tubes", n_tubes=3, radius=2.5, overlap_frac=0.02)
    b = synth.make_case((24, 40, 72), [5, 5, 5], seed=5, kind="tubes", n_tubes=3, radius=2.5, overlap_frac=0.02)
    c = synth.make_case((24, 40, 72), [5, 5, 5], seed=6, kind="tubes", n_tubes=3, radius=2.5, overlap_frac=0.02)
    for k in ("pred", "foreground", "numinst", "labels"):
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["labels"], c["labels"])
    assert np.array_equal(a["foreground"], a["labels"] != 0)
    assert a["pred"].shape == (125, 24, 40, 72) and a["pred"].dtype == np.float32
    assert a["numinst"].max() == 2 and not np.any(a["numinst"][~a["foreground"]])


@pytest.mark.parametrize("shape,ps,n", SETS)
def test_every_tube_is_present_and_foreground_is_sparse(shape, ps, n):
    lab = synth.tube_labels(shape, n_tubes=n, radius=2.5, seed=0)
    assert sorted(np.unique(lab).tolist()) == list(range(n + 1))
    r = [p // 2 for p in ps]
    inner = lab[r[0]:shape[0] - r[0], r[1]:shape[1] - r[1], r[2]:shape[2] - r[2]]
    share = float(np.count_nonzero(inner)) / inner.size
    print("interior foreground share", shape, share)
    assert 0.01 <= share <= 0.05, share


def test_cells_are_unchanged():
    """kind="cells" for a fixed seed, bit for bit what the generator made before kind="tubes" existed"""
    c = synth.make_case((20, 22, 24), [5, 5, 5], seed=3, kind="cells", overlap_frac=0.02)
    assert _sha(c["pred"]) == "a6e5a70a7080251a73c0b565a7ac342420008262130615bb38a6c5fdbf25aee3"
    assert _sha(c["foreground"]) == "61e96975140ed592b4d5fd5efafea2cd94fe338fc7a182fdcaef97e2781941f8"
    assert _sha(c["numinst"]) == "008673b28ecc3ea6d5a557c7911db8e8ca01771af9645c462e2c62af3de1306f"
    assert _sha(c["labels"]) == "8cd30ee2d22bcb3756b4a94bf497120cbc1c1a8795b5d9b9c6baf17e0cbeb095"
