"""The count and select sweeps of a greedy-cover / thinning round (csrc/ppp_cover.hip) where their lane groups
can go wrong.

The recount of a listed patch is dealt to a group of lanes that strides over the pz * py rows of its window
(hits = the sum over the group, witness = the minimum of the lanes' first-hit codes); the select sweep asks for
the other slices of its candidates by groups of lanes and clears the windows of several winners of a wave
together.  None of that may change what a round computes.  Same method as tests/test_cover_sweeps.py: whole
passes against the one-shard step model of tests/shard_lockstep.py -- state, cleared counts, running mask, kept
set and the NUMBER OF ROUNDS (rounded up to the batch the host synchronises after), all exact -- on shapes
chosen for the groups:

  * (19, 19, 70) with 9^3: 81 window rows, more than one row a lane and a second trip of the select's rows;
    windows straddle the mask words at x = 32 and 64;
  * (15, 14, 37) and (11, 16, 40) with 7^3: a volume below one count workgroup's 4 096 voxels and one just
    over it (a part-filled last workgroup); X is no multiple of 32;
  * (9, 12, 67) with 5^3: groups of 4 lanes;
  * (7, 11, 45) with (3, 5, 7): anisotropic, the run-time filter;
  * (1, 30, 66) with (1, 11, 11): one plane -- the select has no other slice to ask for;
  * (2, 60, 70) with (1, 25, 25): a 25-bit window that almost always spans two mask words.
Both pix_th values run: 0 is the witness path, 10 the dirty-mark path.  The witness volume is not reachable
through the step API; its equality is implied by the round count -- a patch whose witness is not the first
covered voxel of its window is recounted, and so rejected, in another round than the model's, and a wrong
witness that points at a cleared voxel or outside the window changes the recounts the same way.
The same passes also run through the device's one-shard STEP entry points (the sharded bodies: local table
index from loc_vol), which must take exactly the model's number of rounds."""
import numpy as np
import pytest

import shard_lockstep as ls

COVER_BATCH = 8                     # rounds per host synchronisation (ppp_cover.hip)
PIX_THS = [10, 0]
CASES = {"p9": ((19, 19, 70), (9, 9, 9)), "p7_small": ((15, 14, 37), (7, 7, 7)), "p7_two_wg": ((11, 16, 40), (7, 7, 7)),
         "p5": ((9, 12, 67), (5, 5, 5)), "p3x5x7": ((7, 11, 45), (3, 5, 7)), "p1x11x11": ((1, 30, 66), (1, 11, 11)),
         "p1x25x25": ((2, 60, 70), (1, 25, 25))}
_MODEL = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert backend.device_count() >= 1
    return torch


def model_of(name):
    """the case and its one-shard model runs (CPU), made once and left unchanged"""
    if name not in _MODEL:
        shape, ps = CASES[name]
        case = ls.Case(shape, ps, seed=3)
        side = ls.ModelSide()
        whole = (0, shape[0])
        _MODEL[name] = (case, ls.run_cover(case, whole, [side], PIX_THS)["passes"],
                        ls.run_thin(case, whole, [side])["passes"][0])
    return _MODEL[name]


def batches(rounds):
    return (rounds + COVER_BATCH - 1) // COVER_BATCH * COVER_BATCH


def kept_set(case, model):
    """the model's kept patches in the order the loop picks them (count descending, index ascending), cut where
    the interior is empty"""
    kept = np.flatnonzero(model["state"] == 1)
    order = kept[np.lexsort((kept, -model["count"][kept]))]
    left = case.interior - np.cumsum(model["cleared"][order])
    done = np.flatnonzero(left <= 0)
    chosen = np.zeros(case.n, dtype=bool)
    chosen[order[:done[0] + 1] if len(done) else order] = True
    if not len(done):
        chosen[0] = True                                  # every count 0 with voxels left: np.argmax picks patch 0
    return chosen


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_cover_passes_equal_step_model(name, torch_cuda):
    from patchperpix_amd import backend
    torch = torch_cuda
    case, model_passes, _ = model_of(name)
    assert len(model_passes) == len(PIX_THS), "the first pass emptied the interior: the case is too easy"
    assert model_passes[0]["rounds"] > COVER_BATCH
    P = case.params()
    bits_d = case.bits(ls.DeviceSide())
    assert np.array_equal(bits_d.cpu().numpy(), case.bits(ls.ModelSide()).numpy())
    lin_d = torch.from_numpy(case.lin).cuda()
    mask_d = torch.from_numpy(case.mask.copy()).cuda()
    selected = np.zeros(case.n, dtype=bool)
    for p, pix_th in enumerate(PIX_THS):
        model = model_passes[p]
        state_d = torch.from_numpy(selected.astype(np.int32)).cuda()
        cleared_d, rounds = backend.cover_pass_device(mask_d, bits_d, lin_d, state_d, pix_th, P)
        state, cleared = state_d.cpu().numpy(), cleared_d.cpu().numpy()
        print("%s pix_th %d: %d rounds (model %d), %d selected" % (name, pix_th, rounds, model["rounds"],
                                                                   int((state == 1).sum())))
        assert np.array_equal(state, model["state"]), "pass %d: state" % p
        assert np.array_equal(cleared, model["cleared"]), "pass %d: cleared interior voxels" % p
        assert np.array_equal(mask_d.cpu().numpy(), model["mask"]), "pass %d: running mask" % p
        assert rounds == batches(model["rounds"]), "pass %d: %d rounds, the model needs %d" % (p, rounds, model["rounds"])
        selected = model["selected"].copy()               # (the stop rule between the passes is the model's)
    assert selected.sum() > 30


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_thinning_equals_step_model(name, torch_cuda):
    from patchperpix_amd import backend
    torch = torch_cuda
    case, _, model = model_of(name)
    P = case.params()
    bits_d = case.bits(ls.DeviceSide())
    mask_d = torch.from_numpy(case.mask.copy()).cuda()
    keep = backend.thin_cover_device(mask_d, bits_d, torch.from_numpy(case.lin).cuda(), P).cpu().numpy()
    rounds = int(backend.NOTES["thin_rounds"])
    print("%s thinning: %d rounds (model %d), %d of %d kept" % (name, rounds, model["rounds"], int(keep.sum()), case.n))
    assert np.array_equal(mask_d.cpu().numpy(), case.mask), "the thinning wrote the caller's mask"
    assert np.array_equal(keep != 0, kept_set(case, model)), "kept set of the step model"
    assert 0 < keep.sum() < case.n
    assert rounds == batches(model["rounds"]), "%d rounds, the model needs %d" % (rounds, model["rounds"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_step_entry_points_equal_step_model(name, torch_cuda):
    """the one-shard run of the device's step entry points: state, cleared counts, mask and the exact number of
    rounds of every cover pass and of the thinning (which also records the count a patch was kept with)"""
    case, model_passes, model_thin = model_of(name)
    whole = (0, case.shape[0])
    got = ls.run_cover(case, whole, [ls.DeviceSide()], PIX_THS)["passes"]
    assert len(got) == len(model_passes)
    for p, (g, m) in enumerate(zip(got, model_passes)):
        for what in ("state", "cleared", "mask", "selected"):
            assert np.array_equal(g[what], m[what]), "cover pass %d: %s" % (p, what)
        assert g["rounds"] == m["rounds"], "cover pass %d: %d rounds, the model needs %d" % (p, g["rounds"], m["rounds"])
    g = ls.run_thin(case, whole, [ls.DeviceSide()])["passes"][0]
    for what in ("state", "cleared", "count", "mask"):
        assert np.array_equal(g[what], model_thin[what]), "thinning: %s" % what
    assert g["rounds"] == model_thin["rounds"], "thinning: %d rounds, the model needs %d" % (g["rounds"], model_thin["rounds"])
