"""CPU: the host side of the batched 2-d mode (``independent_slices=True``): what it refuses,
the chunk plan, the per-slice split of the intermediates."""
import os

import numpy as np
import pytest

from patchperpix_amd import tiling
from patchperpix_amd.flags import FLYLIGHT
from patchperpix_amd.vote_instances import batch2d
from patchperpix_amd.vote_instances import vote_instances as vi


def _case(N=3, Y=20, X=22):
    pred = np.zeros((25, N, Y, X), np.float32)
    fg = np.zeros((N, Y, X), bool)
    return pred, fg, fg.copy(), np.zeros((N, Y, X), np.uint8)


def test_a_stack_without_the_opt_in_is_still_refused():
    pred, fg, mask, ni = _case()
    with pytest.raises(ValueError, match="call once per slice"):
        vi.to_instance_seg(pred, fg, mask, ni, (1, 5, 5), **FLYLIGHT)


def test_the_opt_in_needs_2d_patches():
    pred, fg, mask, ni = _case()
    with pytest.raises(ValueError, match="2-d patches"):
        vi.to_instance_seg(pred, fg, mask, ni, (3, 5, 5), independent_slices=True, **FLYLIGHT)


@pytest.mark.parametrize("flag", batch2d.UNSUPPORTED_FLAGS)
def test_flags_a_batch_cannot_reproduce_are_refused_by_name(flag):
    pred, fg, mask, ni = _case()
    with pytest.raises(NotImplementedError, match=flag):
        vi.to_instance_seg(pred, fg, mask, ni, (1, 5, 5), independent_slices=True, **dict(FLYLIGHT, **{flag: True}))


@pytest.mark.parametrize("name", batch2d.UNSUPPORTED_INPUTS)
def test_stored_stage_inputs_are_refused_by_name(name):
    pred, fg, mask, ni = _case()
    with pytest.raises(NotImplementedError, match=name):
        vi.to_instance_seg(pred, fg, mask, ni, (1, 5, 5), independent_slices=True, **dict(FLYLIGHT, **{name: "x"}))


def test_numpy_semantics_and_sampling_are_refused():
    pred, fg, mask, ni = _case()
    with pytest.raises(NotImplementedError, match="cuda=False"):
        vi.to_instance_seg(pred, fg, mask, ni, (1, 5, 5), independent_slices=True, **dict(FLYLIGHT, cuda=False))
    with pytest.raises(NotImplementedError, match="sample"):
        vi.to_instance_seg(pred, fg, mask, ni, (1, 5, 5), independent_slices=True, **dict(FLYLIGHT, sample=0.5))


def test_slice_chunks():
    assert tiling.plan_slice_chunks(32, 100, 1000) == 10
    assert tiling.plan_slice_chunks(32, 100, 10 ** 9) == 32
    assert tiling.plan_slice_chunks(32, 100, 50) == 1           # at least one slice
    assert tiling.plan_slice_chunks(0, 100, 1000) == 1
    assert tiling.plan_slice_chunks(5, 100, -1) == 1
    # a 256^2 slice at 25^2 patches: compact planes + voxel-major rows, ~0.95 GB
    b = batch2d.slice_bytes((256, 256), (1, 25, 25))
    assert 0.9e9 < b < 1.0e9


def test_rows_split_by_slice_keep_their_order_with_local_z():
    rows = np.array([[0, 5, 5, 0, 5, 8], [2, 4, 4, 2, 6, 4], [0, 5, 8, 0, 9, 9],
                     [0, 5, 5, 0, 5, 5], [2, 4, 4, 2, 4, 4]], np.uint32)
    aff = np.arange(5, dtype=np.float32)
    out = batch2d.split_rows(rows, aff, 3)
    assert out[1] == (None, None)
    assert np.array_equal(out[0][0], rows[[0, 2, 3]]) and np.array_equal(out[0][1], aff[[0, 2, 3]])
    want = rows[[1, 4]].copy()
    want[:, [0, 3]] = 0
    assert np.array_equal(out[2][0], want) and np.array_equal(out[2][1], aff[[1, 4]])


def test_cli_batches_are_voted_as_soon_as_they_fill(tmp_path, monkeypatch):
    """do_all_batched (run_ppp --do label with batch_2d) holds at most batch_2d samples of a shape:
    5 samples of one shape with batch_2d = 2 are voted as 2, 2 and 1, each group right after its
    last sample was read; a sample of another shape forms a group of its own."""
    rng = np.random.default_rng(0)
    names = ["a0", "a1", "a2", "a3", "a4", "b0"]
    for n in names:
        Y, X = (20, 22) if n[0] == "a" else (18, 24)
        np.save(tmp_path / (n + ".npy"), rng.random((25, Y, X), dtype=np.float32))
    events = []
    load = vi.loadAffinities

    def loading(aff_file, *a, **k):
        events.append(("load", os.path.basename(aff_file)))
        return load(aff_file, *a, **k)

    def voting(pred, fg, mask, ni, ps, **k):
        assert k.get("independent_slices") is True
        events.append(("vote", int(pred.shape[1])))
        return np.zeros(fg.shape, np.uint16), fg.astype(np.uint8)

    written = []
    monkeypatch.setattr(vi, "loadAffinities", loading)
    monkeypatch.setattr(vi, "to_instance_seg", voting)
    monkeypatch.setattr(vi, "write_result", lambda fn, ds: written.append(os.path.basename(fn)))
    files = [str(tmp_path / (n + ".npy")) for n in names]
    vi.do_all_batched(files, patchshape=[1, 5, 5], batch_2d=2, **dict(FLYLIGHT, result_folder=str(tmp_path)))
    assert [e[1] for e in events if e[0] == "vote"] == [2, 2, 1, 1]
    assert events[:3] == [("load", "a0.npy"), ("load", "a1.npy"), ("vote", 2)]
    assert events[3:6] == [("load", "a2.npy"), ("load", "a3.npy"), ("vote", 2)]
    assert sorted(written) == sorted(n + ".hdf" for n in names)
