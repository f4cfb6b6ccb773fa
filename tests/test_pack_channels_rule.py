"""`no_overlap_per_channel` (graph_to_labeling.py:57-115) in closed form, on the CPU.  The reference
places every component by painting it and testing it against the channels painted so far; the closed
form (stated at the head of csrc/ppp_pack_channels.hip) needs only the components' sizes and the set of
overlapping label pairs (ppp_host_pack_channels), and gives the map as one "largest label of the
channel wins" paint.  Both are held equal to the loop here: on random voxel sets, and on the direct
cases of test_pack_channels_gpu.py against the oracle's paint_per_channel."""
import numpy as np
import pytest

import pack_channels_cases as pc
from patchperpix_amd import backend


def closed_form(masks, min_voxels):
    sizes = masks.reshape(len(masks), -1).sum(1)
    chan, n_ch = backend.host_pack_channels(sizes, pc.overlap_pairs(masks), min_voxels)
    return chan, n_ch, pc.map_from_channels(masks, chan, n_ch)


def check(masks, min_voxels):
    want_chan, want_map = pc.loop_on_masks(masks, min_voxels)
    chan, n_ch, got = closed_form(masks, min_voxels)
    assert np.array_equal(chan, want_chan), (min_voxels, chan, want_chan)
    assert n_ch == want_map.shape[0]
    assert np.array_equal(got, want_map)
    return n_ch


def random_masks(rng, K, shape=(12, 14), p_empty=0.15):
    """K boxes of random size and place on a small grid, thinned at random; some are empty"""
    masks = np.zeros((K,) + shape, bool)
    for k in range(K):
        if rng.random() < p_empty:
            continue
        h, w = rng.integers(1, shape[0] + 1), rng.integers(1, shape[1] + 1)
        y, x = rng.integers(0, shape[0] - h + 1), rng.integers(0, shape[1] - w + 1)
        masks[k, y:y + h, x:x + w] = rng.random((h, w)) < rng.choice([0.3, 0.7, 1.0])
    return masks


@pytest.mark.parametrize("seed", range(12))
def test_walk_equals_the_loop_on_random_voxel_sets(seed):
    rng = np.random.default_rng(seed)
    masks = random_masks(rng, int(rng.integers(1, 15)))
    largest = int(masks.reshape(len(masks), -1).sum(1).max())
    channels = {check(masks, mv) for mv in sorted({0, 1, largest // 4, largest // 2, largest - 1, largest} - {-1})}
    assert 1 in channels                  # min_voxels = the largest size: everything lands in channel 0


def test_walk_on_the_corner_cases():
    full = np.ones((6, 7), bool)
    K = 6
    # all large and mutually overlapping: a channel each
    assert check(np.stack([full] * K), 0) == K
    # all small: one channel, the last one on top
    assert check(np.stack([full] * K), full.sum()) == 1
    # a large component 0, then small ones over it and a large one that has to move on
    masks = np.zeros((4, 6, 7), bool)
    masks[0] = full
    masks[1, :2, :2] = True
    masks[2, 1:3, 1:3] = True
    masks[3, :, 3:] = True
    assert check(masks, 5) == 2
    # empty components: the first opens channel 0 without taking a voxel of it, a later one changes nothing
    masks = np.zeros((4, 6, 7), bool)
    masks[1] = full
    masks[3, 2:, :] = True
    assert check(masks, 3) == 2 and check(masks, 0) == 2 and check(masks, 100) == 1
    # disjoint large components share channel 0; one that overlaps only a SMALL one of channel 0 still moves on
    masks = np.zeros((4, 6, 7), bool)
    masks[0, :, :2] = True
    masks[1, :, 2:4] = True
    masks[2, 0, 4] = True
    masks[3, :, 4:] = True
    assert check(masks, 5) == 2
    # no component at all
    chan, n_ch = backend.host_pack_channels(np.zeros(0, np.int64), np.zeros(0, np.uint64), 2000)
    assert len(chan) == 0 and n_ch == 0


def test_walk_takes_repeated_pairs_in_any_order_and_refuses_bad_ones():
    rng = np.random.default_rng(5)
    masks = random_masks(rng, 10, p_empty=0.0)
    sizes = masks.reshape(len(masks), -1).sum(1)
    pairs = pc.overlap_pairs(masks)
    want = backend.host_pack_channels(sizes, pairs, 20)
    shuffled = rng.permutation(np.concatenate([pairs, pairs, pairs[:3]]))
    got = backend.host_pack_channels(sizes, shuffled, 20)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    for bad in ((3 << 32) | 3, (2 << 32) | 3, (11 << 32) | 1, 1):      # a == b, a > b, b > K, b == 0
        with pytest.raises(RuntimeError):
            backend.host_pack_channels(sizes, np.array([bad], np.uint64), 20)


@pytest.mark.parametrize("i", range(len(pc.DIRECT)))
def test_closed_form_equals_the_oracle_on_the_direct_cases(i):
    """fact 3 (and the walk at the reference's 2000 voxels) on the cases the device path is run on"""
    want, masks = pc.direct_expected(i)
    chan, n_ch, got = closed_form(masks, backend.PACK_MIN_VOXELS)
    assert n_ch == want.shape[0]
    assert np.array_equal(got, want)
