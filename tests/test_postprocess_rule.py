"""CPU: the closed form the device dilation computes (csrc/ppp_postprocess.hip, "dilation") equals the
reference's in-place ascending loop, and postprocess.post_steps on the host path equals the block
the label drivers used to spell out.

The rule, with N[v] = v and its six face neighbours and everything outside the volume background:
    a voxel u with id a > 0 SURVIVES  iff  no face neighbour w with 0 < id(w) < a survives
    result(v) = the largest id among the survivors in N[v], 0 when there is none
It is restated here in NumPy, round by round like the kernels, so that the algorithm is pinned on a
machine without a GPU; tests/test_postprocess_gpu.py runs the kernels on the same maps."""
import numpy as np
import pytest

from patchperpix_amd import postprocess

SHIFTS = [(0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1)]


def _shifted(a, axis, step, fill):
    """a moved by one voxel along axis: out[v] = a[v + step], `fill` outside"""
    out = np.full_like(a, fill)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if a.shape[axis] > 1:
        src[axis] = slice(1, None) if step > 0 else slice(None, -1)
        dst[axis] = slice(None, -1) if step > 0 else slice(1, None)
        out[tuple(dst)] = a[tuple(src)]
    return out


def survivor_dilate(ids):
    """(dilated map, rounds): the survivor rule, decided in synchronous rounds"""
    a = np.asarray(ids).astype(np.int64)
    UND, SURV, DEAD = 0, 1, 2
    state = np.where(a > 0, UND, DEAD)
    rounds = 0
    while (state == UND).any():
        killed = np.zeros(a.shape, bool)
        wait = np.zeros(a.shape, bool)
        for axis, step in SHIFTS:
            b = _shifted(a, axis, step, 0)
            sb = _shifted(state, axis, step, DEAD)
            smaller = (b > 0) & (b < a)
            killed |= smaller & (sb == SURV)
            wait |= smaller & (sb == UND)
        und = state == UND
        new = state.copy()
        new[und & killed] = DEAD
        new[und & ~killed & ~wait] = SURV
        assert not np.array_equal(new, state), "a round decided nothing"
        state = new
        rounds += 1
    best = np.where(state == SURV, a, 0)
    for axis, step in SHIFTS:
        best = np.maximum(best, np.where(_shifted(state, axis, step, DEAD) == SURV, _shifted(a, axis, step, 0), 0))
    return best.astype(np.asarray(ids).dtype), max(rounds, 1)


def random_maps():
    """seeded maps, 1 .. 9 voxels per axis, up to 12 labels, some background"""
    rng = np.random.default_rng(20241)
    shapes = [(1, 7, 9), (1, 1, 1), (5, 1, 1), (9, 1, 1), (1, 9, 1), (2, 2, 2), (3, 4, 5), (9, 9, 9), (4, 9, 2)]
    shapes += [tuple(int(v) for v in rng.integers(1, 10, 3)) for _ in range(40)]
    maps = []
    for k, shape in enumerate(shapes):
        n_labels = int(rng.integers(1, 13))
        m = rng.integers(0, n_labels + 1, shape).astype(np.uint32)
        if k % 3 == 0:
            m[rng.random(shape) < 0.4] = 0
        maps.append(m)
    return maps


def staircases():
    """ids descending along an axis: every voxel waits for its smaller neighbour, one round per step"""
    maps = []
    line = np.arange(10, 0, -1, dtype=np.uint32)
    maps.append(line.reshape(1, 1, 10).copy())
    maps.append(line.reshape(10, 1, 1).copy())
    yy, xx = np.meshgrid(np.arange(6), np.arange(8), indexing="ij")
    maps.append((20 - yy - xx).astype(np.uint32)[None].copy())                    # a 2-d staircase
    zz, yy, xx = np.meshgrid(np.arange(4), np.arange(4), np.arange(5), indexing="ij")
    maps.append((3 * (13 - zz - yy - xx) + 1).astype(np.uint32))                  # 3-d, ids with gaps
    m = np.tile(np.arange(9, 0, -1, dtype=np.uint32), (3, 4, 1))
    m[1, 2, 4] = 0                                                                # a hole in the stairs
    maps.append(m)
    return maps


@pytest.mark.parametrize("k", range(len(random_maps())))
def test_survivor_rule_equals_the_ascending_loop_on_random_maps(k):
    m = random_maps()[k]
    got, _ = survivor_dilate(m)
    assert np.array_equal(got, postprocess.dilate_instances(m))


@pytest.mark.parametrize("k", range(len(staircases())))
def test_survivor_rule_equals_the_ascending_loop_on_staircases(k):
    m = staircases()[k]
    got, rounds = survivor_dilate(m)
    assert np.array_equal(got, postprocess.dilate_instances(m))
    assert rounds >= 2


def stitched_map():
    """the map of test_many_ids.test_stitched_entry_compacts_uint32_ids"""
    inst32 = np.zeros((4, 12, 12), dtype=np.uint32)
    inst32[1, 2:6, 2:6] = 70001
    inst32[2, 6:10, 6:10] = 400123
    inst32[3, 1, 1] = 99999
    return inst32


def inline_block(instances, foreground, res_key, **kw):
    """the post-step block as tiling._stitch_main spelled it out before post_steps existed"""
    if kw.get("remove_small_comps", 0) > 0:
        instances = postprocess.relabel(postprocess.remove_small_components(instances, kw["remove_small_comps"]))
    masked = instances.copy()
    masked[foreground == 0] = 0
    datasets = {res_key: instances.astype(np.uint16), "vote_foreground": foreground.astype(np.uint16),
                res_key + "_masked": masked.astype(np.uint16)}
    if kw.get("dilate_instances", False):
        dil = postprocess.dilate_instances(instances)
        datasets[res_key + "_dil_1"] = dil.astype(np.uint16)
        datasets[res_key + "_masked_dil_1"] = np.where(foreground == 0, 0, dil).astype(np.uint16)
    return instances, datasets


@pytest.mark.parametrize("kw", [dict(remove_small_comps=2, dilate_instances=True), dict(remove_small_comps=2),
                                dict(dilate_instances=True), dict()])
def test_post_steps_on_the_host_equals_the_inline_block(kw, monkeypatch):
    monkeypatch.setenv("PPP_POSTPROCESS", "host")
    assert not postprocess.use_device()
    inst32 = stitched_map()
    fg = inst32 > 0
    fg[1, 2, 2] = False                       # the masked datasets differ from the plain ones
    want_inst, want = inline_block(inst32.copy(), fg, "vote_instances", **kw)
    got_inst, got = postprocess.post_steps(inst32.copy(), fg, "vote_instances", **kw)
    assert got_inst.dtype == want_inst.dtype and np.array_equal(got_inst, want_inst)
    assert list(got) == list(want)
    for key in want:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    if kw.get("remove_small_comps"):
        assert set(np.unique(got_inst)) == {0, 1, 2}
