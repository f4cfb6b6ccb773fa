"""The exactness argument of the device cover with `mark_close_neighboorhood` and
`select_patches_overlap_neighborhood` (csrc/ppp_cover.hip, foreground_cover.cover_options_device),
without a GPU: a NumPy model of the parallel rounds

    mark test  every undecided patch whose centre is marked is decided "not selected" -- in every round,
               whatever the dirty marks say;
    count      a patch whose neighbourhood changed is recounted; <= pix_th: "not selected";
    ready      no undecided patch of higher rank within (p_z - 1, max(p_y - 1, 3), max(p_x - 1, 3));
    select     every ready patch clears its voxels and writes its mark box (NumPy's slice rules),

followed by the stop rule's cut in rank order and the rebuild of the marks from the surviving set, must
select what the sequential loop of the oracle selects."""
import numpy as np
import pytest
import scipy.ndimage

import cover_marks_cases as cases

NONE = 1 << 40     # (exactly representable as the double scipy passes cval through)


def _pix_thresholds(ps, kw):
    if kw["select_patches_for_sparse_data"]:
        return [0]
    mid = int(np.prod(ps) / 2)
    return [t for t in [500, 100, 50, 10, 0] if t < mid]


def _mark_box(marked, c):
    # (plain slices, as the reference writes them: a negative start wraps around)
    marked[int(c[0]), slice(int(c[1]) - 3, int(c[1]) + 4), slice(int(c[2]) - 3, int(c[2]) + 4)] = True


class Model:
    def __init__(self, case, kw, mark_radius=3):
        self.c, self.kw = case, kw
        self.ps = case.ps
        self.rad = [p // 2 for p in self.ps]
        self.mark = bool(kw.get("mark_close_neighboorhood", False))
        self.coords = case.ranked_coords
        n = len(self.coords)
        fc = np.float32(kw["fc_threshold"])
        self.patch = (case.pred[(slice(None),) + tuple(self.coords.T)].T > fc).reshape([n] + self.ps)
        self.marked = np.zeros(case.shape, dtype=bool)
        self.selected = np.zeros(n, dtype=bool)
        r = [p - 1 for p in self.ps]
        if self.mark:
            r = [r[0], max(r[1], mark_radius), max(r[2], mark_radius)]
        self.ready_size = [2 * v + 1 for v in r]
        self.rounds = 0
        self.cut = 0

    def win(self, k):
        c = self.coords[k]
        return tuple(slice(int(c[i]) - self.rad[i], int(c[i]) + self.rad[i] + 1) for i in range(3))

    def one_pass(self, running, remaining, never, pix_th):
        """One pass: rounds, then the cut and the marks' rebuild.  Returns the interior voxels left."""
        shape, ps = self.c.shape, self.ps
        take = np.flatnonzero(~self.selected & ~never)
        rank_vol = np.full(shape, NONE, dtype=np.int64)
        rank_vol[tuple(self.coords[take].T)] = take
        dirty = np.ones(shape, dtype=bool)
        interior = np.zeros(shape, dtype=bool)
        interior[self.c.radslice] = True
        picked, cleared = [], {}
        while True:
            und = rank_vol[rank_vol != NONE]
            if len(und) == 0:
                break
            self.rounds += 1
            for k in und:
                c = tuple(self.coords[k])
                if self.mark and self.marked[c]:
                    rank_vol[c] = NONE
                elif dirty[c] and np.count_nonzero(running[self.win(k)] & self.patch[k]) <= pix_th:
                    rank_vol[c] = NONE
            dirty[:] = False
            nbr = scipy.ndimage.minimum_filter(rank_vol, size=self.ready_size, mode="constant", cval=NONE)
            for k in rank_vol[(rank_vol != NONE) & (nbr == rank_vol)]:
                c, w = self.coords[k], self.win(k)
                hit = running[w] & self.patch[k]
                cleared[k] = int(np.count_nonzero(hit & interior[w]))
                running[w][hit] = False
                dirty[tuple(slice(max(int(c[i]) - (ps[i] - 1), 0), int(c[i]) + ps[i]) for i in range(3))] = True
                if self.mark:
                    _mark_box(self.marked, c)
                rank_vol[tuple(c)] = NONE
                picked.append(int(k))
        # the stop rule: the loop ends right after the patch that empties the interior
        raw = len(picked)
        kept = []
        for k in sorted(picked):
            if remaining <= 0:
                break
            kept.append(k)
            remaining -= cleared[k]
        self.cut += raw - len(kept)
        self.selected[kept] = True
        if self.mark:       # a patch behind the cut has marked nothing
            self.marked[:] = False
            for k in np.flatnonzero(self.selected):
                _mark_box(self.marked, self.coords[k])
        return remaining

    def run(self):
        c, kw = self.c, self.kw
        n = len(self.coords)
        thr = kw.get("score_threshold", False)
        thr = thr if isinstance(thr, float) else None

        def first_below(cand):
            out = np.zeros(n, dtype=bool)
            below = np.flatnonzero(cand & (c.ranked_scores.astype(np.float64) < thr))
            if len(below):
                out[below[0]:] = True
            return out

        never = c.overlap_mask[tuple(self.coords.T)] > 0
        if thr is not None:
            never = never | first_below(np.ones(n, dtype=bool))
        running = c.mask_to_cover.astype(bool).copy()
        remaining = int(np.count_nonzero(running[c.radslice]))
        for pix_th in _pix_thresholds(self.ps, kw):
            if remaining > 0:
                remaining = self.one_pass(running, remaining, never, pix_th)
            if remaining < 1:
                break
        if not kw.get("select_patches_overlap_neighborhood", False):
            idx = np.flatnonzero(self.selected)
            return self.coords[idx], c.ranked_scores[idx]
        ov = c.overlap_mask > 0
        ring = ~scipy.ndimage.binary_dilation(ov, iterations=2) & scipy.ndimage.binary_dilation(ov, iterations=5) \
            & (c.mask_to_cover != 0)
        cand = ring[tuple(self.coords.T)] & ~self.selected
        never = ~cand
        if thr is not None:
            never = never | first_below(cand)
        remaining = int(np.count_nonzero(ring[c.radslice]))
        if cand.any() and remaining > 0:
            self.one_pass(ring.copy(), remaining, never, pix_th)
        chosen = np.zeros(c.shape, dtype=bool)
        chosen[tuple(self.coords[self.selected].T)] = True
        coords = np.argwhere(chosen)
        return coords, np.asarray(c.scores)[tuple(coords.T)]


def _same(got, want):
    assert np.array_equal(np.asarray(got[0]).reshape(-1, 3), np.asarray(want[0]).reshape(-1, 3))
    assert np.array_equal(np.asarray(got[1], dtype=np.float32), np.asarray(want[1], dtype=np.float32))


@pytest.mark.parametrize("option", ["mark", "ring", "both"])
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_rounds_model_equals_the_sequential_loop(name, option):
    case = cases.synthetic(name)
    want = case.oracle_cover(option)
    assert len(want[0]) > 0
    _same(Model(case, case.flags(option)).run(), want)


@pytest.mark.parametrize("name", ["c2d_p5_mark", "c3d_p3_mark_nosparse", "c3d_p3_near_overlap"])
def test_rounds_model_equals_the_reference_goldens(name):
    case = cases.from_golden(name)
    got = Model(case, case.kw).run()
    assert np.array_equal(got[0], case.cover_coords)


def test_the_wider_ready_radius_is_what_makes_3x3x3_exact():
    """At p = 3 the mark box (+-3) is wider than the window overlap radius (p - 1 = 2): with the ready
    radius left at p - 1, two patches 3 apart are selected in one round although the better ranked
    one marks the other's centre."""
    case = cases.synthetic("A")
    want = case.oracle_cover("mark")
    got = Model(case, case.flags("mark"), mark_radius=0).run()
    assert not np.array_equal(got[0], want[0])


def test_marks_come_from_the_patches_that_survive_the_cut():
    """cover_marks_cases.stop_rule: the rounds select a patch behind the cut, whose mark box holds the
    ring cover's candidate; with the marks rebuilt from the surviving set the candidate is selected."""
    case = cases.stop_rule()
    want = case.oracle_cover("both")
    assert [tuple(c) for c in want[0]] == [(0, 2, 22), (0, 4, 8), (0, 4, 22)]
    model = Model(case, case.flags("both"))
    _same(model.run(), want)
    assert model.cut == 1
