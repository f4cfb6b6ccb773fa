"""Inputs shared by tests/test_cover_marks_rule.py and tests/test_cover_marks_gpu.py: the synthetic
cases at which `mark_close_neighboorhood` / `select_patches_overlap_neighborhood` bite, each run
through the oracle once (consensus, scores, ranked list) and cached for the session."""
import functools

import numpy as np

from oracle import ppp_oracle as orc
from patchperpix_amd import synth
from tests_flags import FLYLIGHT

MARK = dict(mark_close_neighboorhood=True)
RING = dict(select_patches_overlap_neighborhood=True)
OPTIONS = {"mark": MARK, "ring": RING, "both": dict(MARK, **RING)}

# name -> (shape, patchshape, seed, cell, extra flags)
CASES = {
    # the 7 x 7 mark box exceeds p - 1; selected centres with cy < 3 or cx < 3 mark nothing
    "A": ((12, 40, 44), (3, 3, 3), 71, [5, 7, 7], {}),
    # 2-d
    "B": ((1, 60, 64), (1, 5, 5), 72, [1, 11, 11], {}),
    # passes at 50, 10 and 0 share one mark volume
    "C": ((20, 36, 40), (5, 5, 5), 73, [8, 9, 10], dict(select_patches_for_sparse_data=False)),
    # the score-threshold break
    "D": ((20, 36, 40), (5, 5, 5), 73, [8, 9, 10], dict(score_threshold=0.55)),
    # marks with a larger patch
    "E": ((14, 34, 36), (7, 7, 7), 74, [7, 10, 10], {}),
    # Y < 7: the mark box wraps, the host loop's business
    "W": ((10, 6, 30), (3, 3, 3), 76, [5, 3, 8], {}),
}


class Case:
    def __init__(self, shape, ps, pred, foreground, numinst, kw):
        self.shape, self.ps, self.kw = tuple(shape), [int(p) for p in ps], dict(kw)
        self.pred = np.ascontiguousarray(pred, dtype=np.float32)
        self.foreground, self.numinst = foreground, numinst
        self.overlap_mask = 1 * (numinst > 1)
        self.mask_to_cover = foreground.copy()
        self.mask_to_cover[self.overlap_mask > 0] = 0
        self.rad = np.array([p // 2 for p in self.ps])
        self.radslice = tuple(slice(int(self.rad[i]), self.shape[i] - int(self.rad[i])) for i in range(3))
        cons = orc.consensus(self.pred, self.overlap_mask, self.ps, **self.kw)
        self.scores = orc.rank(self.pred, cons, self.overlap_mask, self.ps, **self.kw)
        coords = orc.interior_fg_coords(foreground, self.rad)
        self.ranked_coords, self.ranked_scores = orc.rank_by_score(coords, self.scores)
        self.ranked_coords = np.ascontiguousarray(self.ranked_coords, dtype=np.int32)
        self.ranked_scores = np.ascontiguousarray(self.ranked_scores, dtype=np.float32)
        self._want = {}

    def flags(self, option):
        return dict(self.kw, **(OPTIONS[option] if option else {}))

    def oracle_cover(self, option):
        """(coords [m, 3], scores [m]) of oracle.foreground_cover, computed once per option."""
        if option not in self._want:
            sel = orc.foreground_cover(self.ranked_coords, self.ranked_scores, self.overlap_mask,
                                       self.mask_to_cover.copy(), self.pred, self.ps, scores_array=self.scores,
                                       **self.flags(option))
            if isinstance(sel, tuple):
                self._want[option] = (np.asarray(sel[0]).reshape(-1, 3), np.asarray(sel[1]))
            else:
                self._want[option] = (self.ranked_coords[sel], self.ranked_scores[sel])
        return self._want[option]


@functools.lru_cache(maxsize=None)
def synthetic(name):
    shape, ps, seed, cell, extra = CASES[name]
    c = synth.make_case(shape, ps, seed=seed, cell=cell, overlap_frac=0.03, kind="cells")
    return Case(shape, ps, c["pred"], c["foreground"], c["numinst"], dict(FLYLIGHT, **extra))


@functools.lru_cache(maxsize=None)
def from_golden(name):
    """A reference-made golden as a Case (its ranked list and cover are the reference's own)."""
    from conftest import Golden
    g = Golden(name)
    c = Case.__new__(Case)
    c.shape, c.ps, c.kw = tuple(g.foreground.shape), g.patchshape, dict(g.kw)
    c.pred, c.foreground, c.numinst = g.pred, g.foreground, g.numinst
    c.overlap_mask = g.overlap_mask
    c.mask_to_cover = g.foreground.copy()
    c.mask_to_cover[c.overlap_mask > 0] = 0
    c.rad = np.array([p // 2 for p in c.ps])
    c.radslice = tuple(slice(int(c.rad[i]), c.shape[i] - int(c.rad[i])) for i in range(3))
    c.scores = g["scores"]
    c.ranked_coords = np.ascontiguousarray(g["ranked_coords"], dtype=np.int32)
    c.ranked_scores = np.ascontiguousarray(g["ranked_scores"], dtype=np.float32)
    c.cover_coords = g["cover_coords"]
    c._want = {}
    return c


@functools.lru_cache(maxsize=None)
def stop_rule():
    """A hand-built 2-d case, p = (1, 5, 5) on (1, 9, 48), in which the stop rule's cut decides the ring
    cover.  Every patch predicts its whole window.  The mask holds two interior voxels, (4, 8) and
    (4, 22), and one voxel of a border row, (1, 17); (4, 26) is an overlap voxel.  Ranked list:
        0  (4, 8)    selected, clears (4, 8)
        1  (2, 22)   selected, clears (4, 22): the interior is empty, the sequential loop ENDS here.
                     cy < 3: this patch marks nothing.
        2  (3, 19)   still covers the border voxel (1, 17): a pass that decides every patch selects
                     it, the cut drops it.  Its mark box (y 0..6, x 16..22) holds (4, 22).
        3  (4, 22)   not selected in the first cover (its window is empty by then); the ring (distance
                     3..5 from the overlap voxel, inside the mask) is the voxel (4, 22) alone, so it is
                     the ring cover's one candidate -- selected there unless patch 2 left its marks."""
    shape, ps = (1, 9, 48), (1, 5, 5)
    kw = dict(FLYLIGHT, **OPTIONS["both"])
    c = Case.__new__(Case)
    c.shape, c.ps, c.kw = shape, list(ps), kw
    c.pred = np.full((25,) + shape, 0.95, dtype=np.float32)
    c.foreground = np.zeros(shape, dtype=bool)
    for y, x in [(4, 8), (4, 22), (1, 17)]:
        c.foreground[0, y, x] = True
    c.numinst = c.foreground.astype(np.uint8)
    c.numinst[0, 4, 26] = 2
    c.overlap_mask = 1 * (c.numinst > 1)
    c.mask_to_cover = c.foreground.copy()
    c.rad = np.array([0, 2, 2])
    c.radslice = (slice(0, 1), slice(2, 7), slice(2, 46))
    c.ranked_coords = np.array([[0, 4, 8], [0, 2, 22], [0, 3, 19], [0, 4, 22]], dtype=np.int32)
    c.ranked_scores = np.array([0.9, 0.8, 0.7, 0.6], dtype=np.float32)
    c.scores = np.zeros(shape, dtype=np.float32)
    c.scores[tuple(c.ranked_coords.T)] = c.ranked_scores
    c._want = {}
    return c
