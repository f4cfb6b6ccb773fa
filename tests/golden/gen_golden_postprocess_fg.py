#!/usr/bin/env python3
"""tests/golden/postprocess_fg/fg_*.npz (a folder of their own: tests/conftest.py takes every *.npz directly under
tests/golden that it does not know by prefix for a vote_instances golden): the reference's own `postprocess_fg` (PatchPerPix/util/postprocess.py:122-199,
imported in place as fuzz_postprocess_vs_reference.py does; stubs for colorcet, skimage, zarr, h5py and
nrrd: zarr.open -> a dict of arrays, h5py.File -> a recorder) on small foreground predictions, with
export_skeleton_nrrds off.  Each file holds the input array, the kwargs (JSON), `volumes/fg` and
`volumes/instances`.  Development container only.

  python tests/golden/gen_golden_postprocess_fg.py

Every case with a positive max_distance_to_fg is built so that the reference is defined on it: a big
component exists and at least one small component is removed -- and, with T = the smallest integer whose
square root reaches the distance, small components sit at the two squared distances next to the bound
that a separate component can have (`around`): the smallest one >= T (T itself for distances 2 and 3, 8 for
2.5, because 7 is no sum of three squares; removed) and the largest one < T (8 for 3, 6 for 2.5; kept;
none for 2, where T = 4 and anything nearer touches the big component).  The generator asserts all of it."""
import contextlib
import importlib.util
import io
import json
import os
import sys
import types

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "postprocess_fg")
REF = "/root/reference/PatchPerPix/util/postprocess.py"

STORE = {}          # "file name" -> {key: array}: what the stubbed zarr.open hands out
WRITTEN = {}        # "file name" -> {dataset: array}: what the stubbed h5py.File recorded


class Recorder:
    def __init__(self, fn, mode):
        assert mode == "w"
        self.sets = WRITTEN.setdefault(fn, {})

    def create_dataset(self, name, data=None, dtype=None, compression=None):
        assert compression == "gzip"
        self.sets[name] = np.asarray(data).astype(dtype)


def load_reference():
    for name in ("colorcet", "skimage", "skimage.morphology", "zarr", "h5py", "nrrd"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["skimage.morphology"].skeletonize_3d = None
    sys.modules["zarr"].open = lambda fn, mode="r": STORE[fn]
    sys.modules["h5py"].File = Recorder
    spec = importlib.util.spec_from_file_location("ppp_ref_postprocess", REF)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def smallest_square(m):
    t = 0
    while np.sqrt(np.float64(t)) < np.float64(m):
        t += 1
    return t


def around(T):
    """(lo, hi): the squared distances a separate component can have that lie next to T on either side.
    hi = the smallest sum of three squares >= T (7 is none: max_distance_to_fg = 2.5 has T = 7, hi = 8);
    lo = the largest one below T that is >= 4, or None (a voxel at d2 <= 3 is within one step on every axis
    of a big voxel, so it belongs to that component: at max_distance_to_fg = 2, T = 4, nothing small can
    be nearer than T and none is kept)."""
    sums = sorted({a * a + b * b + c * c for a in range(6) for b in range(6) for c in range(6)})
    hi = min(v for v in sums if v >= T)
    lo = [v for v in sums if 4 <= v < T]
    return (max(lo) if lo else None), hi


def build_case(shape, T, seed):
    """Two big blocks in opposite corners; single voxels at the squared distances lo, hi (`around`), the
    next value above hi, and lo and hi once more
    from them (each the first free voxel in raster order at exactly that distance with nothing set within
    two voxels of it); then dust: single voxels and pairs with nothing set within two voxels.  The
    distances are measured again by `brute_min_d2`, not trusted from here."""
    rng = np.random.default_rng(seed)
    Z, Y, X = shape
    m = np.zeros(shape, dtype=bool)
    m[0:3, 0:4, 0:4] = True                            # 48 voxels
    m[Z - 3:Z, Y - 4:Y, X - 6:X] = True                # 72 voxels
    d2_big = np.rint(ndimage.distance_transform_edt(~m) ** 2).astype(np.int64)
    small = np.zeros(shape, dtype=bool)

    def free(z, y, x0, x1):
        """not 26-adjacent to a big block (d2 >= 4), no small voxel within two voxels"""
        return d2_big[z, y, x0:x1 + 1].min() >= 4 and \
            not small[max(z - 2, 0):z + 3, max(y - 2, 0):y + 3, max(x0 - 2, 0):x1 + 3].any()
    if T > 0:
        lo, hi = around(T)
        for want in (lo, hi, around(hi + 1)[1], lo, hi):
            if want is None:
                continue
            for z, y, x in np.argwhere(d2_big == want):
                if free(z, y, x, x):
                    small[z, y, x] = True
                    break
            else:
                raise AssertionError("no room for a component at d2 = %d" % want)
    for _ in range(12):
        z, y, x = (int(rng.integers(0, n)) for n in shape)
        n = int(rng.integers(1, 3))
        if x + n <= X and free(z, y, x, x + n - 1):
            small[z, y, x:x + n] = True
    return m | small


def brute_min_d2(mask, compsize):
    """per small component of scipy's labelling: the minimum integer squared distance to a big voxel"""
    labels, n = ndimage.label(mask, np.ones((3, 3, 3)))
    counts = np.bincount(labels.ravel(), minlength=n + 1)
    big_vox = np.argwhere((counts > compsize)[labels] & mask).astype(np.int64)
    out = {}
    for lbl in range(1, n + 1):
        if counts[lbl] <= compsize:
            vox = np.argwhere(labels == lbl).astype(np.int64)
            out[lbl] = int(((vox[:, None, :] - big_vox[None]) ** 2).sum(-1).min()) if len(big_vox) else None
    return out, int((counts[1:] > compsize).sum())


CASES = [
    # name, shape, input dtype, fg_threshold, remove_small_comps, max_distance_to_fg
    ("fg_f32_d2", (8, 12, 30), np.float32, 0.5, 20, 2),
    ("fg_f32_d2p5", (9, 14, 33), np.float32, 0.9, 20, 2.5),
    ("fg_u8_d3", (10, 13, 40), np.uint8, 127, 20, 3),
    ("fg_u8_else", (8, 12, 30), np.uint8, 100, 20, 0),
    ("fg_f32_longx", (6, 10, 70), np.float32, 0.5, 20, 3),
    ("fg_f32_d2_noinst", (12, 14, 21), np.float32, 0.3, 20, 2),
]


def main():
    ref = load_reference()
    os.makedirs(OUT, exist_ok=True)
    for k, (name, shape, dtype, thr, compsize, dist) in enumerate(CASES):
        T = smallest_square(dist) if dist > 0 else 0
        mask = build_case(shape, T, seed=100 + k)
        rng = np.random.default_rng(500 + k)
        if dtype == np.float32:
            pred = np.where(mask, rng.uniform(thr + 0.01, 1.0, shape), rng.uniform(0.0, thr, shape)).astype(np.float32)
        else:
            pred = np.where(mask, rng.integers(thr + 1, 256, shape), rng.integers(0, thr + 1, shape)).astype(np.uint8)
        assert np.array_equal(pred > thr, mask)
        kwargs = dict(fg_key="volumes/pred_fgbg", fg_threshold=thr, remove_small_comps=compsize,
                      max_distance_to_fg=dist, cc_instances=not name.endswith("noinst"), export_skeleton_nrrds=False)
        mind2, n_big = brute_min_d2(mask, compsize)
        if dist > 0:
            values = sorted(mind2.values())
            assert n_big >= 1, name
            assert any(v >= T for v in values), (name, "nothing is removed")
            lo, hi = around(T)
            assert hi in values, (name, T, values)
            if lo is not None:
                assert lo in values, (name, T, values)          # (and so one small component is kept)
            else:
                assert min(values) == T, (name, T, values)
        sample = name + ".zarr"
        STORE[sample] = {kwargs["fg_key"]: pred}
        with contextlib.redirect_stdout(io.StringIO()):        # (the reference prints its labels)
            ref.postprocess_fg([sample], "out", **kwargs)
        got = WRITTEN[os.path.join("out", name + ".hdf")]
        fg = got["volumes/fg"]
        assert fg.dtype == np.uint8 and (not kwargs["cc_instances"] or got["volumes/instances"].dtype == np.uint16)
        inst = got.get("volumes/instances", np.zeros((0,), np.uint16))
        np.savez_compressed(os.path.join(OUT, name + ".npz"), pred=pred, kwargs=json.dumps(kwargs), fg=fg,
                            instances=inst)
        print("%-18s %-12s T = %d  small min d2 = %s  fg %d -> %d voxels" % (
            name, shape, T, sorted(mind2.values()), int(mask.sum()), int(fg.sum())))


if __name__ == "__main__":
    main()
