#!/usr/bin/env python3
"""tests/golden/visualize/*.npz: the reference's own `visualize_patches` (reshape_affinities,
reshape_affinities_3d), `visualize_instances` and `util.postprocess.color`
(PatchPerPix/visualize/patches.py, visualize/instances.py, util/postprocess.py, imported in place) on small
inputs.  Stubs stand in for h5py (a dict of arrays behind `File`, which also records `create_dataset`), zarr,
skimage.io (a recorder that keeps the array handed to `imsave`), colorcet and nrrd.  Development container
only.

  python tests/golden/gen_golden_visualize.py

A file holds `input` (the array, or the dataset of the stubbed file), `selected` where the case has one,
`kwargs` (JSON: patchshape and the keyword arguments of the call) and `output`: what the call returned, the
dataset it created (`out_key` names it) or the array it handed to `imsave`.  The reference writes into its
input; every call gets a copy, and the stored input is the untouched one.  The archives are written with
fixed timestamps, so a second run gives the same bytes."""
import contextlib
import importlib.util
import io
import json
import os
import sys
import types
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "visualize")
REF = "/root/reference/PatchPerPix"

STORE = {}          # "file name" -> {key: array}: what the stubbed h5py.File hands out and records
SAVED = []          # (file name, array) of every skimage.io.imsave call


class FileStub:
    def __init__(self, fn, mode="r"):
        self.sets = STORE.setdefault(fn, {}) if mode != "r" else STORE[fn]

    def __getitem__(self, key):
        return self.sets[key]

    def create_dataset(self, key, data=None, compression=None, **kw):
        assert key not in self.sets and compression == "gzip"
        self.sets[key] = np.array(data)

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for name in ("colorcet", "skimage", "skimage.morphology", "skimage.io", "zarr", "h5py", "nrrd", "PatchPerPix",
                 "PatchPerPix.util"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["skimage.morphology"].skeletonize_3d = None
    sys.modules["skimage"].io = sys.modules["skimage.io"]
    sys.modules["skimage.io"].imsave = lambda fn, arr, **kw: SAVED.append((fn, np.array(arr)))
    sys.modules["h5py"].File = FileStub
    post = _load("ppp_ref_postprocess", os.path.join(REF, "util", "postprocess.py"))
    sys.modules["PatchPerPix.util"].color = post.color
    sys.modules["PatchPerPix.util"].relabel = post.relabel
    patches = _load("ppp_ref_visualize_patches", os.path.join(REF, "visualize", "patches.py"))
    instances = _load("ppp_ref_visualize_instances", os.path.join(REF, "visualize", "instances.py"))
    return patches, instances, post


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings(), np.errstate(invalid="ignore"):
        warnings.simplefilter("ignore")
        return fn(*args, **kwargs)


# ----------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------
def make_pred(rng, patch, spatial, dtype, logits=False):
    """values on a grid of eighths, so that several k hold the maximum; exact 0 and 1 among them"""
    C = int(np.prod(patch))
    a = rng.integers(0, 9, (C,) + tuple(spatial)) / 8.0
    if logits:
        a = (a - 0.5) * 12.0
    a = a.astype(dtype)
    if not logits:
        assert (a == 0).any() and (a == 1).any()
        pz = patch[0]
        if pz > 1:
            k = a.reshape((pz, -1) + tuple(spatial))
            top = k.max(axis=0)
            assert ((k == top).sum(axis=0) > 1).any(), "no tie among the k"
    return a


def save(name, **arrays):
    """np.savez_compressed with fixed timestamps: the same arrays give the same bytes"""
    path = os.path.join(OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)
    z = np.load(path)
    print("%-20s %7d bytes  %s" % (name, os.path.getsize(path), {k: z[k].shape for k in z.files if k != "kwargs"}))


def check_mine(name, inp, patchshape, kwargs, output, selected=None):
    """this project's host definition gives the same (the tests say it again, without the reference)"""
    os.environ["PPP_POSTPROCESS"] = "host"
    sys.path.insert(0, ROOT)
    from patchperpix_amd.visualize import patches as mine
    before = inp.copy()
    kw = dict(kwargs)
    if selected is not None:
        kw["selected"] = selected
    got = mine.visualize_patches(inp, patchshape, **kw)
    assert np.array_equal(before, inp, equal_nan=True), name
    assert got.dtype == output.dtype and got.shape == output.shape, (name, got.dtype, got.shape, output.dtype, output.shape)
    assert np.array_equal(got.view(np.uint8), output.view(np.uint8)), name


def array_case(ref, name, patchshape, inp, selected=None, **kwargs):
    """visualize_patches on an array, returning the mosaic"""
    kw = dict(kwargs)
    if selected is not None:
        STORE[name + "_sel.hdf"] = {"selected": selected}
        kw["selected"] = name + "_sel.hdf"
    out = quiet(ref.visualize_patches, inp.copy(), patchshape, **kw)
    check_mine(name, inp, patchshape, kwargs, out, selected)
    extra = {} if selected is None else {"selected": selected}
    save(name, input=inp, output=out, kwargs=json.dumps(dict(kwargs, patchshape=list(patchshape))), **extra)


def main():
    patches, instances, post = load_reference()
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20240607)

    array_case(patches, "m3d_p3_f16", (3, 3, 3), make_pred(rng, (3, 3, 3), (3, 5, 70), np.float16))
    array_case(patches, "m3d_p357_f32", (3, 5, 7), make_pred(rng, (3, 5, 7), (2, 4, 66), np.float32))
    chw = make_pred(rng, (1, 5, 5), (6, 70), np.float32)
    array_case(patches, "m2d_p5_chw", (1, 5, 5), chw)
    hwc = np.ascontiguousarray(np.moveaxis(make_pred(rng, (1, 5, 5), (6, 70), np.float16, logits=True), 0, -1))
    assert hwc.shape == (6, 70, 25) and hwc.min() < 0 and hwc.max() > 1
    array_case(patches, "m2d_p5_hwc_sigmoid", (1, 5, 5), hwc, sigmoid=True)
    sel1 = (rng.uniform(size=(1, 6, 70)) < 0.5).astype(np.uint8)
    array_case(patches, "m2d_p5_sel1", (1, 5, 5), chw, selected=sel1)
    sel3 = (rng.uniform(size=(3, 6, 70)) < 0.35).astype(np.uint8)
    flags = sel3.sum(axis=0)
    assert (flags == 0).any() and (flags > 1).any() and (sel3[0] == 0).any()
    array_case(patches, "m2d_p5_sel3", (1, 5, 5), chw, selected=sel3)
    array_case(patches, "m2d_p25", (1, 25, 25), make_pred(rng, (1, 25, 25), (3, 66), np.float16))
    # the NaN case, kept apart: NaN in one k of some voxels, in all k of others, and in channels with j == 0 / i == 0
    nan = make_pred(rng, (3, 3, 3), (2, 3, 9), np.float32)
    nan[rng.uniform(size=nan.shape) < 0.1] = np.nan
    nan[:, 1, 2, 4] = np.nan
    array_case(patches, "m3d_p3_nan", (3, 3, 3), nan)

    # threshold + store_int into an .hdf, default key
    inp = make_pred(rng, (3, 3, 3), (2, 4, 9), np.float16)
    STORE["thr.hdf"] = {"volumes/pred_affs": inp.copy()}
    kwargs = dict(in_key="volumes/pred_affs", threshold=0.5, store_int=True)
    assert quiet(patches.visualize_patches, "thr.hdf", (3, 3, 3), out_file="thr_out.hdf", **kwargs) == 0
    (out_key, out), = STORE["thr_out.hdf"].items()
    assert out_key == "volumes/pred_affs_patched" and out.dtype == np.uint8
    save("m3d_p3_thr_int", input=inp, output=out, out_key=out_key, kwargs=json.dumps(dict(kwargs, patchshape=[3, 3, 3])))

    # a .png target: the array handed to imsave
    assert quiet(patches.visualize_patches, chw.copy(), (1, 5, 5), out_file="m2d.png") == 0
    (fn, pix), = SAVED
    assert fn == "m2d.png" and pix.dtype == np.uint8 and pix.ndim == 2
    save("m2d_p5_png", input=chw, output=pix, kwargs=json.dumps(dict(patchshape=[1, 5, 5])))

    # visualize_instances: np.random.seed(7) before the call
    lab3 = np.zeros((4, 9, 11), dtype=np.uint16)
    for k, lbl in enumerate((3, 9, 300, 4, 17, 65000)):
        z, y, x = int(rng.integers(0, 4)), int(rng.integers(0, 6)), int(rng.integers(0, 8))
        lab3[z, y:y + 3, x:x + 4] = lbl
    lab2 = lab3.max(axis=0) * (rng.uniform(size=(9, 11)) < 0.8).astype(np.uint16)
    for name, lab, max_axis in (("inst_mip", lab3, 0), ("inst_2d", lab2, None)):
        STORE[name + ".hdf"] = {"vote_instances": lab.copy()}
        del SAVED[:]
        np.random.seed(7)
        quiet(instances.visualize_instances, name + ".hdf", "vote_instances", name + ".png", max_axis=max_axis)
        (fn, pix), = SAVED
        assert pix.dtype == np.uint8 and pix.shape == (9, 11, 3) and len(np.unique(lab)) > 3
        np.random.seed(7)
        flat = lab if max_axis is None else lab.max(axis=max_axis)
        assert np.array_equal(quiet(post.color, flat).astype(np.uint8), pix)
        save(name, input=lab, output=pix, kwargs=json.dumps(dict(max_axis=max_axis, seed=7)))


if __name__ == "__main__":
    main()
