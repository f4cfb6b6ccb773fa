"""`ppp_patch_mosaic` (csrc/ppp_mosaic.hip) against `visualize.patches.mosaic_host`, bit for bit, on the smallest
shapes at which the kernel can go wrong; every golden of the reference through the device path; chunk independence;
the refusals of the entry point."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from patchperpix_amd.visualize import patches, visualize_patches

pytestmark = pytest.mark.gpu

VIS_DIR = os.path.join(GOLDEN_DIR, "visualize")
SENTINEL = 7.0          # no input value and no 1: an element that still holds it was not written

# x lines of 1, 63, 64, 65, 70 and 130 voxels (several 64- and 128-voxel runs with ragged ends); Y X odd, with the
# channel stride tz Y X odd (3 slices: every other channel starts misaligned for 2-byte pairs) and even (2 slices)
SPATIAL = [(3, 1), (3, 63), (3, 64), (3, 65), (3, 70), (3, 130), (3, 5)]
# ((2, 4, 6): even sides -- the LDS tile then has a gap per voxel and the 16-byte store reads it element by element)
PATCHES = [(3, 3, 3), (5, 5, 5), (3, 5, 7), (1, 5, 5), (1, 25, 25), (1, 11, 11), (2, 4, 6)]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                                                                       np.ascontiguousarray(b).view(np.uint8))


def make_pred(rng, patch, vol):
    """eighths (exact in every element type, ties among the k), with exact 0 and 1"""
    return (rng.integers(0, 9, (int(np.prod(patch)),) + tuple(vol)) / 8.0).astype(np.float32)


def run_device(pred32, patch, dtype, sel=None):
    """the kernel on `pred32` cast to `dtype`, into a sentinel-filled buffer; returns (out as NumPy, its float32 form)"""
    import torch
    from patchperpix_amd import backend
    t = torch.from_numpy(pred32).cuda().to(dtype).contiguous()
    C, tz, Y, X = pred32.shape
    plane = (tz, Y * patch[1], X * patch[2])
    out = torch.full(plane if sel is None else (3,) + plane, SENTINEL, dtype=dtype, device="cuda")
    d_sel = None if sel is None else torch.from_numpy(sel).cuda()
    res = backend.patch_mosaic(t, patch, d_sel, out=out)
    torch.cuda.synchronize()
    assert res is out
    return out.float().cpu().numpy()


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("patch", PATCHES, ids=lambda p: "x".join(map(str, p)))
def test_mosaic_equals_host(patch, dtype):
    import torch
    rng = np.random.default_rng(sum(patch))
    np_dtype = np.float16 if dtype == "float16" else np.float32        # (bfloat16: the float32 form of the same values)
    for yx in SPATIAL:
        for tz in ((2, 3) if yx == (3, 5) else (2,)) if patch[0] > 1 else (1,):
            pred = make_pred(rng, patch, (tz,) + yx)
            want = patches.mosaic_host(pred.astype(np_dtype), patch).astype(np.float32)
            got = run_device(pred, patch, getattr(torch, dtype))
            assert not (got == SENTINEL).any(), (yx, tz, "elements left unwritten")
            assert same_bits(got, want), (yx, tz)


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("S", [1, 3])
def test_mosaic_selected(S, dtype):
    import torch
    rng = np.random.default_rng(S)
    patch = (1, 5, 5)
    for yx in [(3, 65), (3, 5), (2, 130)]:
        pred = make_pred(rng, patch, (1,) + yx)
        sel = (rng.uniform(size=(S, 1) + yx) < 0.4).astype(np.uint8)
        if S == 3:
            flags = sel.sum(axis=0)
            assert (flags == 0).any() and (flags > 1).any()
        np_dtype = np.float16 if dtype == "float16" else np.float32
        want = patches.mosaic_host(pred.astype(np_dtype), patch, sel).astype(np.float32)
        got = run_device(pred, patch, getattr(torch, dtype), sel)
        assert not (got == SENTINEL).any(), "elements left unwritten (the zeros of dropped tiles are the kernel's)"
        assert same_bits(got, want), yx


def load(name):
    z = np.load(os.path.join(VIS_DIR, name + ".npz"))
    kw = json.loads(str(z["kwargs"]))
    return z, kw.pop("patchshape", None), kw


@pytest.mark.parametrize("name", ["m3d_p3_f16", "m3d_p357_f32", "m2d_p5_chw", "m2d_p5_hwc_sigmoid", "m2d_p5_sel1",
                                  "m2d_p5_sel3", "m2d_p25", "m3d_p3_nan"])
def test_goldens_through_the_device(name, monkeypatch):
    import torch
    from patchperpix_amd import backend
    monkeypatch.delenv("PPP_POSTPROCESS", raising=False)
    calls = []
    real = backend.patch_mosaic
    monkeypatch.setattr(backend, "patch_mosaic", lambda *a, **k: calls.append(1) or real(*a, **k))
    z, patchshape, kw = load(name)
    if "selected" in z.files:
        kw["selected"] = z["selected"]
    inp = z["input"].copy()
    got = visualize_patches(inp, patchshape, **kw)
    assert same_bits(got, z["output"]) and same_bits(inp, z["input"])
    if name == "m2d_p5_hwc_sigmoid":
        # scipy.special.expit makes float64 of the float16 logits: no element type of the kernel, the host's
        assert got.dtype == np.float64 and not calls
    else:
        assert calls, "the device path was not taken"
        # a device tensor in, a device tensor out
        t = visualize_patches(torch.from_numpy(z["input"].copy()).cuda(), patchshape, **kw)
        assert t.is_cuda and same_bits(t.cpu().numpy(), z["output"])


def test_golden_files_through_the_device(tmp_path, monkeypatch):
    from patchperpix_amd import minihdf5, minipng
    monkeypatch.delenv("PPP_POSTPROCESS", raising=False)
    z, patchshape, kw = load("m3d_p3_thr_int")
    src = str(tmp_path / "thr.hdf")
    with minihdf5.File(src, "w") as f:
        f.create_dataset(kw["in_key"], data=z["input"])
    out = str(tmp_path / "thr_out.hdf")
    assert visualize_patches(src, patchshape, out_file=out, **kw) == 0
    with minihdf5.File(out, "r") as f:
        assert same_bits(np.asarray(f[str(z["out_key"])]), z["output"])
    z, patchshape, kw = load("m2d_p5_png")
    fn = str(tmp_path / "m.png")
    assert visualize_patches(z["input"].copy(), patchshape, out_file=fn) == 0
    assert np.array_equal(minipng.read(fn), z["output"])


def test_chunk_independence():
    rng = np.random.default_rng(5)
    patch = (3, 5, 7)
    pred = make_pred(rng, patch, (5, 3, 65)).astype(np.float16)
    want = patches.mosaic_host(pred, patch)
    for tz in (1, 2, 5, None):
        got = patches.mosaic_device(lambda z, n: pred[:, z:z + n], pred.shape, pred.dtype, patch, tz=tz)
        assert same_bits(got, want), tz


def test_nan_propagates():
    import torch
    rng = np.random.default_rng(9)
    patch = (3, 3, 3)
    pred = make_pred(rng, patch, (2, 3, 65))
    pred[rng.uniform(size=pred.shape) < 0.1] = np.nan        # in one k, in several, first, last
    pred[:, 0, 1, 7] = np.nan
    for dtype, np_dtype in ((torch.float32, np.float32), (torch.float16, np.float16), (torch.bfloat16, np.float32)):
        want = patches.mosaic_host(pred.astype(np_dtype), patch).astype(np.float32)
        got = run_device(pred, patch, dtype)
        assert np.isnan(want).any() and np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(got, want, equal_nan=True)
    # float32: the bits too (one quiet NaN pattern in, the same out)
    assert same_bits(run_device(pred, patch, torch.float32), patches.mosaic_host(pred, patch))


def test_refusals_by_the_sizes_alone():
    """no pointer is looked at before the sizes are, and nothing is launched: the calls pass NULL"""
    from patchperpix_amd import backend
    L = backend.lib()

    def call(C, S, tz, Y, X, patch, dtype=backend.F16):
        return L.ppp_patch_mosaic(None, dtype, C, None, S, None, tz, Y, X, (ctypes.c_int32 * 3)(*patch), None)
    INVALID, UNSUPPORTED = -1, -4
    assert call(26, 0, 1, 4, 4, (3, 3, 3)) == INVALID                       # C != pz py px
    assert call(25, 2, 1, 4, 4, (1, 5, 5)) == INVALID                       # S not in {0, 1, 3}
    assert call(27, 1, 1, 4, 4, (3, 3, 3)) == INVALID                       # selected with pz > 1
    assert call(27, 0, 0, 4, 4, (3, 3, 3)) == INVALID
    assert call(0, 0, 1, 4, 4, (3, 0, 3)) == INVALID
    assert call(27, 0, 1, 4, 4, (3, 3, 3), dtype=99) == INVALID
    assert call(27, 0, 1 << 15, 1 << 15, 2, (3, 3, 3)) == UNSUPPORTED       # 2^31 voxels
    assert b"2^31" in L.ppp_last_error()
    assert call(64 * 64, 0, 1, 4, 4, (1, 64, 64)) == UNSUPPORTED            # px beyond the LDS tile
    assert call(9 * (1 << 20), 0, 1, 4, 1 << 11, (1, 9, 1 << 20)) == UNSUPPORTED     # X px = 2^31
    assert call(27, 0, 1, 4, 4, (3, 3, 3)) == INVALID and b"pointer" in L.ppp_last_error()   # sizes fine: the NULLs


def test_label_task_with_save_mip(tmp_path):
    """`--do label` with the flags of the shipped flylight default.toml and its `[visualize] save_mip = true`: the
    coloured projection of the instance map lies beside the result file, before and after remove_small_comps."""
    from patchperpix_amd import minihdf5, minipng, minizarr, run_ppp, synth
    ps = (5, 5, 5)
    c = synth.make_case((14, 18, 22), ps, seed=73, cell=[7, 7, 7], overlap_frac=0.03)
    numinst = c["numinst"]
    prob = np.zeros((3,) + numinst.shape, dtype=np.float16)     # channel k = P(k instances)
    prob[0][numinst == 0] = 0.97
    prob[1][numinst == 1] = 0.95
    prob[2][numinst == 2] = 0.6
    pred_dir, out_dir = tmp_path / "pred", tmp_path / "inst"
    zf = minizarr.open(str(pred_dir / "sampleZ.zarr"), "w")
    zf.create_dataset("volumes/pred_affs", data=c["pred"].astype(np.float16), chunks=(125, 10, 10, 10))
    zf.create_dataset("volumes/pred_numinst", data=prob, chunks=(3, 10, 10, 10))
    extra = tmp_path / "mip.toml"
    extra.write_text("[visualize]\nsave_mip = true\n[vote_instances]\nremove_small_comps = 2\n")
    run_ppp.main(["--config", os.path.join(GOLDEN_DIR, "label_config_flylight_zarr.toml"), "--config", str(extra),
                  "--do", "label", "--pred-folder", str(pred_dir), "--output-folder", str(out_dir)])
    assert sorted(os.listdir(str(out_dir))) == ["sampleZ.hdf", "sampleZ.png", "sampleZ_cleaned.png"]
    with minihdf5.File(str(out_dir / "sampleZ.hdf"), "r") as f:
        inst = np.asarray(f["vote_instances"])
    assert inst.max() > 1
    mip = np.max(inst, axis=0)
    cleaned = minipng.read(str(out_dir / "sampleZ_cleaned.png"))
    assert cleaned.shape == mip.shape + (3,) and np.array_equal(cleaned.any(axis=-1), mip != 0)
    for lbl in np.unique(mip)[1:]:
        assert len(np.unique(cleaned[mip == lbl], axis=0)) == 1
    before = minipng.read(str(out_dir / "sampleZ.png"))
    assert not (before.any(axis=-1) < cleaned.any(axis=-1)).any()      # removal only takes pixels away
