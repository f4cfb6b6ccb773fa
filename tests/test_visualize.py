"""The `visualize` task on the host: `mosaic_host` and the public functions under PPP_POSTPROCESS=host against
goldens of the reference's own functions (tests/golden/gen_golden_visualize.py), `postprocess.color`'s draw
sequence, the PNG writer, the container round trips, `save_mip` in the label drivers and `--do visualize`."""
import glob
import json
import os
import struct
import zlib

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from patchperpix_amd import minihdf5, minipng, minizarr, postprocess
from patchperpix_amd.visualize import patches, visualize_instances, visualize_patches

VIS_DIR = os.path.join(GOLDEN_DIR, "visualize")
MOSAICS = ["m3d_p3_f16", "m3d_p357_f32", "m2d_p5_chw", "m2d_p5_hwc_sigmoid", "m2d_p5_sel1", "m2d_p5_sel3", "m2d_p25",
           "m3d_p3_nan"]

needs_hdf5 = pytest.mark.skipif(not minihdf5.available(), reason="no HDF5 C library")


def load(name):
    z = np.load(os.path.join(VIS_DIR, name + ".npz"))
    kw = json.loads(str(z["kwargs"]))
    return z, kw.pop("patchshape", None), kw


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                                                                       np.ascontiguousarray(b).view(np.uint8))


@pytest.fixture(autouse=True)
def _host(monkeypatch):
    monkeypatch.setenv("PPP_POSTPROCESS", "host")


def test_every_golden_is_listed():
    have = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(VIS_DIR, "*.npz")))
    assert have == sorted(MOSAICS + ["m3d_p3_thr_int", "m2d_p5_png", "inst_mip", "inst_2d"])


@pytest.mark.parametrize("name", MOSAICS)
def test_visualize_patches_equals_reference(name):
    z, patchshape, kw = load(name)
    inp = z["input"].copy()
    if "selected" in z.files:
        kw["selected"] = z["selected"]
    got = visualize_patches(inp, patchshape, **kw)
    assert same_bits(got, z["output"])
    assert same_bits(inp, z["input"]), "the input was written to"


@pytest.mark.parametrize("name", ["m3d_p3_f16", "m3d_p357_f32", "m2d_p5_chw", "m2d_p5_sel1", "m2d_p5_sel3", "m2d_p25",
                                  "m3d_p3_nan"])
def test_mosaic_host_equals_reference(name):
    z, patchshape, kw = load(name)
    inp = z["input"]
    two_d = inp.ndim == 3
    arr4 = inp[:, None] if two_d else inp
    sel = z["selected"][:, None] if "selected" in z.files else None
    got = patches.mosaic_host(arr4, patchshape, sel)
    want = z["output"]
    if two_d:
        want = want.reshape((1,) + want.shape[1:]) if sel is None else want[:, None]
    assert same_bits(got, want)
    if name == "m3d_p3_nan":
        assert np.isnan(want).any() and (want == 1).sum() >= want.size // 9 * 5      # row 0 / column 0 stay 1


def test_reshape_functions_and_refusals():
    z, patchshape, _ = load("m2d_p5_chw")
    assert same_bits(patches.reshape_affinities(z["input"], [5, 5]), z["output"])
    z3, ps3, _ = load("m3d_p357_f32")
    assert same_bits(patches.reshape_affinities_3d(z3["input"], ps3), z3["output"])
    with pytest.raises(NotImplementedError):
        patches.reshape_affinities(z3["input"], ps3)
    with pytest.raises(NotImplementedError):
        patches.reshape_affinities_3d(z["input"], patchshape)
    with pytest.raises(NotImplementedError, match="tif"):
        visualize_patches(z["input"], patchshape, out_file="x.tif")
    with pytest.raises(NotImplementedError, match="nrrd"):
        visualize_patches(z["input"], patchshape, out_file="x.nrrd")
    with pytest.raises(NotImplementedError):
        visualize_patches("pred.npy", patchshape, in_key="k")
    with pytest.raises(ValueError):
        patches.mosaic_host(z["input"][:, None], (1, 5, 4))


# ---------------------------------------------------------------------------------------- colouring
@pytest.mark.parametrize("name", ["inst_mip", "inst_2d"])
def test_color_draw_sequence(name):
    z, _, kw = load(name)
    lab = z["input"] if kw["max_axis"] is None else np.max(z["input"], axis=kw["max_axis"])
    np.random.seed(kw["seed"])
    got = postprocess.color(lab)
    assert got.dtype == lab.dtype and got.shape == lab.shape + (3,)
    assert np.array_equal(got.astype(np.uint8), z["output"])
    assert not got[lab == 0].any()
    for lbl in np.unique(lab):
        assert len(np.unique(got[lab == lbl], axis=0)) == 1
    # one draw per non-zero label, in ascending order
    np.random.seed(kw["seed"])
    for lbl in np.unique(lab)[1:]:
        assert np.array_equal(got[lab == lbl][0], np.random.randint(0, 255, 3).astype(lab.dtype))


def test_color_refuses_glasbey():
    with pytest.raises(NotImplementedError, match="colorcet"):
        postprocess.color(np.ones((2, 2), dtype=np.uint8), colormap="glasbey")


# ---------------------------------------------------------------------------------------- minipng
@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (5, 7, 3), (1, 1, 3), (33, 130)])
def test_minipng_round_trip(shape, tmp_path):
    a = np.random.default_rng(1).integers(0, 256, shape).astype(np.uint8)
    fn = str(tmp_path / "a.png")
    minipng.write(fn, a)
    assert np.array_equal(minipng.read(fn), a)
    raw = open(fn, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n" and raw[12:16] == b"IHDR" and raw[-8:-4] == b"IEND"
    assert raw.count(b"IDAT") == 1
    w, h, depth, ctype, comp, flt, inter = struct.unpack(">IIBBBBB", raw[16:29])
    assert (w, h, depth, ctype, comp, flt, inter) == (shape[1], shape[0], 8, 0 if len(shape) == 2 else 2, 0, 0, 0)
    assert struct.unpack(">I", raw[29:33])[0] == zlib.crc32(raw[12:29]) & 0xFFFFFFFF
    PIL = pytest.importorskip("PIL.Image")
    assert np.array_equal(np.asarray(PIL.open(fn)), a)


def test_minipng_refuses(tmp_path):
    fn = str(tmp_path / "a.png")
    minipng.write(fn, np.arange(12, dtype=np.uint8).reshape(3, 4))
    raw = bytearray(open(fn, "rb").read())
    raw[-13] ^= 0x40                                   # a byte of the IDAT chunk's CRC
    open(fn, "wb").write(bytes(raw))
    with pytest.raises(ValueError, match="CRC"):
        minipng.read(fn)
    with pytest.raises(TypeError):
        minipng.write(fn, np.zeros((3, 4), dtype=np.uint16))
    with pytest.raises(ValueError):
        minipng.write(fn, np.zeros((3, 4, 2), dtype=np.uint8))


# ---------------------------------------------------------------------------------------- containers
@needs_hdf5
def test_zarr_to_hdf_list_keys(tmp_path):
    z, patchshape, _ = load("m3d_p3_f16")
    z2, _, _ = load("m3d_p3_nan")
    src = str(tmp_path / "s.zarr")
    g = minizarr.open(src, "w")
    g.create_dataset("volumes/pred_affs", data=z["input"], chunks=(27, 2, 4, 32))
    g.create_dataset("volumes/other", data=z2["input"][None], chunks=(1, 27, 2, 3, 9))       # a unit axis
    out = str(tmp_path / "o.hdf")
    assert visualize_patches(src, patchshape, in_key=["volumes/pred_affs", "volumes/other"], out_file=out) == 0
    with minihdf5.File(out, "r") as f:
        a = np.asarray(f["volumes/pred_affs_patched"])
        b = np.asarray(f["volumes/other_patched"])
    assert same_bits(a, z["output"].astype(np.float32))        # float16 -> float32 for an .hdf
    assert same_bits(b, z2["output"])
    out2 = str(tmp_path / "o2.hdf")
    visualize_patches(src, patchshape, in_key=["volumes/pred_affs", "volumes/other"], out_file=out2, out_key=["a", "b"])
    with minihdf5.File(out2, "r") as f:
        assert sorted(f.keys()) == ["a", "b"] and same_bits(np.asarray(f["b"]), z2["output"])
    assert same_bits(visualize_patches(src, patchshape, in_key="volumes/pred_affs"), z["output"])


@needs_hdf5
def test_threshold_store_int_hdf(tmp_path):
    z, patchshape, kw = load("m3d_p3_thr_int")
    src = str(tmp_path / "thr.hdf")
    with minihdf5.File(src, "w") as f:
        f.create_dataset(kw["in_key"], data=z["input"])
    out = str(tmp_path / "thr_out.hdf")
    assert visualize_patches(src, patchshape, out_file=out, **kw) == 0
    with minihdf5.File(out, "r") as f:
        assert list(f["volumes"].keys()) == ["pred_affs_patched"] and str(z["out_key"]) == "volumes/pred_affs_patched"
        assert same_bits(np.asarray(f[str(z["out_key"])]), z["output"])


def test_png_target(tmp_path):
    z, patchshape, kw = load("m2d_p5_png")
    fn = str(tmp_path / "m.png")
    assert visualize_patches(z["input"].copy(), patchshape, out_file=fn) == 0
    assert np.array_equal(minipng.read(fn), z["output"])
    zs, _, _ = load("m2d_p5_sel3")
    visualize_patches(zs["input"].copy(), patchshape, out_file=fn, selected=zs["selected"])
    assert np.array_equal(minipng.read(fn), np.moveaxis((zs["output"] * 255).astype(np.uint8), 0, -1))
    z3, ps3, _ = load("m3d_p3_f16")
    with pytest.raises(ValueError, match="picture"):
        visualize_patches(z3["input"], ps3, out_file=fn)


@needs_hdf5
@pytest.mark.parametrize("name", ["inst_mip", "inst_2d"])
def test_visualize_instances(name, tmp_path):
    z, _, kw = load(name)
    src = str(tmp_path / (name + ".hdf"))
    with minihdf5.File(src, "w") as f:
        f.create_dataset("vote_instances", data=z["input"][None] if name == "inst_2d" else z["input"])
    fn = str(tmp_path / "i.png")
    np.random.seed(kw["seed"])
    visualize_instances(src, "vote_instances", fn, max_axis=kw["max_axis"])
    assert np.array_equal(minipng.read(fn), z["output"])
    with pytest.raises(NotImplementedError, match="colorcet"):
        visualize_instances(src, "vote_instances", fn, show_outline=True)
    if name == "inst_mip":
        with pytest.raises(ValueError):
            visualize_instances(src, "vote_instances", fn)


# ---------------------------------------------------------------------------------------- save_mip
def _label_run(tmp_path, monkeypatch, sub, **extra):
    """the reference-semantics blockwise driver behind stitch_patch_graph.main, served by the oracle stand-ins of
    tests/test_blockwise.py, on its smallest golden"""
    import test_blockwise as tb
    from patchperpix_amd import blockwise
    from patchperpix_amd.vote_instances import stitch_patch_graph as spg
    z, kw = tb.load("bw_p3_cc_overlap")
    pred_file = str(tmp_path / "sample.zarr")
    if not os.path.exists(pred_file):
        g = minizarr.open(pred_file, "w")
        g.create_dataset("volumes/pred_affs", data=z["pred_f16"], chunks=(z["pred_f16"].shape[0], 8, 8, 8))
    monkeypatch.setattr(blockwise, "_do_block", tb.oracle_do_block)
    monkeypatch.setattr(blockwise, "label_graph", tb.cpu_label_graph)
    out_dir = str(tmp_path / sub)
    kw.pop("save_mip", None)
    kw = dict(kw, **extra)
    inst = spg.main(pred_file, result_folder=out_dir, blockwise_semantics="reference", **kw)
    return inst, out_dir


@needs_hdf5
def test_save_mip(tmp_path, monkeypatch):
    plain, d0 = _label_run(tmp_path, monkeypatch, "plain")
    inst, d1 = _label_run(tmp_path, monkeypatch, "mip", save_mip=True)
    assert sorted(os.listdir(d0)) == ["sample.hdf", "sample.zarr"]
    assert sorted(os.listdir(d1)) == ["sample.hdf", "sample.png", "sample.zarr"]
    assert np.array_equal(plain, inst) and inst.max() > 0
    pic = minipng.read(os.path.join(d1, "sample.png"))
    mip = np.max(inst, axis=0)
    assert pic.shape == mip.shape + (3,)
    # randint(0, 255, 3) gives (0, 0, 0) with probability 255^-3 per label: the zero pixels are the MIP's zeros
    assert np.array_equal(pic.any(axis=-1), mip != 0)
    for lbl in np.unique(mip)[1:]:
        assert len(np.unique(pic[mip == lbl], axis=0)) == 1
    cleaned, d2 = _label_run(tmp_path, monkeypatch, "cleaned", save_mip=True, remove_small_comps=3)
    assert sorted(os.listdir(d2)) == ["sample.hdf", "sample.png", "sample.zarr", "sample_cleaned.png"]
    assert np.array_equal(minipng.read(os.path.join(d2, "sample.png")).any(axis=-1), mip != 0)        # BEFORE the removal
    assert np.array_equal(minipng.read(os.path.join(d2, "sample_cleaned.png")).any(axis=-1), np.max(cleaned, axis=0) != 0)
    _, d3 = _label_run(tmp_path, monkeypatch, "off", save_mip=False, remove_small_comps=3)
    assert sorted(os.listdir(d3)) == ["sample.hdf", "sample.zarr"]


def test_post_steps_save_mip_needs_a_stem():
    inst = np.zeros((2, 3, 3), dtype=np.uint32)
    with pytest.raises(ValueError, match="mip_stem"):
        postprocess.post_steps(inst, inst != 0, "vote_instances", save_mip=True)
    postprocess.post_steps(inst, inst != 0, "vote_instances")


# ---------------------------------------------------------------------------------------- the CLI
@needs_hdf5
def test_cli_visualize(tmp_path):
    from patchperpix_amd import run_ppp
    z, patchshape, _ = load("m3d_p3_f16")
    zi, _, _ = load("inst_mip")
    pred, out = tmp_path / "pred", tmp_path / "out"
    pred.mkdir(), out.mkdir()
    for s in ("a", "b", "c"):
        g = minizarr.open(str(pred / (s + ".zarr")), "w")
        g.create_dataset("volumes/pred_affs", data=z["input"], chunks=(27, 3, 5, 70))
        with minihdf5.File(str(out / (s + ".hdf")), "w") as f:
            f.create_dataset("vote_instances", data=zi["input"])
    (pred / "b.hdf").write_bytes(b"kept")
    (out / "b.png").write_bytes(b"kept")
    cfg = tmp_path / "c.toml"
    cfg.write_text('[model]\npatchshape = [3, 3, 3]\n[prediction]\noutput_format = "zarr"\n'
                   '[vote_instances]\noutput_format = "hdf"\none_instance_per_channel = true\n'
                   '[visualize]\nshow_patches = true\nshow_instances = true\nsamples_to_visualize = ["a", "b", "missing"]\n')
    run_ppp.main(["-c", str(cfg), "--do", "visualize", "--pred-folder", str(pred), "--output-folder", str(out)])
    assert sorted(os.listdir(pred)) == ["a.hdf", "a.zarr", "b.hdf", "b.zarr", "c.zarr"]
    assert sorted(os.listdir(out)) == ["a.hdf", "a.png", "b.hdf", "b.png", "c.hdf"]
    assert (pred / "b.hdf").read_bytes() == b"kept" and (out / "b.png").read_bytes() == b"kept"
    with minihdf5.File(str(pred / "a.hdf"), "r") as f:
        assert same_bits(np.asarray(f["volumes/pred_affs_patched"]), z["output"].astype(np.float32))
    pic = minipng.read(str(out / "a.png"))
    assert np.array_equal(pic.any(axis=-1), np.max(zi["input"], axis=0) != 0)
