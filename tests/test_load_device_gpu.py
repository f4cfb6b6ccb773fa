"""GPU: the `label` task with ``load_on_device`` -- the prediction loaded by minizarr.Array.read_device (codec on
host threads, un-shuffle, logits test and scatter on the device) -- against the same run with the host load: equal
result files, no read of ``volumes/pred_affs`` through the host reader (minizarr.Array._read), for stored
probabilities and logits, crops, a foreground from the centre channel and 2-d data; tiling.ZarrProvider with
``device_decode``; and the containers the device path does not serve, through the host fallback."""
import argparse
import copy
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from patchperpix_amd import minihdf5, minizarr, run_ppp, synth, tiling
from test_cli_gpu import _load_result
from test_validate_gpu import MARGIN, PS, SHAPE, SPECK, make_sample

pytestmark = pytest.mark.gpu

BASE = os.path.join(GOLDEN_DIR, "label_config_flylight_zarr.toml")
CHUNKS = (PS[0] * PS[1] * PS[2], 12, 12, 13)        # 2 x 2 x 2 chunks, clipped at the upper edges
SHAPE_2D, PS_2D = (1, 40, 44), (1, 5, 5)


def logit16(p):
    p = np.clip(p.astype(np.float64), 1e-3, 1 - 1e-3)
    return np.log(p / (1 - p)).astype(np.float16)


def sample_2d(seed):
    c = synth.make_case(SHAPE_2D, PS_2D, seed=seed, cell=[1, 9, 9])
    lab = np.zeros(SHAPE_2D, dtype=np.int64)
    inner = (slice(None), slice(MARGIN, SHAPE_2D[1] - MARGIN), slice(MARGIN, SHAPE_2D[2] - MARGIN))
    lab[inner] = c["labels"][inner]
    pred16 = synth.pred_from_labels(lab, PS_2D, seed=seed).astype(np.float16)
    prob = np.zeros((3,) + SHAPE_2D, dtype=np.float16)
    prob[0][lab == 0] = 0.97
    prob[1][lab != 0] = 0.95
    return pred16[:, 0], prob[:, 0]                 # the 2-d convention: (C, Y, X), (K, Y, X)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    root = tmp_path_factory.mktemp("load_device")
    lab, pred16, prob = make_sample(91)
    assert pred16.dtype == np.float16 and pred16.shape == (CHUNKS[0],) + SHAPE

    def write(folder, name, affs, numinst, chunks, compressor="default"):
        zf = minizarr.open(str(root / folder / (name + ".zarr")), "w")
        zf.create_dataset("volumes/pred_affs", data=affs, chunks=chunks, compressor=compressor)
        zf.create_dataset("volumes/pred_numinst", data=numinst, chunks=(3,) + tuple(chunks[1:]))
    # float16, Blosc-zstd with bit shuffle (the writer's default = the prediction step's compressor), 8 chunks
    write("pred", "vol", pred16, prob, CHUNKS)
    write("pred", "logit", logit16(pred16), prob, CHUNKS)
    assert logit16(pred16).min() < 0 and logit16(pred16).max() > 1
    flat_affs, flat_prob = sample_2d(92)
    write("pred2d", "flat", flat_affs, flat_prob, (PS_2D[1] * PS_2D[2], 20, 22))
    # what the device path does not serve: channels last, and an HDF5 container
    zf = minizarr.open(str(root / "last" / "vol.zarr"), "w")
    zf.create_dataset("volumes/pred_affs", data=np.ascontiguousarray(np.moveaxis(pred16, 0, -1)), chunks=CHUNKS[1:] + CHUNKS[:1])
    zf.create_dataset("volumes/pred_numinst", data=prob, chunks=(3,) + CHUNKS[1:])
    os.makedirs(str(root / "hdf"))
    with minihdf5.File(str(root / "hdf" / "vol.hdf"), "w") as f:
        f.create_dataset("volumes/pred_affs", data=pred16, compression="gzip")
        f.create_dataset("volumes/pred_numinst", data=prob, compression="gzip")
    config = run_ppp.load_config([BASE])
    config["vote_instances"].update(only_bb=True, ignore_small_comps=SPECK, skeletonize_foreground=False)
    return dict(root=root, config=config)


def label(world, folder, out, on, sample=None, patchshape=None, fmt="zarr", drop_numinst=False, **vote):
    """one `label` run; returns the number of reads of ``volumes/pred_affs`` that reached the host reader"""
    config = copy.deepcopy(world["config"])
    config["vote_instances"].update(vote, load_on_device=on)
    config["prediction"]["output_format"] = fmt
    if patchshape is not None:
        config["model"]["patchshape"] = list(patchshape)
    if drop_numinst:
        del config["prediction"]["numinst_key"]
    reads = []
    real = minizarr.Array._read

    def counted(arr, ranges, out_):
        if arr.path.rstrip("/").endswith("pred_affs"):
            reads.append(ranges)
        return real(arr, ranges, out_)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PPP_ZARR", "mini")
        mp.delenv("PPP_LOAD_DEVICE", raising=False)
        mp.delenv("PPP_STREAM_PRED", raising=False)
        mp.setattr(minizarr.Array, "_read", counted)
        run_ppp.label(argparse.Namespace(pred_folder=str(world["root"] / folder), output_folder=str(out), sample=sample,
                                         checkpoint=None), config)
    return len(reads)


def same_results(a_folder, b_folder, name):
    a, b = _load_result(str(a_folder), name), _load_result(str(b_folder), name)
    assert set(a) == set(b) and "vote_instances" in a
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (name, k)
    return a


CASES = {
    "probabilities": dict(folder="pred", sample="vol"),
    "logits": dict(folder="pred", sample="logit"),
    "crops": dict(folder="pred", sample="vol", crop_z_s=2, crop_y_e=SHAPE[1] - 1),
    "centre-channel": dict(folder="pred", sample="vol", drop_numinst=True),
    "centre-channel-logits": dict(folder="pred", sample="logit", drop_numinst=True),
    "2d": dict(folder="pred2d", sample="flat", patchshape=PS_2D),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_label_on_device_equals_host_load(world, tmp_path, case):
    kw = dict(CASES[case])
    name = kw["sample"]
    host_reads = label(world, out=tmp_path / "host", on=False, **kw)
    dev_reads = label(world, out=tmp_path / "dev", on=True, **kw)
    res = same_results(tmp_path / "host", tmp_path / "dev", name)
    assert res["vote_instances"].max() > 1
    # host: the array, and once more for the centre channel; device: never through the host reader
    assert host_reads == (2 if kw.get("drop_numinst") else 1) and dev_reads == 0


def test_environment_switch_overrides_the_option(world, tmp_path, monkeypatch):
    real, calls = minizarr.Array.read_device, []
    monkeypatch.setattr(minizarr.Array, "read_device", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    for env, on, want in (("1", False, 1), ("0", True, 0)):
        del calls[:]
        config = copy.deepcopy(world["config"])
        config["vote_instances"]["load_on_device"] = on
        monkeypatch.setenv("PPP_ZARR", "mini")
        monkeypatch.setenv("PPP_LOAD_DEVICE", env)
        run_ppp.label(argparse.Namespace(pred_folder=str(world["root"] / "pred"), output_folder=str(tmp_path / env), sample="vol",
                                         checkpoint=None), config)
        assert len(calls) == want
    same_results(tmp_path / "0", tmp_path / "1", "vol")


@pytest.mark.parametrize("folder,fmt", [("hdf", "hdf"), ("last", "zarr")], ids=["hdf", "channels-last"])
def test_unserved_containers_fall_back_to_the_host_load(world, tmp_path, folder, fmt):
    label(world, folder, tmp_path / "off", on=False, sample="vol", fmt=fmt)
    reads = label(world, folder, tmp_path / "on", on=True, sample="vol", fmt=fmt)
    same_results(tmp_path / "off", tmp_path / "on", "vol")
    assert reads == (1 if fmt == "zarr" else 0)
    # and the same instances as the channels-first zarr store of the same values
    label(world, "pred", tmp_path / "first", on=True, sample="vol")
    assert np.array_equal(_load_result(str(tmp_path / "on"), "vol")["vote_instances"],
                          _load_result(str(tmp_path / "first"), "vol")["vote_instances"])


@pytest.mark.parametrize("expit", [False, True], ids=["as-stored", "expit"])
def test_zarr_provider_device_decode(world, expit):
    import torch
    arr = minizarr.open(str(world["root"] / "pred" / ("logit.zarr" if expit else "vol.zarr")), "r")["volumes/pred_affs"]
    boxes = [(0, 22, 0, 24, 0, 26), (3, 15, 2, 13, 5, 26), (11, 13, 12, 24, 0, 13), (12, 22, 11, 14, 12, 14)]
    base = tiling.ZarrProvider(arr, expit=expit)
    dev = tiling.ZarrProvider(arr, expit=expit, device_decode=True)
    assert dev.device_decode and not base.device_decode
    want = [base.pred_box(b).cpu().numpy() for b in boxes]
    # on demand
    for b, w in zip(boxes, want):
        t = dev.pred_box(b)
        assert t.is_cuda and t.dtype == (torch.float32 if expit else torch.float16) and t.is_contiguous()
        assert w.dtype == t.cpu().numpy().dtype and w.tobytes() == t.cpu().numpy().tobytes()
    # with the next box decoded ahead on the worker thread
    dev.prefetch(boxes[0])
    for i, (b, w) in enumerate(zip(boxes, want)):
        t = dev.pred_box(b)
        dev.prefetch(boxes[i + 1] if i + 1 < len(boxes) else None)
        assert w.tobytes() == t.cpu().numpy().tobytes()
    assert dev.boxes_prefetched == len(boxes) and dev.boxes_uploaded_ahead == len(boxes)
    assert dev.bytes_read == 2 * sum(w.size * 2 for w in want)
    assert dev._pinned == [None, None]              # no host image of a box was ever made
