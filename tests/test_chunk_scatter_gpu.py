"""ppp_chunk_scatter and Array.read_device("cuda") against the host reader Array.__getitem__ and against the
flags of minizarr.chunk_scatter_host: the table of tests/test_chunk_scatter.py on the device, one chunk with
full waves and full Blosc blocks, the unserved element size, and the upload counter."""
import itertools
import os

import numpy as np
import pytest

from patchperpix_amd import backend, minizarr as mz

from test_chunk_scatter import (CHUNKS, FLAG_CASES, SELECTIONS, blosc, same_bits, scatter_all, store,
                                unsqueezed, values)

pytestmark = pytest.mark.gpu


def device_scatter_all(arr, sel, flags=False):
    """ppp_chunk_scatter over every chunk of `arr`, called directly"""
    import torch
    ranges, _ = arr._normalise(sel)
    tdt = torch.from_numpy(np.empty(0, dtype=arr.dtype)).dtype
    out = torch.full([b - a for a, b in ranges], 77, dtype=tdt, device="cuda")
    fl = torch.zeros(3, dtype=torch.int32, device="cuda") if flags else None
    for idx in itertools.product(*[range(-(-s // c)) for s, c in zip(arr.shape, arr.chunks)]):
        src, ts, bs, kind = arr.decode_chunk_shuffled(arr.read_chunk_bytes(idx))
        dev = torch.from_numpy(np.array(src)).cuda()
        assert backend.chunk_scatter(dev, ts, bs, kind, arr.chunks, [i * c for i, c in zip(idx, arr.chunks)], ranges, out, fl)
    return out.cpu().numpy(), (tuple(bool(v) for v in fl.cpu().tolist()) if flags else None)


@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.uint8])
@pytest.mark.parametrize("shuffle", ["bit", "byte", None])
def test_blosc_zstd_every_selection(tmp_path, dtype, shuffle):
    arr = store(tmp_path, values(dtype), blosc(shuffle, np.dtype(dtype).itemsize))
    for name, sel in SELECTIONS.items():
        want = unsqueezed(arr, sel)
        host, _ = scatter_all(arr, sel)
        got, _ = device_scatter_all(arr, sel)
        # (77 wherever the selection is not covered: nowhere -- and the kernel wrote nothing else)
        assert same_bits(got, want) and same_bits(got, host), name
        t = arr.read_device(sel, device="cuda")
        assert t.is_cuda and same_bits(t.cpu().numpy(), want), name


@pytest.mark.parametrize("compressor", [{"id": "gzip", "level": 1}, None], ids=["gzip", "none"])
def test_unshuffled_compressors(tmp_path, compressor):
    arr = store(tmp_path, values(np.float16, seed=1), compressor)
    for name, sel in SELECTIONS.items():
        assert same_bits(arr.read_device(sel, device="cuda").cpu().numpy(), unsqueezed(arr, sel)), name


def test_writes_the_intersection_and_nothing_else(tmp_path):
    """one chunk into a selection that reaches beyond it: everything outside the intersection keeps its bytes"""
    import torch
    arr = store(tmp_path, values(np.float16, seed=6), blosc("bit", 2))
    ranges, _ = arr._normalise(SELECTIONS["box"])
    idx = (0, 1, 1, 1)
    origin = [i * c for i, c in zip(idx, arr.chunks)]
    src, ts, bs, kind = arr.decode_chunk_shuffled(arr.read_chunk_bytes(idx))
    out = torch.full([b - a for a, b in ranges], 77, dtype=torch.float16, device="cuda")
    assert backend.chunk_scatter(torch.from_numpy(np.array(src)).cuda(), ts, bs, kind, arr.chunks, origin, ranges, out)
    want = np.full([b - a for a, b in ranges], 77, dtype=np.float16)
    mz.chunk_scatter_host(src, ts, bs, kind, arr.chunks, origin, ranges, want)
    assert (want == 77).any() and (want != 77).any() and same_bits(out.cpu().numpy(), want)


def test_missing_chunk_keeps_fill_value(tmp_path):
    data = values(np.float16, seed=2)
    root = mz.open(str(tmp_path / "s.zarr"), "a")
    arr = root.create("a", data.shape, CHUNKS, data.dtype, compressor=blosc("bit", 2), fill_value=-2.0, overwrite=True)
    arr[...] = data
    os.remove(arr.chunk_file((0, 1, 1, 2)))
    arr = mz.open(str(tmp_path / "s.zarr"), "r")["a"]
    for name, sel in SELECTIONS.items():
        want = unsqueezed(arr, sel)
        t, flags = arr.read_device(sel, device="cuda", flags=True)
        assert same_bits(t.cpu().numpy(), want) and flags == mz.value_flags(want), name


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("case", sorted(FLAG_CASES))
def test_flags(tmp_path, dtype, case):
    edits, whole = FLAG_CASES[case]
    data = values(dtype, seed=3)
    for at, v in edits.items():
        data[at] = v
    arr = store(tmp_path, data, blosc("bit", np.dtype(dtype).itemsize))
    for name, sel in SELECTIONS.items():
        want = unsqueezed(arr, sel)
        host = scatter_all(arr, sel, flags=True)[1]
        got, dev = device_scatter_all(arr, sel, flags=True)
        t, through = arr.read_device(sel, device="cuda", flags=True)
        assert same_bits(got, want) and same_bits(t.cpu().numpy(), want), name
        assert dev == host and through == host, (name, dev, through, host)
    assert arr.read_device(SELECTIONS["all"], device="cuda", flags=True)[1] == whole
    if case == "outside":
        assert arr.read_device(SELECTIONS["box"], device="cuda", flags=True)[1] == (False, False, False)


def test_full_waves_and_blocks(tmp_path):
    """one chunk of (27, 16, 32, 32) float16, the writer's own block size: 442 368 elements = 3 full blocks of
    131 072 elements (64 full waves each) and a last block of 49 152; 16-byte stores on aligned rows"""
    rng = np.random.default_rng(7)
    data = (rng.random((27, 16, 32, 32)) * 4 - 2).astype(np.float16)
    data[5, 3, 2, 1] = np.nan
    root = mz.open(str(tmp_path / "s.zarr"), "a")
    arr = root.create("a", data.shape, data.shape, data.dtype, overwrite=True)      # the reference's compressor
    arr[...] = data
    arr = mz.open(str(tmp_path / "s.zarr"), "r")["a"]
    src, ts, bs, kind = arr.decode_chunk_shuffled(arr.read_chunk_bytes((0, 0, 0, 0)))
    assert (ts, bs, kind, len(src)) == (2, 1 << 18, "bit", 884736)
    for sel in [(slice(None),) * 4, (slice(None), slice(1, 15), slice(3, 30), slice(5, 31)), (slice(2, 3), slice(None), 7, slice(None))]:
        want = unsqueezed(arr, sel)
        t, flags = arr.read_device(sel, device="cuda", flags=True)
        assert same_bits(t.cpu().numpy(), want) and flags == mz.value_flags(want)


def test_unserved_element_size(tmp_path):
    import torch
    data = values(np.float64, seed=4)
    arr = store(tmp_path, data, blosc("bit", 8))
    src, ts, bs, kind = arr.decode_chunk_shuffled(arr.read_chunk_bytes((0, 0, 0, 0)))
    ranges, _ = arr._normalise(SELECTIONS["all"])
    out = torch.zeros(data.shape, dtype=torch.float64, device="cuda")
    rc = backend.chunk_scatter_rc(torch.from_numpy(np.array(src)).cuda(), ts, bs, kind, arr.chunks, [0, 0, 0, 0], ranges, out)
    assert ts == 8 and rc == backend.ERR_UNSUPPORTED == -4
    assert not out.any()
    for name, sel in SELECTIONS.items():
        t = arr.read_device(sel, device="cuda")
        assert t.is_cuda and same_bits(t.cpu().numpy(), unsqueezed(arr, sel)), name


def test_one_upload_per_call(tmp_path):
    arr16 = store(tmp_path, values(np.float16, seed=5), blosc("bit", 2), name="a")
    arr64 = store(tmp_path, values(np.float64, seed=5), blosc("bit", 8), name="b")
    for arr in (arr16, arr64):
        for sel in SELECTIONS.values():
            before = backend.PRED_UPLOADS
            arr.read_device(sel, device="cuda", flags=True)
            assert backend.PRED_UPLOADS == before + 1
    before = backend.PRED_UPLOADS
    arr16.read_device(SELECTIONS["all"], device="cpu")
    assert backend.PRED_UPLOADS == before
