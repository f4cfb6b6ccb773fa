"""minizarr.chunk_scatter_host and Array.read_device(device="cpu") against the host reader Array.__getitem__
(which tests/test_minizarr.py pins): equal bits for every shuffle kind, compressor, element size and
selection, and the value flags of the elements written.  No GPU: the planning, ring and clipping code of the
device path runs with chunk_scatter_host in place of the kernel."""
import ctypes.util
import itertools
import os

import numpy as np
import pytest

from patchperpix_amd import minizarr as mz

SHAPE, CHUNKS = (7, 9, 10, 11), (7, 3, 5, 5)      # 525 elements a chunk: Blosc blocks of 256, 256 and 13 (8 + 5) at blocksize 512 / 2
SELECTIONS = {
    "all": (slice(None),) * 4,
    "box": (slice(1, 6), slice(2, 8), slice(3, 9), slice(4, 10)),       # aligned to no chunk edge
    "column": (slice(None), slice(4, 5), slice(7, 8), slice(6, 7)),     # one voxel column
    "index": (slice(None), 5, slice(1, 9), slice(None)),                # an integer index on one axis
}
HAVE_LZ4 = ctypes.util.find_library("lz4") is not None


def blosc(shuffle, typesize, cname="zstd"):
    return {"id": "blosc", "cname": cname, "clevel": 3, "shuffle": {None: 0, "byte": 1, "bit": 2}[shuffle],
            "blocksize": 256 * typesize}


def values(dtype, seed=0):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "f":
        return rng.random(SHAPE).astype(dtype)
    return rng.integers(0, 256, SHAPE).astype(dtype)


def store(tmp_path, data, compressor, name="a", chunks=CHUNKS):
    root = mz.open(str(tmp_path / "s.zarr"), "a")
    arr = root.create(name, data.shape, chunks, data.dtype, compressor=compressor, overwrite=True)
    arr[...] = data
    return mz.open(str(tmp_path / "s.zarr"), "r")[name]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def unsqueezed(arr, sel):
    ranges, _ = arr._normalise(sel)
    return arr[tuple(slice(a, b) for a, b in ranges)]


def scatter_all(arr, sel, flags=False):
    """chunk_scatter_host over every chunk of `arr`, the way read_device plans them"""
    ranges, _ = arr._normalise(sel)
    out = np.full([b - a for a, b in ranges], 77, dtype=arr.dtype)
    seen = [False] * 3
    for idx in itertools.product(*[range(-(-s // c)) for s, c in zip(arr.shape, arr.chunks)]):
        raw = arr.read_chunk_bytes(idx)
        src, ts, bs, kind = arr.decode_chunk_shuffled(raw)
        f = mz.chunk_scatter_host(src, ts, bs, kind, arr.chunks, [i * c for i, c in zip(idx, arr.chunks)], ranges, out, flags=flags)
        if flags:
            seen = [a or b for a, b in zip(seen, f)]
    return out, tuple(seen)


@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.uint8])
@pytest.mark.parametrize("shuffle", ["bit", "byte", None])
def test_blosc_zstd_every_selection(tmp_path, dtype, shuffle):
    data = values(dtype)
    arr = store(tmp_path, data, blosc(shuffle, np.dtype(dtype).itemsize))
    # (the store is what the test says it is: three blocks a chunk, the last of 13 elements)
    src, ts, bs, kind = arr.decode_chunk_shuffled(arr.read_chunk_bytes((0, 0, 0, 0)))
    assert (ts, bs, len(src)) == (np.dtype(dtype).itemsize, 256 * ts, 525 * ts)
    assert kind == (shuffle if (shuffle == "bit" or ts > 1) else None)
    for name, sel in SELECTIONS.items():
        want = unsqueezed(arr, sel)
        got, _ = scatter_all(arr, sel)
        assert same_bits(got, want), name
        t = arr.read_device(sel, device="cpu")
        assert same_bits(t.numpy(), want), name
        assert same_bits(np.squeeze(t.numpy(), axis=arr._normalise(sel)[1]), arr[sel]), name


@pytest.mark.parametrize("compressor", [
    pytest.param(blosc("bit", 2, "lz4"), id="blosc-lz4", marks=pytest.mark.skipif(not HAVE_LZ4, reason="liblz4 does not load")),
    pytest.param({"id": "gzip", "level": 1}, id="gzip"),
    pytest.param({"id": "zlib", "level": 1}, id="zlib"),
    pytest.param(None, id="none"),
])
def test_other_compressors(tmp_path, compressor):
    data = values(np.float16, seed=1)
    if compressor and compressor.get("cname") == "lz4":
        # the writer makes zstd and zlib frames only: every zstd frame is rewritten with its (still shuffled)
        # blocks compressed by liblz4 and the lz4 codec id in the header
        import ctypes
        L = mz._lz4()
        L.LZ4_compress_default.restype = ctypes.c_int
        L.LZ4_compress_default.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
        arr = store(tmp_path, data, blosc("bit", 2, "zstd"))
        packed = 0
        for fn in os.listdir(arr.path):
            if fn.startswith("."):
                continue
            raw = open(os.path.join(arr.path, fn), "rb").read()
            src = mz.blosc_decode(raw, unshuffle=False)[0]
            frame = bytearray(raw[:16])
            frame[2] = (frame[2] & 0x1f) | (1 << 5)
            nblocks = -(-len(src) // 512)
            body, starts, pos = b"", [], 16 + 4 * nblocks
            for b in range(nblocks):
                blk = src[b * 512:(b + 1) * 512].tobytes()
                dst = ctypes.create_string_buffer(len(blk) + 64)
                n = L.LZ4_compress_default(blk, dst, len(blk), len(dst))
                comp = dst.raw[:n] if 0 < n < len(blk) else blk
                packed += comp is not blk
                starts.append(pos + len(body))
                body += len(comp).to_bytes(4, "little") + comp
            frame[12:16] = (pos + len(body)).to_bytes(4, "little")
            open(os.path.join(arr.path, fn), "wb").write(bytes(frame) + b"".join(s.to_bytes(4, "little") for s in starts) + body)
        assert packed > 0 and same_bits(arr[...], data)
    else:
        arr = store(tmp_path, data, compressor)
    for name, sel in SELECTIONS.items():
        assert same_bits(arr.read_device(sel, device="cpu").numpy(), unsqueezed(arr, sel)), name
        assert same_bits(scatter_all(arr, sel)[0], unsqueezed(arr, sel)), name


def test_missing_chunk_keeps_fill_value(tmp_path):
    data = values(np.float16, seed=2)
    root = mz.open(str(tmp_path / "s.zarr"), "a")
    arr = root.create("a", data.shape, CHUNKS, data.dtype, compressor=blosc("bit", 2), fill_value=-2.0, overwrite=True)
    arr[...] = data
    os.remove(arr.chunk_file((0, 1, 1, 2)))
    arr = mz.open(str(tmp_path / "s.zarr"), "r")["a"]
    for name, sel in SELECTIONS.items():
        want = unsqueezed(arr, sel)
        t, flags = arr.read_device(sel, device="cpu", flags=True)
        assert same_bits(t.numpy(), want), name
        assert flags == mz.value_flags(want), name
    assert arr.read_device(SELECTIONS["all"], device="cpu", flags=True)[1] == (True, False, False)
    # the column selection misses the deleted chunk: its fill value must not count
    assert arr.read_device(SELECTIONS["column"], device="cpu", flags=True)[1] == (False, False, False)


FLAG_CASES = {
    "unit": ({}, (False, False, False)),
    "negative": ({(3, 4, 5, 6): -0.25}, (True, False, False)),
    "above": ({(3, 4, 5, 6): 1.5}, (False, True, False)),
    "both": ({(3, 4, 5, 6): -3.0, (1, 2, 3, 4): 7.0}, (True, True, False)),
    "both+nan": ({(3, 4, 5, 6): -3.0, (1, 2, 3, 4): 7.0, (5, 7, 8, 9): float("nan")}, (True, True, True)),
    "edges": ({(3, 4, 5, 6): -0.0, (1, 2, 3, 4): 0.0, (5, 7, 8, 9): 1.0, (2, 2, 3, 5): float("inf")}, (False, True, False)),
    # the only negative value lies outside the box selection (axis 0 index 0): its flag stays clear there
    "outside": ({(0, 0, 0, 0): -1.0}, (True, False, False)),
}


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
        flags = (bool((want < 0).any()), bool((want > 1).any()), bool(np.isnan(want).any()))
        t, got = arr.read_device(sel, device="cpu", flags=True)
        assert same_bits(t.numpy(), want) and got == flags, (name, got, flags)
        assert scatter_all(arr, sel, flags=True)[1] == flags, name
    assert arr.read_device(SELECTIONS["all"], device="cpu", flags=True)[1] == whole
    if case == "outside":
        assert arr.read_device(SELECTIONS["box"], device="cpu", flags=True)[1] == (False, False, False)
    # loadAffinities' rule, derived from the three flags
    neg, gt1, nan = arr.read_device(SELECTIONS["all"], device="cpu", flags=True)[1]
    with np.errstate(invalid="ignore"):
        assert ((not nan) and neg and gt1) == bool(np.min(data) < 0 and np.max(data) > 1)


def test_unserved_forms_take_the_host_reader(tmp_path):
    data = values(np.float64, seed=4)
    arr = store(tmp_path, data, blosc("bit", 8))
    for name, sel in SELECTIONS.items():
        assert same_bits(arr.read_device(sel, device="cpu").numpy(), unsqueezed(arr, sel)), name
    with pytest.raises(NotImplementedError):
        arr.read_device((slice(None, None, 2),), device="cpu")


def test_ring_is_bounded_and_reused(tmp_path):
    data = values(np.float16, seed=5)
    arr = store(tmp_path, data, blosc("bit", 2))          # 3 x 2 x 3 = 18 chunks through 4 slots
    a = arr.read_device(SELECTIONS["all"], device="cpu")
    ring = arr._rings["cpu"]
    assert len(ring["host"]) == mz.RING_SLOTS == 4 and all(h.numel() == 525 * 2 for h in ring["host"])
    b = arr.read_device(SELECTIONS["box"], device="cpu")
    assert arr._rings["cpu"] is ring
    assert same_bits(a.numpy(), data) and same_bits(b.numpy(), data[SELECTIONS["box"]])
