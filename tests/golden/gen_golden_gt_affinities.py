#!/usr/bin/env python3
"""tests/golden/gt_affinities/*.npz (a folder of their own: tests/conftest.py takes every *.npz directly under
tests/golden that it does not know by prefix for a vote_instances golden): the reference's own
`seg_to_affgraph_*_torch*` functions (PatchPerPix/util/train_util.py:349-695, imported in place with `gunpowder`
stubbed) on small CPU tensors.  Development container only.

  python tests/golden/gen_golden_gt_affinities.py

A file holds the inputs (`seg` int32, `nhood`, for the sampled forms `samples`, `ps`, `psH`) and the reference's
outputs: the 0/1 results as uint8, the id-squared results as float32.  The archives are written with fixed
time stamps, so a second run gives the same bytes.  The generator asserts that each case holds what it is for
and that this project's NumPy definition gives the same arrays (the tests say it again without the reference)."""
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "gt_affinities")
REF = "/root/reference/PatchPerPix"


def load_reference():
    gp = types.ModuleType("gunpowder")
    sys.modules["gunpowder"] = gp
    spec = importlib.util.spec_from_file_location("ppp_ref_train_util", os.path.join(REF, "util", "train_util.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def save(name, **arrays):
    """a compressed .npz with fixed time stamps: the same arrays give the same bytes"""
    path = os.path.join(OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            a = np.asarray(arrays[key])
            np.lib.format.write_array(buf, a if a.ndim == 0 else np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())
    print("%-12s %7d bytes  %s" % (name, os.path.getsize(path), sorted(arrays)))


def boxes(rng, L, spatial, n_inst, first_id=1):
    """random boxes, each put into the first channel in which it covers no earlier instance: the later channels
    receive the boxes that overlap, so voxels with two non-zero channels exist"""
    labels = np.zeros((L,) + spatial, dtype=np.int32)
    for k in range(n_inst):
        lo = [int(rng.integers(0, max(1, s - 2))) for s in spatial]
        hi = [min(s, a + int(rng.integers(2, 6))) for a, s in zip(lo, spatial)]
        box = tuple(slice(a, b) for a, b in zip(lo, hi))
        for c in range(L):
            if not labels[c][box].any():
                labels[c][box] = first_id + 7 * k
                break
    return labels


def centred(r, ndim):
    g = np.meshgrid(*[np.arange(-r, r + 1)] * ndim, indexing="ij")
    return np.stack([a.reshape(-1) for a in g], axis=1)


def raster(ps, ndim):
    g = np.meshgrid(*[np.arange(ps)] * ndim, indexing="ij")
    return np.stack([a.reshape(-1) for a in g], axis=1)


def ours():
    sys.path.insert(0, ROOT)
    from patchperpix_amd import train_util
    return train_util


def lift(seg, nhood, ndim, single):
    """the arguments of gt_affs_dense_host for 2-d / 3-d data"""
    lead = seg.shape[:-ndim]
    seg5 = seg.reshape(lead + (1,) * (3 - ndim) + seg.shape[-ndim:])
    n3 = nhood if ndim == 3 else np.concatenate([np.zeros_like(nhood[:, :1]), nhood], axis=1)
    return seg5, n3


def dense_case(ref, name, fn, seg, nhood, ndim, single=False):
    import torch
    aff = getattr(ref, fn)(torch.from_numpy(seg), nhood, "cpu").numpy()
    assert aff.dtype == np.float32
    seg5, n3 = lift(seg, nhood, ndim, single)
    mine = ours().gt_affs_dense_host(seg5, n3, single=single)
    assert np.array_equal(mine.reshape(aff.shape), aff), name
    if single:
        assert aff.max() > 1 and np.array_equal(np.unique(aff), np.unique(aff.astype(np.int64)))
        save(name, seg=seg, nhood=nhood, aff=aff)
    else:
        assert set(np.unique(aff)) == {0.0, 1.0}, name
        save(name, seg=seg, nhood=nhood, aff=aff.astype(np.uint8))
    return aff


def d3_multi(ref):
    rng = np.random.default_rng(101)
    spatial = (6, 9, 21)
    seg = np.stack([boxes(rng, 3, spatial, 14, first_id=3 + 100 * b) for b in range(2)])
    # one id that sits in channel 0 on one side of the plane x = 10 and in channel 1 on the other
    seg[0, :, 1:4, 2:6, 6:14] = 0
    seg[0, 0, 1:4, 2:6, 6:10] = 77
    seg[0, 1, 1:4, 2:6, 10:14] = 77
    seg[1, 2, 3:6, 5:9, 15:21][seg[1, 2, 3:6, 5:9, 15:21] == 0] = -5          # one negative id
    nhood = centred(2, 3)
    aff = dense_case(ref, "d3_multi", "seg_to_affgraph_3d_multi_torch", seg, nhood, 3)
    assert ((seg != 0).sum(axis=1) > 1).any(), "no overlap voxel"
    assert (seg == -5).sum() > 4
    e = int(np.where((nhood == [0, 0, 1]).all(axis=1))[0][0])
    assert seg[0, 0, 2, 3, 9] == 77 and seg[0, 1, 2, 3, 10] == 77 and aff[0, e, 2, 3, 9] == 0, "the per-channel rule"
    assert aff[0, e, 2, 3, 8] == 1


def d3_thin(ref):
    rng = np.random.default_rng(102)
    seg = boxes(rng, 2, (2, 5, 3), 6)[None]
    assert seg.any()
    dense_case(ref, "d3_thin", "seg_to_affgraph_3d_multi_torch", seg, centred(2, 3), 3)


def d3_offsets(ref):
    rng = np.random.default_rng(103)
    spatial = (6, 9, 21)
    seg = boxes(rng, 1, spatial, 10)[None]
    far = [[6, 0, 0], [-6, 0, 0], [0, 9, 0], [0, -9, 0], [0, 0, 21], [0, 0, -21]]
    nhood = np.concatenate([raster(5, 3), np.array(far)])
    aff = dense_case(ref, "d3_offsets", "seg_to_affgraph_3d_multi_torch", seg, nhood, 3)
    assert not aff[:, 125:].any() and aff[:, :125].any()


def d2_multi(ref):
    rng = np.random.default_rng(104)
    seg = np.stack([boxes(rng, 2, (11, 23), 9, first_id=2 + 50 * b) for b in range(2)])
    assert ((seg != 0).sum(axis=1) > 1).any()
    dense_case(ref, "d2_multi", "seg_to_affgraph_2d_multi_torch", seg, centred(3, 2), 2)


def singles(ref):
    rng = np.random.default_rng(105)
    seg = np.stack([boxes(rng, 1, (4, 5, 7), 5, first_id=11 + 40 * b)[0] for b in range(2)])
    assert 0 < seg.max() < 300
    aff = dense_case(ref, "d3_single", "seg_to_affgraph_3d_torch", seg, centred(1, 3), 3, single=True)
    assert np.array_equal(aff[:, 13], seg.astype(np.float32) ** 2), "the centre channel is id squared"
    seg = np.stack([boxes(rng, 1, (9, 10), 5, first_id=13 + 60 * b)[0] for b in range(2)])
    assert 0 < seg.max() < 300
    aff = dense_case(ref, "d2_single", "seg_to_affgraph_2d_torch", seg, centred(1, 2), 2, single=True)
    assert np.array_equal(aff[:, 4], seg.astype(np.float32) ** 2)


def sample_rows(rng, B, spatial, ps, n):
    """seeded random corners, every corner at the extreme in-bounds position of each axis, and duplicated rows"""
    top = [s - ps for s in spatial]
    rows = [[b] + [t if (k >> a) & 1 else 0 for a, t in enumerate(top)] for b in range(B) for k in range(2 ** len(top))]
    while len(rows) < n - 6:
        rows.append([int(rng.integers(0, B))] + [int(rng.integers(0, t + 1)) for t in top])
    rows += [rows[-1], rows[-1], rows[0], rows[20], rows[20], rows[3]]
    rows = np.array(rows, dtype=np.int64)
    assert len(rows) == n
    return rows[rng.permutation(n)]


def sampled_case(ref, name, ndim, B, L, spatial, ps, seed):
    import torch
    rng = np.random.default_rng(seed)
    seg = np.stack([boxes(rng, L, spatial, 12, first_id=4 + 90 * b) for b in range(B)])
    psH = ps // 2
    nhood = raster(ps, ndim)
    rows = sample_rows(rng, B, spatial, ps, 70)
    d = "%dd" % ndim
    tseg = torch.from_numpy(seg)
    fn = getattr(ref, "seg_to_affgraph_%s_multi_torch_code" % d)
    fnb = getattr(ref, "seg_to_affgraph_%s_multi_torch_code_batch" % d)
    aff = fn(tseg, nhood, "cpu", ps, psH, rows).numpy()
    aff_n1 = fn(tseg, nhood, "cpu", ps, psH, rows[:1]).numpy()
    batch_rows = rows[rows[:, 0] == 1][:, 1:]
    aff_batch = fnb(tseg, nhood, "cpu", ps, psH, batch_rows, 1).numpy()
    assert aff.shape == (70, ps ** ndim) and aff.any() and not aff.all() and np.array_equal(aff_n1, aff[:1])
    assert np.array_equal(aff_batch, aff[rows[:, 0] == 1])
    # this project's definition, and the dense result at loc + psH
    tu = ours()
    seg5, _ = lift(seg, nhood, ndim, False)
    rows4 = rows if ndim == 3 else np.concatenate([rows[:, :1], np.zeros_like(rows[:, :1]), rows[:, 1:]], axis=1)
    n3 = nhood if ndim == 3 else np.concatenate([np.zeros_like(nhood[:, :1]), nhood], axis=1)
    ps3, ctr3 = (1,) * (3 - ndim) + (ps,) * ndim, (0,) * (3 - ndim) + (psH,) * ndim
    assert np.array_equal(tu.gt_affs_samples_host(seg5, rows4, n3, ps3, ctr3), aff), name
    dense = tu.gt_affs_dense_host(seg5, n3 - np.array(ctr3))
    at = rows4[:, 1:] + np.array(ctr3)
    assert np.array_equal(dense[rows4[:, 0], :, at[:, 0], at[:, 1], at[:, 2]], aff), name
    save(name, seg=seg, nhood=nhood, ps=np.int64(ps), psH=np.int64(psH), samples=rows, aff=aff.astype(np.uint8),
         aff_n1=aff_n1.astype(np.uint8), batch_b=np.int64(1), batch_rows=batch_rows, aff_batch=aff_batch.astype(np.uint8))


def main():
    ref = load_reference()
    os.makedirs(OUT, exist_ok=True)
    d3_multi(ref)
    d3_thin(ref)
    d3_offsets(ref)
    d2_multi(ref)
    singles(ref)
    sampled_case(ref, "s3_multi", 3, 2, 2, (12, 13, 14), 5, seed=106)
    sampled_case(ref, "s2_multi", 2, 2, 3, (17, 19), 7, seed=107)
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    assert total < 1000000, total
    print("total %d bytes" % total)


if __name__ == "__main__":
    main()
