"""CompactPrediction (patchperpix_amd.compact) on the CPU: rows for the mask voxels in raster order,
the torch form of expand / compact, the provider protocol of the tiled assembly with the oracle
standing in for the kernels (tests/oracle_ops.py), and the refusals."""
import os

import numpy as np
import pytest
import torch

from patchperpix_amd import synth, tiling
from patchperpix_amd.compact import CompactPrediction
from patchperpix_amd.flags import FLYLIGHT_NOTHIN_CC as FLYLIGHT


def _dense(rows, mask):
    D = np.zeros((rows.shape[1],) + mask.shape, dtype=rows.dtype)
    D[:, mask] = rows.T
    return D


def test_rows_are_the_mask_voxels_in_raster_order():
    rng = np.random.default_rng(1)
    shape, C = (3, 4, 5), 7
    mask = rng.uniform(size=shape) < 0.4
    # value of (channel c, voxel v) = 1000 v + c: a row names its voxel
    lin = np.arange(mask.size).reshape(shape)
    D = (1000.0 * lin[None] + np.arange(C)[:, None, None, None]).astype(np.float32)
    cp = CompactPrediction.from_dense(torch.from_numpy(D), mask, box_voxels=23)      # several boxes
    assert cp.n_rows == int(mask.sum()) and tuple(cp.rows.shape) == (cp.n_rows, C)
    want_vox = np.flatnonzero(mask.reshape(-1))                                    # raster order, x fastest
    assert np.array_equal(cp.rows[:, 0].numpy(), 1000.0 * want_vox)
    assert np.array_equal(cp.rows.numpy(), D.reshape(C, -1)[:, want_vox].T)
    assert cp.shape == shape and cp.nbytes >= cp.rows.numel() * 4
    with pytest.raises(ValueError, match="rows for a mask"):
        CompactPrediction.from_rows(cp.rows[:-1], mask)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_round_trip_and_unaligned_boxes(dtype):
    rng = np.random.default_rng(2)
    shape, C = (4, 6, 9), 27
    mask = rng.uniform(size=shape) < 0.3
    rows = torch.from_numpy(rng.normal(size=(int(mask.sum()), C)).astype(np.float32)).to(dtype)
    cp = CompactPrediction.from_rows(rows, mask, patchshape=(3, 3, 3))
    D = torch.zeros((C,) + shape, dtype=dtype)
    D[:, torch.from_numpy(mask)] = rows.t()
    assert torch.equal(cp.to_dense(), D)
    back = CompactPrediction.from_dense(cp.to_dense(), mask)
    assert torch.equal(back.rows, rows)
    for box in [(0, 4, 0, 6, 0, 9), (1, 3, 2, 5, 3, 8), (3, 4, 5, 6, 8, 9), (0, 1, 0, 6, 1, 2)]:
        z0, z1, y0, y1, x0, x1 = box
        got = cp.pred_box(box)
        assert got.dtype == dtype and torch.equal(got, D[:, z0:z1, y0:y1, x0:x1])
    # a provider is compacted box by box
    class Prov:
        def pred_box(self, b):
            return D[:, b[0]:b[1], b[2]:b[3], b[4]:b[5]]
    again = CompactPrediction.from_dense(Prov(), mask, C=C, dtype=dtype, device="cpu", box_voxels=60)
    assert torch.equal(again.rows, rows)


def test_expit_is_applied_at_the_mask_voxels_only():
    rng = np.random.default_rng(3)
    shape, C = (2, 5, 6), 27
    mask = rng.uniform(size=shape) < 0.5
    rows = torch.from_numpy(rng.normal(scale=4.0, size=(int(mask.sum()), C)).astype(np.float16))
    cp = CompactPrediction.from_rows(rows, mask, expit=True)
    got = cp.to_dense()
    want = torch.zeros((C,) + shape, dtype=torch.float32)
    want[:, torch.from_numpy(mask)] = torch.sigmoid(rows.double()).float().t()
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert not got[:, torch.from_numpy(~mask)].any()


def test_tiled_assembly_on_a_compact_prediction_equals_the_dense_one_cpu():
    """rows kept for the foreground only; two slabs, y/x tiles (1, 2): the instance map of the dense D"""
    from oracle import ppp_oracle as orc
    from oracle_ops import OracleOps
    ps, kw = [3, 3, 3], dict(FLYLIGHT)
    c = synth.make_case((20, 17, 19), ps, seed=63, cell=[5, 5, 5], overlap_frac=0.02)
    fg = c["foreground"].astype(bool)
    D = np.where(fg[None], c["pred"], 0).astype(np.float32)
    cp = CompactPrediction.from_dense(torch.from_numpy(D), fg, patchshape=ps)
    assert cp.n_rows == int(fg.sum()) < fg.size
    ref = orc.to_instance_seg(D, fg, fg.copy(), c["numinst"], ps, **kw)
    inst, _ = tiling.assemble(cp, 0, fg.shape, fg.copy(), fg.copy(), c["numinst"], ps,
                              tiling.plan_slabs(fg.shape[0], 2), ops=OracleOps(**kw), _yx_tiles=(1, 2), **kw)
    assert np.array_equal(inst, ref["instances"]) and inst.max() > 1
    dense, _ = tiling.assemble(torch.from_numpy(D), 0, fg.shape, fg.copy(), fg.copy(), c["numinst"], ps,
                               tiling.plan_slabs(fg.shape[0], 2), ops=OracleOps(**kw), _yx_tiles=(1, 2), **kw)
    assert np.array_equal(inst, dense)

    class Two(tiling.LocalComm):
        world = 2
    with pytest.raises(NotImplementedError, match="compact prediction: one rank only"):
        tiling.assemble(cp, 0, fg.shape, fg.copy(), fg.copy(), c["numinst"], ps,
                        tiling.plan_slabs(fg.shape[0], 2), ops=OracleOps(**kw), comm=Two(), **kw)


def test_refusals(tmp_path):
    from conftest import GOLDEN_DIR
    from patchperpix_amd import run_ppp
    from patchperpix_amd.vote_instances import vote_instances as vi
    mask = np.ones((3, 3, 3), dtype=bool)
    cp = CompactPrediction.from_rows(torch.zeros((27, 27)), mask, patchshape=(3, 3, 3))
    with pytest.raises(NotImplementedError, match="compact prediction"):
        vi.to_instance_seg(cp, mask.copy(), mask.copy(), mask.astype(np.uint8), [3, 3, 3],
                           **dict(FLYLIGHT, cuda=False))
    # vote_from_code with blockwise = false: refused by name, by the driver and by the entry point
    cfg = tmp_path / "from_code.toml"
    cfg.write_text("[vote_instances]\nvote_from_code = true\nblockwise = false\n")
    (tmp_path / "pred").mkdir()
    with pytest.raises(NotImplementedError, match="vote_from_code"):
        run_ppp.main(["--config", os.path.join(GOLDEN_DIR, "label_config.toml"), "--config", str(cfg), "--do", "label",
                      "--pred-folder", str(tmp_path / "pred"), "--output-folder", str(tmp_path / "out")])
    with pytest.raises(NotImplementedError, match="vote_from_code"):
        tiling.stitch_main(str(tmp_path / "x.zarr"), patchshape=[3, 3, 3], vote_from_code=True, blockwise=False)
