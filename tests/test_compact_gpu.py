"""GPU: a prediction kept as rows for the foreground voxels (csrc/ppp_rows.hip, patchperpix_amd.compact,
decode.decode_rows) -- index, expand and compact against torch bit for bit, the vote on a
CompactPrediction against the vote on the dense block, decode_rows against decode_volume, and
`--do label` with ``vote_from_code`` against `--do decode` + `--do label`."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from patchperpix_amd import backend, decode as dec, tiling
from patchperpix_amd.compact import CompactPrediction
from patchperpix_amd.flags import FLYLIGHT
from test_decode import AE_2D_25, AE_SHIPPED, _reference_named_state

pytestmark = pytest.mark.gpu

INT_VIEW = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def _masks(shape, rng):
    V = int(np.prod(shape))
    out = {"empty": np.zeros(shape, bool), "full": np.ones(shape, bool),
           "r30": rng.uniform(size=shape) < 0.3, "r03": rng.uniform(size=shape) < 0.03}
    last = np.zeros(shape, bool)
    last.reshape(-1)[-1] = True
    out["last"] = last
    # every set voxel in ONE 64-voxel word of one x-line
    one = np.zeros(shape, bool)
    x_hi = min(shape[2], 64)
    one[shape[0] // 2, shape[1] // 2, 1:x_hi:3] = True
    out["one_word"] = one
    assert V == one.size
    return out


def _boxes(shape):
    Z, Y, X = shape
    boxes = {"whole": (0, Z, 0, Y, 0, X), "voxel": (Z - 1, Z, Y // 2, Y // 2 + 1, X - 2, X - 1)}
    if X >= 70:
        boxes["interior"] = (0 if Z < 3 else 1, Z, 1, Y - 1, 3, 69)       # crosses a word boundary at both ends
    return boxes


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape,C", [((5, 7, 70), 27), ((5, 7, 70), 343), ((3, 9, 130), 27), ((3, 9, 130), 343),
                                     ((1, 20, 67), 25)])
def test_expand_and_compact_equal_torch_bit_for_bit(shape, C, dtype):
    rng = np.random.default_rng(hash((shape, C)) % 1000)
    g = torch.Generator(device="cpu").manual_seed(C + shape[2])
    iv = INT_VIEW[dtype]
    info = torch.iinfo(iv)
    for mname, mask in _masks(shape, rng).items():
        n = int(mask.sum())
        # every bit pattern is a legal element: the kernels move bits (nan payloads included)
        rows = torch.randint(info.min, info.max, (n, C), generator=g, dtype=torch.int64).to(iv).cuda().view(dtype)
        mask_t = torch.from_numpy(mask).cuda()
        index, n_rows = backend.rows_index_build(mask_t)
        assert n_rows == n, mname
        D = torch.zeros((C,) + shape, dtype=iv, device="cuda")
        D[:, mask_t] = rows.view(iv).t()
        boxes = dict(_boxes(shape))
        if mname == "last":                 # a box without any mask voxel: all zeros, no row touched
            boxes["no_mask_voxel"] = (0, shape[0], 0, max(1, shape[1] - 1), 0, max(1, shape[2] - 1))
        for bname, box in boxes.items():
            z0, z1, y0, y1, x0, x1 = box
            out = torch.full((C, z1 - z0, y1 - y0, x1 - x0), 0x5a5a if iv == torch.int16 else 0x5a5a5a5a,
                             dtype=iv, device="cuda").view(dtype)            # an unwritten voxel shows
            backend.rows_expand(rows, index, shape, box, out=out)
            want = D[:, z0:z1, y0:y1, x0:x1]
            assert torch.equal(out.view(iv), want), (mname, bname)
            # compact: the rows of the box's mask voxels, every other row untouched
            back = torch.full((n, C), 0x3c3c if iv == torch.int16 else 0x3c3c3c3c, dtype=iv, device="cuda").view(dtype)
            keep = back.clone()
            backend.rows_compact(out, box, index, shape, back)
            inbox = torch.zeros(shape, dtype=torch.bool, device="cuda")
            inbox[z0:z1, y0:y1, x0:x1] = True
            sel = inbox[mask_t]
            assert torch.equal(back.view(iv)[sel], rows.view(iv)[sel]), (mname, bname)
            assert torch.equal(back.view(iv)[~sel], keep.view(iv)[~sel]), (mname, bname)
            if bname == "no_mask_voxel":
                assert not bool(sel.any()) and not bool(out.view(iv).any())


@pytest.mark.parametrize("shape", [(3, 5, 64), (4, 6, 1), (2, 3, 200), (1, 1, 1), (9, 130, 70)])
def test_rows_index_counts_the_mask(shape):
    rng = np.random.default_rng(shape[2])
    mask = rng.uniform(size=shape) < 0.4
    mask_t = torch.from_numpy(mask).cuda()
    index, n = backend.rows_index_build(mask_t)
    assert n == int(mask.sum())
    # the row of every mask voxel through a one-channel expand: D holds k + 1 at the k-th voxel
    rows = torch.arange(1, n + 1, dtype=torch.float32, device="cuda").reshape(n, 1)
    got = backend.rows_expand(rows, index, shape, (0, shape[0], 0, shape[1], 0, shape[2]))
    want = torch.zeros(shape, dtype=torch.float32, device="cuda")
    want[mask_t] = rows[:, 0]
    assert torch.equal(got[0], want)
    assert int(index.numel()) <= max(4096, int(np.prod(shape)))          # at most a byte per voxel


def test_rows_index_refuses_2_31_voxels_by_the_sizes_alone():
    L = backend.lib()
    assert L.ppp_rows_index_bytes(2048, 1024, 1024) == -4              # PPP_ERR_UNSUPPORTED
    assert "2^31" in L.ppp_last_error().decode()
    assert L.ppp_rows_index_bytes(2047, 1024, 1024) > 0
    probe = torch.zeros(64, dtype=torch.uint8, device="cuda")           # never read: the sizes are refused first
    n = ctypes.c_int64(-1)
    rc = L.ppp_rows_index_build(backend._dev_ptr(probe), 2048, 1024, 1024, backend._dev_ptr(probe), ctypes.byref(n), None)
    assert rc == -4 and "2^31" in L.ppp_last_error().decode()
    box = backend.Box(0, 0, 0, 1, 1, 1)
    rc = L.ppp_rows_expand(backend._dev_ptr(probe), backend.F16, 27, backend._dev_ptr(probe), 2048, 1024, 1024,
                           ctypes.byref(box), backend._dev_ptr(probe), None)
    assert rc == -4


# ---- the vote --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def p7_case():
    """the recipe of test_decode_provider_votes_like_the_decoded_volume_p7 with 30 % foreground"""
    from patchperpix_amd.vote_instances import vote_instances as vi
    torch.manual_seed(7)
    rng = np.random.default_rng(7)
    d = dec.PatchDecoder(dict(AE_SHIPPED)).cuda().eval()
    shape = (22, 24, 26)
    code = torch.from_numpy(rng.normal(size=(176,) + shape).astype(np.float32)).cuda().half()
    fg = rng.uniform(size=shape) < 0.3
    probe = dec.decode_volume(d, code, fg, batch_size=2048, out_dtype=torch.float32)
    vals = probe[:, torch.as_tensor(fg, device="cuda")]
    with torch.no_grad():
        scale = 8.0 / float(vals.std())
        d.up_conv[-1][-1].weight.mul_(scale)
        d.up_conv[-1][-1].bias.mul_(scale).sub_(float(vals.median()) * scale)
    del probe, vals
    logits16 = dec.decode_volume(d, code, fg, batch_size=2048, out_dtype=torch.float16)
    fg_t = torch.as_tensor(fg, device="cuda")
    pred16 = torch.where(fg_t.expand_as(logits16), torch.sigmoid(logits16.double()).float(),
                         torch.zeros(logits16.shape, dtype=torch.float32, device="cuda"))
    kw = dict(FLYLIGHT, overlapping_inst=False)
    ps = [7, 7, 7]
    want, _ = vi.to_instance_seg(pred16, fg.copy(), fg.copy(), fg.astype(np.uint8), ps, **dict(kw, _n_slabs=1))
    cp = dec.decode_rows(d, code, fg, batch_size=2048, out_dtype=torch.float16, expit=True)
    return dict(d=d, code=code, fg=fg, shape=shape, logits16=logits16, pred16=pred16, kw=kw, ps=ps, want=want, cp=cp)


def test_compact_prediction_votes_like_the_dense_block_p7(p7_case):
    c = p7_case
    fg, shape, kw, ps, cp = c["fg"], c["shape"], c["kw"], c["ps"], c["cp"]
    assert c["want"].any()
    assert cp.voxels_decoded == int(fg.sum()) == cp.n_rows                  # every voxel decoded exactly once
    assert torch.equal(cp.to_dense(), c["pred16"])
    got, _ = tiling.assemble(cp, 0, shape, fg.copy(), fg.copy(), fg.astype(np.uint8), ps,
                             tiling.plan_slabs(shape[0], 2), _yx_tiles=(1, 2), **kw)
    assert np.array_equal(got, c["want"])
    prov = dec.DecodeProvider(c["d"], c["code"], fg, batch_size=2048, expit=True)
    again, _ = tiling.assemble(prov, 0, shape, fg.copy(), fg.copy(), fg.astype(np.uint8), ps,
                               tiling.plan_slabs(shape[0], 2), _yx_tiles=(1, 2), **kw)
    assert np.array_equal(again, c["want"])
    assert prov.voxels_decoded > cp.voxels_decoded                           # the halos, decoded again per tile
    assert cp.nbytes < cp.dense_nbytes


def test_to_instance_seg_accepts_a_compact_prediction(p7_case):
    from patchperpix_amd.vote_instances import vote_instances as vi
    c = p7_case
    fg, kw, ps, cp = c["fg"], c["kw"], c["ps"], c["cp"]
    got, _ = vi.to_instance_seg(cp, fg.copy(), fg.copy(), fg.astype(np.uint8), ps, **dict(kw, _n_slabs=1))
    assert np.array_equal(got, c["want"])
    pairs_w, aff_w = vi.to_instance_seg(c["pred16"], fg.copy(), fg.copy(), fg.astype(np.uint8), ps,
                                        **dict(kw, _n_slabs=1, return_intermediates=True))
    pairs, aff = vi.to_instance_seg(cp, fg.copy(), fg.copy(), fg.astype(np.uint8), ps,
                                    **dict(kw, _n_slabs=2, _yx_tiles=(1, 2), return_intermediates=True))
    assert np.array_equal(pairs, pairs_w) and len(pairs) > 0
    assert np.array_equal(np.asarray(aff).view(np.uint32), np.asarray(aff_w).view(np.uint32))
    # the path of a block that does NOT fit (forced): tiles planned from the free HBM, and forced tiles
    for extra in (dict(), dict(_n_slabs=2, _yx_tiles=(1, 2))):
        got, _ = vi.to_instance_seg(cp, fg.copy(), fg.copy(), fg.astype(np.uint8), ps,
                                    **dict(kw, _compact_resident=False, **extra))
        assert np.array_equal(got, c["want"]), extra
    with pytest.raises(NotImplementedError, match="compact prediction"):
        vi.to_instance_seg(cp, fg.copy(), fg.copy(), fg.astype(np.uint8), ps, **dict(kw, cuda=False))


# ---- decode straight into rows ---------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "torch_tail"])
def test_decode_rows_equals_decode_volume_at_the_foreground(fused):
    torch.manual_seed(11)
    d = dec.PatchDecoder(dict(AE_SHIPPED)).cuda().eval()
    shape = (6, 9, 11)
    V = int(np.prod(shape))
    g = torch.Generator(device="cpu").manual_seed(3)
    code = torch.randn((176,) + shape, generator=g).cuda()
    fg = torch.zeros(V, dtype=torch.bool)
    fg[torch.randperm(V, generator=g)[:401]] = True
    fg = fg.reshape(shape).cuda()
    rows = {}
    for dt in (torch.float16, torch.float32):
        vol = dec.decode_volume(d, code, fg, batch_size=128, out_dtype=dt, fused=fused)
        cp = dec.decode_rows(d, code, fg, batch_size=128, out_dtype=dt, fused=fused)
        assert cp.n_rows == 401 == cp.voxels_decoded and cp.rows.dtype == dt
        want = vol[:, fg].t().contiguous()
        assert torch.equal(cp.rows.view(INT_VIEW[dt]), want.view(INT_VIEW[dt]))
        assert float(cp.rows.float().abs().max()) > 0
        assert torch.equal(cp.to_dense().view(INT_VIEW[dt]), vol.view(INT_VIEW[dt]))
        rows[dt] = cp.rows
    if fused:       # the kernel rounds to float16 before it widens: narrowing the float32 rows is exact
        assert torch.equal(rows[torch.float32].to(torch.float16), rows[torch.float16])


def test_decode_rows_with_the_2d_decoder_uses_the_torch_tail():
    torch.manual_seed(12)
    rng = np.random.default_rng(12)
    d = dec.PatchDecoder(dict(AE_2D_25)).cuda().eval()
    assert d.fused_tail_params() is None
    shape = (2, 9, 10)
    code = rng.normal(size=(256,) + shape).astype(np.float32)
    fg = rng.uniform(size=shape) < 0.6
    vol = dec.decode_volume(d, code, fg, batch_size=64, device="cuda", out_dtype=torch.float32)
    cp = dec.decode_rows(d, code, fg, batch_size=64, device="cuda", out_dtype=torch.float32)
    assert cp.C == 625 and cp.shape == shape and cp.patchshape == (1, 25, 25)
    assert torch.equal(cp.rows, vol[:, torch.as_tensor(fg, device="cuda")].t())
    assert torch.equal(cp.to_dense(), vol)
    with pytest.raises(RuntimeError, match="no fused kernel"):
        dec.decode_rows(d, code, fg, batch_size=64, device="cuda", fused=True)


# ---- the driver ------------------------------------------------------------------------------
def test_label_from_code_equals_decode_then_label(tmp_path, p7_case):
    """`--do label` with vote_from_code on the container that holds the code, against `--do decode`
    followed by `--do label` on the decoded float16 array (loaded whole): the same dataset"""
    from patchperpix_amd import minizarr, run_ppp
    from test_cli_gpu import _load_result
    c = p7_case
    fg, shape = c["fg"], c["shape"]
    ckpt = tmp_path / "model.pt"
    torch.save({"model_state_dict": {k: v.detach().cpu() for k, v in _reference_named_state(c["d"]).items()}}, ckpt)
    prob = np.zeros((3,) + shape, dtype=np.float16)          # channel k = P(k instances)
    prob[0][~fg] = 0.97
    prob[1][fg] = 0.95
    pred_dir, dec_dir = tmp_path / "pred", tmp_path / "decoded"
    for folder, with_code in ((pred_dir, True), (dec_dir, False)):
        zf = minizarr.open(str(folder / "sampleC.zarr"), "w")
        zf.create_dataset("volumes/pred_numinst", data=prob, chunks=(3, 12, 12, 13))
        if with_code:
            zf.create_dataset("volumes/pred_code", data=c["code"].cpu().numpy(), chunks=(176, 11, 12, 13))
    base = os.path.join(GOLDEN_DIR, "label_config_flylight_zarr.toml")
    ae = dict(AE_SHIPPED)
    ae.pop("input_shape_squeezed")
    lines = ["[model]", "patchshape = [7, 7, 7]", "overlapping_inst = false", "code_units = 176", "[model.autoencoder]"]
    lines += ["%s = %s" % (k, ('"%s"' % v) if isinstance(v, str) else str(v).replace("(", "[").replace(")", "]"))
              for k, v in ae.items()]
    lines += ["[prediction]", 'code_key = "volumes/pred_code"', "decode_batch_size = 2048"]
    common = tmp_path / "common.toml"
    common.write_text("\n".join(lines) + "\n")
    dense, rows = tmp_path / "dense.toml", tmp_path / "rows.toml"
    dense.write_text("[vote_instances]\nstream_prediction = false\n")
    rows.write_text("[vote_instances]\nvote_from_code = true\n")
    run_ppp.main(["--config", base, "--config", str(common), "--do", "decode", "--checkpoint", str(ckpt),
                  "--pred-folder", str(pred_dir), "--output-folder", str(dec_dir)])
    run_ppp.main(["--config", base, "--config", str(common), "--config", str(dense), "--do", "label",
                  "--pred-folder", str(dec_dir), "--output-folder", str(tmp_path / "out_dense")])
    run_ppp.main(["--config", base, "--config", str(common), "--config", str(rows), "--do", "label",
                  "--checkpoint", str(ckpt), "--pred-folder", str(pred_dir), "--output-folder", str(tmp_path / "out_rows")])
    a, b = _load_result(str(tmp_path / "out_dense"), "sampleC"), _load_result(str(tmp_path / "out_rows"), "sampleC")
    assert a["vote_instances"].max() > 0
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # the decoded array was never written next to the code
    held = sorted(n for n in os.listdir(str(pred_dir / "sampleC.zarr" / "volumes")) if not n.startswith("."))
    assert held == ["pred_code", "pred_numinst"]
