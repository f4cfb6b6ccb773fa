"""GPU: the ground-truth patch affinities kernels (csrc/ppp_gt_affs.hip) through the reference's names of
patchperpix_amd/train_util.py and through backend.gt_affs_dense / gt_affs_samples: every golden of
tests/golden/gt_affinities bit for bit, the NumPy definition on seeded random cases sized by the kernel's plan
(tile overhang on every axis, staged and direct loads, 1 .. 6 label channels, asymmetric halos), the three
output types, boxes at odd offsets, `out=` under a sentinel, N = 0 / 1 / duplicates, determinism, check=False,
output offsets past 2^31, the cross-check with ppp_eval_patch's num_gt, and the ABI's argument codes.
0 / 1 and small integer squares throughout: every comparison is exact."""
import ctypes

import numpy as np
import pytest

from test_gt_affinities import DENSE, SAMPLED, load
from test_gt_affinities import test_entry_points_check_their_arguments_before_any_device as argument_codes

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _needs_gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"


def tu():
    from patchperpix_amd import train_util
    return train_util


def be():
    from patchperpix_amd import backend
    return backend


def dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def bits(t):
    import torch
    a = t.detach().cpu()
    return a.view({4: torch.int32, 2: torch.int16}[a.element_size()]).numpy()


def same(t, want):
    """a float32 device result equals the float32 array `want` bit for bit"""
    got = t.detach().cpu().numpy()
    return got.dtype == np.float32 and got.shape == want.shape and \
        np.array_equal(got.view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32))


def make_labels(rng, B, L, spatial, n=None, negative=True):
    """boxes of about a third of each extent dealt to the channels in turn, so that they overlap; ids repeat
    across channels (the per-channel rule matters) and one id is negative"""
    seg = np.zeros((B, L) + spatial, dtype=np.int32)
    n = n or 4 * L + 3
    for b in range(B):
        for k in range(n):
            lo = [int(rng.integers(0, s)) for s in spatial]
            box = tuple(slice(a, a + max(1, s // 3) + 1) for a, s in zip(lo, spatial))
            seg[b, k % L][box] = 3 + k % 5
        if negative:
            seg[b, L - 1].reshape(-1)[: max(1, seg[b, L - 1].size // 7)] = -9
    return seg


def centred(r):
    g = np.meshgrid(np.arange(-r[0], r[0] + 1), np.arange(-r[1], r[1] + 1), np.arange(-r[2], r[2] + 1), indexing="ij")
    return np.stack([a.reshape(-1) for a in g], axis=1)


def halo_of(nhood):
    lo, hi = nhood.min(axis=0), nhood.max(axis=0)
    return (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2])


def plan_of(seg, nhood, out_dtype=None, single=False, box=None):
    B, L = seg.shape[0], (1 if single else seg.shape[1])
    vol = seg.shape[-3:]
    return be().gt_affs_dense_plan(B, L, vol, len(nhood), halo_of(nhood), box or (0, vol[0], 0, vol[1], 0, vol[2]),
                                   out_dtype, single)


# ---------------------------------------------------------------------------------------------
# the goldens, through the reference's names
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DENSE))
def test_dense_goldens_bit_for_bit(name):
    import torch
    g = load(name)
    fn = getattr(tu(), DENSE[name][0])
    want = g["aff"].astype(np.float32)
    got = fn(dev(g["seg"]), g["nhood"], "cuda")
    assert got.is_cuda and same(got, want)
    # int64 labels and a device nhood tensor, as torch_model.py hands them over
    got = fn(dev(g["seg"], torch.int64), dev(g["nhood"]), "cuda")
    assert same(got, want)


def test_the_offsets_golden_takes_the_direct_path_and_the_others_the_staged_one():
    g = load("d3_offsets")
    n3 = g["nhood"]
    assert plan_of(g["seg"], n3)[3] == 0
    g = load("d3_multi")
    assert plan_of(g["seg"], g["nhood"])[3] == 1


@pytest.mark.parametrize("name", sorted(SAMPLED))
def test_sampled_goldens_bit_for_bit(name):
    import torch
    g = load(name)
    d = "%dd" % SAMPLED[name]
    fn = getattr(tu(), "seg_to_affgraph_%s_multi_torch_code" % d)
    fnb = getattr(tu(), "seg_to_affgraph_%s_multi_torch_code_batch" % d)
    ps, psH = int(g["ps"]), int(g["psH"])
    seg = dev(g["seg"])
    assert same(fn(seg, g["nhood"], "cuda", ps, psH, dev(g["samples"])), g["aff"].astype(np.float32))
    assert same(fn(seg, dev(g["nhood"]), "cuda", ps, psH, dev(g["samples"][:1])), g["aff_n1"].astype(np.float32))
    assert same(fnb(seg, g["nhood"], "cuda", ps, psH, dev(g["batch_rows"]), int(g["batch_b"])),
                g["aff_batch"].astype(np.float32))
    # int32 rows as torch_model.py:198 builds its batch column, and host rows
    assert same(fn(seg, g["nhood"], "cuda", ps, psH, dev(g["samples"], torch.int32)), g["aff"].astype(np.float32))
    assert same(fn(seg, g["nhood"], "cuda", ps, psH, g["samples"]), g["aff"].astype(np.float32))


# ---------------------------------------------------------------------------------------------
# seeded random cases against the NumPy definition
# ---------------------------------------------------------------------------------------------
def test_every_axis_exceeds_the_tile_by_a_non_multiple():
    """chosen AFTER the kernel's tile was fixed: 4 x 8 x 32 for 27 edges and two channels"""
    rng = np.random.default_rng(1)
    spatial = (6, 19, 75)
    seg = make_labels(rng, 2, 2, spatial)
    nhood = centred((1, 1, 1))
    tile = plan_of(seg, nhood)
    assert tile[:4] == (4, 8, 32, 1)
    assert all(s > t and s % t for s, t in zip(spatial, tile[:3])) and np.prod(spatial) <= 40 * 40 * 150
    want = tu().gt_affs_dense_host(seg, nhood)
    assert want.any() and not want.all()
    assert same(tu().seg_to_affgraph_3d_multi_torch(dev(seg), nhood, "cuda"), want)


@pytest.mark.parametrize("L", [1, 4, 6])
def test_channel_counts(L):
    """L = 6: more channels than a lane keeps centre labels of in registers"""
    rng = np.random.default_rng(10 + L)
    seg = make_labels(rng, 1, L, (5, 11, 37))
    nhood = centred((1, 2, 2))
    assert plan_of(seg, nhood)[3] == 1
    assert same(tu().seg_to_affgraph_3d_multi_torch(dev(seg), nhood, "cuda"), tu().gt_affs_dense_host(seg, nhood))


@pytest.mark.parametrize("L", [2, 5])
def test_direct_loads_where_tile_and_halo_do_not_fit(L):
    rng = np.random.default_rng(20 + L)
    seg = make_labels(rng, 2, L, (5, 9, 70))
    nhood = np.concatenate([centred((1, 1, 2)), [[0, 0, 40], [0, 0, -40], [4, 8, 69], [-4, -8, -69], [0, 0, 70], [5, 0, 0],
                                                 [0, 0, 2 ** 31 - 1], [0, -2 ** 31, 0]]])
    assert plan_of(seg, nhood)[3] == 0
    want = tu().gt_affs_dense_host(seg, nhood)
    assert want[:, -8:-4].any() and not want[:, -4:].any()
    assert same(tu().seg_to_affgraph_3d_multi_torch(dev(seg), nhood, "cuda"), want)


def test_asymmetric_halo_staged():
    rng = np.random.default_rng(30)
    seg = make_labels(rng, 1, 3, (7, 13, 41))
    g = np.meshgrid(np.arange(3), np.arange(3), np.arange(4), indexing="ij")
    nhood = np.stack([a.reshape(-1) for a in g], axis=1)                 # raster: nothing negative, nothing centred
    assert plan_of(seg, nhood)[3] == 1
    assert same(tu().seg_to_affgraph_3d_multi_torch(dev(seg), nhood, "cuda"), tu().gt_affs_dense_host(seg, nhood))
    assert same(tu().seg_to_affgraph_3d_multi_torch(dev(seg), -nhood, "cuda"), tu().gt_affs_dense_host(seg, -nhood))
    far = nhood + [1, 2, 3]                                              # offset 0 outside [min, max]
    assert same(tu().seg_to_affgraph_3d_multi_torch(dev(seg), far, "cuda"), tu().gt_affs_dense_host(seg, far))


def test_2d_image_with_a_wide_patch_and_split_edges():
    rng = np.random.default_rng(40)
    seg = make_labels(rng, 2, 2, (1, 37, 70))[:, :, 0]
    g = np.meshgrid(np.arange(-6, 7), np.arange(-6, 7), indexing="ij")
    nhood = np.stack([a.reshape(-1) for a in g], axis=1)                 # 169 edges: several edge ranges per tile
    n3 = np.concatenate([np.zeros_like(nhood[:, :1]), nhood], axis=1)
    plan = plan_of(seg[:, :, None], n3)
    assert plan[0] == 1 and plan[3] == 1 and plan[4] > 1
    want = tu().gt_affs_dense_host(seg[:, :, None], n3)[:, :, 0]
    assert same(tu().seg_to_affgraph_2d_multi_torch(dev(seg), nhood, "cuda"), want)


def test_single_channel_form_random():
    rng = np.random.default_rng(50)
    seg = make_labels(rng, 2, 1, (6, 11, 45))[:, 0] * 1000                # ids up to 7000, and -9000
    seg[0, 0, 0, :2] = (46340, -46340)
    nhood = centred((1, 1, 2))
    assert plan_of(seg, nhood, single=True)[3] == 1
    want = tu().gt_affs_dense_host(seg, nhood, single=True)
    assert want.max() == np.float32(46340 ** 2)
    assert same(tu().seg_to_affgraph_3d_torch(dev(seg), nhood, "cuda"), want)
    far = np.concatenate([nhood, [[0, 0, 44], [0, 0, 45], [0, -11, 0], [5, 10, 44], [-5, -10, -44]]])
    assert plan_of(seg, far, single=True)[3] == 0
    assert same(tu().seg_to_affgraph_3d_torch(dev(seg), far, "cuda"), tu().gt_affs_dense_host(seg, far, single=True))
    assert same(tu().seg_to_affgraph_2d_torch(dev(seg[:, 2]), nhood[:, 1:], "cuda"),
                tu().gt_affs_dense_host(seg[:, 2:3], np.concatenate([0 * nhood[:, :1], nhood[:, 1:]], axis=1), single=True)[:, :, 0])


@pytest.mark.parametrize("X", [40, 44, 45])
def test_half_types_equal_the_float32_result_cast(X):
    """X = 40: whole 16-byte stores of eight; 44: every other row 8 bytes off; 45: rows at every 2-byte phase"""
    import torch
    rng = np.random.default_rng(60 + X)
    seg = make_labels(rng, 2, 3, (5, 10, X))
    nhood = centred((1, 1, 1))
    d_seg = dev(seg)
    f32 = tu().seg_to_affgraph_3d_multi_torch(d_seg, nhood, "cuda")
    assert same(f32, tu().gt_affs_dense_host(seg, nhood))
    for dt in (torch.float16, torch.bfloat16):
        got = tu().seg_to_affgraph_3d_multi_torch(d_seg, nhood, "cuda", out_dtype=dt)
        assert got.dtype == dt and np.array_equal(bits(got), bits(f32.to(dt)))
    rows = dev(np.array([[0, 0, 0, 0], [1, 2, 7, X - 3], [1, 2, 7, X - 3]]))
    ras = centred((1, 1, 1)) + 1
    s32 = tu().seg_to_affgraph_3d_multi_torch_code(d_seg, ras, "cuda", 3, 1, rows)
    for dt in (torch.float16, torch.bfloat16):
        got = tu().seg_to_affgraph_3d_multi_torch_code(d_seg, ras, "cuda", 3, 1, rows, out_dtype=dt)
        assert got.dtype == dt and np.array_equal(bits(got), bits(s32.to(dt)))


def test_box_at_odd_offsets_and_out_under_a_sentinel():
    import torch
    rng = np.random.default_rng(70)
    seg = make_labels(rng, 2, 2, (9, 21, 53))
    nhood = centred((2, 2, 2))
    d_seg = dev(seg)
    full = tu().seg_to_affgraph_3d_multi_torch(d_seg, nhood, "cuda")
    assert same(full, tu().gt_affs_dense_host(seg, nhood))
    for box in ((1, 8, 3, 20, 5, 52), (2, 7, 2, 19, 2, 51), (3, 4, 1, 2, 7, 8), (0, 9, 0, 21, 1, 53)):
        crop = full[:, :, box[0]:box[1], box[2]:box[3], box[4]:box[5]]
        got = tu().seg_to_affgraph_3d_multi_torch(d_seg, nhood, "cuda", box=box)
        assert got.shape == crop.shape and np.array_equal(bits(got), bits(crop.contiguous()))
        for dt in (torch.float32, torch.float16):
            out = torch.full(crop.shape, float("nan"), dtype=dt, device="cuda")
            res = be().gt_affs_dense(d_seg, dev(nhood.astype(np.int32)), box=box, out=out)
            assert res is out and not torch.isnan(out).any()
            assert np.array_equal(bits(out), bits(crop.to(dt).contiguous()))
    one = dev(seg[:, 0] * 100)
    full1 = tu().seg_to_affgraph_3d_torch(one, nhood, "cuda")
    out = torch.full((2, 125, 7, 17, 47), float("nan"), device="cuda")
    be().gt_affs_dense(one, dev(nhood.astype(np.int32)), box=(1, 8, 3, 20, 5, 52), out=out, single=True)
    assert not torch.isnan(out).any() and np.array_equal(bits(out), bits(full1[:, :, 1:8, 3:20, 5:52].contiguous()))


def test_samples_none_one_duplicates_and_rows_that_leave_the_volume():
    import torch
    rng = np.random.default_rng(80)
    seg = make_labels(rng, 3, 2, (9, 10, 11))
    d_seg = dev(seg)
    g = np.meshgrid(np.arange(5), np.arange(5), np.arange(5), indexing="ij")
    nhood = np.stack([a.reshape(-1) for a in g], axis=1)
    fn = tu().seg_to_affgraph_3d_multi_torch_code
    got = fn(d_seg, nhood, "cuda", 5, 2, torch.zeros((0, 4), dtype=torch.int64, device="cuda"))
    assert got.is_cuda and tuple(got.shape) == (0, 125) and got.dtype == torch.float32
    rows = np.array([[rng.integers(0, 3), rng.integers(0, 5), rng.integers(0, 6), rng.integers(0, 7)] for _ in range(300)])
    rows[100:200] = rows[7]                                              # one row a hundred times
    want = tu().gt_affs_samples_host(seg, rows, nhood, (5, 5, 5), (2, 2, 2))
    assert want.any() and not want.all()
    assert same(fn(d_seg, nhood, "cuda", 5, 2, dev(rows)), want)
    assert same(fn(d_seg, nhood, "cuda", 5, 2, dev(rows[7:8])), want[7:8])
    # the C entry point reads voxels outside the volume as 0: check=False, patches that leave the volume
    wild = np.array([[0, 7, 0, 0], [1, -3, 2, 2], [2, 0, 8, 9], [3, 0, 0, 0], [-1, 0, 0, 0], [2, 4, 5, 6], [0, -9, -9, -9]])
    with pytest.raises(ValueError, match="leaves the volume"):
        fn(d_seg, nhood, "cuda", 5, 2, dev(wild))
    assert same(fn(d_seg, nhood, "cuda", 5, 2, dev(wild), check=False),
                tu().gt_affs_samples_host(seg, wild, nhood, (5, 5, 5), (2, 2, 2)))


def test_check_off_and_two_calls_give_identical_bits():
    import torch
    g = load("d3_multi")
    seg, nhood = dev(g["seg"]), dev(g["nhood"])
    a = tu().seg_to_affgraph_3d_multi_torch(seg, nhood, "cuda")
    b = tu().seg_to_affgraph_3d_multi_torch(seg, nhood, "cuda", check=False)
    c = tu().seg_to_affgraph_3d_multi_torch(seg, nhood, "cuda", check=False)
    assert torch.equal(a, b) and torch.equal(b, c) and same(a, g["aff"].astype(np.float32))
    s = load("s3_multi")
    args = (dev(s["seg"]), s["nhood"], "cuda", int(s["ps"]), int(s["psH"]), dev(s["samples"]))
    x = tu().seg_to_affgraph_3d_multi_torch_code(*args)
    y = tu().seg_to_affgraph_3d_multi_torch_code(*args, check=False)
    assert torch.equal(x, y) and same(y, s["aff"].astype(np.float32))
    with pytest.raises(ValueError, match="fit int32"):
        big = dev(g["seg"], torch.int64)
        big[0, 0, 0, 0, 0] = 2 ** 31
        tu().seg_to_affgraph_3d_multi_torch(big, nhood, "cuda")
    with pytest.raises(ValueError, match="46340"):
        tu().seg_to_affgraph_3d_torch(dev(np.full((1, 2, 3, 4), 46341, dtype=np.int32)), g["nhood"], "cuda")


def test_a_changed_nhood_tensor_is_seen():
    """the converted copy and the halo kept on a device nhood follow the tensor's version"""
    g = load("d3_thin")
    seg, nhood = dev(g["seg"]), dev(g["nhood"])
    assert same(tu().seg_to_affgraph_3d_multi_torch(seg, nhood, "cuda"), g["aff"].astype(np.float32))
    nhood.mul_(-1)
    assert same(tu().seg_to_affgraph_3d_multi_torch(seg, nhood, "cuda"), tu().gt_affs_dense_host(g["seg"], -g["nhood"]))


def test_output_offsets_past_two_to_the_31():
    """E V = 2200 x 2^20 float16 elements: the last edges lie past element 2^31"""
    import torch
    rng = np.random.default_rng(90)
    seg = make_labels(rng, 1, 1, (64, 128, 128), n=40)
    nhood = rng.integers(-2, 3, size=(2200, 3))
    nhood[-1] = (1, -2, 2)
    assert len(nhood) * seg[0, 0].size > 2 ** 31
    out = tu().seg_to_affgraph_3d_multi_torch(dev(seg), nhood, "cuda", out_dtype=torch.float16, check=False)
    assert out.numel() > 2 ** 31
    for e in (0, 1023, 2047, 2048, 2198, 2199):
        want = tu().gt_affs_dense_host(seg, nhood[e:e + 1])[:, 0]
        assert want.any() and np.array_equal(out[:, e].float().cpu().numpy(), want), e
    del out
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------
# the predicate is ppp_eval_patch's G
# ---------------------------------------------------------------------------------------------
def test_num_gt_of_eval_patch_is_the_sum_of_G_outside_the_overlap():
    """ppp_eval_patch takes ids >= 0 (a negative value is background there), G takes every non-zero value as an
    id: the negative id of batch item 1 is renamed to an unused positive one for BOTH, which changes no
    equality -- asserted: G of the renamed labels is G of the golden's."""
    import torch
    g = load("d3_multi")
    seg = g["seg"].copy()
    assert (seg < 0).any() and not (seg == 5005).any()
    seg[seg < 0] = 5005
    nhood = g["nhood"]
    G = tu().seg_to_affgraph_3d_multi_torch(dev(seg), nhood, "cuda")
    assert same(G, g["aff"].astype(np.float32))
    G = G.cpu().numpy() > 0
    for b in range(seg.shape[0]):
        ov = (seg[b] > 0).sum(axis=0) > 1
        assert ov.any()
        counts = torch.zeros(3, dtype=torch.int64, device="cuda")
        pred = torch.zeros((125,) + seg.shape[2:], dtype=torch.float32, device="cuda")
        be().eval_patch(pred, dev(seg[b]), (5, 5, 5), 0, [0.5], counts)
        num_gt, num_pred, tp = counts.cpu().tolist()
        assert (num_pred, tp) == (0, 0)
        assert num_gt == int((G[b] & ~ov[None]).sum()) and num_gt > 0


# ---------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------
def test_abi_symbols_and_argument_codes():
    L = ctypes.CDLL(be().library_path())
    for name in ("ppp_gt_affs_dense", "ppp_gt_affs_samples", "ppp_gt_affs_dense_plan"):
        assert hasattr(L, name)
    argument_codes()
    # with a device: a NULL or misaligned pointer is refused, and N = 0 succeeds with NULL rows
    import torch
    seg = torch.zeros((1, 1, 4, 5, 6), dtype=torch.int32, device="cuda")
    nhood = torch.zeros((1, 3), dtype=torch.int32, device="cuda")
    out = torch.empty((1, 1, 4, 5, 6), dtype=torch.float32, device="cuda")
    i3, i6 = (ctypes.c_int32 * 3), (ctypes.c_int32 * 6)
    lib = be().lib()
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    args = lambda o: (p(seg), 1, 1, i3(4, 5, 6), p(nhood), 1, i6(0, 0, 0, 0, 0, 0), i6(0, 4, 0, 5, 0, 6), o, 0, 0, None)
    assert lib.ppp_gt_affs_dense(*args(p(out, 2))) == -1 and b"misaligned" in lib.ppp_last_error()
    assert lib.ppp_gt_affs_dense(*args(p(out))) == 0
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0
    assert lib.ppp_gt_affs_samples(p(seg), 1, 1, i3(4, 5, 6), None, 0, p(nhood), 1, i3(1, 1, 1), i3(0, 0, 0), None, 0, None) == 0
