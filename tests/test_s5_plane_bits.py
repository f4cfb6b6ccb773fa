"""The plane values of patch B in the cubic small-chunk S5 kernels (csrc/ppp_patch_graph_pa.hip, pa_b_in_regs:
3^3, 5^3, 7^3 and 9^3 with the small chunk keep the foreground bits of a lane's patch B as values per
candidate plane in registers, made once per pair row by pa_plane_bits, instead of bit words in LDS: one
64-bit value per plane up to 7^3; at 9^3 a plane is two chunks of candidate rows, rows 0-6 and rows 7-8).

CPU: the extraction function through its host entry ppp_patch_plane_bits against a NumPy restatement, on
random bit words with random bits behind the patch's last bit as well: every plane, those whose bits lie in
two and in three words (5^3: planes start at bit 25 z, 7^3: at bit 49 z, 9^3: at bit 81 z), and the last
plane, which ends before the last word does.

GPU: aff as uint32 bit patterns, cubic kernel == run-time instantiation (PPP_PA_CUBE=0, bits in LDS: the
in-library cross-check) == oracle, on the pair lists of test_s5_cube.py (patches A with 300, 70, 40 and 10
rows: several chunks, idle lanes in the last one; intersecting pairs, pairs apart, a pair at |d| = 2 p - 2),
for two kinds of prediction: the generator's cells as wide as the patch, and per-channel, per-voxel random
values of which half exceed the threshold -- every plane of every B has its own bits -- with the centre
channel cleared in the lowest quarter of the volume, so that patches B with whole background planes occur.
Each through backend.patch_graph_prepare / patch_graph_by_patch with the small chunk, the bits from the
table and built in the kernel, and masks for all intersecting rows, for none, for the first batch only."""
import ctypes

import numpy as np
import pytest

from test_s5_cube import ROW_COUNTS, _check_plan, _env, list_properties, mask_budget_for_first_group, pair_rows

# patch width: volume, seed
CUBES = {3: ((16, 16, 16), 31), 5: ((16, 16, 16), 32), 7: ((24, 24, 24), 33), 9: ((28, 28, 28), 34)}
KINDS = ("cells", "random")


def chunk_rows(p):
    """candidate rows of a plane per 64-bit chunk: the whole plane up to 7^3, 7 + 2 rows at 9^3"""
    rpc = min(64 // p, p)
    return [rpc] if rpc == p else [rpc, p - rpc]


def planes_np(words, p):
    """the bit string in `words` (uint32, bit r = bit r & 31 of word r >> 5) cut into the chunks of its
    planes, as Python integers: [chunk][plane] flattened -- value c * p + z holds the rows of chunk c of
    plane z, bits [z p^2 + first row * p, ... + rows * p)"""
    bits = ((words[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).ravel()
    out, first = [], 0
    for rows in chunk_rows(p):
        for z in range(p):
            o = z * p * p + first * p
            out.append(sum(int(b) << i for i, b in enumerate(bits[o:o + rows * p])))
        first += rows
    return out


def plane_bits(words, p):
    from patchperpix_amd import backend
    words = np.ascontiguousarray(words, dtype=np.uint32)
    out = np.zeros(p * len(chunk_rows(p)), dtype=np.uint64)
    backend.check(backend.lib().ppp_patch_plane_bits(words.ctypes.data, len(words), p, out.ctypes.data))
    return [int(v) for v in out]


@pytest.mark.parametrize("p", sorted(CUBES))
def test_plane_extraction_equals_numpy(p):
    n_words = (p ** 3 + 31) // 32
    rows0 = chunk_rows(p)[0]
    spans = [(z * p * p + rows0 * p - 1) // 32 - (z * p * p) // 32 + 1 for z in range(p)]   # words a value's bits lie in
    assert max(spans) == {3: 1, 5: 2, 7: 3, 9: 3}[p]
    assert p ** 3 < 32 * n_words                             # the last plane ends before the last word does
    rng = np.random.default_rng(100 + p)
    cases = [rng.integers(0, 1 << 32, size=n_words, dtype=np.uint64).astype(np.uint32) for _ in range(200)]
    cases += [np.zeros(n_words, np.uint32), np.full(n_words, 0xFFFFFFFF, np.uint32)]
    # one bit at a time: the first and last bit of every plane and of its first chunk, the first bit behind the patch
    for r in sorted({z * p * p for z in range(p)} | {(z + 1) * p * p - 1 for z in range(p)} | {p ** 3} |
                    {z * p * p + rows0 * p - 1 for z in range(p)} | {(z * p * p + rows0 * p) % p ** 3 for z in range(p)}):
        w = np.zeros(n_words, np.uint32)
        w[r >> 5] = np.uint32(1) << np.uint32(r & 31)
        cases.append(w)
    for w in cases:
        want = planes_np(w, p)
        assert all(v < (1 << (rows0 * p)) for v in want)
        assert plane_bits(w, p) == want, (p, w)
    # all ones: every plane is full, nothing of the bits behind the patch shows
    assert plane_bits(cases[201], p) == [(1 << (rows * p)) - 1 for rows in chunk_rows(p) for _ in range(p)]


def test_plane_extraction_refuses_other_shapes():
    from patchperpix_amd import backend
    L = backend.lib()
    w = np.zeros(23, np.uint32)
    out = np.zeros(18, np.uint64)
    assert L.ppp_patch_plane_bits(w.ctypes.data, 23, 11, out.ctypes.data) != 0      # no such kernel
    assert L.ppp_patch_plane_bits(w.ctypes.data, 22, 9, out.ctypes.data) != 0       # 9^3 has 23 words
    assert L.ppp_patch_plane_bits(w.ctypes.data, 23, 9, out.ctypes.data) == 0
    assert L.ppp_patch_plane_bits(w.ctypes.data, 10, 7, out.ctypes.data) != 0       # 7^3 has 11 words
    assert L.ppp_patch_plane_bits(None, 11, 7, out.ctypes.data) != 0
    assert L.ppp_patch_plane_bits(w.ctypes.data, 11, 7, out.ctypes.data) == 0


def random_pred(shape, ps, seed):
    """float32 [C, Z, Y, X], multiples of 1 / 1024 (float16 holds them), half of them above 0.5; the centre
    channel cleared for z < Z / 4: the windows that reach down there have whole background planes"""
    rng = np.random.default_rng(seed)
    C = int(np.prod(ps))
    pred = (rng.integers(0, 1024, size=(C,) + tuple(shape)) / 1024.0).astype(np.float32)
    pred[C // 2, :shape[0] // 4] = 0.0
    return pred


def b_plane_counts(pred, rows, ps, th=0.5):
    """[rows, pz]: foreground bits per candidate plane of every row's patch B (the kernel's expression:
    centre channel at the window voxel above th and the patch's own channel at B above th)"""
    C = int(np.prod(ps))
    r = [p // 2 for p in ps]
    mid = pred[C // 2] > th
    out = np.zeros((len(rows), ps[0]), dtype=np.int64)
    for i, (bz, by, bx) in enumerate(rows[:, 3:]):
        win = mid[bz - r[0]:bz + r[0] + 1, by - r[1]:by + r[1] + 1, bx - r[2]:bx + r[2] + 1]
        own = pred[:, bz, by, bx].reshape(ps) > th
        out[i] = (win & own).sum(axis=(1, 2))
    return out


@pytest.mark.parametrize("p", sorted(CUBES))
def test_random_predictions_hold_the_cases(p):
    """host arithmetic only: what the comparison below relies on for the random predictions"""
    shape, seed = CUBES[p]
    ps = (p, p, p)
    rows = pair_rows(shape, ps, ROW_COUNTS, np.random.default_rng(seed))
    props = list_properties(rows, ps)
    assert props["largest_group"] > 256 and props["intersecting"] >= 30 and props["apart"] >= 30
    assert props["at_largest_offset"] >= 1
    counts = b_plane_counts(random_pred(shape, ps, seed), rows, ps)
    empty, full = (counts == 0).any(axis=1), (counts > 0).any(axis=1)
    assert (empty & full).sum() >= 10                        # patches B with whole background planes beside others
    assert (counts > 0).all(axis=1).sum() >= 10              # and patches B with bits on every plane
    # the planes of a patch differ: no constant fill could stand in for them
    assert (counts.max(axis=1) != counts.min(axis=1)).sum() >= len(rows) // 2


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert backend.device_count() >= 1
    return torch


class _Case:
    """prediction, consensus, pair rows and the oracle's aff of one patch width and prediction kind"""

    def __init__(self, torch, p, kind):
        from oracle import ppp_oracle as orc
        from patchperpix_amd import backend, synth
        from tests_flags import FLYLIGHT
        shape, seed = CUBES[p]
        self.ps = ps = (p, p, p)
        kw = dict(FLYLIGHT)
        self.rows = rows = pair_rows(shape, ps, ROW_COUNTS, np.random.default_rng(seed))
        self.props = list_properties(rows, ps)
        if kind == "cells":
            pred = synth.make_case(shape, ps, seed=seed, cell=[p] * 3, noise=0.3)["pred"]
        else:
            pred = random_pred(shape, ps, seed)
        self.P = P = backend.make_params(shape, ps, **kw)
        self.cut_bytes = mask_budget_for_first_group(rows, ps, P)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
        self.pred = dev(pred)
        self.rows_d = dev(rows)
        cons = backend.consensus(self.pred, torch.zeros(shape, dtype=torch.uint8, device="cuda"), P)
        self.vm, self.Pv = backend.cons_to_voxel_major(cons, P)
        cons_ref = backend.cons_to_reference(cons, P).cpu().numpy()
        del cons
        self.want = orc.patch_graph(pred, cons_ref, rows.view(np.uint32), ps, **kw).view(np.uint32)

    def run(self, torch, cube, table, masks):
        """(aff bits, kernel name, geometry, job) of one pass through the per-patch path, small chunk"""
        from patchperpix_amd import backend
        env = {"PPP_PA_CHUNK": "small", "PPP_PA_BITS": "1" if table else "0"}
        if not cube:
            env["PPP_PA_CUBE"] = "0"
        if masks == "none":
            env["PPP_PA_LCG_BYTES"] = "0"
        elif masks == "cut":
            env.update(PPP_PA_LCG_BYTES=self.cut_bytes, PPP_PA_LCG_BATCHES=1)
        with _env(**env):
            job = backend.patch_graph_prepare(self.pred, self.rows_d, self.Pv)
            aff = backend.patch_graph_by_patch(self.pred, self.vm, self.rows_d, self.Pv, job=job)
            torch.cuda.synchronize()
            name = backend.lib().ppp_patch_graph_kernel_name().decode()
            geometry = backend.lib().ppp_patch_graph_kernel_geometry().decode()
        return aff.cpu().numpy().view(np.uint32), name, geometry, job


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p", sorted(CUBES))
def test_plane_values_equal_lds_bits_equal_oracle(p, kind, torch_cuda):
    from patchperpix_amd import backend
    torch = torch_cuda
    case = _Case(torch, p, kind)
    props = case.props
    small = int(backend.lib().ppp_patch_graph_by_patch_chunk_small(ctypes.byref(case.Pv)))
    assert small == (128 if p == 9 else 64)
    assert props["largest_group"] > 2 * small and props["largest_group"] % small != 0   # several chunks, the last one not full
    assert props["intersecting"] >= 30 and props["apart"] >= 30 and props["at_largest_offset"] >= 1
    assert np.count_nonzero(case.want) > 50
    for table in (True, False):
        for masks in ("all", "none", "cut"):
            what = (p, kind, table, masks)
            got_c, name_c, geo_c, job = case.run(torch, True, table, masks)
            assert (name_c, geo_c) == ("patch_graph_pa_kernel<small>", "cube"), what
            assert job.chunk == small and (job.bits is not None) == table, what
            _check_plan(case, job, masks)
            got_g, name_g, geo_g, _ = case.run(torch, False, table, masks)
            assert (name_g, geo_g) == ("patch_graph_pa_kernel<small>", "generic"), what
            bad = np.nonzero(got_c != case.want)[0]
            assert bad.size == 0, (what, "cubic differs from the oracle", bad[:8], case.rows[bad[:8]])
            bad = np.nonzero(got_g != case.want)[0]
            assert bad.size == 0, (what, "generic differs from the oracle", bad[:8], case.rows[bad[:8]])
            assert np.array_equal(got_c, got_g), what
