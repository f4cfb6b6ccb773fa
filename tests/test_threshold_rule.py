"""CPU: the covering conditions of tests/threshold_cases.py, so that a thinned-out case table cannot hide a failure of
tests/test_threshold_consumers_gpu.py, and the oracle's own compare under the installed NumPy.

"Differ" means not equal; one differing entry is enough for the cover, the thinning and the paint.  Each consumer is
held on the cells its GPU test runs: bits on every shape, cover and thinning on COVER_CELLS (fc_threshold), pack scan
and paints on PAINT_CELLS (patch_threshold)."""
import numpy as np
import pytest

import threshold_cases as tc
from oracle import ppp_oracle as orc

MIN_BITS = 24


def _popcount(a):
    return int(np.unpackbits(np.ascontiguousarray(a).view(np.uint8)).sum())


def _f32(cells):
    return [c for c in cells if c[2] == "float32"]


def test_the_pairs_are_what_they_are_for():
    d = tc.discriminates
    assert [d(t) for t in (0.3, 0.4, 0.6, 0.8)] == [True] * 4 and [d(t) for t in (0.5, 0.7, 0.9)] == [False] * 3
    assert tc.PAIRS == [(0.6, 0.3), (0.3, 0.6), (0.4, 0.4), (0.5, 0.3), (0.7, 0.5)] and tc.CONTROL == tc.PAIRS[-1]
    assert not d(tc.CONTROL[0]) and not d(tc.CONTROL[1])
    assert sum(th != fc and d(th) and d(fc) for th, fc in tc.PAIRS) >= 2          # a consumer reading the other threshold
    for cells in (tc.BITS_CELLS, tc.PAINT_CELLS, tc.E2E_CELLS):
        assert {c[1] for c in _f32(cells)} == set(tc.PAIRS)
        assert {c[2] for c in cells} == set(tc.DTYPES)
    assert {c[0] for c in tc.BITS_CELLS} == set(tc.SHAPES)
    assert {c[1][1] for c in tc.COVER_CELLS} == {0.3, 0.6} and {c[0] for c in tc.COVER_CELLS} == set(tc.COVER_SHAPES)
    for s in tc.COVER_SHAPES:
        assert len({c[2] for c in tc.COVER_CELLS if c[0] == s}) == 2              # float32 and one 16-bit type
    for ps, vol, _, _ in tc.SHAPES.values():
        assert vol[2] % 64 != 0 and all(v >= p for v, p in zip(vol, ps))


@pytest.mark.parametrize("cell", tc.BITS_CELLS, ids=tc.cell_id)
def test_the_predictions_hold_the_values_around_both_thresholds(cell):
    s, pair, dtype = cell
    pred = tc.prediction(s, pair, dtype)
    C = pred.shape[0]
    for t in pair:
        vals = tc.around(t, dtype)
        assert any(float(v) <= t for v in vals) and any(float(v) >= t for v in vals)
        if dtype == "float32":
            f = np.float32(t)
            assert {float(f), float(np.nextafter(f, np.float32(0))), float(np.nextafter(f, np.float32(1)))} <= {float(v) for v in vals}
        for v in vals:
            assert np.count_nonzero(pred == v) >= MIN_BITS and np.count_nonzero(pred[C // 2] == v) >= 1, (t, v)


@pytest.mark.parametrize("cell", _f32(tc.BITS_CELLS), ids=tc.cell_id)
def test_float32_bits_split_the_two_rules(cell):
    s, pair, _ = cell
    fc = pair[1]
    pred = tc.prediction(s, pair)
    b = tc.base_case(s)
    centres = orc.interior_fg_coords(b["foreground"], np.array([p // 2 for p in b["ps"]]))
    split_all = _popcount(tc.packed_bits(pred, fc) ^ tc.packed_bits(pred, fc, rule=tc.F64))
    split = _popcount(tc.packed_bits(pred, fc, centres) ^ tc.packed_bits(pred, fc, centres, rule=tc.F64))
    if tc.discriminates(fc):
        assert split >= MIN_BITS and split_all >= split
    else:
        assert split_all == 0


@pytest.mark.parametrize("cell", [c for c in tc.BITS_CELLS if c[2] != "float32"], ids=tc.cell_id)
def test_16_bit_cells_split_the_widened_and_the_narrowed_compare(cell):
    """A compare in the storage type rounds the threshold to that type first.  That moves a result only where the
    rounded threshold lies above float32(t) -- the value equal to it is then "above" widened and "not above"
    narrowed; a threshold rounded down, or exact, leaves every result as it is (float16: 0.4, 0.5; bfloat16: 0.5).
    Every 16-bit cell of the table is of the first kind."""
    s, pair, dtype = cell
    fc = pair[1]
    assert float(tc.to_dtype(np.array([fc], np.float32), dtype)[0]) > float(np.float32(fc)), "a cell that cannot tell"
    pred = tc.prediction(s, pair, dtype)
    assert _popcount(tc.packed_bits(pred, fc) ^ tc.narrowed_bits(pred, fc, dtype)) >= MIN_BITS


@pytest.mark.parametrize("cell", _f32(tc.COVER_CELLS) + [(s, tc.CONTROL, "float32") for s in tc.COVER_SHAPES], ids=tc.cell_id)
def test_cover_and_thinning_split_the_two_rules(cell):
    s, pair, _ = cell
    a, b = tc.cover(s, pair), tc.cover(s, pair, rule=tc.F64)
    ta, tb = tc.thinned(s, pair), tc.thinned(s, pair, rule=tc.F64)
    assert len(a) >= 3 and len(ta) >= 3
    if tc.discriminates(pair[1]):
        assert not np.array_equal(a, b) and not np.array_equal(ta, tb)
    else:
        assert np.array_equal(a, b) and np.array_equal(ta, tb)
    # the ladder of pixel thresholds and the marks select other patches than the sparse cover: variants worth running
    assert not np.array_equal(tc.cover(s, pair, sparse=False), a) and not np.array_equal(tc.cover(s, pair, mark=True), a)


@pytest.mark.parametrize("cell", _f32(tc.PAINT_CELLS), ids=tc.cell_id)
def test_paint_splits_the_two_rules(cell):
    s, pair, _ = cell
    th = pair[0]
    b = tc.base_case(s)
    pred, ccs = tc.prediction(s, pair), tc.components(s, pair)
    ma = tc.component_masks(ccs, pred, b["ps"], b["vol"], th)
    mb = tc.component_masks(ccs, pred, b["ps"], b["vol"], th, rule=tc.F64)
    differ = bool((tc.paint_model(ma) != tc.paint_model(mb)).any())
    assert differ == tc.discriminates(th)
    assert np.array_equal(tc.pack_scan_model(ma)[0], tc.pack_scan_model(mb)[0]) != tc.discriminates(th)


@pytest.mark.parametrize("cell", tc.PAINT_CELLS, ids=tc.cell_id)
def test_paint_and_pack_cases_are_not_quiet_ones(cell):
    """by the oracle alone: components that share voxels, one above and one below the packing's size limit"""
    from patchperpix_amd import backend
    s, pair, dtype = cell
    b = tc.base_case(s)
    pred, ccs = tc.prediction(s, pair, dtype), tc.components(s, pair, dtype)
    assert all(len(cc) for cc in ccs)
    own = [orc.paint_instances([cc], pred, b["ps"], b["vol"], pair[0]) > 0 for cc in ccs]
    sizes = [int(m.sum()) for m in own]
    assert max(sizes) > backend.PACK_MIN_VOXELS and 0 < min(sizes) < backend.PACK_MIN_VOXELS
    assert sum(bool((own[i] & own[j]).any()) for i in range(len(own)) for j in range(i)) >= 2
    big = int(np.argmax(sizes))
    assert any(sizes[k] < backend.PACK_MIN_VOXELS and (own[k] & own[big]).any() for k in range(big + 1, len(own)))   # a small one painted over the large one
    # the face nodes of the paint from rows: one on every face, windows that leave the volume
    Z, Y, X = b["vol"]
    nodes = np.array([n for n, _ in tc.face_nodes(s)])
    for a, size in enumerate((Z, Y, X)):
        assert (nodes[:, a] == 0).any() and (nodes[:, a] == size - 1).any()


@pytest.mark.parametrize("cell", _f32(tc.COVER_CELLS)[:6] + [("p5", tc.CONTROL, "float32")], ids=tc.cell_id)
def test_oracle_cover_and_thinning_compare_in_float32(cell):
    """The oracle writes `patch > fc` with a Python float.  A prediction already classified by the explicit
    np.float32(fc) compare (values 0 / 1, on which every promotion rule agrees) must give the same selections: a
    change of NumPy's scalar promotion cannot move the oracle silently."""
    s, pair, _ = cell
    b = tc.base_case(s)
    fc = pair[1]
    rc, rs = tc.ranked(s, pair)
    explicit = (tc.prediction(s, pair) > np.float32(fc)).astype(np.float32)
    for over in (dict(), dict(select_patches_for_sparse_data=False), dict(mark_close_neighboorhood=True)):
        kw = tc.flags(pair, **dict(dict(select_patches_for_sparse_data=True, mark_close_neighboorhood=False), **over))
        want = orc.foreground_cover(rc, rs, b["overlap"], tc.mask_to_cover(s), explicit, b["ps"], **kw)
        assert np.array_equal(tc.cover(s, pair, sparse=kw["select_patches_for_sparse_data"], mark=kw["mark_close_neighboorhood"]), want)
    sel = rc[tc.cover(s, pair)]
    assert np.array_equal(tc.thinned(s, pair), orc.thin_cover(sel, tc.mask_to_cover(s), explicit, b["ps"], **tc.flags(pair)))


@pytest.mark.parametrize("cell", _f32(tc.PAINT_CELLS), ids=tc.cell_id)
def test_oracle_paints_compare_in_float32(cell):
    from patchperpix_amd import backend
    s, pair, _ = cell
    th = pair[0]
    b = tc.base_case(s)
    pred, ccs = tc.prediction(s, pair), tc.components(s, pair)
    masks = tc.component_masks(ccs, pred, b["ps"], b["vol"], th)          # (interior nodes: no window is clipped)
    assert np.array_equal(orc.paint_instances(ccs, pred, b["ps"], b["vol"], th), tc.paint_model(masks))
    want = tc.channels_model(masks, backend.PACK_MIN_VOXELS)
    got = orc.paint_per_channel(ccs, pred, b["ps"], b["vol"], th, packed=True)
    assert want.shape[0] >= 2 and got.shape == want.shape and np.array_equal(got, want)
    each = orc.paint_per_channel(ccs, pred, b["ps"], b["vol"], th, packed=False)
    assert np.array_equal(each > 0, masks)


def test_clipped_paint_model_on_face_nodes():
    """the explicit model clips a window at the faces; plain slices (the oracle's) wrap at a negative start instead"""
    s, pair = "p5", (0.6, 0.3)
    b = tc.base_case(s)
    pred = tc.prediction(s, pair)
    (node, _), = [f for f in tc.face_nodes(s) if f[0] == (0, 0, 0)]
    m = tc.component_masks([[node]], pred, b["ps"], b["vol"], pair[0])[0]
    r = [p // 2 for p in b["ps"]]
    want = (pred[:, 0, 0, 0] > np.float32(pair[0])).reshape(b["ps"])[r[0]:, r[1]:, r[2]:]
    assert want.any() and np.array_equal(m[:r[0] + 1, :r[1] + 1, :r[2] + 1], want) and m.sum() == want.sum()


@pytest.mark.parametrize("cell", tc.E2E_CELLS, ids=tc.cell_id)
@pytest.mark.parametrize("mws", [False, True])
def test_end_to_end_cases_have_instances(mws, cell):
    ref = tc.e2e_expected(*cell, mws)
    assert tc.n_instances(ref["instances"]) >= tc.MIN_INSTANCES and len(ref["pairs"]) and (ref["aff"] != 0).any()


@pytest.mark.parametrize("mws", [False, True])
def test_stack_case_has_instances_in_every_slice(mws):
    for ref in tc.stack_expected(mws):
        assert tc.n_instances(ref["instances"]) >= tc.MIN_INSTANCES
    a, b, _ = tc.stack_expected(mws)
    assert not np.array_equal(a["instances"], b["instances"][..., ::-1])          # three images, not one three times
