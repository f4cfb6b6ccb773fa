"""The flag matrix (tests/flag_matrix_cases.py) is worth running: its table covers the flag space, both parameter
translations accept and agree on every set, the oracle tells every two sets apart that a stage should tell apart,
and the inputs hold the values and populations the GPU cells rely on.  CPU only."""
import itertools

import numpy as np
import pytest

import flag_matrix_cases as fm
from oracle import ppp_oracle as orc

SMALL = ("p3", "p5", "w11")       # the shapes at which the oracle runs every flag set here


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _side(th):
    return "below" if th < 0.5 else ("equal" if th == 0.5 else "above")


def test_table_covers_the_flag_space():
    names = list(fm.FLAG_SETS)
    assert 12 <= len(names) <= 20 and len(set(names)) == len(names)
    G = {n: fm.geo_flags(n) for n in names}
    # every value of every flag that reaches Geo
    assert {g["value_rule"] for g in G.values()} == {orc.VAL_COUNT, orc.VAL_PROB_PRODUCT, orc.VAL_NORM_PROB_PRODUCT}
    assert {g["bg_rule"] for g in G.values()} == {orc.BG_INV_TH, orc.BG_HALF_TH, orc.BG_LESS_THAN_TH}
    for flag in ("use_overlap", "normalise", "norm_rank", "count_pos_neg", "norm_aff"):
        assert {g[flag] for g in G.values()} == {0, 1}, flag
    # every background rule (as the reference's switches name it) with th below / equal to / above 0.5
    have = {(fm.FLAG_RULES[n][0], _side(G[n]["th"])) for n in names}
    assert have == set(itertools.product(("less", "inv", "half"), ("below", "equal", "above")))
    # ... and with every value rule
    have = {fm.FLAG_RULES[n] for n in names}
    assert have == set(itertools.product(("less", "inv", "half"), ("norm_prob", "prob", "count")))
    # every norm switch off under every value rule (counted votes are never normalised: nothing to switch there)
    for val, rule in (("norm_prob", orc.VAL_NORM_PROB_PRODUCT), ("prob", orc.VAL_PROB_PRODUCT), ("count", orc.VAL_COUNT)):
        for flag in ("normalise", "norm_rank", "norm_aff"):
            assert any(g["value_rule"] == rule and g[flag] == 0 for g in G.values()), (val, flag)
    assert all(g["normalise"] == 0 for g in G.values() if g["value_rule"] == orc.VAL_COUNT)
    # both directions of rounding the threshold to float32
    ths = {g["th"] for g in G.values()}
    assert any(float(np.float32(t)) > t for t in ths) and any(float(np.float32(t)) < t for t in ths)
    # ... and of the background threshold (rounded the other way: where (float)bg < bg, "v < bg" holds for v = (float)bg)
    bgs = {g["bg"] for g in G.values()}
    assert any(float(np.float32(t)) > t for t in bgs) and any(float(np.float32(t)) < t for t in bgs)
    # the sets the packed kernel serves / refuses, the TH05 variant with bg below and at 0.5
    assert sum(fm.v3_serves(n) for n in names) >= 6 and sum(not fm.v3_serves(n) for n in names) >= 6
    assert any(fm.th05_variant(n) and not fm.v3_serves(n) for n in names)
    assert fm.v3_serves("inv05") and fm.s1_key("inv05") == fm.s1_key("default")


@pytest.mark.parametrize("name", list(fm.FLAG_SETS))
def test_both_parameter_translations_agree(name):
    from patchperpix_amd import backend
    for shape_name, (ps, vol, _, _) in fm.SHAPES.items():
        kw = fm.FLAG_SETS[name]
        Po, Pb = orc.make_params(vol, ps, **kw), backend.make_params(vol, ps, **kw)
        for f in ("Z", "Y", "X", "pz", "py", "px", "th", "thi", "bg_rule", "value_rule", "use_overlap", "norm_rank",
                  "count_pos_neg", "norm_aff"):
            assert getattr(Po, f) == getattr(Pb, f), (shape_name, f)
        assert (orc.BG_INV_TH, orc.BG_HALF_TH, orc.BG_LESS_THAN_TH, orc.VAL_COUNT, orc.VAL_PROB_PRODUCT,
                orc.VAL_NORM_PROB_PRODUCT) == (backend.BG_INV_TH, backend.BG_HALF_TH, backend.BG_LESS_THAN_TH,
                                               backend.VAL_COUNT, backend.VAL_PROB_PRODUCT, backend.VAL_NORM_PROB_PRODUCT)
        assert Pb.normalise == (1 if kw["consensus_norm_aff"] else 0) == fm.geo_flags(name)["normalise"]
        assert Pb.pred_clean == 0 and Pb.cons_layout == backend.CONS_COMPACT
        assert (Po.oz, Po.oy, Po.ox) == (Pb.origin_z, Pb.origin_y, Pb.origin_x) == (0, 0, 0)


@pytest.mark.parametrize("dtype", fm.DTYPES)
def test_pinned_values_sit_on_both_sides_of_the_thresholds(dtype):
    for name in fm.FLAG_SETS:
        g = fm.geo_flags(name)
        pins = [float(v) for v in fm.pinned_values(name, dtype)]
        assert 0.0 in pins and 1.0 in pins and all(0.0 <= v <= 1.0 for v in pins)
        for t in (g["th"], g["bg"]):
            a = [float(v) for v in fm.around(t, dtype)]
            assert all(float(fm.to_dtype(np.array([v], dtype=np.float32), dtype)[0]) == v for v in a)      # representable
            below, above = [v for v in a if v < t], [v for v in a if v > t]
            assert below and above and (len(a) == 4 or t in a)
            # adjacent values of the format: nothing representable lies between them
            for lo, hi in zip(a, a[1:]):
                assert float(fm._step(np.float32(lo), dtype, True)) == hi
        if dtype == "float32":
            for t in (g["th"], g["bg"]):
                f = np.float32(t)
                assert {float(f), float(np.nextafter(f, np.float32(2))), float(np.nextafter(f, np.float32(-1)))} <= set(pins)


@pytest.mark.parametrize("shape_name", list(fm.SHAPES))
def test_inputs_hold_the_populations(shape_name):
    b = fm.base_case(shape_name)
    ps = b["ps"]
    inner = fm.interior_mask(shape_name)
    mid_ch = int(np.prod(ps)) // 2
    assert np.count_nonzero(b["overlap"][inner]) > 0 and b["overlap"].dtype == np.uint8
    for dtype in fm.DTYPES:
        seen = set()
        for name in fm.FLAG_SETS:
            pins = tuple(float(v) for v in fm.pinned_values(name, dtype))
            if pins in seen:                   # (the prediction of a cell depends on its pinned values only)
                continue
            seen.add(pins)
            pred = fm.prediction(shape_name, name, dtype)
            assert pred.dtype == np.float32 and np.isfinite(pred).all() and pred.min() >= 0 and pred.max() <= 1
            assert np.array_equal(_bits(pred), _bits(fm.to_dtype(pred, dtype)))
            mid, rest = pred[mid_ch], np.delete(pred, mid_ch, axis=0) if pred.shape[0] < 200 else pred[:mid_ch]
            for v in pins:
                in_mid = np.count_nonzero(mid[inner] == np.float32(v))
                assert in_mid >= 20, (name, dtype, v, in_mid)
                assert np.count_nonzero(rest == np.float32(v)) >= 20, (name, dtype, v)
    # the pair list: whole groups, self rows, far rows, one patch with more than 64 partner rows
    pairs = b["pairs"]
    assert 2000 <= len(pairs) <= 20000 and pairs.dtype == np.uint32
    A = pairs[:, :3].astype(np.int64)
    _, per_patch = np.unique((A[:, 0] * b["vol"][1] + A[:, 1]) * b["vol"][2] + A[:, 2], return_counts=True)
    assert per_patch.max() > 64 + 1                         # (+ its self row)
    assert np.count_nonzero((pairs[:, :3] == pairs[:, 3:]).all(axis=1)) == len(b["selected"])
    d = np.abs(pairs[:, :3].astype(np.int64) - pairs[:, 3:].astype(np.int64))
    far = (d >= 2 * np.array(ps) - 1).any(axis=1)            # windows that share no stored consensus offset
    assert np.count_nonzero(far) >= 5
    o = fm.oracle(shape_name, "default")
    assert np.count_nonzero(o["score"] > 0) >= 100
    assert np.count_nonzero(o["aff"] != 0) >= 500
    assert not o["aff"][far].any() and np.count_nonzero(o["aff"][~far]) >= 500


@pytest.mark.parametrize("shape_name", SMALL)
def test_the_oracle_tells_the_flag_sets_apart(shape_name):
    """For every two flag sets that differ in a flag a stage reads, that stage's oracle output differs in its bits:
    a kernel that ignored the flag could not pass both cells.  (Every stage from its own set's earlier stages.)"""
    b = fm.base_case(shape_name)
    names = list(fm.FLAG_SETS)
    out = {n: fm.oracle(shape_name, n) for n in names}
    for n in names:
        assert np.count_nonzero(out[n]["score"] > 0) >= 100, n
        assert np.count_nonzero(out[n]["aff"] != 0) >= 500, n
    for m, n in itertools.combinations(names, 2):
        same_input = fm.pinned_values(m, "float32") == fm.pinned_values(n, "float32")
        if fm.s1_key(m) != fm.s1_key(n):
            assert out[m]["cons_hash"] != out[n]["cons_hash"], (m, n)
        else:
            assert out[m]["cons_hash"] == out[n]["cons_hash"], (m, n)
        if fm.s2_key(m) != fm.s2_key(n):
            assert not np.array_equal(_bits(out[m]["score"]), _bits(out[n]["score"])), (m, n)
        if fm.s5_key(m) != fm.s5_key(n):
            assert not np.array_equal(_bits(out[m]["aff"]), _bits(out[n]["aff"])), (m, n)
        if same_input and (fm.s1_key(m), fm.s2_key(m), fm.s5_key(m)) == (fm.s1_key(n), fm.s2_key(n), fm.s5_key(n)):
            assert np.array_equal(_bits(out[m]["score"]), _bits(out[n]["score"]))
            assert np.array_equal(_bits(out[m]["aff"]), _bits(out[n]["aff"]))
    # the values that make the rounding direction of the kernels' two float compares visible are there
    for n in ("inv03", "less06_count", "half09_count"):
        g = fm.geo_flags(n)
        pred = fm.prediction(shape_name, n)
        for t in (g["th"], g["bg"]):
            if float(np.float32(t)) != t:                 # the value a float compare against (float)t classifies differently
                assert np.count_nonzero(pred == np.float32(t)) >= 40
    # the serial scatter form and the gather form of the oracle's S1 are the same array
    for n in ("default", "half03_prob", "less06_count", "inv09_count_int"):
        pred = fm.prediction(shape_name, n)
        serial = orc.consensus(pred, b["overlap"], b["ps"], **fm.FLAG_SETS[n])
        assert fm.bits_hash(orc.positive_planes(serial, b["ps"])) == out[n]["cons_hash"], n
        if shape_name == "p3":
            planes = fm.oracle_cons_planes(shape_name, n)
            vm = fm.voxel_major_from_planes(planes, b["ps"])
            W = vm.shape[-1]
            assert np.array_equal(np.moveaxis(vm[..., W // 2 + 1:], -1, 0), planes) and not vm[..., W // 2].any()
            # entry -q of voxel v is entry +q of voxel v - q
            q, L = (1, -2, 1), (1 * 5 + -2) * 5 + 1
            assert np.array_equal(vm[1:, :-2, 1:, W // 2 - L], vm[:-1, 2:, :-1, W // 2 + L])
