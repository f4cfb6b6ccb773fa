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


# ---- the clean variant (tests/test_s1_clean_gpu.py) -----------------------------------------------------------------
SERVED = [n for n in fm.FLAG_SETS if fm.v3_serves(n)]
V3_SHAPES = [s for s in fm.SHAPES if fm.SHAPES[s][0][2] in (3, 5, 7, 9)]


@pytest.mark.parametrize("shape_name", list(fm.SHAPES))
def test_existing_predictions_are_unclean(shape_name):
    """Every existing prediction holds a value the float 0.5 of the packed kernel's class tests calls unclean, and
    every existing cell that kernel serves is unclean under its own thresholds (ppp_pred_check by its model): the
    existing cells of the packed kernel keep running its general classification.  (A set whose threshold no float
    equals -- inv03: 0.3 -- can be clean under its own tests; nothing that serves it reads pred_clean.)"""
    for dtype in fm.DTYPES:
        for name in SERVED + ["half05"]:         # every set with a class test at 0.5
            g = fm.geo_flags(name, shape_name)
            assert 0.5 in (g["th"], g["bg"])
            bits = fm.is_clean(fm.prediction(shape_name, name, dtype), dtype, g["th"], g["bg"])
            assert bits == (3 if shape_name == "p9" else 2), (name, dtype, bits)       # (p9: the one negative zero)
    assert [n for n in fm.FLAG_SETS if 0.5 in (fm.geo_flags(n)["th"], fm.geo_flags(n)["bg"])] == \
        [n for n in fm.FLAG_SETS if n in SERVED + ["half05"]]


def test_the_model_of_the_check_knows_its_classes():
    for dtype in fm.DTYPES:
        up, down = (lambda v: fm._step(np.float32(v), dtype, True)), (lambda v: fm._step(np.float32(v), dtype, False))
        one = lambda v, th=0.5, bg=0.5: fm.is_clean(np.array([0.75, v, 0.125], dtype=np.float32), dtype, th, bg)   # noqa: E731
        for v in (0.0, fm.smallest(dtype)[0], fm.smallest(dtype)[1], down(0.5), up(0.5), down(1.0), 1.0):
            assert one(v) == 0, (dtype, v)
        for v in (up(1.0), 2.0, np.inf, -0.0, -fm.smallest(dtype)[0], -1.0, -np.inf):
            assert one(v) == 1, (dtype, v)
        assert one(0.5) == 2 and one(np.nan) == 3 and one(-np.nan) == 3
        assert [one(v, 0.5, 0.25) for v in (down(0.25), 0.25, 0.375, down(0.5), 0.5, up(0.5))] == [0, 2, 2, 2, 2, 0]


@pytest.mark.parametrize("dtype", fm.DTYPES)
def test_clean_pins_are_what_the_short_classification_can_get_wrong(dtype):
    pins = [float(v) for v in fm.clean_pins(dtype)]
    assert len(pins) == 9 <= fm.MAX_PINS and pins == sorted(pins) and 0.5 not in pins
    st = lambda v, up: float(fm._step(np.float32(v), dtype, up))       # noqa: E731
    sub, normal = (float(v) for v in fm.smallest(dtype))
    assert set(pins) == {0.0, sub, normal, st(st(0.5, False), False), st(0.5, False), st(0.5, True),
                         st(st(0.5, True), True), st(1.0, False), 1.0}
    assert 0.0 < sub < normal and st(0.0, True) == sub and st(normal, False) < normal
    man = {"float32": 23, "float16": 10, "bfloat16": 7}[dtype]
    assert st(normal, False) == normal - sub and sub == normal * 2.0 ** -man          # the largest subnormal precedes it
    assert all(float(fm.to_dtype(np.array([v], dtype=np.float32), dtype)[0]) == v for v in pins)      # representable


@pytest.mark.parametrize("shape_name", V3_SHAPES)
def test_clean_predictions_are_clean_and_hold_the_pins(shape_name):
    inner = fm.interior_mask(shape_name)
    mid_ch = int(np.prod(fm.SHAPES[shape_name][0])) // 2
    for dtype in fm.DTYPES:
        pred = fm.prediction(shape_name, "default", dtype, fm.CLEAN)
        for name in SERVED:                     # (one prediction per shape and dtype, whatever the served set)
            assert fm.prediction(shape_name, name, dtype, fm.CLEAN) is pred
            g = fm.geo_flags(name, shape_name)
            assert (g["th"], g["bg"]) == (0.5, 0.5)
        assert fm.is_clean(pred, dtype, 0.5, 0.5) == 0
        assert pred.dtype == np.float32 and not np.signbit(pred).any() and pred.max() <= 1
        assert np.array_equal(_bits(pred), _bits(fm.to_dtype(pred, dtype)))                # narrows exactly
        pat, one = fm.dtype_patterns(pred, dtype)
        assert pat.max() == one
        mid, rest = pred[mid_ch], np.delete(pred, mid_ch, axis=0)        # (rest: every other channel)
        for v in fm.clean_pins(dtype):
            assert np.count_nonzero(mid[inner] == v) >= 20, (dtype, v)
            assert np.count_nonzero(rest == v) >= 20, (dtype, v)
        # apart from the pins (and the sign of zero) it is the existing cells' base prediction
        base = fm.to_dtype(fm.base_case(shape_name)["pred"], dtype)
        same = _bits(pred) == _bits(base)
        assert 0.85 < np.count_nonzero(same) / same.size < 0.95
    with pytest.raises(AssertionError):
        fm.prediction(shape_name, "half05", "float32", fm.CLEAN)          # nothing but the packed kernel reads pred_clean
    # the existing variant keeps its bits: the one negative zero of the 9^3 base included
    neg0 = sum(int(np.count_nonzero(np.signbit(fm.base_case(s)["pred"]))) for s in fm.SHAPES)
    assert neg0 == 1 and np.count_nonzero(np.signbit(fm.base_case("p9")["pred"])) == 1


def _moved(shape_name, dtype, src, dst):
    """the clean-variant hash for `default` with every value src of the prediction replaced by dst"""
    b = fm.base_case(shape_name)
    pred = np.array(fm.prediction(shape_name, "default", dtype, fm.CLEAN))
    assert np.count_nonzero(pred == src) >= 40
    pred[pred == src] = dst
    cons = orc.consensus_planes(pred, b["overlap"], b["ps"], **fm.FLAG_SETS["default"])
    return fm.bits_hash(orc.positive_planes(cons, b["ps"]))


@pytest.mark.parametrize("shape_name", ("p3", "p5", "p357"))
def test_the_neighbours_of_the_threshold_matter(shape_name):
    """A kernel that puts the nearest value below 0.5 on the other side (or the nearest above) cannot pass: the
    oracle's hash changes.  And the four S1 flag keys among the served sets give four hashes."""
    for dtype in fm.DTYPES:
        below, above = fm.around(0.5, dtype)[0], fm.around(0.5, dtype)[2]
        h = fm.oracle(shape_name, "default", dtype, fm.CLEAN)["cons_hash"]
        assert set(fm.oracle(shape_name, "default", dtype, fm.CLEAN)) == {"cons_hash"}      # S1 only
        planes = fm.oracle_cons_planes(shape_name, "default", dtype, fm.CLEAN)
        assert fm.bits_hash(planes) == h and np.count_nonzero(planes) >= 1000
        assert _moved(shape_name, dtype, below, above) != h, (dtype, "below -> above")
        assert _moved(shape_name, dtype, above, below) != h, (dtype, "above -> below")
        by_key = {}
        for name in SERVED:
            by_key.setdefault(fm.s1_key(name), set()).add(fm.oracle(shape_name, name, dtype, fm.CLEAN)["cons_hash"])
        assert len(by_key) == 4 and all(len(v) == 1 for v in by_key.values())
        assert len(set.union(*by_key.values())) == 4
        assert {fm.s1_key(n) for n in ("default", "raw", "noov", "nonorm_s1")} == set(by_key)
        assert fm.oracle(shape_name, "inv05", dtype, fm.CLEAN)["cons_hash"] == h
        # ... and is another array than the existing cell's
        if dtype == "float32":
            assert fm.oracle(shape_name, "default", dtype)["cons_hash"] != h
    # the serial scatter form of the oracle agrees on the clean prediction too
    b = fm.base_case(shape_name)
    serial = orc.consensus(fm.prediction(shape_name, "default", "bfloat16", fm.CLEAN), b["overlap"], b["ps"], **fm.FLAG_SETS["default"])
    assert fm.bits_hash(orc.positive_planes(serial, b["ps"])) == fm.oracle(shape_name, "default", "bfloat16", fm.CLEAN)["cons_hash"]


def test_every_instantiation_of_the_packed_kernel_is_met():
    """consensus_v3_kernel<T, PX, FLAT, CLEAN, dense / lists>: every combination with CLEAN = true meets a cell of
    tests/test_s1_clean_gpu.py, every (PX, FLAT) with CLEAN = false a cell of the existing matrix."""
    import test_flag_matrix_gpu as mg
    import test_s1_clean_gpu as cg
    want = set(itertools.product(fm.DTYPES, (3, 5, 7, 9), (True, False), (False, True)))
    forms = [cg.cell_form(c) for c in cg.CELLS]
    clean = {f[:4] for f in forms if f[4]}
    assert clean == want
    assert len(cg.CELLS) == len(set(cg.CELLS)) and 250 <= len(cg.CELLS) <= 320
    assert all(fm.v3_serves(c[2]) for c in cg.CELLS)
    # the general classification on every clean prediction: every shape, every dtype
    assert {(c[1], c[3]) for c, f in zip(cg.CELLS, forms) if not f[4]} == set(itertools.product(cg.FIVE, fm.DTYPES))
    # the four S1 keys under both dense forms and the lists, in every dtype and at every shape
    keys = {fm.s1_key(n) for n in cg.SERVED}
    assert len(keys) == 4 and {fm.s1_key(n) for n in cg.KEYS} == keys and len(cg.KEYS) == 4 and len(cg.SERVED) == 8
    for fam in ("v3c_flat", "v3c_line", "lists_c"):
        have = {(c[1], c[3], fm.s1_key(c[2])) for c in cg.CELLS if c[0] == fam}
        assert have == set(itertools.product(cg.FIVE, fm.DTYPES, keys)), fam
    assert {c[2] for c in cg.CELLS if c[0] == "v3c_flat" and c[3] == "float32"} == set(cg.SERVED)
    # the boxes that take their form by the rule
    assert {cg.part_form(*c)[1:4] for c in cg.PART_CELLS} == set(itertools.product((5, 7), (True, False), (False,)))
    # CLEAN = false: the existing matrix's cells of the packed kernel (all unclean, see above)
    unclean = set()
    for fam, shape, name, dtype in mg.S1_CELLS:
        if fam in ("v3", "v3_line", "v3_vm", "lists") and fm.v3_serves(name):
            unclean.add((fm.SHAPES[shape][0][2], fm.v3_flat_form(shape, mg.S1[fam]["env"])))
    assert unclean == set(itertools.product((3, 5, 7, 9), (True, False)))
    # ... and its earlier ids are all still there
    assert len(mg.S1_CELLS) == len(set(mg.S1_CELLS))
    assert sum(c[0] == "v3_line" for c in mg.S1_CELLS) == 5 * len(fm.FLAG_SETS) + 4
