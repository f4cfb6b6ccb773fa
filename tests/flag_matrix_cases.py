"""The flag matrix of the S1 / S2 / S5 kernel families: flag sets, shapes, predictions with values pinned
at the thresholds, pair rows and the oracle's stage outputs (plain module, no GPU; imported by
tests/test_flag_matrix_rule.py and tests/test_flag_matrix_gpu.py).

A CELL is (shape name, flag set name, dtype).  Everything here is a pure function of the cell, computed
once per process and shared by all families that meet the cell.

Two VARIANTS of the prediction: "pinned" holds the thresholds themselves (so ppp_pred_check calls it unclean and
the packed S1 kernel classifies in its general form), "clean" holds their neighbours and no value the check
objects to (the short form; S1 outputs only; tests/test_s1_clean_gpu.py)."""
import functools
import hashlib

import numpy as np

from oracle import ppp_oracle as orc
from patchperpix_amd import synth
from tests_flags import FLYLIGHT

DTYPES = ("float32", "float16", "bfloat16")

_BG = {"less": dict(vi_bg_use_less_than_th=True, vi_bg_use_inv_th=False, vi_bg_use_half_th=False),
       "inv": dict(vi_bg_use_less_than_th=False, vi_bg_use_inv_th=True, vi_bg_use_half_th=False),
       "half": dict(vi_bg_use_less_than_th=False, vi_bg_use_inv_th=False, vi_bg_use_half_th=True)}
_VAL = {"norm_prob": dict(consensus_norm_prob_product=True, consensus_prob_product=True),
        "prob": dict(consensus_norm_prob_product=False, consensus_prob_product=True),
        # (the reference asserts: counted votes are never normalised)
        "count": dict(consensus_norm_prob_product=False, consensus_prob_product=False,
                      consensus_norm_aff=False, consensus_interleaved_cnt=False)}


def _set(th=0.5, bg="less", val="norm_prob", **kw):
    return dict(_BG[bg], **_VAL[val], patch_threshold=th, **kw)


# name -> (bg rule, value rule, change from the kernels-only FLYLIGHT set).  Hand-written; the covering
# conditions that keep it from being thinned out are asserted by tests/test_flag_matrix_rule.py.
_TABLE = [
    ("default", "less", "norm_prob", {}),
    ("inv05", "inv", "norm_prob", {}),                     # same arithmetic as default: v3 must still serve
    ("half05", "half", "norm_prob", {}),                   # bg 0.25: v3 refuses, v2's TH05 variant with bg_lt < 0.5
    ("inv03", "inv", "norm_prob", dict(th=0.3)),           # maps to less-than; (float)th > th
    ("half03_prob", "half", "prob", dict(th=0.3, rank_norm_patch_score=False)),
    ("less04_prob", "less", "prob", dict(th=0.4, consensus_norm_aff=False, patch_graph_norm_aff=False)),
    ("less06_count", "less", "count", dict(th=0.6, patch_graph_norm_aff=False)),
    ("inv07_prob_noov", "inv", "prob", dict(th=0.7, overlapping_inst=False)),      # (float)th < th
    ("half09_count", "half", "count", dict(th=0.9, rank_norm_patch_score=False)),           # (float)bg < bg = 0.45
    ("inv09_count_int", "inv", "count", dict(th=0.9, rank_int_counter=True)),
    ("raw", "less", "norm_prob", dict(consensus_norm_aff=False, rank_norm_patch_score=False,
                                      patch_graph_norm_aff=False, overlapping_inst=False)),
    ("int", "less", "norm_prob", dict(rank_int_counter=True)),
    ("noov", "less", "norm_prob", dict(overlapping_inst=False)),
    ("nonorm_s1", "less", "norm_prob", dict(consensus_norm_aff=False)),
    ("nonorm_s2", "less", "norm_prob", dict(rank_norm_patch_score=False)),
    ("nonorm_s5", "less", "norm_prob", dict(patch_graph_norm_aff=False)),
]
FLAG_RULES = {name: (bg, val) for name, bg, val, _ in _TABLE}
FLAG_SETS = {name: dict(FLYLIGHT, **_set(bg=bg, val=val, **kw)) for name, bg, val, kw in _TABLE}

# name -> (patch shape, volume, cell size of the synthetic labels, seed).  The smallest volumes at which the
# families can still go wrong: an x line longer than one 64-lane run and no multiple of 64, interior extents that
# leave ragged 8 x 8 x 8 / 8 x 8 x 16 centre tiles on every axis.
SHAPES = {
    "p3": ((3, 3, 3), (8, 9, 70), [5, 5, 5], 301),
    "p5": ((5, 5, 5), (9, 11, 97), [8, 8, 8], 302),
    "p7": ((7, 7, 7), (13, 15, 75), [9, 9, 9], 303),
    "p9": ((9, 9, 9), (12, 13, 70), [12, 12, 12], 304),
    "p357": ((3, 5, 7), (10, 16, 70), [4, 7, 9], 305),
    "w25": ((1, 25, 25), (1, 40, 90), [1, 30, 30], 306),
    "w11": ((1, 11, 11), (1, 30, 70), [1, 13, 13], 307),
}
MID_PINS = 24          # interior voxels of the mid channel that get each pinned value
PIN_SHARE = 0.01       # share of ALL entries (every channel) that gets each pinned value
# centres of the pair list: a dense cluster (its first patch in x order has more than 64 partners) + a seeded sample
# of the others (far rows); fewer of those where the oracle's S5 costs C^2 = 5 * 10^5 pixel pairs per row
N_CLUSTER = 66
N_SPREAD = {"p3": 50, "p5": 50, "p7": 30, "p9": 20, "p357": 50, "w25": 20, "w11": 50}


# ---- the flags as the kernels see them -----------------------------------------------------------------------------
def geo_flags(name, shape_name="p3"):
    """What reaches Geo for a flag set, read from the oracle's parameter struct (th, bg: the double thresholds of
    the two class tests)."""
    ps, vol, _, _ = SHAPES[shape_name]
    P = orc.make_params(vol, ps, **FLAG_SETS[name])
    bg = {orc.BG_INV_TH: P.thi, orc.BG_HALF_TH: P.th / 2, orc.BG_LESS_THAN_TH: P.th}[P.bg_rule]
    kw = FLAG_SETS[name]
    return dict(th=P.th, bg=bg, bg_rule=P.bg_rule, value_rule=P.value_rule, use_overlap=P.use_overlap,
                normalise=1 if kw.get("consensus_norm_aff", True) else 0, norm_rank=P.norm_rank,
                count_pos_neg=P.count_pos_neg, norm_aff=P.norm_aff)


def s1_key(name):
    g = geo_flags(name)
    return (g["th"], g["bg"], g["value_rule"], g["use_overlap"], g["normalise"])


def s2_key(name):
    g = geo_flags(name)
    return (g["th"], g["bg"], g["use_overlap"], g["norm_rank"], g["count_pos_neg"])


def s5_key(name):
    g = geo_flags(name)
    return (g["th"], g["norm_aff"])


def v3_serves(name):
    """the packed S1 kernel (and the item lists): th 0.5, normalised product, bg test at 0.5"""
    g = geo_flags(name)
    return g["th"] == 0.5 and g["bg"] == 0.5 and g["value_rule"] == orc.VAL_NORM_PROB_PRODUCT


def v3_flat_form(shape_name, env=None, part=None):
    """The packed kernel's form for a compute box (the whole volume, or part = (z0, y0, x0, z1, y1, x1)): True for
    FLAT (64 base voxels flattened over two lines), False for one line per run.  The rule of v3_flat in
    csrc/ppp_consensus_v3.hip with its switch PPP_S1_FLAT (env: the family's development switches)."""
    ps, vol, _, _ = SHAPES[shape_name]
    cY, cX = (vol[1], vol[2]) if part is None else (part[4] - part[1], part[5] - part[2])
    flat = cX >= 64 and cX % 64 != 0 and ps[1] >= 3 and cY > 1
    e = (env or {}).get("PPP_S1_FLAT")
    if e == "0":
        flat = False
    if e == "1" and cX >= 64 and ps[1] >= 3:
        flat = True
    return flat


def th05_variant(name):
    """consensus_v2_kernel's TH05 variant: th 0.5, normalised product, bg test at or below 0.5"""
    g = geo_flags(name)
    return g["th"] == 0.5 and g["bg"] <= 0.5 and g["value_rule"] == orc.VAL_NORM_PROB_PRODUCT


# ---- number formats -----------------------------------------------------------------------------------------------
def _bf16_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def to_dtype(a, dtype):
    """float32 array of the values the device gets: `a` rounded to nearest-even in `dtype` and widened again"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dtype == "float32":
        return a
    if dtype == "float16":
        return a.astype(np.float16).astype(np.float32)
    u = _bf16_bits(a).astype(np.uint64)                       # (non-negative finite values only)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(a.shape)


def _step(v, dtype, up):
    """neighbour of the representable value v (float32 holding a `dtype` value) in `dtype`"""
    if dtype == "float32":
        return np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf))
    if dtype == "float16":
        return np.float32(np.nextafter(np.float16(v), np.float16(np.inf if up else -np.inf)))
    u = np.array([v], dtype=np.float32).view(np.uint32)
    u = u + np.uint32(0x10000) if up else u - np.uint32(0x10000)
    return u.view(np.float32)[0]


def around(t, dtype):
    """The representable values at or next to the double t on each side, and the next one further out on each
    side: [below-below, largest <= t, smallest >= t, above-above] without duplicates, ascending, float32.
    For float32 that holds float32(t) and both its neighbours."""
    t = float(t)
    if dtype == "float32":
        lo = np.float32(t)
    elif dtype == "float16":
        lo = np.float32(np.float16(t))
    else:
        lo = (np.array([t], dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)[0]
    while float(lo) > t:
        lo = _step(lo, dtype, False)
    while float(_step(lo, dtype, True)) <= t:
        lo = _step(lo, dtype, True)
    hi = lo if float(lo) == t else _step(lo, dtype, True)
    vals = sorted({float(v) for v in (_step(lo, dtype, False), lo, hi, _step(hi, dtype, True))})
    return [np.float32(v) for v in vals]


def pinned_values(name, dtype):
    g = geo_flags(name)
    vals = {0.0, 1.0}
    for t in (g["th"], g["bg"]):
        vals.update(float(v) for v in around(t, dtype))
    return [np.float32(v) for v in sorted(vals)]


# ---- inputs -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base_case(shape_name):
    """synthetic labels, the float32-perturbed prediction (inside [0, 1]), overlap mask, pair rows"""
    ps, vol, cell, seed = SHAPES[shape_name]
    c = synth.make_case(vol, ps, seed=seed, cell=cell, noise=0.3, overlap_frac=0.03)
    rng = np.random.default_rng(seed)
    pred = (c["pred"] * rng.uniform(0.97, 1.0, size=c["pred"].shape)).astype(np.float32)
    pred = np.clip(pred, np.float32(0.0), np.float32(1.0))
    ov = (c["numinst"] > 1).astype(np.uint8)
    rad = np.array([p // 2 for p in ps])
    centres = orc.interior_fg_coords(c["foreground"], rad)
    # a dense cluster around a seeded x (its first patch in x order has the whole cluster as partners) + a sample
    x0 = int(rng.integers(rad[2] + ps[2], vol[2] - rad[2] - ps[2]))
    near = np.argsort(np.abs(centres[:, 2] - x0), kind="stable")
    cluster, rest = near[:N_CLUSTER], near[N_CLUSTER:]
    spread = rng.permutation(rest)[:N_SPREAD[shape_name]]
    sel = centres[np.sort(np.concatenate([cluster, spread]))]
    _, pairs = orc.patch_pairs(sel, ps, include_single=True, max_ps_dist=2)
    for a in (pred, ov, pairs):
        a.setflags(write=False)
    return dict(ps=ps, vol=vol, pred=pred, overlap=ov, foreground=c["foreground"], pairs=pairs, selected=sel)


def interior_mask(shape_name):
    ps, vol, _, _ = SHAPES[shape_name]
    m = np.zeros(vol, dtype=bool)
    m[tuple(slice(p // 2, s - p // 2) for p, s in zip(ps, vol))] = True
    return m


MAX_PINS = 10          # 0, 1 and four values around each of the two thresholds


@functools.lru_cache(maxsize=None)
def _pin_slots(shape_name):
    """Where the k-th pinned value of a cell goes (flat indices into [C, Z, Y, X]): a seeded share of every channel,
    the mid channel included, and a fixed number of interior voxels of the mid channel."""
    ps, vol, _, seed = SHAPES[shape_name]
    C, V = int(np.prod(ps)), int(np.prod(vol))
    rng = np.random.default_rng(seed + 1000)
    bucket = np.floor(rng.uniform(size=C * V) / PIN_SHARE).astype(np.int32)
    inner = rng.permutation(np.flatnonzero(interior_mask(shape_name).ravel()))
    assert len(inner) >= MID_PINS * MAX_PINS
    return [np.concatenate([np.flatnonzero(bucket == k),
                            (C // 2) * V + inner[k * MID_PINS:(k + 1) * MID_PINS]]) for k in range(MAX_PINS)]


@functools.lru_cache(maxsize=4)
def _prediction(shape_name, dtype, pins, clean):      # (no default: one cache key per array)
    b = base_case(shape_name)
    pred = to_dtype(b["pred"], dtype).copy()
    if clean:
        # (the clean variant only: the existing predictions and their cached oracle outputs keep their bits)
        pred[pred == 0] = np.float32(0.0)        # -0.0 -> +0.0: "pred.min() >= 0" does not see it, the check does
    slots = _pin_slots(shape_name)
    assert len(pins) <= MAX_PINS
    for k in range(len(pins)):                   # (share first, the mid channel's fixed voxels last: they hold)
        pred.ravel()[slots[k][:-MID_PINS]] = pins[k]
    for k in range(len(pins)):
        pred.ravel()[slots[k][-MID_PINS:]] = pins[k]
    assert np.array_equal(pred, to_dtype(pred, dtype)) and pred.min() >= 0.0 and pred.max() <= 1.0
    pred.setflags(write=False)
    return pred


def _pins(flag_name, dtype, variant):
    assert variant in VARIANTS
    if variant == CLEAN:
        assert v3_serves(flag_name), "nothing but the packed S1 kernel reads pred_clean"
        return tuple(float(v) for v in clean_pins(dtype))
    return tuple(float(v) for v in pinned_values(flag_name, dtype))


def prediction(shape_name, flag_name, dtype="float32", variant="pinned"):
    """float32 [C, Z, Y, X]: the exact widening of what the device gets for this cell"""
    return _prediction(shape_name, dtype, _pins(flag_name, dtype, variant), variant == CLEAN)


# ---- the clean variant: what ppp_pred_check passes, with the values next to the threshold ---------------------------
PINNED, CLEAN = "pinned", "clean"
VARIANTS = (PINNED, CLEAN)


def smallest(dtype):
    """(smallest positive subnormal, smallest positive normal) of the format, as float32"""
    sub = _step(np.float32(0.0), dtype, True)
    normal = {"float32": 2.0 ** -126, "float16": 2.0 ** -14, "bfloat16": 2.0 ** -126}[dtype]
    return np.float32(sub), np.float32(normal)


def clean_pins(dtype):
    """The nine pinned values of the clean variant, ascending: 0, the smallest subnormal and normal, the two
    representable values below 0.5 and the two above it (never 0.5 itself), the largest value below 1, and 1."""
    a = around(0.5, dtype)
    assert len(a) == 3 and float(a[1]) == 0.5
    sub, normal = smallest(dtype)
    vals = {0.0, float(sub), float(normal), float(_step(a[0], dtype, False)), float(a[0]), float(a[2]),
            float(_step(a[2], dtype, True)), float(_step(np.float32(1.0), dtype, False)), 1.0}
    assert len(vals) == 9 and 0.5 not in vals
    return [np.float32(v) for v in sorted(vals)]


def dtype_patterns(a, dtype):
    """(unsigned bit patterns of the float32 array `a` narrowed exactly to `dtype`, the pattern of 1.0)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dtype == "float32":
        return a.view(np.uint32), 0x3F800000
    if dtype == "float16":
        return a.astype(np.float16).view(np.uint16), 0x3C00
    assert dtype == "bfloat16"
    return (a.view(np.uint32) >> np.uint32(16)).astype(np.uint16), 0x3F80


def is_clean(pred_f32, dtype, th, bg):
    """NumPy restatement of ppp_pred_check (csrc/ppp_aux.hip): the bits it returns for a buffer of `dtype` values
    (given widened to float32) under the class tests v > th / v < bg.  0 = clean.
    Bit 1: a value whose unsigned pattern in the format exceeds that of 1.0 (above 1, inf, nan, every negative value
    and -0).  Bit 2: a value that is neither > th nor < bg -- the oracle's two compares, in doubles (make_geo rounds
    the kernels' float thresholds, th down and bg up, so that their float compares agree)."""
    a = np.ascontiguousarray(pred_f32, dtype=np.float32)
    pat, one = dtype_patterns(a, dtype)
    v = a.astype(np.float64)
    with np.errstate(invalid="ignore"):
        between = ~(v > float(th)) & ~(v < float(bg))
    return (1 if bool((pat > one).any()) else 0) | (2 if bool(between.any()) else 0)


# ---- the oracle's stage outputs --------------------------------------------------------------------------------
_OUT = {}       # (shape, flag set, dtype) -> dict(cons_hash, score, aff)


def bits_hash(a):
    return hashlib.blake2b(np.ascontiguousarray(a, dtype=np.float32).tobytes(), digest_size=16).hexdigest()


@functools.lru_cache(maxsize=1)
def _oracle_s1(shape_name, dtype, pins, key, rep):
    """The oracle's consensus in the reference layout for (prediction, S1 flags); `rep`: a flag set with these S1
    flags.  With the array at hand, the scores and affinities of EVERY flag set that shares it are made too."""
    b = base_case(shape_name)
    pred = _prediction(shape_name, dtype, pins, False)
    # (the gather form of the oracle's S1: the same array as orc.consensus bit for bit -- tests/test_oracle_golden.py
    # and test_flag_matrix_rule.py hold it to that -- on all cores instead of one: 0.4 s instead of 10 s at 9^3)
    cons = orc.consensus_planes(pred, b["overlap"], b["ps"], **FLAG_SETS[rep])
    h = bits_hash(orc.positive_planes(cons, b["ps"]))
    scores, affs = {}, {}
    for name in FLAG_SETS:
        if s1_key(name) != key or (shape_name, name, dtype) in _OUT or \
                tuple(float(v) for v in pinned_values(name, dtype)) != pins:
            continue
        kw = FLAG_SETS[name]
        if s2_key(name) not in scores:
            scores[s2_key(name)] = orc.rank(pred, cons, b["overlap"], b["ps"], **kw)
        if s5_key(name) not in affs:
            affs[s5_key(name)] = orc.patch_graph(pred, cons, b["pairs"], b["ps"], **kw)
        _OUT[(shape_name, name, dtype)] = dict(cons_hash=h, score=scores[s2_key(name)], aff=affs[s5_key(name)])
    return cons


def _s1_args(shape_name, flag_name, dtype):
    return (shape_name, dtype, tuple(float(v) for v in pinned_values(flag_name, dtype)), s1_key(flag_name), flag_name)


@functools.lru_cache(maxsize=1)
def _oracle_s1_clean(shape_name, dtype, key, rep):
    """The clean variant's S1 only: the positive offset planes of the oracle's consensus, their hash noted for every
    served flag set with these S1 flags.  No scores, no affinities: S2 and S5 do not read pred_clean."""
    b = base_case(shape_name)
    pred = _prediction(shape_name, dtype, tuple(float(v) for v in clean_pins(dtype)), True)
    planes = orc.positive_planes(orc.consensus_planes(pred, b["overlap"], b["ps"], **FLAG_SETS[rep]), b["ps"])
    h = bits_hash(planes)
    for name in FLAG_SETS:
        if v3_serves(name) and s1_key(name) == key:
            _OUT[(shape_name, name, dtype, CLEAN)] = dict(cons_hash=h)
    planes.setflags(write=False)
    return planes


def oracle(shape_name, flag_name, dtype="float32", variant="pinned"):
    """dict(cons_hash: bits_hash of the positive offset planes, score (Z, Y, X), aff [rows]) of the cell; the clean
    variant: cons_hash only"""
    if variant == CLEAN:
        k = (shape_name, flag_name, dtype, CLEAN)
        if k not in _OUT:
            assert v3_serves(flag_name)
            _oracle_s1_clean(shape_name, dtype, s1_key(flag_name), _representative(s1_key(flag_name)))
        return _OUT[k]
    assert variant == PINNED
    k = (shape_name, flag_name, dtype)
    if k not in _OUT:
        a = _s1_args(*k)
        # (the representative only names the S1 flags: any set with the same key gives the same array)
        _oracle_s1(*a[:4], _representative(a[3]))
    return _OUT[k]


def _representative(key):
    return next(n for n in FLAG_SETS if s1_key(n) == key)


def oracle_cons_planes(shape_name, flag_name, dtype="float32", variant="pinned"):
    """the positive offset planes [planes, Z, Y, X] (the compact device layout) of the cell's consensus"""
    if variant == CLEAN:
        assert v3_serves(flag_name)
        return _oracle_s1_clean(shape_name, dtype, s1_key(flag_name), _representative(s1_key(flag_name)))
    assert variant == PINNED
    a = _s1_args(shape_name, flag_name, dtype)
    return orc.positive_planes(_oracle_s1(*a[:4], _representative(a[3])), SHAPES[shape_name][0])


def voxel_major_from_planes(planes, ps):
    """The symmetric voxel-major rows [Z, Y, X, W] of compact planes: entry L = Lc + q of voxel v is the consensus
    between v and v + q -- planes[q][v] for q > 0, planes[-q][v + q] for q < 0 (0 where v + q leaves the volume), 0
    for q = 0."""
    pz, py, px = ps
    n, Z, Y, X = planes.shape
    wy, wx = 2 * py - 1, 2 * px - 1
    W = (2 * pz - 1) * wy * wx
    Lc = (W - 1) // 2
    assert n == Lc
    vm = np.zeros((Z, Y, X, W), dtype=np.float32)
    k = 0
    for dz in range(0, pz):
        for dy in range(-(py - 1), py):
            for dx in range(-(px - 1), px):
                if (dz, dy, dx) <= (0, 0, 0):
                    continue
                L = (dz * wy + dy) * wx + dx
                assert L == k + 1
                vm[..., Lc + L] = planes[k]
                # the later voxel v = e + q sees the same entry at -q
                src = planes[k][:Z - dz, max(0, -dy):Y - max(0, dy), max(0, -dx):X - max(0, dx)]
                vm[dz:, max(0, dy):Y + min(0, dy), max(0, dx):X + min(0, dx), Lc - L] = src
                k += 1
    return vm
