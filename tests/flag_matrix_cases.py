"""The flag matrix of the S1 / S2 / S5 kernel families: flag sets, shapes, predictions with values pinned
at the thresholds, pair rows and the oracle's stage outputs (plain module, no GPU; imported by
tests/test_flag_matrix_rule.py and tests/test_flag_matrix_gpu.py).

A CELL is (shape name, flag set name, dtype).  Everything here is a pure function of the cell, computed
once per process and shared by all families that meet the cell."""
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
def _prediction(shape_name, dtype, pins):
    b = base_case(shape_name)
    pred = to_dtype(b["pred"], dtype).copy()
    slots = _pin_slots(shape_name)
    assert len(pins) <= MAX_PINS
    for k in range(len(pins)):                   # (share first, the mid channel's fixed voxels last: they hold)
        pred.ravel()[slots[k][:-MID_PINS]] = pins[k]
    for k in range(len(pins)):
        pred.ravel()[slots[k][-MID_PINS:]] = pins[k]
    assert np.array_equal(pred, to_dtype(pred, dtype)) and pred.min() >= 0.0 and pred.max() <= 1.0
    pred.setflags(write=False)
    return pred


def prediction(shape_name, flag_name, dtype="float32"):
    """float32 [C, Z, Y, X]: the exact widening of what the device gets for this cell"""
    return _prediction(shape_name, dtype, tuple(float(v) for v in pinned_values(flag_name, dtype)))


# ---- the oracle's stage outputs --------------------------------------------------------------------------------
_OUT = {}       # (shape, flag set, dtype) -> dict(cons_hash, score, aff)


def bits_hash(a):
    return hashlib.blake2b(np.ascontiguousarray(a, dtype=np.float32).tobytes(), digest_size=16).hexdigest()


@functools.lru_cache(maxsize=1)
def _oracle_s1(shape_name, dtype, pins, key, rep):
    """The oracle's consensus in the reference layout for (prediction, S1 flags); `rep`: a flag set with these S1
    flags.  With the array at hand, the scores and affinities of EVERY flag set that shares it are made too."""
    b = base_case(shape_name)
    pred = _prediction(shape_name, dtype, pins)
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


def oracle(shape_name, flag_name, dtype="float32"):
    """dict(cons_hash: bits_hash of the positive offset planes, score (Z, Y, X), aff [rows]) of the cell"""
    k = (shape_name, flag_name, dtype)
    if k not in _OUT:
        a = _s1_args(*k)
        # (the representative only names the S1 flags: any set with the same key gives the same array)
        _oracle_s1(*a[:4], _representative(a[3]))
    return _OUT[k]


def _representative(key):
    return next(n for n in FLAG_SETS if s1_key(n) == key)


def oracle_cons_planes(shape_name, flag_name, dtype="float32"):
    """the positive offset planes [planes, Z, Y, X] (the compact device layout) of the cell's consensus"""
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
