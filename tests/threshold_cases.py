"""The consumers of the prediction after S2 -- cover bits, cover, thinning, pack scan, the three paints -- and the
rule they compare by: the float32 value against float32(threshold), as NumPy does in the reference's host stages
(plain module, no GPU; imported by tests/test_threshold_rule.py and tests/test_threshold_consumers_gpu.py).

S1, S2 and S5 compare the float value with the DOUBLE threshold instead (tests/flag_matrix_cases.py holds them).
The two rules differ only for a value equal to float32(t), and only where float32(t) > t: t = 0.3, 0.4, 0.6, 0.8.

A CELL is (shape name, (patch_threshold, fc_threshold), dtype).  Its prediction is the flag matrix's perturbed
synthetic prediction in which a seeded share of ALL entries holds each representable value at and next to either
threshold (flag_matrix_cases.around).  Everything here is a pure function of the cell, computed once per process."""
import functools

import numpy as np

from flag_matrix_cases import DTYPES, around, to_dtype  # noqa: F401  (one definition of the number formats)
from oracle import ppp_oracle as orc
from patchperpix_amd import synth
from tests_flags import FLYLIGHT_CC

# (patch_threshold, fc_threshold): unequal, so that a consumer reading the wrong one of the two fails too
PAIRS = [(0.6, 0.3),      # both discriminate, and differ from each other
         (0.3, 0.6),      # both discriminate, and differ from each other
         (0.4, 0.4),      # both discriminate
         (0.5, 0.3),      # only fc discriminates
         (0.7, 0.5)]      # control: the rules agree
CONTROL = (0.7, 0.5)

# name -> (patch shape, volume, cell size of the synthetic labels, seed): the smallest volumes at which each consumer
# can still go wrong; x is no multiple of 64 where the volume allows
SHAPES = {
    "p3": ((3, 3, 3), (8, 9, 30), [5, 5, 5], 401),          # one partial bit word
    "p5": ((5, 5, 5), (9, 11, 40), [5, 6, 7], 402),         # 4 words, 29 bits in the last; cells that stay apart
    "p7": ((7, 7, 7), (13, 15, 40), [9, 9, 9], 403),        # 11 words: several 64-lane ballots, odd word count
    "p9": ((9, 9, 9), (12, 13, 40), [12, 12, 12], 404),     # 23 words
    "p357": ((3, 5, 7), (10, 16, 40), [4, 7, 9], 405),      # anisotropic
    "w5": ((1, 5, 5), (1, 30, 40), [1, 8, 8], 406),         # 2-d
    "w25": ((1, 25, 25), (1, 40, 60), [1, 30, 30], 407),    # 2-d, 20 words
}
PIN_SHARE = 0.02       # share of ALL entries (every channel, the mid channel included) that gets each pinned value
NOISE = 0.3            # of the synthetic prediction, as in the flag matrix
MAX_PINS = 8           # up to four values around each of the two thresholds

F32, F64 = "float32", "double"     # the two rules


def discriminates(t):
    """float32(t) > t: a value equal to float32(t) is "above" for the double compare and "not above" for NumPy's"""
    return float(np.float32(t)) > float(t)


def above(v, t, rule=F32):
    """v > t by the rule: float32 value against float32(t) (host stages), or against the double t (S1 / S2 / S5)"""
    if rule == F32:
        return np.asarray(v, dtype=np.float32) > np.float32(t)
    assert rule == F64
    return np.asarray(v).astype(np.float64) > float(t)


def flags(pair, **over):
    """connected components + thinning with the cell's two thresholds"""
    th, fc = pair
    return dict(FLYLIGHT_CC, patch_threshold=th, fc_threshold=fc, **over)


def words_of(ps):
    return (int(np.prod(ps)) + 31) // 32


# ---- inputs -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base_case(shape_name):
    """synthetic labels and the float32-perturbed prediction (inside [0, 1]), as flag_matrix_cases.base_case makes it"""
    ps, vol, cell, seed = SHAPES[shape_name]
    c = synth.make_case(vol, ps, seed=seed, cell=cell, noise=NOISE, overlap_frac=0.03)
    rng = np.random.default_rng(seed)
    pred = (c["pred"] * rng.uniform(0.97, 1.0, size=c["pred"].shape)).astype(np.float32)
    pred = np.clip(pred, np.float32(0.0), np.float32(1.0))
    fg, ni = c["foreground"], c["numinst"]
    for a in (pred, fg, ni):
        a.setflags(write=False)
    return dict(ps=ps, vol=vol, pred=pred, foreground=fg, numinst=ni, overlap=1 * (ni > 1))


def pinned_values(pair, dtype):
    vals = set()
    for t in pair:
        vals.update(float(v) for v in around(t, dtype))
    assert len(vals) <= MAX_PINS
    return [np.float32(v) for v in sorted(vals)]


@functools.lru_cache(maxsize=None)
def _pin_bucket(shape_name):
    ps, vol, _, seed = SHAPES[shape_name]
    rng = np.random.default_rng(seed + 1000)
    return np.floor(rng.uniform(size=int(np.prod(ps)) * int(np.prod(vol))) / PIN_SHARE).astype(np.int32)


@functools.lru_cache(maxsize=6)
def prediction(shape_name, pair, dtype="float32"):
    """float32 [C, Z, Y, X]: the exact widening of what the device gets for this cell"""
    b = base_case(shape_name)
    pred = to_dtype(b["pred"], dtype).copy()
    bucket = _pin_bucket(shape_name)
    for k, v in enumerate(pinned_values(pair, dtype)):
        pred.ravel()[bucket == k] = v
    assert np.array_equal(pred, to_dtype(pred, dtype)) and pred.min() >= 0.0 and pred.max() <= 1.0
    pred.setflags(write=False)
    return pred


def interior_mask(shape_name):
    ps, vol, _, _ = SHAPES[shape_name]
    m = np.zeros(vol, dtype=bool)
    m[tuple(slice(p // 2, s - p // 2) for p, s in zip(ps, vol))] = True
    return m


def centre_list(shape_name, n=200):
    """int32 [n, 3]: seeded centres anywhere in the volume with the first and the last voxel and repeats"""
    _, vol, _, seed = SHAPES[shape_name]
    rng = np.random.default_rng(seed + 2000)
    cen = np.stack([rng.integers(0, s, n) for s in vol], 1).astype(np.int32)
    cen[0] = (0, 0, 0)
    cen[1] = [s - 1 for s in vol]
    cen[2:30] = cen[30:58]
    cen[-1] = cen[1]
    return cen


# ---- models --------------------------------------------------------------------------------------------------------
def pack_rows(on):
    """bool [n, C] -> uint32 [n, ceil(C / 32)]: bit r of a row sits in word r // 32 at position r % 32"""
    on = np.asarray(on, dtype=bool)
    n, C = on.shape
    words = (C + 31) // 32
    padded = np.zeros((n, words * 32), dtype=bool)
    padded[:, :C] = on
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u4").reshape(n, words)


def packed_bits(pred, t, centres=None, rule=F32):
    """The packed patch bits: bit r of a centre = pred[r][centre] > t.  centres None: every voxel in raster order."""
    C = pred.shape[0]
    if centres is None:
        vals = pred.reshape(C, -1).T
    else:
        c = np.asarray(centres).reshape(-1, 3)
        vals = pred[:, c[:, 0], c[:, 1], c[:, 2]].T
    return pack_rows(above(vals, t, rule))


def narrowed_bits(pred, t, dtype, centres=None):
    """What a compare carried out in the storage type gives: the threshold rounded to `dtype` first"""
    return packed_bits(pred, float(to_dtype(np.array([t], np.float32), dtype)[0]), centres)


def fg_bits(pred, t, ps, centres):
    """S5's foreground bits of interior centres (ppp_patch_fg_bits): bit r = mid[r-th voxel of the window] > t and
    pred[r][centre] > t, both by the DOUBLE rule"""
    rad = [p // 2 for p in ps]
    mid = above(pred[int(np.prod(ps)) // 2], t, F64)
    rows = []
    for c in np.asarray(centres).reshape(-1, 3):
        win = mid[tuple(slice(int(c[a]) - rad[a], int(c[a]) + rad[a] + 1) for a in range(3))]
        rows.append(win.reshape(-1) & above(pred[:, c[0], c[1], c[2]], t, F64))
    return pack_rows(np.array(rows, dtype=bool).reshape(len(rows), int(np.prod(ps))))


def component_masks(ccs, pred, ps, shape, t, rule=F32):
    """bool [K, Z, Y, X]: a component's voxels are the union over its patches of window & (patch > t); a window that
    leaves the volume is clipped"""
    rad = [p // 2 for p in ps]
    masks = np.zeros((len(ccs),) + tuple(shape), bool)
    for k, cc in enumerate(ccs):
        for c in cc:
            patch = above(pred[(slice(None),) + tuple(int(v) for v in c)], t, rule).reshape(ps)
            lo = [int(c[a]) - rad[a] for a in range(3)]
            src = tuple(slice(max(0, -lo[a]), min(ps[a], shape[a] - lo[a])) for a in range(3))
            dst = tuple(slice(max(0, lo[a]), min(shape[a], lo[a] + ps[a])) for a in range(3))
            masks[k][dst] |= patch[src]
    return masks


def paint_model(masks):
    """int64 (Z, Y, X): the largest label wins (what the reference's in-order overwrite yields)"""
    out = np.zeros(masks.shape[1:], np.int64)
    for k, m in enumerate(masks):
        out = np.maximum(out, np.where(m, k + 1, 0))
    return out


def pack_scan_model(masks):
    """(sizes int64 [K + 1], slot 0 unused; sorted unique keys (b << 32) | a of the labels a < b sharing a voxel)"""
    flat = masks.reshape(len(masks), -1).astype(np.int64)
    inter = flat @ flat.T
    keys = [((b + 1) << 32) | (a + 1) for b in range(len(masks)) for a in range(b) if inter[a, b]]
    return np.concatenate([[0], flat.sum(1)]), np.array(sorted(keys), dtype=np.uint64)


def channels_model(masks, min_voxels):
    """The reference's channel loop (graph_to_labeling.py:86-106) on explicit voxel sets: int64 (channels, Z, Y, X)"""
    channels = []
    for k, m in enumerate(masks):
        cur = np.where(m, k + 1, 0)
        if not channels:
            channels.append(cur)
        elif m.sum() > min_voxels:
            for ch in channels:
                if not (ch[m] != 0).any():
                    ch[m] = k + 1
                    break
            else:
                channels.append(cur)
        else:
            channels[0][m] = k + 1
    return np.stack(channels, 0)


# ---- the oracle's host stages per cell --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ranked(shape_name, pair, dtype="float32"):
    """The oracle's ranked list of the cell: (coords int [n, 3], scores float32 [n]) of the interior foreground"""
    b = base_case(shape_name)
    pred = prediction(shape_name, pair, dtype)
    kw = flags(pair)
    cons = orc.consensus_planes(pred, b["overlap"], b["ps"], **kw)
    scores = orc.rank(pred, cons, b["overlap"], b["ps"], **kw)
    coords = orc.interior_fg_coords(b["foreground"], np.array([p // 2 for p in b["ps"]]))
    rc, rs = orc.rank_by_score(coords, scores)
    for a in (rc, rs):
        a.setflags(write=False)
    return rc, rs


def mask_to_cover(shape_name):
    b = base_case(shape_name)
    m = b["foreground"].copy()
    m[b["overlap"] > 0] = 0
    return m


@functools.lru_cache(maxsize=None)
def cover(shape_name, pair, dtype="float32", rule=F32, sparse=True, mark=False):
    """indices into the ranked list: orc.foreground_cover under the rule (the double rule: the oracle is fed the
    prediction as float64, so that NumPy compares in doubles)"""
    b = base_case(shape_name)
    rc, rs = ranked(shape_name, pair, dtype)
    pred = prediction(shape_name, pair, dtype)
    pred = pred.astype(np.float64) if rule == F64 else pred
    kw = flags(pair, select_patches_for_sparse_data=sparse, mark_close_neighboorhood=mark)
    sel = orc.foreground_cover(rc, rs, b["overlap"], mask_to_cover(shape_name), pred, b["ps"], **kw)
    sel.setflags(write=False)
    return sel


@functools.lru_cache(maxsize=None)
def thinned(shape_name, pair, dtype="float32", rule=F32):
    """indices into the float32-rule cover's coordinates: orc.thin_cover under the rule"""
    b = base_case(shape_name)
    rc, _ = ranked(shape_name, pair, dtype)
    sel = rc[cover(shape_name, pair, dtype)]
    pred = prediction(shape_name, pair, dtype)
    pred = pred.astype(np.float64) if rule == F64 else pred
    keep = orc.thin_cover(sel, mask_to_cover(shape_name), pred, b["ps"], **flags(pair))
    keep.setflags(write=False)
    return keep


# ---- components for the pack scan and the paints ----------------------------------------------------------------------
PAINT_SHAPES = ("p5", "p7", "p357")       # (volumes in which a component can hold more than PACK_MIN_VOXELS voxels)
# shares of the thinned nodes: a small component first and last, so that both get painted over and paint over
_SHARES = (0.08, 0.72, 0.07, 0.06, 0.07)


@functools.lru_cache(maxsize=None)
def components(shape_name, pair, dtype="float32"):
    """ccs (list of lists of centres, in label order): a seeded partition of the cell's thinned nodes"""
    _, _, _, seed = SHAPES[shape_name]
    rc, _ = ranked(shape_name, pair, dtype)
    nodes = rc[cover(shape_name, pair, dtype)][thinned(shape_name, pair, dtype)]
    rng = np.random.default_rng(seed + 3000)
    lab = rng.choice(len(_SHARES), size=len(nodes), p=_SHARES)
    return [[tuple(int(v) for v in c) for c in nodes[lab == k]] for k in range(len(_SHARES))]


def face_nodes(shape_name):
    """nodes on all six faces of the volume (two corners among them), as (node, label) pairs"""
    _, (Z, Y, X), _, _ = SHAPES[shape_name]
    return [((0, Y // 2, X // 2), 1), ((Z - 1, Y // 3, X // 3), 3), ((Z // 2, 0, X // 2), 2), ((Z // 3, Y - 1, X // 4), 5),
            ((Z // 2, Y // 2, 0), 4), ((Z // 2, Y // 3, X - 1), 1), ((0, 0, 0), 5), ((Z - 1, Y - 1, X - 1), 2)]


def nodes_and_labels(ccs):
    nodes = np.array([c for cc in ccs for c in cc], dtype=np.int32).reshape(-1, 3)
    labels = np.array([k + 1 for k, cc in enumerate(ccs) for _ in cc], dtype=np.int32)
    return nodes, labels


# ---- the case tables (hand-written; tests/test_threshold_rule.py asserts the covering conditions) -------------------------
# bits: every shape, every pair in float32, the 16-bit types on two pairs each
_BITS_16 = {"float16": [(0.6, 0.3), (0.3, 0.6)], "bfloat16": [(0.4, 0.4), (0.5, 0.3)]}
BITS_CELLS = [(s, pair, "float32") for s in SHAPES for pair in PAIRS] + \
             [(s, pair, d) for s in SHAPES for d in ("float16", "bfloat16") for pair in _BITS_16[d]]
# cover and thinning: the pairs with fc 0.3 and 0.6, float32 and one 16-bit type (alternating over the shapes)
COVER_SHAPES = ("p3", "p5", "p7", "p357", "w5")
COVER_PAIRS = [(0.6, 0.3), (0.3, 0.6), (0.5, 0.3)]
COVER_CELLS = [(s, pair, d) for i, s in enumerate(COVER_SHAPES) for pair in COVER_PAIRS
               for d in ("float32", ("float16", "bfloat16")[i % 2])]
# pack scan and paints: every pair in float32, (0.6, 0.3) in the 16-bit types
PAINT_CELLS = [(s, pair, "float32") for s in PAINT_SHAPES for pair in PAIRS] + \
              [(s, (0.6, 0.3), d) for s in PAINT_SHAPES for d in ("float16", "bfloat16")]


def cell_id(cell):
    s, (th, fc), d = cell
    return "%s-th%g-fc%g-%s" % (s, th, fc, d)


# ---- end to end ---------------------------------------------------------------------------------------------------
E2E_SHAPES = ("p5", "w5")
E2E_CELLS = [(s, pair, "float32") for s in E2E_SHAPES for pair in PAIRS] + \
            [(s, (0.6, 0.3), d) for s in E2E_SHAPES for d in ("float16", "bfloat16")]
MIN_INSTANCES = 3      # an empty result cannot pass


@functools.lru_cache(maxsize=None)
def e2e_expected(shape_name, pair, dtype, mws):
    """orc.to_instance_seg of the cell: dict(instances, foreground, pairs, aff)"""
    b = base_case(shape_name)
    ref = orc.to_instance_seg(prediction(shape_name, pair, dtype), b["foreground"], b["foreground"].copy(), b["numinst"],
                              list(b["ps"]), **flags(pair, mws=mws))
    return {k: ref[k] for k in ("instances", "foreground", "pairs", "aff")}


def n_instances(inst):
    return len(np.unique(inst)) - (1 if (np.asarray(inst) == 0).any() else 0)


STACK = ("w5", (0.6, 0.3), "float32")


@functools.lru_cache(maxsize=None)
def stack_case():
    """Three independent 2-d images: the w5 cell, the same mirrored in x, and mirrored in y (the mirrored images are
    other data to the patch channels, which is all they need to be).  dict(pred, foreground, numinst)."""
    s, pair, dtype = STACK
    b = base_case(s)
    flips = [lambda a: a, lambda a: a[..., ::-1], lambda a: a[..., ::-1, :]]
    return dict(pred=np.ascontiguousarray(np.concatenate([f(prediction(s, pair, dtype)) for f in flips], axis=1)),
                foreground=np.ascontiguousarray(np.concatenate([f(b["foreground"]) for f in flips])),
                numinst=np.ascontiguousarray(np.concatenate([f(b["numinst"]) for f in flips])))


@functools.lru_cache(maxsize=None)
def stack_expected(mws):
    """per slice: orc.to_instance_seg of that image alone"""
    s, pair, _ = STACK
    c = stack_case()
    out = []
    for k in range(c["foreground"].shape[0]):
        sl = slice(k, k + 1)
        ref = orc.to_instance_seg(c["pred"][:, sl], c["foreground"][sl], c["foreground"][sl].copy(), c["numinst"][sl],
                                  list(SHAPES[s][0]), **flags(pair, mws=mws))
        out.append({k2: ref[k2] for k2 in ("instances", "foreground", "pairs", "aff")})
    return out
