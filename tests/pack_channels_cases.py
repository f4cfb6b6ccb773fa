"""Cases shared by test_pack_channels_rule.py and test_pack_channels_gpu.py: components given directly
(balls of patch centres on a random prediction) and crossing bars for the end-to-end runs, each with
the oracle's result, computed once per process."""
import functools

import numpy as np

TH = 0.5
# (shape, patchshape, R, r, seed): seven balls of radius R and five of radius r, in shuffled order
DIRECT = [((20, 28, 30), (3, 3, 3), 8.5, 3.0, 1),
          ((22, 26, 28), (5, 5, 5), 7.5, 2.0, 4),
          ((1, 90, 100), (1, 25, 25), 16.0, 3.0, 4),
          ((18, 24, 26), (3, 5, 7), 7.5, 2.0, 4)]


def _interior(shape, ps):
    """centres whose window lies inside the volume (the reference's window indexing fails on a clipped one)"""
    m = np.zeros(shape, bool)
    m[tuple(slice(p // 2, s - p // 2) for s, p in zip(shape, ps))] = True
    return m


@functools.lru_cache(maxsize=None)
def direct_case(i):
    """(pred float32 (C, Z, Y, X), ccs = list of lists of centres, in component order)"""
    shape, ps, R, r, seed = DIRECT[i]
    rng = np.random.default_rng(seed)
    pred = ((rng.random((int(np.prod(ps)),) + shape) < 0.8) * 0.9 + 0.05).astype(np.float32)
    zz, yy, xx = np.mgrid[:shape[0], :shape[1], :shape[2]]
    free = _interior(shape, ps)
    ccs = []
    for rr in rng.permutation([R] * 7 + [r] * 5):
        c = [int(rng.integers(0, s)) for s in shape]
        ball = ((zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= rr * rr) & free & (rng.random(shape) < 0.5)
        free &= ~ball                      # disjoint from the centres already taken
        ccs.append([tuple(int(v) for v in p) for p in np.argwhere(ball)])
    pred.setflags(write=False)
    return pred, ccs


def nodes_and_labels(ccs):
    nodes = np.array([c for cc in ccs for c in cc], dtype=np.int32).reshape(-1, 3)
    labels = np.array([k + 1 for k, cc in enumerate(ccs) for _ in cc], dtype=np.int32)
    return nodes, labels


def component_masks(ccs, pred, ps, shape, th=TH):
    """M_k: the union over the component's patches of the window voxels whose patch value is > th,
    clipped to the volume (bool [K, Z, Y, X])"""
    rad = [p // 2 for p in ps]
    th = np.float32(th)
    masks = np.zeros((len(ccs),) + tuple(shape), bool)
    for k, cc in enumerate(ccs):
        for c in cc:
            patch = pred[(slice(None),) + tuple(c)].reshape(ps) > th
            lo = [c[a] - rad[a] for a in range(3)]
            src = tuple(slice(max(0, -lo[a]), min(ps[a], shape[a] - lo[a])) for a in range(3))
            dst = tuple(slice(max(0, lo[a]), min(shape[a], lo[a] + ps[a])) for a in range(3))
            masks[k][dst] |= patch[src]
    return masks


def loop_on_masks(masks, min_voxels):
    """the reference's loop (graph_to_labeling.py:86-106) on explicit voxel sets: (chan, map)"""
    channels, chan = [], []
    for k, m in enumerate(masks):
        cur = np.where(m, k + 1, 0)
        if not channels:
            channels.append(cur)
            chan.append(0)
        elif m.sum() > min_voxels:
            for c, ch in enumerate(channels):
                if not (ch[m] != 0).any():
                    ch[m] = k + 1
                    chan.append(c)
                    break
            else:
                channels.append(cur)
                chan.append(len(channels) - 1)
        else:
            channels[0][m] = k + 1
            chan.append(0)
    return np.array(chan, np.int32), np.stack(channels, 0)


def overlap_pairs(masks):
    """keys (b << 32) | a of the labels a < b whose masks share a voxel"""
    flat = masks.reshape(len(masks), -1).astype(np.int64)
    inter = flat @ flat.T
    return np.array([((b + 1) << 32) | (a + 1) for b in range(len(masks)) for a in range(b) if inter[a, b]], dtype=np.uint64)


def map_from_channels(masks, chan, n_channels):
    """fact 3: channel c holds at a voxel the largest label among the components of c that cover it"""
    out = np.zeros((n_channels,) + masks.shape[1:], np.int64)
    for k, m in enumerate(masks):
        out[chan[k]] = np.maximum(out[chan[k]], np.where(m, k + 1, 0))
    return out


@functools.lru_cache(maxsize=None)
def direct_expected(i):
    """the oracle's packed map of direct case i, and the masks; asserts the case is not a quiet one"""
    from oracle import ppp_oracle as orc
    shape, ps = DIRECT[i][:2]
    pred, ccs = direct_case(i)
    want = orc.paint_per_channel(ccs, pred, list(ps), shape, TH, packed=True)
    masks = component_masks(ccs, pred, ps, shape)
    assert want.shape[0] >= 2, "the case needs a second channel"
    assert (masks.sum(0) >= 3).any(), "the case needs a voxel covered by three components"
    sizes = masks.reshape(len(masks), -1).sum(1)
    chan, _ = loop_on_masks(masks, 2000)
    small_over_large = any(sizes[k] <= 2000 and sizes[j] > 2000 and chan[j] == 0 and (masks[j] & masks[k]).any()
                           for k in range(1, len(masks)) for j in range(k))
    assert small_over_large, "the case needs a small component painted over a large one in channel 0"
    want.setflags(write=False)
    masks.setflags(write=False)
    return want, masks


# ---- end to end: crossing bars with thin overlaps ---------------------------------------------------
BARS = {(5, 5, 5): ((22, 30, 32), [(3, 11, 4, 14, 0, 32), (9, 19, 0, 30, 8, 19), (3, 11, 17, 28, 0, 32), (15, 19, 22, 28, 24, 31)]),
        (3, 3, 3): ((20, 28, 30), [(2, 10, 3, 13, 0, 30), (9, 19, 0, 28, 8, 19), (2, 10, 16, 27, 0, 30), (14, 18, 22, 27, 23, 29)])}


def _hash01(n, seed):
    """n reproducible values in [0, 1) (an integer hash, no generator state)"""
    x = (np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(29)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(32)
    return (x >> np.uint64(40)).astype(np.float64) / float(1 << 24)


def bars_case(ps, shape=None, boxes=None):
    """numinst = bars on a voxel, foreground = their union; a voxel owned by exactly one bar predicts
    that bar's mask in its window (0.9 inside, 0.1 outside), any other voxel 0.1; +- 0.05 of hashed
    noise, rounded through float16.  Returns a dict like synth.make_case's."""
    if shape is None:
        shape, boxes = BARS[tuple(ps)]
    Z, Y, X = shape
    bars = np.zeros((len(boxes),) + tuple(shape), bool)
    for k, (z0, z1, y0, y1, x0, x1) in enumerate(boxes):
        bars[k, z0:z1, y0:y1, x0:x1] = True
    numinst = bars.sum(0).astype(np.uint8)
    assert len(boxes) <= 64
    member = np.zeros(shape, np.uint64)                 # bit k: bar k holds the voxel
    for k in range(len(boxes)):
        member |= bars[k].astype(np.uint64) << np.uint64(k)
    single = numinst == 1
    owner = np.where(single, bars.argmax(0), 0).astype(np.uint64)
    rad = [p // 2 for p in ps]
    padded = np.pad(member, [(r, r) for r in rad])
    pred = np.full((int(np.prod(ps)),) + tuple(shape), 0.1, np.float32)
    r = 0
    for dz in range(ps[0]):
        for dy in range(ps[1]):
            for dx in range(ps[2]):
                shifted = padded[dz:dz + Z, dy:dy + Y, dx:dx + X]          # the bars at voxel + offset r
                pred[r][single & (((shifted >> owner) & np.uint64(1)) != 0)] = 0.9
                pred[r] += ((_hash01(member.size, 17 + r * member.size) - 0.5) * 0.1).astype(np.float32).reshape(shape)
                r += 1
    pred = pred.astype(np.float16).astype(np.float32)
    return {"pred": pred, "foreground": numinst > 0, "numinst": numinst}


@functools.lru_cache(maxsize=None)
def bars_expected(ps, flagset):
    """(case, flags, the oracle's map) of the crossing bars"""
    from oracle import ppp_oracle as orc
    from patchperpix_amd import flags as flagsets
    case = bars_case(ps)
    kw = dict(flagsets.FLAG_SETS[flagset], no_overlap_per_channel=True)
    want = orc.to_instance_seg(case["pred"], case["foreground"], case["foreground"].copy(), case["numinst"],
                               list(ps), **kw)["instances"]
    assert want.ndim == 4 and want.shape[0] >= 2, "the bars need a second channel"
    want.setflags(write=False)
    return case, kw, want
