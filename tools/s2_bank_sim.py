"""LDS bank conflicts of the row reads of rank_wg_kernel (ppp_rank_wg.hip), counted on the CPU.

Every term of the kernel's chain is one ds_read_b32 of the row image at
    base(lane) + immediate(partner),   base(lane) = -(az * SZ + ay * SY + ax * SX)
so the banks of an instruction are those of the lanes' bases shifted by a constant, and the passes
it takes depend only on how the items (ax, ay, az) of a row are dealt to the lanes and on the image's
strides.  ds_read_b32: bank = (byte address / 4) % 32, the two 32-lane halves are served one after the
other, lanes of a half that read the same address share a pass, every further distinct address on a
bank costs a further pass (SQ_LDS_BANK_CONFLICT counts the further passes, SQ_LDS_IDX_ACTIVE all).

A row of an interior tile is a box of nx x ny x nz items (n = 1 .. P per axis: P only where the voxel
is at least the patch radius inside the tile), so a tile's rows fall into P^3 classes with known
counts; per class the script deals the items to chunks of 64 lanes exactly as item_geom() does
(lanes beyond the row's items read item 0's address, every lane is taken as active) and counts passes.

    python tools/s2_bank_sim.py                       today's layouts, every patch size and tile
    python tools/s2_bank_sim.py --patch 7 --enum xyz  another enumeration on today's strides
    python tools/s2_bank_sim.py --patch 7 --search    strides x enumerations for one patch size (minutes)

A layout is (enumeration, SX, SY, SZ): the enumeration names the axes from the fastest, 'xyz' is
ax = i % nx, ay = i / nx % ny, az = i / (nx ny); 'best' picks per row class the order with the fewest
passes (a kernel would choose it per row from nx, ny, nz); 'pad8:...' pads the fastest axis to 8 lanes;
'bank' is the table of rank_deal_table_kernel (bank_dealing below), what 7^3 runs.  --enum overrides.

Model against counter (140^3 / 7^3, SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE of the kernel, which also
holds the accumulator and table reads): x-runs on strides 13 / 169 predicted 0.44, measured 0.41.
"""
import argparse
import itertools
import json

import numpy as np


def axis_classes(T, P):
    """{n: rows} along one axis of a tile T centres wide: n = how many window positions of the voxel
    have their centre inside the tile"""
    out = {}
    for u in range(T + P - 1):
        n = min(P - 1, u) - max(0, u - (T - 1)) + 1
        out[n] = out.get(n, 0) + 1
    return out


ORDERS = ["".join(p) for p in itertools.permutations("xyz")]


def bank_dealing(n, strides):
    """The dealing of rank_deal_table_kernel (ppp_rank_wg.hip): lane l of a half-wave takes items whose
    base falls on bank class l = (ax * SX + ay * SY + az * SZ) % 32 -- half-wave k the k-th such item in
    (az, ay) order -- so the half-waves are conflict-free by construction; the row keeps its dense number
    of chunks, and the items of a class that has more than that many half-waves go, in order, to the
    lanes left empty (those cost their half-wave a further pass).  Returns (ax, ay, az, live) per slot."""
    nx, ny, nz = n
    H = (nx * ny * nz + 63) // 64 * 2
    slot = -np.ones((H, 32, 3), dtype=np.int64)
    over = []
    for r in range(32):
        k = 0
        for az in range(nz):
            for ay in range(ny):
                ax = (r - strides[1] * ay - strides[2] * az) % 32
                if strides[0] != 1:
                    raise ValueError("x is the contiguous axis")
                if ax < nx:
                    if k < H:
                        slot[k, r] = (ax, ay, az)
                    else:
                        over.append((ax, ay, az))
                    k += 1
    free = [(k, l) for k in range(H) for l in range(32) if slot[k, l, 0] < 0]
    for item, (k, l) in zip(over, free):
        slot[k, l] = item
    flat = slot.reshape(-1, 3)
    live = flat[:, 0] >= 0
    flat = np.where(live[:, None], flat, 0)          # (an empty lane reads item (0, 0, 0)'s address)
    return flat[:, 0], flat[:, 1], flat[:, 2], live


class Dealing:
    """the half-waves of every row class of a tile under one enumeration: coordinates per lane, which
    lanes carry an address of their own, the class and its number of rows"""

    def __init__(self, P, tile, order, pad8=False, strides=None):
        cz, cy, cx = (axis_classes(t, P) for t in tile)
        X, Y, Z, K, cls, self.w, self.chunks, self.chunks0 = [], [], [], [], [], [], [], []
        for nz, wz in cz.items():
            for ny, wy in cy.items():
                for nx, wx in cx.items():
                    n = (nx, ny, nz)
                    ext = [n["xyz".index(c)] for c in order]
                    lanes0 = 8 if pad8 else ext[0]
                    total = lanes0 * ext[1] * ext[2]
                    i = np.arange((total + 63) // 64 * 64)
                    live = i < total
                    ii = np.where(live, i, 0)       # lanes beyond the row read item 0's address
                    c0, c1, c2 = ii % lanes0, (ii // lanes0) % ext[1], ii // (lanes0 * ext[1])
                    # (a padded run's idle lanes read the run's last item: a broadcast)
                    dup = ~live | (c0 >= ext[0])
                    c0 = np.minimum(c0, ext[0] - 1)
                    co = {order[0]: c0, order[1]: c1, order[2]: c2}
                    if strides is not None:          # (the bank dealing: a table, not an enumeration)
                        bx, by, bz, blive = bank_dealing(n, strides)
                        co, dup, i = {"x": bx, "y": by, "z": bz}, ~blive, np.arange(len(bx))
                    # lanes that repeat an address of their half-wave add no pass: keep the first
                    # such lane of a half-wave only where the address is not already there
                    key = (co["z"] * 64 + co["y"]) * 64 + co["x"]
                    keep = ~dup
                    for h in range(len(i) // 32):
                        sl = slice(32 * h, 32 * h + 32)
                        seen = set(key[sl][keep[sl]].tolist())
                        for l in np.nonzero(dup[sl])[0]:
                            if int(key[sl][l]) not in seen:
                                seen.add(int(key[sl][l])); keep[32 * h + l] = True
                    X.append(co["x"]); Y.append(co["y"]); Z.append(co["z"]); K.append(keep)
                    cls += [len(self.w)] * (len(i) // 32)
                    self.w.append(wz * wy * wx)
                    self.chunks.append(len(i) // 64)
                    self.chunks0.append((nx * ny * nz + 63) // 64)
        self.X, self.Y, self.Z, self.K = (np.concatenate(v).reshape(-1, 32) for v in (X, Y, Z, K))
        self.cls = np.array(cls)
        self.w, self.chunks, self.chunks0 = np.array(self.w), np.array(self.chunks), np.array(self.chunks0)

    def passes(self, strides):
        """LDS passes of one read instruction per row class"""
        bank = (-(self.X * strides[0] + self.Y * strides[1] + self.Z * strides[2])) % 32
        cnt = ((bank[:, :, None] == np.arange(32)[None, None, :]) & self.K[:, :, None]).sum(1).max(1)
        return np.bincount(self.cls, weights=np.maximum(cnt, 1), minlength=len(self.w))


_dealings = {}


def tile_share(P, tile, enum, strides):
    """(conflict share = further passes / all passes over the rows of an interior tile, passes per
    chunk of the dense dealing, chunks walked relative to the dense dealing: a padded enumeration's idle lanes)"""
    pad8 = enum.startswith("pad8:")
    orders = ORDERS if enum == "best" else [enum.split(":")[-1]]
    if enum == "bank":
        orders = ["xyz"]
    ds = []
    for o in orders:
        k = (P, tile, o, pad8, tuple(strides) if enum == "bank" else None)
        if k not in _dealings:
            _dealings[k] = Dealing(P, tile, o, pad8, strides if enum == "bank" else None)
        ds.append(_dealings[k])
    p = np.min([d.passes(strides) for d in ds], axis=0)      # ('best': per row class)
    d = ds[0]
    tot = float((d.w * p).sum())
    chunks, chunks0 = float((d.w * d.chunks).sum()), float((d.w * d.chunks0).sum())
    return (tot - 2 * chunks) / tot, tot / (2.0 * chunks0), chunks / chunks0


def current_layout(P):
    """(enumeration, strides) of the kernel as committed: lines of 2 P - 1 floats; 9^3 walks z-runs on
    a plane stride padded to 9 mod 32, 7^3 deals by banks (rw_bankdeal)"""
    WX = 2 * P - 1
    SZ = WX * WX
    if P == 9:
        return "xzy", (1, WX, SZ + ((9 - SZ % 32) + 32) % 32)
    return ("bank" if P == 7 else "xyz"), (1, WX, SZ)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patch", type=int, default=0)
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--tile", default="8x16x16")
    ap.add_argument("--enum", default=None, help="xyz | xzy | ... | best | bank | pad8:xyz instead of the kernel's")
    args = ap.parse_args()
    if not args.search:
        for P in ([args.patch] if args.patch else [5, 7, 9]):
            enum, st = current_layout(P)
            if args.enum:
                enum = args.enum
            for tile in ((8, 16, 16), (8, 8, 16), (16, 8, 16)):
                s, rel, ch = tile_share(P, tile, enum, st)
                print(json.dumps({"patch": P, "tile": "%dx%dx%d" % tile, "enum": enum, "strides": st,
                                  "conflict_share": round(s, 3), "passes_per_dense_chunk": round(2 * rel, 3)}))
        return
    P = args.patch or 7
    tile = tuple(int(v) for v in args.tile.split("x"))
    WX = 2 * P - 1
    res = []
    # strides mod 32 decide the banks; x stays the contiguous axis (SX = 1: any odd SX is the same
    # lattice up to a renaming of the banks), the line is padded by 0 .. 31 floats, the plane by 0 .. 31
    for enum in ORDERS + ["best", "pad8:xyz", "pad8:xzy"]:
        for py in range(32):
            sy = WX + py
            for pz in range(32):
                sz = WX * sy + pz
                s, rel, ch = tile_share(P, tile, enum, (1, sy, sz))
                res.append((rel, s, ch, enum, sy, sz))
        best = min(r for r in res if r[3] == enum)
        print(json.dumps({"patch": P, "tile": args.tile, "enum": enum, "line_stride": best[4], "plane_stride": best[5],
                          "conflict_share": round(best[1], 3), "passes_per_dense_chunk": round(2 * best[0], 3),
                          "chunks_vs_dense": round(best[2], 3)}), flush=True)


if __name__ == "__main__":
    main()
