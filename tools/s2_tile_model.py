"""CPU model of a rank_wg_kernel launch (ppp_rank_wg.hip): the launcher's own tile weight
(rank_tile_weight_kernel: per valid voxel of the tile grown by the radius, ceil(items / 64) + 1) with every voxel
valid, the y-major tile numbering, and the eight XCD ranges -- contiguous, by tile count or cut at the prefix sums
of the weight (rank_tile_order_kernel, clamped to the slots) -- for tiles t x 16 x 16 of every thickness t.
Set it against the sweep in profiles/r12_a_s2_tile_sweep.txt: the model knows nothing about how a CU behaves
with fewer resident workgroups or with a launch in lockstep.

    python tools/s2_tile_model.py [--size 140] [--patch 7] [--resident 5] [--cus 32]"""
import argparse
import itertools
import json


def axis_counts(c0, t, lo, hi, p):
    """for the voxels u of the tile [c0, c0 + t) grown by the radius and cut to [lo, hi): how many have
    n = 1 .. p of their p window positions with the centre inside the tile"""
    r = p // 2
    cnt = [0] * (p + 1)
    for u in range(max(c0 - r, lo), min(c0 + t - 1 + r, hi - 1) + 1):
        n = min(p - 1, u + r - c0) - max(0, u + r - (c0 + t - 1)) + 1
        if n > 0:
            cnt[n] += 1
    return cnt


def tile_weights(size, p, tz, ty=16, tx=16):
    """weights in y-major tile order (x fastest, then z, then y), and the rows the launch stages"""
    cdiv = lambda a, b: -(-a // b)
    nz, ny, nx = cdiv(size, tz), cdiv(size, ty), cdiv(size, tx)
    per_axis = []
    for n, t in ((nz, tz), (ny, ty), (nx, tx)):
        per_axis.append([axis_counts(i * t, min(t, size - i * t), 0, size, p) for i in range(n)])
    chunks = [[[(a * b * c + 63) // 64 + 1 for c in range(p + 1)] for b in range(p + 1)] for a in range(p + 1)]
    w, rows = [], 0
    for iy, iz, ix in itertools.product(range(ny), range(nz), range(nx)):
        cz, cy, cx = per_axis[0][iz], per_axis[1][iy], per_axis[2][ix]
        s = 0
        for a in range(1, p + 1):
            for b in range(1, p + 1):
                for c in range(1, p + 1):
                    s += cz[a] * cy[b] * cx[c] * chunks[a][b][c]
        w.append(s)
        rows += sum(cz) * sum(cy) * sum(cx)
    return w, rows


def ranges_by_count(w):
    per = -(-len(w) // 8)
    return [min(k * per, len(w)) for k in range(9)]


def ranges_by_weight(w, slots):
    total, cut, run, i = sum(w), [0], 0, 0
    for k in range(1, 8):
        want = (total * k + 7) // 8
        while i < len(w) and run < want:
            run += w[i]
            i += 1
        cut.append(i)
    cut.append(len(w))
    for k in range(1, 8):
        cut[k] = min(max(cut[k], cut[k - 1], len(w) - (8 - k) * slots), cut[k - 1] + slots)
    return cut


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=140)
    ap.add_argument("--patch", type=int, default=7)
    ap.add_argument("--resident", type=int, default=5, help="workgroups a CU holds")
    ap.add_argument("--cus", type=int, default=32, help="CUs per XCD")
    args = ap.parse_args()
    res = args.resident * args.cus
    for t in range(8, 17):
        w, rows = tile_weights(args.size, args.patch, t)
        per = -(-len(w) // 8)
        line = {"t": t, "tiles": len(w), "per_xcd": per, "fits_one_round": per <= res, "total_weight": sum(w), "rows_staged": rows}
        for kind, cut in (("count", ranges_by_count(w)), ("weight", ranges_by_weight(w, per + (per + 3) // 4))):
            xw = [sum(w[a:b]) for a, b in zip(cut[:-1], cut[1:])]
            line[kind] = {"lightest_xcd": min(xw), "heaviest_xcd": max(xw), "longest_range": max(b - a for a, b in zip(cut[:-1], cut[1:]))}
        print(json.dumps(line))


if __name__ == "__main__":
    main()
