"""The step-wise device interfaces of the multi-rank path next to their NumPy models.

backend.CoverShard / ThinShard / LabelState / pair_counts_subset / pairs_subset each have a model with the
same contract in tests/oracle_ops.py; the CPU suite drives the tiled assembly through the models and the
multi-process GPU test compares final instance maps only.  Here a device object and its model run side by
side in ONE process and are compared after every step, so a difference is reported where it arises: pass,
round, step, shard, voxel, both values.  All comparisons are exact."""
import numpy as np
import pytest

import shard_lockstep as ls

# shape, patch, slab cuts, what runs ("c0": cover [0]; "c10": cover [10, 0]; "thin") -- the smallest shapes
# at which each hazard exists
VOLUMES = {
    # X = 33 spills one bit into a second mask word; > 4096 voxels: several count workgroups
    "base": ((20, 12, 33), (5, 5, 5), (0, 10, 20)),
    # slabs of 5 and 4 slices, thinner than the 8-slice zone (the all-reduce form); a shard between two zones
    "thin_slabs": ((22, 11, 32), (5, 5, 5), (0, 5, 9, 22)),
    # a middle shard with two neighbours; two full mask words, windows straddle the word boundary
    "three": ((21, 13, 64), (5, 5, 5), (0, 7, 14, 21)),
    "p7": ((26, 14, 34), (7, 7, 7), (0, 13, 26)),
    # the headline patch size, py == MAXPY of the count kernel
    "p9": ((28, 20, 36), (9, 9, 9), (0, 14, 28)),
    # py = 11: the count kernel's generic row loop; anisotropic radius
    "aniso": ((12, 26, 34), (3, 11, 11), (0, 6, 12)),
}
RUNS = [("base", "c0"), ("base", "c10"), ("base", "thin"), ("thin_slabs", "c10"), ("thin_slabs", "thin"),
        ("three", "c10"), ("p7", "c0"), ("p7", "thin"), ("p9", "c0"), ("aniso", "c10"), ("aniso", "thin")]
PIX_THS = {"c0": [0], "c10": [10, 0]}
SEED = 3
_CASES = {}


def case_of(name):
    if name not in _CASES:
        shape, ps, _ = VOLUMES[name]
        _CASES[name] = ls.Case(shape, ps, SEED)
    return _CASES[name]


def run(name, what, sides, on_step=None, cuts=None):
    case = case_of(name)
    cuts = VOLUMES[name][2] if cuts is None else cuts
    if what == "thin":
        return ls.run_thin(case, cuts, sides, on_step)
    return ls.run_cover(case, cuts, sides, PIX_THS[what], on_step)


def assert_not_quiet(res, what):
    """A case must exercise what it is for: selections inside the boundary zones, many rounds, and in the
    [10, 0] cover a patch that the pix_th = 10 pass drops and the pix_th = 0 pass selects."""
    geo, passes = res["geo"], res["passes"]
    taken = np.zeros(geo.case.n, dtype=bool)
    for p in passes:
        taken |= p["state"] == 1
    in_zone, rounds = int(np.count_nonzero(taken & geo.in_zone)), sum(p["rounds"] for p in passes)
    print("%s %s: %d patches, %d selected, %d of them in a zone, %d rounds" % (
        geo.case.shape, what, geo.case.n, int(taken.sum()), in_zone, rounds))
    assert in_zone >= 20, "only %d selections inside a boundary zone" % in_zone
    assert rounds > 16, "only %d rounds" % rounds
    if what == "c10":
        assert len(passes) == 2, "the pix_th = 10 pass emptied the interior"
        assert np.any((passes[0]["state"] == 2) & (passes[1]["state"] == 1)), \
            "no patch is dropped at pix_th = 10 and selected at pix_th = 0"


# ---- the driver against itself: k model shards == one model shard over the whole volume ------------------
@pytest.mark.parametrize("name,what", RUNS)
def test_model_shards_equal_one_model_shard(name, what):
    side = ls.ModelSide()
    cut = run(name, what, [side])
    whole = run(name, what, [side], cuts=(0, VOLUMES[name][0][0]))
    assert_not_quiet(cut, what)
    assert len(cut["passes"]) == len(whole["passes"])
    for p, (a, b) in enumerate(zip(cut["passes"], whole["passes"])):
        for key in ("state", "cleared", "count", "mask"):
            if key in a:
                assert np.array_equal(a[key], b[key]), "pass %d: %s of the shards differs from the whole volume's" % (p, key)
        assert (a["state"] == 1).any()


# ---- the product's zone geometry against the driver's -----------------------------------------------------
# all(z1 - z0 >= 2 (pz - 1)) from the cuts above: slabs of 10, 10 against 8; 13, 13 against 12; 6, 6 against 4 --
# and 5, 4, 13 against 8; 7, 7, 7 against 8; 14, 14 against 16
PAIRWISE = {"base": True, "p7": True, "aniso": True, "thin_slabs": False, "three": False, "p9": False}


def test_shard_zones_match_the_lockstep_geometry():
    """tiling.zone_geometry -- what the product's round loop exchanges -- gives every shard of every volume the
    buffer [a, b), zones, membership, own slices and zone length of shard_lockstep.Geometry, the independent
    restatement that the step tests run on; and "a zone concerns two neighbours only" where no slab is thinner
    than a zone."""
    from types import SimpleNamespace
    from patchperpix_amd import tiling
    assert set(PAIRWISE) == set(VOLUMES)
    for name, (shape, ps, cuts) in VOLUMES.items():
        geo = ls.Geometry(SimpleNamespace(shape=shape, ps=ps, centres=np.zeros((0, 3), dtype=np.int64), n=0), cuts)
        assert geo.k == len(cuts) - 1 >= 2
        for s in range(geo.k):
            g = tiling.zone_geometry(geo.ranges, geo.ranges[s], ps[0] - 1, shape[0])
            what = "%s, shard %d" % (name, s)
            assert (g.a, g.b) == geo.ab[s], what
            assert list(g.bounds) == geo.bounds and list(g.zones) == geo.zones, what
            assert list(g.mine) == geo.mine[s] and len(g.mine) == (1 if s in (0, geo.k - 1) else 2), what
            assert tuple(g.own_loc) == geo.own_loc(s), what
            assert g.zslices * shape[1] * shape[2] == geo.zlen, what
            assert g.pairwise is PAIRWISE[name], what


# ---- device against model, step by step -------------------------------------------------------------------
def _fail(tag, thin, s, what, where, dev, mod):
    p, pix_th, rnd, step, phase = tag
    head = "thinning" if thin else "cover pass %d (pix_th %d)" % (p, pix_th)
    raise AssertionError("%s, round %d, step %s%s, shard %d: %s differs, first at (z, y, x) = %s: device %s, model %s" % (
        head, rnd, step, " " + phase if phase else "", s, what, where, dev, mod))


def compare(tag, sh):
    """The comparison callback of shard_lockstep: everything the public interface shows of every shard.

    `clean` bytes: the model marks the clipped (2p-1)^3 box of centres at every select and clears all marks
    at every count; the device keeps the same marks in the thinning and in cover passes with pix_th > 0, and
    they are compared exactly there.  In a pix_th == 0 cover pass the device decides "does the patch still
    cover any voxel" from one witness voxel per patch (csrc/ppp_cover.hip, witness_ok): it neither consumes nor
    sets dirty marks (mark_dirty = 0), so its clean bytes carry no information in that pass and are not
    compared -- the states, ranks and masks that the marks exist to keep right are."""
    mod, dev = sh
    geo, thin = mod.geo, mod.thin
    p, pix_th, rnd, step, phase = tag
    pz, py, px = geo.case.ps
    clean_too = thin or pix_th != 0 or not (pz * py < 2047 and px <= 32)
    for s in range(geo.k):
        centre = lambda i: tuple(int(v) for v in geo.case.centres[geo.own_idx[s][i]])
        d_state, m_state = dev.list_np(s, "state"), mod.list_np(s, "state")
        bad = np.flatnonzero(d_state != m_state)
        if len(bad):
            _fail(tag, thin, s, "state", centre(bad[0]), d_state[bad[0]], m_state[bad[0]])
        for name in ("cleared", "count") if thin else ("cleared",):
            d, m = dev.list_np(s, name), mod.list_np(s, name)
            bad = np.flatnonzero((d != m) & (m_state == 1))
            if len(bad):
                _fail(tag, thin, s, name, centre(bad[0]), d[bad[0]], m[bad[0]])
        if step == "count":
            d, m = dev.shards[s].alive(), mod.shards[s].alive()
            if d != m:
                _fail(tag, thin, s, "alive", "(flag)", d, m)
        d, m = dev.volume(s, True), mod.volume(s, True)
        bad = np.flatnonzero(d != m)
        if len(bad):
            _fail(tag, thin, s, "key volume" if thin else "rank volume", geo.global_zyx(s, bad[0]), d[bad[0]], m[bad[0]])
        (d_mask, d_clean), (m_mask, m_clean) = dev.volume(s, False), mod.volume(s, False)
        bad = np.flatnonzero(d_mask != m_mask)
        if len(bad):
            _fail(tag, thin, s, "running mask", geo.global_zyx(s, bad[0]), d_mask[bad[0]], m_mask[bad[0]])
        bad = np.flatnonzero(d_clean != m_clean) if clean_too else ()
        if len(bad):
            _fail(tag, thin, s, "clean bytes", geo.global_zyx(s, bad[0]), d_clean[bad[0]], m_clean[bad[0]])
        if step in ("keys", "mask"):
            # export: what the shard wrote for its zones; import: what the MIN left -- and what the shard
            # exports for the same zones once it has taken that in
            sets = [(dev.key_buf[s], mod.key_buf[s])] if step == "keys" else [(dev.mask_buf[s], mod.mask_buf[s])]
            names = ["exchanged buffer"]
            if phase == "import":
                sets.append((dev.reexport(s, step == "keys"), mod.reexport(s, step == "keys")))
                names.append("zone exported again")
            for (d_buf, m_buf), what in zip(sets, names):
                for i in geo.mine[s]:
                    n = geo.zone_n(i)
                    parts = [("keys" if thin else "ranks", d_buf[i][:n], m_buf[i][:n])] if step == "keys" else \
                        [("mask", d_buf[i, 0][:n], m_buf[i, 0][:n])] + \
                        ([("clean", d_buf[i, 1][:n], m_buf[i, 1][:n])] if clean_too else [])
                    for part, d, m in parts:
                        d, m = d.cpu().numpy(), m.cpu().numpy()
                        bad = np.flatnonzero(d != m)
                        if len(bad):
                            _fail(tag, thin, s, "%s of zone %d (%s)" % (what, i, part), geo.zone_zyx(i, bad[0]),
                                  d[bad[0]], m[bad[0]])
        if step == "close":
            d, m = dev.mask_ab[s].cpu().numpy().reshape(-1), mod.mask_ab[s].numpy().reshape(-1)
            bad = np.flatnonzero(d != m)
            if len(bad):
                _fail(tag, thin, s, "the caller's mask", geo.global_zyx(s, bad[0]), d[bad[0]], m[bad[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("name,what", RUNS)
def test_device_shards_follow_the_model_step_by_step(name, what):
    """compare() after every step of every round, for every shard (see there for what is compared)."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    mod, dev = ls.ModelSide(), ls.DeviceSide()
    case = case_of(name)
    assert np.array_equal(case.bits(dev).cpu().numpy(), case.bits(mod).numpy()), "patch bits differ"
    res = run(name, what, [mod, dev], compare)
    assert_not_quiet(res, what)
    m, d = res["sides"]
    for key in ("state", "cleared") + (("count",) if what == "thin" else ()):
        sel = ls.gather(m, "state") == 1
        assert np.array_equal(ls.gather(d, key)[sel], ls.gather(m, key)[sel])
    assert np.array_equal(ls.own_mask(d), ls.own_mask(m))


# ---- LabelState against OracleLabelState ------------------------------------------------------------------
LABEL_SHAPE = (9, 11, 13)


def _label_rows():
    """400 nodes; ~3000 rows in id order with aff in {-1, 0, +1}: positive rows join nodes of small clusters
    only (many components), with duplicate rows, self rows, nodes met in negative rows only and nodes in no row."""
    rs = np.random.RandomState(11)
    Z, Y, X = LABEL_SHAPE
    lin = rs.permutation(Z * Y * X)[:400]
    nodes = np.stack(np.unravel_index(lin, LABEL_SHAPE), axis=1).astype(np.int32)
    free, neg_only, used = np.arange(0, 20), np.arange(20, 40), np.arange(40, 400)
    cluster = rs.randint(0, 60, size=len(used))
    u, v, aff = [], [], []
    for _ in range(1400):                                   # inside a cluster: any sign
        c = rs.randint(0, 60)
        members = used[cluster == c]
        if len(members) < 2:
            continue
        a, b = rs.choice(members, 2, replace=False)
        u.append(a); v.append(b); aff.append(rs.choice([0.7, 0.0, -0.4], p=[0.5, 0.2, 0.3]))
    for _ in range(1300):                                   # anywhere: never positive
        a, b = rs.choice(used, 2, replace=False)
        u.append(a); v.append(b); aff.append(rs.choice([0.0, -1.5]))
    for k in neg_only:                                      # met in negative rows only, on either side
        for _ in range(2):
            o = rs.choice(used)
            a, b = (k, o) if rs.rand() < 0.5 else (o, k)
            u.append(a); v.append(b); aff.append(-0.25)
    for a in rs.choice(used, 30, replace=False):            # self rows
        u.append(a); v.append(a); aff.append(rs.choice([0.5, 0.0, -0.5]))
    for j in rs.randint(0, len(u), size=150):               # duplicate rows (other ids, same nodes)
        u.append(u[j]); v.append(v[j]); aff.append(aff[j])
    order = rs.permutation(len(u))                          # ids = positions in this fixed list
    u, v, aff = np.array(u)[order], np.array(v)[order], np.array(aff, dtype=np.float32)[order]
    rows = np.concatenate([nodes[u], nodes[v]], axis=1).astype(np.int32)
    return nodes, rows, aff, free, neg_only


def _roots(parent_lin, node_lin):
    """root (a position in the node list) of every node of a forest given as parent voxel indices"""
    at = {int(l): i for i, l in enumerate(node_lin)}
    par = np.array([at[int(l)] for l in parent_lin])
    while True:
        nxt = par[par]
        if np.array_equal(nxt, par):
            return par
        par = nxt


def _same_partition(a, b):
    pairs = np.unique(np.stack([a, b], axis=1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) and len(np.unique(pairs[:, 1])) == len(pairs)


@pytest.mark.gpu
def test_label_state_follows_its_model_in_any_order_and_split():
    import torch
    from oracle_ops import OracleLabelState
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    nodes, rows, aff, free, neg_only = _label_rows()
    n_rows = len(rows)
    assert 2500 <= n_rows <= 3500
    P = backend.make_params(LABEL_SHAPE, (5, 5, 5), **dict(ls.FLAGS))
    nodes_d = torch.from_numpy(nodes).cuda()
    rows_t, aff_t, gid_t = torch.from_numpy(rows), torch.from_numpy(aff), torch.arange(n_rows, dtype=torch.int64)
    Z, Y, X = LABEL_SHAPE
    node_lin = (nodes[:, 0].astype(np.int64) * Y + nodes[:, 1]) * X + nodes[:, 2]

    def both():
        return OracleLabelState(nodes, LABEL_SHAPE), backend.LabelState(nodes_d, P)

    def add(pair, idx, explicit=True, first_id=0):
        idx = torch.as_tensor(idx, dtype=torch.int64)
        r, a, g = rows_t[idx].contiguous(), aff_t[idx].contiguous(), gid_t[idx].contiguous()
        pair[0].add(r, a, gid=g if explicit else None, first_id=first_id)
        pair[1].add(r.cuda(), a.cuda(), gid=g.cuda() if explicit else None, first_id=first_id)

    def check_export(pair, what):
        (mp, mf, mh), (dp, df, dh) = pair[0].export(), pair[1].export()
        assert np.array_equal(df.cpu().numpy(), mf.numpy()), "%s: firstpos differs" % what
        assert np.array_equal(dh.cpu().numpy(), mh.numpy()), "%s: haspos differs" % what
        assert _same_partition(_roots(dp.cpu().numpy(), node_lin), _roots(mp.numpy(), node_lin)), \
            "%s: the forests are different partitions" % what
        return (mp, mf, mh), (dp, df, dh)

    def finish(pair, what):
        m, d = pair[0].finish().numpy(), pair[1].finish().cpu().numpy()
        assert np.array_equal(d, m), "%s: finish() differs from the model's" % what
        return d

    rs = np.random.RandomState(5)
    results = {}
    # (a) one state, shuffled chunks of 1, 255, 256, 257 rows and the rest, explicit ids
    pair = both()
    order, at = rs.permutation(n_rows), 0
    for size in (1, 255, 256, 257, n_rows):
        add(pair, order[at:at + size])
        at += size
    (_, mf, mh), _ = check_export(pair, "(a)")
    results["a"] = finish(pair, "(a)")
    # the special nodes, from the model's own export (the device's was just held to it)
    assert np.all(mf.numpy()[neg_only] != backend.NONE_KEY64) and not mh.numpy()[neg_only].any()
    assert np.all(results["a"][neg_only] == backend.NONE_KEY64)
    assert np.all(mf.numpy()[free] == backend.NONE_KEY64) and np.all(results["a"][free] == backend.NONE_KEY64)
    n_comp = len(np.unique(results["a"])) - 1
    assert n_comp >= 20, "only %d components" % n_comp
    # (b) in order, ids from first_id
    pair = both()
    for lo, hi in ((0, 1000), (1000, n_rows)):
        add(pair, np.arange(lo, hi), explicit=False, first_id=lo)
    check_export(pair, "(b)")
    results["b"] = finish(pair, "(b)")
    # (c) two and three states with disjoint rows, merged as the ranks merge theirs
    for k in (2, 3):
        owner = rs.randint(0, k, size=n_rows)
        pairs_ = [both() for _ in range(k)]
        for r in range(k):
            add(pairs_[r], rs.permutation(np.flatnonzero(owner == r)))
        exp = [check_export(pairs_[r], "(c) %d states, state %d" % (k, r)) for r in range(k)]
        for side in (0, 1):
            parents = torch.stack([e[side][0] for e in exp])
            firstpos = torch.stack([e[side][1] for e in exp]).min(0).values
            haspos = torch.stack([e[side][2] for e in exp]).max(0).values
            for r in range(k):
                pairs_[r][side].merge(parents, firstpos, haspos)
        for r in range(k):
            check_export(pairs_[r], "(c) %d states merged, state %d" % (k, r))
            results["c%d_%d" % (k, r)] = finish(pairs_[r], "(c) %d states, state %d" % (k, r))
    for key, got in results.items():
        assert np.array_equal(got, results["a"]), "(%s) differs from (a)" % key
    one = backend.label_components(rows_t.cuda(), aff_t.cuda(), nodes_d, P).cpu().numpy()
    want = np.where(results["a"] == backend.NONE_KEY64, backend.NONE_KEY, results["a"])
    assert np.array_equal(one, want), "the one-shot label_components differs"


# ---- pair_counts_subset / pairs_subset against OracleOps ---------------------------------------------------
PAIR_SHAPE = (14, 16, 40)


def _x_sorted(pts):
    pts = np.asarray(pts, dtype=np.int32)
    return np.ascontiguousarray(pts[np.argsort(pts[:, 2], kind="stable")])


def _pair_list(kind):
    rs = np.random.RandomState(17)
    Z, Y, X = PAIR_SHAPE
    if kind == "random":
        return _x_sorted(np.stack(np.unravel_index(rs.permutation(Z * Y * X)[:400], PAIR_SHAPE), axis=1))
    if kind == "ties":          # five x columns only: the order inside a column is the (stable) input order
        zy = rs.permutation(Z * Y * 5)[:300]
        return _x_sorted(np.stack([zy // (Y * 5), (zy // 5) % Y, np.array([3, 4, 9, 20, 21])[zy % 5]], axis=1))
    # "scan": groups of 64, 65, 66 and 129 patches within three x columns, 12 columns apart: the first patch of
    # a group has exactly 63, 64, 65, 128 candidates in its partner scan range (x_j - x_i <= max_ps_dist * 5)
    pts = []
    for x0, m in ((0, 64), (12, 65), (24, 66), (36, 129)):
        zy = rs.permutation(Z * Y)[:m]
        xs = np.sort(rs.randint(0, 3, size=m))
        xs[0] = 0
        pts.append(np.stack([zy // Y, zy % Y, x0 + xs], axis=1))
    return _x_sorted(np.concatenate(pts))


def _subsets(n):
    return {"empty": np.zeros(0, np.int64), "first": np.array([0]), "last": np.array([n - 1]), "all": np.arange(n),
            "every third": np.arange(0, n, 3), "run": np.arange(n // 3, n // 3 + 70), "last 5": np.arange(n - 5, n)}


@pytest.mark.gpu
@pytest.mark.parametrize("kind,ps", [("random", (5, 5, 5)), ("random", (3, 5, 7)), ("scan", (5, 5, 5)), ("ties", (5, 5, 5))])
def test_pairs_of_a_subset_follow_the_model(kind, ps):
    import torch
    from oracle_ops import OracleOps
    from patchperpix_amd import backend
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    pts = _pair_list(kind)
    n = len(pts)
    assert len(np.unique(pts, axis=0)) == n and np.all(np.diff(pts[:, 2]) >= 0)
    P = backend.make_params(PAIR_SHAPE, ps, **dict(ls.FLAGS))
    pts_t, pts_d = torch.from_numpy(pts), torch.from_numpy(pts).cuda()
    model = OracleOps()
    for d in (1, 2):
        if kind == "scan":
            x = pts[:, 2]
            cand = np.searchsorted(x, x + d * ps[2], side="right") - np.arange(n) - 1
            assert {63, 64, 65, 128} <= set(cand.tolist())
        whole_m = model.pair_counts(pts_t, torch.arange(n), P, d)
        whole_d = backend.pair_counts_subset(pts_d, torch.arange(n, device="cuda"), P, max_ps_dist=d)
        assert np.array_equal(whole_d.cpu().numpy(), whole_m.numpy()), "counts of the whole list, max_ps_dist %d" % d
        n_rows = int(whole_m.sum())
        assert n_rows > n
        goff_m = torch.cumsum(whole_m, 0) - whole_m
        goff_d = goff_m.cuda()
        for name, sub in _subsets(n).items():
            what = "%s, max_ps_dist %d, subset %s" % (kind, d, name)
            sub_t = torch.from_numpy(sub.astype(np.int64))
            got = backend.pair_counts_subset(pts_d, sub_t.cuda(), P, max_ps_dist=d).cpu().numpy()
            assert np.array_equal(got, model.pair_counts(pts_t, sub_t, P, d).numpy()), what + ": counts"
            for single in (True, False):
                want_rows, want_gid = model.pairs_subset(pts_t, sub_t, whole_m, goff_m, n_rows, P, d, single)
                rows, gid = backend.pairs_subset(pts_d, sub_t.cuda(), whole_d, goff_d, n_rows, P, max_ps_dist=d,
                                                 include_single=single)
                if want_rows is None:
                    assert rows is None and gid is None, what
                    continue
                assert rows is not None, what
                assert np.array_equal(rows.cpu().numpy(), want_rows.numpy()), what + ": rows (single %s)" % single
                assert np.array_equal(gid.cpu().numpy(), want_gid.numpy()), what + ": ids (single %s)" % single
                if single:
                    assert np.array_equal(want_gid.numpy()[-len(sub):], n_rows + sub), what + ": self-row ids"
        # a partition of the list into three subsets, put together by id, is the one-shot list
        for single in (True, False):
            want = backend.device_patch_pairs(pts_d, P, max_ps_dist=d, include_single=single).cpu().numpy()
            assert len(want) == n_rows + (n if single else 0), "the counts do not sum to the one-shot row count"
            parts = [backend.pairs_subset(pts_d, torch.arange(r, n, 3, device="cuda"), whole_d, goff_d, n_rows, P,
                                          max_ps_dist=d, include_single=single) for r in range(3)]
            rows = torch.cat([p[0] for p in parts]).cpu().numpy()
            gid = torch.cat([p[1] for p in parts]).cpu().numpy()
            assert np.array_equal(np.sort(gid), np.arange(len(want)))
            assert np.array_equal(rows[np.argsort(gid)], want), "%s, max_ps_dist %d: union of three subsets" % (kind, d)
