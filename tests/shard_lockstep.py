"""k shards of the sharded greedy cover / set-cover thinning stepping together in ONE process.

tiling.sharded_cover_own / sharded_thin_own run one shard per rank and exchange the boundary zones
through a communicator.  Here the same rounds run on every shard of a volume in turn, the MIN that
the communicator would take is taken in place, and after every step the shards of every "side" --
backend.CoverShard / ThinShard on CUDA tensors, OracleCoverShard / OracleThinShard on CPU tensors --
are handed to a callback that compares them (tests/test_shard_steps.py).  TEST INFRASTRUCTURE ONLY.

Geometry, zones and membership are tiling's: a shard holds its own slices + pz - 1 halo slices
(clipped) with local linear indices and origin_z = first slice; a zone is the 2(pz - 1) slices around
an internal slab boundary; a shard takes part in the zones at its own two boundaries."""
import numpy as np
import torch

from patchperpix_amd import backend, synth
from patchperpix_amd.flags import FLYLIGHT_NOTHIN_CC as FLAGS

INT32_MAX = 0x7FFFFFFF
INT64_MAX = 0x7FFFFFFFFFFFFFFF
COUNT, FILTER, SELECT = 0, 1, 2


class Case:
    """Inputs of one volume (synth.make_case): the mask to cover (foreground and not overlap), the
    prediction, and a seeded random permutation of the interior centres of the mask -- the "ranked
    list" of the cover, the "selected list" of the thinning (index = position)."""

    def __init__(self, shape, ps, seed=3):
        self.shape, self.ps = tuple(int(v) for v in shape), tuple(int(p) for p in ps)
        c = synth.make_case(self.shape, self.ps, seed, cell=[max(p + 2, 6) for p in self.ps], overlap_frac=0.02)
        self.pred = c["pred"]
        self.mask = (c["foreground"] & (c["numinst"] <= 1)).astype(np.uint8)
        self.rad = tuple(p // 2 for p in self.ps)
        self.radslice = tuple(slice(r, s - r) for r, s in zip(self.rad, self.shape))
        inner = np.zeros(self.shape, dtype=bool)
        inner[self.radslice] = self.mask[self.radslice] != 0
        centres = np.argwhere(inner)
        self.centres = np.ascontiguousarray(centres[np.random.RandomState(seed).permutation(len(centres))])
        Z, Y, X = self.shape
        self.lin = (self.centres[:, 0].astype(np.int64) * Y + self.centres[:, 1]) * X + self.centres[:, 2]
        self.n = len(self.lin)
        self.interior = int(np.count_nonzero(self.mask[self.radslice]))
        self._bits = {}

    def params(self, a=0, b=None):
        Z, Y, X = self.shape
        b = Z if b is None else b
        return backend.make_params((b - a, Y, X), self.ps, origin=(a, 0, 0), **dict(FLAGS))

    def bits(self, side):
        """patch bits of every centre, in list order (prediction > 0.5 at the centre)"""
        if side.name not in self._bits:
            self._bits[side.name] = side.patch_bits(self)
        return self._bits[side.name]


class ModelSide:
    """The NumPy models of tests/oracle_ops.py on CPU tensors."""
    name, device = "model", "cpu"

    def __init__(self):
        import oracle_ops
        self.cover_cls, self.thin_cls = oracle_ops.OracleCoverShard, oracle_ops.OracleThinShard
        self.ops = oracle_ops.OracleOps()

    def patch_bits(self, case):
        return self.ops.patch_bits(torch.from_numpy(case.pred), torch.from_numpy(case.centres), 0.5, case.params())


class DeviceSide:
    """The HIP kernels behind backend.CoverShard / ThinShard on CUDA tensors."""
    name, device = "device", "cuda"

    def __init__(self):
        self.cover_cls, self.thin_cls = backend.CoverShard, backend.ThinShard

    def patch_bits(self, case):
        return backend.patch_bits(torch.from_numpy(case.pred).cuda(),
                                  torch.from_numpy(case.centres.astype(np.int32)).cuda(), 0.5, case.params())


class Geometry:
    """Slabs, local buffers, zones and who takes part in which -- restated here, held to tiling.zone_geometry
    by test_shard_zones_match_the_lockstep_geometry."""

    def __init__(self, case, cuts):
        self.case = case
        Z, Y, X = case.shape
        self.h = h = case.ps[0] - 1
        self.plane = Y * X
        self.ranges = [(int(cuts[i]), int(cuts[i + 1])) for i in range(len(cuts) - 1)]
        assert self.ranges[0][0] == 0 and self.ranges[-1][1] == Z and all(z1 > z0 for z0, z1 in self.ranges)
        self.k = len(self.ranges)
        self.ab = [(max(0, z0 - h), min(Z, z1 + h)) for z0, z1 in self.ranges]
        self.bounds = [r[1] for r in self.ranges[:-1]]
        self.zones = [(max(0, zb - h), min(Z, zb + h)) for zb in self.bounds]
        self.mine = [[i for i, zb in enumerate(self.bounds) if zb == z0 or zb == z1] for z0, z1 in self.ranges]
        self.zlen = 2 * h * self.plane
        cz = case.centres[:, 0]
        self.own_idx = [np.flatnonzero((cz >= z0) & (cz < z1)) for z0, z1 in self.ranges]       # ascending = list order
        self.in_zone = np.zeros(case.n, dtype=bool)
        for lo, hi in self.zones:
            self.in_zone |= (cz >= lo) & (cz < hi)

    def own_loc(self, s):
        return self.ranges[s][0] - self.ab[s][0], self.ranges[s][1] - self.ab[s][0]

    def zone_loc(self, s, i):
        return self.zones[i][0] - self.ab[s][0], self.zones[i][1] - self.ab[s][0]

    def zone_n(self, i):
        return (self.zones[i][1] - self.zones[i][0]) * self.plane

    def global_zyx(self, s, local_linear):
        """(z, y, x) in the whole volume of a linear index into shard s's local buffer"""
        Y, X = self.case.shape[1:]
        v = int(local_linear)
        return (v // (Y * X) + self.ab[s][0], (v // X) % Y, v % X)

    def zone_zyx(self, i, t):
        """(z, y, x) in the whole volume of element t of zone i's buffer"""
        Y, X = self.case.shape[1:]
        t = int(t)
        return (t // (Y * X) + self.zones[i][0], (t // X) % Y, t % X)


class Shards:
    """One side's k shard objects of one volume, with the buffers the zones travel in."""

    def __init__(self, side, geo, thin):
        self.side, self.geo, self.thin = side, geo, thin
        case, dev = geo.case, side.device
        bits = case.bits(side)
        self.mask_ab, self.shards, self.own_t = [], [], []
        for s in range(geo.k):
            a, b = geo.ab[s]
            own = geo.own_idx[s]
            own_t = torch.from_numpy(own).to(dev)
            mask_ab = torch.from_numpy(case.mask[a:b].copy()).to(dev)
            lin_local = torch.from_numpy(case.lin[own] - a * geo.plane).to(dev).contiguous()
            b_own = bits[own_t].contiguous()
            P = case.params(a, b)
            if thin:
                shard = side.thin_cls(mask_ab, lin_local, torch.from_numpy(own.astype(np.int64)).to(dev), b_own, P, case.shape[0])
            else:
                shard = side.cover_cls(mask_ab, lin_local, torch.from_numpy(own.astype(np.int32)).to(dev), b_own, P, case.shape[0])
            self.mask_ab.append(mask_ab)
            self.shards.append(shard)
            self.own_t.append(own_t)
        nz = max(len(geo.zones), 1)
        self.key_dtype = torch.int64 if thin else torch.int32
        self.key_none = INT64_MAX if thin else INT32_MAX
        # per shard, as every rank has its own: [zone][zlen] ranks / keys, [zone][mask | clean][zlen]
        self.key_buf = [torch.empty((nz, geo.zlen), dtype=self.key_dtype, device=dev) for _ in range(geo.k)]
        self.mask_buf = [torch.empty((nz, 2, geo.zlen), dtype=torch.uint8, device=dev) for _ in range(geo.k)]

    # -- what a test may look at, through the public interface only
    def list_np(self, s, name):
        t = getattr(self.shards[s], name)
        return t[:len(self.geo.own_idx[s])].cpu().numpy()

    def volume(self, s, with_key):
        """the complete local rank / key volume, or (running mask, clean bytes): zone(False, 0, Zl, own = all)"""
        a, b = self.geo.ab[s]
        Zl, n = b - a, (b - a) * self.geo.plane
        dev = self.side.device
        if with_key:
            buf = torch.empty(n, dtype=self.key_dtype, device=dev)
            self.shards[s].zone(False, 0, Zl, (0, Zl), key=buf)
            return buf.cpu().numpy()
        m, c = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        self.shards[s].zone(False, 0, Zl, (0, Zl), mask=m, clean=c)
        return m.cpu().numpy(), c.cpu().numpy()

    def zone_io(self, imp, s, i, with_key, buf=None):
        lo, hi = self.geo.zone_loc(s, i)
        if with_key:
            buf = self.key_buf[s] if buf is None else buf
            self.shards[s].zone(imp, lo, hi, self.geo.own_loc(s), key=buf[i])
        else:
            buf = self.mask_buf[s] if buf is None else buf
            self.shards[s].zone(imp, lo, hi, self.geo.own_loc(s), mask=buf[i, 0], clean=buf[i, 1])

    def reexport(self, s, with_key):
        """the shard's real zones exported once more (after an import), into buffers of their own"""
        buf = torch.empty_like(self.key_buf[s] if with_key else self.mask_buf[s])
        for i in self.geo.mine[s]:
            self.zone_io(False, s, i, with_key, buf)
        return buf


def _exchange(sh, with_key, on_step, tag):
    """Step 2 / 4: every shard exports its zones; element-wise MIN over the shards (the all-reduce; with
    two neighbours per zone also what neighbour_min leaves); every shard imports its zones."""
    geo = sh[0].geo
    if not geo.zones:
        return
    for side in sh:
        bufs = side.key_buf if with_key else side.mask_buf
        for s in range(geo.k):
            bufs[s].fill_(side.key_none if with_key else 1)
            for i in geo.mine[s]:
                side.zone_io(False, s, i, with_key)
    if on_step:
        on_step(tag + ("export",), sh)
    for side in sh:
        bufs = side.key_buf if with_key else side.mask_buf
        low = bufs[0].clone()
        for s in range(1, geo.k):
            low = torch.minimum(low, bufs[s])
        for s in range(geo.k):
            bufs[s].copy_(low)
            for i in geo.mine[s]:
                side.zone_io(True, s, i, with_key)
    if on_step:
        on_step(tag + ("import",), sh)


def _rounds(sh, step_args, on_step, tag):
    """COUNT, exchange ranks / keys, FILTER, SELECT, exchange mask and clean bytes, until no shard of
    the FIRST side is alive (the comparison holds the others to it).  Returns the number of rounds."""
    rounds, alive = 0, True
    while alive:
        t = tag + (rounds,)
        for side in sh:
            for shard in side.shards:
                shard.step(COUNT, *step_args)
        if on_step:
            on_step(t + ("count", ""), sh)
        _exchange(sh, True, on_step, t + ("keys",))
        for side in sh:
            for shard in side.shards:
                shard.step(FILTER)
        if on_step:
            on_step(t + ("filter", ""), sh)
        for side in sh:
            for shard in side.shards:
                shard.step(SELECT, *step_args)
        if on_step:
            on_step(t + ("select", ""), sh)
        _exchange(sh, False, on_step, t + ("mask",))
        alive = any(shard.alive() for shard in sh[0].shards)
        rounds += 1
        assert rounds < 10000, "the rounds do not end"
    return rounds


def gather(side, name):
    """a per-patch list of all shards, in the order of the whole list"""
    geo = side.geo
    out = np.zeros(geo.case.n, dtype=np.int64)
    for s in range(geo.k):
        out[geo.own_idx[s]] = side.list_np(s, name)
    return out


def own_mask(side):
    """the callers' mask tensors, every shard's OWN slices, put together"""
    geo = side.geo
    out = np.zeros(geo.case.shape, dtype=np.uint8)
    for s in range(geo.k):
        lo, hi = geo.own_loc(s)
        out[geo.ranges[s][0]:geo.ranges[s][1]] = side.mask_ab[s][lo:hi].cpu().numpy()
    return out


def run_cover(case, cuts, sides, pix_ths, on_step=None):
    """The passes of sharded_cover_own on every side in lockstep: every pass restarts with open(state),
    state 1 for the patches selected so far; between passes the loop's stop rule is applied as there.
    Returns a dict per pass: state / cleared of the first side in list order, rounds, the selection so far."""
    geo = Geometry(case, cuts)
    sh = [Shards(side, geo, thin=False) for side in sides]
    selected = np.zeros(case.n, dtype=bool)
    remaining = case.interior
    passes = []
    for p, pix_th in enumerate(pix_ths):
        if remaining <= 0:
            break
        for side in sh:
            for s in range(geo.k):
                st = torch.from_numpy(selected[geo.own_idx[s]].astype(np.int32))
                side.shards[s].open(st.to(side.side.device))
        if on_step:
            on_step((p, pix_th, -1, "open", ""), sh)
        rounds = _rounds(sh, (pix_th,), on_step, (p, pix_th))
        for side in sh:
            for shard in side.shards:
                shard.close()
        if on_step:
            on_step((p, pix_th, rounds, "close", ""), sh)
        state, cleared = gather(sh[0], "state"), gather(sh[0], "cleared")
        new = np.flatnonzero((state == 1) & ~selected)          # list order = rank order
        left = remaining - np.cumsum(cleared[new])
        done = np.flatnonzero(left <= 0)
        if len(done):
            new, remaining = new[:done[0] + 1], 0
        elif len(new):
            remaining = int(left[-1])
        selected[new] = True
        passes.append(dict(pix_th=pix_th, state=state, cleared=cleared, rounds=rounds, selected=selected.copy(),
                           mask=own_mask(sh[0])))
    return dict(geo=geo, passes=passes, sides=sh)


def run_thin(case, cuts, sides, on_step=None):
    """The rounds of sharded_thin_own on every side in lockstep."""
    geo = Geometry(case, cuts)
    sh = [Shards(side, geo, thin=True) for side in sides]
    if on_step:
        on_step((0, None, -1, "open", ""), sh)
    rounds = _rounds(sh, (), on_step, (0, None))
    for side in sh:
        for shard in side.shards:
            shard.close()
    if on_step:
        on_step((0, None, rounds, "close", ""), sh)
    return dict(geo=geo, sides=sh, passes=[dict(
        pix_th=None, state=gather(sh[0], "state"), cleared=gather(sh[0], "cleared"), count=gather(sh[0], "count"),
        rounds=rounds, mask=own_mask(sh[0]))])
