"""Time the watershed's host loop (ppp_host_mws_sorted) on a synthetic edge list: a 3-d grid of
nodes, edges to the neighbours within `reach`, random order (the loop takes edges that are already
sorted by |aff|), a given share of repulsive edges -- the decoded-noise workload of dec256_p7 has
about half -- or on an edge list saved by tools/dump_host_stage_inputs.py (--edges FILE.npz with
eu, ev, n_nodes).  The plain loop (PPP_MWS_PRUNE=0) and the blocked loop with the prune alternate
in one process; the blocked loop's line carries the stats array of ppp_host_mws_sorted_stats.
--classes: what every edge of the list does in the plain loop, and the loop's time with each class
of edges taken out of the list beforehand.
    python tools/time_mws.py [--n 96] [--reach 2] [--repulsive 0.5] [--edges FILE.npz] [--classes]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CLASSES = ("attractive: both unassigned (new id)", "attractive: one unassigned (joins)",
           "attractive: both assigned (merge)", "attractive: same cluster", "attractive: refused by a mutex key",
           "repulsive: same cluster", "repulsive: key already there", "repulsive: key inserted")


def grid_edges(args):
    rng = np.random.default_rng(0)
    n = args.n
    idx = np.arange(n ** 3, dtype=np.int64).reshape(n, n, n)
    eu, ev = [], []
    r = args.reach
    for dz in range(0, r + 1):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if (dz, dy, dx) <= (0, 0, 0):
                    continue
                a = idx[:n - dz, max(0, -dy):n - max(0, dy), max(0, -dx):n - max(0, dx)]
                b = idx[dz:, max(0, dy):n - max(0, -dy), max(0, dx):n - max(0, -dx)]
                keep = rng.random(a.shape) < args.keep
                eu.append(a[keep]); ev.append(b[keep])
    eu = np.concatenate(eu).astype(np.int32); ev = np.concatenate(ev).astype(np.int32)
    order = rng.permutation(len(eu))
    eu, ev = eu[order], ev[order]
    attractive = rng.random(len(eu)) >= args.repulsive
    ev = np.where(attractive, ev | np.int32(-2 ** 31), ev).astype(np.int32)
    return eu, ev, n ** 3


def run(backend, eu, ev, n_nodes, prune):
    """one call: (ms, ids issued, labels, stats)"""
    L = backend.lib()
    labels = np.zeros(n_nodes, dtype=np.int32)
    stats = np.zeros(8, dtype=np.int64)
    if prune:
        os.environ.pop("PPP_MWS_PRUNE", None)
    else:
        os.environ["PPP_MWS_PRUNE"] = "0"
    t0 = time.perf_counter()
    issued = int(L.ppp_host_mws_sorted_stats(backend._np_ptr(eu), backend._np_ptr(ev), len(eu), n_nodes,
                                             backend._np_ptr(labels), backend._np_ptr(stats)))
    dt = time.perf_counter() - t0
    os.environ.pop("PPP_MWS_PRUNE", None)
    return dt * 1e3, issued, labels, stats


def best_plain(backend, eu, ev, n_nodes, repeat):
    eu, ev = np.ascontiguousarray(eu), np.ascontiguousarray(ev)
    return min(run(backend, eu, ev, n_nodes, False)[0] for _ in range(repeat))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=96)
    ap.add_argument("--reach", type=int, default=2)
    ap.add_argument("--repulsive", type=float, default=0.5)
    ap.add_argument("--keep", type=float, default=0.5, help="share of the candidate edges kept")
    ap.add_argument("--edges", default=None, help=".npz with eu, ev (bit 31 of ev = attractive), n_nodes")
    ap.add_argument("--repeat", type=int, default=5, help="plain / pruned pairs")
    ap.add_argument("--classes", action="store_true")
    args = ap.parse_args()
    from patchperpix_amd import backend
    if args.edges:
        z = np.load(args.edges)
        eu, ev, n_nodes = np.ascontiguousarray(z["eu"], np.int32), np.ascontiguousarray(z["ev"], np.int32), int(z["n_nodes"])
        what = os.path.basename(args.edges)
    else:
        eu, ev, n_nodes = grid_edges(args)
        what = "grid %d^3 reach %d" % (args.n, args.reach)
    print("%s: nodes %d edges %d repulsive %.2f, PPP_MWS_PRUNE_BLOCK=%s PPP_MWS_PRUNE_MIN=%s OMP_NUM_THREADS=%s"
          % (what, n_nodes, len(eu), float((ev >= 0).mean()) if len(ev) else 0.0, os.environ.get("PPP_MWS_PRUNE_BLOCK"),
             os.environ.get("PPP_MWS_PRUNE_MIN"), os.environ.get("OMP_NUM_THREADS")))
    want = None
    for i in range(args.repeat):
        for prune in (False, True):
            ms, issued, labels, stats = run(backend, eu, ev, n_nodes, prune)
            if want is None:
                want = (issued, labels)
            same = issued == want[0] and np.array_equal(labels, want[1])
            print("%s %d: %.2f ms (%.1f ns / edge), ids issued %d, labels checksum %d%s%s"
                  % ("pruned" if prune else "plain ", i, ms, ms * 1e6 / max(len(eu), 1), issued,
                     int(labels.astype(np.int64).sum() % (1 << 31)), "" if same else "  DIFFERS FROM THE FIRST RUN",
                     ("  blocks %d dropped by rule 1-4 %s visited %d threads %d prunes %d"
                      % (stats[0], stats[1:5].tolist(), stats[5], stats[6], stats[7])) if prune else ""))
    if args.classes:
        cls = np.zeros(len(eu), dtype=np.uint8)
        labels = np.zeros(n_nodes, dtype=np.int32)
        backend.lib().ppp_host_mws_sorted_classes(backend._np_ptr(eu), backend._np_ptr(ev), len(eu), n_nodes,
                                                  backend._np_ptr(labels), backend._np_ptr(cls))
        # (taking the edges of a class that changes nothing out of the list leaves what every other
        # edge does as it was; without a class that does change something the rest of the loop runs
        # on other clusters -- its line says what the loop costs without them, no more)
        full = best_plain(backend, eu, ev, n_nodes, args.repeat)
        print("plain loop, best of %d: %.2f ms" % (args.repeat, full))
        print("%-40s %10s %7s %12s %10s" % ("class", "edges", "share", "ms without", "ms saved"))
        for c, name in enumerate(CLASSES):
            keep = cls != c
            t = best_plain(backend, eu[keep], ev[keep], n_nodes, args.repeat)
            print("%-40s %10d %6.1f%% %12.2f %10.2f" % (name, int((~keep).sum()), 100.0 * (~keep).mean(), t, full - t))
        noop = np.isin(cls, (3, 4, 5, 6))
        t = best_plain(backend, eu[~noop], ev[~noop], n_nodes, args.repeat)
        print("%-40s %10d %6.1f%% %12.2f %10.2f" % ("all four classes that change nothing", int(noop.sum()),
                                                   100.0 * noop.mean(), t, full - t))


if __name__ == "__main__":
    main()
