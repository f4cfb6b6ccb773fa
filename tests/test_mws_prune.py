"""The blocked watershed loop with its parallel prune (csrc/ppp_host_mws.cpp) makes the decisions of
the plain loop: same label for every node, same number of ids, whatever the block size and the
number of threads, and no edge is lost on the way (dropped + visited = edges).  Host code only."""
import numpy as np
import pytest

A = np.int32(-2 ** 31)          # bit 31 of ev: attractive
ENV = ("PPP_MWS_PRUNE", "PPP_MWS_PRUNE_BLOCK", "PPP_MWS_PRUNE_MIN", "OMP_NUM_THREADS")
BLOCKS, R1, R2, R3, R4, VISITED, THREADS, PRUNES = range(8)


def run(monkeypatch, eu, ev, n_nodes, **env):
    """ppp_host_mws_sorted_stats under the given switches: (labels, ids issued, stats)"""
    from patchperpix_amd import backend
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    eu = np.ascontiguousarray(eu, dtype=np.int32)
    ev = np.ascontiguousarray(ev, dtype=np.int32)
    labels = np.full((n_nodes,), -1, dtype=np.int32)
    stats = np.full((8,), -1, dtype=np.int64)
    issued = int(backend.lib().ppp_host_mws_sorted_stats(backend._np_ptr(eu), backend._np_ptr(ev), len(eu), n_nodes,
                                                         backend._np_ptr(labels), backend._np_ptr(stats)))
    assert stats[R1:VISITED + 1].sum() == len(eu), "an edge was lost or counted twice"
    return labels, issued, stats


def plain(monkeypatch, eu, ev, n_nodes):
    labels, issued, stats = run(monkeypatch, eu, ev, n_nodes, PPP_MWS_PRUNE=0)
    assert stats[BLOCKS] == 0 and stats[VISITED] == len(eu) and stats[PRUNES] == 0
    return labels, issued


def random_graph(seed, n_nodes, per_node, repulsive, unique):
    """edges in visiting order: mostly between near node numbers (so that clusters form and
    collide), some anywhere, some self-loops; unique: no unordered pair twice"""
    rng = np.random.default_rng(seed)
    n = n_nodes * per_node
    a = rng.integers(0, n_nodes, size=n)
    b = (a + rng.integers(-4, 5, size=n)) % n_nodes
    far = rng.random(n) < 1 / 16
    b[far] = rng.integers(0, n_nodes, size=int(far.sum()))
    if unique:
        _, first = np.unique(np.minimum(a, b) * n_nodes + np.maximum(a, b), return_index=True)
        first.sort()
        a, b = a[first], b[first]
    attractive = rng.random(len(a)) >= repulsive
    # |aff| in a few levels, descending: many equal weights
    w = np.sort(rng.integers(1, 9, size=len(a)))[::-1] / 8.0
    return a.astype(np.int32), np.where(attractive, b | A, b).astype(np.int32), w


def python_mws(eu, ev, w, n_nodes):
    """the project's restatement of graph_mws.mws on the same list: (labels, ids issued)"""
    from patchperpix_amd.vote_instances.graph_mws import _mws_core
    edges = [(int(u), int(v & 0x7FFFFFFF), float(x) if v < 0 else -float(x)) for u, v, x in zip(eu, ev, w)]
    ccs = _mws_core(list(range(n_nodes)), edges)
    labels = np.zeros((n_nodes,), dtype=np.int32)
    for k, cc in enumerate(ccs):
        labels[cc] = k + 1
    return labels, len(ccs)


GRAPHS = [(50, 2), (50, 40), (173, 9), (600, 40), (2000, 17), (2000, 2)]


@pytest.mark.parametrize("repulsive", [0, 0.05, 0.5, 1])
@pytest.mark.parametrize("n_nodes,per_node", GRAPHS)
def test_random_graphs_equal_plain_loop(monkeypatch, n_nodes, per_node, repulsive):
    eu, ev, _w = random_graph(n_nodes * 41 + per_node, n_nodes, per_node, repulsive, unique=False)
    want, want_ids = plain(monkeypatch, eu, ev, n_nodes)
    for block in (1, 7, 64):
        if block == 1 and len(eu) > 4000:
            continue        # a prune pass per edge: quadratic, kept to the short lists
        got, ids, stats = run(monkeypatch, eu, ev, n_nodes, PPP_MWS_PRUNE_BLOCK=block, PPP_MWS_PRUNE_MIN=0,
                              OMP_NUM_THREADS=3)
        assert ids == want_ids and np.array_equal(got, want), "block %d" % block
        assert stats[BLOCKS] >= 1 and stats[PRUNES] >= min(1, len(eu) // (block + 1))
    if repulsive in (0.05, 0.5):
        assert stats[R1:R4 + 1].sum() > 0, "the prune never dropped an edge: the case checks nothing"


@pytest.mark.parametrize("repulsive", [0, 0.05, 0.5, 1])
@pytest.mark.parametrize("n_nodes,per_node", [(50, 2), (50, 40), (173, 9), (300, 6)])
def test_random_graphs_equal_python_restatement(monkeypatch, n_nodes, per_node, repulsive):
    """(unique node pairs, as the patch graph has them: the restatement keeps the reference's
    treatment of an attractive edge whose very pair is already a mutex edge)"""
    eu, ev, w = random_graph(n_nodes * 43 + per_node, n_nodes, per_node, repulsive, unique=True)
    want, want_ids = python_mws(eu, ev, w, n_nodes)
    got, ids = plain(monkeypatch, eu, ev, n_nodes)
    assert ids == want_ids and np.array_equal(got, want)
    for block in (1, 7, 64):
        got, ids, _ = run(monkeypatch, eu, ev, n_nodes, PPP_MWS_PRUNE_BLOCK=block, PPP_MWS_PRUNE_MIN=0,
                          OMP_NUM_THREADS=3)
        assert ids == want_ids and np.array_equal(got, want), "block %d" % block


def att(a, b):
    return (a, int(b) | int(A))


def rep(a, b):
    return (a, b)


# name: (edges, nodes, block, labels, ids, edges dropped by rules 1-4)
HAND = {
    # rule 2 must not take the self-loop on a node never seen: it issues an id
    "self_loop_on_unseen_node": ([att(1, 2), att(0, 0)], 3, 1, [2, 1, 1], 2, [0, 0, 0, 0]),
    # rule 4 must not take it: the first branch does not look at the mutex
    "repulsive_then_attractive_both_unassigned": ([rep(0, 1), att(0, 1)], 2, 1, [1, 1], 1, [0, 0, 0, 0]),
    "repulsive_inside_a_cluster": ([att(0, 1), rep(0, 1)], 2, 1, [1, 1], 1, [1, 0, 0, 0]),
    "attractive_inside_a_cluster": ([att(0, 1), att(1, 2), att(0, 2)], 3, 2, [1, 1, 1], 1, [0, 1, 0, 0]),
    "repeated_repulsive_between_clusters": ([att(0, 1), att(2, 3), rep(0, 2), rep(1, 3), rep(0, 2)], 4, 3,
                                            [1, 1, 2, 2], 2, [0, 0, 2, 0]),
    "attractive_across_key_one_side_unassigned": ([att(0, 1), rep(0, 2), att(1, 2)], 3, 2, [1, 1, 0], 1, [0, 0, 0, 1]),
    "attractive_across_key_both_assigned": ([att(0, 1), att(2, 3), rep(0, 2), att(1, 3)], 4, 3, [1, 1, 2, 2], 2,
                                            [0, 0, 0, 1]),
    # dropped while node 2 has no id; it picks one up later, through the first branch: still refused
    "unassigned_side_assigned_later": ([att(0, 1), rep(0, 2), att(2, 3), att(1, 2)], 4, 2, [1, 1, 2, 2], 2, [0, 0, 0, 1]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_cases(monkeypatch, name):
    edges, n_nodes, block, labels, ids, dropped = HAND[name]
    eu, ev = [e[0] for e in edges], [e[1] for e in edges]
    got, got_ids = plain(monkeypatch, eu, ev, n_nodes)
    assert got.tolist() == labels and got_ids == ids
    got, got_ids, stats = run(monkeypatch, eu, ev, n_nodes, PPP_MWS_PRUNE_BLOCK=block, PPP_MWS_PRUNE_MIN=0)
    assert got.tolist() == labels and got_ids == ids
    assert stats[R1:R4 + 1].tolist() == dropped
    assert stats[PRUNES] >= 1
    # a prune after every edge as well
    got, got_ids, _ = run(monkeypatch, eu, ev, n_nodes, PPP_MWS_PRUNE_BLOCK=1, PPP_MWS_PRUNE_MIN=0)
    assert got.tolist() == labels and got_ids == ids


def test_empty_list_one_edge_and_one_past_a_block(monkeypatch):
    none = np.zeros((0,), np.int32)
    got, ids, stats = run(monkeypatch, none, none, 3, PPP_MWS_PRUNE_BLOCK=1, PPP_MWS_PRUNE_MIN=0)
    assert got.tolist() == [0, 0, 0] and ids == 0 and stats[BLOCKS] == 0 and stats[VISITED] == 0
    got, ids, stats = run(monkeypatch, [0], [att(0, 1)[1]], 2, PPP_MWS_PRUNE_BLOCK=1, PPP_MWS_PRUNE_MIN=0)
    assert got.tolist() == [1, 1] and ids == 1 and stats[BLOCKS] == 1 and stats[VISITED] == 1 and stats[PRUNES] == 0
    # five edges, blocks of four: one prune, which has nothing to drop, and a block of one
    edges = [att(0, 1), att(2, 3), att(4, 5), att(6, 7), att(8, 9)]
    got, ids, stats = run(monkeypatch, [e[0] for e in edges], [e[1] for e in edges], 10, PPP_MWS_PRUNE_BLOCK=4,
                          PPP_MWS_PRUNE_MIN=0)
    assert got.tolist() == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5] and ids == 5
    assert stats[BLOCKS] == 2 and stats[PRUNES] == 1 and stats[VISITED] == 5


def test_thread_counts_and_minimum_length(monkeypatch):
    n_nodes = 600
    eu, ev, _w = random_graph(7, n_nodes, 20, 0.3, unique=False)
    want, want_ids = plain(monkeypatch, eu, ev, n_nodes)
    seen = []
    for threads in (1, 3, 16):
        got, ids, stats = run(monkeypatch, eu, ev, n_nodes, PPP_MWS_PRUNE_BLOCK=64, PPP_MWS_PRUNE_MIN=0,
                              OMP_NUM_THREADS=threads)
        assert ids == want_ids and np.array_equal(got, want), "%d threads" % threads
        assert 1 <= stats[THREADS] <= threads
        seen.append(stats[BLOCKS:VISITED + 1].tolist())
    assert seen[0] == seen[1] == seen[2] and seen[0][0] > 1 and sum(seen[0][1:5]) > 0
    # a list below the minimum length: the plain loop -- by the switch, and by the default
    for env in (dict(PPP_MWS_PRUNE_MIN=len(eu) + 1), dict()):
        got, ids, stats = run(monkeypatch, eu, ev, n_nodes, **env)
        assert ids == want_ids and np.array_equal(got, want)
        assert stats[BLOCKS] == 0 and stats[THREADS] == 0 and stats[VISITED] == len(eu)
    # the default schedule (first block a share of the list, later blocks growing) on the same list
    got, ids, stats = run(monkeypatch, eu, ev, n_nodes, PPP_MWS_PRUNE_MIN=0)
    assert ids == want_ids and np.array_equal(got, want) and stats[BLOCKS] >= 2


def test_all_host_path_goes_through_the_prune(monkeypatch):
    """ppp_host_mws (pair lists from outside) shares watershed(): same nodes and labels with and
    without the prune"""
    from patchperpix_amd import backend
    rng = np.random.default_rng(3)
    shape = (8, 9, 10)
    n = 3000
    pa = rng.integers(0, [8, 9, 10], size=(n, 3))
    pb = np.clip(pa + rng.integers(-2, 3, size=(n, 3)), 0, np.array(shape) - 1)
    pairs = np.concatenate([pa, pb], axis=1).astype(np.uint32)
    aff = (rng.integers(-6, 7, size=n) / 8.0).astype(np.float32)
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PPP_MWS_PRUNE", "0")
    want = backend.host_mws(pairs, aff, shape)
    monkeypatch.delenv("PPP_MWS_PRUNE")
    monkeypatch.setenv("PPP_MWS_PRUNE_MIN", "0")
    monkeypatch.setenv("PPP_MWS_PRUNE_BLOCK", "7")
    got = backend.host_mws(pairs, aff, shape)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert len(want[0]) > 0
