// ppp_host_mws.cpp -- mutex watershed on the patch graph, host side like the reference
// (PatchPerPix/vote_instances/graph_mws.py:7-85 on the graph built by setAffgraph,
// aff_patch_graph.py:31-40).
//
// Same decisions as the reference, without its O(E * |mutex|) scans:
//   * nodes are numbered by first appearance among the rows with aff != 0, edges are visited in
//     networkx's order (node-major in insertion order, neighbours in insertion order, each edge
//     once at its first-visited endpoint; a repeated row overwrites the value of its edge) and
//     stably sorted by |aff| descending (graph_mws.py:23-29);
//   * component membership lives in a union-find whose roots carry the reference's component id;
//     a new component gets max(ids in use) + 1, a merge keeps the smaller id (:37-38, :66-72);
//   * "is there a mutex edge between these components" (:46-48, :59-62) is one lookup in a hash
//     set of (root, root) keys that is rewritten, small-to-large, when components merge;
//   * the output order is the creation order of the ids -- a re-issued id keeps its first
//     position and a component emptied by a merge stays in the list (:79-82) -- so the instance
//     label of a node is 1 + position of its component's id in that order.
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <system_error>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/ppp_mi355x.h"

namespace {

struct Edge {
    int32_t a, b;
    float w;        // |aff|
    int8_t attractive;
};

struct Dsu {
    std::vector<int32_t> parent;
    int32_t find(int32_t x) {
        while (parent[x] != x) {
            parent[x] = parent[parent[x]];
            x = parent[x];
        }
        return x;
    }
};

// Open-addressing set of 64-bit keys (linear probing, tombstones), grown by doubling.
struct KeySet {
    static constexpr uint64_t EMPTY = ~0ull, TOMB = ~0ull - 1;
    std::vector<uint64_t> slot;
    size_t used = 0, live = 0;     // used: non-EMPTY slots (incl. tombstones)
    explicit KeySet(size_t cap = 1024) : slot(cap, EMPTY) {}
    static size_t hash(uint64_t k) {
        k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
        return (size_t)k;
    }
    void grow() {
        std::vector<uint64_t> old;
        old.swap(slot);
        slot.assign(live * 4 + 1024 > old.size() ? old.size() * 2 : old.size(), EMPTY);
        used = live = 0;
        for (uint64_t k : old)
            if (k != EMPTY && k != TOMB) insert(k);
    }
    bool contains(uint64_t k) const {
        const size_t m = slot.size() - 1;
        for (size_t i = hash(k) & m;; i = (i + 1) & m) {
            if (slot[i] == k) return true;
            if (slot[i] == EMPTY) return false;
        }
    }
    // true if the key was not there
    bool insert(uint64_t k) {
        if ((used + 1) * 2 > slot.size()) grow();
        const size_t m = slot.size() - 1;
        size_t tomb = (size_t)-1;
        for (size_t i = hash(k) & m;; i = (i + 1) & m) {
            if (slot[i] == k) return false;
            if (slot[i] == TOMB && tomb == (size_t)-1) tomb = i;
            if (slot[i] == EMPTY) {
                if (tomb != (size_t)-1) { slot[tomb] = k; }
                else { slot[i] = k; ++used; }
                ++live;
                return true;
            }
        }
    }
    void erase(uint64_t k) {
        const size_t m = slot.size() - 1;
        for (size_t i = hash(k) & m;; i = (i + 1) & m) {
            if (slot[i] == k) { slot[i] = TOMB; --live; return; }
            if (slot[i] == EMPTY) return;
        }
    }
};

// Runs f(0) .. f(n - 1) at once, f(0) on the calling thread; the other threads are started once
// per watershed and sleep between the prune passes.  (Letting the first of them start the rest
// while the caller walks its first block measured no different: r16_a_time_mws.txt.)
class Pool {
    int n_ = 1;
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable go_, done_;
    uint64_t gen_ = 0;
    int pending_ = 0;
    bool stop_ = false;
    const std::function<void(int)> *job_ = nullptr;
    void worker(int t) {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> l(m_);
        for (;;) {
            go_.wait(l, [&] { return gen_ != seen; });
            seen = gen_;
            if (stop_) return;
            const std::function<void(int)> *f = job_;
            l.unlock();
            (*f)(t);
            l.lock();
            if (--pending_ == 0) done_.notify_one();
        }
    }

public:
    explicit Pool(int n) {
        th_.reserve((size_t)std::max(n, 1));
        try {
            for (int t = 1; t < n; ++t) {
                th_.emplace_back([this, t] { worker(t); });
                ++n_;
            }
        } catch (const std::system_error &) {}     // no more threads to be had: go on with these
    }
    ~Pool() {
        {
            std::lock_guard<std::mutex> l(m_);
            stop_ = true;
            ++gen_;
        }
        go_.notify_all();
        for (std::thread &t : th_) t.join();
    }
    int size() const { return n_; }
    void run(const std::function<void(int)> &f) {
        {
            std::lock_guard<std::mutex> l(m_);
            job_ = &f;
            pending_ = n_ - 1;
            ++gen_;
        }
        go_.notify_all();
        f(0);
        std::unique_lock<std::mutex> l(m_);
        done_.wait(l, [&] { return pending_ == 0; });
    }
};

// at most 16 threads, fewer where OMP_NUM_THREADS or the machine says fewer
int prune_threads() {
    int n = 16;
    const unsigned hw = std::thread::hardware_concurrency();
    if (hw > 0 && (int)hw < n) n = (int)hw;
    if (const char *s = getenv("OMP_NUM_THREADS")) {
        const long v = strtol(s, nullptr, 10);
        if (v >= 1 && v < n) n = (int)v;
    }
    return n;
}

int64_t env_i64(const char *name, int64_t fallback) {
    const char *s = getenv(name);
    if (!s || !*s) return fallback;
    char *end = nullptr;
    const long long v = strtoll(s, &end, 10);
    return end == s || v < 0 ? fallback : (int64_t)v;
}

// The loop of graph_mws.mws (:31-77) over edges that are already in visiting order.
//   eu / ev [n_edges]: node numbers, bit 31 of ev = attractive; label [n_nodes] out: 1 + position
//   of the node's component id in creation order, 0 = the node ended in no component.
// Every node is a union-find element from the start (an unassigned node is a singleton without
// a component id).  "Is there a mutex edge between two clusters" (:46-48, :59-62) is ONE lookup:
// the set `mutex` holds a key (smaller root, larger root) for every pair of CURRENT clusters with
// a repulsive edge between them.  It is kept exact under merges by rewriting the keys of the
// absorbed cluster -- each root carries the list of the clusters it has a key with (entries may
// name a cluster by any of its former roots; duplicates are harmless), the cluster with the
// shorter list is the one absorbed, so a key is rewritten O(log n) times.  (Round 3 walked the
// shorter of two endpoint lists with a find per entry: 140 entries per check on a graph with half
// of its edges repulsive -- BASELINE config [4] with a random decoder -- 705 ns per edge; this
// form: see tools/time_mws.py.)  A mutex edge inside one cluster can never matter again (clusters
// only grow) and is dropped.
//
// Most edges of a patch graph do nothing: with some 54 edges per node the clusters and the keys
// between them are settled long before the list ends, and the loop still pays two finds and a
// branch for each of them, one after the other.  So long lists are walked in blocks
// (filter-Kruskal): after a block, the edges not yet visited that can never do anything again are
// dropped by several threads at once and the rest is compacted stably -- the survivors keep their
// order, so the loop makes exactly the decisions it would have made on the whole list.  Three
// facts carry every rule: (i) clusters only grow; (ii) a cluster with an id keeps an id for ever
// -- every merge gives the united root one -- so an unassigned cluster is a singleton, and only
// the first branch, which asks for two unassigned nodes, ever merges across a key; (iii) hence two
// clusters with a key between them, one of which has an id, never merge, and the key follows them
// through their own merges.  An unvisited edge (a, b) with roots r0, r1 is dropped iff
//   1. repulsive, r0 == r1: it is skipped now, and by (i) a and b stay together;
//   2. attractive, r0 == r1, the root has an id: no branch fires for c0 == c1 != 0, and by (i),
//      (ii) that is what a and b's cluster will always show;
//   3. repulsive, r0 != r1, key (r0, r1) present: the insert finds its key.  Later the two
//      clusters are either still apart, with the key rewritten to their roots, or -- both were
//      unassigned -- merged by the first branch, and then rule 1 describes the edge;
//   4. attractive, r0 != r1, key (r0, r1) present, r0 or r1 has an id: the second or third branch
//      refuses it.  By (iii) the two never merge; an unassigned side can only pick up an id (then
//      the third branch refuses), and the key stays between whatever the two grow into.
// Kept on purpose: an attractive edge whose cluster has no id -- r0 == r1 is then the self-loop
// a == b on an unseen node, which issues an id -- and an attractive edge between two unassigned
// nodes whatever keys there are, because the first branch (:36-42) does not look at the mutex.
// A prune writes nothing the threads read: one sequential pass points every node at its root,
// after which a find is parent[x], and KeySet::contains does not modify the set.
enum { ST_BLOCKS = 0, ST_RULE1, ST_RULE2, ST_RULE3, ST_RULE4, ST_VISITED, ST_THREADS, ST_PRUNES, ST_N };
static_assert(ST_N == PPP_MWS_N_STATS, "stats layout");
// classes of ppp_host_mws_sorted_classes (what the visit of an edge did)
enum { CL_A_NEW = 0, CL_A_JOIN, CL_A_MERGE, CL_A_SAME, CL_A_REFUSED, CL_R_SAME, CL_R_KNOWN, CL_R_INSERT };

// Measured on the flagship's list (1 292 850 edges, 23 946 nodes; profiles/r16_a_time_mws.txt):
// first block = 1 / PRUNE_FIRST_SHARE of the list, every later block PRUNE_GROWTH times the one
// before.  A prune costs about as much per edge as a visit (two parents and a key lookup) and gains
// by its threads alone, so it must come late enough to drop most of what it looks at: after 1/32 of
// the list it dropped 1 % of the rest, after 1/8 90 %.
constexpr int64_t PRUNE_FIRST_SHARE = 8, PRUNE_GROWTH = 4;
constexpr int64_t PRUNE_MIN_EDGES = 200000;     // shorter lists: the plain loop, no thread started

struct Mws {
    int32_t N;
    Dsu dsu;
    std::vector<int32_t> cc_of_root;               // component id carried by a root (0: none)
    std::vector<std::vector<int32_t>> nbrs;        // clusters this root has a mutex key with
    std::vector<int32_t> n_nbrs;                   // list lengths, next to each other (the vector
                                                   // headers are 24 bytes apiece)
    KeySet mutex;
    // ids currently held by some node: only "the largest one" is ever asked (:37-38), so a flag
    // per id and a maximum that is walked down lazily when its id dies (amortised O(1), no tree)
    std::vector<uint8_t> alive;
    int32_t max_alive = 0;
    std::vector<int32_t> created;                  // ids in creation order (first issue)
    std::vector<uint8_t> ever;                     // id was issued before (ids are <= N)

    explicit Mws(int32_t n)
        : N(n), cc_of_root((size_t)n, 0), nbrs((size_t)n), n_nbrs((size_t)n, 0), mutex(1 << 16),
          alive((size_t)n + 2, 0), ever((size_t)n + 2, 0) {
        dsu.parent.resize((size_t)n);
        for (int32_t i = 0; i < n; ++i) dsu.parent[i] = i;
    }
    static uint64_t key(int32_t a, int32_t b) {
        const uint32_t lo = (uint32_t)std::min(a, b), hi = (uint32_t)std::max(a, b);
        return ((uint64_t)lo << 32) | hi;
    }
    bool has_mutex(int32_t r0, int32_t r1) const { return mutex.contains(key(r0, r1)); }
    // the two clusters become one; returns its root (the one with the longer list)
    int32_t unite(int32_t ra, int32_t rb) {
        int32_t keep = ra, drop = rb;
        if (n_nbrs[keep] < n_nbrs[drop]) std::swap(keep, drop);
        if (n_nbrs[drop]) {
            std::vector<int32_t> &kl = nbrs[keep], &dl = nbrs[drop];
            // (find() of the neighbours BEFORE the link: keep and drop are still both roots)
            for (int32_t x : dl) {
                const int32_t p = dsu.find(x);
                if (p == keep || p == drop) continue;          // becomes internal
                mutex.erase(key(drop, p));
                if (mutex.insert(key(keep, p))) kl.push_back(p);
            }
            mutex.erase(key(keep, drop));
            std::vector<int32_t>().swap(dl);
            n_nbrs[keep] = (int32_t)kl.size();
            n_nbrs[drop] = 0;
        }
        dsu.parent[drop] = keep;
        return keep;
    }

    // TRACE: also note what each edge did (cls [n_edges], CL_*)
    template <bool TRACE>
    void visit(const int32_t *eu, const int32_t *ev, int64_t n_edges, uint8_t *cls) {
        constexpr int64_t AHEAD = 24;      // the edge list is known: fetch the nodes' entries early
        for (int64_t i = 0; i < n_edges; ++i) {
            if (i + AHEAD < n_edges) {
                const int32_t pa = eu[i + AHEAD], pb = ev[i + AHEAD] & 0x7FFFFFFF;
                __builtin_prefetch(&dsu.parent[pa]);
                __builtin_prefetch(&dsu.parent[pb]);
            }
            const int32_t a = eu[i], b = ev[i] & 0x7FFFFFFF;
            const int32_t r0 = dsu.find(a), r1 = dsu.find(b);
            if (ev[i] < 0) {                                  // attractive
                const int32_t c0 = cc_of_root[r0], c1 = cc_of_root[r1];
                if (TRACE) cls[i] = CL_A_SAME;
                if (c0 == 0 && c1 == 0) {
                    // both unassigned (:36-42): a new component, id = max id in use + 1
                    while (max_alive > 0 && !alive[(size_t)max_alive]) --max_alive;
                    const int32_t id = max_alive + 1;
                    const int32_t r = r0 != r1 ? unite(r0, r1) : r0;
                    cc_of_root[r] = id;
                    alive[(size_t)id] = 1;
                    max_alive = id;
                    if (!ever[(size_t)id]) { ever[(size_t)id] = 1; created.push_back(id); }
                    if (TRACE) cls[i] = CL_A_NEW;
                } else if (c0 == 0 || c1 == 0) {
                    // the unassigned node joins unless a mutex edge links it to the component (:44-56)
                    if (TRACE) cls[i] = CL_A_REFUSED;
                    if (!has_mutex(r0, r1)) {
                        const int32_t id = c0 == 0 ? c1 : c0;
                        cc_of_root[unite(r0, r1)] = id;
                        if (TRACE) cls[i] = CL_A_JOIN;
                    }
                } else if (c0 != c1) {
                    // two components merge into the smaller id unless a mutex edge links them (:57-71)
                    if (TRACE) cls[i] = CL_A_REFUSED;
                    if (!has_mutex(r0, r1)) {
                        const int32_t keep = std::min(c0, c1), drop = std::max(c0, c1);
                        cc_of_root[unite(r0, r1)] = keep;
                        alive[(size_t)drop] = 0;
                        if (TRACE) cls[i] = CL_A_MERGE;
                    }
                }
            } else if (r0 != r1) {                            // repulsive (:76-77)
                if (TRACE) cls[i] = CL_R_KNOWN;
                if (mutex.insert(key(r0, r1))) {
                    nbrs[r0].push_back(r1);
                    nbrs[r1].push_back(r0);
                    ++n_nbrs[r0];
                    ++n_nbrs[r1];
                    if (TRACE) cls[i] = CL_R_INSERT;
                }
            } else if (TRACE) {
                cls[i] = CL_R_SAME;
            }
        }
    }

    // the rule (1-4) by which an unvisited edge is dropped, 0 = it stays.  Read-only; every
    // node points at its root (compress()).
    int settled(int32_t a, int32_t evb) const {
        const int32_t r0 = dsu.parent[a], r1 = dsu.parent[evb & 0x7FFFFFFF];
        if (evb < 0) {
            if (r0 == r1) return cc_of_root[r0] != 0 ? 2 : 0;
            return (cc_of_root[r0] != 0 || cc_of_root[r1] != 0) && has_mutex(r0, r1) ? 4 : 0;
        }
        if (r0 == r1) return 1;
        return has_mutex(r0, r1) ? 3 : 0;
    }
    void compress() {
        for (int32_t x = 0; x < N; ++x) dsu.parent[x] = dsu.find(x);
    }

    void labels(int32_t *label, int64_t *issued) {
        std::vector<int32_t> label_of_id((size_t)N + 2, 0);
        for (size_t i = 0; i < created.size(); ++i) label_of_id[(size_t)created[i]] = (int32_t)i + 1;
        for (int32_t n = 0; n < N; ++n) label[n] = label_of_id[(size_t)cc_of_root[dsu.find(n)]];
        *issued = (int64_t)created.size();
    }
};

// what one thread keeps of its slice of a prune pass
struct alignas(64) Slice {
    int64_t dropped[5] = {0, 0, 0, 0, 0};        // by rule; [0]: kept
    int64_t kept = 0, at = 0;                    // this pass: survivors, and where they go
};

// stats [PPP_MWS_N_STATS] or null
void watershed(const int32_t *eu, const int32_t *ev, int64_t n_edges, int32_t N, int32_t *label,
               int64_t *issued, int64_t *stats) {
    int64_t st[ST_N] = {0};
    Mws w(N);
    const int64_t min_len = env_i64("PPP_MWS_PRUNE_MIN", PRUNE_MIN_EDGES);
    const int64_t fixed_block = env_i64("PPP_MWS_PRUNE_BLOCK", 0);
    if (env_i64("PPP_MWS_PRUNE", 1) == 0 || n_edges < min_len || n_edges == 0) {
        w.visit<false>(eu, ev, n_edges, nullptr);
        st[ST_VISITED] = n_edges;
    } else {
        Pool pool(prune_threads());
        const int T = pool.size();
        st[ST_THREADS] = T;
        std::vector<Slice> part((size_t)T);
        std::unique_ptr<int32_t[]> su, sv;             // the survivors of the latest prune
        std::unique_ptr<uint8_t[]> rule;               // per unvisited edge: the rule that drops it, 0 = none
        const int32_t *cu = eu, *cv = ev;              // the edges not yet visited
        int64_t left = n_edges;
        int64_t block = fixed_block > 0 ? fixed_block : std::max<int64_t>(n_edges / PRUNE_FIRST_SHARE, 1);
        for (;;) {
            const int64_t b = std::min(block, left);
            w.visit<false>(cu, cv, b, nullptr);
            ++st[ST_BLOCKS];
            st[ST_VISITED] += b;
            cu += b; cv += b; left -= b;
            if (left == 0) break;
            w.compress();
            if (!rule) rule.reset(new uint8_t[(size_t)left]);
            const int64_t per = (left + T - 1) / T;
            pool.run([&](int t) {
                Slice &s = part[(size_t)t];
                s.kept = 0;
                const int64_t lo = std::min(left, per * t), hi = std::min(left, lo + per);
                for (int64_t i = lo; i < hi; ++i) {
                    const int r = w.settled(cu[i], cv[i]);
                    rule[(size_t)i] = (uint8_t)r;
                    ++s.dropped[r];
                    s.kept += r == 0;
                }
            });
            int64_t kept = 0;
            for (Slice &s : part) { s.at = kept; kept += s.kept; }
            // (not std::vector: it would write zeros over what is overwritten at once)
            std::unique_ptr<int32_t[]> nu(new int32_t[(size_t)kept]), nv(new int32_t[(size_t)kept]);
            pool.run([&](int t) {
                int64_t at = part[(size_t)t].at;
                const int64_t lo = std::min(left, per * t), hi = std::min(left, lo + per);
                for (int64_t i = lo; i < hi; ++i)
                    if (rule[(size_t)i] == 0) { nu[(size_t)at] = cu[i]; nv[(size_t)at] = cv[i]; ++at; }
            });
            su.swap(nu); sv.swap(nv);
            cu = su.get(); cv = sv.get(); left = kept;
            ++st[ST_PRUNES];
            if (left == 0) break;
            if (fixed_block <= 0) block *= PRUNE_GROWTH;
        }
        for (const Slice &s : part)
            for (int r = 1; r <= 4; ++r) st[ST_RULE1 + r - 1] += s.dropped[r];
    }
    w.labels(label, issued);
    if (stats) std::copy(st, st + ST_N, stats);
}

}  // namespace

extern "C" {

// ppp_host_mws_sorted: the watershed over an edge list that is already in visiting order (made
// on the device by ppp_mws_edges).  labels int32 [n_nodes] out; returns the number of ids issued.
int64_t ppp_host_mws_sorted(const int32_t *eu, const int32_t *ev, int64_t n_edges, int64_t n_nodes,
                            int32_t *labels) {
    return ppp_host_mws_sorted_stats(eu, ev, n_edges, n_nodes, labels, nullptr);
}

// The same, and stats int64 [PPP_MWS_N_STATS] (may be null): blocks run (0: the plain loop), edges
// dropped by rules 1-4, edges visited, threads, prune passes.  dropped + visited = n_edges.
int64_t ppp_host_mws_sorted_stats(const int32_t *eu, const int32_t *ev, int64_t n_edges, int64_t n_nodes,
                                  int32_t *labels, int64_t *stats) {
    int64_t issued = 0;
    if (stats) std::fill(stats, stats + PPP_MWS_N_STATS, 0);
    if (n_nodes <= 0) return 0;
    watershed(eu, ev, n_edges, (int32_t)n_nodes, labels, &issued, stats);
    return issued;
}

// The plain loop, noting what every edge did: cls uint8 [n_edges], 0-4 attractive (new component,
// joined, merged, same cluster, refused by a mutex key), 5-7 repulsive (same cluster, key already
// there, key inserted).  For tools/time_mws.py --classes.
int64_t ppp_host_mws_sorted_classes(const int32_t *eu, const int32_t *ev, int64_t n_edges, int64_t n_nodes,
                                    int32_t *labels, uint8_t *cls) {
    int64_t issued = 0;
    if (n_nodes <= 0) return 0;
    Mws w((int32_t)n_nodes);
    w.visit<true>(eu, ev, n_edges, cls);
    w.labels(labels, &issued);
    return issued;
}

// pairs u32 [n_rows][6] (A zyx, B zyx), aff f32 [n_rows], vol = volume shape (for node keys).
// out_nodes int32 [cap][3] / out_labels int32 [cap]: every node of the graph (first-appearance
// order) with its label, 0 for nodes the watershed left unassigned.  *n_labels = number of
// labels issued (including emptied components).  Returns the number of nodes, -1 if cap is
// too small, -2 for a coordinate outside vol.
int64_t ppp_host_mws(const uint32_t *pairs, const float *aff, int64_t n_rows, const int32_t *vol,
                     int32_t *out_nodes, int32_t *out_labels, int64_t cap, int64_t *n_labels) {
    const int64_t Y = vol[1], X = vol[2];
    auto lin = [&](const uint32_t *c) { return ((int64_t)c[0] * Y + c[1]) * X + c[2]; };

    // ---- nodes and (deduplicated) edges in insertion order --------------------------------
    // voxel -> node id: a direct table for volumes up to 2^28 voxels, a hash map beyond
    const int64_t V = (int64_t)vol[0] * Y * X;
    const bool direct = V <= (1ll << 28);
    std::vector<int32_t> table(direct ? (size_t)V : 0, -1);
    std::unordered_map<int64_t, int32_t> node_id;
    std::vector<int64_t> node_key;
    struct Row { int32_t u, v; float a; };
    std::vector<Row> rows;
    rows.reserve((size_t)n_rows);
    for (int64_t i = 0; i < n_rows; ++i) {
        if (aff[i] == 0.0f) continue;          // setAffgraph skips exact zeros (NaN is kept)
        int32_t id[2];
        for (int s = 0; s < 2; ++s) {
            const int64_t k = lin(pairs + i * 6 + 3 * s);
            if (direct) {
                if (k < 0 || k >= V) return -2;
                if (table[k] < 0) {
                    table[k] = (int32_t)node_key.size();
                    node_key.push_back(k);
                }
                id[s] = table[k];
            } else {
                auto it = node_id.find(k);
                if (it == node_id.end()) {
                    it = node_id.emplace(k, (int32_t)node_key.size()).first;
                    node_key.push_back(k);
                }
                id[s] = it->second;
            }
        }
        rows.push_back({id[0], id[1], aff[i]});
    }
    std::vector<int32_t>().swap(table);
    const int32_t N = (int32_t)node_key.size();
    if (N > cap) return -1;
    // a repeated (unordered) node pair keeps its first position and takes the last value
    {
        std::vector<uint64_t> key(rows.size());
        for (size_t i = 0; i < rows.size(); ++i) {
            const uint32_t lo = (uint32_t)std::min(rows[i].u, rows[i].v), hi = (uint32_t)std::max(rows[i].u, rows[i].v);
            key[i] = ((uint64_t)lo << 32) | hi;
        }
        std::vector<uint64_t> sorted(key);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) {
            std::unordered_map<uint64_t, size_t> first;
            std::vector<Row> uniq;
            for (size_t i = 0; i < rows.size(); ++i) {
                auto it = first.find(key[i]);
                if (it == first.end()) {
                    first.emplace(key[i], uniq.size());
                    uniq.push_back(rows[i]);
                } else {
                    uniq[it->second].a = rows[i].a;
                }
            }
            rows.swap(uniq);
        }
    }
    // adjacency in insertion order (CSR), then networkx's edge order
    std::vector<int64_t> start((size_t)N + 1, 0);
    for (const Row &r : rows) {
        ++start[r.u + 1];
        if (r.u != r.v) ++start[r.v + 1];
    }
    for (int32_t n = 0; n < N; ++n) start[n + 1] += start[n];
    std::vector<int32_t> nbr((size_t)start[N]);
    std::vector<float> nbr_a((size_t)start[N]);
    {
        std::vector<int64_t> fill(start.begin(), start.end() - 1);
        for (const Row &r : rows) {
            nbr[fill[r.u]] = r.v; nbr_a[fill[r.u]++] = r.a;
            if (r.u != r.v) { nbr[fill[r.v]] = r.u; nbr_a[fill[r.v]++] = r.a; }
        }
    }
    std::vector<Edge> edges;
    edges.reserve(rows.size());
    for (int32_t n = 0; n < N; ++n)
        for (int64_t j = start[n]; j < start[n + 1]; ++j)
            if (nbr[j] >= n) {
                const float a = nbr_a[j];
                // graph_mws.py:17-21: a > 0 attractive, everything else (incl. NaN) repulsive
                edges.push_back(a > 0 ? Edge{n, nbr[j], a, 1} : Edge{n, nbr[j], -a, -1});
            }
    std::vector<int32_t>().swap(nbr);
    std::vector<float>().swap(nbr_a);
    std::vector<Row>().swap(rows);
    std::stable_sort(edges.begin(), edges.end(), [](const Edge &x, const Edge &y) { return x.w > y.w; });

    // ---- the watershed ---------------------------------------------------------------------
    std::vector<int32_t> eu(edges.size()), ev(edges.size());
    for (size_t i = 0; i < edges.size(); ++i) {
        eu[i] = edges[i].a;
        ev[i] = edges[i].b | (edges[i].attractive == 1 ? (int32_t)0x80000000 : 0);
    }
    std::vector<Edge>().swap(edges);
    std::vector<int32_t> label((size_t)N);
    int64_t issued = 0;
    watershed(eu.data(), ev.data(), (int64_t)eu.size(), N, label.data(), &issued, nullptr);

    // ---- labels ------------------------------------------------------------------------------
    for (int32_t n = 0; n < N; ++n) {
        const int64_t k = node_key[n];
        out_nodes[3 * (int64_t)n + 0] = (int32_t)(k / (Y * X));
        out_nodes[3 * (int64_t)n + 1] = (int32_t)((k / X) % Y);
        out_nodes[3 * (int64_t)n + 2] = (int32_t)(k % X);
        out_labels[n] = label[(size_t)n];
    }
    if (n_labels) *n_labels = issued;
    return N;
}

}  // extern "C"
