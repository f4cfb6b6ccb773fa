// mws_prune_main.cpp -- the watershed's host loop on its own, for the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread tests/csrc/mws_prune_main.cpp -o mws_prune_asan
//   g++ -std=c++17 -O1 -g -fsanitize=thread            -pthread tests/csrc/mws_prune_main.cpp -o mws_prune_tsan
// Random graphs as in tests/test_mws_prune.py (50-2000 nodes, 2-40 edges per node, repulsive share
// 0 / 0.05 / 0.5 / 1, self-loops and repeated pairs included): the blocked loop with blocks of 1,
// 7 and 64 edges and 1, 3 and 16 threads must give the labels and the ids of the plain loop, and
// its stats must add up.  Exit status 0 = all equal.
//   mws_prune_main FILE N_NODES [repeat]: times the plain and the blocked loop alternating on a
//   raw edge list instead (int32 eu [n] then int32 ev [n]).
#include <stdio.h>
#include <string.h>

#include <chrono>
#include <random>
#include <string>

#include "../../patchperpix_amd/csrc/ppp_host_mws.cpp"

static int64_t run(const std::vector<int32_t> &eu, const std::vector<int32_t> &ev, int32_t n_nodes,
                   std::vector<int32_t> &labels, int64_t *stats) {
    labels.assign((size_t)n_nodes, -1);
    return ppp_host_mws_sorted_stats(eu.data(), ev.data(), (int64_t)eu.size(), n_nodes, labels.data(), stats);
}

static int time_file(const char *path, int32_t n_nodes, int repeat) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); return 2; }
    fseek(f, 0, SEEK_END);
    const size_t n = (size_t)ftell(f) / 8;
    fseek(f, 0, SEEK_SET);
    std::vector<int32_t> eu(n), ev(n), labels;
    if (fread(eu.data(), 4, n, f) != n || fread(ev.data(), 4, n, f) != n) { fclose(f); return 2; }
    fclose(f);
    for (int i = 0; i < repeat; ++i)
        for (int prune = 0; prune < 2; ++prune) {
            int64_t st[PPP_MWS_N_STATS];
            if (prune) unsetenv("PPP_MWS_PRUNE"); else setenv("PPP_MWS_PRUNE", "0", 1);
            const auto t0 = std::chrono::steady_clock::now();
            const int64_t issued = run(eu, ev, n_nodes, labels, st);
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            printf("%s %.2f ms ids %lld blocks %lld dropped %lld %lld %lld %lld visited %lld threads %lld\n",
                   prune ? "pruned" : "plain ", ms, (long long)issued, (long long)st[0], (long long)st[1], (long long)st[2],
                   (long long)st[3], (long long)st[4], (long long)st[5], (long long)st[6]);
        }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 3) return time_file(argv[1], atoi(argv[2]), argc > 3 ? atoi(argv[3]) : 5);
    std::mt19937_64 rng(20240521);
    const double rep_share[4] = {0.0, 0.05, 0.5, 1.0};
    const int n_nodes_of[4] = {50, 173, 600, 2000}, per_node_of[4] = {2, 9, 40, 17};
    int bad = 0, cases = 0;
    for (int g = 0; g < 16; ++g) {
        const int32_t N = n_nodes_of[g % 4];
        const int64_t E = (int64_t)N * per_node_of[(g / 4 + g) % 4];
        const double rep = rep_share[g / 4];
        std::vector<int32_t> eu((size_t)E), ev((size_t)E);
        for (int64_t i = 0; i < E; ++i) {
            // near neighbours mostly, so that clusters form; now and then a self-loop
            const int32_t a = (int32_t)(rng() % (uint64_t)N);
            int32_t b = (int32_t)((a + (int64_t)(rng() % 9) - 4 + N) % N);
            if (rng() % 16 == 0) b = (int32_t)(rng() % (uint64_t)N);
            const bool attractive = (double)(rng() % 1000000) / 1e6 >= rep;
            eu[(size_t)i] = a;
            ev[(size_t)i] = attractive ? (int32_t)((uint32_t)b | 0x80000000u) : b;
        }
        std::vector<int32_t> want, got;
        int64_t st[PPP_MWS_N_STATS];
        setenv("PPP_MWS_PRUNE", "0", 1);
        const int64_t want_ids = run(eu, ev, N, want, st);
        unsetenv("PPP_MWS_PRUNE");
        if (st[0] != 0 || st[5] != E) { printf("graph %d: plain stats wrong\n", g); ++bad; }
        setenv("PPP_MWS_PRUNE_MIN", "0", 1);
        for (const char *block : {"1", "7", "64"}) {
            if (block[0] == '1' && block[1] == 0 && E > 4000) continue;      // a prune per edge: short lists only
            for (const char *threads : {"1", "3", "16"}) {
                setenv("PPP_MWS_PRUNE_BLOCK", block, 1);
                setenv("OMP_NUM_THREADS", threads, 1);
                const int64_t ids = run(eu, ev, N, got, st);
                ++cases;
                const int64_t sum = st[1] + st[2] + st[3] + st[4] + st[5];
                if (ids != want_ids || got != want || sum != E || st[0] < 1) {
                    printf("graph %d (N %d E %lld repulsive %.2f) block %s threads %s: DIFFERS (ids %lld / %lld, stats sum %lld)\n",
                           g, N, (long long)E, rep, block, threads, (long long)ids, (long long)want_ids, (long long)sum);
                    ++bad;
                }
            }
        }
        unsetenv("PPP_MWS_PRUNE_BLOCK");
        unsetenv("PPP_MWS_PRUNE_MIN");
        unsetenv("OMP_NUM_THREADS");
    }
    printf("%d cases, %d differ\n", cases, bad);
    return bad ? 1 : 0;
}
