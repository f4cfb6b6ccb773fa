// pack_host_check.cpp -- the channel walk of no_overlap_per_channel under a sanitizer, as a program of
// its own (nothing is loaded into Python).  Build and run on the CPU:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/pack_host_check.cpp patchperpix_amd/csrc/ppp_host_pack.cpp -o /tmp/pack_host_check && /tmp/pack_host_check
//
// It runs ppp_host_pack_channels on cases with a known answer (a clique of large components, small
// ones, empty ones, repeated and unordered pairs, no component at all, pairs it must refuse) and on a
// larger pseudo-random graph checked against a plain O(K^2) restatement; exit status 0 = all as expected.
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

extern "C" int64_t ppp_host_pack_channels(int64_t n_labels, const int64_t *sizes, const uint64_t *pairs, int64_t n_pairs,
                                          int64_t min_voxels, int32_t *chan_out, int32_t *n_channels_out);

static uint64_t key(uint64_t a, uint64_t b) { return (b << 32) | a; }

static bool run(const char *name, const std::vector<int64_t> &sizes, const std::vector<uint64_t> &pairs, int64_t min_voxels,
                const std::vector<int32_t> &want, int32_t want_channels) {
    std::vector<int32_t> chan(sizes.size(), -7);
    int32_t n_ch = -7;
    const int64_t rc = ppp_host_pack_channels((int64_t)sizes.size(), sizes.data(), pairs.data(), (int64_t)pairs.size(), min_voxels,
                                              chan.data(), &n_ch);
    const bool ok = rc == want_channels && n_ch == want_channels && chan == want;
    std::printf("%-28s %s (%d channels)\n", name, ok ? "ok" : "WRONG", (int)n_ch);
    return ok;
}

int main() {
    int rc = 0;
    // four large components, every two overlap: a channel each
    std::vector<uint64_t> clique;
    for (uint64_t b = 2; b <= 4; ++b)
        for (uint64_t a = 1; a < b; ++a) clique.push_back(key(a, b));
    rc |= !run("clique of large", {9, 9, 9, 9}, clique, 2, {0, 1, 2, 3}, 4);
    rc |= !run("clique of small", {9, 9, 9, 9}, clique, 9, {0, 0, 0, 0}, 1);
    // 1 large, 2 small over it, 3 large overlapping only the small 2 (channel 0 is taken all the same), 4 empty
    rc |= !run("small one blocks channel 0", {50, 3, 40, 0}, {key(1, 2), key(2, 3)}, 5, {0, 0, 1, 0}, 2);
    // repeated pairs in any order; 4 overlaps 1 (channel 0) and 2 (channel 1) and opens a third
    rc |= !run("repeats, unordered", {50, 40, 30, 20}, {key(2, 4), key(1, 2), key(1, 4), key(1, 2), key(2, 4)}, 5, {0, 1, 0, 2}, 3);
    rc |= !run("no component", {}, {}, 2000, {}, 0);
    rc |= !run("one empty component", {0}, {}, 2000, {0}, 1);
    {   // refused: a == b, a > b, b > K, label 0
        const std::vector<int64_t> sizes = {5, 5, 5};
        for (uint64_t bad : {key(2, 2), key(3, 2), key(1, 4), key(0, 2)}) {
            int32_t chan[3], n_ch = 0;
            if (ppp_host_pack_channels(3, sizes.data(), &bad, 1, 0, chan, &n_ch) != -1) { std::printf("bad pair accepted\n"); rc = 1; }
        }
        if (ppp_host_pack_channels(3, sizes.data(), nullptr, 0, 0, nullptr, nullptr) != -1) { std::printf("NULL accepted\n"); rc = 1; }
    }
    {   // a larger graph against the plain restatement
        const int K = 700;
        uint64_t s = 12345;
        auto next = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); };
        std::vector<int64_t> sizes(K);
        std::vector<std::vector<char>> adj(K, std::vector<char>(K, 0));
        std::vector<uint64_t> pairs;
        for (int k = 0; k < K; ++k) sizes[k] = next() % 4000;
        for (int b = 1; b < K; ++b)
            for (int a = 0; a < b; ++a)
                if (next() % 100 < 3) { adj[a][b] = 1; pairs.push_back(key(a + 1, b + 1)); if (next() % 4 == 0) pairs.push_back(key(a + 1, b + 1)); }
        for (size_t i = pairs.size(); i > 1; --i) std::swap(pairs[i - 1], pairs[next() % i]);
        std::vector<int32_t> want(K, 0);
        int32_t n_want = 1;
        for (int k = 1; k < K; ++k) {
            if (sizes[k] <= 2000) continue;
            int c = 0;
            for (; c < n_want; ++c) {
                bool taken = false;
                for (int j = 0; j < k && !taken; ++j) taken = adj[j][k] && want[j] == c;
                if (!taken) break;
            }
            if (c == n_want) ++n_want;
            want[k] = c;
        }
        rc |= !run("random graph, 700 labels", sizes, pairs, 2000, want, n_want);
    }
    return rc;
}
