// ppp_host_pack.cpp -- the greedy channel walk of `no_overlap_per_channel`
// (graph_to_labeling.py:86-106) on sizes and overlap pairs instead of painted volumes; the closed
// form it rests on is stated at the head of ppp_pack_channels.hip.
//
// Component k (label k + 1) goes to channel 0 when it is the first or has at most min_voxels voxels;
// otherwise to the first channel none of whose earlier components overlaps it, a new one when every
// channel is taken.  The pairs are held in CSR by their LARGER label, so the walk reads, for
// component k, exactly the earlier components it overlaps: O(K + pairs).
#include <cstdint>
#include <vector>

#include "../../include/ppp_mi355x.h"

extern "C" int64_t ppp_host_pack_channels(int64_t n_labels, const int64_t *sizes, const uint64_t *pairs, int64_t n_pairs,
                                          int64_t min_voxels, int32_t *chan_out, int32_t *n_channels_out) {
    if (n_labels < 0 || n_pairs < 0 || n_labels > 0x7FFFFFFF || !n_channels_out || (n_labels > 0 && (!sizes || !chan_out)) ||
        (n_pairs > 0 && !pairs))
        return -1;
    *n_channels_out = 0;
    const uint64_t K = (uint64_t)n_labels;
    // CSR by the larger label b of a key (b << 32) | a, 1 <= a < b <= K; anything else is refused
    std::vector<int64_t> start(K + 2, 0);
    for (int64_t i = 0; i < n_pairs; ++i) {
        const uint64_t b = pairs[i] >> 32, a = pairs[i] & 0xFFFFFFFFull;
        if (a < 1 || a >= b || b > K) return -1;
        ++start[b + 1];
    }
    for (uint64_t b = 1; b <= K + 1; ++b) start[b] += start[b - 1];
    std::vector<uint32_t> lower((size_t)n_pairs);
    {
        std::vector<int64_t> at(start.begin(), start.end() - 1);
        for (int64_t i = 0; i < n_pairs; ++i) lower[(size_t)at[pairs[i] >> 32]++] = (uint32_t)(pairs[i] & 0xFFFFFFFFull);
    }
    std::vector<int64_t> taken;        // taken[c] == k + 1: an earlier component of channel c overlaps component k
    int32_t n_channels = 0;
    for (uint64_t k = 0; k < K; ++k) {
        if (k == 0) {
            chan_out[0] = 0;
            n_channels = 1;
            taken.push_back(0);
            continue;
        }
        if (sizes[k] <= min_voxels) {
            chan_out[k] = 0;
            continue;
        }
        const uint64_t b = k + 1;
        for (int64_t i = start[b]; i < start[b + 1]; ++i) taken[(size_t)chan_out[lower[(size_t)i] - 1]] = (int64_t)b;
        int32_t c = 0;
        while (c < n_channels && taken[(size_t)c] == (int64_t)b) ++c;
        if (c == n_channels) {
            ++n_channels;
            taken.push_back(0);
        }
        chan_out[k] = c;
    }
    *n_channels_out = n_channels;
    return n_channels;
}
