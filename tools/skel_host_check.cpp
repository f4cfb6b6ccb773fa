// skel_host_check.cpp -- the host side of the 3-d thinning under a sanitizer, as a program of its own
// (nothing is loaded into Python).  Build and run on the CPU:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tools/skel_host_check.cpp patchperpix_amd/csrc/ppp_host_skel.cpp -o /tmp/skel_host_check && /tmp/skel_host_check
//
// It runs ppp_host_skel_rule_mismatches on a single-threaded and on a threaded sub-range and
// ppp_host_skeletonize_3d on the 6 x 6 x 34 bar of tests/test_skeleton.py; exit status 0 = all as expected.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int64_t ppp_host_skel_rule_mismatches(uint32_t first, uint32_t count);
extern "C" int64_t ppp_host_skeletonize_3d(const uint8_t *mask, const int32_t *vol, uint8_t *out);

int main() {
    int rc = 0;
    const int64_t a = ppp_host_skel_rule_mismatches(12345u, 1u << 16);               // one thread
    const int64_t b = ppp_host_skel_rule_mismatches((1u << 26) - (1u << 21), 1u << 21);  // 16 threads, up to the end
    const int64_t c = ppp_host_skel_rule_mismatches(1u << 26, 1u);                   // out of range
    std::printf("rule mismatches: %lld %lld (out of range: %lld)\n", (long long)a, (long long)b, (long long)c);
    if (a != 0 || b != 0 || c != -1) rc = 1;

    const int32_t vol[3] = {12, 14, 40};
    std::vector<uint8_t> mask((size_t)vol[0] * vol[1] * vol[2], 0), out(mask.size(), 7);
    for (int z = 3; z < 9; ++z)
        for (int y = 4; y < 10; ++y)
            for (int x = 3; x < 37; ++x) mask[((size_t)z * vol[1] + y) * vol[2] + x] = 1;
    const int64_t kept = ppp_host_skeletonize_3d(mask.data(), vol, out.data());
    int64_t sum = 0;
    for (uint8_t v : out) sum += v;
    std::printf("bar 6 x 6 x 34: kept %lld (sum %lld)\n", (long long)kept, (long long)sum);
    if (kept != 30 || sum != 30) rc = 1;
    return rc;
}
