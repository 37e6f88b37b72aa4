// indirect_pass_check.cpp — prints what rray_amd/csrc/frame_plan.hpp decides for the passes of rr_indirect_at_device
// and rr_render_indirect_device (plan_indirect_passes), the cases of tests/test_indirect_host.py: one line per case,
// "ind <case> key=value ...".  The passes are walked the way api_sampled.cpp walks them (first += points, the last pass takes
// what is left): sum is their total in points, largest and smallest the extremes, count how many there were, misaligned
// how many start at a point index or a ray index that is not a multiple of 64, pass_rays the largest pass's rays.
// A stand-alone subject for -fsanitize=address,undefined on the header.
#include <algorithm>
#include <cstdio>

#include "frame_plan.hpp"

using namespace rr;

namespace {

void ind(const char* name, int64_t n_points, int32_t samples, int64_t batch, int64_t want) {
    const IndirectPassPlan p = plan_indirect_passes(n_points, samples, batch, want);
    int64_t sum = 0, largest = 0, smallest = 0, count = 0, misaligned = 0;
    for (int64_t first = 0; p.points > 0 && first < n_points; first += p.points) {
        const int64_t np = std::min<int64_t>(p.points, n_points - first);
        sum += np;
        largest = std::max(largest, np);
        smallest = count ? std::min(smallest, np) : np;
        misaligned += first % 64 != 0 || (first * samples) % 64 != 0;
        ++count;
    }
    std::printf("ind %s points=%lld passes=%lld sum=%lld largest=%lld smallest=%lld count=%lld misaligned=%lld "
                "pass_rays=%lld\n",
                name, (long long)p.points, (long long)p.passes, (long long)sum, (long long)largest, (long long)smallest,
                (long long)count, (long long)misaligned, (long long)(largest * samples));
}

}  // namespace

int main() {
    const int64_t big = (int64_t)1 << 27;  // the context's default batch
    ind("none", 0, 4, big, 0);
    ind("no_samples", 100, 0, big, 0);
    ind("no_batch", 100, 4, 0, 0);
    // n = 1, 63, 64, 65 with K = 1, 3, 1024 under a pass of 64 points
    ind("n1_k1_pass64", 1, 1, big, 64);
    ind("n63_k3_pass64", 63, 3, big, 64);
    ind("n64_k1024_pass64", 64, 1024, big, 64);
    ind("n65_k3_pass64", 65, 3, big, 64);
    ind("n65_k1024_pass64", 65, 1024, big, 64);
    // the override rounds up to a multiple of 64
    ind("n65_k3_pass1", 65, 3, big, 1);
    ind("n384_k16_pass65", 384, 16, big, 65);
    // the default: the largest multiple of 64 points with at most 2^22 rays, at least 64 points
    ind("n1_k1", 1, 1, big, 0);
    ind("n65_k1024", 65, 1024, big, 0);
    ind("hd_k1", 1920 * 1080, 1, big, 0);
    ind("hd_k3", 1920 * 1080, 3, big, 0);
    ind("hd_k4", 1920 * 1080, 4, big, 0);
    ind("hd_k1024", 1920 * 1080, 1024, big, 0);
    ind("k100000", 1000, 100000, big, 0);  // beyond RR_MAX_INDIRECT_SAMPLES: the function itself is total
    // the context's batch caps a pass, rounded down to a multiple of 64 (rr_create keeps RRAY_BATCH >= 1024)
    ind("hd_k4_batch1024", 1920 * 1080, 4, 1024, 0);
    ind("n3000_k1_batch1100", 3000, 1, 1100, 0);
    ind("n3000_k1_batch1100_pass4096", 3000, 1, 1100, 4096);
    ind("n100_k1_batch10", 100, 1, 10, 0);
    // an override never reaches 2^32 rays
    ind("huge_override_k1024", 10000000, 1024, (int64_t)1 << 40, (int64_t)1 << 50);
    ind("huge_override_k1", 1000, 1, (int64_t)1 << 50, (int64_t)1 << 50);
    return 0;
}
