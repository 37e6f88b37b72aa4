// ray_pass_check.cpp — prints what rray_amd/csrc/frame_plan.hpp decides for the passes of rr_hit_at_device
// (plan_ray_passes), the cases of tests/test_rays_host.py: one line per case, "pass <case> key=value ...".  The pass
// sizes are walked the way api_queries.cpp walks them (first += pass, the last pass takes what is left): sum is their total,
// largest and smallest the extremes, count how many there were.
#include <algorithm>
#include <cstdio>

#include "frame_plan.hpp"

using namespace rr;

namespace {

void pass(const char* name, int64_t n, int64_t batch) {
    const RayPassPlan p = plan_ray_passes(n, batch);
    int64_t sum = 0, largest = 0, smallest = 0, count = 0;
    for (int64_t first = 0; p.pass > 0 && first < n; first += p.pass) {
        const int64_t np = std::min<int64_t>(p.pass, n - first);
        sum += np;
        largest = std::max(largest, np);
        smallest = count ? std::min(smallest, np) : np;
        ++count;
    }
    std::printf("pass %s n=%lld batch=%lld pass=%lld passes=%lld sum=%lld largest=%lld smallest=%lld count=%lld\n", name,
                (long long)n, (long long)batch, (long long)p.pass, (long long)p.passes, (long long)sum,
                (long long)largest, (long long)smallest, (long long)count);
}

}  // namespace

int main() {
    const int64_t big = (int64_t)1 << 27, cap = (int64_t)1 << 22;
    std::printf("pass_max limit value=%lld\n", (long long)kRayPassMax);
    pass("none", 0, big);
    pass("negative", -5, big);
    pass("one", 1, big);
    pass("one_batch_1", 1, 1);
    pass("seven_batch_1", 7, 1);
    // the GPU tests' batches: 300 rays under a batch of 128, 2500 under 1024
    pass("n300_batch_128", 300, 128);
    pass("n2500_batch_1024", 2500, 1024);
    // a pass size exactly, one less, one more: under the context's batch ...
    pass("exactly_batch_1024", 1024, 1024);
    pass("batch_1024_minus_1", 1023, 1024);
    pass("batch_1024_plus_1", 1025, 1024);
    pass("three_batches_1024", 3072, 1024);
    // ... and under the staging cap with the default batch beyond it
    pass("exactly_cap", cap, big);
    pass("cap_minus_1", cap - 1, big);
    pass("cap_plus_1", cap + 1, big);
    pass("small_default", 300, big);
    pass("limit_32_bit", ((int64_t)1 << 32) - 1, big);
    pass("batch_below_cap", 3 * cap, cap / 2);
    return 0;
}
