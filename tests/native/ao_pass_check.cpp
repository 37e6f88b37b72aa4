// ao_pass_check.cpp — prints what rray_amd/csrc/frame_plan.hpp decides for the passes of rr_render_ao_device
// (plan_ao_passes), the cases of tests/test_ao_host.py: one line per case, "ao <case> key=value ...".  The passes are
// walked the way api_sampled.cpp walks them (first += points, the last pass takes what is left): sum is their total in points,
// largest and smallest the extremes, count how many there were, misaligned how many start at a point index that is not
// a multiple of 64, pass_pairs the largest pass's pairs.
// It also runs rray_amd/csrc/ao_dir.hpp on the host over the basis's edge normals ("dir <case> finite=.. ..."), so the
// program is a stand-alone subject for -fsanitize=address,undefined on both headers.
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "ao_dir.hpp"
#include "frame_plan.hpp"

using namespace rr;

namespace {

void ao(const char* name, int64_t n_points, int32_t samples, int64_t batch, int64_t want) {
    const AoPassPlan p = plan_ao_passes(n_points, samples, batch, want);
    int64_t sum = 0, largest = 0, smallest = 0, count = 0, misaligned = 0;
    for (int64_t first = 0; p.points > 0 && first < n_points; first += p.points) {
        const int64_t np = std::min<int64_t>(p.points, n_points - first);
        sum += np;
        largest = std::max(largest, np);
        smallest = count ? std::min(smallest, np) : np;
        misaligned += first % 64 != 0;
        ++count;
    }
    std::printf("ao %s points=%lld passes=%lld sum=%lld largest=%lld smallest=%lld count=%lld misaligned=%lld "
                "pass_pairs=%lld\n",
                name, (long long)p.points, (long long)p.passes, (long long)sum, (long long)largest, (long long)smallest,
                (long long)count, (long long)misaligned, (long long)(largest * samples));
}

void dir(const char* name, double x, double y, double z) {
    const double N[3] = {x, y, z};
    int finite = 1, above = 1;
    double worst = 0.0;
    for (uint64_t i = 0; i < 4; ++i) {
        const uint32_t base = ao_base(7, ((uint64_t)1 << 32) - 70 + i);
        for (uint32_t k = 0; k < 1024; k += 31) {
            double w[3];
            ao_direction(base, k, N, w);
            finite = finite && std::isfinite(w[0]) && std::isfinite(w[1]) && std::isfinite(w[2]);
            above = above && (w[0] * N[0] + w[1] * N[1]) + w[2] * N[2] >= 0.0;
            worst = std::max(worst, std::fabs(std::sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]) - 1.0));
        }
    }
    std::printf("dir %s finite=%d above=%d unit=%d\n", name, finite, above, worst <= 4 * 2.220446049250313e-16 ? 1 : 0);
}

}  // namespace

int main() {
    const int64_t big = (int64_t)1 << 27;  // the context's default batch
    ao("none", 0, 16, big, 0);
    ao("no_samples", 100, 0, big, 0);
    ao("no_batch", 100, 16, 0, 0);
    // the GPU tests' frames under RRAY_AO_PASS=64 and =1 (rounded up), and by default
    ao("t65_k3_pass64", 65, 3, big, 64);
    ao("t65_k3_pass1", 65, 3, big, 1);
    ao("t384_k16_pass65", 384, 16, big, 65);
    ao("t384_k16_default", 384, 16, big, 0);
    // the default: the largest multiple of 64 points with at most 2^22 pairs, at least 64 points
    ao("hd_k16", 1920 * 1080, 16, big, 0);
    ao("hd_k1", 1920 * 1080, 1, big, 0);
    ao("hd_k5", 1920 * 1080, 5, big, 0);
    ao("hd_k1024", 1920 * 1080, 1024, big, 0);
    ao("k100000", 1000, 100000, big, 0);  // beyond RR_MAX_AO_SAMPLES: the function itself is total
    // the context's batch caps a pass, rounded down to a multiple of 64 (rr_create keeps RRAY_BATCH >= 1024)
    ao("hd_k16_batch1024", 1920 * 1080, 16, 1024, 0);
    ao("t3000_k1_batch1100", 3000, 1, 1100, 0);
    ao("t3000_k1_batch1100_pass4096", 3000, 1, 1100, 4096);
    ao("t100_k1_batch10", 100, 1, 10, 0);
    // an override never reaches 2^32 pairs
    ao("huge_override_k1024", 10000000, 1024, (int64_t)1 << 40, (int64_t)1 << 50);
    ao("huge_override_k1", 1000, 1, (int64_t)1 << 50, (int64_t)1 << 50);

    dir("x", 1, 0, 0);
    dir("-x", -1, 0, 0);
    dir("y", 0, 1, 0);
    dir("-y", 0, -1, 0);
    dir("z", 0, 0, 1);
    dir("-z", 0, 0, -1);
    dir("z+0", 0.6, 0.8, 0.0);
    dir("z-0", 0.6, 0.8, -0.0);
    {
        const double e = 1e-9, z = -1.0 + e, r = std::sqrt(1.0 - z * z);
        dir("near-z", r * 0.6, r * 0.8, z);
    }
    return 0;
}
