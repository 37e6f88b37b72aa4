// lens_pass_check.cpp — prints what rray_amd/csrc/frame_plan.hpp decides for the passes of rr_render_lens_device
// (plan_lens_passes), the cases of tests/test_lens_host.py: one line per case, "lens <case> key=value ...".  The passes
// are walked the way api_sampled.cpp walks them (first += pixels, the last pass takes what is left): sum is their total in
// pixels, largest and smallest the extremes, count how many there were, misaligned how many start at a ray index that
// is not a multiple of 64.
#include <algorithm>
#include <cstdio>

#include "frame_plan.hpp"

using namespace rr;

namespace {

void lens(const char* name, int64_t n_pixels, int32_t samples, int64_t want) {
    const LensPassPlan p = plan_lens_passes(n_pixels, samples, want);
    int64_t sum = 0, largest = 0, smallest = 0, count = 0, misaligned = 0;
    for (int64_t first = 0; p.pixels > 0 && first < n_pixels; first += p.pixels) {
        const int64_t np = std::min<int64_t>(p.pixels, n_pixels - first);
        sum += np;
        largest = std::max(largest, np);
        smallest = count ? std::min(smallest, np) : np;
        misaligned += (first * samples) % 64 != 0;
        ++count;
    }
    std::printf("lens %s pixels=%lld passes=%lld sum=%lld largest=%lld smallest=%lld count=%lld misaligned=%lld "
                "pass_rays=%lld\n",
                name, (long long)p.pixels, (long long)p.passes, (long long)sum, (long long)largest, (long long)smallest,
                (long long)count, (long long)misaligned, (long long)(largest * samples));
}

}  // namespace

int main() {
    lens("none", 0, 8, 0);
    lens("no_samples", 100, 0, 0);
    // the GPU tests' frame: 20 x 10, S = 3, under RRAY_LENS_PASS=64 and =1 (rounded up), and by default
    lens("t200_s3_pass64", 200, 3, 64);
    lens("t200_s3_pass1", 200, 3, 1);
    lens("t200_s3_pass65", 200, 3, 65);
    lens("t200_s3_default", 200, 3, 0);
    // the default: the largest multiple of 64 pixels with at most 2^22 rays, at least 64 pixels
    lens("hd_s8", 1920 * 1080, 8, 0);
    lens("hd_s1", 1920 * 1080, 1, 0);
    lens("hd_s5", 1920 * 1080, 5, 0);
    lens("hd_s4096", 1920 * 1080, 4096, 0);
    lens("hd_s3000", 1920 * 1080, 3000, 0);
    lens("s100000", 1000, 100000, 0);  // beyond RR_MAX_LENS_SAMPLES: the function itself is total
    lens("exactly_one_pass_s8", 524288, 8, 0);
    lens("one_more_pixel_s8", 524289, 8, 0);
    lens("huge_override", 1000, 2, (int64_t)1 << 50);
    return 0;
}
