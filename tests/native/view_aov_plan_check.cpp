// view_aov_plan_check.cpp — prints what rray_amd/csrc/frame_plan.hpp decides for the passes of rr_render_views_aov
// (plan_views_aov), the cases of tests/test_views_aov_host.py: one line per case ("<kind> <case> key=value ...", a
// plan's message last).
#include <cstdio>

#include "frame_plan.hpp"

using namespace rr;

namespace {

void plan(const char* name, int64_t batch, int64_t hs, int64_t vs, int32_t views) {
    const ViewAovPlan p = plan_views_aov(batch, hs, vs, views);
    std::printf("plan %s view_e=%lld views_per_pass=%lld passes=%lld tile_fast=%d err=%d msg=%s\n", name,
                (long long)p.view_e, (long long)p.views_per_pass, (long long)p.passes, (int)p.tile_fast, p.err,
                p.msg ? p.msg : "");
}

// the colour batches' plan of the same shape (plan_frame's view branch): the arithmetic is shared, so both agree
void colour(const char* name, int64_t batch, int64_t hs, int64_t vs, int32_t views) {
    FrameRequest r{};
    r.views = views;
    r.view_e = view_events(hs, vs);
    r.total = views * r.view_e;
    r.max_depth = 5;
    r.hs = hs;
    r.lrows = vs;
    r.aa = 1;
    r.block_rows = 8;
    r.batch = batch;
    r.queue_budget = (size_t)32 << 30;
    r.zero_next = true;
    const FramePlan f = plan_frame(FrameTraits{0, 0, 0, 0, 0, true, false, false}, FrameSwitches{}, r);
    std::printf("colour %s views_per_pass=%lld err=%d msg=%s\n", name, (long long)f.views_per_pass, f.err,
                f.msg ? f.msg : "");
}

}  // namespace

int main() {
    const int64_t big = (int64_t)1 << 27, cap31 = ((int64_t)1 << 31) - 64;
    std::printf("cap limits default=%lld small=%lld huge=%lld msg=\n", (long long)view_pass_cap(big),
                (long long)view_pass_cap(1024), (long long)view_pass_cap((int64_t)1 << 40));
    // the GPU test's passes: a context under RRAY_BATCH=1024
    plan("nine_16x16_batch_1024", 1024, 16, 16, 9);
    plan("seven_13x11_batch_1024", 1024, 13, 11, 7);
    plan("two_40x32_batch_1024", 1024, 40, 32, 2);
    plan("one_40x32_batch_2048", 2048, 40, 32, 1);
    colour("nine_16x16_batch_1024", 1024, 16, 16, 9);
    colour("seven_13x11_batch_1024", 1024, 13, 11, 7);
    colour("two_40x32_batch_1024", 1024, 40, 32, 2);
    // never more views per pass than the batch has; nothing to do for none
    plan("three_16x16", big, 16, 16, 3);
    plan("none", big, 16, 16, 0);
    plan("one_1x1", big, 1, 1, 1);
    // a view of exactly the pass cap fits, one wave more does not: the context's batch ...
    plan("exactly_batch_1024", 1024, 32, 32, 3);
    plan("batch_1024_plus_64", 1024, 32, 34, 3);
    // ... and the 32-bit index limit under a batch beyond it: 2^31 - 64 = (2^25 - 1) x 64 samples, then 2^25 x 64
    plan("exactly_cap31", (int64_t)1 << 40, cap31 / 64, 64, 2);
    plan("cap31_plus_64", (int64_t)1 << 40, cap31 / 64 + 1, 64, 2);
    plan("bad_size", big, 0, 16, 2);
    plan("negative_views", big, 16, 16, -1);
    return 0;
}
