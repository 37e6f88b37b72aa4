// view_plan_check.cpp — prints what rray_amd/csrc/frame_plan.hpp decides for batches of views (rr_render_views), the
// cases of tests/test_views_host.py: one line per case ("<kind> <case> key=value ...", a plan's message last).
#include <cstdio>

#include "frame_plan.hpp"

using namespace rr;

namespace {

const char* family_name(Family f) {
    switch (f) {
        case Family::Tree: return "Tree";
        case Family::Chain: return "Chain";
        case Family::Level0: return "Level0";
        case Family::FusedLevels: return "FusedLevels";
        case Family::Unfused: return "Unfused";
    }
    return "?";
}

FrameTraits flat() { return FrameTraits{0, 0, 0, 0, 0, true, false, false}; }
FrameTraits grouped() { return FrameTraits{1, 0, 0, 0, 0, true, false, false}; }
FrameTraits reflective(bool chain) { return FrameTraits{0, 0, 0, 0, 1, true, chain, false}; }
FrameTraits transparent(bool tree) { return FrameTraits{0, 0, 0, 1, 2, false, false, tree}; }

// `views` views of hs x vs samples at aa 1, depth 5, the frame's first run
FrameRequest batch_of(int32_t views, int64_t hs, int64_t vs, int64_t batch = (int64_t)1 << 27) {
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
    return r;
}

void events(const char* name, int64_t hs, int64_t vs) {
    std::printf("events %s E=%lld\n", name, (long long)view_events(hs, vs));
}

void plan(const char* name, const FrameTraits& t, const FrameRequest& r, const FrameSwitches& sw = FrameSwitches{}) {
    const FramePlan f = plan_frame(t, sw, r);
    std::printf("plan %s family=%s B=%lld views_per_pass=%lld levels=%d tile_fast=%d passes=%d spill=%d order=%d "
                "persist=%d zero_lcount=%d err=%d msg=%s\n",
                name, family_name(f.family), (long long)f.B, (long long)f.views_per_pass, f.P.levels, (int)f.tile_fast,
                (int)f.passes, (int)f.spill, (int)f.order.ok, (int)f.persist_candidate, (int)f.zero_lcount, f.err,
                f.msg ? f.msg : "");
}

}  // namespace

int main() {
    events("16x16", 16, 16);
    events("13x11", 13, 11);
    events("15x12", 15, 12);
    events("8x8", 8, 8);
    events("1x1", 1, 1);
    events("1920x1080", 1920, 1080);

    // passes of whole views
    plan("nine_16x16_batch_1024", flat(), batch_of(9, 16, 16, 1024));
    plan("seven_13x11_batch_1024", flat(), batch_of(7, 13, 11, 1024));
    plan("three_16x16", flat(), batch_of(3, 16, 16));
    plan("one_40x32_batch_1024", flat(), batch_of(1, 40, 32, 1024));
    plan("two_32x32_batch_1024", flat(), batch_of(2, 32, 32, 1024));

    // the in-wave families serve, the per-level ones are refused
    plan("chain", reflective(true), batch_of(3, 16, 16));
    plan("tree", transparent(true), batch_of(3, 16, 16));
    {
        FrameRequest r = batch_of(3, 16, 16);
        r.max_depth = 0;
        plan("level0_depth0", reflective(false), r);
    }
    plan("fused_levels", reflective(false), batch_of(3, 16, 16));
    plan("unfused", transparent(false), batch_of(3, 16, 16));

    // nothing of the single frames' per-camera machinery: a grouped scene's frame would be cost-ordered, a flat one a
    // candidate for the resident loop, a deep chain frame would spill under RRAY_DEEP
    plan("grouped_64x64", grouped(), batch_of(2, 64, 64));
    plan("flat_64x64", flat(), batch_of(1, 64, 64));
    {
        FrameSwitches sw;
        sw.deep = true;
        plan("chain_deep", reflective(true), batch_of(2, 64, 64), sw);
    }
    {  // the same shapes as single frames, for contrast
        FrameRequest r = batch_of(1, 64, 64);
        r.views = 0;
        r.view_e = 0;
        plan("single_grouped_64x64", grouped(), r);
        plan("single_flat_64x64", flat(), r);
    }
    {  // a request that is no whole number of views
        FrameRequest r = batch_of(3, 16, 16);
        r.total -= 64;
        plan("bad_total", flat(), r);
    }
    return 0;
}
