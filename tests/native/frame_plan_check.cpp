// frame_plan_check.cpp — prints what rray_amd/csrc/frame_plan.hpp decides for the cases of
// tests/test_frame_plan_host.py, one line per case ("<kind> <case> key=value ...", a plan's message last).
#include <cstdio>
#include <functional>

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

// scenes: flat and opaque unless the case says otherwise
FrameTraits flat() { return FrameTraits{0, 0, 0, 0, 0, true, false, false}; }
FrameTraits grouped() { return FrameTraits{1, 0, 0, 0, 0, true, false, false}; }
FrameTraits reflective(bool chain) { return FrameTraits{0, 0, 0, 0, 1, true, chain, false}; }
FrameTraits transparent(bool tree) { return FrameTraits{0, 0, 0, 1, 2, false, false, tree}; }
FrameTraits unfused(int k) { return FrameTraits{0, 0, 0, 0, k, false, false, false}; }

// a 64 x 64 frame at aa 1, depth 5, one batch, the frame's first run
FrameRequest frame(int64_t hs = 64, int64_t lrows = 64) {
    FrameRequest r{};
    r.total = hs * lrows;
    r.max_depth = 5;
    r.hs = hs;
    r.lrows = lrows;
    r.aa = 1;
    r.block_rows = 8;
    r.batch = (int64_t)1 << 27;
    r.queue_budget = (size_t)32 << 30;
    r.zero_next = true;
    return r;
}

void levels(const char* name, int64_t nb, int k, int depth, bool ext, bool fused) {
    const LevelPlan p = plan_levels(nb, k, depth, ext, fused);
    std::printf("levels %s levels=%d max_cap=%lld ev_a=%lld ev_b=%lld bytes=%zu cap=", name, p.levels,
                (long long)p.max_cap, (long long)p.ev_cap[0], (long long)p.ev_cap[1], p.bytes);
    for (int d = 0; d < p.levels; ++d) std::printf("%s%lld", d ? "," : "", (long long)p.cap[d]);
    std::printf(" seg_cap=");
    for (int d = 0; d < p.levels; ++d) std::printf("%s%lld", d ? "," : "", (long long)p.seg_cap[d]);
    std::printf("\n");
}

void plan(const char* name, const FrameTraits& t, const FrameRequest& r, const FrameSwitches& sw = FrameSwitches{}) {
    const FramePlan f = plan_frame(t, sw, r);
    std::printf("plan %s family=%s k=%d plan_depth=%d B=%lld levels=%d max_cap=%lld zero_lcount=%d pad_children=%d "
                "tile_fast=%d passes=%d spill=%d deep_nseg=%lld deep_seg_cap=%lld order=%d n_tiles=%lld n_pad=%lld "
                "group=%d pad=%d pw_n=%lld persist=%d err=%d msg=%s\n",
                name, family_name(f.family), f.k, f.plan_depth, (long long)f.B, f.P.levels, (long long)f.P.max_cap,
                (int)f.zero_lcount, (int)f.pad_children, (int)f.tile_fast, (int)f.passes, (int)f.spill,
                (long long)f.deep_nseg, (long long)f.deep_seg_cap, (int)f.order.ok, (long long)f.order.n_tiles,
                (long long)f.order.n_pad, f.order.group, (int)f.order.pad, (long long)f.pw_n, (int)f.persist_candidate,
                f.err, f.msg ? f.msg : "");
}
// a case that changes a few fields of a request / the switches
using Req = std::function<void(FrameRequest&)>;
using Sw = std::function<void(FrameSwitches&)>;
void plan(const char* name, const FrameTraits& t, FrameRequest r, const Req& edit, const Sw& sw_edit = nullptr) {
    FrameSwitches sw;
    if (edit) edit(r);
    if (sw_edit) sw_edit(sw);
    plan(name, t, r, sw);
}

void output(const char* name, const FrameTraits& t, bool want_avg, int32_t aa, int64_t hs, int64_t lrows, int depth = 5,
            int32_t block = 8, int64_t batch = (int64_t)1 << 27, bool no_pw = false) {
    FrameSwitches sw;
    sw.no_pw = no_pw;
    const OutputPlan o = plan_output(t, sw, want_avg, aa, hs, lrows, depth, block, batch);
    std::printf("output %s wave_avg=%d pw=%d direct_avg=%d pw_wpb=%u\n", name, (int)o.wave_avg, (int)o.pw,
                (int)o.direct_avg, o.pw_wpb);
}

// the pixel-wave part of W x H output pixels at aa 3
FrameRequest pw_frame(int64_t W, int64_t H) {
    FrameRequest r = frame(3 * W, 3 * H);
    r.aa = 3;
    r.pw = true;
    r.pw_rows = (int32_t)H;
    r.pw_wpb = (uint32_t)((2 * W + 6) / 7);
    return r;
}

}  // namespace

int main() {
    std::printf("sizes Event=%zu HitRec=%zu CombRec=%zu CombExt=%zu DeepRec=%zu nseg=%d deep_from=%d deep_shift=%d "
                "max_depth=%d e_arg=%d e_limit=%d\n",
                sizeof(Event), sizeof(HitRec), sizeof(CombRec), sizeof(CombExt), sizeof(DeepRec), RR_NSEG, RR_DEEP_FROM,
                RR_DEEP_SHIFT, RR_MAX_DEPTH, RR_E_ARG, RR_E_LIMIT);

    // 1. plan_levels
    levels("unfused_k2_d3", 4096, 2, 3, false, false);
    levels("fused_k1_d2", 768, 1, 2, false, true);
    levels("k0", 1000, 0, 5, false, false);
    levels("ext_k2_d1", 64, 2, 1, true, false);

    // 2. family
    plan("flat_opaque", flat(), frame());
    plan("reflective_d5", reflective(true), frame());
    plan("reflective_d0", reflective(false), frame(), [](FrameRequest& r) { r.max_depth = 0; });
    plan("fused_levels_d3", reflective(false), frame(), [](FrameRequest& r) { r.max_depth = 3; });
    plan("tree_d0", transparent(true), frame(), [](FrameRequest& r) { r.max_depth = 0; });
    plan("tree_d5", transparent(true), frame());
    plan("transparent_no_tree_d2", transparent(false), frame(), [](FrameRequest& r) { r.max_depth = 2; });

    // 3. output mode
    output("aa1", flat(), true, 1, 64, 64);
    output("aa2_level0", flat(), true, 2, 64, 64);
    output("aa4_chain", reflective(true), true, 4, 64, 64);
    output("aa8_level0_d0", reflective(false), true, 8, 64, 64, 0);
    output("aa2_tree", transparent(true), true, 2, 64, 64);
    output("aa2_fused_levels", reflective(false), true, 2, 64, 64);
    output("aa2_unfused", transparent(false), true, 2, 64, 64);
    output("aa2_ragged_13x9", flat(), true, 2, 26, 18);
    output("aa2_no_avg", flat(), false, 2, 64, 64);
    output("aa3_chain", reflective(true), true, 3, 42, 30);
    output("aa3_tree", transparent(true), true, 3, 42, 30);
    output("aa3_level0", flat(), true, 3, 42, 30);
    output("aa3_chain_no_pw", reflective(true), true, 3, 42, 30, 5, 8, (int64_t)1 << 27, true);
    output("aa3_chain_odd_block", reflective(true), true, 3, 42, 30, 5, 1);
    output("aa3_chain_no_avg", reflective(true), false, 3, 42, 30);
    output("aa3_chain_over_batch", reflective(true), true, 3, 42, 30, 5, 8, 1259);
    plan("pw_14x10", reflective(true), pw_frame(14, 10));

    // 4. batch
    const Req million = [](FrameRequest& r) {
        r.total = 1000000;
        r.hs = 1000;
        r.lrows = 1000;
        r.max_depth = 3;
    };
    plan("batch_fits", unfused(2), frame(), million);
    plan("batch_halves", unfused(2), frame(), [&](FrameRequest& r) {
        million(r);
        r.queue_budget = 435159040;
    });
    plan("batch_stops_4096", unfused(2), frame(), [&](FrameRequest& r) {
        million(r);
        r.queue_budget = 1;
    });
    plan("batch_limit", unfused(6), frame(), [&](FrameRequest& r) {
        million(r);
        r.max_depth = 8;
        r.queue_budget = 1;
    });

    // 5. order
    const Req two_batches = [](FrameRequest& r) { r.batch = 2048; };
    const Sw group4 = [](FrameSwitches& s) { s.order_group = kOrderGroup; };
    plan("order_groups", grouped(), frame());
    plan("order_chain", reflective(true), frame());
    plan("order_flat", flat(), frame());
    FrameTraits general = grouped();
    general.general = 1;
    plan("order_general", general, frame());
    plan("order_two_batches", grouped(), frame(), two_batches);
    plan("order_no_chain_order", reflective(true), frame(), nullptr, [](FrameSwitches& s) { s.no_chain_order = true; });
    plan("order_group4", grouped(), frame(), nullptr, group4);
    plan("order_9_tiles", grouped(), frame(24, 24));
    plan("order_9_tiles_group4", grouped(), frame(24, 24), nullptr, group4);
    plan("order_pw_270_rows", reflective(true), pw_frame(3840, 270));
    plan("order_ragged", grouped(), frame(26, 18));

    // 6. persist candidate
    plan("persist", flat(), frame());
    plan("persist_listed", flat(), frame(), [](FrameRequest& r) { r.listed = true; });
    plan("persist_pw", flat(), pw_frame(14, 10));
    plan("persist_ragged", flat(), frame(26, 18));
    plan("persist_levels", reflective(false), frame());
    plan("persist_two_batches", flat(), frame(), two_batches);
    plan("persist_second_run", flat(), frame(), [](FrameRequest& r) { r.zero_next = false; });

    // 7. guards
    plan("listed_fused_levels", reflective(false), frame(), [](FrameRequest& r) { r.listed = true; });
    plan("listed_two_batches", flat(), frame(), [&](FrameRequest& r) {
        r.listed = true;
        two_batches(r);
    });
    plan("listed_chain", reflective(true), frame(), [](FrameRequest& r) { r.listed = true; });
    plan("pw_two_batches", reflective(true), pw_frame(14, 10), [](FrameRequest& r) { r.batch = 1024; });
    const Req canvas = [](FrameRequest& r) { r.canvas = true; };
    const Sw deep = [](FrameSwitches& s) { s.deep = true; };
    plan("spill", reflective(true), frame(), canvas, deep);
    plan("spill_1m", reflective(true), frame(1024, 1024), canvas, deep);
    plan("spill_off", reflective(true), frame(), canvas);
    plan("spill_tree", transparent(true), frame(), canvas, deep);
    plan("spill_level0", flat(), frame(), canvas, deep);
    plan("spill_aa_wave", reflective(true), frame(), [](FrameRequest& r) { r.aa_wave = 4; }, deep);
    plan("spill_pw", reflective(true), pw_frame(14, 10), nullptr, deep);
    plan("spill_listed", reflective(true), frame(), [](FrameRequest& r) { r.listed = true; }, deep);
    plan("spill_depth_1", reflective(true), frame(), [](FrameRequest& r) { r.max_depth = 1; }, deep);
    const Req box48 = [](FrameRequest& r) {  // 16 x 16 pixels at aa 3 through the canvas
        r.aa = 3;
        r.canvas = r.box_avg = true;
    };
    const Sw np2 = [](FrameSwitches& s) { s.aa_passes = 2; };
    plan("passes_2", reflective(true), frame(48, 48), box48, np2);
    plan("passes_default", reflective(true), frame(48, 48), box48);
    plan("passes_8_of_4_units", reflective(true), frame(48, 96), box48, [](FrameSwitches& s) { s.aa_passes = 8; });
    plan("passes_part_unit", reflective(true), frame(48, 40), box48, np2);
    plan("passes_small_batch", reflective(true), frame(48, 48), [&](FrameRequest& r) {
        box48(r);
        r.batch = 1024;
    }, np2);
    plan("passes_direct", reflective(true), frame(48, 48), [](FrameRequest& r) { r.aa = 3; }, np2);
    return 0;
}
