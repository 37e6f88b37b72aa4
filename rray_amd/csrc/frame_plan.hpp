// frame_plan.hpp — which kernels serve a frame, decided once and on the host alone: the kernel family, the batch and
// its queues, the AA passes, the deep queue, the level-0 cost order and whether the persistent loop may serve.  Pure
// functions of plain values: no HIP, no environment, no allocation, no context (api.cpp reads the scene, the
// switches and the context into FrameTraits / FrameSwitches / FrameRequest, and launches what the plan says).
// Compiles with a plain host compiler; tests/test_frame_plan_host.py pins the decisions.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "../../include/rray/rray.h"
#include "wavefront.hpp"

namespace rr {

// Worst-case queue bytes of a batch of nb level-0 events: every shading event queues max_children
// children (k), so level d holds at most nb * k^d events.  The levels are launched for that capacity
// and read their live counts from HBM (no host round trip between levels).
struct LevelPlan {
    int64_t cap[RR_MAX_DEPTH + 1];  // capacity per level (array size; segmented: nseg * seg_cap)
    int64_t seg_cap[RR_MAX_DEPTH + 1];  // segmented (fused) levels >= 1: capacity of each of RR_NSEG segments
    int levels;                     // levels launched (depth + 1, or 1 without secondary rays)
    int64_t ev_cap[2];              // ev_a (odd levels), ev_b (even levels >= 2)
    int64_t max_cap;
    size_t bytes;
};
// fused: levels >= 1 in RR_NSEG segments (wavefront.hpp); level 0's block b fills segment b % RR_NSEG
// of level 1, so a segment holds at most ceil(blocks / RR_NSEG) * 256 * k events, and a segment of
// level d feeds only the same segment of level d + 1
inline LevelPlan plan_levels(int64_t nb, int k, int max_depth, bool ext, bool fused = false) {
    LevelPlan p{};
    int64_t w = nb;
    for (int d = 0; d <= max_depth; ++d) {
        p.cap[d] = w;
        p.levels = d + 1;
        p.max_cap = std::max(p.max_cap, w);
        const bool kids = d < max_depth && k > 0;
        if (!kids) break;
        p.bytes += (size_t)w * (sizeof(rr::CombRec) + (ext ? sizeof(rr::CombExt) : 0) + sizeof(int32_t));
        if (fused) {
            p.seg_cap[d + 1] = d == 0 ? (((nb + 255) / 256 + rr::RR_NSEG - 1) / rr::RR_NSEG) * 256 * k : p.seg_cap[d] * k;
            p.seg_cap[d + 1] = (p.seg_cap[d + 1] + 255) / 256 * 256;
            w = rr::RR_NSEG * p.seg_cap[d + 1];
        } else {
            w *= k;
        }
        int64_t& e = p.ev_cap[d % 2];  // level d+1 lands in ev_a when d is even
        e = std::max(e, w);
    }
    p.bytes += (size_t)p.max_cap * (sizeof(rr::HitRec) + 2 * sizeof(double) + sizeof(int32_t));
    p.bytes += (size_t)(p.ev_cap[0] + p.ev_cap[1]) * sizeof(rr::Event);
    return p;
}

// The scene facts the decisions read, and the three family predicates as the device units answer them for this
// scene and depth (fused_levels / chain_levels / tree_levels, kernels.hpp: they read RRAY_UNFUSED / RRAY_NO_CHAIN /
// RRAY_NO_TREE).
struct FrameTraits {
    int has_groups, general, has_area, has_transparent, max_children;
    bool fused, chain, tree;
};

// api.cpp's own switches, as read for this call
struct FrameSwitches {
    int aa_passes = 1;            // RRAY_AA_PASSES (>= 1)
    bool deep = false;            // RRAY_DEEP=1
    int order_group = 1;          // RRAY_ORDER_GROUP=4: kOrderGroup, else 1
    bool no_chain_order = false;  // RRAY_NO_CHAIN_ORDER
    bool no_tile_guess = false;   // RRAY_NO_TILE_GUESS
    bool no_pw = false;           // RRAY_NO_PW
};
constexpr int kOrderGroup = 4;  // kernels.hpp RR_ORDER_GROUP: a launch block's four tiles

// Tree: the color_at trees of transparent scenes inside the camera lanes.  Chain: reflection chains inside the
// level-0 waves.  Level0: fused trace + shade with no secondary ray (no reflective material, or depth 0).  These
// three finish every sample in its level-0 wave: one level, no recursion queues.  FusedLevels: fused trace + shade
// per level, segmented queues between them.  Unfused: trace / n1n2 / shade per level and the bottom-up combine.
enum class Family { Tree, Chain, Level0, FusedLevels, Unfused };
inline Family frame_family(const FrameTraits& t, int max_depth) {
    if (t.tree) return Family::Tree;
    if (t.chain) return Family::Chain;
    if (!t.fused) return Family::Unfused;
    return t.max_children == 0 || max_depth == 0 ? Family::Level0 : Family::FusedLevels;
}
inline bool in_wave(Family f) { return f == Family::Tree || f == Family::Chain || f == Family::Level0; }

// level-0 tiles all full 8x8 and the batch tile-aligned: a wave is one tile (LevelArgs.tile_fast)
inline bool full_tiles(bool rays0, int64_t hs, int64_t lrows, int64_t base) {
    return !rays0 && lrows > 0 && hs % 8 == 0 && lrows % 8 == 0 && base % 64 == 0;
}
// pixel waves of a part: bands of two output rows, wpb waves each
inline int64_t pixel_waves(int32_t pw_rows, uint32_t pw_wpb) { return (int64_t)((pw_rows + 1) / 2) * pw_wpb; }

// How a camera frame's averaged image is produced.  wave_avg: by the level-0 waves themselves (deliver_wave_avg) —
// every pixel's samples lie in one wave's 8x8 tile (aa in {2, 4, 8}, full tiles) and every sample is final in its
// wave (an in-wave family).  pw: aa == 3 frames of the chain / tree families in pixel waves (7 whole pixels per wave,
// pw_wpb waves per band of two output rows), which average in the wave too.  direct_avg: the kernels write the
// average (aa == 1, wave_avg or pw); otherwise it is a box average over the canvas.
struct OutputPlan {
    bool wave_avg, pw, direct_avg;
    uint32_t pw_wpb;
};
inline OutputPlan plan_output(const FrameTraits& t, const FrameSwitches& sw, bool want_avg, int32_t aa, int64_t hs,
                              int64_t lrows, int max_depth, int32_t block_rows, int64_t batch) {
    const Family f = frame_family(t, max_depth);
    OutputPlan o{};
    o.wave_avg = want_avg && (aa == 2 || aa == 4 || aa == 8) && hs % 8 == 0 && lrows % 8 == 0 && lrows > 0 && in_wave(f);
    o.pw = want_avg && !o.wave_avg && aa == 3 && (f == Family::Tree || f == Family::Chain) && block_rows % 2 == 0 &&
           hs * lrows <= batch && !sw.no_pw;
    o.direct_avg = want_avg && (aa == 1 || o.wave_avg || o.pw);
    o.pw_wpb = (uint32_t)((2 * (hs / aa) + 6) / 7);
    return o;
}

// One run of the levels: the frame's shape, what the caller supplies and asks for, the context's limits and state.
struct FrameRequest {
    int64_t total;  // level-0 events
    int max_depth;
    int64_t hs, lrows;
    int32_t aa, block_rows;
    bool rays0;     // level-0 rays are the caller's (rr_color_at)
    bool listed;    // level-0 events are the samples of listed pixels (adaptive frames' refine pass)
    bool pw;        // pixel waves, and their geometry
    int32_t pw_rows;
    uint32_t pw_wpb;
    bool canvas;    // samples are delivered one by one
    bool box_avg;   // ... and box-averaged after the levels (the AA passes' candidate)
    int32_t aa_wave;  // the level-0 waves average (0: off)
    int64_t batch;
    size_t queue_budget;
    bool zero_next;  // the frame's first run: its first launch clears the next frame's counters
    // a batch of views (rr_render_views): `views` cameras of hs x lrows samples each, every view view_e =
    // view_events(hs, lrows) level-0 events (total = views * view_e).  0: a single frame.  Last, value-initialised.
    int32_t views{};
    int64_t view_e{};
    // an ordered ray batch (rr_color_at_device_ordered): with rays0, level-0 slot t works on ray
    // perm[t]; served by the listed kernels, which hold the in-wave families only.  Last, value-initialised.
    bool ordered{};
};

// level-0 events of one view of a batch: its samples rounded up to whole waves, so a wave never holds two views
inline int64_t view_events(int64_t hs, int64_t lrows) { return (hs * lrows + 63) / 64 * 64; }
// level-0 events one pass of a batch of views may hold: the context's batch, indexed in 32 bits as a part's samples
inline int64_t view_pass_cap(int64_t batch) { return std::min<int64_t>(batch, ((int64_t)1 << 31) - 64); }
// whole views per pass of a batch of `views` views of view_e events each (never more than the batch has), or 0 when
// one view does not fit a pass
inline int64_t views_in_pass(int64_t batch, int64_t view_e, int64_t views) {
    const int64_t cap = view_pass_cap(batch);
    return view_e > cap ? 0 : std::min<int64_t>(cap / view_e, views);
}

// The pass split of rr_render_views_aov (first-hit planes of a batch of views): the view branch of
// plan_frame's arithmetic and nothing else of a frame's plan — the first-hit kernel has no family, no queues, no
// order and no resident loop.  Pass p renders views [p * views_per_pass, min(views, (p + 1) * views_per_pass)).
struct ViewAovPlan {
    int64_t view_e;          // level-0 events of one view (view_events)
    int64_t views_per_pass;  // whole views per launch
    int64_t passes;          // launches
    bool tile_fast;          // every view is full 8x8 tiles
    int err;                 // RR_OK, or RR_E_ARG / RR_E_LIMIT and its text
    const char* msg;
};
inline ViewAovPlan plan_views_aov(int64_t batch, int64_t hs, int64_t lrows, int32_t views) {
    ViewAovPlan p{};
    if (hs <= 0 || lrows <= 0 || views < 0 || batch <= 0 || hs > ((int64_t)1 << 31) || lrows > ((int64_t)1 << 31)) {
        p.err = RR_E_ARG;
        p.msg = "internal: a view batch is views of hs x lrows samples, hs and lrows in 1 .. 2^31";
        return p;
    }
    p.view_e = view_events(hs, lrows);
    p.tile_fast = full_tiles(false, hs, lrows, 0);
    if (views == 0) return p;
    p.views_per_pass = views_in_pass(batch, p.view_e, views);
    if (p.views_per_pass == 0) {
        p.err = RR_E_LIMIT;
        p.msg = "one view's samples must fit one pass of the context (render such a view with rr_render_aov)";
        return p;
    }
    p.passes = (views + p.views_per_pass - 1) / p.views_per_pass;
    return p;
}

// The pass split of rr_hit_at_device (first hits of a device-resident ray batch): the first-hit
// kernel writes a pass's records as planes into the context's staging buffer and hit_records_kernel turns them into
// the caller's records, so a pass holds at most min(batch, kRayPassMax) rays and the staging never exceeds
// kRayPassMax * sizeof(rr_hit) bytes.  Pass p holds rays [p * pass, min(n, (p + 1) * pass)): every pass but the last is
// `pass` rays, and the sizes sum to n.  n <= 0 (or batch <= 0): no pass.
constexpr int64_t kRayPassMax = (int64_t)1 << 22;
struct RayPassPlan {
    int64_t pass;    // rays per pass (the last may be shorter)
    int64_t passes;  // launches
};
inline RayPassPlan plan_ray_passes(int64_t n, int64_t batch) {
    RayPassPlan p{};
    if (n <= 0 || batch <= 0) return p;
    p.pass = std::min<int64_t>(std::min<int64_t>(batch, kRayPassMax), n);
    p.passes = (n + p.pass - 1) / p.pass;
    return p;
}

// The pass split of rr_render_lens_device (lens frames): passes of whole pixels, S rays each.  Every
// pass but the last holds `pixels` pixels, a multiple of 64, so each pass starts at a ray index that is a multiple of 64
// and its level-0 waves are the one-shot batch's.  want > 0 (RRAY_LENS_PASS): that many pixels rounded up to a multiple
// of 64; else the largest multiple of 64 with at most kRayPassMax rays, and at least 64 pixels.  Pass k holds pixels
// [k * pixels, min(n_pixels, (k + 1) * pixels)).
struct LensPassPlan {
    int64_t pixels;  // per pass (the last may be shorter)
    int64_t passes;
};
inline LensPassPlan plan_lens_passes(int64_t n_pixels, int32_t samples, int64_t want) {
    LensPassPlan p{};
    if (n_pixels <= 0 || samples < 1) return p;
    if (want > 0)
        p.pixels = want > ((int64_t)1 << 40) ? (int64_t)1 << 40 : (want + 63) / 64 * 64;
    else
        p.pixels = std::max<int64_t>(64, kRayPassMax / samples / 64 * 64);
    p.passes = (n_pixels + p.pixels - 1) / p.pixels;
    return p;
}

// The pass split of rr_render_ao_device (ambient-occlusion frames): passes of whole points (canvas
// samples), K occlusion pairs each.  Every pass but the last holds `points` points, a multiple of 64, so a pass's
// camera rays and first hits fill whole waves.  want > 0 (RRAY_AO_PASS): that many points rounded up to a multiple of
// 64; else the largest multiple of 64 with at most kRayPassMax pairs, and at least 64 points.  Either is then capped by
// the context's batch rounded down to a multiple of 64 (at least 64): a pass's first hits are one launch of the
// first-hit kernel.  Pass k holds points [k * points, min(n_points, (k + 1) * points)).
struct AoPassPlan {
    int64_t points;  // per pass (the last may be shorter)
    int64_t passes;
};
inline AoPassPlan plan_ao_passes(int64_t n_points, int32_t samples, int64_t batch, int64_t want) {
    AoPassPlan p{};
    if (n_points <= 0 || samples < 1 || batch <= 0) return p;
    if (want > 0)
        p.points = want > ((int64_t)1 << 40) ? (int64_t)1 << 40 : (want + 63) / 64 * 64;
    else
        p.points = std::max<int64_t>(64, kRayPassMax / samples / 64 * 64);
    p.points = std::min<int64_t>(p.points, std::max<int64_t>(64, batch / 64 * 64));
    // an override never asks a launch for 2^32 pairs or more (the kernel indexes its pairs in 32 bits)
    p.points = std::min<int64_t>(p.points, std::max<int64_t>(64, ((((int64_t)1 << 32) - 1) / samples) / 64 * 64));
    p.passes = (n_points + p.points - 1) / p.points;
    return p;
}

// The pass split of rr_indirect_at_device and rr_render_indirect_device (one-bounce indirect light):
// passes of whole points, K gathered rays each, so that the scratch of a pass (48 + 24 bytes per ray) is bounded whatever
// the batch or the frame.  plan_ao_passes' rules with RRAY_INDIRECT_PASS for `want`: every pass but the last holds
// `points` points, a multiple of 64 (a pass's first ray is then a multiple of 64 too: whole waves); want > 0: that many
// points rounded up to a multiple of 64; else the largest multiple of 64 with at most kRayPassMax rays, and at least 64
// points.  Either is capped by the context's batch rounded down to a multiple of 64 (at least 64: a frame pass's first
// hits are one launch of the first-hit kernel) and kept below 2^32 rays.  Pass k holds points
// [k * points, min(n_points, (k + 1) * points)).
struct IndirectPassPlan {
    int64_t points;  // per pass (the last may be shorter)
    int64_t passes;
};
inline IndirectPassPlan plan_indirect_passes(int64_t n_points, int32_t samples, int64_t batch, int64_t want) {
    IndirectPassPlan p{};
    if (n_points <= 0 || samples < 1 || batch <= 0) return p;
    if (want > 0)
        p.points = want > ((int64_t)1 << 40) ? (int64_t)1 << 40 : (want + 63) / 64 * 64;
    else
        p.points = std::max<int64_t>(64, kRayPassMax / samples / 64 * 64);
    p.points = std::min<int64_t>(p.points, std::max<int64_t>(64, batch / 64 * 64));
    p.points = std::min<int64_t>(p.points, std::max<int64_t>(64, ((((int64_t)1 << 32) - 1) / samples) / 64 * 64));
    p.passes = (n_points + p.points - 1) / p.points;
    return p;
}

struct FramePlan {
    Family family;
    bool fused, ext;  // segmented queues between the levels; refraction halves beside the pending sums
    int k, plan_depth;  // children per event and depth the queues are planned for (0, 0: the in-wave families)
    int64_t B;        // level-0 events per batch
    LevelPlan P;      // of a whole batch
    bool zero_lcount;  // the per-level queue counters are zeroed per batch (the in-wave chains and trees use none)
    bool pad_children;  // fused levels queue a wave's children in a 64-slot block of its own
    bool tile_fast;   // full_tiles at base 0
    bool passes;      // AA passes: B is whole output rows, each batch's rows are averaged on the second stream
    bool spill;       // chain frames send chains still reflecting at RR_DEEP_FROM to the deep queue
    int64_t deep_nseg, deep_seg_cap;
    struct {
        bool ok;          // the level-0 waves run costliest tile first
        int64_t n_tiles;  // tiles or pixel waves of the part (0: a ragged frame or explicit rays)
        int64_t n_pad;    // ... rounded up to whole launch blocks
        int group;
        int32_t pad;      // the order key's variant bits: chain / tree frames, single-wave units
    } order;
    int64_t pw_n;     // pixel waves: the launch's events, whole waves of 64 lanes
    bool persist_candidate;  // all the persistent loop asks of a frame but rr::persist_plan's own answer
    int64_t views_per_pass;  // a batch of views: whole views per pass (B = views_per_pass * view_e), else 0
    int err;          // RR_OK, or the code and text the run fails with
    const char* msg;
};

inline FramePlan plan_frame(const FrameTraits& t, const FrameSwitches& sw, const FrameRequest& r) {
    FramePlan f{};
    f.family = frame_family(t, r.max_depth);
    f.fused = t.fused;
    f.ext = t.has_transparent != 0;
    const bool one_level = in_wave(f.family);
    const bool chain = f.family == Family::Tree || f.family == Family::Chain;
    f.k = chain ? 0 : t.max_children;
    f.plan_depth = chain ? 0 : r.max_depth;
    // batch: at most r.batch camera samples, shrunk (power-of-two steps, tile-aligned) until the
    // worst-case queues fit the context's budget and every event index fits in int32
    f.B = std::max<int64_t>(64, std::min<int64_t>(r.batch, r.total));
    for (;;) {
        const LevelPlan p = plan_levels(f.B, f.k, f.plan_depth, f.ext, f.fused);
        const int64_t last = p.cap[p.levels - 1];
        if (f.B <= 4096 || (p.bytes <= r.queue_budget && last < ((int64_t)1 << 31) && p.max_cap < ((int64_t)1 << 31)))
            break;
        f.B = std::max<int64_t>(4096, (f.B / 2) & ~(int64_t)63);
    }
    // AA passes: batches of whole output rows (a multiple of lcm(8, aa) sample rows, so every batch is whole
    // 8-row tile bands and whole pixels), about sw.aa_passes of them.  Default one pass: measured on C3 (chain
    // kernel), 2 / 4 / 8 passes cost 7.29 / 7.61 / 8.01 ms per frame against 7.08 — each pass ends in its own tail
    // of long chains, and the averages did not overlap it
    if (r.box_avg && r.canvas && !r.rays0 && r.hs % 8 == 0 && r.lrows % 8 == 0) {
        int64_t rows_unit = 8;
        while (rows_unit % r.aa) rows_unit += 8;
        const int64_t unit = rows_unit * r.hs;
        const int64_t units = r.total / unit;
        if (r.total % unit == 0 && units >= 2 && sw.aa_passes > 1 && f.B >= unit) {
            f.B = std::min((units + sw.aa_passes - 1) / sw.aa_passes, f.B / unit) * unit;
            f.passes = true;
        }
    }
    // listed pixels: one batch, served by the in-wave kernels only
    if (r.listed && (f.B < r.total || !one_level)) {
        f.err = RR_E_ARG;
        f.msg = "internal: the listed-pixel pass needs one batch of a production kernel family";
        return f;
    }
    // an ordered ray batch: any number of batches, the in-wave kernels only
    if (r.ordered && (!r.rays0 || r.listed || r.views > 0 || r.pw || r.box_avg)) {
        f.err = RR_E_ARG;
        f.msg = "internal: an ordered ray batch is the caller's rays and nothing else";
        return f;
    }
    if (r.ordered && !one_level) {
        f.err = RR_E_ARG;
        f.msg = "ordered ray batches are not served by the per-level paths (RRAY_UNFUSED / RRAY_NO_TREE / RRAY_NO_CHAIN)";
        return f;
    }
    // a batch of views: passes of whole views through the in-wave kernels, one launch each.  No per-camera state of
    // the context serves it: no cached bundles, no cost order, no resident loop, no deep queue, no pixel waves
    if (r.views > 0) {
        if (r.view_e < 64 || r.view_e % 64 != 0 || r.view_e < r.hs * r.lrows || r.total != r.views * r.view_e || r.rays0 ||
            r.listed || r.pw || r.box_avg) {
            f.err = RR_E_ARG;
            f.msg = "internal: a view batch is whole views of whole waves from camera rays";
            return f;
        }
        if (!one_level) {
            f.err = RR_E_ARG;
            f.msg = "batches of views are not served by the per-level paths (RRAY_UNFUSED / RRAY_NO_TREE / RRAY_NO_CHAIN)";
            return f;
        }
        // a pass's samples are indexed in 32 bits, as a part's
        f.views_per_pass = views_in_pass(r.batch, r.view_e, r.views);
        if (f.views_per_pass == 0) {
            f.err = RR_E_LIMIT;
            f.msg = "one view's samples must fit one pass of the context (render such a view with rr_render)";
            return f;
        }
        f.B = f.views_per_pass * r.view_e;
        f.passes = false;
    }
    f.P = plan_levels(f.B, f.k, f.plan_depth, f.ext, f.fused);
    if (f.P.max_cap >= ((int64_t)1 << 31)) {
        f.err = RR_E_LIMIT;
        f.msg = "recursion queues exceed 2^31 events (lower max_depth)";
        return f;
    }
    if (r.pw && (!chain || f.B < r.total)) {  // the launch holds whole waves of 7 pixels
        f.err = RR_E_ARG;
        f.msg = "internal: pixel waves need one chain-kernel batch";
        return f;
    }
    f.zero_lcount = f.P.levels > 1 || (f.ext && f.family != Family::Tree);
    // the blocks keep a secondary wave one camera tile's rays, as coherent as they come: packed queues mixed 2-4
    // tiles per wave (C3 10.54 -> 8.98 ms with the blocks); the area-light scenes' block-wide sample dealing
    // prefers packed waves (C5 2.27 vs 2.30 ms)
    f.pad_children = f.fused && !t.has_area;
    f.tile_fast = full_tiles(r.rays0, r.hs, r.lrows, 0);  // a batch of views: of each view
    // deep chains: frames whose samples are delivered one by one (not the in-wave AA average).  Opt-in: on C3 the
    // deep launch took 1.85 ms for what the camera waves did in 1.54 — the deep rays' walks are latency-bound
    // whether their waves are full or not
    f.spill = f.family == Family::Chain && r.aa_wave == 0 && !r.pw && !r.listed && !r.ordered && r.views == 0 && r.max_depth >= RR_DEEP_FROM && sw.deep;
    f.deep_seg_cap = (int64_t)256 << RR_DEEP_SHIFT;
    f.deep_nseg = (((f.B + 255) / 256) + (1 << RR_DEEP_SHIFT) - 1) >> RR_DEEP_SHIFT;
    // cost-ordered level-0 tiles: one-batch frames of full 8x8 tiles whose level 0 is the whole frame (no
    // secondary rays) in scenes with groups, where tile costs spread widest (mesh silhouettes against floor:
    // C4 0.596 -> 0.511 ms per frame).  Flat scenes' tiles cost alike (C2 +0.6 % with the order), and frames
    // with queued reflections lose their children queues' tile order (C3 +2 %): both keep launch order.
    // Chain frames order their camera waves too (tiles or pixel waves; the chains' depths spread tile costs widely)
    const int64_t n_tiles = r.pw ? pixel_waves(r.pw_rows, r.pw_wpb) : f.tile_fast ? r.hs * r.lrows / 64 : 0;
    // the order's unit: single waves, so a block's four waves cost alike (the costliest first) and the block's
    // resources free together.  Groups of a block's four adjacent tiles (their output rows join into whole cache
    // lines) measured slower: C3 6.33 vs 7.17 ms, C4 0.510 vs 0.520 ms, C5 equal
    f.order.group = sw.order_group;
    f.order.n_tiles = n_tiles;
    // the launch's last block may hold up to three wave slots past the last tile (n_tiles not a multiple of 4: a
    // pixel-wave part of 270 output rows has 148 230 waves): the order and cost arrays run to whole blocks, the extra
    // slots' order entries are their own indices (their lanes are past the launch's samples and do nothing but record
    // a cost nobody sorts)
    f.order.n_pad = (n_tiles + 3) & ~(int64_t)3;
    f.order.ok = r.views == 0 && (f.fused || t.tree) && !t.general && f.B >= r.total && n_tiles > 0 && n_tiles < ((int64_t)1 << 31) &&
                 (sw.order_group == 1 || n_tiles % 4 == 0) &&  // the group order permutes a block's four tiles
                 (r.pw || n_tiles * 64 == r.total) &&
                 ((t.has_groups && (f.k == 0 || r.max_depth == 0)) || (chain && !sw.no_chain_order));
    f.pw_n = r.pw ? n_tiles * 64 : 0;
    // chain and level-0-only frames of one layout, and each order unit, keep orders of their own
    f.order.pad = (chain ? 1 : 0) | (sw.order_group == 1 ? 2 : 0);
    // a one-level, one-batch frame of full tiles may run as one resident launch
    f.persist_candidate = f.family == Family::Level0 && !r.listed && r.views == 0 && f.B >= r.total && f.tile_fast && !r.pw &&
                          r.total % 64 == 0 && r.total / 64 < ((int64_t)1 << 31) && r.zero_next;
    return f;
}

}  // namespace rr
