// api.cpp — the core of the C ABI of include/rray/rray.h: error state, device context, scene upload, and the wavefront
// level loop that replaces Camera::render (camera.rs:107-121) with the frame entries built on it.  The other entry
// points are in api_queries.cpp, api_frames.cpp, api_sampled.cpp and api_filters.cpp, over api_ctx.hpp.
#include "api_ctx.hpp"

static thread_local std::string g_err;

void rr_set_error(const char* msg) { g_err = msg ? msg : ""; }

#pragma GCC visibility push(hidden)
namespace rr::api {

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int check_opts(const rr_camera* cam, const rr_render_opts* o) {
    if (!cam || !o) return fail(RR_E_ARG, "null camera/options");
    if (o->aa < 1) return fail(RR_E_ARG, "aa must be >= 1");
    if (o->max_depth < 0 || o->max_depth > RR_MAX_DEPTH) return fail(RR_E_LIMIT, "max_depth out of range");
    if (o->nparts < 1 || o->part < 0 || o->part >= o->nparts) return fail(RR_E_ARG, "bad part/nparts");
    if (cam->hsize <= 0 || cam->vsize <= 0 || cam->hsize % o->aa || cam->vsize % o->aa)
        return fail(RR_E_ARG, "camera size must be a positive multiple of aa");
    if (cam->hsize > (1ll << 31) || cam->vsize > (1ll << 31)) return fail(RR_E_LIMIT, "camera too large");
    if (o->row_begin != 0 || o->row_end != 0) {  // a band of output rows (ABI 10)
        if (o->part != 0 || o->nparts != 1) return fail(RR_E_ARG, "a band (row_begin / row_end) is part 0 of 1");
        if (o->row_begin < 0 || o->row_end <= o->row_begin || o->row_end > cam->vsize / o->aa)
            return fail(RR_E_ARG, "band rows out of range: need 0 <= row_begin < row_end <= height");
    }
    return RR_OK;
}

// output rows of the part (interleaved blocks) or band (rr_render_opts row_begin / row_end)
static int64_t opts_rows(const rr_render_opts* o, int64_t H) {
    if (o->row_begin != 0 || o->row_end != 0) return (int64_t)o->row_end - o->row_begin;
    return rr::part_rows_count(H, o->part, o->nparts, o->block_rows > 0 ? o->block_rows : 8);
}

rr::DevCamera dev_camera(const rr_camera* c) {
    rr::DevCamera d{};
    d.hsize = c->hsize;
    d.vsize = c->vsize;
    d.half_width = c->half_width;
    d.half_height = c->half_height;
    d.pixel_size = c->pixel_size;
    rr::M4 t{};
    for (int i = 0; i < 16; ++i) t.m[i] = c->transform[i];
    rr::M4 inv = rr::inverse(t);  // camera.rs:85 (cached inverse, same value)
    for (int i = 0; i < 16; ++i) d.inv[i] = inv.m[i];
    for (int r = 0; r < 4; ++r)  // camera.rs:86 with the kernel's operation order (no contraction)
        d.origin[r] = d.inv[4 * r] * 0.0 + d.inv[4 * r + 1] * 0.0 + d.inv[4 * r + 2] * 0.0 + d.inv[4 * r + 3] * 1.0;
    return d;
}

// the level-0 arguments a camera frame starts from: the camera, the part layout and the jitter
void set_camera(rr::LevelArgs& A, const rr_camera* cam) {
    A.cam = dev_camera(cam);
    A.cam_affine = A.cam.inv[12] == 0.0 && A.cam.inv[13] == 0.0 && A.cam.inv[14] == 0.0 && A.cam.inv[15] == 1.0 &&
                   A.cam.origin[3] == 1.0;
}
rr::LevelArgs camera_args(const rr_camera* cam, const rr_render_opts* o, int32_t aa, int32_t part, int32_t block) {
    rr::LevelArgs A{};
    set_camera(A, cam);
    A.hs = cam->hsize;
    A.aa = aa;
    A.part = part;
    A.nparts = o->nparts;
    A.block_rows = block;
    A.rays0 = nullptr;
    A.seed = o->seed;
    A.jitter_mode = o->jitter_mode;
    return A;
}

constexpr int kRR_ORDER_EVERY = 64;  // frames between re-sorts of the level-0 tile order

// A frame's counter buffers.  begin: the frame's first run_levels counts into buffer `epoch` and has its first launch
// clear the other one (zero_next).  end: the frame's buffer becomes the statistics' source, and the cleared one the
// next frame's.  A frame that launched nothing (a part with no rows: total == 0) cleared nothing and counted nothing:
// its buffer, still all zero, stays the next frame's — handed the other one, the next frame would count on top of the
// counts of the frame before, and the persistent level-0 loop would find its queue heads (C_WORK) used up and render
// no tile.
void begin_frame_counters(rr_ctx* c) {
    c->zero_next = true;
    c->next_zeroed = false;
    c->persist_last = {0, 0};
}
void end_frame_counters(rr_ctx* c) {
    c->stats_src = frame_counters(c, c->epoch);
    if (c->next_zeroed) c->epoch ^= 1;
}

// Heads of the persistent level-0 loop's tile queue (persist_map.hpp): a power of two <= RR_PERSIST_MAX_HEADS.
// RRAY_PERSIST_HEADS=n overrides the default (rounded down to a power of two), read at launch.  128: C2 0.1087 ms
// per frame against 0.1102 with 32 and 0.1086 with 256 (profiles/persist/ab_design.json, session 3).
constexpr uint32_t kRR_PERSIST_HEADS = 128;
static uint32_t persist_heads() {
    uint32_t want = kRR_PERSIST_HEADS;
    if (const char* e = std::getenv("RRAY_PERSIST_HEADS")) want = (uint32_t)std::max(1, std::atoi(e));
    uint32_t h = 1;
    while (h * 2u <= want && h * 2u <= rr::RR_PERSIST_MAX_HEADS) h *= 2u;
    return h;
}

// level-0 index math: magic divisors, and the wave-uniform tile path when every tile is a full 8x8 and the
// batch starts on a tile boundary
void set_level0_index(rr::LevelArgs& A) {
    A.aa_magic = A.aa > 1 ? (uint32_t)((1ull << 32) / (uint64_t)A.aa) : 0u;
    A.br_magic = A.block_rows > 1 ? (uint32_t)((1ull << 32) / (uint64_t)A.block_rows) : 0u;
    A.tile_fast = rr::full_tiles(A.rays0 != nullptr, A.hs, A.lrows, A.base) ? 1 : 0;
    A.tiles_per_row = (uint32_t)(A.hs / 8);
}

// The per-tile camera bundles of this render's part (tile_bundle_kernel), recomputed only when the camera or
// the part layout changed since the last render on this context.  Null when the tiles are not all full 8x8
// or the camera is not affine (the walks build their bundles themselves then).
int tile_bundles(rr_ctx* c, const rr::LevelArgs& base_args, hipStream_t st, const float** out) {
    *out = nullptr;
    rr::LevelArgs T = base_args;
    T.base = 0;
    T.level = 0;
    set_level0_index(T);
    if ((!T.tile_fast && !T.pw) || !T.cam_affine) return RR_OK;
    // few-node flat scenes with LDS culls walk node by node without bundles (walk_nodes)
    if (!c->S.has_groups && !c->S.general && c->S.lds_culls && c->S.n_nodes <= rr::RR_BUNDLE_MIN_NODES) return RR_OK;
    // one bundle per 8x8 tile, or per pixel wave (A.pw)
    const int64_t n_tiles = T.pw ? rr::pixel_waves(T.pw_rows, T.pw_wpb) : T.hs * T.lrows / 64;
    const size_t want = (size_t)n_tiles * rr::RR_TILE_BUNDLE_FLOATS * sizeof(float);
    if (want > c->tiles.bytes) {
        HIPCHK(c->tiles.ensure(want));
        c->tiles_valid = false;
    }
    rr_ctx::TileKey key{};
    key.cam = T.cam;
    key.hs = T.hs;
    key.lrows = T.lrows;
    key.aa = T.aa;
    key.part = T.part;
    key.nparts = T.nparts;
    key.block_rows = T.block_rows;
    key.pw = T.pw;
    if (!c->tiles_valid || std::memcmp(&key, &c->tile_key, sizeof key) != 0) {
        if (T.pw)
            HIPCHK(rr::launch_pixel_wave_bundles(T, c->tiles.as<float>(), n_tiles, st));
        else
            HIPCHK(rr::launch_tile_bundles(c->S, T, c->tiles.as<float>(), n_tiles, st));
        c->tile_key = key;
        c->tiles_valid = true;
    }
    *out = c->tiles.as<float>();
    return RR_OK;
}

static_assert(rr::kOrderGroup == rr::RR_ORDER_GROUP, "frame_plan.hpp's order group is the sort's");
// api.cpp's own switches in one pass over the environment, which costs what one getenv does (six of them per
// frame would show in the sub-millisecond frames)
static rr::FrameSwitches read_switches() {
    rr::FrameSwitches s;
    for (char** e = environ; e && *e; ++e) {
        if (std::strncmp(*e, "RRAY_", 5) != 0) continue;
        const char* name = *e + 5;
        const char* eq = std::strchr(name, '=');
        if (!eq) continue;
        const std::string_view key(name, (size_t)(eq - name));
        if (key == "AA_PASSES")
            s.aa_passes = std::max(1, std::atoi(eq + 1));
        else if (key == "DEEP")
            s.deep = std::atoi(eq + 1) == 1;
        else if (key == "ORDER_GROUP")
            s.order_group = std::atoi(eq + 1) == rr::kOrderGroup ? rr::kOrderGroup : 1;
        else if (key == "NO_CHAIN_ORDER")
            s.no_chain_order = true;
        else if (key == "NO_TILE_GUESS")
            s.no_tile_guess = true;
        else if (key == "NO_PW")
            s.no_pw = true;
    }
    return s;
}
FrameFacts frame_facts(const rr_ctx* c, int max_depth) {
    const rr::DevScene& S = c->S;
    FrameFacts f;
    f.traits.has_groups = S.has_groups;
    f.traits.general = S.general;
    f.traits.has_area = S.has_area;
    f.traits.has_transparent = c->host.has_transparent;
    f.traits.max_children = c->host.max_children;
    f.traits.fused = rr::fused_levels(S);
    f.traits.chain = rr::chain_levels(S, c->host.max_children, max_depth);
    f.traits.tree = rr::tree_levels(S);
    f.sw = read_switches();
    return f;
}


// `rows` output rows from row y0 on, from their samples at src
static hipError_t launch_average(const AaPasses& a, const double* src, int64_t y0, int64_t rows, hipStream_t st,
                          rr::KernelProf* kp) {
    return a.f32 ? rr::launch_aa_f32(src, static_cast<float*>(a.avg) + 3 * y0 * a.width, a.width, rows, a.aa, st, kp)
                 : rr::launch_aa(src, static_cast<double*>(a.avg) + 3 * y0 * a.width, a.width, rows, a.aa, st, kp);
}


rr::FramePlan plan_run(const rr_ctx* c, const FrameFacts& facts, const rr::LevelArgs& A, int64_t total, int max_depth,
                       const FrameOut& o) {
    rr::FrameRequest r{};
    r.total = total;
    r.max_depth = max_depth;
    r.hs = A.hs;
    r.lrows = A.lrows;
    r.aa = A.aa;
    r.block_rows = A.block_rows;
    r.rays0 = A.rays0 != nullptr;
    r.listed = A.list != nullptr && !A.rays0;
    r.ordered = A.list != nullptr && A.rays0 != nullptr;  // the listed kernels' second source: an ordered ray batch
    r.pw = A.pw != 0;
    r.pw_rows = A.pw_rows;
    r.pw_wpb = A.pw_wpb;
    r.canvas = o.out != nullptr;
    r.box_avg = o.aap != nullptr;
    r.aa_wave = o.aa_wave;
    r.batch = c->batch;
    r.queue_budget = c->queue_budget;
    r.zero_next = c->zero_next;
    if (A.views) {
        r.view_e = A.view_e;
        r.views = (int32_t)(total / A.view_e);
    }
    return rr::plan_frame(facts.traits, facts.sw, r);
}

namespace {  // run_levels' own steps

int grow_workspace(rr_ctx* c, const rr::FramePlan& plan) {
    const rr::LevelPlan& P = plan.P;
    if ((int)c->comb.size() < P.levels) {
        c->comb.resize(P.levels);
        c->comb_ext.resize(P.levels);
        c->pend.resize(P.levels);
    }
    if (plan.family == rr::Family::Unfused) {  // hit records and n1/n2 lists: the trace / n1n2 / shade kernels only
        HIPCHK(c->hit.ensure(P.max_cap * sizeof(rr::HitRec)));
        HIPCHK(c->n12.ensure(P.max_cap * 2 * sizeof(double)));
        HIPCHK(c->n1n2.ensure(P.max_cap * sizeof(int32_t)));
    }
    for (int d = 0; d + 1 < P.levels; ++d) {
        HIPCHK(c->comb[d].ensure(P.cap[d] * sizeof(rr::CombRec)));
        if (plan.ext) HIPCHK(c->comb_ext[d].ensure(P.cap[d] * sizeof(rr::CombExt)));
        HIPCHK(c->pend[d].ensure(P.cap[d] * sizeof(int32_t)));
    }
    if (P.ev_cap[0]) HIPCHK(c->ev_a.ensure(P.ev_cap[0] * sizeof(rr::Event)));
    if (P.ev_cap[1]) HIPCHK(c->ev_b.ensure(P.ev_cap[1] * sizeof(rr::Event)));
    if (plan.passes && !c->aa_stream) HIPCHK(hipStreamCreateWithFlags(&c->aa_stream, hipStreamNonBlocking));
    if (plan.spill) {
        HIPCHK(c->deep.ensure((size_t)plan.deep_nseg * plan.deep_seg_cap * sizeof(rr::DeepRec)));
        HIPCHK(c->deep_count.ensure((size_t)(plan.deep_nseg + 2) * sizeof(unsigned int)));
    }
    if (plan.order.ok) {
        HIPCHK(c->tile_cost.ensure((size_t)plan.order.n_pad * sizeof(uint32_t)));
        HIPCHK(c->tile_perm.ensure((size_t)plan.order.n_pad * sizeof(uint32_t)));
        HIPCHK(c->tile_hist.ensure(256 * sizeof(uint32_t)));
    }
    return RR_OK;
}

// ---- the level-0 cost order of frames with plan.order.ok: the three functions below are all that touches the
// context's order state (order_valid / order_age / order_key / order_tiles / perm_tail) ----
int sort_order(rr_ctx* c, const rr::FramePlan& plan, hipStream_t st) {
    HIPCHK(rr::launch_tile_order(c->tile_cost.as<uint32_t>(), c->tile_perm.as<uint32_t>(), c->tile_hist.as<uint32_t>(),
                                 plan.order.n_tiles, plan.order.group, st));
    c->order_valid = true;
    return RR_OK;
}
// before the frame's launches: a new layout drops the order, and a layout's first frame is ordered by a guess
int refresh_order(rr_ctx* c, const rr::LevelArgs& base_args, const rr::FramePlan& plan, bool guess, hipStream_t st) {
    const int64_t n_tiles = plan.order.n_tiles, n_pad = plan.order.n_pad;
    rr_ctx::TileKey key{};  // the layout only: a camera change keeps the order (costs stay a good guess)
    key.hs = base_args.hs;
    key.lrows = base_args.lrows;
    key.aa = base_args.aa;
    key.part = base_args.part;
    key.nparts = base_args.nparts;
    key.block_rows = base_args.block_rows;
    key.pw = base_args.pw;
    key.pad = plan.order.pad;
    if (c->order_tiles != n_tiles || std::memcmp(&key, &c->order_key, sizeof key) != 0) {
        c->order_valid = false;
        c->order_tiles = n_tiles;
        c->order_key = key;
        if (n_pad > n_tiles) {  // the identity for the slots past the last tile
            for (int64_t t = n_tiles; t < n_pad; ++t) c->perm_tail[t - n_tiles] = (uint32_t)t;
            HIPCHK(hipMemcpyAsync(c->tile_perm.as<uint32_t>() + n_tiles, c->perm_tail,
                                  (size_t)(n_pad - n_tiles) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        }
    }
    // a layout's first frame: order by a guess from the camera bundles (launch order left the first frame's
    // slowest tiles last: C4 0.59 vs 0.51 ms), and re-sort by the measured costs right after it
    if (!c->order_valid && base_args.tile_bundles && guess) {
        HIPCHK(rr::launch_tile_guess(c->S, base_args.tile_bundles, c->tile_cost.as<uint32_t>(), n_tiles, st));
        int rc = sort_order(c, plan, st);
        if (rc != RR_OK) return rc;
        c->order_age = kRR_ORDER_EVERY - 1;
    }
    return RR_OK;
}
// level 0's arguments.  The waves record their costs only in a frame the sort after it reads (every
// kRR_ORDER_EVERY-th): each record is one scattered 4-byte store per wave, a partial line that L2 writes back alone
// (47 MB of the C3 chain kernel's 0.55 GB of writes per frame, profiles/r05/attrib_c3.txt)
void order_level0_args(const rr_ctx* c, const rr::FramePlan& plan, rr::LevelArgs& A) {
    const bool sort_after = !c->order_valid || c->order_age + 1 >= kRR_ORDER_EVERY;
    A.tile_perm = c->order_valid ? c->tile_perm.as<uint32_t>() : nullptr;
    A.tile_cost = sort_after ? c->tile_cost.as<uint32_t>() : nullptr;
    A.order_group = plan.order.group;
}
// after level 0's launch: one frame older, re-sorted by the costs it recorded when due
int age_order(rr_ctx* c, const rr::FramePlan& plan, hipStream_t st) {
    if (c->order_valid && ++c->order_age < kRR_ORDER_EVERY) return RR_OK;
    int rc = sort_order(c, plan, st);
    if (rc == RR_OK) c->order_age = 0;
    return rc;
}

// Level d of the batch at `base` (p: the batch's queues): the frame's arguments plus the level's queues, outputs,
// counters and, at level 0 of ordered frames, the order.
rr::LevelArgs level_args(rr_ctx* c, const rr::LevelArgs& base_args, const rr::FramePlan& plan, const rr::LevelPlan& p,
                         int64_t base, int d, int max_depth, const FrameOut& o) {
    unsigned int* lc = c->lcount.as<unsigned int>();  // per-level queue counters [level][LC_*]
    const bool fused = plan.fused, ext = plan.ext, children_possible = d + 1 < p.levels;
    rr::LevelArgs A = base_args;
    A.base = base;
    set_level0_index(A);
    A.level = d;
    A.rem = max_depth - d;
    A.n = A.pw ? plan.pw_n : p.cap[d];  // pixel waves: whole waves of 7 pixels
    A.n_dev = d > 0 ? lc + (d - 1) * rr::LC_COUNT + rr::LC_CHILDREN : base_args.list ? base_args.n_dev : nullptr;
    A.nseg = fused && d > 0 ? rr::RR_NSEG : 1;
    A.nseg_out = fused ? rr::RR_NSEG : 1;
    A.seg_cap = fused && d > 0 ? p.seg_cap[d] : 0;
    A.seg_cap_out = fused && children_possible ? p.seg_cap[d + 1] : 0;
    A.seg_count = lc + d * rr::LC_COUNT + rr::LC_SEG0;
    A.seg_out_count = children_possible ? lc + (d + 1) * rr::LC_COUNT + rr::LC_SEG0 : nullptr;
    // level d reads ev_b when d is even (d >= 2), ev_a when odd; writes the other one
    A.ev = d == 0 ? nullptr : (d % 2 ? c->ev_a : c->ev_b).as<rr::Event>();
    A.hit = c->hit.as<rr::HitRec>();
    A.n12 = c->n12.as<double>();
    A.comb = children_possible ? c->comb[d].as<rr::CombRec>() : nullptr;
    A.parent_comb = d > 0 ? c->comb[d - 1].as<rr::CombRec>() : nullptr;
    A.comb_ext = ext && children_possible ? c->comb_ext[d].as<rr::CombExt>() : nullptr;
    A.parent_ext = ext && d > 0 ? c->comb_ext[d - 1].as<rr::CombExt>() : nullptr;
    for (int q = 0; q <= RR_MAX_DEPTH; ++q) A.chain[q] = q + 1 < p.levels ? c->comb[q].as<rr::ChainRec>() : nullptr;
    A.out = o.out;
    A.avg = o.avg;
    A.avg_f32 = o.avg_f32;
    A.aa_wave = (d == 0 && A.tile_fast) ? o.aa_wave : 0;
    A.pad_children = plan.pad_children ? 1 : 0;
    // null when no material is reflective or transparent (or at the last level)
    A.next = children_possible ? (d % 2 ? c->ev_b : c->ev_a).as<rr::Event>() : nullptr;
    A.pending = children_possible ? c->pend[d].as<int32_t>() : nullptr;
    A.n1n2_list = c->n1n2.as<int32_t>();
    A.lcount = lc + d * rr::LC_COUNT;
    if (plan.order.ok && d == 0) order_level0_args(c, plan, A);
    A.counters = frame_counters(c, c->epoch);
    A.counters_zero = (c->zero_next && d == 0 && base == 0) ? frame_counters(c, c->epoch ^ 1) : nullptr;
    if (base_args.views) {  // a pass of whole views: the events, the camera table and the outputs start at its first view
        const int64_t v0 = base / base_args.view_e, vsamples = base_args.hs * base_args.lrows;
        A.base = 0;
        A.views = base_args.views + v0;
        if (A.out) A.out += 3 * v0 * vsamples;
        if (A.avg) A.avg = static_cast<double*>(A.avg) + 3 * v0 * (vsamples / ((int64_t)A.aa * A.aa));
    }
    return A;
}

// The chain family's camera launch; with the deep queue (plan.spill) it appends the chains still reflecting at
// RR_DEEP_FROM to the queue's segments, and a second launch (one block per segment) finishes them.
hipError_t launch_chain_frame(rr_ctx* c, const rr::FramePlan& plan, rr::LevelArgs& A, hipStream_t st) {
    if (!plan.spill) return rr::launch_chain(c->S, A, st, kprof(c));
    A.deep = c->deep.as<rr::DeepRec>();
    A.deep_from = rr::RR_DEEP_FROM;
    A.nseg_out = (int32_t)plan.deep_nseg;
    A.seg_out_count = c->deep_count.as<unsigned int>();
    A.seg_cap_out = plan.deep_seg_cap;
    hipError_t e = rr::launch_chain(c->S, A, st, kprof(c));
    if (e != hipSuccess) return e;
    rr::LevelArgs D = A;
    D.nseg = (int32_t)plan.deep_nseg;
    D.seg_count = A.seg_out_count;
    D.seg_cap = plan.deep_seg_cap;
    D.seg_out_count = nullptr;
    D.counters_zero = nullptr;
    return rr::launch_chain(c->S, D, st, kprof(c), true);
}

// A level-0-only frame that qualifies (plan.persist_candidate) runs as one resident launch when rr::persist_plan
// agrees.  Its tile queue's heads are the C_WORK words of this frame's counter slots, which no kernel counts into:
// zero like the rest of the buffer — at rr_create, or by the first kernels of the frame before (counters_zero).  A
// frame that launches nothing (a part with no rows) zeroes nothing, and does not take the buffer either:
// end_frame_counters leaves the untouched buffer to the next frame
hipError_t launch_level0_frame(rr_ctx* c, const rr::FramePlan& plan, rr::LevelArgs& A, hipStream_t st) {
    if (!plan.persist_candidate) return rr::launch_level(c->S, A, st, kprof(c));
    A.persist_tiles = (uint32_t)(A.n / 64);
    A.persist_heads = persist_heads();
    A.persist_head = A.counters + rr::C_WORK;
    const rr::PersistPlan persist = rr::persist_plan(c->S, A, &c->persist_resident);
    if (persist.blocks <= 0) return rr::launch_level(c->S, A, st, kprof(c));
    c->persist_last = persist;
    return rr::launch_persist(c->S, A, persist, st, kprof(c));
}

hipError_t launch_family(rr_ctx* c, const rr::FramePlan& plan, rr::LevelArgs& A, hipStream_t st) {
    const bool listed = A.list != nullptr;  // the plan admits the in-wave families only
    if (A.views) {  // a batch of views: the plan admits the in-wave families only
        switch (plan.family) {
            case rr::Family::Tree:
                return rr::launch_tree_views(c->S, A, st, kprof(c));
            case rr::Family::Chain:
                return rr::launch_chain_views(c->S, A, st, kprof(c));
            case rr::Family::Level0:
                return rr::launch_level_views(c->S, A, st, kprof(c));
            default:
                return hipErrorInvalidValue;
        }
    }
    switch (plan.family) {
        case rr::Family::Tree:
            return listed ? rr::launch_tree_listed(c->S, A, st, kprof(c)) : rr::launch_tree(c->S, A, st, kprof(c));
        case rr::Family::Chain:
            return listed ? rr::launch_chain_listed(c->S, A, st, kprof(c)) : launch_chain_frame(c, plan, A, st);
        case rr::Family::Level0:
            return listed ? rr::launch_level_listed(c->S, A, st, kprof(c)) : launch_level0_frame(c, plan, A, st);
        case rr::Family::FusedLevels:
        case rr::Family::Unfused:
            break;
    }
    return rr::launch_level(c->S, A, st, kprof(c));
}

// bottom-up shade_hit sums of the events with children (scene.rs:172-177), for the unfused levels; fused levels
// finish their chains in the kernels
int combine_levels(rr_ctx* c, const rr::LevelArgs& base_args, const rr::FramePlan& plan, const rr::LevelPlan& p,
                   int64_t base, const FrameOut& o, hipStream_t st) {
    unsigned int* lc = c->lcount.as<unsigned int>();
    for (int d = p.levels - 2; d >= 0; --d) {
        rr::CombArgs C{};
        C.level = d;
        C.n = p.cap[d];
        C.n_dev = lc + d * rr::LC_COUNT + rr::LC_PENDING;
        C.base = base;
        C.pending = c->pend[d].as<int32_t>();
        C.comb = c->comb[d].as<rr::CombRec>();
        C.parent_comb = d > 0 ? c->comb[d - 1].as<rr::CombRec>() : nullptr;
        C.comb_ext = plan.ext ? c->comb_ext[d].as<rr::CombExt>() : nullptr;
        C.parent_ext = plan.ext && d > 0 ? c->comb_ext[d - 1].as<rr::CombExt>() : nullptr;
        C.out = o.out;
        C.avg = o.avg;
        C.avg_f32 = o.avg_f32;
        C.hs = base_args.hs;
        C.lrows = base_args.rays0 ? 0 : base_args.lrows;
        HIPCHK(rr::launch_combine(C, st, kprof(c)));
    }
    return RR_OK;
}

// an AA pass: the output rows of the batch [base, base + nb), averaged on the second stream after the batch
int average_pass(rr_ctx* c, const rr::FramePlan& plan, const FrameOut& o, int64_t hs, int64_t base, int64_t nb,
                 hipStream_t st) {
    const AaPasses& a = *o.aap;
    const int64_t y0 = base / hs / a.aa, y1 = (base + nb) / hs / a.aa;
    const size_t pi = (size_t)(base / plan.B);
    while (c->pass_ev.size() <= pi) {
        hipEvent_t e = nullptr;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->pass_ev.push_back(e);
    }
    HIPCHK(hipEventRecord(c->pass_ev[pi], st));
    HIPCHK(hipStreamWaitEvent(c->aa_stream, c->pass_ev[pi], 0));
    HIPCHK(launch_average(a, o.out + 3 * y0 * a.aa * hs, y0, y1 - y0, c->aa_stream, kprof(c)));
    return RR_OK;
}

}  // namespace

// Runs the wavefront levels for `total` level-0 events; level-0 rays come from the camera or from ctx->rays0
// (color_at).  Results (color_at values) land in `out` (3 doubles per event), or averaged in `avg`.  facts: the
// call's frame_facts for this max_depth.  frame_plan.hpp decides what runs; the steps below launch it.
// base0: the index of the run's first event (a multiple of 64 and rays0 only: a pass of a lens frame, whose events are
// the frame's base0 .. base0 + total — sample identity, ray and output slot — through pointers the caller biased by
// -base0 entries).
int run_levels(rr_ctx* c, const FrameFacts& facts, const rr::LevelArgs& base_args, int64_t total, int max_depth,
               double* out, hipStream_t st, void* avg, int32_t avg_f32, int32_t aa_wave, const AaPasses* aap,
               int64_t base0) {
    const FrameOut o{out, avg, avg_f32, aa_wave, aap};
    const rr::FramePlan plan = plan_run(c, facts, base_args, total, max_depth, o);
    if (plan.err != RR_OK) return fail(plan.err, plan.msg);
    int rc = grow_workspace(c, plan);
    if (rc == RR_OK && plan.order.ok) rc = refresh_order(c, base_args, plan, !facts.sw.no_tile_guess, st);
    if (rc != RR_OK) return rc;
    if (base0 != 0 && (!base_args.rays0 || base0 % 64 != 0 || aap)) return fail(RR_E_ARG, "internal: a starting base needs explicit rays and whole waves");
    // an ordered batch whose live count is on the device (the indirect frames' live list): the kernels compare the count
    // with the launch's own slots, so the list is one batch from slot 0
    if (base_args.rays0 && base_args.list && base_args.n_dev && (plan.B < total || base0 != 0))
        return fail(RR_E_ARG, "internal: a device-counted ordered batch is one batch");
    for (int64_t off = 0; off < total; off += plan.B) {
        const int64_t base = base0 + off, nb = std::min(plan.B, total - off);
        rr::LevelPlan short_batch;
        if (nb != plan.B) short_batch = rr::plan_levels(nb, plan.k, plan.plan_depth, plan.ext, plan.fused);
        const rr::LevelPlan& p = nb != plan.B ? short_batch : plan.P;
        // the queue counters are zeroed once per batch (appends, pending, n1/n2 lists): no memset in the frames of
        // the in-wave chains and trees, which use none (it cost a C1 frame 9.6 us as two fills)
        if (plan.zero_lcount)
            HIPCHK(hipMemsetAsync(c->lcount.p, 0, (size_t)p.levels * rr::LC_COUNT * sizeof(unsigned int), st));
        if (plan.spill) HIPCHK(hipMemsetAsync(c->deep_count.p, 0, (size_t)plan.deep_nseg * sizeof(unsigned int), st));
        for (int d = 0; d < p.levels; ++d) {
            rr::LevelArgs A = level_args(c, base_args, plan, p, base, d, max_depth, o);
            if (aa_wave && !A.aa_wave) return fail(RR_E_ARG, "internal: in-wave AA average without full tiles");
            HIPCHK(launch_family(c, plan, A, st));
            if (A.counters_zero) c->next_zeroed = true;  // the launch above clears the next frame's buffer
            if (plan.order.ok && d == 0 && (rc = age_order(c, plan, st)) != RR_OK) return rc;
        }
        if (plan.family == rr::Family::Unfused) rc = combine_levels(c, base_args, plan, p, base, o, st);
        if (rc == RR_OK && plan.passes) rc = average_pass(c, plan, o, base_args.hs, off, nb, st);
        if (rc != RR_OK) return rc;
    }
    if (plan.passes) {  // the caller's stream continues after the last pass's average
        HIPCHK(hipEventRecord(c->aa_done, c->aa_stream));
        HIPCHK(hipStreamWaitEvent(st, c->aa_done, 0));
    } else if (aap) {  // one pass: the average follows on the caller's stream
        HIPCHK(launch_average(*aap, out, 0, total / base_args.hs / aap->aa, st, kprof(c)));
    }
    return RR_OK;
}

void collect_stats(rr_ctx* c, rr_stats* s) {
    std::memset(s, 0, sizeof(*s));
    unsigned long long h[rr::RR_CNT_STRIDE] = {};
    for (int sl = 0; sl < rr::RR_CNT_SLOTS; ++sl)
        for (int k = 0; k < rr::C_COUNT; ++k) h[k] += c->h_counters[sl * rr::RR_CNT_STRIDE + k];
    s->rays = h[rr::C_RAYS];
    s->shadow_rays = h[rr::C_SHADOW];
    s->shade_events = h[rr::C_SHADE];
    s->n1n2_scans = h[rr::C_N1N2];
    s->group_tests = h[rr::C_GROUP_TESTS];
    s->group_hits = h[rr::C_GROUP_HITS];
    s->samples = h[rr::C_SAMPLES];
    s->prim_tests = h[rr::C_PRIM_TESTS];
    for (int k = 0; k < 3; ++k) {
        s->exact_flops[k] = h[rr::C_FLOPS_TRACE + k];
        s->wave_visits[k] = h[rr::C_VISITS_TRACE + k];
    }
    s->nan_rays = h[rr::C_NAN];
}
int nan_fail(uint64_t n) {
    return fail(RR_E_NAN, std::to_string(n) +
                              " ray(s) met a NaN intersection t in a list of >= 2 entries: the reference panics in "
                              "Vec::sort_by(partial_cmp().unwrap()) (scene.rs:104)");
}

static int resolve_prof(rr_ctx* c) {
    for (auto& m : c->prof.marks) {
        HIPCHK(hipEventSynchronize(m.second.second));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, m.second.first, m.second.second));
        c->kms[m.first] += ms;
        c->kcount[m.first] += 1;
    }
    c->prof.marks.clear();
    c->prof.used = 0;
    return RR_OK;
}

static int finish_stats(rr_ctx* c) {
    if (!c->stats_pending) return RR_OK;
    float ms = 0.f;
    if (c->frame_timed) {
        HIPCHK(hipEventSynchronize(c->e1));
        HIPCHK(hipEventElapsedTime(&ms, c->e0, c->e1));
    } else {
        HIPCHK(sync_ctx(c));
    }
    // the counters of the last render stay in HBM until the next one zeroes them: copy on demand
    // (a per-frame device-to-host copy behind a cross-stream wait blocks the host in HIP)
    HIPCHK(hipMemcpy(c->h_counters, c->stats_src ? c->stats_src : frame_counters(c, c->epoch), kCounterBytes,
                     hipMemcpyDeviceToHost));
    collect_stats(c, &c->last);
    c->last.kernel_ms = ms;
    c->stats_pending = false;
    return RR_OK;
}

}  // namespace rr::api
#pragma GCC visibility pop

namespace rr {
// Every check rr_render_device makes before it enqueues anything (the multi-device group validates all
// of its parts with it first, so a bad argument never leaves peers waiting in a collective).
int render_validate(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o) {
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return fail(RR_E_ARG, "multi-device context: use rr_render_gather_device or rr_render");
    if (!c->has_scene) return fail(RR_E_ARG, "no scene uploaded");
    int rc = check_opts(cam, o);
    if (rc != RR_OK) return rc;
    const int64_t rows = opts_rows(o, cam->vsize / o->aa);
    if (rows * o->aa * cam->hsize >= ((int64_t)1 << 31))
        return fail(RR_E_LIMIT, "a part must hold fewer than 2^31 samples (use more parts)");
    return RR_OK;
}
}  // namespace rr

extern "C" {

int32_t rr_abi_version(void) { return RR_ABI_VERSION; }
const char* rr_last_error(void) { return g_err.c_str(); }

int rr_device_count(int* out) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    if (out) *out = n;
    return e == hipSuccess ? RR_OK : fail(RR_E_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
}

int rr_create(int device, rr_ctx** out) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!out) return fail(RR_E_ARG, "null out");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(RR_E_HIP, "no HIP device available");
    if (device < 0 || device >= n) return fail(RR_E_ARG, "device index out of range");
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(RR_E_HIP, std::string("device is ") + prop.gcnArchName + ", this build targets gfx950 only");
    rr_ctx* c = new rr_ctx();
    c->device = device;
    if (const char* b = std::getenv("RRAY_BATCH")) c->batch = std::max<int64_t>(1024, std::atoll(b));
    if (const char* b = std::getenv("RRAY_LENS_PASS")) c->lens_pass = std::max<int64_t>(0, std::atoll(b));
    if (const char* b = std::getenv("RRAY_AO_PASS")) c->ao_pass = std::max<int64_t>(0, std::atoll(b));
    if (const char* b = std::getenv("RRAY_INDIRECT_PASS")) c->indirect_pass = std::max<int64_t>(0, std::atoll(b));
    if (const char* b = std::getenv("RRAY_DENOISE_LDS"))
        c->dn_lds_step = (int32_t)std::min<long long>(rr::RR_DN_LDS_MAX_STEP, std::max<long long>(0, std::atoll(b)));
    if (const char* b = std::getenv("RRAY_TEMPORAL_ROWS")) c->tp_rows = std::atoll(b) != 0 ? 1 : 0;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) c->queue_budget = free_b / 2;
    if (const char* q = std::getenv("RRAY_QUEUE_BUDGET_MB")) c->queue_budget = (size_t)std::max(1ll, std::atoll(q)) << 20;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&c->e0);
    if (e == hipSuccess) e = hipEventCreate(&c->e1);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_out, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->aa_done, hipEventDisableTiming);
    if (e == hipSuccess)
        e = hipHostMalloc((void**)&c->h_counters, kCounterBytes, hipHostMallocDefault);
    if (e == hipSuccess) e = c->counters.ensure(3 * kCounterBytes);
    if (e == hipSuccess) e = hipMemset(c->counters.p, 0, 3 * kCounterBytes);
    if (e == hipSuccess) e = c->lcount.ensure((RR_MAX_DEPTH + 1) * rr::LC_COUNT * sizeof(unsigned int));
    if (e != hipSuccess) {
        rr_destroy(c);
        return fail(RR_E_HIP, std::string("context setup: ") + hipGetErrorString(e));
    }
    *out = c;
    return RR_OK;
}

int rr_create_multi(int n, const int* device_ids, rr_ctx** out) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!out) return fail(RR_E_ARG, "null out");
    *out = nullptr;
    rr_group* g = nullptr;
    int rc = rr::group_create_local(n, device_ids, &g);
    if (rc != RR_OK) return rc;
    rr_ctx* c = new rr_ctx();
    c->group = g;
    *out = c;
    return RR_OK;
}

int rr_create_rank(int device, int nranks, int rank, const uint8_t* unique_id, rr_ctx** out) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!out) return fail(RR_E_ARG, "null out");
    *out = nullptr;
    rr_group* g = nullptr;
    int rc = rr::group_create_rank(device, nranks, rank, unique_id, &g);
    if (rc != RR_OK) return rc;
    rr_ctx* c = new rr_ctx();
    c->group = g;
    *out = c;
    return RR_OK;
}

int rr_context_info(const rr_ctx* c, int32_t* nranks, int32_t* rank, int32_t* ndevices) {
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return rr::group_info(c->group, nranks, rank, ndevices);
    if (nranks) *nranks = 1;
    if (rank) *rank = 0;
    if (ndevices) *ndevices = 1;
    return RR_OK;
}

void rr_destroy(rr_ctx* c) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!c) return;
    if (c->group) {
        rr::group_destroy(c->group);
        delete c;
        return;
    }
    (void)hipSetDevice(c->device);
    rr::trace("rr_destroy %p: synchronise", (void*)c);
    if (c->stream) (void)sync_ctx(c);
    rr::trace("rr_destroy %p: free", (void*)c);
    for (DBuf* b : {&c->culls, &c->inner, &c->chunks, &c->nodes, &c->groups, &c->shapes, &c->tris, &c->mats, &c->pats, &c->lights, &c->textures, &c->texels, &c->counters,
                    &c->lcount, &c->hit, &c->n12, &c->n1n2, &c->ev_a, &c->ev_b, &c->canvas, &c->rays0, &c->qout, &c->tiles,
                    &c->tile_cost, &c->tile_perm, &c->tile_hist, &c->deep, &c->deep_count, &c->node_object, &c->hitrec, &c->aov,
                    &c->adapt_flags, &c->adapt_blocks, &c->adapt_counts, &c->adapt_list, &c->adapt_mask, &c->views,
                    &c->shadow_sink, &c->order_scratch, &c->order_perm, &c->lens_rays, &c->lens_rgb,
                    &c->ao_count, &c->ao_rays, &c->ind_rays, &c->ind_rgb, &c->ind_cam, &c->ind_list, &c->ind_counts, &c->dn_guides, &c->dn_img[0], &c->dn_img[1], &c->dn_host, &c->dv_var[0], &c->dv_var[1],
                    &c->tp_host})
        b->release();
    for (auto& b : c->comb) b.release();
    for (auto& b : c->comb_ext) b.release();
    for (auto& b : c->pend) b.release();
    for (hipEvent_t e : c->prof.pool) (void)hipEventDestroy(e);
    if (c->h_counters) (void)hipHostFree(c->h_counters);
    if (c->e0) (void)hipEventDestroy(c->e0);
    if (c->e1) (void)hipEventDestroy(c->e1);
    if (c->ev_in) (void)hipEventDestroy(c->ev_in);
    if (c->ev_out) (void)hipEventDestroy(c->ev_out);
    if (c->aa_done) (void)hipEventDestroy(c->aa_done);
    for (hipEvent_t e : c->pass_ev) (void)hipEventDestroy(e);
    if (c->aa_stream) (void)hipStreamDestroy(c->aa_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    rr::trace("rr_destroy %p: done", (void*)c);
    delete c;
}

int rr_scene_upload(rr_ctx* c, const rr_scene_desc* d) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!c || !d) return fail(RR_E_ARG, "null context/descriptor");
    if (c->group) return rr::group_upload(c->group, d);
    std::string err;
    rr::HostScene hs;
    int rc = rr::flatten_scene(*d, hs, err);
    if (rc != RR_OK) return fail(rc, err);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_ctx(c));  // renders in flight may still read the previous scene
    hipStream_t st = c->stream;
    HIPCHK(upload(c->culls, hs.culls, st));
    HIPCHK(upload(c->inner, hs.inner, st));
    HIPCHK(upload(c->chunks, hs.chunks, st));
    {  // the node records, then the planes' normals (rr_device.hpp DevScene.nodes)
        const size_t nb = hs.nodes.size() * sizeof(rr::DevNode), fb = hs.flat_normal.size() * sizeof(double);
        HIPCHK(c->nodes.ensure(std::max<size_t>(nb + fb, 16)));
        if (nb) HIPCHK(hipMemcpyAsync(c->nodes.p, hs.nodes.data(), nb, hipMemcpyHostToDevice, st));
        if (fb) HIPCHK(hipMemcpyAsync((char*)c->nodes.p + nb, hs.flat_normal.data(), fb, hipMemcpyHostToDevice, st));
    }
    HIPCHK(upload(c->groups, hs.groups, st));
    HIPCHK(upload(c->shapes, hs.shapes, st));
    HIPCHK(upload(c->tris, hs.tris, st));
    HIPCHK(upload(c->mats, hs.mats, st));
    HIPCHK(upload(c->pats, hs.pats, st));
    HIPCHK(upload(c->lights, hs.lights, st));
    HIPCHK(upload(c->textures, hs.textures, st));
    HIPCHK(upload(c->texels, hs.texels, st));
    std::vector<int32_t> node_object(hs.nodes.size(), -1);  // the ids hit_kernel reports (Intersection.object)
    for (size_t i = 0; i < hs.node_of_object.size(); ++i)
        if (hs.node_of_object[i] >= 0 && (size_t)hs.node_of_object[i] < node_object.size())
            node_object[hs.node_of_object[i]] = (int32_t)i;
    HIPCHK(upload(c->node_object, node_object, st));
    HIPCHK(hipStreamSynchronize(st));
    c->host = std::move(hs);
    // the level-0 tile order is the previous scene's tile costs: drop it (the next frame records new ones).
    // The tile bundles depend on the camera only; they are rebuilt too, for a clean start
    c->order_valid = false;
    c->order_age = 0;
    c->tiles_valid = false;
    c->persist_resident = -1;  // the resident launch's LDS follows the scene's lights
    rr::DevScene& S = c->S;
    S.culls = c->culls.as<rr::DevCull>();
    S.inner = c->inner.as<rr::DevCull>();
    S.chunks = c->chunks.as<rr::DevChunk>();
    S.n_chunks = (int32_t)c->host.chunks.size();
    S.n_free = 0;
    for (int k = S.n_chunks - 1; k >= 0; --k) {  // lone unbounded top-level leaves at the end of the order
        const rr::DevChunk& ch = c->host.chunks[k];
        const rr::DevNode& nd = c->host.nodes[ch.start];
        if (ch.count != 1 || ch.cull.r < HUGE_VALF || nd.parent != -1 || rr::is_container(nd.kind) ||
            ch.start != (int32_t)c->host.nodes.size() - 1 - S.n_free)
            break;
        ++S.n_free;
    }
    S.free_planes = 1;
    for (int k = 0; k < S.n_free; ++k) {
        const rr::DevNode& nd = c->host.nodes[c->host.nodes.size() - 1 - k];
        if (nd.kind != RR_PLANE || !(nd.flags & rr::NF_IDENT)) S.free_planes = 0;
    }
    S.nodes = c->nodes.as<rr::DevNode>();
    S.groups = c->groups.as<rr::DevGroup>();
    S.shapes = c->shapes.as<rr::DevShape>();
    S.tris = c->tris.as<rr::DevTri>();
    S.mats = c->mats.as<rr::DevMaterial>();
    S.pats = c->pats.as<rr::DevPattern>();
    S.lights = c->lights.as<rr::DevLight>();
    S.textures = c->textures.as<rr::DevTexture>();
    S.texels = c->texels.as<uint32_t>();
    S.n_nodes = (int32_t)c->host.nodes.size();
    S.n_lights = (int32_t)c->host.lights.size();
    S.has_transparent = c->host.has_transparent;
    S.has_area = 0;
    for (const rr::DevLight& l : c->host.lights) S.has_area |= l.kind == RR_LIGHT_AREA ? 1 : 0;
    S.complex_patterns = c->host.complex_patterns;
    S.tri_inline = c->host.tri_inline;
    S.has_groups = c->host.groups.empty() ? 0 : 1;
    S.general = (c->host.has_csg || c->host.has_quad) ? 1 : 0;
    const size_t lds_bytes = (size_t)S.n_nodes * sizeof(rr::DevCull) + (size_t)S.n_chunks * sizeof(rr::DevChunk);
    S.lds_culls = (lds_bytes <= (size_t)rr::RR_LDS_CULL_BYTES && !std::getenv("RRAY_GLOBAL_CULLS")) ? 1 : 0;
    // sphere around the bounded nodes' culls (make_bundle moves far ray origins next to it)
    {
        double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
        bool any = false;
        for (const rr::DevCull& cl : c->host.culls) {
            if (!(cl.r < HUGE_VALF)) continue;
            any = true;
            for (int k = 0; k < 3; ++k) {
                lo[k] = std::min(lo[k], (double)cl.c[k] - cl.r);
                hi[k] = std::max(hi[k], (double)cl.c[k] + cl.r);
            }
        }
        S.bs_r = -1.0f;
        if (any && std::isfinite(hi[0] - lo[0]) && std::isfinite(hi[1] - lo[1]) && std::isfinite(hi[2] - lo[2])) {
            double r = 0.0;
            for (int k = 0; k < 3; ++k) S.bs_c[k] = (float)(0.5 * (lo[k] + hi[k]));
            for (const rr::DevCull& cl : c->host.culls) {
                if (!(cl.r < HUGE_VALF)) continue;
                const double dx = cl.c[0] - S.bs_c[0], dy = cl.c[1] - S.bs_c[1], dz = cl.c[2] - S.bs_c[2];
                r = std::max(r, std::sqrt(dx * dx + dy * dy + dz * dz) + cl.r);
            }
            if (r < 1e30) S.bs_r = (float)r;
        }
    }
    c->has_scene = true;
    return RR_OK;
}

int rr_scene_inspect(const rr_scene_desc* d, double* inverses, double* group_aabbs, int32_t* node_of_object) {
    if (!d) return fail(RR_E_ARG, "null descriptor");
    std::string err;
    rr::HostScene hs;
    int rc = rr::flatten_scene(*d, hs, err);
    if (rc != RR_OK) return fail(rc, err);
    for (int i = 0; i < d->n_objects; ++i) {
        int node = hs.node_of_object[i];
        if (node_of_object) node_of_object[i] = node;
        if (inverses) {
            double* o = inverses + 16 * (size_t)i;
            if (node >= 0 && (hs.nodes[node].flags & rr::NF_TRI_INLINE)) {  // identity (slots hold p1/e1/e2)
                for (int k = 0; k < 12; ++k) o[k] = (k % 5 == 0) ? 1.0 : 0.0;
            } else if (node >= 0) {
                for (int k = 0; k < 12; ++k) o[k] = hs.nodes[node].inv[k];
            } else {
                for (int k = 0; k < 12; ++k) o[k] = 0.0;
            }
            o[12] = 0.0;
            o[13] = 0.0;
            o[14] = 0.0;
            o[15] = 1.0;
        }
        if (group_aabbs) {
            double* o = group_aabbs + 6 * (size_t)i;
            for (int k = 0; k < 6; ++k) o[k] = 0.0;
            if (node >= 0 && rr::is_container(hs.nodes[node].kind))
                for (int k = 0; k < 6; ++k) o[k] = hs.groups[hs.nodes[node].aux].aabb[k];
        }
    }
    return RR_OK;
}

int rr_camera_new(int64_t hsize, int64_t vsize, double fov, const double transform[16], rr_camera* out) {
    if (!out || hsize <= 0 || vsize <= 0) return fail(RR_E_ARG, "bad camera size");
    double half_view = std::tan(fov / 2.0);  // camera.rs:41-63
    double aspect = (double)hsize / (double)vsize;
    double hw, hh;
    if (aspect >= 1.0) {
        hw = half_view;
        hh = half_view / aspect;
    } else {
        hw = half_view * aspect;
        hh = half_view;
    }
    out->hsize = hsize;
    out->vsize = vsize;
    out->field_of_view = fov;
    out->half_width = hw;
    out->half_height = hh;
    out->pixel_size = (hw * 2.0) / (double)hsize;
    rr::M4 id = rr::identity();
    for (int i = 0; i < 16; ++i) out->transform[i] = transform ? transform[i] : id.m[i];
    return RR_OK;
}

int64_t rr_part_rows(int64_t height, int32_t part, int32_t nparts, int32_t block, int64_t* rows_out) {
    if (nparts < 1 || part < 0 || part >= nparts || block < 1 || height < 0) return fail(RR_E_ARG, "bad partition");
    const int64_t n = rr::part_rows_count(height, part, nparts, block);
    if (rows_out) {
        int64_t k = 0;
        for (int64_t b0 = (int64_t)part * block; b0 < height; b0 += (int64_t)nparts * block)
            for (int64_t y = b0; y < std::min<int64_t>(b0 + block, height); ++y) rows_out[k++] = y;
    }
    return n;
}

int64_t rr_stage_row_offset(int64_t height, int32_t part, int32_t nparts, int32_t block) {
    if (height < 0 || nparts < 1 || block < 1 || part < 0 || part > nparts)
        return fail(RR_E_ARG, "rr_stage_row_offset: bad arguments");
    return rr::stage_row_offset(height, part, nparts, block);
}

int rr_unshuffle_host(const double* staged, double* frame, int64_t width, int64_t height, int32_t nparts,
                      int32_t block) {
    if (!staged || !frame || width < 0 || height < 0 || nparts < 1 || block < 1)
        return fail(RR_E_ARG, "rr_unshuffle_host: bad arguments");
    const int64_t row = width * 3;
    for (int32_t p = 0; p < nparts; ++p) {  // the runs place_tile_kernel moves on rank 0 (partition.hpp)
        const double* tile = staged + rr::stage_row_offset(height, p, nparts, block) * row;
        rr::for_each_part_run(height, p, nparts, block, [&](int64_t j, int64_t y, int64_t n) {
            std::memcpy(frame + y * row, tile + j * row, (size_t)(n * row) * sizeof(double));
        });
    }
    return RR_OK;
}

int rr_create_virtual(int device, int nparts, rr_ctx** out) {
    rr::DeviceGuard device_guard;
    if (!out) return fail(RR_E_ARG, "null out");
    *out = nullptr;
    rr_group* g = nullptr;
    int rc = rr::group_create_virtual(device, nparts, &g);
    if (rc != RR_OK) return rc;
    rr_ctx* c = new rr_ctx();
    c->group = g;
    *out = c;
    return RR_OK;
}

int rr_render_device(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, void* d_canvas, void* d_avg,
                     void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = rr::render_validate(c, cam, o);
    if (rc != RR_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    int32_t block = o->block_rows > 0 ? o->block_rows : 8;
    const int64_t H = cam->vsize / o->aa, W = cam->hsize / o->aa;
    const int64_t rows = opts_rows(o, H);
    const int64_t local_rows = rows * o->aa;
    // a band [row_begin, row_end) is part row_begin / block of nparts = 1: the kernels' row arithmetic
    // (bi * nparts + part) * block + kb is then row_begin + the local row, with a block that divides row_begin (8
    // rows, else 2 — pixel waves need an even block — else 1)
    int32_t part = o->part;
    if (o->row_begin != 0 || o->row_end != 0) {
        if (o->row_begin % block != 0) block = o->row_begin % 2 == 0 ? 2 : 1;
        part = o->row_begin / block;
    }
    const int64_t total = local_rows * cam->hsize;
    // Everything is enqueued on the caller's stream (no cross-stream events per call: a HIP event
    // handoff between streams costs host time every frame).  The context's workspace is reused, so
    // a render on a different stream than the previous one first waits for that one.
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    // aa == 1, the level-0 waves' own average or pixel waves (rr::plan_output): the average is written by the
    // kernels directly; the canvas only when asked for
    const FrameFacts facts = frame_facts(c, o->max_depth);
    const rr::OutputPlan mode = rr::plan_output(facts.traits, facts.sw, d_avg != nullptr, o->aa, cam->hsize, local_rows,
                                                o->max_depth, block, c->batch);
    double* canvas = static_cast<double*>(d_canvas);
    if (!canvas && !mode.direct_avg) {
        HIPCHK(c->canvas.ensure(std::max<int64_t>(total, 1) * 3 * sizeof(double)));
        canvas = c->canvas.as<double>();
    }
    HIPCHK(st.start_timer(!(o->flags & RR_NO_FRAME_TIMING)));
    rr::LevelArgs A = camera_args(cam, o, o->aa, part, block);
    A.lrows = local_rows;
    if (mode.pw) {
        A.pw = 1;
        A.pw_rows = (int32_t)rows;
        A.pw_wpb = mode.pw_wpb;
    }
    const int32_t f32 = (o->flags & RR_OUT_AVG_F32) ? 1 : 0;
    rc = tile_bundles(c, A, st, &A.tile_bundles);
    if (rc != RR_OK) return rc;
    begin_frame_counters(c);
    const AaPasses aap{d_avg, f32, W, o->aa};
    rc = run_levels(c, facts, A, total, o->max_depth, canvas, st, mode.direct_avg ? d_avg : nullptr, f32,
                    mode.wave_avg ? o->aa : 0, (d_avg && !mode.direct_avg) ? &aap : nullptr);
    c->zero_next = false;
    if (rc != RR_OK) return rc;
    end_frame_counters(c);
    HIPCHK(st.close());
    c->stats_pending = true;
    // C_SAMPLES is not incremented by the wavefront kernels; it is the level-0 event count
    c->last.samples = (uint64_t)total;
    c->adapt_pending = false;
    return RR_OK;
}

int rr_render_gather_device(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, void* d_frame, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return rr::group_render_gather(c->group, cam, o, d_frame, hip_stream);
    if (o && (o->nparts != 1 || o->part != 0)) return fail(RR_E_ARG, "rr_render_gather_device renders the whole frame");
    if (o && (o->flags & (RR_OUT_CANVAS | RR_OUT_AVG_F32)))
        return fail(RR_E_ARG, "rr_render_gather_device writes the f64 AA-averaged image only");
    if (!d_frame) return fail(RR_E_ARG, "null frame buffer");
    return rr_render_device(c, cam, o, nullptr, d_frame, hip_stream);
}

int rr_kernel_profile(rr_ctx* c, int enable) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return rr::group_kernel_profile(c->group, enable);
    HIPCHK(sync_ctx(c));
    int rc = resolve_prof(c);
    if (rc != RR_OK) return rc;
    c->profile = enable != 0;
    for (int k = 0; k < rr::K_COUNT; ++k) {
        c->kms[k] = 0.0;
        c->kcount[k] = 0;
    }
    return RR_OK;
}

int rr_kernel_times(rr_ctx* c, double* ms, uint64_t* launches, int32_t n) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return rr::group_kernel_times(c->group, ms, launches, n);
    HIPCHK(sync_ctx(c));
    int rc = resolve_prof(c);
    if (rc != RR_OK) return rc;
    for (int k = 0; k < n && k < rr::K_COUNT; ++k) {
        if (ms) ms[k] = c->kms[k];
        if (launches) launches[k] = c->kcount[k];
    }
    return rr::K_COUNT;
}

int rr_resident_launch(rr_ctx* c, int32_t* blocks, int32_t* heads) {
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return fail(RR_E_ARG, "multi-device context: ask a single-device context");
    if (blocks) *blocks = c->persist_last.blocks;
    if (heads) *heads = (int32_t)c->persist_last.heads;
    return RR_OK;
}

int rr_last_stats(rr_ctx* c, rr_stats* s) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!c || !s) return fail(RR_E_ARG, "null argument");
    if (c->group) return rr::group_last_stats(c->group, s);
    uint64_t samples = c->last.samples;
    int rc = finish_stats(c);
    if (rc != RR_OK) return rc;
    if (c->adapt_pending) {  // an adaptive frame (finished by now): + the refine pass's samples, counted on the device
        uint32_t events = 0;
        HIPCHK(hipMemcpy(&events, c->adapt_counts.as<uint32_t>() + 1, sizeof events, hipMemcpyDeviceToHost));
        samples += events;
        c->adapt_pending = false;
    }
    c->last.samples = samples;
    *s = c->last;
    return RR_OK;
}

int rr_render(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, double* out_canvas, double* out_avg,
              rr_stats* stats) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return rr::group_render(c->group, cam, o, out_canvas, out_avg, stats);
    int rc = check_opts(cam, o);
    if (rc != RR_OK) return rc;
    const int64_t H = cam->vsize / o->aa, W = cam->hsize / o->aa;
    const int64_t rows = opts_rows(o, H);
    const int64_t total = rows * o->aa * cam->hsize;
    HIPCHK(hipSetDevice(c->device));
    const bool want_avg = (o->flags & RR_OUT_AVG) && out_avg;
    HIPCHK(c->qout.ensure(std::max<int64_t>(W * rows, 1) * 3 * sizeof(double)));
    const bool want_canvas = (o->flags & RR_OUT_CANVAS) && out_canvas;
    if (want_canvas) HIPCHK(c->canvas.ensure(std::max<int64_t>(total, 1) * 3 * sizeof(double)));
    rc = rr_render_device(c, cam, o, want_canvas ? c->canvas.p : nullptr, want_avg ? c->qout.p : nullptr, nullptr);
    if (rc != RR_OK) return rc;
    if (want_canvas)
        HIPCHK(hipMemcpyAsync(out_canvas, c->canvas.p, total * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (want_avg)
        HIPCHK(hipMemcpyAsync(out_avg, c->qout.p, W * rows * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return finish_host_frame(c, stats);
}

}  // extern "C"

// ---- ABI 10: cost-balanced bands (multi.cpp) ----
extern "C" int rr_balance_bands(const double* row_cost, int64_t height, int32_t nparts, double root_extra, int32_t align,
                                int64_t* bounds) {
    if (!row_cost || !bounds || height < 1 || nparts < 1 || align < 1)
        return fail(RR_E_ARG, "rr_balance_bands: need row costs, height >= 1, nparts >= 1, align >= 1");
    rr::balance_bands(row_cost, height, nparts, root_extra, align, bounds);
    return RR_OK;
}

extern "C" int rr_group_bands(rr_ctx* c, int64_t* bounds, int32_t n) {
    if (!c || !bounds) return fail(RR_E_ARG, "null argument");
    if (!c->group) return fail(RR_E_ARG, "rr_group_bands: not a multi-device context");
    return rr::group_bands(c->group, bounds, n);
}

extern "C" int rr_group_set_bands(rr_ctx* c, const int64_t* bounds, int32_t n) {
    if (!c || !bounds) return fail(RR_E_ARG, "null argument");
    if (!c->group) return fail(RR_E_ARG, "rr_group_set_bands: not a multi-device context");
    return rr::group_set_bands(c->group, bounds, n);
}
