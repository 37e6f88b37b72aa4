// api.cpp — the C ABI of include/rray/rray.h: device context, scene upload, the wavefront level
// loop that replaces Camera::render (camera.rs:107-121), and the batch query entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include <unistd.h>

#include "../../include/rray/rray.h"
#include "device_guard.hpp"
#include "flatten.hpp"
#include "ao_dir.hpp"
#include "denoise_tap.hpp"
#include "denoise_var_tap.hpp"
#include "temporal_tap.hpp"
#include "frame_plan.hpp"
#include "kernels.hpp"
#include "multi.hpp"
#include "partition.hpp"
#include "trace.hpp"
#include "rr_math.hpp"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIPCHK(expr)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(RR_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

// grow-only device buffer
struct DBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t want) {
        if (want <= bytes) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        size_t cap = std::max(want, (size_t)256);
        hipError_t e = hipMalloc(&p, cap);
        if (e == hipSuccess) bytes = cap;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

}  // namespace

void rr_set_error(const char* msg) { g_err = msg ? msg : ""; }

struct rr_ctx {
    rr_group* group = nullptr;  // multi-device context (multi.cpp): everything below is unused
    int device = 0;
    hipStream_t stream = nullptr;
    bool has_scene = false;
    rr::HostScene host;
    rr::DevScene S{};
    DBuf culls, inner, chunks, nodes, groups, shapes, tris, mats, pats, lights, textures, texels;
    // workspace
    DBuf counters, lcount, hit, n12, n1n2, ev_a, ev_b, canvas, rays0, qout;
    DBuf deep, deep_count;  // chain kernels' deep queue (rr::DeepRec segments) and its segment counters
    // first-hit queries (hit_kernel): node index -> rr_scene_desc object id (flatten's node_of_object inverted, built
    // at upload), and rr_hit_at's result planes
    DBuf node_object, hitrec, aov;  // aov: rr_render_aov's device planes
    // rr_is_shadowed_device's walk counters: a sink nobody reads, so that the query leaves pending stats (which may be
    // the query buffer's) as they are
    DBuf shadow_sink;
    // ordered ray batches (rr_ray_order_device, rr_*_at_device_ordered): the sort's scratch (rr::ray_order_scratch_bytes)
    // and the order of a call that brings none (d_perm == NULL); grow on demand, freed with the context
    DBuf order_scratch, order_perm;
    // lens frames (rr_render_lens_device): one pass's rays (48 bytes each) and colours (24), grown on demand; the pass
    // size RRAY_LENS_PASS asks for in pixels (0: rr::plan_lens_passes' default), read at context creation
    DBuf lens_rays, lens_rgb;
    int64_t lens_pass = 0;
    // ambient occlusion (rr_ao_at_device, rr_render_ao_device): the per-point counts of occluded pairs (4 bytes per
    // point of a batch or a pass) and one pass's camera rays (48 bytes each; its first hits go to hitrec), grown on
    // demand; the pass size RRAY_AO_PASS asks for in points (0: rr::plan_ao_passes' default), read at context creation
    DBuf ao_count, ao_rays;
    int64_t ao_pass = 0;
    // one-bounce indirect light (rr_indirect_at_device, rr_render_indirect_device): one pass's gathered rays (48 bytes
    // each) and colours (24); for the frames also the pass's camera rays (48 bytes per point; its first hits go to
    // hitrec), the live list (4 bytes per ray) and the compaction's counts (one per 256 rays, then the live count and
    // one per trace chunk); grown on demand.  The pass size RRAY_INDIRECT_PASS asks for in points (0:
    // rr::plan_indirect_passes' default), read at context creation
    DBuf ind_rays, ind_rgb, ind_cam, ind_list, ind_counts;
    int64_t indirect_pass = 0;
    // the denoiser (rr_denoise_device): the guide records (32 bytes per pixel) and the two images the levels ping-pong
    // between (8 * channels bytes per pixel each; none for one iteration), grown on demand; dn_host: the device copies
    // of rr_denoise's host buffers
    DBuf dn_guides, dn_img[2], dn_host;
    // variance-guided denoising (rr_denoise_var_device): the two variance planes the levels ping-pong between beside
    // dn_img (8 bytes per pixel each; none for one iteration), grown on demand.  rr_variance_device needs dn_guides only
    DBuf dv_var[2];
    // levels with holes of at most this many pixels run the LDS-tiled kernel, the wider ones the direct kernel.  -1: the
    // measured choice (DESIGN.md §3.22's A/B): 2 for one channel, 1 for three.  RRAY_DENOISE_LDS=<0..2> overrides (0: every
    // level direct), read at context creation
    int32_t dn_lds_step = -1;
    // temporal accumulation (rr_temporal_device needs no scratch): tp_host holds the device copies of rr_temporal's host
    // buffers.  tp_rows: the kernel's lane map, 0 the 32 x 8 tile, 1 row-major (DESIGN.md §3.24's A/B);
    // RRAY_TEMPORAL_ROWS=<0|1> overrides the default, read at context creation
    DBuf tp_host;
    int32_t tp_rows = 0;
    // adaptive frames (rr_render_adaptive_device): per-pixel flags, per-block counts / offsets, the totals
    // {refined pixels, refine-pass events} and the list of refined pixels; the refine pass's samples go to `canvas`
    DBuf adapt_flags, adapt_blocks, adapt_counts, adapt_list, adapt_mask;
    // batches of views (rr_render_views_device): the camera table on the device, and the host copy it is filled from
    // (the caller's array is read before the call returns)
    DBuf views;
    std::vector<rr::DevView> views_host;
    // per-tile camera-ray bundles of the last camera / part layout (tile_bundle_kernel), reused while they match
    DBuf tiles;
    struct TileKey {
        rr::DevCamera cam;
        int64_t hs, lrows;
        int32_t aa, part, nparts, block_rows;
        int32_t pw, pad;
    } tile_key{};
    bool tiles_valid = false;
    // level-0 launch order of one-batch fused frames: every wave stores its tile's cost (clock cycles) and the
    // tiles are re-sorted costliest-first on the first frame of a part layout and every kRR_ORDER_EVERY frames
    DBuf tile_cost, tile_perm, tile_hist;
    int64_t order_tiles = 0;  // the layout the order was built for (tiles; key below)
    TileKey order_key{};
    bool order_valid = false;
    uint32_t perm_tail[3] = {0, 0, 0};  // the order's entries past the last tile (their own indices), copied from here
    int order_age = 0;
    std::vector<DBuf> comb, comb_ext, pend;  // one per level (comb_ext: scenes with transparency)
    unsigned long long* h_counters = nullptr;
    // counters: [frame buffer 0][frame buffer 1][queries]; frames alternate (`epoch`), and each
    // frame's first kernels zero the other buffer for the next frame
    int epoch = 0;
    bool zero_next = false;
    bool next_zeroed = false;  // a launch of the running frame took the other buffer to zero (end_frame_counters)
    // the persistent level-0 loop (rr::persist_plan): the blocks the GPU holds at once for the uploaded scene (< 0: not
    // asked yet), and the last frame's launch (rr_resident_launch; blocks 0: per-tile)
    int persist_resident = -1;
    rr::PersistPlan persist_last{0, 0};
    unsigned long long* stats_src = nullptr;  // buffer holding the last frame's counters
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    // the stream of the last render (compared, never used: a caller may destroy its stream before the context) and
    // ev_out, recorded after the last render's work on it — what later renders on other streams and the context's
    // teardown wait for (the round-4 teardown hang: rr_destroy synchronised a group's render stream after the group
    // had destroyed it)
    hipStream_t last_st = nullptr;
    bool have_out = false;
    // canvas-path frames: the per-pass box averages run on aa_stream (run_levels AaPasses)
    hipStream_t aa_stream = nullptr;
    std::vector<hipEvent_t> pass_ev;
    hipEvent_t aa_done = nullptr;
    rr_stats last{};
    bool stats_pending = false;
    // the pending frame is an adaptive one: its refine pass's sample count is still on the device (adapt_counts[1]);
    // rr_last_stats adds it to last.samples
    bool adapt_pending = false;
    bool frame_timed = true;  // e0/e1 bracket the last frame
    // camera samples per wavefront pass: large, so that the deep levels of a frame (few, slow,
    // incoherent rays) run once per frame rather than once per batch; the queues of a 2^27-sample
    // pass need ~50 GB at depth 5, well inside the 288 GB of HBM
    int64_t batch = (int64_t)1 << 27;
    // bytes the worst-case recursion queues of one batch may take (run_levels shrinks the batch to fit;
    // half of the free HBM at context creation, RRAY_QUEUE_BUDGET_MB overrides)
    size_t queue_budget = (size_t)32 << 30;
    // per-kernel timing (rr_kernel_times)
    bool profile = false;
    rr::KernelProf prof;
    double kms[rr::K_COUNT] = {0};
    uint64_t kcount[rr::K_COUNT] = {0};
};

namespace {

template <class T>
hipError_t upload(DBuf& b, const std::vector<T>& v, hipStream_t st) {
    hipError_t e = b.ensure(std::max<size_t>(v.size() * sizeof(T), 16));
    if (e != hipSuccess) return e;
    if (!v.empty()) e = hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st);
    return e;
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
int64_t opts_rows(const rr_render_opts* o, int64_t H) {
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

// The context's workspace is used on one stream at a time: a call on another stream than the
// previous one first waits for it (one event, only when the stream changes).
hipError_t claim_stream(rr_ctx* c, hipStream_t st) {
    if (c->have_out && c->last_st != st) {
        hipError_t e = hipStreamWaitEvent(st, c->ev_out, 0);
        if (e != hipSuccess) return e;
    }
    c->last_st = st;
    return hipSuccess;
}
// marks the end of the work a call enqueued on `st` (claim_stream and sync_ctx wait for it)
hipError_t release_stream(rr_ctx* c, hipStream_t st) {
    hipError_t e = hipEventRecord(c->ev_out, st);
    if (e == hipSuccess) c->have_out = true;
    return e;
}
// Scope guard of a call's work on `st`: ev_out is recorded on every exit after claim_stream, error returns
// included, so work a failed call already launched is still covered by what the next call and rr_destroy wait for.
struct StreamClaim {
    rr_ctx* c;
    hipStream_t st;
    bool released = false;
    hipError_t release() {
        released = true;
        return release_stream(c, st);
    }
    ~StreamClaim() {
        if (!released) (void)release_stream(c, st);
    }
};
hipError_t sync_ctx(rr_ctx* c) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && c->have_out) e = hipEventSynchronize(c->ev_out);
    return e;
}

constexpr int kRR_ORDER_EVERY = 64;  // frames between re-sorts of the level-0 tile order
constexpr size_t kCounterBytes = (size_t)rr::RR_CNT_SLOTS * rr::RR_CNT_STRIDE * sizeof(unsigned long long);
unsigned long long* frame_counters(rr_ctx* c, int k) {
    return c->counters.as<unsigned long long>() + (size_t)k * rr::RR_CNT_SLOTS * rr::RR_CNT_STRIDE;
}

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
uint32_t persist_heads() {
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

// What a call's plans (frame_plan.hpp) read of the scene and the environment, gathered once per ABI call and never
// kept: the tests flip the switches between renders on one context.  The family predicates are the device units'
// own answers (each switch of theirs keeps its one reader) for the depth the call renders at.
struct FrameFacts {
    rr::FrameTraits traits;
    rr::FrameSwitches sw;
};
static_assert(rr::kOrderGroup == rr::RR_ORDER_GROUP, "frame_plan.hpp's order group is the sort's");
// api.cpp's own switches in one pass over the environment, which costs what one getenv does (six of them per
// frame would show in the sub-millisecond frames)
rr::FrameSwitches read_switches() {
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

rr::KernelProf* kprof(rr_ctx* c) { return c->profile ? &c->prof : nullptr; }

// The box average of a canvas-path frame (aa outside the in-wave cases, e.g. C3's aa = 3) overlapped with the
// render: the frame runs in passes of whole output rows, and each pass's rows are averaged on the context's
// second stream while the next pass renders (the render is VALU-bound, the average HBM-bound).  Null: no passes.
struct AaPasses {
    void* avg;
    int32_t f32;
    int64_t width;  // output pixels per row
    int32_t aa;
};
// `rows` output rows from row y0 on, from their samples at src
hipError_t launch_average(const AaPasses& a, const double* src, int64_t y0, int64_t rows, hipStream_t st,
                          rr::KernelProf* kp) {
    return a.f32 ? rr::launch_aa_f32(src, static_cast<float*>(a.avg) + 3 * y0 * a.width, a.width, rows, a.aa, st, kp)
                 : rr::launch_aa(src, static_cast<double*>(a.avg) + 3 * y0 * a.width, a.width, rows, a.aa, st, kp);
}

// where a run's results go (run_levels' arguments)
struct FrameOut {
    double* out;
    void* avg;
    int32_t avg_f32, aa_wave;
    const AaPasses* aap;
};

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

// Runs the wavefront levels for `total` level-0 events; level-0 rays come from the camera or from ctx->rays0
// (color_at).  Results (color_at values) land in `out` (3 doubles per event), or averaged in `avg`.  facts: the
// call's frame_facts for this max_depth.  frame_plan.hpp decides what runs; the steps below launch it.
// base0: the index of the run's first event (a multiple of 64 and rays0 only: a pass of a lens frame, whose events are
// the frame's base0 .. base0 + total — sample identity, ray and output slot — through pointers the caller biased by
// -base0 entries).
int run_levels(rr_ctx* c, const FrameFacts& facts, const rr::LevelArgs& base_args, int64_t total, int max_depth,
               double* out, hipStream_t st, void* avg = nullptr, int32_t avg_f32 = 0, int32_t aa_wave = 0,
               const AaPasses* aap = nullptr, int64_t base0 = 0) {
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

int resolve_prof(rr_ctx* c) {
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

int finish_stats(rr_ctx* c) {
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

}  // namespace

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
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
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
    c->frame_timed = !(o->flags & RR_NO_FRAME_TIMING);
    if (c->frame_timed) HIPCHK(hipEventRecord(c->e0, st));
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
    if (c->frame_timed) HIPCHK(hipEventRecord(c->e1, st));
    HIPCHK(claim.release());
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
    rr_stats local;
    rc = rr_last_stats(c, stats ? stats : &local);
    if (rc != RR_OK) return rc;
    const uint64_t nan = (stats ? stats : &local)->nan_rays;
    return nan ? nan_fail(nan) : RR_OK;
}

int rr_color_at(rr_ctx* c, int64_t n, const double* origins, const double* directions, int32_t remaining,
                uint64_t seed, int32_t jitter_mode, double* out_rgb) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (c && c->group) return rr_color_at(rr::group_local(c->group, 0), n, origins, directions, remaining, seed, jitter_mode, out_rgb);
    if (!c || (n > 0 && (!origins || !directions || !out_rgb))) return fail(RR_E_ARG, "null argument");
    if (!c->has_scene) return fail(RR_E_ARG, "no scene uploaded");
    if (remaining < 0 || remaining > RR_MAX_DEPTH) return fail(RR_E_LIMIT, "remaining out of range");
    if (n == 0) return RR_OK;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    std::vector<double> rays((size_t)n * 6);
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            rays[6 * i + k] = origins[3 * i + k];
            rays[6 * i + 3 + k] = directions[3 * i + k];
        }
    HIPCHK(upload(c->rays0, rays, st));
    HIPCHK(c->qout.ensure(n * 3 * sizeof(double)));
    const int saved_epoch = c->epoch;
    c->epoch = 2;  // the query buffer (frame buffers keep their state)
    HIPCHK(hipMemsetAsync(frame_counters(c, 2), 0, kCounterBytes, st));
    rr::LevelArgs A{};
    A.hs = 1;
    A.aa = 1;
    A.part = 0;
    A.nparts = 1;
    A.block_rows = 1;
    A.rays0 = c->rays0.as<double>();
    A.seed = seed;
    A.jitter_mode = jitter_mode;
    int rc = run_levels(c, frame_facts(c, remaining), A, n, remaining, c->qout.as<double>(), st);
    c->epoch = saved_epoch;
    if (rc != RR_OK) return rc;
    HIPCHK(hipMemcpyAsync(out_rgb, c->qout.p, n * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    // the counters on the same (non-blocking) stream, then wait: out_rgb and the counters are both
    // complete on return, whatever kind of host memory the caller passed
    HIPCHK(hipMemcpyAsync(c->h_counters, frame_counters(c, 2), kCounterBytes, hipMemcpyDeviceToHost, st));
    HIPCHK(claim.release());
    HIPCHK(hipStreamSynchronize(st));
    rr_stats q;
    collect_stats(c, &q);
    return q.nan_rays ? nan_fail(q.nan_rays) : RR_OK;
}

int rr_is_shadowed(rr_ctx* c, int64_t n, const double* points, const double* light_positions, int32_t* out) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (c && c->group) return rr_is_shadowed(rr::group_local(c->group, 0), n, points, light_positions, out);
    if (!c || (n > 0 && (!points || !light_positions || !out))) return fail(RR_E_ARG, "null argument");
    if (!c->has_scene) return fail(RR_E_ARG, "no scene uploaded");
    if (n == 0) return RR_OK;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    std::vector<double> buf((size_t)n * 6);
    std::memcpy(buf.data(), points, n * 3 * sizeof(double));
    std::memcpy(buf.data() + 3 * n, light_positions, n * 3 * sizeof(double));
    HIPCHK(upload(c->rays0, buf, st));
    HIPCHK(c->qout.ensure(n * sizeof(int32_t)));
    HIPCHK(rr::launch_shadow_query(c->S, c->rays0.as<double>(), c->rays0.as<double>() + 3 * n, n,
                                   c->qout.as<int32_t>(), frame_counters(c, 2), st));
    HIPCHK(hipMemcpyAsync(out, c->qout.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(claim.release());
    HIPCHK(hipStreamSynchronize(st));
    return RR_OK;
}

// ---- ABI 11: first-hit queries (render_hit.inc hit_kernel) ----
static_assert(sizeof(rr_hit) == 192, "rr_hit is 192 bytes (rray.h)");

int rr_hit_at(rr_ctx* c, int64_t n, const double* origins, const double* directions, rr_hit* out) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (c && c->group) return rr_hit_at(rr::group_local(c->group, 0), n, origins, directions, out);
    if (!c || n < 0 || (n > 0 && (!origins || !directions || !out))) return fail(RR_E_ARG, "null argument");
    if (!c->has_scene) return fail(RR_E_ARG, "no scene uploaded");
    if (n == 0) return RR_OK;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    std::vector<double> rays((size_t)n * 6);
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            rays[6 * i + k] = origins[3 * i + k];
            rays[6 * i + 3 + k] = directions[3 * i + k];
        }
    HIPCHK(upload(c->rays0, rays, st));
    // the records as planes: RR_HIT_DOUBLES double planes, then the two int planes
    const size_t d_bytes = (size_t)n * rr::RR_HIT_DOUBLES * sizeof(double), i_bytes = (size_t)n * 2 * sizeof(int32_t);
    HIPCHK(c->hitrec.ensure(d_bytes + i_bytes));
    HIPCHK(hipMemsetAsync(frame_counters(c, 2), 0, kCounterBytes, st));  // the query buffer (frame buffers keep their state)
    rr::HitOut O{};
    O.node_object = c->node_object.as<int32_t>();
    O.rec_d = c->hitrec.as<double>();
    O.rec_i = reinterpret_cast<int32_t*>(c->hitrec.as<char>() + d_bytes);
    O.stride = n;
    rr::LevelArgs A{};
    A.hs = 1;
    A.aa = 1;
    A.part = 0;
    A.nparts = 1;
    A.block_rows = 1;
    A.rays0 = c->rays0.as<double>();
    A.nseg = A.nseg_out = 1;
    A.counters = frame_counters(c, 2);
    for (int64_t base = 0; base < n; base += c->batch) {
        A.base = base;
        A.n = std::min<int64_t>(c->batch, n - base);
        set_level0_index(A);
        HIPCHK(rr::launch_hit(c->S, A, O, st));
    }
    std::vector<double> hd((size_t)n * rr::RR_HIT_DOUBLES);
    std::vector<int32_t> hi((size_t)n * 2);
    HIPCHK(hipMemcpyAsync(hd.data(), O.rec_d, d_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hi.data(), O.rec_i, i_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(c->h_counters, frame_counters(c, 2), kCounterBytes, hipMemcpyDeviceToHost, st));
    HIPCHK(claim.release());
    HIPCHK(hipStreamSynchronize(st));
    for (int64_t i = 0; i < n; ++i) {
        rr_hit& h = out[i];
        const auto f = [&](int k) { return hd[(size_t)k * n + i]; };
        h.object = hi[i];
        h.inside = hi[(size_t)n + i];
        h.t = f(0);
        h.u = f(1);
        h.v = f(2);
        for (int k = 0; k < 3; ++k) {
            h.point[k] = f(3 + k);
            h.eyev[k] = f(6 + k);
            h.normalv[k] = f(9 + k);
            h.over_point[k] = f(12 + k);
            h.under_point[k] = f(15 + k);
            h.reflectv[k] = f(18 + k);
        }
        h.n1 = f(21);
        h.n2 = f(22);
    }
    // these are the context's last stats now (rr_last_stats): complete, nothing pending
    collect_stats(c, &c->last);
    c->last.samples = (uint64_t)n;
    c->last.kernel_ms = 0.0;
    c->stats_pending = false;
    c->adapt_pending = false;
    return c->last.nan_rays ? nan_fail(c->last.nan_rays) : RR_OK;
}

int rr_render_aov_device(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, int32_t planes, void* d_depth,
                         void* d_normal, void* d_object, void* d_albedo, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (c && c->group)
        return rr_render_aov_device(rr::group_local(c->group, 0), cam, o, planes, d_depth, d_normal, d_object, d_albedo,
                                    hip_stream);
    if (!c) return fail(RR_E_ARG, "null context");
    if (!c->has_scene) return fail(RR_E_ARG, "no scene uploaded");
    if (!cam || !o) return fail(RR_E_ARG, "null camera/options");
    rr_render_opts opts = *o;
    opts.max_depth = 0;  // ignored here (as seed, jitter_mode and flags): no recursion in a first-hit frame
    int rc = check_opts(cam, &opts);
    if (rc != RR_OK) return rc;
    if (o->part != 0 || o->nparts != 1 || o->row_begin != 0 || o->row_end != 0)
        return fail(RR_E_ARG, "AOV frames are whole frames: part 0 of 1, no band");
    const int32_t all = RR_AOV_DEPTH | RR_AOV_NORMAL | RR_AOV_OBJECT | RR_AOV_ALBEDO;
    if (planes == 0 || (planes & ~all)) return fail(RR_E_ARG, "planes must be a non-empty combination of RR_AOV_*");
    if (((planes & RR_AOV_DEPTH) && !d_depth) || ((planes & RR_AOV_NORMAL) && !d_normal) ||
        ((planes & RR_AOV_OBJECT) && !d_object) || ((planes & RR_AOV_ALBEDO) && !d_albedo))
        return fail(RR_E_ARG, "a requested plane has a null buffer");
    const int64_t total = cam->hsize * cam->vsize;
    if (total >= ((int64_t)1 << 31)) return fail(RR_E_LIMIT, "an AOV frame must hold fewer than 2^31 samples");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    c->frame_timed = true;
    HIPCHK(hipEventRecord(c->e0, st));
    HIPCHK(hipMemsetAsync(frame_counters(c, 2), 0, kCounterBytes, st));  // the query buffer (frame buffers keep their state)
    rr::LevelArgs A{};
    set_camera(A, cam);
    A.hs = cam->hsize;
    A.lrows = cam->vsize;
    A.aa = o->aa;
    A.part = 0;
    A.nparts = 1;
    A.block_rows = o->block_rows > 0 ? o->block_rows : 8;
    A.rays0 = nullptr;
    A.nseg = A.nseg_out = 1;
    rc = tile_bundles(c, A, st, &A.tile_bundles);  // the colour frames' cached table (same key: camera and layout)
    if (rc != RR_OK) return rc;
    A.base = 0;
    A.level = 0;
    A.n = total;
    set_level0_index(A);
    A.counters = frame_counters(c, 2);
    rr::HitOut O{};
    O.node_object = c->node_object.as<int32_t>();
    O.depth = (planes & RR_AOV_DEPTH) ? static_cast<double*>(d_depth) : nullptr;
    O.normal = (planes & RR_AOV_NORMAL) ? static_cast<double*>(d_normal) : nullptr;
    O.object = (planes & RR_AOV_OBJECT) ? static_cast<int32_t*>(d_object) : nullptr;
    O.albedo = (planes & RR_AOV_ALBEDO) ? static_cast<double*>(d_albedo) : nullptr;
    HIPCHK(rr::launch_hit(c->S, A, O, st));
    c->stats_src = frame_counters(c, 2);
    HIPCHK(hipEventRecord(c->e1, st));
    HIPCHK(claim.release());
    c->stats_pending = true;
    c->last.samples = (uint64_t)total;
    c->adapt_pending = false;
    return RR_OK;
}

int rr_render_aov(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, int32_t planes, double* depth,
                  double* normal, int32_t* object, double* albedo, rr_stats* stats) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (c && c->group) return rr_render_aov(rr::group_local(c->group, 0), cam, o, planes, depth, normal, object, albedo, stats);
    if (!c) return fail(RR_E_ARG, "null context");
    if (!c->has_scene) return fail(RR_E_ARG, "no scene uploaded");
    if (!cam || !o) return fail(RR_E_ARG, "null camera/options");
    if (((planes & RR_AOV_DEPTH) && !depth) || ((planes & RR_AOV_NORMAL) && !normal) ||
        ((planes & RR_AOV_OBJECT) && !object) || ((planes & RR_AOV_ALBEDO) && !albedo))
        return fail(RR_E_ARG, "a requested plane has a null buffer");
    if (cam->hsize <= 0 || cam->vsize <= 0 || cam->hsize > (1ll << 31) || cam->vsize > (1ll << 31))
        return fail(RR_E_ARG, "bad camera size");
    HIPCHK(hipSetDevice(c->device));
    // the device planes back to back: depth, normal, albedo (doubles), then object
    const size_t total = (size_t)cam->hsize * (size_t)cam->vsize;
    const size_t off_normal = total * sizeof(double), off_albedo = off_normal + total * 3 * sizeof(double);
    const size_t off_object = off_albedo + total * 3 * sizeof(double);
    HIPCHK(c->aov.ensure(off_object + total * sizeof(int32_t)));
    char* base = c->aov.as<char>();
    int rc = rr_render_aov_device(c, cam, o, planes, base, base + off_normal, base + off_object, base + off_albedo, nullptr);
    if (rc != RR_OK) return rc;
    hipStream_t st = c->stream;
    if (planes & RR_AOV_DEPTH) HIPCHK(hipMemcpyAsync(depth, base, total * sizeof(double), hipMemcpyDeviceToHost, st));
    if (planes & RR_AOV_NORMAL)
        HIPCHK(hipMemcpyAsync(normal, base + off_normal, total * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (planes & RR_AOV_ALBEDO)
        HIPCHK(hipMemcpyAsync(albedo, base + off_albedo, total * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (planes & RR_AOV_OBJECT)
        HIPCHK(hipMemcpyAsync(object, base + off_object, total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    rr_stats local;
    rc = rr_last_stats(c, stats ? stats : &local);
    if (rc != RR_OK) return rc;
    const uint64_t nan = (stats ? stats : &local)->nan_rays;
    return nan ? nan_fail(nan) : RR_OK;
}

// ---- adaptive anti-aliasing (render_adapt.hip) ----
// what both entry points refuse before they look at the context (so a host without a device can test it)
static int adaptive_check_args(const rr_camera* cam, const rr_render_opts* o, double threshold, const void* avg) {
    if (!cam || !o || !avg) return fail(RR_E_ARG, "rr_render_adaptive: null camera / options / output image");
    if (threshold != threshold) return fail(RR_E_ARG, "rr_render_adaptive: the threshold is NaN");
    if (o->part != 0 || o->nparts != 1 || o->row_begin != 0 || o->row_end != 0)
        return fail(RR_E_ARG, "adaptive frames are whole frames: part 0 of 1, no band");
    if (o->flags & ~RR_NO_FRAME_TIMING) return fail(RR_E_ARG, "adaptive frames take no flag but RR_NO_FRAME_TIMING");
    return RR_OK;
}

int rr_render_adaptive_device(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, double threshold, void* d_avg,
                              void* d_mask, void* d_n_refined, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = adaptive_check_args(cam, o, threshold, d_avg);
    if (rc != RR_OK) return rc;
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return fail(RR_E_ARG, "adaptive frames need a single-device context (no multi-device or virtual context)");
    rc = rr::render_validate(c, cam, o);  // rr_render's own checks (scene, depth, sizes)
    if (rc != RR_OK) return rc;
    const int32_t aa = o->aa;
    const int64_t W = cam->hsize / aa, H = cam->vsize / aa;
    if ((uint64_t)cam->hsize * (uint64_t)cam->vsize >= (1ull << 32))
        return fail(RR_E_LIMIT, "an adaptive frame must hold fewer than 2^32 samples");
    const int64_t total = W * H * aa * aa;  // the refine pass's capacity: every pixel listed
    if (total > c->batch) return fail(RR_E_LIMIT, "an adaptive frame's samples must fit one pass of the context");
    const FrameFacts facts = frame_facts(c, o->max_depth);
    if (!rr::in_wave(rr::frame_family(facts.traits, o->max_depth)))
        return fail(RR_E_ARG, "adaptive frames are not served by the per-level paths (RRAY_UNFUSED / RRAY_NO_TREE / RRAY_NO_CHAIN)");
    // 1. the probe's camera and options: the aa 1 frame of the same view
    rr_camera cam1;
    rc = rr_camera_new(W, H, cam->field_of_view, cam->transform, &cam1);
    if (rc != RR_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    const int64_t n_blocks = (W * H + rr::RR_ADAPT_BLOCK - 1) / rr::RR_ADAPT_BLOCK;
    HIPCHK(c->adapt_flags.ensure((size_t)(W * H)));
    HIPCHK(c->adapt_blocks.ensure((size_t)n_blocks * sizeof(uint32_t)));
    HIPCHK(c->adapt_counts.ensure(2 * sizeof(uint32_t)));
    HIPCHK(c->adapt_list.ensure((size_t)(W * H) * sizeof(uint32_t)));
    if (aa > 1) HIPCHK(c->canvas.ensure((size_t)total * 3 * sizeof(double)));  // the refine pass's compact samples
    c->frame_timed = !(o->flags & RR_NO_FRAME_TIMING);
    if (c->frame_timed) HIPCHK(hipEventRecord(c->e0, st));
    const int32_t block = o->block_rows > 0 ? o->block_rows : 8;
    // the probe is rr_render_device's aa 1 frame, launch for launch: straight into d_avg; its first kernels zero the
    // next frame's counters
    rr::LevelArgs A1 = camera_args(&cam1, o, 1, 0, block);  // part 0 of 1 (adaptive_check_args)
    A1.lrows = H;
    rc = tile_bundles(c, A1, st, &A1.tile_bundles);
    if (rc != RR_OK) return rc;
    begin_frame_counters(c);
    rc = run_levels(c, facts, A1, W * H, o->max_depth, nullptr, st, d_avg, 0, 0, nullptr);
    c->zero_next = false;
    if (rc != RR_OK) return rc;
    // 2. mask, ordered compaction: the list and its length stay on the device
    rr::AdaptArgs P{};
    P.frame = static_cast<const double*>(d_avg);
    P.avg = static_cast<double*>(d_avg);
    P.w = W;
    P.h = H;
    P.aa = aa;
    P.thr = threshold;
    P.flags = c->adapt_flags.as<uint8_t>();
    P.mask = static_cast<uint8_t*>(d_mask);
    P.block_count = c->adapt_blocks.as<uint32_t>();
    P.counts = c->adapt_counts.as<uint32_t>();
    P.n_refined = static_cast<int64_t*>(d_n_refined);
    P.list = c->adapt_list.as<uint32_t>();
    P.samples = c->canvas.as<double>();
    HIPCHK(rr::launch_adapt_select(P, st));
    if (aa > 1) {
        // 3. the refine pass: the listed pixels' samples through the scene's own kernel family, counted into the
        // probe's counters (same epoch, nothing zeroed); launched for the capacity, the live count is P.counts[1]
        rr::LevelArgs A2 = camera_args(cam, o, aa, 0, block);
        A2.lrows = 0;  // no tile layout: events are list entries
        A2.list = P.list;
        A2.list_w = (uint32_t)W;
        A2.n_dev = P.counts + 1;
        rc = run_levels(c, facts, A2, total, o->max_depth, c->canvas.as<double>(), st);
        if (rc != RR_OK) return rc;
        // 4. canvas.rs:85-96 per listed pixel, over its aa 1 colour
        HIPCHK(rr::launch_adapt_resolve(P, st));
    }
    end_frame_counters(c);
    if (c->frame_timed) HIPCHK(hipEventRecord(c->e1, st));
    HIPCHK(claim.release());
    c->stats_pending = true;
    c->last.samples = (uint64_t)(W * H);  // + aa^2 x the refined pixels, still on the device: rr_last_stats adds them
    c->adapt_pending = true;
    return RR_OK;
}

int rr_render_adaptive(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, double threshold, double* out_avg,
                       uint8_t* out_mask, int64_t* n_refined, rr_stats* stats) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = adaptive_check_args(cam, o, threshold, out_avg);
    if (rc != RR_OK) return rc;
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return fail(RR_E_ARG, "adaptive frames need a single-device context (no multi-device or virtual context)");
    rc = check_opts(cam, o);
    if (rc != RR_OK) return rc;
    const int64_t W = cam->hsize / o->aa, H = cam->vsize / o->aa;
    HIPCHK(hipSetDevice(c->device));
    // device outputs: the image in qout, then the count, then the mask
    const size_t img = (size_t)(W * H) * 3 * sizeof(double);
    HIPCHK(c->qout.ensure(img));
    HIPCHK(c->adapt_mask.ensure((size_t)(W * H) + 16));
    char* mbase = c->adapt_mask.as<char>();  // [0, 8): n_refined; [16, ...): the mask
    rc = rr_render_adaptive_device(c, cam, o, threshold, c->qout.p, mbase + 16, mbase, nullptr);
    if (rc != RR_OK) return rc;
    int64_t n = 0;
    HIPCHK(hipMemcpyAsync(out_avg, c->qout.p, img, hipMemcpyDeviceToHost, c->stream));
    if (out_mask) HIPCHK(hipMemcpyAsync(out_mask, mbase + 16, (size_t)(W * H), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&n, mbase, sizeof n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (n_refined) *n_refined = n;
    rr_stats local;
    rc = rr_last_stats(c, stats ? stats : &local);
    if (rc != RR_OK) return rc;
    const uint64_t nan = (stats ? stats : &local)->nan_rays;
    return nan ? nan_fail(nan) : RR_OK;
}

// ---- batches of views (render_views.hip) ----
// what both entry points refuse before they look at the context (so a host without a device can test it)
static int views_check_args(const rr_camera* cams, int32_t n_views, const rr_render_opts* o, const void* canvas,
                            const void* avg) {
    if (!cams) return fail(RR_E_ARG, "rr_render_views: null camera array");
    if (!o) return fail(RR_E_ARG, "rr_render_views: null options");
    if (n_views < 0) return fail(RR_E_ARG, "rr_render_views: n_views is negative");
    if (o->part != 0 || o->nparts != 1 || o->row_begin != 0 || o->row_end != 0)
        return fail(RR_E_ARG, "batches of views are whole frames: part 0 of 1, no band");
    if (o->flags & RR_OUT_AVG_F32) return fail(RR_E_ARG, "batches of views write f64 images: RR_OUT_AVG_F32 is not served");
    if (o->flags & RR_PART_INTERLEAVE)
        return fail(RR_E_ARG, "batches of views run on one device: RR_PART_INTERLEAVE is not served");
    if ((o->flags & RR_OUT_CANVAS) && !canvas) return fail(RR_E_ARG, "rr_render_views: RR_OUT_CANVAS with a null canvas buffer");
    if ((o->flags & RR_OUT_AVG) && !avg) return fail(RR_E_ARG, "rr_render_views: RR_OUT_AVG with a null image buffer");
    for (int32_t k = 1; k < n_views; ++k)
        if (cams[k].hsize != cams[0].hsize || cams[k].vsize != cams[0].vsize)
            return fail(RR_E_ARG, "the cameras of a batch must share hsize and vsize: camera " + std::to_string(k) + " is " +
                                      std::to_string(cams[k].hsize) + "x" + std::to_string(cams[k].vsize) + ", camera 0 " +
                                      std::to_string(cams[0].hsize) + "x" + std::to_string(cams[0].vsize));
    return RR_OK;
}

int rr_render_views_device(rr_ctx* c, const rr_camera* cams, int32_t n_views, const rr_render_opts* o, void* d_canvas,
                           void* d_avg, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = views_check_args(cams, n_views, o, d_canvas, d_avg);
    if (rc != RR_OK) return rc;
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return fail(RR_E_ARG, "batches of views need a single-device context (no multi-device or virtual context)");
    if (n_views == 0) return RR_OK;
    rc = rr::render_validate(c, &cams[0], o);  // rr_render's own checks (scene, depth, sizes against aa)
    if (rc != RR_OK) return rc;
    const int32_t aa = o->aa;
    const int64_t hs = cams[0].hsize, vs = cams[0].vsize, W = hs / aa, H = vs / aa;
    const int64_t E = rr::view_events(hs, vs), total = (int64_t)n_views * E;
    const FrameFacts facts = frame_facts(c, o->max_depth);
    double* canvas = (o->flags & RR_OUT_CANVAS) ? static_cast<double*>(d_canvas) : nullptr;
    double* avg = (o->flags & RR_OUT_AVG) ? static_cast<double*>(d_avg) : nullptr;
    // as rr_render_device's frames: aa 1 and the level-0 waves' own average (aa 2 / 4 / 8, full tiles) write the image
    // directly; every other aa goes through the stacked canvases, n_views * vs rows of hs samples, which aa_kernel
    // averages as one image (vs = H * aa: no pixel's box crosses a view).  Pixel waves do not serve batches.
    rr::OutputPlan mode = rr::plan_output(facts.traits, facts.sw, avg != nullptr, aa, hs, vs, o->max_depth, 8, c->batch);
    mode.pw = false;
    mode.direct_avg = avg && (aa == 1 || mode.wave_avg);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->views.ensure(((size_t)n_views + rr::RR_VIEW_TABLE_PAD) * sizeof(rr::DevView)));
    rr::LevelArgs A = camera_args(&cams[0], o, aa, 0, 8);  // part 0 of 1 (views_check_args); A.cam itself is not read
    A.lrows = vs;
    A.views = c->views.as<rr::DevView>();
    A.view_e = (uint32_t)std::min<int64_t>(E, (int64_t)1 << 31);
    {  // what the plan refuses (a per-level family, a view larger than a pass), before anything is enqueued
        const FrameOut o0{canvas, mode.direct_avg ? avg : nullptr, 0, mode.wave_avg ? aa : 0, nullptr};
        const rr::FramePlan pre = plan_run(c, facts, A, total, o->max_depth, o0);
        if (pre.err != RR_OK) return fail(pre.err, pre.msg);
    }
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    if (!canvas && avg && !mode.direct_avg) {
        HIPCHK(c->canvas.ensure((size_t)n_views * hs * vs * 3 * sizeof(double)));
        canvas = c->canvas.as<double>();
    }
    // the camera table: the context's host copy (the caller's array is free after this call), then its device buffer,
    // on the render's stream
    c->views_host.assign((size_t)n_views + rr::RR_VIEW_TABLE_PAD, rr::DevView{});
    for (int32_t k = 0; k < n_views; ++k) {
        rr::LevelArgs T{};
        set_camera(T, &cams[k]);
        c->views_host[k].cam = T.cam;
        c->views_host[k].affine = T.cam_affine;
    }
    HIPCHK(hipMemcpyAsync(c->views.p, c->views_host.data(), c->views_host.size() * sizeof(rr::DevView),
                          hipMemcpyHostToDevice, st));
    c->frame_timed = !(o->flags & RR_NO_FRAME_TIMING);
    if (c->frame_timed) HIPCHK(hipEventRecord(c->e0, st));
    // the colour frames' per-camera state stays as it is: no cached bundles, no cost order, no resident launch
    begin_frame_counters(c);
    rc = run_levels(c, facts, A, total, o->max_depth, canvas, st, mode.direct_avg ? avg : nullptr, 0,
                    mode.wave_avg ? aa : 0, nullptr);
    c->zero_next = false;
    if (rc != RR_OK) return rc;
    if (avg && !mode.direct_avg) HIPCHK(rr::launch_aa(canvas, avg, W, (int64_t)n_views * H, aa, st, kprof(c)));
    end_frame_counters(c);
    if (c->frame_timed) HIPCHK(hipEventRecord(c->e1, st));
    HIPCHK(claim.release());
    c->stats_pending = true;
    c->last.samples = (uint64_t)n_views * (uint64_t)(hs * vs);
    c->adapt_pending = false;
    return RR_OK;
}

int rr_render_views(rr_ctx* c, const rr_camera* cams, int32_t n_views, const rr_render_opts* o, double* out_canvas,
                    double* out_avg, rr_stats* stats) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = views_check_args(cams, n_views, o, out_canvas, out_avg);
    if (rc != RR_OK) return rc;
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return fail(RR_E_ARG, "batches of views need a single-device context (no multi-device or virtual context)");
    if (n_views == 0) return RR_OK;
    rc = check_opts(&cams[0], o);
    if (rc != RR_OK) return rc;
    const int64_t hs = cams[0].hsize, vs = cams[0].vsize, W = hs / o->aa, H = vs / o->aa;
    const size_t img = (size_t)n_views * W * H * 3 * sizeof(double), cnv = (size_t)n_views * hs * vs * 3 * sizeof(double);
    const bool want_avg = (o->flags & RR_OUT_AVG) != 0, want_canvas = (o->flags & RR_OUT_CANVAS) != 0;
    HIPCHK(hipSetDevice(c->device));
    if (want_avg) HIPCHK(c->qout.ensure(img));
    if (want_canvas) HIPCHK(c->canvas.ensure(cnv));
    rc = rr_render_views_device(c, cams, n_views, o, want_canvas ? c->canvas.p : nullptr, want_avg ? c->qout.p : nullptr,
                                nullptr);
    if (rc != RR_OK) return rc;
    if (want_canvas) HIPCHK(hipMemcpyAsync(out_canvas, c->canvas.p, cnv, hipMemcpyDeviceToHost, c->stream));
    if (want_avg) HIPCHK(hipMemcpyAsync(out_avg, c->qout.p, img, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    rr_stats local;
    rc = rr_last_stats(c, stats ? stats : &local);
    if (rc != RR_OK) return rc;
    const uint64_t nan = (stats ? stats : &local)->nan_rays;
    return nan ? nan_fail(nan) : RR_OK;
}

// ---- first-hit planes of batches of views (render_views.hip launch_hit_views) ----
// what both entry points refuse before they look at the context (so a host without a device can test it)
static int views_aov_check_args(const rr_camera* cams, int32_t n_views, const rr_render_opts* o, int32_t planes,
                                const void* depth, const void* normal, const void* object, const void* albedo) {
    if (!cams) return fail(RR_E_ARG, "rr_render_views_aov: null camera array");
    if (!o) return fail(RR_E_ARG, "rr_render_views_aov: null options");
    if (n_views < 0) return fail(RR_E_ARG, "rr_render_views_aov: n_views is negative");
    if (o->part != 0 || o->nparts != 1 || o->row_begin != 0 || o->row_end != 0)
        return fail(RR_E_ARG, "batches of AOV frames are whole frames: part 0 of 1, no band");
    const int32_t all = RR_AOV_DEPTH | RR_AOV_NORMAL | RR_AOV_OBJECT | RR_AOV_ALBEDO;
    if (planes == 0 || (planes & ~all)) return fail(RR_E_ARG, "planes must be a non-empty combination of RR_AOV_*");
    if (((planes & RR_AOV_DEPTH) && !depth) || ((planes & RR_AOV_NORMAL) && !normal) ||
        ((planes & RR_AOV_OBJECT) && !object) || ((planes & RR_AOV_ALBEDO) && !albedo))
        return fail(RR_E_ARG, "a requested plane has a null buffer");
    for (int32_t k = 1; k < n_views; ++k)
        if (cams[k].hsize != cams[0].hsize || cams[k].vsize != cams[0].vsize)
            return fail(RR_E_ARG, "the cameras of a batch must share hsize and vsize: camera " + std::to_string(k) + " is " +
                                      std::to_string(cams[k].hsize) + "x" + std::to_string(cams[k].vsize) + ", camera 0 " +
                                      std::to_string(cams[0].hsize) + "x" + std::to_string(cams[0].vsize));
    return RR_OK;
}
// ... and what they ask of the context and of the sizes, with the batch's pass split (nothing is enqueued before it)
static int views_aov_validate(rr_ctx* c, const rr_camera* cams, int32_t n_views, const rr_render_opts* o,
                              rr::ViewAovPlan* plan) {
    if (!c->has_scene) return fail(RR_E_ARG, "no scene uploaded");
    rr_render_opts opts = *o;
    opts.max_depth = 0;  // ignored here (as seed, jitter_mode and flags): no recursion in a first-hit frame
    int rc = check_opts(&cams[0], &opts);
    if (rc != RR_OK) return rc;
    *plan = rr::plan_views_aov(c->batch, cams[0].hsize, cams[0].vsize, n_views);
    return plan->err != RR_OK ? fail(plan->err, plan->msg) : RR_OK;
}

int rr_render_views_aov_device(rr_ctx* c, const rr_camera* cams, int32_t n_views, const rr_render_opts* o, int32_t planes,
                               void* d_depth, void* d_normal, void* d_object, void* d_albedo, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = views_aov_check_args(cams, n_views, o, planes, d_depth, d_normal, d_object, d_albedo);
    if (rc != RR_OK) return rc;
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return fail(RR_E_ARG, "batches of views need a single-device context (no multi-device or virtual context)");
    if (n_views == 0) return RR_OK;
    rr::ViewAovPlan plan{};
    rc = views_aov_validate(c, cams, n_views, o, &plan);
    if (rc != RR_OK) return rc;
    const int64_t hs = cams[0].hsize, vs = cams[0].vsize, vsamples = hs * vs;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->views.ensure(((size_t)n_views + rr::RR_VIEW_TABLE_PAD) * sizeof(rr::DevView)));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    // the camera table: the context's host copy (the caller's array is free after this call), then its device buffer,
    // on the call's stream; the padding's flags say "not affine" to the last block's waves past the events
    c->views_host.assign((size_t)n_views + rr::RR_VIEW_TABLE_PAD, rr::DevView{});
    for (int32_t k = 0; k < n_views; ++k) {
        rr::LevelArgs T{};
        set_camera(T, &cams[k]);
        c->views_host[k].cam = T.cam;
        c->views_host[k].affine = T.cam_affine;
    }
    HIPCHK(hipMemcpyAsync(c->views.p, c->views_host.data(), c->views_host.size() * sizeof(rr::DevView),
                          hipMemcpyHostToDevice, st));
    c->frame_timed = true;
    HIPCHK(hipEventRecord(c->e0, st));
    HIPCHK(hipMemsetAsync(frame_counters(c, 2), 0, kCounterBytes, st));  // the query buffer (frame buffers keep their state)
    // the single frames' per-camera state stays as it is: no cached bundles (tiles_valid), no order, no resident launch
    rr::LevelArgs A{};
    set_camera(A, &cams[0]);  // A.cam itself is not read: every wave takes its view's camera from the table
    A.hs = hs;
    A.lrows = vs;
    A.aa = o->aa;
    A.part = 0;
    A.nparts = 1;
    A.block_rows = o->block_rows > 0 ? o->block_rows : 8;
    A.rays0 = nullptr;
    A.nseg = A.nseg_out = 1;
    A.base = 0;
    A.level = 0;
    A.view_e = (uint32_t)plan.view_e;  // <= the pass cap < 2^31 (plan_views_aov)
    set_level0_index(A);
    A.counters = frame_counters(c, 2);
    for (int64_t v0 = 0; v0 < n_views; v0 += plan.views_per_pass) {  // a pass: whole views, one launch
        const int64_t nv = std::min<int64_t>(plan.views_per_pass, n_views - v0);
        A.views = c->views.as<rr::DevView>() + v0;
        A.n = nv * plan.view_e;
        rr::HitOut O{};
        O.node_object = c->node_object.as<int32_t>();
        O.depth = (planes & RR_AOV_DEPTH) ? static_cast<double*>(d_depth) + v0 * vsamples : nullptr;
        O.normal = (planes & RR_AOV_NORMAL) ? static_cast<double*>(d_normal) + 3 * v0 * vsamples : nullptr;
        O.object = (planes & RR_AOV_OBJECT) ? static_cast<int32_t*>(d_object) + v0 * vsamples : nullptr;
        O.albedo = (planes & RR_AOV_ALBEDO) ? static_cast<double*>(d_albedo) + 3 * v0 * vsamples : nullptr;
        HIPCHK(rr::launch_hit_views(c->S, A, O, st));
    }
    c->stats_src = frame_counters(c, 2);
    HIPCHK(hipEventRecord(c->e1, st));
    HIPCHK(claim.release());
    c->stats_pending = true;
    c->last.samples = (uint64_t)n_views * (uint64_t)vsamples;
    c->adapt_pending = false;
    return RR_OK;
}

int rr_render_views_aov(rr_ctx* c, const rr_camera* cams, int32_t n_views, const rr_render_opts* o, int32_t planes,
                        double* depth, double* normal, int32_t* object, double* albedo, rr_stats* stats) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = views_aov_check_args(cams, n_views, o, planes, depth, normal, object, albedo);
    if (rc != RR_OK) return rc;
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return fail(RR_E_ARG, "batches of views need a single-device context (no multi-device or virtual context)");
    if (n_views == 0) return RR_OK;
    rr::ViewAovPlan plan{};
    rc = views_aov_validate(c, cams, n_views, o, &plan);  // before the staging buffers grow
    if (rc != RR_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    // the device planes back to back, each stacked over the views: depth, normal, albedo (doubles), then object
    const size_t total = (size_t)n_views * (size_t)cams[0].hsize * (size_t)cams[0].vsize;
    const size_t off_normal = total * sizeof(double), off_albedo = off_normal + total * 3 * sizeof(double);
    const size_t off_object = off_albedo + total * 3 * sizeof(double);
    HIPCHK(c->aov.ensure(off_object + total * sizeof(int32_t)));
    char* base = c->aov.as<char>();
    rc = rr_render_views_aov_device(c, cams, n_views, o, planes, base, base + off_normal, base + off_object,
                                    base + off_albedo, nullptr);
    if (rc != RR_OK) return rc;
    hipStream_t st = c->stream;
    if (planes & RR_AOV_DEPTH) HIPCHK(hipMemcpyAsync(depth, base, total * sizeof(double), hipMemcpyDeviceToHost, st));
    if (planes & RR_AOV_NORMAL)
        HIPCHK(hipMemcpyAsync(normal, base + off_normal, total * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (planes & RR_AOV_ALBEDO)
        HIPCHK(hipMemcpyAsync(albedo, base + off_albedo, total * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (planes & RR_AOV_OBJECT)
        HIPCHK(hipMemcpyAsync(object, base + off_object, total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    rr_stats local;
    rc = rr_last_stats(c, stats ? stats : &local);
    if (rc != RR_OK) return rc;
    const uint64_t nan = (stats ? stats : &local)->nan_rays;
    return nan ? nan_fail(nan) : RR_OK;
}

// ---- device-resident ray queries (render_rays.hip) ----
// The caller's buffers go to the kernels as they are (LevelArgs.rays0 / out, launch_shadow_query's arrays); nothing is
// staged but rr_hit_at_device's planes, nothing is copied to the host and nothing waits.  None of them touches the
// frames' state: no tile_bundles (tiles_valid), no order, no begin_frame_counters (persist_last), counters in buffer 2.
int rr_camera_rays_device(rr_ctx* c, const rr_camera* cam, void* d_rays, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!c || !cam || !d_rays) return fail(RR_E_ARG, "rr_camera_rays_device: null argument");
    if (c->group) return fail(RR_E_ARG, "device-resident ray queries need a single-device context (no multi-device or virtual context)");
    if (cam->hsize < 1 || cam->vsize < 1) return fail(RR_E_ARG, "camera sizes must be >= 1");
    if (cam->hsize >= ((int64_t)1 << 32) || cam->vsize >= ((int64_t)1 << 32) ||
        cam->hsize * cam->vsize >= ((int64_t)1 << 32))
        return fail(RR_E_LIMIT, "a camera's rays must number fewer than 2^32");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    rr::LevelArgs A{};
    set_camera(A, cam);  // the frames' DevCamera and affine flag
    HIPCHK(rr::launch_camera_rays(A.cam, A.cam_affine != 0, cam->hsize * cam->vsize, static_cast<double*>(d_rays), st));
    HIPCHK(claim.release());
    return RR_OK;
}

// what the three queries refuse alike (n == 0 is the caller's early RR_OK, after these)
static int rays_check(const rr_ctx* c, int64_t n, bool null_buffer) {
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return fail(RR_E_ARG, "device-resident ray queries need a single-device context (no multi-device or virtual context)");
    if (n < 0) return fail(RR_E_ARG, "n is negative");
    if (n > 0 && null_buffer) return fail(RR_E_ARG, "null device buffer");
    if (!c->has_scene) return fail(RR_E_ARG, "no scene uploaded");
    if (n >= ((int64_t)1 << 32)) return fail(RR_E_LIMIT, "a ray batch must hold fewer than 2^32 rays");
    return RR_OK;
}
// the call's counters are the context's pending stats (rr_render_views_aov_device's pattern)
static void rays_stats_pending(rr_ctx* c, int64_t n) {
    c->stats_src = frame_counters(c, 2);
    c->stats_pending = true;
    c->last.samples = (uint64_t)n;
    c->adapt_pending = false;
}

int rr_color_at_device(rr_ctx* c, int64_t n, const void* d_rays, int32_t remaining, uint64_t seed, int32_t jitter_mode,
                       void* d_rgb, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = rays_check(c, n, !d_rays || !d_rgb);
    if (rc != RR_OK) return rc;
    if (remaining < 0 || remaining > RR_MAX_DEPTH) return fail(RR_E_LIMIT, "remaining out of range");
    if (n == 0) return RR_OK;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    c->frame_timed = true;
    HIPCHK(hipEventRecord(c->e0, st));
    const int saved_epoch = c->epoch;
    c->epoch = 2;  // the query buffer (frame buffers keep their state)
    HIPCHK(hipMemsetAsync(frame_counters(c, 2), 0, kCounterBytes, st));
    rr::LevelArgs A{};  // rr_color_at's level 0 on the caller's rays: sample i's jitter identity is (i, path 1)
    A.hs = 1;
    A.aa = 1;
    A.part = 0;
    A.nparts = 1;
    A.block_rows = 1;
    A.rays0 = static_cast<const double*>(d_rays);
    A.seed = seed;
    A.jitter_mode = jitter_mode;
    rc = run_levels(c, frame_facts(c, remaining), A, n, remaining, static_cast<double*>(d_rgb), st);
    c->epoch = saved_epoch;
    if (rc != RR_OK) return rc;
    HIPCHK(hipEventRecord(c->e1, st));
    HIPCHK(claim.release());
    rays_stats_pending(c, n);
    return RR_OK;
}

int rr_hit_at_device(rr_ctx* c, int64_t n, const void* d_rays, void* d_hits, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = rays_check(c, n, !d_rays || !d_hits);
    if (rc != RR_OK) return rc;
    if (n == 0) return RR_OK;
    const rr::RayPassPlan plan = rr::plan_ray_passes(n, c->batch);
    HIPCHK(hipSetDevice(c->device));
    // one pass's records as planes: RR_HIT_DOUBLES double planes, then the two int planes (never more than
    // kRayPassMax * 192 bytes, whatever n is)
    const size_t d_bytes = (size_t)plan.pass * rr::RR_HIT_DOUBLES * sizeof(double);
    HIPCHK(c->hitrec.ensure(d_bytes + (size_t)plan.pass * 2 * sizeof(int32_t)));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    c->frame_timed = true;
    HIPCHK(hipEventRecord(c->e0, st));
    HIPCHK(hipMemsetAsync(frame_counters(c, 2), 0, kCounterBytes, st));  // the query buffer (frame buffers keep their state)
    rr::HitOut O{};
    O.node_object = c->node_object.as<int32_t>();
    O.rec_d = c->hitrec.as<double>();
    O.rec_i = reinterpret_cast<int32_t*>(c->hitrec.as<char>() + d_bytes);
    O.stride = plan.pass;
    rr::LevelArgs A{};
    A.hs = 1;
    A.aa = 1;
    A.part = 0;
    A.nparts = 1;
    A.block_rows = 1;
    A.nseg = A.nseg_out = 1;
    A.counters = frame_counters(c, 2);
    A.base = 0;
    for (int64_t first = 0; first < n; first += plan.pass) {  // a pass: the planes of its rays, then their records
        const int64_t np = std::min<int64_t>(plan.pass, n - first);
        A.rays0 = static_cast<const double*>(d_rays) + 6 * first;
        A.n = np;
        set_level0_index(A);
        HIPCHK(rr::launch_hit(c->S, A, O, st));
        HIPCHK(rr::launch_hit_records(O, np, static_cast<char*>(d_hits) + sizeof(rr_hit) * (size_t)first, st));
    }
    HIPCHK(hipEventRecord(c->e1, st));
    HIPCHK(claim.release());
    rays_stats_pending(c, n);
    return RR_OK;
}

// ---- ordered ray batches (render_order.inc) ----
// The order of a batch is a permutation on the device; the two ordered queries walk the batch in it and answer ray i in
// slot i, as the plain entries do.  The isolation rule above holds for all three.
static int order_into(rr_ctx* c, int64_t n, const void* d_rays, uint32_t* perm, hipStream_t st) {
    HIPCHK(c->order_scratch.ensure(rr::ray_order_scratch_bytes(n)));
    HIPCHK(rr::launch_ray_order(static_cast<const double*>(d_rays), n, perm, c->order_scratch.p, st));
    return RR_OK;
}
// the order an ordered query walks: the caller's, or the library's own into the context's buffer (on st)
static int order_for(rr_ctx* c, int64_t n, const void* d_rays, const void* d_perm, hipStream_t st, const uint32_t** perm) {
    *perm = static_cast<const uint32_t*>(d_perm);
    if (d_perm) return RR_OK;
    HIPCHK(c->order_perm.ensure((size_t)n * sizeof(uint32_t)));
    *perm = c->order_perm.as<uint32_t>();
    return order_into(c, n, d_rays, c->order_perm.as<uint32_t>(), st);
}

int rr_ray_order_device(rr_ctx* c, int64_t n, const void* d_rays, void* d_perm, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return fail(RR_E_ARG, "device-resident ray queries need a single-device context (no multi-device or virtual context)");
    if (n < 0) return fail(RR_E_ARG, "n is negative");
    if (n > 0 && (!d_rays || !d_perm)) return fail(RR_E_ARG, "null device buffer");
    if (n >= ((int64_t)1 << 32)) return fail(RR_E_LIMIT, "a ray batch must hold fewer than 2^32 rays");
    if (n == 0) return RR_OK;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    int rc = order_into(c, n, d_rays, static_cast<uint32_t*>(d_perm), st);
    if (rc != RR_OK) return rc;
    HIPCHK(claim.release());
    return RR_OK;
}

int rr_color_at_device_ordered(rr_ctx* c, int64_t n, const void* d_rays, const void* d_perm, int32_t remaining,
                               uint64_t seed, int32_t jitter_mode, void* d_rgb, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = rays_check(c, n, !d_rays || !d_rgb);
    if (rc != RR_OK) return rc;
    if (remaining < 0 || remaining > RR_MAX_DEPTH) return fail(RR_E_LIMIT, "remaining out of range");
    if (n == 0) return RR_OK;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    c->frame_timed = true;
    HIPCHK(hipEventRecord(c->e0, st));
    const uint32_t* perm = nullptr;
    rc = order_for(c, n, d_rays, d_perm, st, &perm);
    if (rc != RR_OK) return rc;
    const int saved_epoch = c->epoch;
    c->epoch = 2;  // the query buffer (frame buffers keep their state)
    HIPCHK(hipMemsetAsync(frame_counters(c, 2), 0, kCounterBytes, st));
    rr::LevelArgs A{};  // rr_color_at_device's level 0 with slot t on ray perm[t]: its jitter identity is (perm[t], path 1)
    A.hs = 1;
    A.aa = 1;
    A.part = 0;
    A.nparts = 1;
    A.block_rows = 1;
    A.rays0 = static_cast<const double*>(d_rays);
    A.list = perm;
    A.seed = seed;
    A.jitter_mode = jitter_mode;
    rc = run_levels(c, frame_facts(c, remaining), A, n, remaining, static_cast<double*>(d_rgb), st);
    c->epoch = saved_epoch;
    if (rc != RR_OK) return rc;
    HIPCHK(hipEventRecord(c->e1, st));
    HIPCHK(claim.release());
    rays_stats_pending(c, n);
    return RR_OK;
}

int rr_hit_at_device_ordered(rr_ctx* c, int64_t n, const void* d_rays, const void* d_perm, void* d_hits,
                             void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = rays_check(c, n, !d_rays || !d_hits);
    if (rc != RR_OK) return rc;
    if (n == 0) return RR_OK;
    const rr::RayPassPlan plan = rr::plan_ray_passes(n, c->batch);
    HIPCHK(hipSetDevice(c->device));
    const size_t d_bytes = (size_t)plan.pass * rr::RR_HIT_DOUBLES * sizeof(double);
    HIPCHK(c->hitrec.ensure(d_bytes + (size_t)plan.pass * 2 * sizeof(int32_t)));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    c->frame_timed = true;
    HIPCHK(hipEventRecord(c->e0, st));
    const uint32_t* perm = nullptr;
    rc = order_for(c, n, d_rays, d_perm, st, &perm);
    if (rc != RR_OK) return rc;
    HIPCHK(hipMemsetAsync(frame_counters(c, 2), 0, kCounterBytes, st));  // the query buffer (frame buffers keep their state)
    rr::HitOut O{};
    O.node_object = c->node_object.as<int32_t>();
    O.rec_d = c->hitrec.as<double>();
    O.rec_i = reinterpret_cast<int32_t*>(c->hitrec.as<char>() + d_bytes);
    O.stride = plan.pass;
    rr::LevelArgs A{};
    A.hs = 1;
    A.aa = 1;
    A.part = 0;
    A.nparts = 1;
    A.block_rows = 1;
    A.nseg = A.nseg_out = 1;
    A.counters = frame_counters(c, 2);
    A.base = 0;
    A.rays0 = static_cast<const double*>(d_rays);  // the whole batch: a pass's slots read rays anywhere in it
    for (int64_t first = 0; first < n; first += plan.pass) {  // a pass: positions [first, first + np) of the order
        const int64_t np = std::min<int64_t>(plan.pass, n - first);
        A.list = perm + first;
        A.n = np;
        set_level0_index(A);
        HIPCHK(rr::launch_hit_ordered(c->S, A, O, st));
        HIPCHK(rr::launch_hit_records_ordered(O, np, perm + first, d_hits, st));
    }
    HIPCHK(hipEventRecord(c->e1, st));
    HIPCHK(claim.release());
    rays_stats_pending(c, n);
    return RR_OK;
}

int rr_is_shadowed_device(rr_ctx* c, int64_t n, const void* d_points, const void* d_light_positions, void* d_out,
                          void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = rays_check(c, n, !d_points || !d_light_positions || !d_out);
    if (rc != RR_OK) return rc;
    if (n == 0) return RR_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->shadow_sink.ensure(kCounterBytes));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    HIPCHK(rr::launch_shadow_query(c->S, static_cast<const double*>(d_points), static_cast<const double*>(d_light_positions),
                                   n, static_cast<int32_t*>(d_out), c->shadow_sink.as<unsigned long long>(), st));
    HIPCHK(claim.release());
    return RR_OK;
}

// ---- lens frames (render_lens.inc) ----
// S rays per pixel from lens_rays_kernel, traced by the colour families' rays0 path a pass of whole pixels at a time and
// summed per pixel by lens_resolve_kernel.  The isolation rule of the ray queries holds: counters in buffer 2, no frame
// state touched.
int rr_camera_inverse(const rr_camera* cam, double inv[16]) {
    if (!cam || !inv) return fail(RR_E_ARG, "rr_camera_inverse: null argument");
    const rr::DevCamera d = dev_camera(cam);
    for (int i = 0; i < 16; ++i) inv[i] = d.inv[i];
    return RR_OK;
}

// what the lens entries refuse of the camera and the lens alike; fills the kernel's argument
static int lens_check(const rr_camera* cam, const rr_lens* lens, rr::DevLens* L) {
    if (!cam || !lens) return fail(RR_E_ARG, "lens frames: null camera / lens");
    if (lens->samples < 1 || lens->samples > RR_MAX_LENS_SAMPLES)
        return fail(RR_E_ARG, "lens samples must be in 1.." + std::to_string(RR_MAX_LENS_SAMPLES));
    if (!(std::isfinite(lens->aperture) && lens->aperture >= 0.0)) return fail(RR_E_ARG, "the aperture must be finite and >= 0");
    if (lens->aperture > 0.0 && !(std::isfinite(lens->focal_distance) && lens->focal_distance > 0.0))
        return fail(RR_E_ARG, "the focal distance of a thin lens must be finite and > 0");
    if (cam->hsize < 1 || cam->vsize < 1) return fail(RR_E_ARG, "camera sizes must be >= 1");
    if (cam->hsize >= ((int64_t)1 << 32) || cam->vsize >= ((int64_t)1 << 32) ||
        cam->hsize * cam->vsize >= ((int64_t)1 << 32) || cam->hsize * cam->vsize * lens->samples >= ((int64_t)1 << 32))
        return fail(RR_E_LIMIT, "a lens frame's rays (W * H * samples) must number fewer than 2^32");
    rr::LevelArgs A{};
    set_camera(A, cam);  // the frames' DevCamera and affine flag
    if (!A.cam_affine) return fail(RR_E_NONAFFINE, "lens frames need a camera whose inverse is affine (last row 0, 0, 0, 1)");
    for (int i = 0; i < 12; ++i) L->inv[i] = A.cam.inv[i];
    L->half_width = A.cam.half_width;
    L->half_height = A.cam.half_height;
    L->pixel_size = A.cam.pixel_size;
    L->aperture = lens->aperture;
    L->focal_distance = lens->aperture > 0.0 ? lens->focal_distance : 1.0;
    L->seed = lens->seed;
    L->samples = (uint32_t)lens->samples;
    L->width = (uint32_t)cam->hsize;
    L->pixel_jitter = lens->pixel_jitter ? 1 : 0;
    L->pad = 0;
    return RR_OK;
}

int rr_lens_rays_device(rr_ctx* c, const rr_camera* cam, const rr_lens* lens, int64_t first_pixel, int64_t n_pixels,
                        void* d_rays, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!c || !d_rays) return fail(RR_E_ARG, "rr_lens_rays_device: null argument");
    if (c->group) return fail(RR_E_ARG, "lens frames need a single-device context (no multi-device or virtual context)");
    rr::DevLens L{};
    int rc = lens_check(cam, lens, &L);
    if (rc != RR_OK) return rc;
    if (first_pixel < 0 || n_pixels < 0 || first_pixel > cam->hsize * cam->vsize ||
        n_pixels > cam->hsize * cam->vsize - first_pixel)
        return fail(RR_E_ARG, "the pixel window [first_pixel, first_pixel + n_pixels) must lie inside the frame");
    if (n_pixels == 0) return RR_OK;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    HIPCHK(rr::launch_lens_rays(L, first_pixel * L.samples, n_pixels * L.samples, static_cast<double*>(d_rays), st));
    HIPCHK(claim.release());
    return RR_OK;
}

// what both frame entries refuse before they look at the context
static int lens_frame_check(const rr_camera* cam, const rr_render_opts* o, const rr_lens* lens, const void* avg,
                            rr::DevLens* L) {
    if (!cam || !o || !lens || !avg) return fail(RR_E_ARG, "rr_render_lens: null argument");
    if (o->aa != 1) return fail(RR_E_ARG, "lens frames take opts->aa == 1: the lens samples take aa's place");
    if (o->part != 0 || o->nparts != 1 || o->row_begin != 0 || o->row_end != 0)
        return fail(RR_E_ARG, "lens frames are whole frames: part 0 of 1, no band");
    if (o->flags & ~RR_NO_FRAME_TIMING) return fail(RR_E_ARG, "lens frames take no flag but RR_NO_FRAME_TIMING");
    if (o->max_depth < 0 || o->max_depth > RR_MAX_DEPTH) return fail(RR_E_LIMIT, "max_depth out of range");
    return lens_check(cam, lens, L);
}

int rr_render_lens_device(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, const rr_lens* lens, void* d_avg,
                          void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    rr::DevLens L{};
    int rc = lens_frame_check(cam, o, lens, d_avg, &L);
    if (rc != RR_OK) return rc;
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return fail(RR_E_ARG, "lens frames need a single-device context (no multi-device or virtual context)");
    if (!c->has_scene) return fail(RR_E_ARG, "no scene uploaded");
    const int64_t S = lens->samples, n_pixels = cam->hsize * cam->vsize;
    const rr::LensPassPlan plan = rr::plan_lens_passes(n_pixels, lens->samples, c->lens_pass);
    const int64_t pass_rays = std::min(plan.pixels, n_pixels) * S;
    const FrameFacts facts = frame_facts(c, o->max_depth);
    HIPCHK(hipSetDevice(c->device));
    // one pass's rays and colours (grown on demand, as rr_hit_at_device's planes)
    HIPCHK(c->lens_rays.ensure((size_t)pass_rays * 6 * sizeof(double)));
    HIPCHK(c->lens_rgb.ensure((size_t)pass_rays * 3 * sizeof(double)));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    c->frame_timed = !(o->flags & RR_NO_FRAME_TIMING);
    if (c->frame_timed) HIPCHK(hipEventRecord(c->e0, st));
    const int saved_epoch = c->epoch;
    c->epoch = 2;  // the query buffer (frame buffers keep their state), zeroed once per frame
    HIPCHK(hipMemsetAsync(frame_counters(c, 2), 0, kCounterBytes, st));
    rr::LevelArgs A{};  // rr_color_at_device's level 0: sample i's jitter identity is (i, path 1)
    A.hs = 1;
    A.aa = 1;
    A.part = 0;
    A.nparts = 1;
    A.block_rows = 1;
    A.seed = o->seed;
    A.jitter_mode = o->jitter_mode;
    double* const rays = c->lens_rays.as<double>();
    double* const rgb = c->lens_rgb.as<double>();
    for (int64_t first = 0; first < n_pixels && rc == RR_OK; first += plan.pixels) {
        const int64_t np = std::min(plan.pixels, n_pixels - first), r0 = first * S;
        hipError_t e = rr::launch_lens_rays(L, r0, np * S, rays, st);
        if (e != hipSuccess) {
            rc = fail(RR_E_HIP, std::string("launch_lens_rays: ") + hipGetErrorString(e));
            break;
        }
        // The pass's events are the frame's r0 .. r0 + np * S: the kernels index the rays, the sample identity and the
        // output slot by base + lane, so the scratch pointers are biased by -r0 entries and never dereferenced outside
        // the pass (integer arithmetic: the biased addresses may lie below the allocations).
        A.rays0 = reinterpret_cast<const double*>(reinterpret_cast<uintptr_t>(rays) - (uintptr_t)r0 * 6 * sizeof(double));
        double* out = reinterpret_cast<double*>(reinterpret_cast<uintptr_t>(rgb) - (uintptr_t)r0 * 3 * sizeof(double));
        rc = run_levels(c, facts, A, np * S, o->max_depth, out, st, nullptr, 0, 0, nullptr, r0);
        if (rc != RR_OK) break;
        e = rr::launch_lens_resolve(rgb, lens->samples, np, static_cast<double*>(d_avg) + 3 * first, st);
        if (e != hipSuccess) rc = fail(RR_E_HIP, std::string("launch_lens_resolve: ") + hipGetErrorString(e));
    }
    c->epoch = saved_epoch;
    if (rc != RR_OK) return rc;
    if (c->frame_timed) HIPCHK(hipEventRecord(c->e1, st));
    HIPCHK(claim.release());
    rays_stats_pending(c, n_pixels * S);
    return RR_OK;
}

int rr_render_lens(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, const rr_lens* lens, double* out_avg,
                   rr_stats* stats) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    rr::DevLens L{};
    int rc = lens_frame_check(cam, o, lens, out_avg, &L);
    if (rc != RR_OK) return rc;
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return fail(RR_E_ARG, "lens frames need a single-device context (no multi-device or virtual context)");
    if (!c->has_scene) return fail(RR_E_ARG, "no scene uploaded");
    const size_t img = (size_t)(cam->hsize * cam->vsize) * 3 * sizeof(double);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->qout.ensure(img));
    rc = rr_render_lens_device(c, cam, o, lens, c->qout.p, nullptr);
    if (rc != RR_OK) return rc;
    HIPCHK(hipMemcpyAsync(out_avg, c->qout.p, img, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    rr_stats local;
    rc = rr_last_stats(c, stats ? stats : &local);
    if (rc != RR_OK) return rc;
    const uint64_t nan = (stats ? stats : &local)->nan_rays;
    return nan ? nan_fail(nan) : RR_OK;
}

// ---- ambient occlusion (render_ao.inc, ao_dir.hpp) ----
// K occlusion segments per point, one lane each (ao_pairs_kernel), counted per point and resolved to (K - c) / K.  The
// isolation rule of the ray queries holds: the query counts into the shadow sink, the frame into buffer 2, and neither
// touches the frames' state.
static_assert(sizeof(rr_ao) == 24, "rr_ao is 24 bytes (rray.h)");

// what every AO entry refuses of the parameters; fills the kernel's argument
static int ao_check(const rr_ao* ao, rr::DevAo* P) {
    if (!ao) return fail(RR_E_ARG, "ambient occlusion: null rr_ao");
    if (ao->samples < 1 || ao->samples > RR_MAX_AO_SAMPLES)
        return fail(RR_E_ARG, "ambient-occlusion samples must be in 1.." + std::to_string(RR_MAX_AO_SAMPLES));
    if (ao->reserved != 0) return fail(RR_E_ARG, "rr_ao.reserved must be 0");
    if (!(std::isfinite(ao->radius) && ao->radius > 0.0)) return fail(RR_E_ARG, "the ambient-occlusion radius must be finite and > 0");
    P->radius = ao->radius;
    P->seed = ao->seed;
    P->samples = (uint32_t)ao->samples;
    P->pad = 0;
    return RR_OK;
}

int rr_ao_directions(const rr_ao* ao, int64_t first, int64_t n, const double* normals, double* out_w) {
    rr::DevAo P{};
    int rc = ao_check(ao, &P);
    if (rc != RR_OK) return rc;
    if (first < 0 || n < 0) return fail(RR_E_ARG, "rr_ao_directions: first and n must be >= 0");
    if (n > 0 && (!normals || !out_w)) return fail(RR_E_ARG, "rr_ao_directions: null argument");
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t base = rr::ao_base(P.seed, (uint64_t)(first + i));
        for (uint32_t k = 0; k < P.samples; ++k)
            rr::ao_direction(base, k, normals + 3 * i, out_w + 3 * ((size_t)i * P.samples + k));
    }
    return RR_OK;
}

int rr_ao_at_device(rr_ctx* c, int64_t n, const void* d_points, const void* d_normals, const rr_ao* ao, void* d_ao,
                    void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    rr::DevAo P{};
    int rc = ao_check(ao, &P);
    if (rc != RR_OK) return rc;
    rc = rays_check(c, n, !d_points || !d_normals || !d_ao);
    if (rc != RR_OK) return rc;
    if (n * (int64_t)P.samples >= ((int64_t)1 << 32))
        return fail(RR_E_LIMIT, "an ambient-occlusion batch must hold fewer than 2^32 pairs (n * samples)");
    if (n == 0) return RR_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->shadow_sink.ensure(kCounterBytes));
    HIPCHK(c->ao_count.ensure((size_t)n * sizeof(int32_t)));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    const rr::AoPoints I{static_cast<const double*>(d_points), static_cast<const double*>(d_normals), 3, 1, nullptr, 0};
    HIPCHK(rr::launch_ao_pairs(c->S, P, I, n, c->ao_count.as<int32_t>(), c->shadow_sink.as<unsigned long long>(), st));
    HIPCHK(rr::launch_ao_resolve(c->ao_count.as<int32_t>(), ao->samples, n, static_cast<double*>(d_ao), st));
    HIPCHK(claim.release());
    return RR_OK;
}

// what both frame entries refuse before they look at the context
static int ao_frame_check(const rr_camera* cam, const rr_render_opts* o, const rr_ao* ao, const void* out, rr::DevAo* P) {
    if (!cam || !o || !out) return fail(RR_E_ARG, "rr_render_ao: null argument");
    return ao_check(ao, P);
}

int rr_render_ao_device(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, const rr_ao* ao, void* d_ao,
                        void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    rr::DevAo P{};
    int rc = ao_frame_check(cam, o, ao, d_ao, &P);
    if (rc != RR_OK) return rc;
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return fail(RR_E_ARG, "ambient-occlusion frames need a single-device context (no multi-device or virtual context)");
    if (!c->has_scene) return fail(RR_E_ARG, "no scene uploaded");
    rr_render_opts opts = *o;
    opts.max_depth = 0;  // ignored here (as seed, jitter_mode and flags): no recursion in an occlusion frame
    rc = check_opts(cam, &opts);
    if (rc != RR_OK) return rc;
    if (o->part != 0 || o->nparts != 1 || o->row_begin != 0 || o->row_end != 0)
        return fail(RR_E_ARG, "ambient-occlusion frames are whole frames: part 0 of 1, no band");
    const int64_t total = cam->hsize * cam->vsize;
    if (total >= ((int64_t)1 << 31)) return fail(RR_E_LIMIT, "an ambient-occlusion frame must hold fewer than 2^31 samples");
    const rr::AoPassPlan plan = rr::plan_ao_passes(total, ao->samples, c->batch, c->ao_pass);
    const int64_t pass = std::min(plan.points, total);
    HIPCHK(hipSetDevice(c->device));
    // one pass's camera rays, first-hit planes (RR_HIT_DOUBLES double planes, then the two int planes) and counts
    const size_t d_bytes = (size_t)pass * rr::RR_HIT_DOUBLES * sizeof(double);
    HIPCHK(c->ao_rays.ensure((size_t)pass * 6 * sizeof(double)));
    HIPCHK(c->hitrec.ensure(d_bytes + (size_t)pass * 2 * sizeof(int32_t)));
    HIPCHK(c->ao_count.ensure((size_t)pass * sizeof(int32_t)));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    c->frame_timed = true;
    HIPCHK(hipEventRecord(c->e0, st));
    HIPCHK(hipMemsetAsync(frame_counters(c, 2), 0, kCounterBytes, st));  // the query buffer (frame buffers keep their state)
    rr::HitOut O{};
    O.node_object = c->node_object.as<int32_t>();
    O.rec_d = c->hitrec.as<double>();
    O.rec_i = reinterpret_cast<int32_t*>(c->hitrec.as<char>() + d_bytes);
    O.stride = pass;
    rr::LevelArgs C{};
    set_camera(C, cam);  // the frames' DevCamera and affine flag
    rr::LevelArgs A{};   // rr_hit_at_device's level 0 on the pass's rays
    A.hs = 1;
    A.aa = 1;
    A.part = 0;
    A.nparts = 1;
    A.block_rows = 1;
    A.nseg = A.nseg_out = 1;
    A.counters = frame_counters(c, 2);
    A.base = 0;
    A.rays0 = c->ao_rays.as<double>();
    // over_point and normalv are planes 12..14 and 9..11 of the records (HitOut.rec_d), object the first int plane
    const rr::AoPoints planes{O.rec_d + 12 * pass, O.rec_d + 9 * pass, 1, pass, O.rec_i, 0};
    for (int64_t first = 0; first < total; first += plan.points) {
        const int64_t np = std::min(plan.points, total - first);
        HIPCHK(rr::launch_camera_rays_window(C.cam, C.cam_affine != 0, first, np, c->ao_rays.as<double>(), st));
        A.n = np;
        set_level0_index(A);
        HIPCHK(rr::launch_hit(c->S, A, O, st));
        rr::AoPoints I = planes;
        I.first = first;
        HIPCHK(rr::launch_ao_pairs(c->S, P, I, np, c->ao_count.as<int32_t>(), frame_counters(c, 2), st));
        HIPCHK(rr::launch_ao_resolve(c->ao_count.as<int32_t>(), ao->samples, np, static_cast<double*>(d_ao) + first, st));
    }
    HIPCHK(hipEventRecord(c->e1, st));
    HIPCHK(claim.release());
    rays_stats_pending(c, total);
    return RR_OK;
}

int rr_render_ao(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, const rr_ao* ao, double* out_ao,
                 rr_stats* stats) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    rr::DevAo P{};
    int rc = ao_frame_check(cam, o, ao, out_ao, &P);
    if (rc != RR_OK) return rc;
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return fail(RR_E_ARG, "ambient-occlusion frames need a single-device context (no multi-device or virtual context)");
    if (!c->has_scene) return fail(RR_E_ARG, "no scene uploaded");
    if (cam->hsize <= 0 || cam->vsize <= 0 || cam->hsize > (1ll << 31) || cam->vsize > (1ll << 31))
        return fail(RR_E_ARG, "bad camera size");
    const size_t img = (size_t)cam->hsize * (size_t)cam->vsize * sizeof(double);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->qout.ensure(img));
    rc = rr_render_ao_device(c, cam, o, ao, c->qout.p, nullptr);
    if (rc != RR_OK) return rc;
    HIPCHK(hipMemcpyAsync(out_ao, c->qout.p, img, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    rr_stats local;
    rc = rr_last_stats(c, stats ? stats : &local);
    if (rc != RR_OK) return rc;
    const uint64_t nan = (stats ? stats : &local)->nan_rays;
    return nan ? nan_fail(nan) : RR_OK;
}

// ---- the edge-avoiding denoiser (render_denoise.inc, denoise_tap.hpp) ----
// One pack kernel per call and one level kernel per iteration, through two context-owned images.  It reads no scene and
// counts nothing: frame state and pending stats stay as they are.
static_assert(sizeof(rr_denoise_desc) == 40, "rr_denoise_desc is 40 bytes (rray.h)");

namespace {
struct DnPlanes {
    const void *in, *depth, *normal, *object, *albedo;
    void* out;
};
bool dn_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + nb && y < x + na;
}
}  // namespace

// what every denoiser entry refuses of its arguments (the context apart); fills the terms that are switched on
static int dn_check(const rr_denoise_desc* d, int64_t W, int64_t H, int32_t C, const DnPlanes& P, int32_t* terms,
                    const std::string& who = "rr_denoise") {
    if (!d || !P.in || !P.out) return fail(RR_E_ARG, who + ": null argument");
    if (C != 1 && C != 3) return fail(RR_E_ARG, who + ": channels must be 1 or 3");
    if (W < 1 || H < 1) return fail(RR_E_ARG, who + ": width and height must be >= 1");
    if (d->iterations < 1 || d->iterations > RR_MAX_DENOISE_ITERATIONS)
        return fail(RR_E_ARG, who + ": iterations must be in 1.." + std::to_string(RR_MAX_DENOISE_ITERATIONS));
    if (d->flags & ~RR_DN_OBJECT) return fail(RR_E_ARG, who + ": unknown flag bits");
    for (double s : {d->sigma_color, d->sigma_normal, d->sigma_depth, d->sigma_albedo})
        if (!(std::isfinite(s) && s >= 0.0)) return fail(RR_E_ARG, who + ": every sigma must be finite and >= 0");
    int32_t t = 0;
    if (d->flags & RR_DN_OBJECT) t |= rr::DN_T_OBJECT;
    if (d->sigma_color > 0.0) t |= rr::DN_T_COLOR;
    if (d->sigma_normal > 0.0) t |= rr::DN_T_NORMAL;
    if (d->sigma_depth > 0.0) t |= rr::DN_T_DEPTH;
    if (d->sigma_albedo > 0.0) t |= rr::DN_T_ALBEDO;
    if (((t & rr::DN_T_OBJECT) && !P.object) || ((t & rr::DN_T_NORMAL) && !P.normal) ||
        ((t & rr::DN_T_DEPTH) && !P.depth) || ((t & rr::DN_T_ALBEDO) && !P.albedo))
        return fail(RR_E_ARG, who + ": a term that is switched on needs its plane");
    if (W > (((int64_t)1 << 31) - 1) / H) return fail(RR_E_LIMIT, "a denoised frame must hold fewer than 2^31 pixels");
    const size_t n = (size_t)(W * H), img = n * (size_t)C * sizeof(double);
    if (dn_overlap(P.out, img, P.in, img) || dn_overlap(P.out, img, P.depth, n * sizeof(double)) ||
        dn_overlap(P.out, img, P.normal, n * 3 * sizeof(double)) || dn_overlap(P.out, img, P.object, n * sizeof(int32_t)) ||
        dn_overlap(P.out, img, P.albedo, n * 3 * sizeof(double)))
        return fail(RR_E_ARG, who + ": out overlaps an input");
    *terms = t;
    return RR_OK;
}

static void dn_reference_level(const rr::DnLevel& L, int64_t W, int64_t H, int32_t C, const double* src,
                               const rr::DnGuide* g, double* dst) {
    for (int64_t y = 0; y < H; ++y)
        for (int64_t x = 0; x < W; ++x) {
            if (C == 3)
                rr::dn_pixel<3>(L, W, H, x, y, src, g, dst + 3 * (y * W + x));
            else
                rr::dn_pixel<1>(L, W, H, x, y, src, g, dst + (y * W + x));
        }
}

int rr_denoise_reference(const rr_denoise_desc* d, int64_t W, int64_t H, int32_t C, const double* in, const double* depth,
                         const double* normal, const int32_t* object, const double* albedo, double* out) {
    int32_t terms = 0;
    int rc = dn_check(d, W, H, C, DnPlanes{in, depth, normal, object, albedo, out}, &terms);
    if (rc != RR_OK) return rc;
    const int64_t n = W * H;
    std::vector<rr::DnGuide> g((size_t)n);
    for (int64_t p = 0; p < n; ++p) g[(size_t)p] = rr::dn_guide(p, depth, normal, object, albedo);
    std::vector<double> a, b;
    if (d->iterations > 1) a.resize((size_t)n * C);
    if (d->iterations > 2) b.resize((size_t)n * C);
    const double* src = in;
    for (int32_t i = 0; i < d->iterations; ++i) {
        double* dst = i == d->iterations - 1 ? out : (i & 1 ? b.data() : a.data());
        const rr::DnLevel L = rr::dn_level(terms, i, d->sigma_color, d->sigma_normal, d->sigma_depth, d->sigma_albedo);
        dn_reference_level(L, W, H, C, src, g.data(), dst);
        src = dst;
    }
    return RR_OK;
}

static int dn_ctx_check(const rr_ctx* c, const std::string& who = "rr_denoise") {
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return fail(RR_E_ARG, who + " needs a single-device context (no multi-device or virtual context)");
    return RR_OK;
}

int rr_denoise_device(rr_ctx* c, const rr_denoise_desc* d, int64_t W, int64_t H, int32_t C, const void* d_in,
                      const void* d_depth, const void* d_normal, const void* d_object, const void* d_albedo, void* d_out,
                      void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = dn_ctx_check(c);
    if (rc != RR_OK) return rc;
    int32_t terms = 0;
    rc = dn_check(d, W, H, C, DnPlanes{d_in, d_depth, d_normal, d_object, d_albedo, d_out}, &terms);
    if (rc != RR_OK) return rc;
    const int64_t n = W * H;
    const size_t img = (size_t)n * (size_t)C * sizeof(double);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    // the scratch is claimed before it may grow: a call on another stream may still read the buffers that ensure frees
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    if (c->dn_guides.bytes < (size_t)n * sizeof(rr::DnGuide) || (d->iterations > 1 && c->dn_img[0].bytes < img) ||
        (d->iterations > 2 && c->dn_img[1].bytes < img))
        HIPCHK(hipStreamSynchronize(st));  // growing frees: nothing enqueued may still use the old buffers
    HIPCHK(c->dn_guides.ensure((size_t)n * sizeof(rr::DnGuide)));
    if (d->iterations > 1) HIPCHK(c->dn_img[0].ensure(img));
    if (d->iterations > 2) HIPCHK(c->dn_img[1].ensure(img));
    rr::DnGuide* g = c->dn_guides.as<rr::DnGuide>();
    HIPCHK(rr::launch_denoise_pack(n, static_cast<const double*>(d_depth), static_cast<const double*>(d_normal),
                                   static_cast<const int32_t*>(d_object), static_cast<const double*>(d_albedo), g, st));
    const double* src = static_cast<const double*>(d_in);
    const int32_t lds_step = c->dn_lds_step >= 0 ? c->dn_lds_step : (C == 1 ? 2 : 1);
    for (int32_t i = 0; i < d->iterations; ++i) {
        double* dst = i == d->iterations - 1 ? static_cast<double*>(d_out) : c->dn_img[i & 1].as<double>();
        const rr::DnLevel L = rr::dn_level(terms, i, d->sigma_color, d->sigma_normal, d->sigma_depth, d->sigma_albedo);
        HIPCHK(rr::launch_denoise_level(L, L.step <= lds_step, C, W, H, src, g, dst, st));
        src = dst;
    }
    HIPCHK(claim.release());
    return RR_OK;
}

int rr_denoise(rr_ctx* c, const rr_denoise_desc* d, int64_t W, int64_t H, int32_t C, const double* in, const double* depth,
               const double* normal, const int32_t* object, const double* albedo, double* out) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = dn_ctx_check(c);
    if (rc != RR_OK) return rc;
    int32_t terms = 0;
    rc = dn_check(d, W, H, C, DnPlanes{in, depth, normal, object, albedo, out}, &terms);
    if (rc != RR_OK) return rc;
    const size_t n = (size_t)(W * H);
    // one device block: out, in, then the planes that are given, each 256-byte aligned
    const void* host[5] = {in, depth, normal, object, albedo};
    const size_t bytes[5] = {n * C * sizeof(double), n * sizeof(double), n * 3 * sizeof(double), n * sizeof(int32_t),
                             n * 3 * sizeof(double)};
    size_t off[6], total = (bytes[0] + 255) & ~(size_t)255;  // out first
    for (int k = 0; k < 5; ++k) {
        off[k] = total;
        if (host[k]) total += (bytes[k] + 255) & ~(size_t)255;
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_ctx(c));  // dn_host may grow, and a call on another stream may still read it
    HIPCHK(c->dn_host.ensure(total));
    char* base = c->dn_host.as<char>();
    const void* dev[5];
    for (int k = 0; k < 5; ++k) {
        dev[k] = host[k] ? base + off[k] : nullptr;
        if (host[k]) HIPCHK(hipMemcpyAsync(base + off[k], host[k], bytes[k], hipMemcpyHostToDevice, c->stream));
    }
    rc = rr_denoise_device(c, d, W, H, C, dev[0], dev[1], dev[2], dev[3], dev[4], base, nullptr);
    if (rc != RR_OK) return rc;
    HIPCHK(hipMemcpyAsync(out, base, bytes[0], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return RR_OK;
}

// ---- variance-guided denoising (render_denoise_var.inc, denoise_var_tap.hpp) ----
// rr_variance: one pack kernel and one variance kernel.  rr_denoise_var: one pack kernel and one level kernel per
// iteration, the images through dn_img[2] as in rr_denoise and the variance planes through dv_var[2].  Neither reads a
// scene or counts anything: frame state and pending stats stay as they are.
static_assert(sizeof(rr_variance_desc) == 32, "rr_variance_desc is 32 bytes (rray.h)");
static_assert(sizeof(rr_denoise_var_desc) == 48, "rr_denoise_var_desc is 48 bytes (rray.h)");

namespace {
struct VarPlanes {
    const void *in, *m2, *count, *depth, *normal, *object, *albedo;
    void* var;
};
}  // namespace

// what every rr_variance entry refuses of its arguments (the context apart); fills the guide terms that are switched on
static int var_check(const rr_variance_desc* d, int64_t W, int64_t H, int32_t C, const VarPlanes& P, int32_t* terms) {
    if (!d || !P.in || !P.var) return fail(RR_E_ARG, "rr_variance: null argument");
    if (C != 1 && C != 3) return fail(RR_E_ARG, "rr_variance: channels must be 1 or 3");
    if (W < 1 || H < 1) return fail(RR_E_ARG, "rr_variance: width and height must be >= 1");
    if (d->flags & ~RR_DN_OBJECT) return fail(RR_E_ARG, "rr_variance: unknown flag bits");
    if (d->min_history < 0 || d->min_history > RR_MAX_TEMPORAL_HISTORY)
        return fail(RR_E_ARG, "rr_variance: min_history must be in 0.." + std::to_string(RR_MAX_TEMPORAL_HISTORY));
    for (double s : {d->sigma_normal, d->sigma_depth, d->sigma_albedo})
        if (!(std::isfinite(s) && s >= 0.0)) return fail(RR_E_ARG, "rr_variance: every sigma must be finite and >= 0");
    if ((P.m2 != nullptr) != (P.count != nullptr)) return fail(RR_E_ARG, "rr_variance: m2 and count go together");
    int32_t t = 0;
    if (d->flags & RR_DN_OBJECT) t |= rr::DN_T_OBJECT;
    if (d->sigma_normal > 0.0) t |= rr::DN_T_NORMAL;
    if (d->sigma_depth > 0.0) t |= rr::DN_T_DEPTH;
    if (d->sigma_albedo > 0.0) t |= rr::DN_T_ALBEDO;
    if (((t & rr::DN_T_OBJECT) && !P.object) || ((t & rr::DN_T_NORMAL) && !P.normal) ||
        ((t & rr::DN_T_DEPTH) && !P.depth) || ((t & rr::DN_T_ALBEDO) && !P.albedo))
        return fail(RR_E_ARG, "rr_variance: a term that is switched on needs its plane");
    if (W > (((int64_t)1 << 31) - 1) / H) return fail(RR_E_LIMIT, "a variance plane must hold fewer than 2^31 pixels");
    const size_t n = (size_t)(W * H), img = n * (size_t)C * sizeof(double), vb = n * sizeof(double);
    if (dn_overlap(P.var, vb, P.in, img) || dn_overlap(P.var, vb, P.m2, img) || dn_overlap(P.var, vb, P.count, n * sizeof(int32_t)) ||
        dn_overlap(P.var, vb, P.depth, n * sizeof(double)) || dn_overlap(P.var, vb, P.normal, n * 3 * sizeof(double)) ||
        dn_overlap(P.var, vb, P.object, n * sizeof(int32_t)) || dn_overlap(P.var, vb, P.albedo, n * 3 * sizeof(double)))
        return fail(RR_E_ARG, "rr_variance: var overlaps an input");
    *terms = t;
    return RR_OK;
}

int rr_variance_reference(const rr_variance_desc* d, int64_t W, int64_t H, int32_t C, const double* in, const double* m2,
                          const int32_t* count, const double* depth, const double* normal, const int32_t* object,
                          const double* albedo, double* var) {
    int32_t terms = 0;
    int rc = var_check(d, W, H, C, VarPlanes{in, m2, count, depth, normal, object, albedo, var}, &terms);
    if (rc != RR_OK) return rc;
    const int64_t n = W * H;
    std::vector<rr::DnGuide> g((size_t)n);
    for (int64_t p = 0; p < n; ++p) g[(size_t)p] = rr::dn_guide(p, depth, normal, object, albedo);
    const rr::DnLevel G = rr::dv_guide_level(terms, 1, d->sigma_normal, d->sigma_depth, d->sigma_albedo);
    for (int64_t y = 0; y < H; ++y)
        for (int64_t x = 0; x < W; ++x)
            var[y * W + x] = C == 3 ? rr::dv_variance<3>(G, d->min_history, W, H, x, y, in, g.data(), m2, count)
                                    : rr::dv_variance<1>(G, d->min_history, W, H, x, y, in, g.data(), m2, count);
    return RR_OK;
}

int rr_variance_device(rr_ctx* c, const rr_variance_desc* d, int64_t W, int64_t H, int32_t C, const void* d_in,
                       const void* d_m2, const void* d_count, const void* d_depth, const void* d_normal,
                       const void* d_object, const void* d_albedo, void* d_var, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = dn_ctx_check(c, "rr_variance");
    if (rc != RR_OK) return rc;
    int32_t terms = 0;
    rc = var_check(d, W, H, C, VarPlanes{d_in, d_m2, d_count, d_depth, d_normal, d_object, d_albedo, d_var}, &terms);
    if (rc != RR_OK) return rc;
    const int64_t n = W * H;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    // the scratch is claimed before it may grow: a call on another stream may still read the buffers that ensure frees
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    if (c->dn_guides.bytes < (size_t)n * sizeof(rr::DnGuide))
        HIPCHK(hipStreamSynchronize(st));  // growing frees: nothing enqueued may still use the old buffer
    HIPCHK(c->dn_guides.ensure((size_t)n * sizeof(rr::DnGuide)));
    rr::DnGuide* g = c->dn_guides.as<rr::DnGuide>();
    HIPCHK(rr::launch_denoise_pack(n, static_cast<const double*>(d_depth), static_cast<const double*>(d_normal),
                                   static_cast<const int32_t*>(d_object), static_cast<const double*>(d_albedo), g, st));
    const rr::DnLevel G = rr::dv_guide_level(terms, 1, d->sigma_normal, d->sigma_depth, d->sigma_albedo);
    HIPCHK(rr::launch_variance(G, d->min_history, C, W, H, static_cast<const double*>(d_in), static_cast<const double*>(d_m2),
                               static_cast<const int32_t*>(d_count), g, static_cast<double*>(d_var), st));
    HIPCHK(claim.release());
    return RR_OK;
}

// The blocking entries' device block in dn_host: the outputs first, then the inputs that are given, each 256-byte
// aligned.  Copies the inputs on the context's stream; dev[k] is null where host[k] is.
static int dv_stage(rr_ctx* c, int n_planes, int n_out, void* const* host, const size_t* bytes, void** dev) {
    size_t off[16], total = 0;
    for (int k = 0; k < n_planes; ++k) {
        off[k] = total;
        if (host[k]) total += (bytes[k] + 255) & ~(size_t)255;
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_ctx(c));  // dn_host may grow, and a call on another stream may still read it
    HIPCHK(c->dn_host.ensure(total));
    char* base = c->dn_host.as<char>();
    for (int k = 0; k < n_planes; ++k) {
        dev[k] = host[k] ? base + off[k] : nullptr;
        if (k >= n_out && host[k]) HIPCHK(hipMemcpyAsync(dev[k], host[k], bytes[k], hipMemcpyHostToDevice, c->stream));
    }
    return RR_OK;
}

int rr_variance(rr_ctx* c, const rr_variance_desc* d, int64_t W, int64_t H, int32_t C, const double* in, const double* m2,
                const int32_t* count, const double* depth, const double* normal, const int32_t* object, const double* albedo,
                double* var) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = dn_ctx_check(c, "rr_variance");
    if (rc != RR_OK) return rc;
    int32_t terms = 0;
    rc = var_check(d, W, H, C, VarPlanes{in, m2, count, depth, normal, object, albedo, var}, &terms);
    if (rc != RR_OK) return rc;
    const size_t n = (size_t)(W * H), img = n * C * sizeof(double);
    void* host[8] = {var, (void*)in, (void*)m2, (void*)count, (void*)depth, (void*)normal, (void*)object, (void*)albedo};
    const size_t bytes[8] = {n * sizeof(double), img, img, n * sizeof(int32_t), n * sizeof(double), n * 3 * sizeof(double),
                             n * sizeof(int32_t), n * 3 * sizeof(double)};
    void* dev[8];
    rc = dv_stage(c, 8, 1, host, bytes, dev);
    if (rc != RR_OK) return rc;
    rc = rr_variance_device(c, d, W, H, C, dev[1], dev[2], dev[3], dev[4], dev[5], dev[6], dev[7], dev[0], nullptr);
    if (rc != RR_OK) return rc;
    HIPCHK(hipMemcpyAsync(var, dev[0], bytes[0], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return RR_OK;
}

// what every rr_denoise_var entry refuses of its arguments (the context apart): rr_denoise's refusals, then its own
static int dv_check(const rr_denoise_var_desc* d, int64_t W, int64_t H, int32_t C, const DnPlanes& P, const void* var,
                    const void* var_out, rr_denoise_desc* base, int32_t* terms) {
    if (!d) return fail(RR_E_ARG, "rr_denoise_var: null argument");
    *base = rr_denoise_desc{d->iterations, d->flags, d->sigma_color, d->sigma_normal, d->sigma_depth, d->sigma_albedo};
    int rc = dn_check(base, W, H, C, P, terms, "rr_denoise_var");
    if (rc != RR_OK) return rc;
    if (!var) return fail(RR_E_ARG, "rr_denoise_var: null var");
    if (!(std::isfinite(d->epsilon) && d->epsilon > 0.0)) return fail(RR_E_ARG, "rr_denoise_var: epsilon must be finite and > 0");
    const size_t n = (size_t)(W * H), img = n * (size_t)C * sizeof(double), vb = n * sizeof(double);
    if (dn_overlap(P.out, img, var, vb)) return fail(RR_E_ARG, "rr_denoise_var: out overlaps an input");
    if (dn_overlap(var_out, vb, P.in, img) || dn_overlap(var_out, vb, var, vb) || dn_overlap(var_out, vb, P.depth, n * sizeof(double)) ||
        dn_overlap(var_out, vb, P.normal, n * 3 * sizeof(double)) || dn_overlap(var_out, vb, P.object, n * sizeof(int32_t)) ||
        dn_overlap(var_out, vb, P.albedo, n * 3 * sizeof(double)))
        return fail(RR_E_ARG, "rr_denoise_var: var_out overlaps an input");
    if (dn_overlap(var_out, vb, P.out, img)) return fail(RR_E_ARG, "rr_denoise_var: the two outputs overlap");
    return RR_OK;
}

int rr_denoise_var_reference(const rr_denoise_var_desc* d, int64_t W, int64_t H, int32_t C, const double* in,
                             const double* var, const double* depth, const double* normal, const int32_t* object,
                             const double* albedo, double* out, double* var_out) {
    int32_t terms = 0;
    rr_denoise_desc base;
    int rc = dv_check(d, W, H, C, DnPlanes{in, depth, normal, object, albedo, out}, var, var_out, &base, &terms);
    if (rc != RR_OK) return rc;
    const int64_t n = W * H;
    std::vector<rr::DnGuide> g((size_t)n);
    for (int64_t p = 0; p < n; ++p) g[(size_t)p] = rr::dn_guide(p, depth, normal, object, albedo);
    std::vector<double> f[2], v[2], vlast;
    for (int k = 0; k < 2; ++k)
        if (d->iterations > k + 1) f[k].resize((size_t)n * C), v[k].resize((size_t)n);
    if (!var_out) vlast.resize((size_t)n);
    const double *src = in, *vsrc = var;
    for (int32_t i = 0; i < d->iterations; ++i) {
        const bool last = i == d->iterations - 1;
        double* dst = last ? out : f[i & 1].data();
        double* vdst = last ? (var_out ? var_out : vlast.data()) : v[i & 1].data();
        const rr::DnLevel L = rr::dv_level(terms, i, d->sigma_color, d->sigma_normal, d->sigma_depth, d->sigma_albedo);
        for (int64_t y = 0; y < H; ++y)
            for (int64_t x = 0; x < W; ++x) {
                const int64_t p = y * W + x;
                if (C == 3)
                    rr::dv_pixel<3>(L, d->epsilon, W, H, x, y, src, vsrc, g.data(), dst + 3 * p, vdst + p);
                else
                    rr::dv_pixel<1>(L, d->epsilon, W, H, x, y, src, vsrc, g.data(), dst + p, vdst + p);
            }
        src = dst;
        vsrc = vdst;
    }
    return RR_OK;
}

int rr_denoise_var_device(rr_ctx* c, const rr_denoise_var_desc* d, int64_t W, int64_t H, int32_t C, const void* d_in,
                          const void* d_var, const void* d_depth, const void* d_normal, const void* d_object,
                          const void* d_albedo, void* d_out, void* d_var_out, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = dn_ctx_check(c, "rr_denoise_var");
    if (rc != RR_OK) return rc;
    int32_t terms = 0;
    rr_denoise_desc base;
    rc = dv_check(d, W, H, C, DnPlanes{d_in, d_depth, d_normal, d_object, d_albedo, d_out}, d_var, d_var_out, &base, &terms);
    if (rc != RR_OK) return rc;
    const int64_t n = W * H;
    const size_t img = (size_t)n * (size_t)C * sizeof(double), vb = (size_t)n * sizeof(double);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    // the scratch is claimed before it may grow: a call on another stream may still read the buffers that ensure frees
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    const int32_t I = d->iterations;
    if (c->dn_guides.bytes < (size_t)n * sizeof(rr::DnGuide) || (I > 1 && (c->dn_img[0].bytes < img || c->dv_var[0].bytes < vb)) ||
        (I > 2 && (c->dn_img[1].bytes < img || c->dv_var[1].bytes < vb)))
        HIPCHK(hipStreamSynchronize(st));  // growing frees: nothing enqueued may still use the old buffers
    HIPCHK(c->dn_guides.ensure((size_t)n * sizeof(rr::DnGuide)));
    for (int k = 0; k < 2; ++k)
        if (I > k + 1) {
            HIPCHK(c->dn_img[k].ensure(img));
            HIPCHK(c->dv_var[k].ensure(vb));
        }
    rr::DnGuide* g = c->dn_guides.as<rr::DnGuide>();
    HIPCHK(rr::launch_denoise_pack(n, static_cast<const double*>(d_depth), static_cast<const double*>(d_normal),
                                   static_cast<const int32_t*>(d_object), static_cast<const double*>(d_albedo), g, st));
    const double *src = static_cast<const double*>(d_in), *vsrc = static_cast<const double*>(d_var);
    for (int32_t i = 0; i < I; ++i) {
        const bool last = i == I - 1;
        double* dst = last ? static_cast<double*>(d_out) : c->dn_img[i & 1].as<double>();
        double* vdst = last ? static_cast<double*>(d_var_out) : c->dv_var[i & 1].as<double>();  // null: not stored
        const rr::DnLevel L = rr::dv_level(terms, i, d->sigma_color, d->sigma_normal, d->sigma_depth, d->sigma_albedo);
        HIPCHK(rr::launch_denoise_var_level(L, d->epsilon, C, W, H, src, vsrc, g, dst, vdst, st));
        src = dst;
        vsrc = vdst;
    }
    HIPCHK(claim.release());
    return RR_OK;
}

int rr_denoise_var(rr_ctx* c, const rr_denoise_var_desc* d, int64_t W, int64_t H, int32_t C, const double* in,
                   const double* var, const double* depth, const double* normal, const int32_t* object, const double* albedo,
                   double* out, double* var_out) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = dn_ctx_check(c, "rr_denoise_var");
    if (rc != RR_OK) return rc;
    int32_t terms = 0;
    rr_denoise_desc base;
    rc = dv_check(d, W, H, C, DnPlanes{in, depth, normal, object, albedo, out}, var, var_out, &base, &terms);
    if (rc != RR_OK) return rc;
    const size_t n = (size_t)(W * H), img = n * C * sizeof(double);
    void* host[8] = {out, var_out, (void*)in, (void*)var, (void*)depth, (void*)normal, (void*)object, (void*)albedo};
    const size_t bytes[8] = {img, n * sizeof(double), img, n * sizeof(double), n * sizeof(double), n * 3 * sizeof(double),
                             n * sizeof(int32_t), n * 3 * sizeof(double)};
    void* dev[8];
    rc = dv_stage(c, 8, 2, host, bytes, dev);
    if (rc != RR_OK) return rc;
    rc = rr_denoise_var_device(c, d, W, H, C, dev[2], dev[3], dev[4], dev[5], dev[6], dev[7], dev[0], dev[1], nullptr);
    if (rc != RR_OK) return rc;
    HIPCHK(hipMemcpyAsync(out, dev[0], bytes[0], hipMemcpyDeviceToHost, c->stream));
    if (var_out) HIPCHK(hipMemcpyAsync(var_out, dev[1], bytes[1], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return RR_OK;
}

// ---- temporal accumulation (render_temporal.inc, temporal_tap.hpp) ----
// One kernel launch per call, no scratch.  It reads no scene and counts nothing: frame state and pending stats stay as
// they are.
static_assert(sizeof(rr_temporal_desc) == 32, "rr_temporal_desc is 32 bytes (rray.h)");
static_assert(sizeof(rr_temporal_frame) == 48, "rr_temporal_frame is 48 bytes (rray.h)");

static bool tp_cameras_equal(const rr_camera* a, const rr_camera* b) {
    bool eq = a->hsize == b->hsize && a->vsize == b->vsize && a->field_of_view == b->field_of_view &&
              a->pixel_size == b->pixel_size && a->half_width == b->half_width && a->half_height == b->half_height;
    for (int i = 0; i < 16; ++i) eq = eq && a->transform[i] == b->transform[i];
    return eq;
}

static rr::TpFrame tp_frame(const rr_temporal_frame* f) {
    return rr::TpFrame{static_cast<const double*>(f->image),   static_cast<const double*>(f->depth),
                       static_cast<const double*>(f->normal),  static_cast<const int32_t*>(f->object),
                       static_cast<const int32_t*>(f->count),  static_cast<const double*>(f->m2)};
}

// what every temporal entry refuses of its arguments (the context apart); fills the kernel's arguments
static int tp_check(const rr_temporal_desc* d, int64_t W, int64_t H, int32_t C, const rr_camera* cam,
                    const rr_temporal_frame* cur, const rr_camera* prev_cam, const rr_temporal_frame* prev, const void* out,
                    const void* n_out, const void* m2_out, rr::TpConst* K, rr::TpFrame* fc, rr::TpFrame* fp) {
    if (!d || !cam || !prev_cam || !cur || !prev || !out || !n_out) return fail(RR_E_ARG, "rr_temporal: null argument");
    if (C != 1 && C != 3) return fail(RR_E_ARG, "rr_temporal: channels must be 1 or 3");
    if (W < 1 || H < 1) return fail(RR_E_ARG, "rr_temporal: width and height must be >= 1");
    if (cam->hsize != W || cam->vsize != H || prev_cam->hsize != W || prev_cam->vsize != H)
        return fail(RR_E_ARG, "rr_temporal: both cameras must have the frame's size");
    if (!cur->image || !cur->depth || !prev->image || !prev->depth || !prev->count)
        return fail(RR_E_ARG, "rr_temporal: the image and depth planes of both frames and the previous count plane are required");
    if (d->flags & ~RR_TP_OBJECT) return fail(RR_E_ARG, "rr_temporal: unknown flag bits");
    if (d->max_history < 1 || d->max_history > RR_MAX_TEMPORAL_HISTORY)
        return fail(RR_E_ARG, "rr_temporal: max_history must be in 1.." + std::to_string(RR_MAX_TEMPORAL_HISTORY));
    if (!(d->alpha >= 0.0 && d->alpha <= 1.0)) return fail(RR_E_ARG, "rr_temporal: alpha must be in 0..1");
    for (double s : {d->sigma_plane, d->sigma_normal})
        if (!(std::isfinite(s) && s >= 0.0)) return fail(RR_E_ARG, "rr_temporal: every sigma must be finite and >= 0");
    int32_t t = 0;
    if (d->flags & RR_TP_OBJECT) t |= rr::TP_T_OBJECT;
    if (d->sigma_normal > 0.0) t |= rr::TP_T_NORMAL;
    if (d->sigma_plane > 0.0) t |= rr::TP_T_PLANE;
    if (((t & rr::TP_T_OBJECT) && (!cur->object || !prev->object)) || ((t & rr::TP_T_NORMAL) && (!cur->normal || !prev->normal)) ||
        ((t & rr::TP_T_PLANE) && !cur->normal))
        return fail(RR_E_ARG, "rr_temporal: a term that is switched on needs its planes");
    if ((m2_out != nullptr) != (prev->m2 != nullptr))
        return fail(RR_E_ARG, "rr_temporal: m2_out and the previous frame's m2 go together");
    if (W > (((int64_t)1 << 31) - 1) / H) return fail(RR_E_LIMIT, "a temporal frame must hold fewer than 2^31 pixels");
    const size_t n = (size_t)(W * H), img = n * (size_t)C * sizeof(double);
    const void* outs[3] = {out, n_out, m2_out};
    const size_t out_bytes[3] = {img, n * sizeof(int32_t), img};
    const void* ins[10] = {cur->image, cur->depth, cur->normal, cur->object, prev->image,
                           prev->depth, prev->normal, prev->object, prev->count, prev->m2};
    const size_t in_bytes[10] = {img, n * sizeof(double), n * 3 * sizeof(double), n * sizeof(int32_t), img,
                                 n * sizeof(double), n * 3 * sizeof(double), n * sizeof(int32_t), n * sizeof(int32_t), img};
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 10; ++b)
            if (dn_overlap(outs[a], out_bytes[a], ins[b], in_bytes[b])) return fail(RR_E_ARG, "rr_temporal: an output overlaps an input");
        for (int b = a + 1; b < 3; ++b)
            if (dn_overlap(outs[a], out_bytes[a], outs[b], out_bytes[b])) return fail(RR_E_ARG, "rr_temporal: two outputs overlap");
    }
    double inv[16], pinv[16];
    int rc = rr_camera_inverse(cam, inv);
    if (rc != RR_OK) return rc;
    rc = rr_camera_inverse(prev_cam, pinv);
    if (rc != RR_OK) return rc;
    K->cur = rr::tp_camera(inv, cam->half_width, cam->half_height, cam->pixel_size);
    K->prev = rr::tp_camera(pinv, prev_cam->half_width, prev_cam->half_height, prev_cam->pixel_size);
    for (int i = 0; i < 12; ++i) K->T[i] = prev_cam->transform[i];
    K->alpha = d->alpha;
    K->sigma_plane = d->sigma_plane;
    K->sigma_normal = d->sigma_normal;
    K->W = W;
    K->H = H;
    K->terms = t;
    K->max_history = d->max_history;
    K->is_static = tp_cameras_equal(cam, prev_cam) ? 1 : 0;
    K->pad = 0;
    *fc = tp_frame(cur);
    *fp = tp_frame(prev);
    fc->count = nullptr;  // previous frame only
    fc->m2 = nullptr;
    return RR_OK;
}

int rr_temporal_reference(const rr_temporal_desc* d, int64_t W, int64_t H, int32_t C, const rr_camera* cam,
                          const rr_temporal_frame* cur, const rr_camera* prev_cam, const rr_temporal_frame* prev, double* out,
                          int32_t* n_out, double* m2_out) {
    rr::TpConst K{};
    rr::TpFrame fc{}, fp{};
    int rc = tp_check(d, W, H, C, cam, cur, prev_cam, prev, out, n_out, m2_out, &K, &fc, &fp);
    if (rc != RR_OK) return rc;
    double unused[3];
    for (int64_t y = 0; y < H; ++y)
        for (int64_t x = 0; x < W; ++x) {
            const int64_t p = y * W + x;
            if (C == 3 && m2_out)
                rr::tp_pixel<3, true>(K, fc, fp, x, y, out + 3 * p, n_out + p, m2_out + 3 * p);
            else if (C == 3)
                rr::tp_pixel<3, false>(K, fc, fp, x, y, out + 3 * p, n_out + p, unused);
            else if (m2_out)
                rr::tp_pixel<1, true>(K, fc, fp, x, y, out + p, n_out + p, m2_out + p);
            else
                rr::tp_pixel<1, false>(K, fc, fp, x, y, out + p, n_out + p, unused);
        }
    return RR_OK;
}

static int tp_ctx_check(const rr_ctx* c) {
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return fail(RR_E_ARG, "rr_temporal needs a single-device context (no multi-device or virtual context)");
    return RR_OK;
}

int rr_temporal_device(rr_ctx* c, const rr_temporal_desc* d, int64_t W, int64_t H, int32_t C, const rr_camera* cam,
                       const rr_temporal_frame* cur, const rr_camera* prev_cam, const rr_temporal_frame* prev, void* d_out,
                       void* d_n_out, void* d_m2_out, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = tp_ctx_check(c);
    if (rc != RR_OK) return rc;
    rr::TpConst K{};
    rr::TpFrame fc{}, fp{};
    rc = tp_check(d, W, H, C, cam, cur, prev_cam, prev, d_out, d_n_out, d_m2_out, &K, &fc, &fp);
    if (rc != RR_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    HIPCHK(rr::launch_temporal(K, C, fc, fp, c->tp_rows != 0, static_cast<double*>(d_out), static_cast<int32_t*>(d_n_out),
                               static_cast<double*>(d_m2_out), st));
    HIPCHK(claim.release());
    return RR_OK;
}

int rr_temporal(rr_ctx* c, const rr_temporal_desc* d, int64_t W, int64_t H, int32_t C, const rr_camera* cam,
                const rr_temporal_frame* cur, const rr_camera* prev_cam, const rr_temporal_frame* prev, double* out,
                int32_t* n_out, double* m2_out) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = tp_ctx_check(c);
    if (rc != RR_OK) return rc;
    rr::TpConst K{};
    rr::TpFrame fc{}, fp{};
    rc = tp_check(d, W, H, C, cam, cur, prev_cam, prev, out, n_out, m2_out, &K, &fc, &fp);
    if (rc != RR_OK) return rc;
    const size_t n = (size_t)(W * H), img = n * C * sizeof(double);
    // one device block: out, n_out, m2_out first, then the planes that are given, each 256-byte aligned
    const void* host[13] = {out,         n_out,       m2_out,       cur->image,   cur->depth,  cur->normal, cur->object,
                            prev->image, prev->depth, prev->normal, prev->object, prev->count, prev->m2};
    const size_t bytes[13] = {img, n * sizeof(int32_t), img, img, n * sizeof(double), n * 3 * sizeof(double),
                              n * sizeof(int32_t), img, n * sizeof(double), n * 3 * sizeof(double), n * sizeof(int32_t),
                              n * sizeof(int32_t), img};
    size_t off[13], total = 0;
    for (int k = 0; k < 13; ++k) {
        off[k] = total;
        if (host[k]) total += (bytes[k] + 255) & ~(size_t)255;
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_ctx(c));  // tp_host may grow, and a call on another stream may still read it
    HIPCHK(c->tp_host.ensure(total));
    char* base = c->tp_host.as<char>();
    void* dev[13];
    for (int k = 0; k < 13; ++k) {
        dev[k] = host[k] ? base + off[k] : nullptr;
        if (k >= 3 && host[k]) HIPCHK(hipMemcpyAsync(dev[k], host[k], bytes[k], hipMemcpyHostToDevice, c->stream));
    }
    const rr_temporal_frame dc{dev[3], dev[4], dev[5], dev[6], nullptr, nullptr};
    const rr_temporal_frame dp{dev[7], dev[8], dev[9], dev[10], dev[11], dev[12]};
    rc = rr_temporal_device(c, d, W, H, C, cam, &dc, prev_cam, &dp, dev[0], dev[1], dev[2], nullptr);
    if (rc != RR_OK) return rc;
    for (int k = 0; k < 3; ++k)
        if (host[k]) HIPCHK(hipMemcpyAsync(const_cast<void*>(host[k]), dev[k], bytes[k], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return RR_OK;
}

// ---- one-bounce indirect light (render_indirect.inc, ao_dir.hpp) ----
// K gathered rays per point from indirect_rays_kernel, traced by the colour families' rays0 path a pass of whole points
// at a time and averaged per point by indirect_resolve_kernel: the lens frames' structure with the occlusion frames'
// points.  The frames trace only the rays of the samples that hit, through the listed kernels' ordered source with the
// live count left on the device.  The isolation rule of the ray queries holds: counters in buffer 2, no frame state
// touched.
static_assert(sizeof(rr_indirect) == 16, "rr_indirect is 16 bytes (rray.h)");

// what every indirect entry refuses of the parameters; fills the kernel's argument
static int indirect_check(const rr_indirect* ind, rr::DevIndirect* P) {
    if (!ind) return fail(RR_E_ARG, "indirect light: null rr_indirect");
    if (ind->samples < 1 || ind->samples > RR_MAX_INDIRECT_SAMPLES)
        return fail(RR_E_ARG, "indirect samples must be in 1.." + std::to_string(RR_MAX_INDIRECT_SAMPLES));
    if (ind->remaining < 0 || ind->remaining > RR_MAX_DEPTH) return fail(RR_E_LIMIT, "rr_indirect.remaining out of range");
    P->seed = ind->seed;
    P->samples = (uint32_t)ind->samples;
    P->pad = 0;
    return RR_OK;
}

// rr_color_at_device's level 0: sample j's jitter identity is (j, path 1)
static rr::LevelArgs indirect_level0(uint64_t seed, int32_t jitter_mode) {
    rr::LevelArgs A{};
    A.hs = 1;
    A.aa = 1;
    A.part = 0;
    A.nparts = 1;
    A.block_rows = 1;
    A.seed = seed;
    A.jitter_mode = jitter_mode;
    return A;
}
// A pass's scratch seen from the frame's ray indices: the kernels index rays, sample identities and output slots by the
// global j, so the pointers are biased by -r0 entries and never dereferenced outside the pass (integer arithmetic: the
// biased addresses may lie below the allocations), as rr_render_lens_device does.
static double* biased(double* p, int64_t r0, int per_ray) {
    return reinterpret_cast<double*>(reinterpret_cast<uintptr_t>(p) - (uintptr_t)r0 * per_ray * sizeof(double));
}

int rr_indirect_at_device(rr_ctx* c, int64_t n, const void* d_points, const void* d_normals, const rr_indirect* ind,
                          uint64_t seed, int32_t jitter_mode, void* d_out, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    rr::DevIndirect P{};
    int rc = indirect_check(ind, &P);
    if (rc != RR_OK) return rc;
    rc = rays_check(c, n, !d_points || !d_normals || !d_out);
    if (rc != RR_OK) return rc;
    const int64_t K = ind->samples;
    if (n * K >= ((int64_t)1 << 32)) return fail(RR_E_LIMIT, "an indirect batch must hold fewer than 2^32 rays (n * samples)");
    if (n == 0) return RR_OK;
    const rr::IndirectPassPlan plan = rr::plan_indirect_passes(n, ind->samples, c->batch, c->indirect_pass);
    const int64_t pass_rays = std::min(plan.points, n) * K;
    const FrameFacts facts = frame_facts(c, ind->remaining);
    HIPCHK(hipSetDevice(c->device));
    // one pass's rays and colours (grown on demand, as the lens frames')
    HIPCHK(c->ind_rays.ensure((size_t)pass_rays * 6 * sizeof(double)));
    HIPCHK(c->ind_rgb.ensure((size_t)pass_rays * 3 * sizeof(double)));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    c->frame_timed = true;
    HIPCHK(hipEventRecord(c->e0, st));
    const int saved_epoch = c->epoch;
    c->epoch = 2;  // the query buffer (frame buffers keep their state), zeroed once per call
    HIPCHK(hipMemsetAsync(frame_counters(c, 2), 0, kCounterBytes, st));
    rr::LevelArgs A = indirect_level0(seed, jitter_mode);
    double* const rays = c->ind_rays.as<double>();
    double* const rgb = c->ind_rgb.as<double>();
    for (int64_t first = 0; first < n && rc == RR_OK; first += plan.points) {
        const int64_t np = std::min(plan.points, n - first), r0 = first * K;  // r0 is a multiple of 64
        const rr::AoPoints I{static_cast<const double*>(d_points) + 3 * first, static_cast<const double*>(d_normals) + 3 * first,
                             3, 1, nullptr, first};
        hipError_t e = rr::launch_indirect_rays(P, I, np, rays, nullptr, nullptr, nullptr, 0, st);
        if (e != hipSuccess) {
            rc = fail(RR_E_HIP, std::string("launch_indirect_rays: ") + hipGetErrorString(e));
            break;
        }
        A.rays0 = biased(rays, r0, 6);
        rc = run_levels(c, facts, A, np * K, ind->remaining, biased(rgb, r0, 3), st, nullptr, 0, 0, nullptr, r0);
        if (rc != RR_OK) break;
        e = rr::launch_indirect_resolve(rgb, nullptr, ind->samples, np, static_cast<double*>(d_out) + 3 * first, st);
        if (e != hipSuccess) rc = fail(RR_E_HIP, std::string("launch_indirect_resolve: ") + hipGetErrorString(e));
    }
    c->epoch = saved_epoch;
    if (rc != RR_OK) return rc;
    HIPCHK(hipEventRecord(c->e1, st));
    HIPCHK(claim.release());
    rays_stats_pending(c, n);
    return RR_OK;
}

// what both frame entries refuse before they look at the context
static int indirect_frame_check(const rr_camera* cam, const rr_render_opts* o, const rr_indirect* ind, const void* out,
                                rr::DevIndirect* P) {
    if (!cam || !o || !out) return fail(RR_E_ARG, "rr_render_indirect: null argument");
    return indirect_check(ind, P);
}
static int indirect_ctx_check(const rr_ctx* c) {
    if (!c) return fail(RR_E_ARG, "null context");
    if (c->group) return fail(RR_E_ARG, "indirect frames need a single-device context (no multi-device or virtual context)");
    if (!c->has_scene) return fail(RR_E_ARG, "no scene uploaded");
    return RR_OK;
}

int rr_render_indirect_device(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, const rr_indirect* ind, void* d_out,
                              void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    rr::DevIndirect P{};
    int rc = indirect_frame_check(cam, o, ind, d_out, &P);
    if (rc != RR_OK) return rc;
    rc = indirect_ctx_check(c);
    if (rc != RR_OK) return rc;
    rr_render_opts opts = *o;
    opts.max_depth = 0;  // ignored here, as flags: the gathered rays' budget is rr_indirect.remaining
    rc = check_opts(cam, &opts);
    if (rc != RR_OK) return rc;
    if (o->part != 0 || o->nparts != 1 || o->row_begin != 0 || o->row_end != 0)
        return fail(RR_E_ARG, "indirect frames are whole frames: part 0 of 1, no band");
    const int64_t total = cam->hsize * cam->vsize, K = ind->samples;
    if (total >= ((int64_t)1 << 32) || total * K >= ((int64_t)1 << 32))
        return fail(RR_E_LIMIT, "an indirect frame's rays (hsize * vsize * samples) must number fewer than 2^32");
    const rr::IndirectPassPlan plan = rr::plan_indirect_passes(total, ind->samples, c->batch, c->indirect_pass);
    const int64_t pass = std::min(plan.points, total), pass_rays = pass * K;
    const FrameFacts facts = frame_facts(c, ind->remaining);
    HIPCHK(hipSetDevice(c->device));
    // one pass's camera rays, first-hit planes (RR_HIT_DOUBLES double planes, then the two int planes), gathered rays,
    // colours and live list
    const size_t d_bytes = (size_t)pass * rr::RR_HIT_DOUBLES * sizeof(double);
    HIPCHK(c->ind_cam.ensure((size_t)pass * 6 * sizeof(double)));
    HIPCHK(c->hitrec.ensure(d_bytes + (size_t)pass * 2 * sizeof(int32_t)));
    HIPCHK(c->ind_rays.ensure((size_t)pass_rays * 6 * sizeof(double)));
    HIPCHK(c->ind_rgb.ensure((size_t)pass_rays * 3 * sizeof(double)));
    HIPCHK(c->ind_list.ensure((size_t)pass_rays * sizeof(uint32_t)));
    double* const rays = c->ind_rays.as<double>();
    double* const rgb = c->ind_rgb.as<double>();
    uint32_t* const list = c->ind_list.as<uint32_t>();
    // The trace of a pass: the live list in chunks of one run_levels batch each (one chunk unless RRAY_BATCH or the queue
    // budget says otherwise), every chunk launched for its capacity with its live count on the device.  Planned before
    // anything is enqueued: the per-level paths refuse here.
    rr::LevelArgs A = indirect_level0(o->seed, o->jitter_mode);
    A.rays0 = rays;
    A.list = list;
    const rr::FramePlan fp = plan_run(c, facts, A, pass_rays, ind->remaining, FrameOut{rgb, nullptr, 0, 0, nullptr});
    if (fp.err != RR_OK) return fail(fp.err, fp.msg);
    const int64_t chunk = std::min(pass_rays, fp.B), n_chunks = (pass_rays + chunk - 1) / chunk;
    const int64_t n_blocks = (pass_rays + 255) / 256;
    HIPCHK(c->ind_counts.ensure((size_t)(n_blocks + 1 + n_chunks) * sizeof(uint32_t)));
    uint32_t* const block_count = c->ind_counts.as<uint32_t>();
    uint32_t* const counts = block_count + n_blocks;
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIPCHK(claim_stream(c, st));
    StreamClaim claim{c, st};
    c->frame_timed = true;
    HIPCHK(hipEventRecord(c->e0, st));
    const int saved_epoch = c->epoch;
    c->epoch = 2;  // the query buffer (frame buffers keep their state), zeroed once per frame
    HIPCHK(hipMemsetAsync(frame_counters(c, 2), 0, kCounterBytes, st));
    rr::HitOut O{};
    O.node_object = c->node_object.as<int32_t>();
    O.rec_d = c->hitrec.as<double>();
    O.rec_i = reinterpret_cast<int32_t*>(c->hitrec.as<char>() + d_bytes);
    O.stride = pass;
    rr::LevelArgs C{};
    set_camera(C, cam);  // the frames' DevCamera and affine flag
    rr::LevelArgs H{};   // rr_hit_at_device's level 0 on the pass's camera rays
    H.hs = 1;
    H.aa = 1;
    H.part = 0;
    H.nparts = 1;
    H.block_rows = 1;
    H.nseg = H.nseg_out = 1;
    H.counters = frame_counters(c, 2);
    H.base = 0;
    H.rays0 = c->ind_cam.as<double>();
    // over_point and normalv are planes 12..14 and 9..11 of the records (HitOut.rec_d), object the first int plane
    const rr::AoPoints planes{O.rec_d + 12 * pass, O.rec_d + 9 * pass, 1, pass, O.rec_i, 0};
    for (int64_t first = 0; first < total && rc == RR_OK; first += plan.points) {
        const int64_t np = std::min(plan.points, total - first), r0 = first * K;
        hipError_t e = rr::launch_camera_rays_window(C.cam, C.cam_affine != 0, first, np, c->ind_cam.as<double>(), st);
        if (e == hipSuccess) {
            H.n = np;
            set_level0_index(H);
            e = rr::launch_hit(c->S, H, O, st);
        }
        if (e == hipSuccess) {
            rr::AoPoints I = planes;
            I.first = first;
            e = rr::launch_indirect_rays(P, I, np, rays, list, block_count, counts, chunk, st);
        }
        if (e != hipSuccess) {
            rc = fail(RR_E_HIP, std::string("indirect pass: ") + hipGetErrorString(e));
            break;
        }
        A.rays0 = biased(rays, r0, 6);
        for (int64_t b = 0; b * chunk < np * K && rc == RR_OK; ++b) {
            A.list = list + b * chunk;
            A.n_dev = counts + 1 + b;
            rc = run_levels(c, facts, A, std::min(chunk, np * K - b * chunk), ind->remaining, biased(rgb, r0, 3), st);
        }
        if (rc != RR_OK) break;
        e = rr::launch_indirect_resolve(rgb, O.rec_i, ind->samples, np, static_cast<double*>(d_out) + 3 * first, st);
        if (e != hipSuccess) rc = fail(RR_E_HIP, std::string("launch_indirect_resolve: ") + hipGetErrorString(e));
    }
    c->epoch = saved_epoch;
    if (rc != RR_OK) return rc;
    HIPCHK(hipEventRecord(c->e1, st));
    HIPCHK(claim.release());
    rays_stats_pending(c, total);
    return RR_OK;
}

int rr_render_indirect(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, const rr_indirect* ind, double* out,
                       rr_stats* stats) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    rr::DevIndirect P{};
    int rc = indirect_frame_check(cam, o, ind, out, &P);
    if (rc != RR_OK) return rc;
    rc = indirect_ctx_check(c);
    if (rc != RR_OK) return rc;
    if (cam->hsize <= 0 || cam->vsize <= 0 || cam->hsize > (1ll << 31) || cam->vsize > (1ll << 31))
        return fail(RR_E_ARG, "bad camera size");
    if (cam->hsize * cam->vsize >= ((int64_t)1 << 32) || cam->hsize * cam->vsize * ind->samples >= ((int64_t)1 << 32))
        return fail(RR_E_LIMIT, "an indirect frame's rays (hsize * vsize * samples) must number fewer than 2^32");
    const size_t img = (size_t)cam->hsize * (size_t)cam->vsize * 3 * sizeof(double);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->qout.ensure(img));
    rc = rr_render_indirect_device(c, cam, o, ind, c->qout.p, nullptr);
    if (rc != RR_OK) return rc;
    HIPCHK(hipMemcpyAsync(out, c->qout.p, img, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    rr_stats local;
    rc = rr_last_stats(c, stats ? stats : &local);
    if (rc != RR_OK) return rc;
    const uint64_t nan = (stats ? stats : &local)->nan_rays;
    return nan ? nan_fail(nan) : RR_OK;
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
