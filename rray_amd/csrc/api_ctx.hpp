// api_ctx.hpp — what the units of the C ABI share (api.cpp: context, scene, frame core; api_queries.cpp, api_frames.cpp,
// api_sampled.cpp, api_filters.cpp: the entry points by feature): the context, the error state, the frame core's
// functions the entries call, and what every entry does first and last.  Internal: nothing here is exported.
#pragma once
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
#include "rr_error.hpp"
#include "rr_math.hpp"

#pragma GCC visibility push(hidden)
namespace rr::api {

int fail(int code, const std::string& msg);  // sets the thread's error text (rr_last_error); returns code
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

}  // namespace rr::api
#pragma GCC visibility pop
using namespace rr::api;  // the api units' own vocabulary (this header is theirs alone)

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

#pragma GCC visibility push(hidden)
namespace rr::api {

template <class T>
hipError_t upload(DBuf& b, const std::vector<T>& v, hipStream_t st) {
    hipError_t e = b.ensure(std::max<size_t>(v.size() * sizeof(T), 16));
    if (e != hipSuccess) return e;
    if (!v.empty()) e = hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st);
    return e;
}

// The context's workspace is used on one stream at a time: a call on another stream than the
// previous one first waits for it (one event, only when the stream changes).
inline hipError_t claim_stream(rr_ctx* c, hipStream_t st) {
    if (c->have_out && c->last_st != st) {
        hipError_t e = hipStreamWaitEvent(st, c->ev_out, 0);
        if (e != hipSuccess) return e;
    }
    c->last_st = st;
    return hipSuccess;
}
// marks the end of the work a call enqueued on `st` (claim_stream and sync_ctx wait for it)
inline hipError_t release_stream(rr_ctx* c, hipStream_t st) {
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
inline hipError_t sync_ctx(rr_ctx* c) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && c->have_out) e = hipEventSynchronize(c->ev_out);
    return e;
}

constexpr size_t kCounterBytes = (size_t)rr::RR_CNT_SLOTS * rr::RR_CNT_STRIDE * sizeof(unsigned long long);
inline unsigned long long* frame_counters(rr_ctx* c, int k) {
    return c->counters.as<unsigned long long>() + (size_t)k * rr::RR_CNT_SLOTS * rr::RR_CNT_STRIDE;
}

// What a call's plans (frame_plan.hpp) read of the scene and the environment, gathered once per ABI call and never
// kept: the tests flip the switches between renders on one context.  The family predicates are the device units'
// own answers (each switch of theirs keeps its one reader) for the depth the call renders at.
struct FrameFacts {
    rr::FrameTraits traits;
    rr::FrameSwitches sw;
};

inline rr::KernelProf* kprof(rr_ctx* c) { return c->profile ? &c->prof : nullptr; }

// The box average of a canvas-path frame (aa outside the in-wave cases, e.g. C3's aa = 3) overlapped with the
// render: the frame runs in passes of whole output rows, and each pass's rows are averaged on the context's
// second stream while the next pass renders (the render is VALU-bound, the average HBM-bound).  Null: no passes.
struct AaPasses {
    void* avg;
    int32_t f32;
    int64_t width;  // output pixels per row
    int32_t aa;
};

// where a run's results go (run_levels' arguments)
struct FrameOut {
    double* out;
    void* avg;
    int32_t avg_f32, aa_wave;
    const AaPasses* aap;
};

// ---- the frame core (api.cpp), as far as the entry points of the other units call it ----
int check_opts(const rr_camera* cam, const rr_render_opts* o);
rr::DevCamera dev_camera(const rr_camera* c);
void set_camera(rr::LevelArgs& A, const rr_camera* cam);
rr::LevelArgs camera_args(const rr_camera* cam, const rr_render_opts* o, int32_t aa, int32_t part, int32_t block);
void begin_frame_counters(rr_ctx* c);
void end_frame_counters(rr_ctx* c);
void set_level0_index(rr::LevelArgs& A);
int tile_bundles(rr_ctx* c, const rr::LevelArgs& base_args, hipStream_t st, const float** out);
FrameFacts frame_facts(const rr_ctx* c, int max_depth);
rr::FramePlan plan_run(const rr_ctx* c, const FrameFacts& facts, const rr::LevelArgs& A, int64_t total, int max_depth,
                       const FrameOut& o);
int run_levels(rr_ctx* c, const FrameFacts& facts, const rr::LevelArgs& base_args, int64_t total, int max_depth,
               double* out, hipStream_t st, void* avg = nullptr, int32_t avg_f32 = 0, int32_t aa_wave = 0,
               const AaPasses* aap = nullptr, int64_t base0 = 0);
void collect_stats(rr_ctx* c, rr_stats* s);
int nan_fail(uint64_t n);

// ---- what every entry point does first and last: a new entry reuses these instead of copying a neighbour ----
// The refusals of the context, in this order: a null one, a group where the entry serves none (`need` is the whole
// prefix, "lens frames need" or "rr_denoise needs"; null where a group was forwarded before), no scene where one is read.
inline int ctx_check(const rr_ctx* c, const char* need, bool scene) {
    if (!c) return fail(RR_E_ARG, "null context");
    if (need && c->group) return fail(RR_E_ARG, std::string(need) + " a single-device context (no multi-device or virtual context)");
    if (scene && !c->has_scene) return fail(RR_E_ARG, "no scene uploaded");
    return RR_OK;
}
// the entries that take no part and no band; `what`: "lens frames", "batches of views", ...
inline int whole_frame_check(const rr_render_opts* o, const char* what) {
    if (o->part != 0 || o->nparts != 1 || o->row_begin != 0 || o->row_end != 0)
        return fail(RR_E_ARG, std::string(what) + " are whole frames: part 0 of 1, no band");
    return RR_OK;
}
// what the ray queries refuse alike (n == 0 is the caller's early RR_OK, after these)
inline int rays_check(const rr_ctx* c, int64_t n, bool null_buffer, bool scene = true) {
    int rc = ctx_check(c, "device-resident ray queries need", false);
    if (rc != RR_OK) return rc;
    if (n < 0) return fail(RR_E_ARG, "n is negative");
    if (n > 0 && null_buffer) return fail(RR_E_ARG, "null device buffer");
    if (scene && !c->has_scene) return fail(RR_E_ARG, "no scene uploaded");
    if (n >= ((int64_t)1 << 32)) return fail(RR_E_LIMIT, "a ray batch must hold fewer than 2^32 rays");
    return RR_OK;
}

// the call's counters are the context's pending stats (rr_render_views_aov_device's pattern)
inline void rays_stats_pending(rr_ctx* c, int64_t n) {
    c->stats_src = frame_counters(c, 2);
    c->stats_pending = true;
    c->last.samples = (uint64_t)n;
    c->adapt_pending = false;
}
// An entry's work on its stream (the caller's, or the context's own): open() claims the stream, start_timer() brackets
// the frame with e0 / e1 where the entry is timed, close() records e1 and releases the claim — which the StreamClaim
// does by itself on every other exit after open().
struct EntryScope {
    rr_ctx* c;
    hipStream_t st;
    StreamClaim claim;
    bool timer = false;
    EntryScope(rr_ctx* ctx, void* hip_stream)
        : c(ctx), st(hip_stream ? (hipStream_t)hip_stream : ctx->stream), claim{ctx, st, true} {}
    operator hipStream_t() const { return st; }  // an entry names its scope `st` and passes it where a stream goes
    hipError_t open() {
        hipError_t e = claim_stream(c, st);
        if (e == hipSuccess) claim.released = false;
        return e;
    }
    hipError_t start_timer(bool timed = true) {
        timer = true;
        c->frame_timed = timed;
        return timed ? hipEventRecord(c->e0, st) : hipSuccess;
    }
    hipError_t close() {
        if (timer && c->frame_timed) {
            hipError_t e = hipEventRecord(c->e1, st);
            if (e != hipSuccess) return e;
        }
        return claim.release();
    }
    // ... of an entry that counted into the query buffer: its n samples become the pending stats
    hipError_t close_counted(int64_t n) {
        hipError_t e = close();
        if (e == hipSuccess) rays_stats_pending(c, n);
        return e;
    }
};

// The query counter buffer (buffer 2; the frame buffers keep their state).  Every entry that counts into it clears it
// first; the entries that run_levels (whose kernels count into buffer `epoch`) also hold a QueryEpoch, which makes it
// the current buffer until the entry returns — on every path, so that a failed query never leaves the next frame
// counting into the query buffer.
inline hipError_t clear_query_counters(rr_ctx* c, hipStream_t st) {
    return hipMemsetAsync(frame_counters(c, 2), 0, kCounterBytes, st);
}
struct QueryEpoch {
    rr_ctx* c;
    int saved;
    explicit QueryEpoch(rr_ctx* ctx) : c(ctx), saved(ctx->epoch) { c->epoch = 2; }
    ~QueryEpoch() { c->epoch = saved; }
    QueryEpoch(const QueryEpoch&) = delete;
};

// level 0 of a query on explicit rays (rr_color_at): one row of single samples; sample i's jitter identity is (i, path 1)
inline rr::LevelArgs query_level0(uint64_t seed, int32_t jitter_mode) {
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
// ... and of a first-hit query (rr_hit_at): no queues, counted into the query buffer
inline rr::LevelArgs hit_level0(rr_ctx* c) {
    rr::LevelArgs A = query_level0(0, 0);
    A.nseg = A.nseg_out = 1;
    A.counters = frame_counters(c, 2);
    A.base = 0;
    return A;
}
// The first-hit records of `stride` rays as planes in c->hitrec (grown here): RR_HIT_DOUBLES double planes of d_bytes in
// all, then the two int planes
inline hipError_t hit_planes(rr_ctx* c, int64_t stride, rr::HitOut* O, size_t* d_bytes = nullptr) {
    const size_t db = (size_t)stride * rr::RR_HIT_DOUBLES * sizeof(double);
    hipError_t e = c->hitrec.ensure(db + (size_t)stride * 2 * sizeof(int32_t));
    *O = rr::HitOut{};
    O->node_object = c->node_object.as<int32_t>();
    O->rec_d = c->hitrec.as<double>();
    O->rec_i = reinterpret_cast<int32_t*>(c->hitrec.as<char>() + db);
    O->stride = stride;
    if (d_bytes) *d_bytes = db;
    return e;
}

// how a blocking frame entry ends, its device call done and its outputs copied: the frame's stats (to the caller's
// rr_stats, if any) and the NaN refusal
inline int finish_host_frame(rr_ctx* c, rr_stats* stats) {
    rr_stats local;
    int rc = rr_last_stats(c, stats ? stats : &local);
    if (rc != RR_OK) return rc;
    const uint64_t nan = (stats ? stats : &local)->nan_rays;
    return nan ? nan_fail(nan) : RR_OK;
}
// The blocking filter entries' device block in `buf`: the outputs first, then the inputs that are given, each 256-byte
// aligned.  Copies the inputs on the context's stream; dev[k] is null where host[k] is.
inline int stage_planes(rr_ctx* c, DBuf& buf, int n_planes, int n_out, const void* const* host, const size_t* bytes,
                        void** dev) {
    size_t off[16], total = 0;
    for (int k = 0; k < n_planes; ++k) {
        off[k] = total;
        if (host[k]) total += (bytes[k] + 255) & ~(size_t)255;
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_ctx(c));  // buf may grow, and a call on another stream may still read it
    HIPCHK(buf.ensure(total));
    char* base = buf.as<char>();
    for (int k = 0; k < n_planes; ++k) {
        dev[k] = host[k] ? base + off[k] : nullptr;
        if (k >= n_out && host[k]) HIPCHK(hipMemcpyAsync(dev[k], host[k], bytes[k], hipMemcpyHostToDevice, c->stream));
    }
    return RR_OK;
}

}  // namespace rr::api
#pragma GCC visibility pop
