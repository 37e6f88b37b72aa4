// api_frames.cpp — the frame entries of include/rray/rray.h beside rr_render: first-hit planes (AOV), adaptive
// anti-aliasing, batches of views and their first-hit planes.
#include "api_ctx.hpp"

static int aov_buffers_check(int32_t planes, const void* depth, const void* normal, const void* object, const void* albedo) {
    if (((planes & RR_AOV_DEPTH) && !depth) || ((planes & RR_AOV_NORMAL) && !normal) ||
        ((planes & RR_AOV_OBJECT) && !object) || ((planes & RR_AOV_ALBEDO) && !albedo))
        return fail(RR_E_ARG, "a requested plane has a null buffer");
    return RR_OK;
}
static int views_same_size(const rr_camera* cams, int32_t n_views) {
    for (int32_t k = 1; k < n_views; ++k)
        if (cams[k].hsize != cams[0].hsize || cams[k].vsize != cams[0].vsize)
            return fail(RR_E_ARG, "the cameras of a batch must share hsize and vsize: camera " + std::to_string(k) + " is " +
                                      std::to_string(cams[k].hsize) + "x" + std::to_string(cams[k].vsize) + ", camera 0 " +
                                      std::to_string(cams[0].hsize) + "x" + std::to_string(cams[0].vsize));
    return RR_OK;
}
// The camera table of a batch: the context's host copy (the caller's array is free after this call), then its device
// buffer, on the call's stream; the padding's flags say "not affine" to the last block's waves past the events
static int upload_views(rr_ctx* c, const rr_camera* cams, int32_t n_views, hipStream_t st) {
    c->views_host.assign((size_t)n_views + rr::RR_VIEW_TABLE_PAD, rr::DevView{});
    for (int32_t k = 0; k < n_views; ++k) {
        rr::LevelArgs T{};
        set_camera(T, &cams[k]);
        c->views_host[k].cam = T.cam;
        c->views_host[k].affine = T.cam_affine;
    }
    HIPCHK(hipMemcpyAsync(c->views.p, c->views_host.data(), c->views_host.size() * sizeof(rr::DevView),
                          hipMemcpyHostToDevice, st));
    return RR_OK;
}

extern "C" {

int rr_render_aov_device(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, int32_t planes, void* d_depth,
                         void* d_normal, void* d_object, void* d_albedo, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (c && c->group)
        return rr_render_aov_device(rr::group_local(c->group, 0), cam, o, planes, d_depth, d_normal, d_object, d_albedo,
                                    hip_stream);
    if (int e = ctx_check(c, nullptr, true)) return e;
    if (!cam || !o) return fail(RR_E_ARG, "null camera/options");
    rr_render_opts opts = *o;
    opts.max_depth = 0;  // ignored here (as seed, jitter_mode and flags): no recursion in a first-hit frame
    int rc = check_opts(cam, &opts);
    if (rc != RR_OK) return rc;
    if (int e = whole_frame_check(o, "AOV frames")) return e;
    const int32_t all = RR_AOV_DEPTH | RR_AOV_NORMAL | RR_AOV_OBJECT | RR_AOV_ALBEDO;
    if (planes == 0 || (planes & ~all)) return fail(RR_E_ARG, "planes must be a non-empty combination of RR_AOV_*");
    if (int e = aov_buffers_check(planes, d_depth, d_normal, d_object, d_albedo)) return e;
    const int64_t total = cam->hsize * cam->vsize;
    if (total >= ((int64_t)1 << 31)) return fail(RR_E_LIMIT, "an AOV frame must hold fewer than 2^31 samples");
    HIPCHK(hipSetDevice(c->device));
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    HIPCHK(st.start_timer());
    HIPCHK(clear_query_counters(c, st));
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
    HIPCHK(st.close_counted(total));
    return RR_OK;
}

int rr_render_aov(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, int32_t planes, double* depth,
                  double* normal, int32_t* object, double* albedo, rr_stats* stats) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (c && c->group) return rr_render_aov(rr::group_local(c->group, 0), cam, o, planes, depth, normal, object, albedo, stats);
    if (int e = ctx_check(c, nullptr, true)) return e;
    if (!cam || !o) return fail(RR_E_ARG, "null camera/options");
    if (int e = aov_buffers_check(planes, depth, normal, object, albedo)) return e;
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
    return finish_host_frame(c, stats);
}

// ---- adaptive anti-aliasing (render_adapt.hip) ----
// what both entry points refuse before they look at the context (so a host without a device can test it)
static int adaptive_check_args(const rr_camera* cam, const rr_render_opts* o, double threshold, const void* avg) {
    if (!cam || !o || !avg) return fail(RR_E_ARG, "rr_render_adaptive: null camera / options / output image");
    if (threshold != threshold) return fail(RR_E_ARG, "rr_render_adaptive: the threshold is NaN");
    if (int e = whole_frame_check(o, "adaptive frames")) return e;
    if (o->flags & ~RR_NO_FRAME_TIMING) return fail(RR_E_ARG, "adaptive frames take no flag but RR_NO_FRAME_TIMING");
    return RR_OK;
}

int rr_render_adaptive_device(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, double threshold, void* d_avg,
                              void* d_mask, void* d_n_refined, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = adaptive_check_args(cam, o, threshold, d_avg);
    if (rc != RR_OK) return rc;
    if ((rc = ctx_check(c, "adaptive frames need", false)) != RR_OK) return rc;
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
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    const int64_t n_blocks = (W * H + rr::RR_ADAPT_BLOCK - 1) / rr::RR_ADAPT_BLOCK;
    HIPCHK(c->adapt_flags.ensure((size_t)(W * H)));
    HIPCHK(c->adapt_blocks.ensure((size_t)n_blocks * sizeof(uint32_t)));
    HIPCHK(c->adapt_counts.ensure(2 * sizeof(uint32_t)));
    HIPCHK(c->adapt_list.ensure((size_t)(W * H) * sizeof(uint32_t)));
    if (aa > 1) HIPCHK(c->canvas.ensure((size_t)total * 3 * sizeof(double)));  // the refine pass's compact samples
    HIPCHK(st.start_timer(!(o->flags & RR_NO_FRAME_TIMING)));
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
    HIPCHK(st.close());
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
    if ((rc = ctx_check(c, "adaptive frames need", false)) != RR_OK) return rc;
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
    return finish_host_frame(c, stats);
}

// ---- batches of views (render_views.hip) ----
// what both entry points refuse before they look at the context (so a host without a device can test it)
static int views_check_args(const rr_camera* cams, int32_t n_views, const rr_render_opts* o, const void* canvas,
                            const void* avg) {
    if (!cams) return fail(RR_E_ARG, "rr_render_views: null camera array");
    if (!o) return fail(RR_E_ARG, "rr_render_views: null options");
    if (n_views < 0) return fail(RR_E_ARG, "rr_render_views: n_views is negative");
    if (int e = whole_frame_check(o, "batches of views")) return e;
    if (o->flags & RR_OUT_AVG_F32) return fail(RR_E_ARG, "batches of views write f64 images: RR_OUT_AVG_F32 is not served");
    if (o->flags & RR_PART_INTERLEAVE)
        return fail(RR_E_ARG, "batches of views run on one device: RR_PART_INTERLEAVE is not served");
    if ((o->flags & RR_OUT_CANVAS) && !canvas) return fail(RR_E_ARG, "rr_render_views: RR_OUT_CANVAS with a null canvas buffer");
    if ((o->flags & RR_OUT_AVG) && !avg) return fail(RR_E_ARG, "rr_render_views: RR_OUT_AVG with a null image buffer");
    return views_same_size(cams, n_views);
}

int rr_render_views_device(rr_ctx* c, const rr_camera* cams, int32_t n_views, const rr_render_opts* o, void* d_canvas,
                           void* d_avg, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = views_check_args(cams, n_views, o, d_canvas, d_avg);
    if (rc != RR_OK) return rc;
    if ((rc = ctx_check(c, "batches of views need", false)) != RR_OK) return rc;
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
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    if (!canvas && avg && !mode.direct_avg) {
        HIPCHK(c->canvas.ensure((size_t)n_views * hs * vs * 3 * sizeof(double)));
        canvas = c->canvas.as<double>();
    }
    if ((rc = upload_views(c, cams, n_views, st)) != RR_OK) return rc;
    HIPCHK(st.start_timer(!(o->flags & RR_NO_FRAME_TIMING)));
    // the colour frames' per-camera state stays as it is: no cached bundles, no cost order, no resident launch
    begin_frame_counters(c);
    rc = run_levels(c, facts, A, total, o->max_depth, canvas, st, mode.direct_avg ? avg : nullptr, 0,
                    mode.wave_avg ? aa : 0, nullptr);
    c->zero_next = false;
    if (rc != RR_OK) return rc;
    if (avg && !mode.direct_avg) HIPCHK(rr::launch_aa(canvas, avg, W, (int64_t)n_views * H, aa, st, kprof(c)));
    end_frame_counters(c);
    HIPCHK(st.close());
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
    if ((rc = ctx_check(c, "batches of views need", false)) != RR_OK) return rc;
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
    return finish_host_frame(c, stats);
}

// ---- first-hit planes of batches of views (render_views.hip launch_hit_views) ----
// what both entry points refuse before they look at the context (so a host without a device can test it)
static int views_aov_check_args(const rr_camera* cams, int32_t n_views, const rr_render_opts* o, int32_t planes,
                                const void* depth, const void* normal, const void* object, const void* albedo) {
    if (!cams) return fail(RR_E_ARG, "rr_render_views_aov: null camera array");
    if (!o) return fail(RR_E_ARG, "rr_render_views_aov: null options");
    if (n_views < 0) return fail(RR_E_ARG, "rr_render_views_aov: n_views is negative");
    if (int e = whole_frame_check(o, "batches of AOV frames")) return e;
    const int32_t all = RR_AOV_DEPTH | RR_AOV_NORMAL | RR_AOV_OBJECT | RR_AOV_ALBEDO;
    if (planes == 0 || (planes & ~all)) return fail(RR_E_ARG, "planes must be a non-empty combination of RR_AOV_*");
    if (int e = aov_buffers_check(planes, depth, normal, object, albedo)) return e;
    return views_same_size(cams, n_views);
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
    if ((rc = ctx_check(c, "batches of views need", false)) != RR_OK) return rc;
    if (n_views == 0) return RR_OK;
    rr::ViewAovPlan plan{};
    rc = views_aov_validate(c, cams, n_views, o, &plan);
    if (rc != RR_OK) return rc;
    const int64_t hs = cams[0].hsize, vs = cams[0].vsize, vsamples = hs * vs;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->views.ensure(((size_t)n_views + rr::RR_VIEW_TABLE_PAD) * sizeof(rr::DevView)));
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    if ((rc = upload_views(c, cams, n_views, st)) != RR_OK) return rc;
    HIPCHK(st.start_timer());
    HIPCHK(clear_query_counters(c, st));
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
    HIPCHK(st.close_counted(n_views * vsamples));
    return RR_OK;
}

int rr_render_views_aov(rr_ctx* c, const rr_camera* cams, int32_t n_views, const rr_render_opts* o, int32_t planes,
                        double* depth, double* normal, int32_t* object, double* albedo, rr_stats* stats) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = views_aov_check_args(cams, n_views, o, planes, depth, normal, object, albedo);
    if (rc != RR_OK) return rc;
    if ((rc = ctx_check(c, "batches of views need", false)) != RR_OK) return rc;
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
    return finish_host_frame(c, stats);
}

}  // extern "C"
