// api_sampled.cpp — the entries of include/rray/rray.h that trace several samples per pixel or point in passes: lens
// frames, ambient occlusion and one-bounce indirect light, with their point queries.
#include "api_ctx.hpp"

// HIPCHK for the launches inside a pass loop: the message names the step instead of quoting the expression
#define HIPCHK_AS(what, expr)                                                                    \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return fail(RR_E_HIP, std::string(what ": ") + hipGetErrorString(e_)); \
    } while (0)

// A pass's scratch seen from the frame's ray indices: the kernels index rays, sample identities and output slots by the
// global j (base + lane), so the pointers are biased by -r0 entries and never dereferenced outside the pass (integer
// arithmetic: the biased addresses may lie below the allocations).
static double* biased(double* p, int64_t r0, int per_ray) {
    return reinterpret_cast<double*>(reinterpret_cast<uintptr_t>(p) - (uintptr_t)r0 * per_ray * sizeof(double));
}

extern "C" {

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
    if (int e = ctx_check(c, "lens frames need", false)) return e;
    rr::DevLens L{};
    int rc = lens_check(cam, lens, &L);
    if (rc != RR_OK) return rc;
    if (first_pixel < 0 || n_pixels < 0 || first_pixel > cam->hsize * cam->vsize ||
        n_pixels > cam->hsize * cam->vsize - first_pixel)
        return fail(RR_E_ARG, "the pixel window [first_pixel, first_pixel + n_pixels) must lie inside the frame");
    if (n_pixels == 0) return RR_OK;
    HIPCHK(hipSetDevice(c->device));
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    HIPCHK(rr::launch_lens_rays(L, first_pixel * L.samples, n_pixels * L.samples, static_cast<double*>(d_rays), st));
    HIPCHK(st.close());
    return RR_OK;
}

// what both frame entries refuse before they look at the context
static int lens_frame_check(const rr_camera* cam, const rr_render_opts* o, const rr_lens* lens, const void* avg,
                            rr::DevLens* L) {
    if (!cam || !o || !lens || !avg) return fail(RR_E_ARG, "rr_render_lens: null argument");
    if (o->aa != 1) return fail(RR_E_ARG, "lens frames take opts->aa == 1: the lens samples take aa's place");
    if (int e = whole_frame_check(o, "lens frames")) return e;
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
    if ((rc = ctx_check(c, "lens frames need", true)) != RR_OK) return rc;
    const int64_t S = lens->samples, n_pixels = cam->hsize * cam->vsize;
    const rr::LensPassPlan plan = rr::plan_lens_passes(n_pixels, lens->samples, c->lens_pass);
    const int64_t pass_rays = std::min(plan.pixels, n_pixels) * S;
    const FrameFacts facts = frame_facts(c, o->max_depth);
    HIPCHK(hipSetDevice(c->device));
    // one pass's rays and colours (grown on demand, as rr_hit_at_device's planes)
    HIPCHK(c->lens_rays.ensure((size_t)pass_rays * 6 * sizeof(double)));
    HIPCHK(c->lens_rgb.ensure((size_t)pass_rays * 3 * sizeof(double)));
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    HIPCHK(st.start_timer(!(o->flags & RR_NO_FRAME_TIMING)));
    QueryEpoch query{c};  // the query buffer, zeroed once per frame
    HIPCHK(clear_query_counters(c, st));
    rr::LevelArgs A = query_level0(o->seed, o->jitter_mode);  // rr_color_at_device's level 0: sample i's jitter identity is (i, path 1)
    double* const rays = c->lens_rays.as<double>();
    double* const rgb = c->lens_rgb.as<double>();
    for (int64_t first = 0; first < n_pixels; first += plan.pixels) {
        const int64_t np = std::min(plan.pixels, n_pixels - first), r0 = first * S;
        HIPCHK_AS("launch_lens_rays", rr::launch_lens_rays(L, r0, np * S, rays, st));
        A.rays0 = biased(rays, r0, 6);  // the pass's events are the frame's r0 .. r0 + np * S
        rc = run_levels(c, facts, A, np * S, o->max_depth, biased(rgb, r0, 3), st, nullptr, 0, 0, nullptr, r0);
        if (rc != RR_OK) return rc;
        HIPCHK_AS("launch_lens_resolve", rr::launch_lens_resolve(rgb, lens->samples, np, static_cast<double*>(d_avg) + 3 * first, st));
    }
    HIPCHK(st.close_counted(n_pixels * S));
    return RR_OK;
}

int rr_render_lens(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, const rr_lens* lens, double* out_avg,
                   rr_stats* stats) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    rr::DevLens L{};
    int rc = lens_frame_check(cam, o, lens, out_avg, &L);
    if (rc != RR_OK) return rc;
    if ((rc = ctx_check(c, "lens frames need", true)) != RR_OK) return rc;
    const size_t img = (size_t)(cam->hsize * cam->vsize) * 3 * sizeof(double);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->qout.ensure(img));
    rc = rr_render_lens_device(c, cam, o, lens, c->qout.p, nullptr);
    if (rc != RR_OK) return rc;
    HIPCHK(hipMemcpyAsync(out_avg, c->qout.p, img, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return finish_host_frame(c, stats);
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
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    const rr::AoPoints I{static_cast<const double*>(d_points), static_cast<const double*>(d_normals), 3, 1, nullptr, 0};
    HIPCHK(rr::launch_ao_pairs(c->S, P, I, n, c->ao_count.as<int32_t>(), c->shadow_sink.as<unsigned long long>(), st));
    HIPCHK(rr::launch_ao_resolve(c->ao_count.as<int32_t>(), ao->samples, n, static_cast<double*>(d_ao), st));
    HIPCHK(st.close());
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
    if ((rc = ctx_check(c, "ambient-occlusion frames need", true)) != RR_OK) return rc;
    rr_render_opts opts = *o;
    opts.max_depth = 0;  // ignored here (as seed, jitter_mode and flags): no recursion in an occlusion frame
    rc = check_opts(cam, &opts);
    if (rc != RR_OK) return rc;
    if (int e = whole_frame_check(o, "ambient-occlusion frames")) return e;
    const int64_t total = cam->hsize * cam->vsize;
    if (total >= ((int64_t)1 << 31)) return fail(RR_E_LIMIT, "an ambient-occlusion frame must hold fewer than 2^31 samples");
    const rr::AoPassPlan plan = rr::plan_ao_passes(total, ao->samples, c->batch, c->ao_pass);
    const int64_t pass = std::min(plan.points, total);
    HIPCHK(hipSetDevice(c->device));
    // one pass's camera rays, first-hit planes (RR_HIT_DOUBLES double planes, then the two int planes) and counts
    rr::HitOut O;
    HIPCHK(c->ao_rays.ensure((size_t)pass * 6 * sizeof(double)));
    HIPCHK(hit_planes(c, pass, &O));
    HIPCHK(c->ao_count.ensure((size_t)pass * sizeof(int32_t)));
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    HIPCHK(st.start_timer());
    HIPCHK(clear_query_counters(c, st));
    rr::LevelArgs C{};
    set_camera(C, cam);  // the frames' DevCamera and affine flag
    rr::LevelArgs A = hit_level0(c);  // rr_hit_at_device's level 0 on the pass's rays
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
    HIPCHK(st.close_counted(total));
    return RR_OK;
}

int rr_render_ao(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, const rr_ao* ao, double* out_ao,
                 rr_stats* stats) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    rr::DevAo P{};
    int rc = ao_frame_check(cam, o, ao, out_ao, &P);
    if (rc != RR_OK) return rc;
    if ((rc = ctx_check(c, "ambient-occlusion frames need", true)) != RR_OK) return rc;
    if (cam->hsize <= 0 || cam->vsize <= 0 || cam->hsize > (1ll << 31) || cam->vsize > (1ll << 31))
        return fail(RR_E_ARG, "bad camera size");
    const size_t img = (size_t)cam->hsize * (size_t)cam->vsize * sizeof(double);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->qout.ensure(img));
    rc = rr_render_ao_device(c, cam, o, ao, c->qout.p, nullptr);
    if (rc != RR_OK) return rc;
    HIPCHK(hipMemcpyAsync(out_ao, c->qout.p, img, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return finish_host_frame(c, stats);
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
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    HIPCHK(st.start_timer());
    QueryEpoch query{c};  // the query buffer, zeroed once per call
    HIPCHK(clear_query_counters(c, st));
    rr::LevelArgs A = query_level0(seed, jitter_mode);
    double* const rays = c->ind_rays.as<double>();
    double* const rgb = c->ind_rgb.as<double>();
    for (int64_t first = 0; first < n; first += plan.points) {
        const int64_t np = std::min(plan.points, n - first), r0 = first * K;  // r0 is a multiple of 64
        const rr::AoPoints I{static_cast<const double*>(d_points) + 3 * first, static_cast<const double*>(d_normals) + 3 * first,
                             3, 1, nullptr, first};
        HIPCHK_AS("launch_indirect_rays", rr::launch_indirect_rays(P, I, np, rays, nullptr, nullptr, nullptr, 0, st));
        A.rays0 = biased(rays, r0, 6);
        rc = run_levels(c, facts, A, np * K, ind->remaining, biased(rgb, r0, 3), st, nullptr, 0, 0, nullptr, r0);
        if (rc != RR_OK) return rc;
        HIPCHK_AS("launch_indirect_resolve",
                  rr::launch_indirect_resolve(rgb, nullptr, ind->samples, np, static_cast<double*>(d_out) + 3 * first, st));
    }
    HIPCHK(st.close_counted(n));
    return RR_OK;
}

// what both frame entries refuse before they look at the context
static int indirect_frame_check(const rr_camera* cam, const rr_render_opts* o, const rr_indirect* ind, const void* out,
                                rr::DevIndirect* P) {
    if (!cam || !o || !out) return fail(RR_E_ARG, "rr_render_indirect: null argument");
    return indirect_check(ind, P);
}

int rr_render_indirect_device(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, const rr_indirect* ind, void* d_out,
                              void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    rr::DevIndirect P{};
    int rc = indirect_frame_check(cam, o, ind, d_out, &P);
    if (rc != RR_OK) return rc;
    rc = ctx_check(c, "indirect frames need", true);
    if (rc != RR_OK) return rc;
    rr_render_opts opts = *o;
    opts.max_depth = 0;  // ignored here, as flags: the gathered rays' budget is rr_indirect.remaining
    rc = check_opts(cam, &opts);
    if (rc != RR_OK) return rc;
    if (int e = whole_frame_check(o, "indirect frames")) return e;
    const int64_t total = cam->hsize * cam->vsize, K = ind->samples;
    if (total >= ((int64_t)1 << 32) || total * K >= ((int64_t)1 << 32))
        return fail(RR_E_LIMIT, "an indirect frame's rays (hsize * vsize * samples) must number fewer than 2^32");
    const rr::IndirectPassPlan plan = rr::plan_indirect_passes(total, ind->samples, c->batch, c->indirect_pass);
    const int64_t pass = std::min(plan.points, total), pass_rays = pass * K;
    const FrameFacts facts = frame_facts(c, ind->remaining);
    HIPCHK(hipSetDevice(c->device));
    // one pass's camera rays, first-hit planes (RR_HIT_DOUBLES double planes, then the two int planes), gathered rays,
    // colours and live list
    rr::HitOut O;
    HIPCHK(c->ind_cam.ensure((size_t)pass * 6 * sizeof(double)));
    HIPCHK(hit_planes(c, pass, &O));
    HIPCHK(c->ind_rays.ensure((size_t)pass_rays * 6 * sizeof(double)));
    HIPCHK(c->ind_rgb.ensure((size_t)pass_rays * 3 * sizeof(double)));
    HIPCHK(c->ind_list.ensure((size_t)pass_rays * sizeof(uint32_t)));
    double* const rays = c->ind_rays.as<double>();
    double* const rgb = c->ind_rgb.as<double>();
    uint32_t* const list = c->ind_list.as<uint32_t>();
    // The trace of a pass: the live list in chunks of one run_levels batch each (one chunk unless RRAY_BATCH or the queue
    // budget says otherwise), every chunk launched for its capacity with its live count on the device.  Planned before
    // anything is enqueued: the per-level paths refuse here.
    rr::LevelArgs A = query_level0(o->seed, o->jitter_mode);
    A.rays0 = rays;
    A.list = list;
    const rr::FramePlan fp = plan_run(c, facts, A, pass_rays, ind->remaining, FrameOut{rgb, nullptr, 0, 0, nullptr});
    if (fp.err != RR_OK) return fail(fp.err, fp.msg);
    const int64_t chunk = std::min(pass_rays, fp.B), n_chunks = (pass_rays + chunk - 1) / chunk;
    const int64_t n_blocks = (pass_rays + 255) / 256;
    HIPCHK(c->ind_counts.ensure((size_t)(n_blocks + 1 + n_chunks) * sizeof(uint32_t)));
    uint32_t* const block_count = c->ind_counts.as<uint32_t>();
    uint32_t* const counts = block_count + n_blocks;
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    HIPCHK(st.start_timer());
    QueryEpoch query{c};  // the query buffer, zeroed once per frame
    HIPCHK(clear_query_counters(c, st));
    rr::LevelArgs C{};
    set_camera(C, cam);  // the frames' DevCamera and affine flag
    rr::LevelArgs H = hit_level0(c);  // rr_hit_at_device's level 0 on the pass's camera rays
    H.rays0 = c->ind_cam.as<double>();
    // over_point and normalv are planes 12..14 and 9..11 of the records (HitOut.rec_d), object the first int plane
    const rr::AoPoints planes{O.rec_d + 12 * pass, O.rec_d + 9 * pass, 1, pass, O.rec_i, 0};
    for (int64_t first = 0; first < total; first += plan.points) {
        const int64_t np = std::min(plan.points, total - first), r0 = first * K;
        HIPCHK_AS("indirect pass", rr::launch_camera_rays_window(C.cam, C.cam_affine != 0, first, np, c->ind_cam.as<double>(), st));
        H.n = np;
        set_level0_index(H);
        HIPCHK_AS("indirect pass", rr::launch_hit(c->S, H, O, st));
        rr::AoPoints I = planes;
        I.first = first;
        HIPCHK_AS("indirect pass", rr::launch_indirect_rays(P, I, np, rays, list, block_count, counts, chunk, st));
        A.rays0 = biased(rays, r0, 6);
        for (int64_t b = 0; b * chunk < np * K; ++b) {
            A.list = list + b * chunk;
            A.n_dev = counts + 1 + b;
            rc = run_levels(c, facts, A, std::min(chunk, np * K - b * chunk), ind->remaining, biased(rgb, r0, 3), st);
            if (rc != RR_OK) return rc;
        }
        HIPCHK_AS("launch_indirect_resolve",
                  rr::launch_indirect_resolve(rgb, O.rec_i, ind->samples, np, static_cast<double*>(d_out) + 3 * first, st));
    }
    HIPCHK(st.close_counted(total));
    return RR_OK;
}

int rr_render_indirect(rr_ctx* c, const rr_camera* cam, const rr_render_opts* o, const rr_indirect* ind, double* out,
                       rr_stats* stats) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    rr::DevIndirect P{};
    int rc = indirect_frame_check(cam, o, ind, out, &P);
    if (rc != RR_OK) return rc;
    rc = ctx_check(c, "indirect frames need", true);
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
    return finish_host_frame(c, stats);
}

}  // extern "C"
