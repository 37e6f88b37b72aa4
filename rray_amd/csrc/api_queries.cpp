// api_queries.cpp — the batch queries of include/rray/rray.h: colours, shadows and first hits of rays given on the host
// (rr_color_at, rr_is_shadowed, rr_hit_at) or resident on the device, in their own order or in a coherent one.
#include "api_ctx.hpp"

// a batch's rays as LevelArgs.rays0 reads them: origin, then direction, per ray
static std::vector<double> pack_rays(const double* origins, const double* directions, int64_t n) {
    std::vector<double> rays((size_t)n * 6);
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            rays[6 * i + k] = origins[3 * i + k];
            rays[6 * i + 3 + k] = directions[3 * i + k];
        }
    return rays;
}

extern "C" {

int rr_color_at(rr_ctx* c, int64_t n, const double* origins, const double* directions, int32_t remaining,
                uint64_t seed, int32_t jitter_mode, double* out_rgb) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (c && c->group) return rr_color_at(rr::group_local(c->group, 0), n, origins, directions, remaining, seed, jitter_mode, out_rgb);
    if (!c || (n > 0 && (!origins || !directions || !out_rgb))) return fail(RR_E_ARG, "null argument");
    if (!c->has_scene) return fail(RR_E_ARG, "no scene uploaded");
    if (remaining < 0 || remaining > RR_MAX_DEPTH) return fail(RR_E_LIMIT, "remaining out of range");
    if (n == 0) return RR_OK;
    HIPCHK(hipSetDevice(c->device));
    EntryScope st{c, nullptr};
    HIPCHK(st.open());
    HIPCHK(upload(c->rays0, pack_rays(origins, directions, n), st));
    HIPCHK(c->qout.ensure(n * 3 * sizeof(double)));
    QueryEpoch query{c};
    HIPCHK(clear_query_counters(c, st));
    rr::LevelArgs A = query_level0(seed, jitter_mode);
    A.rays0 = c->rays0.as<double>();
    int rc = run_levels(c, frame_facts(c, remaining), A, n, remaining, c->qout.as<double>(), st);
    if (rc != RR_OK) return rc;
    HIPCHK(hipMemcpyAsync(out_rgb, c->qout.p, n * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    // the counters on the same (non-blocking) stream, then wait: out_rgb and the counters are both
    // complete on return, whatever kind of host memory the caller passed
    HIPCHK(hipMemcpyAsync(c->h_counters, frame_counters(c, 2), kCounterBytes, hipMemcpyDeviceToHost, st));
    HIPCHK(st.close());
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
    EntryScope st{c, nullptr};
    HIPCHK(st.open());
    std::vector<double> buf((size_t)n * 6);
    std::memcpy(buf.data(), points, n * 3 * sizeof(double));
    std::memcpy(buf.data() + 3 * n, light_positions, n * 3 * sizeof(double));
    HIPCHK(upload(c->rays0, buf, st));
    HIPCHK(c->qout.ensure(n * sizeof(int32_t)));
    HIPCHK(rr::launch_shadow_query(c->S, c->rays0.as<double>(), c->rays0.as<double>() + 3 * n, n,
                                   c->qout.as<int32_t>(), frame_counters(c, 2), st));
    HIPCHK(hipMemcpyAsync(out, c->qout.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(st.close());
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
    EntryScope st{c, nullptr};
    HIPCHK(st.open());
    HIPCHK(upload(c->rays0, pack_rays(origins, directions, n), st));
    rr::HitOut O;
    size_t d_bytes = 0;
    const size_t i_bytes = (size_t)n * 2 * sizeof(int32_t);
    HIPCHK(hit_planes(c, n, &O, &d_bytes));
    HIPCHK(clear_query_counters(c, st));
    rr::LevelArgs A = hit_level0(c);
    A.rays0 = c->rays0.as<double>();
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
    HIPCHK(st.close());
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

// ---- device-resident ray queries (render_rays.hip) ----
// The caller's buffers go to the kernels as they are (LevelArgs.rays0 / out, launch_shadow_query's arrays); nothing is
// staged but rr_hit_at_device's planes, nothing is copied to the host and nothing waits.  None of them touches the
// frames' state: no tile_bundles (tiles_valid), no order, no begin_frame_counters (persist_last), counters in buffer 2.
int rr_camera_rays_device(rr_ctx* c, const rr_camera* cam, void* d_rays, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!c || !cam || !d_rays) return fail(RR_E_ARG, "rr_camera_rays_device: null argument");
    if (int e = ctx_check(c, "device-resident ray queries need", false)) return e;
    if (cam->hsize < 1 || cam->vsize < 1) return fail(RR_E_ARG, "camera sizes must be >= 1");
    if (cam->hsize >= ((int64_t)1 << 32) || cam->vsize >= ((int64_t)1 << 32) ||
        cam->hsize * cam->vsize >= ((int64_t)1 << 32))
        return fail(RR_E_LIMIT, "a camera's rays must number fewer than 2^32");
    HIPCHK(hipSetDevice(c->device));
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    rr::LevelArgs A{};
    set_camera(A, cam);  // the frames' DevCamera and affine flag
    HIPCHK(rr::launch_camera_rays(A.cam, A.cam_affine != 0, cam->hsize * cam->vsize, static_cast<double*>(d_rays), st));
    HIPCHK(st.close());
    return RR_OK;
}

int rr_color_at_device(rr_ctx* c, int64_t n, const void* d_rays, int32_t remaining, uint64_t seed, int32_t jitter_mode,
                       void* d_rgb, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = rays_check(c, n, !d_rays || !d_rgb);
    if (rc != RR_OK) return rc;
    if (remaining < 0 || remaining > RR_MAX_DEPTH) return fail(RR_E_LIMIT, "remaining out of range");
    if (n == 0) return RR_OK;
    HIPCHK(hipSetDevice(c->device));
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    HIPCHK(st.start_timer());
    QueryEpoch query{c};
    HIPCHK(clear_query_counters(c, st));
    rr::LevelArgs A = query_level0(seed, jitter_mode);  // rr_color_at's level 0 on the caller's rays: sample i's jitter identity is (i, path 1)
    A.rays0 = static_cast<const double*>(d_rays);
    rc = run_levels(c, frame_facts(c, remaining), A, n, remaining, static_cast<double*>(d_rgb), st);
    if (rc != RR_OK) return rc;
    HIPCHK(st.close_counted(n));
    return RR_OK;
}

int rr_hit_at_device(rr_ctx* c, int64_t n, const void* d_rays, void* d_hits, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = rays_check(c, n, !d_rays || !d_hits);
    if (rc != RR_OK) return rc;
    if (n == 0) return RR_OK;
    const rr::RayPassPlan plan = rr::plan_ray_passes(n, c->batch);
    HIPCHK(hipSetDevice(c->device));
    rr::HitOut O;  // one pass's records (never more than kRayPassMax * 192 bytes, whatever n is)
    HIPCHK(hit_planes(c, plan.pass, &O));
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    HIPCHK(st.start_timer());
    HIPCHK(clear_query_counters(c, st));
    rr::LevelArgs A = hit_level0(c);
    for (int64_t first = 0; first < n; first += plan.pass) {  // a pass: the planes of its rays, then their records
        const int64_t np = std::min<int64_t>(plan.pass, n - first);
        A.rays0 = static_cast<const double*>(d_rays) + 6 * first;
        A.n = np;
        set_level0_index(A);
        HIPCHK(rr::launch_hit(c->S, A, O, st));
        HIPCHK(rr::launch_hit_records(O, np, static_cast<char*>(d_hits) + sizeof(rr_hit) * (size_t)first, st));
    }
    HIPCHK(st.close_counted(n));
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
    int rc = rays_check(c, n, !d_rays || !d_perm, false);  // orders rays, reads no scene
    if (rc != RR_OK) return rc;
    if (n == 0) return RR_OK;
    HIPCHK(hipSetDevice(c->device));
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    rc = order_into(c, n, d_rays, static_cast<uint32_t*>(d_perm), st);
    if (rc != RR_OK) return rc;
    HIPCHK(st.close());
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
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    HIPCHK(st.start_timer());
    const uint32_t* perm = nullptr;
    rc = order_for(c, n, d_rays, d_perm, st, &perm);
    if (rc != RR_OK) return rc;
    QueryEpoch query{c};
    HIPCHK(clear_query_counters(c, st));
    rr::LevelArgs A = query_level0(seed, jitter_mode);  // rr_color_at_device's level 0 with slot t on ray perm[t]: its jitter identity is (perm[t], path 1)
    A.rays0 = static_cast<const double*>(d_rays);
    A.list = perm;
    rc = run_levels(c, frame_facts(c, remaining), A, n, remaining, static_cast<double*>(d_rgb), st);
    if (rc != RR_OK) return rc;
    HIPCHK(st.close_counted(n));
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
    rr::HitOut O;
    HIPCHK(hit_planes(c, plan.pass, &O));
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    HIPCHK(st.start_timer());
    const uint32_t* perm = nullptr;
    rc = order_for(c, n, d_rays, d_perm, st, &perm);
    if (rc != RR_OK) return rc;
    HIPCHK(clear_query_counters(c, st));
    rr::LevelArgs A = hit_level0(c);
    A.rays0 = static_cast<const double*>(d_rays);  // the whole batch: a pass's slots read rays anywhere in it
    for (int64_t first = 0; first < n; first += plan.pass) {  // a pass: positions [first, first + np) of the order
        const int64_t np = std::min<int64_t>(plan.pass, n - first);
        A.list = perm + first;
        A.n = np;
        set_level0_index(A);
        HIPCHK(rr::launch_hit_ordered(c->S, A, O, st));
        HIPCHK(rr::launch_hit_records_ordered(O, np, perm + first, d_hits, st));
    }
    HIPCHK(st.close_counted(n));
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
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    HIPCHK(rr::launch_shadow_query(c->S, static_cast<const double*>(d_points), static_cast<const double*>(d_light_positions),
                                   n, static_cast<int32_t*>(d_out), c->shadow_sink.as<unsigned long long>(), st));
    HIPCHK(st.close());
    return RR_OK;
}

}  // extern "C"
