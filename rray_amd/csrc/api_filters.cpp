// api_filters.cpp — the image filters of include/rray/rray.h: the edge-avoiding denoiser, the variance estimate and the
// variance-guided denoiser, and temporal accumulation, each with its host reference.  None reads a scene.
#include "api_ctx.hpp"

extern "C" {

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

int rr_denoise_device(rr_ctx* c, const rr_denoise_desc* d, int64_t W, int64_t H, int32_t C, const void* d_in,
                      const void* d_depth, const void* d_normal, const void* d_object, const void* d_albedo, void* d_out,
                      void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = ctx_check(c, "rr_denoise needs", false);
    if (rc != RR_OK) return rc;
    int32_t terms = 0;
    rc = dn_check(d, W, H, C, DnPlanes{d_in, d_depth, d_normal, d_object, d_albedo, d_out}, &terms);
    if (rc != RR_OK) return rc;
    const int64_t n = W * H;
    const size_t img = (size_t)n * (size_t)C * sizeof(double);
    HIPCHK(hipSetDevice(c->device));
    // the scratch is claimed before it may grow: a call on another stream may still read the buffers that ensure frees
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
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
    HIPCHK(st.close());
    return RR_OK;
}

int rr_denoise(rr_ctx* c, const rr_denoise_desc* d, int64_t W, int64_t H, int32_t C, const double* in, const double* depth,
               const double* normal, const int32_t* object, const double* albedo, double* out) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = ctx_check(c, "rr_denoise needs", false);
    if (rc != RR_OK) return rc;
    int32_t terms = 0;
    rc = dn_check(d, W, H, C, DnPlanes{in, depth, normal, object, albedo, out}, &terms);
    if (rc != RR_OK) return rc;
    const size_t n = (size_t)(W * H);
    const size_t img = n * C * sizeof(double);
    const void* host[6] = {out, in, depth, normal, object, albedo};
    const size_t bytes[6] = {img, img, n * sizeof(double), n * 3 * sizeof(double), n * sizeof(int32_t), n * 3 * sizeof(double)};
    void* dev[6];
    rc = stage_planes(c, c->dn_host, 6, 1, host, bytes, dev);
    if (rc != RR_OK) return rc;
    rc = rr_denoise_device(c, d, W, H, C, dev[1], dev[2], dev[3], dev[4], dev[5], dev[0], nullptr);
    if (rc != RR_OK) return rc;
    HIPCHK(hipMemcpyAsync(out, dev[0], img, hipMemcpyDeviceToHost, c->stream));
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
    int rc = ctx_check(c, "rr_variance needs", false);
    if (rc != RR_OK) return rc;
    int32_t terms = 0;
    rc = var_check(d, W, H, C, VarPlanes{d_in, d_m2, d_count, d_depth, d_normal, d_object, d_albedo, d_var}, &terms);
    if (rc != RR_OK) return rc;
    const int64_t n = W * H;
    HIPCHK(hipSetDevice(c->device));
    // the scratch is claimed before it may grow: a call on another stream may still read the buffers that ensure frees
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    if (c->dn_guides.bytes < (size_t)n * sizeof(rr::DnGuide))
        HIPCHK(hipStreamSynchronize(st));  // growing frees: nothing enqueued may still use the old buffer
    HIPCHK(c->dn_guides.ensure((size_t)n * sizeof(rr::DnGuide)));
    rr::DnGuide* g = c->dn_guides.as<rr::DnGuide>();
    HIPCHK(rr::launch_denoise_pack(n, static_cast<const double*>(d_depth), static_cast<const double*>(d_normal),
                                   static_cast<const int32_t*>(d_object), static_cast<const double*>(d_albedo), g, st));
    const rr::DnLevel G = rr::dv_guide_level(terms, 1, d->sigma_normal, d->sigma_depth, d->sigma_albedo);
    HIPCHK(rr::launch_variance(G, d->min_history, C, W, H, static_cast<const double*>(d_in), static_cast<const double*>(d_m2),
                               static_cast<const int32_t*>(d_count), g, static_cast<double*>(d_var), st));
    HIPCHK(st.close());
    return RR_OK;
}

int rr_variance(rr_ctx* c, const rr_variance_desc* d, int64_t W, int64_t H, int32_t C, const double* in, const double* m2,
                const int32_t* count, const double* depth, const double* normal, const int32_t* object, const double* albedo,
                double* var) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = ctx_check(c, "rr_variance needs", false);
    if (rc != RR_OK) return rc;
    int32_t terms = 0;
    rc = var_check(d, W, H, C, VarPlanes{in, m2, count, depth, normal, object, albedo, var}, &terms);
    if (rc != RR_OK) return rc;
    const size_t n = (size_t)(W * H), img = n * C * sizeof(double);
    const void* host[8] = {var, in, m2, count, depth, normal, object, albedo};
    const size_t bytes[8] = {n * sizeof(double), img, img, n * sizeof(int32_t), n * sizeof(double), n * 3 * sizeof(double),
                             n * sizeof(int32_t), n * 3 * sizeof(double)};
    void* dev[8];
    rc = stage_planes(c, c->dn_host, 8, 1, host, bytes, dev);
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
    int rc = ctx_check(c, "rr_denoise_var needs", false);
    if (rc != RR_OK) return rc;
    int32_t terms = 0;
    rr_denoise_desc base;
    rc = dv_check(d, W, H, C, DnPlanes{d_in, d_depth, d_normal, d_object, d_albedo, d_out}, d_var, d_var_out, &base, &terms);
    if (rc != RR_OK) return rc;
    const int64_t n = W * H;
    const size_t img = (size_t)n * (size_t)C * sizeof(double), vb = (size_t)n * sizeof(double);
    HIPCHK(hipSetDevice(c->device));
    // the scratch is claimed before it may grow: a call on another stream may still read the buffers that ensure frees
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
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
    HIPCHK(st.close());
    return RR_OK;
}

int rr_denoise_var(rr_ctx* c, const rr_denoise_var_desc* d, int64_t W, int64_t H, int32_t C, const double* in,
                   const double* var, const double* depth, const double* normal, const int32_t* object, const double* albedo,
                   double* out, double* var_out) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = ctx_check(c, "rr_denoise_var needs", false);
    if (rc != RR_OK) return rc;
    int32_t terms = 0;
    rr_denoise_desc base;
    rc = dv_check(d, W, H, C, DnPlanes{in, depth, normal, object, albedo, out}, var, var_out, &base, &terms);
    if (rc != RR_OK) return rc;
    const size_t n = (size_t)(W * H), img = n * C * sizeof(double);
    const void* host[8] = {out, var_out, in, var, depth, normal, object, albedo};
    const size_t bytes[8] = {img, n * sizeof(double), img, n * sizeof(double), n * sizeof(double), n * 3 * sizeof(double),
                             n * sizeof(int32_t), n * 3 * sizeof(double)};
    void* dev[8];
    rc = stage_planes(c, c->dn_host, 8, 2, host, bytes, dev);
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

int rr_temporal_device(rr_ctx* c, const rr_temporal_desc* d, int64_t W, int64_t H, int32_t C, const rr_camera* cam,
                       const rr_temporal_frame* cur, const rr_camera* prev_cam, const rr_temporal_frame* prev, void* d_out,
                       void* d_n_out, void* d_m2_out, void* hip_stream) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = ctx_check(c, "rr_temporal needs", false);
    if (rc != RR_OK) return rc;
    rr::TpConst K{};
    rr::TpFrame fc{}, fp{};
    rc = tp_check(d, W, H, C, cam, cur, prev_cam, prev, d_out, d_n_out, d_m2_out, &K, &fc, &fp);
    if (rc != RR_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    EntryScope st{c, hip_stream};
    HIPCHK(st.open());
    HIPCHK(rr::launch_temporal(K, C, fc, fp, c->tp_rows != 0, static_cast<double*>(d_out), static_cast<int32_t*>(d_n_out),
                               static_cast<double*>(d_m2_out), st));
    HIPCHK(st.close());
    return RR_OK;
}

int rr_temporal(rr_ctx* c, const rr_temporal_desc* d, int64_t W, int64_t H, int32_t C, const rr_camera* cam,
                const rr_temporal_frame* cur, const rr_camera* prev_cam, const rr_temporal_frame* prev, double* out,
                int32_t* n_out, double* m2_out) {
    rr::DeviceGuard device_guard;  // the caller's current device is restored on return
    int rc = ctx_check(c, "rr_temporal needs", false);
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
    void* dev[13];
    rc = stage_planes(c, c->tp_host, 13, 3, host, bytes, dev);
    if (rc != RR_OK) return rc;
    const rr_temporal_frame dc{dev[3], dev[4], dev[5], dev[6], nullptr, nullptr};
    const rr_temporal_frame dp{dev[7], dev[8], dev[9], dev[10], dev[11], dev[12]};
    rc = rr_temporal_device(c, d, W, H, C, cam, &dc, prev_cam, &dp, dev[0], dev[1], dev[2], nullptr);
    if (rc != RR_OK) return rc;
    for (int k = 0; k < 3; ++k)
        if (host[k]) HIPCHK(hipMemcpyAsync(const_cast<void*>(host[k]), dev[k], bytes[k], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return RR_OK;
}

}  // extern "C"
