// temporal_tap.hpp — temporal accumulation, rr_temporal (rray.h RR_HAS_TEMPORAL holds the definition):
// the camera constants of a call, packed once on the host, and tp_pixel, one pixel of the reprojection, its tap tests
// and the blend.  Header-only and __host__ __device__: temporal_kernel (render_temporal.inc) and the host entry
// rr_temporal_reference (api.cpp) call the same function, so the definition is testable without a device.  Plain f64
// in exactly the order written, compiled without contraction (-ffp-contract=off); only sqrt, fabs and floor.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RR_TP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RR_TP_HD inline
#endif

namespace rr {

// the terms of a call that are switched on (TpConst.terms)
enum : int32_t { TP_T_OBJECT = 1, TP_T_NORMAL = 2, TP_T_PLANE = 4 };

// One camera as the definition reads it: rows 0..2 of its inverse, its pixel geometry, and o = X_M(0, 0, 0), which
// is the same for every pixel and so computed once, by tp_camera, in the definition's order.
struct TpCamera {
    double inv[12];
    double o[3];
    double half_width, half_height, pixel_size;
};

// A call's constants: a kernel argument passed by value (440 bytes; uniform, so the compiler keeps what it reads in
// SGPRs).  T: rows 0..2 of the previous camera's transform.
struct TpConst {
    TpCamera cur, prev;
    double T[12];
    double alpha, sigma_plane, sigma_normal;
    int64_t W, H;
    int32_t terms;
    int32_t max_history;
    int32_t is_static;  // every field of the two rr_camera compares ==
    int32_t pad;
};
static_assert(sizeof(TpConst) == 440, "the temporal constants are 440 bytes");

// a frame's planes, typed (rr_temporal_frame's fields)
struct TpFrame {
    const double* image;
    const double* depth;
    const double* normal;
    const int32_t* object;
    const int32_t* count;
    const double* m2;
};

// X_M(x, y, z)[r] over rows 0..2 of M
RR_TP_HD void tp_xform(const double* M, double x, double y, double z, double* r) {
    for (int k = 0; k < 3; ++k) r[k] = ((M[4 * k] * x + M[4 * k + 1] * y) + M[4 * k + 2] * z) + M[4 * k + 3] * 1.0;
}

RR_TP_HD TpCamera tp_camera(const double inv[16], double half_width, double half_height, double pixel_size) {
    TpCamera c;
    for (int i = 0; i < 12; ++i) c.inv[i] = inv[i];
    tp_xform(c.inv, 0.0, 0.0, 0.0, c.o);
    c.half_width = half_width;
    c.half_height = half_height;
    c.pixel_size = pixel_size;
    return c;
}

// the unit direction of the pinhole ray through the centre of pixel (x, y); its origin is cam.o
RR_TP_HD void tp_ray_dir(const TpCamera& cam, int64_t x, int64_t y, double* dir) {
    const double wx = cam.half_width - ((double)x + 0.5) * cam.pixel_size;
    const double wy = cam.half_height - ((double)y + 0.5) * cam.pixel_size;
    double f[3];
    tp_xform(cam.inv, wx, wy, -1.0, f);
    const double dx = f[0] - cam.o[0], dy = f[1] - cam.o[1], dz = f[2] - cam.o[2];
    const double mag = sqrt((dx * dx + dy * dy) + dz * dz);
    dir[0] = dx / mag;
    dir[1] = dy / mag;
    dir[2] = dz / mag;
}

RR_TP_HD bool tp_void(const TpFrame& f, int64_t p) {
    if (!(f.depth[p] < (double)INFINITY)) return true;
    return f.object && f.object[p] < 0;
}

// Pixel p = (x, y) of a call: out[C], *n_out and, with HAS_M2, m2_out[C].  The planes are read where they lie in
// memory (global memory in the kernel); nothing is written but the three results.
template <int C, bool HAS_M2>
RR_TP_HD void tp_pixel(const TpConst& K, const TpFrame& cur, const TpFrame& prev, int64_t x, int64_t y, double* out,
                       int32_t* n_out, double* m2_out) {
    const int64_t p = y * K.W + x;
    double in[C];
    for (int c = 0; c < C; ++c) in[c] = cur.image[C * p + c];
    // the result of a void pixel and of a pixel without history
    for (int c = 0; c < C; ++c) out[c] = in[c];
    if (HAS_M2)
        for (int c = 0; c < C; ++c) m2_out[c] = in[c] * in[c];
    *n_out = 1;
    if (tp_void(cur, p)) return;

    const double z = cur.depth[p];
    double d[3], P[3];
    tp_ray_dir(K.cur, x, y, d);
    for (int r = 0; r < 3; ++r) P[r] = K.cur.o[r] + z * d[r];

    int64_t x0 = x, y0 = y;
    double ax = 0.0, ay = 0.0, te = z;
    int ntap = 1;
    if (!K.is_static) {
        double c[3];
        for (int r = 0; r < 3; ++r) c[r] = ((K.T[4 * r] * P[0] + K.T[4 * r + 1] * P[1]) + K.T[4 * r + 2] * P[2]) + K.T[4 * r + 3] * 1.0;
        if (!(c[2] < 0.0)) return;
        const double m = -c[2];
        const double sx = c[0] / m, sy = c[1] / m;
        const double fx = (K.prev.half_width - sx) / K.prev.pixel_size - 0.5;
        const double fy = (K.prev.half_height - sy) / K.prev.pixel_size - 0.5;
        if (!(fx > -1.0 && fx < (double)K.W && fy > -1.0 && fy < (double)K.H)) return;
        const double fx0 = floor(fx), fy0 = floor(fy);
        ax = fx - fx0;
        ay = fy - fy0;
        x0 = (int64_t)fx0;
        y0 = (int64_t)fy0;
        const double e0 = P[0] - K.prev.o[0], e1 = P[1] - K.prev.o[1], e2 = P[2] - K.prev.o[2];
        te = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
        ntap = 2;
    }
    double np[3] = {0.0, 0.0, 0.0};
    if (K.terms & (TP_T_NORMAL | TP_T_PLANE))
        for (int r = 0; r < 3; ++r) np[r] = cur.normal[3 * p + r];
    const int32_t idp = (K.terms & TP_T_OBJECT) ? cur.object[p] : 0;

    double acc[C], accm2[C];
    for (int c = 0; c < C; ++c) acc[c] = accm2[c] = 0.0;
    double ws = 0.0;
    int32_t nmin = INT32_MAX;
    bool any = false;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (i >= ntap || j >= ntap) continue;
            const int64_t qx = x0 + i, qy = y0 + j;
            const double w = K.is_static ? 1.0 : (i ? ax : 1.0 - ax) * (j ? ay : 1.0 - ay);
            if (qx < 0 || qx >= K.W || qy < 0 || qy >= K.H) continue;
            const int64_t q = qy * K.W + qx;
            if (tp_void(prev, q)) continue;
            const int32_t nq = prev.count[q];
            if (nq < 1) continue;
            if ((K.terms & TP_T_OBJECT) && prev.object[q] != idp) continue;
            if (K.terms & TP_T_NORMAL) {
                const double dot = (np[0] * prev.normal[3 * q] + np[1] * prev.normal[3 * q + 1]) + np[2] * prev.normal[3 * q + 2];
                if (!(1.0 - dot <= K.sigma_normal)) continue;
            }
            if (K.terms & TP_T_PLANE) {
                double dq[3];
                tp_ray_dir(K.prev, qx, qy, dq);
                const double zq = prev.depth[q];
                const double Q0 = K.prev.o[0] + zq * dq[0], Q1 = K.prev.o[1] + zq * dq[1], Q2 = K.prev.o[2] + zq * dq[2];
                const double g = (np[0] * (Q0 - P[0]) + np[1] * (Q1 - P[1])) + np[2] * (Q2 - P[2]);
                if (!(fabs(g) <= K.sigma_plane * te)) continue;
            }
            if (!(w > 0.0)) continue;
            for (int c = 0; c < C; ++c) acc[c] = acc[c] + w * prev.image[C * q + c];
            if (HAS_M2)
                for (int c = 0; c < C; ++c) accm2[c] = accm2[c] + w * prev.m2[C * q + c];
            ws = ws + w;
            nmin = nq < nmin ? nq : nmin;
            any = true;
        }
    }
    if (!any) return;
    const int64_t n1 = (int64_t)nmin + 1;
    const int32_t n = n1 < (int64_t)K.max_history ? (int32_t)n1 : K.max_history;
    double a = 1.0 / (double)n;
    if (a < K.alpha) a = K.alpha;
    for (int c = 0; c < C; ++c) {
        const double h = acc[c] / ws;
        out[c] = h + (in[c] - h) * a;
    }
    if (HAS_M2)
        for (int c = 0; c < C; ++c) {
            const double hm2 = accm2[c] / ws;
            m2_out[c] = hm2 + (in[c] * in[c] - hm2) * a;
        }
    *n_out = n;
}

}  // namespace rr
