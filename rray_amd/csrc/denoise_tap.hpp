// denoise_tap.hpp — the edge-avoiding a-trous filter of rr_denoise (rray.h RR_HAS_DENOISE holds the
// definition): a pixel's packed guide record, the weight of one tap and the accumulation loop of one pixel of one
// level.  Header-only and __host__ __device__: denoise_level_kernel (render_denoise.inc) and the host entry
// rr_denoise_reference (api.cpp) call the same functions, so the definition is testable without a device.  Plain f64
// in exactly the order written, compiled without contraction (-ffp-contract=off); no transcendental function.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RR_DN_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RR_DN_HD inline
#endif

namespace rr {

// the terms of a call that are switched on (DnLevel.terms)
enum : int32_t { DN_T_OBJECT = 1, DN_T_COLOR = 2, DN_T_NORMAL = 4, DN_T_DEPTH = 8, DN_T_ALBEDO = 16 };

// A pixel's guides, rounded to float as the definition reads them, packed once per call: 32 bytes.  id < 0 marks a
// void pixel: with an object plane a negative id is void by definition, and a pixel that is void by its depth gets
// id -1 (a void pixel's id is never compared).  A plane that is not given packs as zeros.  16-byte aligned: a record
// is two 16-byte loads.
struct alignas(16) DnGuide {
    float z;
    float n[3];
    float a[3];
    int32_t id;
};
static_assert(sizeof(DnGuide) == 32, "a guide record is 32 bytes");

// One level's parameters: `step` = 2^i pixels between taps, sc2 = (sigma_color * 2^-i)^2, sa2 = sigma_albedo^2 (each the
// one rounded product the definition writes per tap).
struct DnLevel {
    int32_t terms;
    int32_t step;
    double sc2;
    double sigma_normal;
    double sigma_depth;
    double sa2;
};

RR_DN_HD DnGuide dn_guide(int64_t p, const double* depth, const double* normal, const int32_t* object,
                          const double* albedo) {
    DnGuide g;
    g.z = depth ? (float)depth[p] : 0.0f;
    for (int r = 0; r < 3; ++r) {
        g.n[r] = normal ? (float)normal[3 * p + r] : 0.0f;
        g.a[r] = albedo ? (float)albedo[3 * p + r] : 0.0f;
    }
    g.id = object ? object[p] : 0;
    if ((depth && !((double)g.z < (double)INFINITY)) || g.id < 0) g.id = -1;
    return g;
}

RR_DN_HD bool dn_void(const DnGuide& g) { return g.id < 0; }

// The weight of the off-centre tap q seen from p: w = h[dy+2] * h[dx+2] on entry, 0.0 for a tap that a term skips (the
// caller drops every tap whose weight is not > 0.0).  reach = max(|dx|, |dy|) * step, the tap's distance in pixels.
template <int C>
RR_DN_HD double dn_tap_weight(const DnLevel& L, double w, const double* fp, const double* fq, const DnGuide& gp,
                              const DnGuide& gq, int32_t reach) {
    if ((L.terms & DN_T_OBJECT) && gq.id != gp.id) return 0.0;
    if (L.terms & DN_T_COLOR) {
        const double d0 = fp[0] - fq[0];
        double dc = d0 * d0;
        if (C == 3) {
            const double d1 = fp[1] - fq[1], d2 = fp[2] - fq[2];
            dc = (d0 * d0 + d1 * d1) + d2 * d2;
        }
        const double t = 1.0 + dc / L.sc2;
        if (!(t > 0.0)) return 0.0;
        w = w * (1.0 / (t * t));
    }
    if (L.terms & DN_T_NORMAL) {
        const double dot = ((double)gp.n[0] * (double)gq.n[0] + (double)gp.n[1] * (double)gq.n[1]) +
                           (double)gp.n[2] * (double)gq.n[2];
        double e = 1.0 - dot;
        if (e < 0.0) e = 0.0;
        const double t = 1.0 - e / L.sigma_normal;
        if (!(t > 0.0)) return 0.0;
        w = w * (t * t);
    }
    if (L.terms & DN_T_DEPTH) {
        const double zp = (double)gp.z, zq = (double)gq.z;
        const double r = (double)reach;
        const double t = 1.0 - fabs(zp - zq) / ((L.sigma_depth * fabs(zp)) * r);
        if (!(t > 0.0)) return 0.0;
        w = w * (t * t);
    }
    if (L.terms & DN_T_ALBEDO) {
        const double a0 = (double)gp.a[0] - (double)gq.a[0], a1 = (double)gp.a[1] - (double)gq.a[1],
                     a2 = (double)gp.a[2] - (double)gq.a[2];
        const double da = (a0 * a0 + a1 * a1) + a2 * a2;
        const double t = 1.0 - da / L.sa2;
        if (!(t > 0.0)) return 0.0;
        w = w * (t * t);
    }
    return w;
}

// F_{i+1}[p] of pixel p = (x, y): dy outer, dx inner, in the definition's order.  The level image and the guide records
// are read through `img(qx, qy, c)` and `guide(qx, qy)`, asked only for pixels inside the W x H frame: global memory on
// the host and in the direct kernel, a staged tile in the LDS kernel — the arithmetic is this one function either way.
template <int C, class Img, class Guide>
RR_DN_HD void dn_pixel_at(const DnLevel& L, int64_t W, int64_t H, int64_t x, int64_t y, const Img& img, const Guide& guide,
                          double* out) {
    const DnGuide gp = guide(x, y);
    double fp[C];
    for (int c = 0; c < C; ++c) fp[c] = img(x, y, c);
    if (dn_void(gp)) {
        for (int c = 0; c < C; ++c) out[c] = fp[c];
        return;
    }
    const double h[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    double acc[C];
    for (int c = 0; c < C; ++c) acc[c] = 0.0;
    double ws = 0.0;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int64_t qy = y + (int64_t)dy * L.step;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int64_t qx = x + (int64_t)dx * L.step;
            if (qx < 0 || qx >= W) continue;
            const DnGuide gq = guide(qx, qy);
            if (dn_void(gq)) continue;
            double fq[C];
            for (int c = 0; c < C; ++c) fq[c] = img(qx, qy, c);
            double w = h[dy + 2] * h[dx + 2];
            if (dx != 0 || dy != 0) {
                const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
                w = dn_tap_weight<C>(L, w, fp, fq, gp, gq, (ax > ay ? ax : ay) * L.step);
            }
            if (!(w > 0.0)) continue;
            for (int c = 0; c < C; ++c) acc[c] = acc[c] + w * fq[c];
            ws = ws + w;
        }
    }
    for (int c = 0; c < C; ++c) out[c] = acc[c] / ws;
}

// the image and the records where they lie in memory: F is W x H x C doubles, G is W x H records
template <int C>
struct DnImageAt {
    const double* F;
    int64_t W;
    RR_DN_HD double operator()(int64_t x, int64_t y, int c) const { return F[C * (y * W + x) + c]; }
};
struct DnGuideAt {
    const DnGuide* G;
    int64_t W;
    RR_DN_HD DnGuide operator()(int64_t x, int64_t y) const { return G[y * W + x]; }
};
template <int C>
RR_DN_HD void dn_pixel(const DnLevel& L, int64_t W, int64_t H, int64_t x, int64_t y, const double* F, const DnGuide* G,
                       double* out) {
    dn_pixel_at<C>(L, W, H, x, y, DnImageAt<C>{F, W}, DnGuideAt{G, W}, out);
}

// the parameters of level i: holes of 2^i pixels, sigma_color halved per level (exact)
RR_DN_HD DnLevel dn_level(int32_t terms, int32_t i, double sigma_color, double sigma_normal, double sigma_depth,
                          double sigma_albedo) {
    DnLevel L;
    L.terms = terms;
    L.step = (int32_t)1 << i;
    const double sc = sigma_color * (1.0 / (double)((int32_t)1 << i));
    L.sc2 = sc * sc;
    L.sigma_normal = sigma_normal;
    L.sigma_depth = sigma_depth;
    L.sa2 = sigma_albedo * sigma_albedo;
    return L;
}

}  // namespace rr
