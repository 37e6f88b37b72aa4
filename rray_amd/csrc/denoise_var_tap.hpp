// denoise_var_tap.hpp — variance-guided denoising (rray.h RR_HAS_DENOISE_VAR holds the definition):
// the per-pixel noise estimate of one pixel (rr_variance) and one level of one pixel of the a-trous filter whose colour
// tolerance follows that estimate (rr_denoise_var).  Header-only and __host__ __device__ like denoise_tap.hpp, whose
// guide records and guide terms it uses: variance_kernel and denoise_var_level_kernel (render_denoise_var.inc), the host
// entries rr_variance_reference and rr_denoise_var_reference (api.cpp) and tests/native/denoise_var_check.cpp call the
// same functions.  Plain f64 in exactly the order written, compiled without contraction; the only functions are fabs
// and the comparisons.
#pragma once
#include "denoise_tap.hpp"

namespace rr {

// The guide terms of the off-centre tap q seen from p applied to the starting weight w: the object, normal, depth and
// albedo terms of rr_denoise in that order — dn_tap_weight with the colour bit cleared, so there is one definition.
// `G` is a level whose terms hold no DN_T_COLOR (dv_guide_level); the colours are not read.
RR_DN_HD double dv_guide_weight(const DnLevel& G, double w, const DnGuide& gp, const DnGuide& gq, int32_t reach) {
    const double none[1] = {0.0};
    return dn_tap_weight<1>(G, w, none, none, gp, gq, reach);
}

// a level's guide terms alone: holes of `step` pixels, the colour bit cleared
RR_DN_HD DnLevel dv_guide_level(int32_t terms, int32_t step, double sigma_normal, double sigma_depth, double sigma_albedo) {
    DnLevel G;
    G.terms = terms & ~DN_T_COLOR;
    G.step = step;
    G.sc2 = 0.0;
    G.sigma_normal = sigma_normal;
    G.sigma_depth = sigma_depth;
    G.sa2 = sigma_albedo * sigma_albedo;
    return G;
}

RR_DN_HD double dv_clamp(double v) { return v > 0.0 ? v : 0.0; }  // !(v > 0.0) -> 0.0, so a NaN becomes 0.0

// the channels' sum in the definition's order
template <int C>
RR_DN_HD double dv_sum(const double* v) {
    if constexpr (C == 3)
        return (v[0] + v[1]) + v[2];
    else
        return v[0];
}

// dc of rr_denoise's colour term: the squared colour distance of two pixels
template <int C>
RR_DN_HD double dv_dc(const double* fp, const double* fq) {
    const double d0 = fp[0] - fq[0];
    if constexpr (C == 3) {
        const double d1 = fp[1] - fq[1], d2 = fp[2] - fq[2];
        return (d0 * d0 + d1 * d1) + d2 * d2;
    } else {
        return d0 * d0;
    }
}

// V_0 of pixel p = (x, y) (rr_variance).  G: dv_guide_level(terms, 1, ...).  m2 and count are rr_temporal's planes
// (W x H x C doubles, W x H int32) or both null; they are read at p only.  The image and the records are read through
// `img(qx, qy, c)` and `guide(qx, qy)`, asked only for pixels inside the frame, as by dn_pixel_at.
template <int C, class Img, class Guide>
RR_DN_HD double dv_variance_at(const DnLevel& G, int32_t min_history, int64_t W, int64_t H, int64_t x, int64_t y,
                               const Img& img, const Guide& guide, const double* m2, const int32_t* count) {
    const DnGuide gp = guide(x, y);
    if (dn_void(gp)) return 0.0;
    if (count) {
        const int64_t p = y * W + x;
        const int32_t n = count[p];
        if (n >= min_history) {  // the temporal branch: the variance of the accumulated mean
            double v[C];
            for (int c = 0; c < C; ++c) {
                const double f = img(x, y, c);
                v[c] = dv_clamp(m2[C * p + c] - f * f);
            }
            return dv_sum<C>(v) / (double)n;
        }
    }
    // the spatial branch: the guided second moment of the 7 x 7 window
    double s1[C], s2[C];
    for (int c = 0; c < C; ++c) s1[c] = s2[c] = 0.0;
    double ws = 0.0;
    for (int dy = -3; dy <= 3; ++dy) {
        const int64_t qy = y + dy;
        if (qy < 0 || qy >= H) continue;
        for (int dx = -3; dx <= 3; ++dx) {
            const int64_t qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            const DnGuide gq = guide(qx, qy);
            if (dn_void(gq)) continue;
            double w = 1.0;
            if (dx != 0 || dy != 0) {
                const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
                w = dv_guide_weight(G, w, gp, gq, ax > ay ? ax : ay);
            }
            if (!(w > 0.0)) continue;
            for (int c = 0; c < C; ++c) {
                const double f = img(qx, qy, c);
                s1[c] = s1[c] + w * f;
                s2[c] = s2[c] + w * (f * f);
            }
            ws = ws + w;
        }
    }
    double v[C];
    for (int c = 0; c < C; ++c) {
        const double m = s1[c] / ws;
        v[c] = dv_clamp(s2[c] / ws - m * m);
    }
    return dv_sum<C>(v);
}

// F_{i+1}[p] and V_{i+1}[p] of pixel p = (x, y) (rr_denoise_var).  L: dn_level's fields with sc2 = sigma_color *
// sigma_color at every level (dv_level) — DN_T_COLOR in L.terms says that the colour term is on.  `var(qx, qy)` reads
// V_i like `img` reads F_i.
template <int C, class Img, class Var, class Guide>
RR_DN_HD void dv_pixel_at(const DnLevel& L, double epsilon, int64_t W, int64_t H, int64_t x, int64_t y, const Img& img,
                          const Var& var, const Guide& guide, double* out, double* vout) {
    const DnGuide gp = guide(x, y);
    double fp[C];
    for (int c = 0; c < C; ++c) fp[c] = img(x, y, c);
    if (dn_void(gp)) {
        for (int c = 0; c < C; ++c) out[c] = fp[c];
        *vout = var(x, y);
        return;
    }
    // the prefiltered variance of p: a 3 x 3 binomial over V_i at step 1, once per pixel
    const double g[3] = {1.0 / 4.0, 1.0 / 2.0, 1.0 / 4.0};
    double ga = 0.0, gs = 0.0;
#pragma unroll
    for (int ey = -1; ey <= 1; ++ey) {
        const int64_t qy = y + ey;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int ex = -1; ex <= 1; ++ex) {
            const int64_t qx = x + ex;
            if (qx < 0 || qx >= W) continue;
            if (dn_void(guide(qx, qy))) continue;
            const double gw = g[ey + 1] * g[ex + 1];
            ga = ga + gw * var(qx, qy);
            gs = gs + gw;
        }
    }
    const double gv = ga / gs;
    const double den = L.sc2 * gv + epsilon;
    DnLevel G = L;
    G.terms = L.terms & ~DN_T_COLOR;
    const double h[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    double acc[C];
    for (int c = 0; c < C; ++c) acc[c] = 0.0;
    double va = 0.0, ws = 0.0;
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
                w = dv_guide_weight(G, w, gp, gq, (ax > ay ? ax : ay) * L.step);
                if (L.terms & DN_T_COLOR) {
                    const double t = 1.0 + dv_dc<C>(fp, fq) / den;
                    if (!(t > 0.0)) continue;
                    w = w * (1.0 / (t * t));
                }
            }
            if (!(w > 0.0)) continue;
            for (int c = 0; c < C; ++c) acc[c] = acc[c] + w * fq[c];
            va = va + (w * w) * var(qx, qy);
            ws = ws + w;
        }
    }
    for (int c = 0; c < C; ++c) out[c] = acc[c] / ws;
    *vout = va / (ws * ws);
}

// a variance plane where it lies in memory: W x H doubles
struct DvVarAt {
    const double* V;
    int64_t W;
    RR_DN_HD double operator()(int64_t x, int64_t y) const { return V[y * W + x]; }
};
template <int C>
RR_DN_HD double dv_variance(const DnLevel& G, int32_t min_history, int64_t W, int64_t H, int64_t x, int64_t y,
                            const double* F, const DnGuide* Gd, const double* m2, const int32_t* count) {
    return dv_variance_at<C>(G, min_history, W, H, x, y, DnImageAt<C>{F, W}, DnGuideAt{Gd, W}, m2, count);
}
template <int C>
RR_DN_HD void dv_pixel(const DnLevel& L, double epsilon, int64_t W, int64_t H, int64_t x, int64_t y, const double* F,
                       const double* V, const DnGuide* Gd, double* out, double* vout) {
    dv_pixel_at<C>(L, epsilon, W, H, x, y, DnImageAt<C>{F, W}, DvVarAt{V, W}, DnGuideAt{Gd, W}, out, vout);
}

// the parameters of level i: holes of 2^i pixels; sigma_color is NOT halved per level (the shrinking variance narrows
// the colour term)
RR_DN_HD DnLevel dv_level(int32_t terms, int32_t i, double sigma_color, double sigma_normal, double sigma_depth,
                          double sigma_albedo) {
    DnLevel L = dn_level(terms, i, sigma_color, sigma_normal, sigma_depth, sigma_albedo);
    L.sc2 = sigma_color * sigma_color;
    return L;
}

}  // namespace rr
