// denoise_var_check.cpp — rray_amd/csrc/denoise_var_tap.hpp (variance-guided denoising's definition, rray.h
// RR_HAS_DENOISE_VAR) on small frames whose variance planes and filtered pixels are derived by hand: the weights are
// products of h = (1/16, 1/4, 3/8, 1/4, 1/16) and g = (1/4, 1/2, 1/4) and the inputs small dyadic numbers, so every sum
// below is exact and each expectation is at most one correctly rounded division away.  Built and run by
// tests/test_denoise_var_host.py with g++ (no device); prints "ok <name>" per case and returns the number of failures.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "denoise_var_tap.hpp"

namespace {

int failures = 0;
const double INF = std::numeric_limits<double>::infinity();
const double QNAN = std::numeric_limits<double>::quiet_NaN();

struct Frame {
    int64_t W, H;
    std::vector<double> in, depth;
    std::vector<int32_t> object;
    std::vector<double> m2;
    std::vector<int32_t> count;
};

std::vector<rr::DnGuide> guides(const Frame& f) {
    std::vector<rr::DnGuide> g((size_t)(f.W * f.H));
    for (int64_t p = 0; p < f.W * f.H; ++p)
        g[(size_t)p] = rr::dn_guide(p, f.depth.empty() ? nullptr : f.depth.data(), nullptr,
                                    f.object.empty() ? nullptr : f.object.data(), nullptr);
    return g;
}

// rr_variance_reference's loop
template <int C>
std::vector<double> variance(const Frame& f, int32_t min_history, bool object, double sz) {
    const std::vector<rr::DnGuide> g = guides(f);
    const int32_t terms = (object ? rr::DN_T_OBJECT : 0) | (sz > 0.0 ? rr::DN_T_DEPTH : 0);
    const rr::DnLevel G = rr::dv_guide_level(terms, 1, 0.0, sz, 0.0);
    std::vector<double> v((size_t)(f.W * f.H));
    for (int64_t y = 0; y < f.H; ++y)
        for (int64_t x = 0; x < f.W; ++x)
            v[(size_t)(y * f.W + x)] = rr::dv_variance<C>(G, min_history, f.W, f.H, x, y, f.in.data(), g.data(),
                                                          f.m2.empty() ? nullptr : f.m2.data(),
                                                          f.count.empty() ? nullptr : f.count.data());
    return v;
}

// rr_denoise_var_reference's loop: the image, then the variance plane behind it
template <int C>
std::vector<double> filter(const Frame& f, std::vector<double> var, int iterations, bool object, double sc, double sz,
                           double epsilon) {
    const std::vector<rr::DnGuide> g = guides(f);
    const int64_t n = f.W * f.H;
    const int32_t terms = (object ? rr::DN_T_OBJECT : 0) | (sc > 0.0 ? rr::DN_T_COLOR : 0) | (sz > 0.0 ? rr::DN_T_DEPTH : 0);
    std::vector<double> src = f.in, dst((size_t)n * C), vdst((size_t)n);
    for (int i = 0; i < iterations; ++i) {
        const rr::DnLevel L = rr::dv_level(terms, i, sc, 0.0, sz, 0.0);
        for (int64_t y = 0; y < f.H; ++y)
            for (int64_t x = 0; x < f.W; ++x)
                rr::dv_pixel<C>(L, epsilon, f.W, f.H, x, y, src.data(), var.data(), g.data(), dst.data() + C * (y * f.W + x),
                                vdst.data() + (y * f.W + x));
        src = dst;
        var = vdst;
    }
    src.insert(src.end(), var.begin(), var.end());
    return src;
}

bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0 || (std::isnan(a) && std::isnan(b)); }

void expect(const char* name, const std::vector<double>& got, const std::vector<double>& want) {
    bool ok = got.size() == want.size();
    for (size_t i = 0; ok && i < got.size(); ++i) ok = same(got[i], want[i]);
    if (ok) {
        std::printf("ok %s\n", name);
        return;
    }
    ++failures;
    std::printf("FAIL %s:", name);
    for (size_t i = 0; i < got.size(); ++i) std::printf(" %.17g (want %.17g)", got[i], i < want.size() ? want[i] : QNAN);
    std::printf("\n");
}

}  // namespace

int main() {
    // ---- rr_variance ----
    // one pixel alone: s1 = f, s2 = f f, ws = 1: v = f f - f f = 0
    {
        Frame f{1, 1, {3.0}, {}, {}, {}, {}};
        expect("var_one_pixel", variance<1>(f, 4, false, 0.0), {0.0});
    }
    // a pair (0, 2) with no guide: both pixels see both with w = 1: s1 = 2, s2 = 4, ws = 2, m = 1, v = 2 - 1 = 1
    {
        Frame f{2, 1, {0.0, 2.0}, {}, {}, {}, {}};
        expect("var_pair", variance<1>(f, 4, false, 0.0), {1.0, 1.0});
        // three channels (0, 0, 0) and (2, 4, 6): v = 1, 4, 9, V = (1 + 4) + 9
        Frame c{2, 1, {0.0, 0.0, 0.0, 2.0, 4.0, 6.0}, {}, {}, {}, {}};
        expect("var_pair_rgb", variance<3>(c, 4, false, 0.0), {14.0, 14.0});
        // a column is the same
        Frame r{1, 2, {0.0, 2.0}, {}, {}, {}, {}};
        expect("var_column", variance<1>(r, 4, false, 0.0), {1.0, 1.0});
    }
    // the window reaches 3 pixels and no further: a row (0, 0, 0, 0, 8) gives pixel 0 four zeros (V = 0), pixel 1 five
    // values: s1 = 8, s2 = 64, ws = 5: m = 8/5, v = 64/5 - m m, and so pixels 2 and 3; pixel 4 sees four: m = 2, v = 16 - 4
    {
        Frame f{5, 1, {0.0, 0.0, 0.0, 0.0, 8.0}, {}, {}, {}, {}};
        const double m = 8.0 / 5.0, v = 64.0 / 5.0 - m * m;
        expect("var_window_reach", variance<1>(f, 4, false, 0.0), {0.0, v, v, v, 12.0});
    }
    // a void pixel has V = 0 and is no tap: (0, 100, 2) with the middle void
    {
        Frame f{3, 1, {0.0, 100.0, 2.0}, {1.0, INF, 1.0}, {}, {}, {}};
        expect("var_void_depth", variance<1>(f, 4, false, 0.0), {1.0, 0.0, 1.0});
        Frame o{3, 1, {0.0, 100.0, 2.0}, {}, {0, -1, 0}, {}, {}};
        expect("var_void_object", variance<1>(o, 4, false, 0.0), {1.0, 0.0, 1.0});
    }
    // the object term cuts the pair apart; without it they mix
    {
        Frame f{2, 1, {0.0, 2.0}, {}, {0, 1}, {}, {}};
        expect("var_object_seam", variance<1>(f, 4, true, 0.0), {0.0, 0.0});
        expect("var_object_off", variance<1>(f, 4, false, 0.0), {1.0, 1.0});
    }
    // the depth term with step 1: z = (4, 4.25), sigma 1/8: from pixel 0 t = 1 - 0.25 / ((0.125 * 4) * 1) = 1/2, w = 1/4:
    // s1 = 1/2, s2 = 1, ws = 5/4; from pixel 1 t = 1 - 0.25 / (0.125 * 4.25), the tap is in = 0: s1 = 2, s2 = 4, ws = 1 + w
    {
        Frame f{2, 1, {0.0, 2.0}, {4.0, 4.25}, {}, {}, {}};
        const double m0 = 0.5 / 1.25, v0 = 1.0 / 1.25 - m0 * m0;
        const double t1 = 1.0 - 0.25 / ((0.125 * 4.25) * 1.0), ws1 = (1.0 * (t1 * t1)) + 1.0;
        const double m1 = 2.0 / ws1, v1 = 4.0 / ws1 - m1 * m1;
        expect("var_depth_term", variance<1>(f, 4, false, 0.125), {v0, v1});
        Frame cut{2, 1, {0.0, 2.0}, {4.0, 5.0}, {}, {}, {}};
        expect("var_depth_cut", variance<1>(cut, 4, false, 0.125), {0.0, 0.0});
    }
    // the temporal branch: count >= min_history: v = m2 - in in clamped at 0, divided by the count
    {
        Frame f{4, 1, {3.0, 3.0, 3.0, 3.0}, {}, {}, {10.0, 9.0, 8.0, 10.0}, {4, 4, 4, 3}};
        // 10 - 9 = 1 -> 1/4; m2 == in in -> 0.0 exactly; m2 below in in -> clamped; count 3 < 4 -> spatial: constant row -> 0
        expect("var_temporal", variance<1>(f, 4, false, 0.0), {0.25, 0.0, 0.0, 0.0});
        Frame c{1, 1, {1.0, 2.0, 3.0}, {}, {}, {2.0, 3.0, 13.0}, {8}};
        expect("var_temporal_rgb", variance<3>(c, 1, false, 0.0), {((1.0 + 0.0) + 4.0) / 8.0});
        // min_history = 0 takes a count of 0 as it is: 1 / 0 and 0 / 0
        Frame z{2, 1, {3.0, 3.0}, {}, {}, {10.0, 9.0}, {0, 0}};
        expect("var_temporal_zero_count", variance<1>(z, 0, false, 0.0), {INF, QNAN});
        // a NaN moment is clamped to 0; a void pixel is 0 whatever its history
        Frame n{2, 1, {3.0, 3.0}, {1.0, INF}, {}, {QNAN, 100.0}, {4, 4}};
        expect("var_temporal_nan_void", variance<1>(n, 4, false, 0.0), {0.0, 0.0});
    }
    // a NaN colour in the window makes s1 NaN, and the clamp makes that 0
    {
        Frame f{2, 1, {QNAN, 2.0}, {}, {}, {}, {}};
        expect("var_nan_colour", variance<1>(f, 4, false, 0.0), {0.0, 0.0});
    }
    // ---- rr_denoise_var ----
    // one pixel: the centre tap alone: F' = (9/64 F) / (9/64), V' = ((9/64)^2 V) / (9/64)^2
    {
        Frame f{1, 1, {2.0}, {}, {}, {}, {}};
        expect("dv_one_pixel", filter<1>(f, {2.0}, 8, false, 4.0, 0.0, 1e-12), {2.0, 2.0});
        Frame c{1, 1, {2.0, 0.5, 64.0}, {}, {}, {}, {}};
        expect("dv_one_pixel_rgb", filter<3>(c, {0.5}, 3, false, 0.0, 0.0, 1.0), {2.0, 0.5, 64.0, 0.5});
    }
    // a row of five, colour term off, V = 1 everywhere: denoise_check's row5_level0 for F; the variance of pixel 2 is
    // sum (3/8 h_k)^2 / (3/8)^2 = sum h_k^2 = 70/256, of pixel 0 (taps dx = 0..2) 9/64 * 53/256 / (3/8 * 11/16)^2, of
    // pixel 1 (dx = -1..2) 9/64 * 69/256 / (3/8 * 15/16)^2
    {
        Frame f{5, 1, {0.0, 0.0, 16.0, 0.0, 0.0}, {}, {}, {}, {}};
        const double e0 = 0.375 / (33.0 / 128.0), e1 = 1.5 / (45.0 / 128.0), e2 = 2.25 / 0.375;
        const double w0 = 0.375 * 0.6875, w1 = 0.375 * 0.9375;
        const double v0 = (0.140625 * (53.0 / 256.0)) / (w0 * w0), v1 = (0.140625 * (69.0 / 256.0)) / (w1 * w1), v2 = 35.0 / 128.0;
        expect("dv_row5_plain", filter<1>(f, {1.0, 1.0, 1.0, 1.0, 1.0}, 1, false, 0.0, 0.0, 1.0), {e0, e1, e2, e1, e0, v0, v1, v2, v1, v0});
        Frame c{1, 5, f.in, {}, {}, {}, {}};
        expect("dv_col5_plain", filter<1>(c, {1.0, 1.0, 1.0, 1.0, 1.0}, 1, false, 0.0, 0.0, 1.0), {e0, e1, e2, e1, e0, v0, v1, v2, v1, v0});
    }
    // the interior pixel of a 5 x 5 constant-variance plane: V' = V (35/128)^2
    {
        Frame f{5, 5, std::vector<double>(25, 1.0), {}, {}, {}, {}};
        const std::vector<double> got = filter<1>(f, std::vector<double>(25, 4.0), 1, false, 0.0, 0.0, 1.0);
        expect("dv_interior_variance", {got[12], got[25 + 12]}, {1.0, 4.0 * (35.0 / 128.0) * (35.0 / 128.0)});
    }
    // the colour term on a pair (0, 1) with V = 1/2, sigma_color 1, epsilon 1/2: gv = (1/4 * 1/2 + 1/8 * 1/2) / (3/8) = 1/2,
    // den = 1 * 1/2 + 1/2 = 1, dc = 1, t = 2: the neighbour's weight is 3/32 / 4 = 3/128 against the centre's 9/64
    {
        Frame f{2, 1, {0.0, 1.0}, {}, {}, {}, {}};
        const double wc = 0.140625, wn = 0.0234375, ws = 0.1640625;
        const double v = ((wc * wc) * 0.5 + (wn * wn) * 0.5) / (ws * ws);
        expect("dv_colour_term", filter<1>(f, {0.5, 0.5}, 1, false, 1.0, 0.0, 0.5), {wn / ws, wc / ws, v, v});
        // the prefilter reads the neighbour's variance: V = (0, 3/2): gv = (1/8 * 3/2) / (3/8) = 1/2 at pixel 0 and
        // (1/4 * 3/2) / (3/8) = 1 at pixel 1: den = 1 and 3/2, t = 2 and 1 + 1 / 1.5
        const double t1 = 1.0 + 1.0 / 1.5, w1 = 0.09375 * (1.0 / (t1 * t1));
        expect("dv_prefilter", filter<1>(f, {0.0, 1.5}, 1, false, 1.0, 0.0, 0.5),
               {wn / ws, wc / (w1 + wc), ((wn * wn) * 1.5) / (ws * ws), ((wc * wc) * 1.5) / ((w1 + wc) * (w1 + wc))});
    }
    // zero variance: den = epsilon, t * t overflows for a large difference and the tap drops out by w > 0
    {
        const double big = std::ldexp(1.0, 300);  // dc = 2^600, t about 2^640, t * t = +inf, w = w * (1 / inf) = 0
        Frame f{2, 1, {0.0, big}, {}, {}, {}, {}};
        expect("dv_zero_variance_overflow", filter<1>(f, {0.0, 0.0}, 3, false, 4.0, 0.0, 1e-12), {0.0, big, 0.0, 0.0});
        // a void pixel keeps F and V and lends nothing to the prefilter or the taps: (8, 100, 0) with the middle void and
        // the colour term off: denoise_check's void_depth, and V' = sum w^2 V / ws^2 over the two taps
        Frame v{3, 1, {8.0, 100.0, 0.0}, {1.0, INF, 1.0}, {}, {}, {}};
        const double wc = 0.140625, wf = 0.0234375, ws = 21.0 / 128.0;
        expect("dv_void", filter<1>(v, {1.0, 7.0, 2.0}, 1, false, 0.0, 0.0, 1.0),
               {1.125 / ws, 100.0, 0.1875 / ws, ((wc * wc) * 1.0 + (wf * wf) * 2.0) / (ws * ws), 7.0,
                ((wf * wf) * 1.0 + (wc * wc) * 2.0) / (ws * ws)});
    }
    // a NaN variance at a pixel: its own den is NaN and every off-centre tap is skipped, so it keeps F (its V stays
    // NaN); the neighbour's prefilter takes the NaN in and it keeps F and its own V too.  An infinite variance: den = inf, t = 1, the
    // plain weights, V' = inf
    {
        Frame f{2, 1, {1.0, 3.0}, {}, {}, {}, {}};
        expect("dv_nan_variance", filter<1>(f, {QNAN, 1.0}, 1, false, 1.0, 0.0, 0.5), {1.0, 3.0, QNAN, 1.0});
        const double wc = 0.140625, wn = 0.09375;
        expect("dv_inf_variance", filter<1>(f, {INF, INF}, 1, false, 1.0, 0.0, 0.5),
               {(wc * 1.0 + wn * 3.0) / (wc + wn), (wn * 1.0 + wc * 3.0) / (wn + wc), INF, INF});
    }
    // a NaN colour stays where it is under the colour term and spreads without it
    {
        Frame f{2, 1, {QNAN, 1.0}, {}, {}, {}, {}};
        expect("dv_nan_colour_stays", filter<1>(f, {1.0, 1.0}, 2, false, 1.0, 0.0, 0.5), {QNAN, 1.0, 1.0, 1.0});
        const std::vector<double> got = filter<1>(f, {1.0, 1.0}, 1, false, 0.0, 0.0, 0.5);
        expect("dv_nan_colour_spreads", {got[0], got[1]}, {QNAN, QNAN});
    }
    // level 1 has holes of 2 pixels but the prefilter keeps step 1: a row of three, V = (0, 4, 0), level 0 with the colour
    // term off, then level 1 with it on reads V_1 of the neighbours at distance 1 while the taps lie at distance 2
    {
        Frame f{3, 1, {0.0, 0.0, 4.0}, {}, {}, {}, {}};
        const std::vector<double> l0 = filter<1>(f, {0.0, 4.0, 0.0}, 1, false, 0.0, 0.0, 0.5);
        // by hand for pixel 0 at level 1 (taps dx = 0, 1 at x = 0, 2): gv = (1/4 V1[0] + 1/8 V1[1]) / (3/8)
        const double F0 = l0[0], F2 = l0[2], V0 = l0[3], V1 = l0[4], V2 = l0[5];
        const double gv = (0.25 * V0 + 0.125 * V1) / 0.375, den = 1.0 * gv + 0.5;
        const double d = F0 - F2, t = 1.0 + (d * d) / den, w = 0.09375 * (1.0 / (t * t)), wc = 0.140625;
        const double want_f = (wc * F0 + w * F2) / (wc + w), want_v = ((wc * wc) * V0 + (w * w) * V2) / ((wc + w) * (wc + w));
        Frame g{3, 1, {l0[0], l0[1], l0[2]}, {}, {}, {}, {}};
        const rr::DnLevel L = rr::dv_level(rr::DN_T_COLOR, 1, 1.0, 0.0, 0.0, 0.0);
        const std::vector<rr::DnGuide> gd = guides(g);
        const double vin[3] = {V0, V1, V2};
        double fo, vo;
        rr::dv_pixel<1>(L, 0.5, 3, 1, 0, 0, g.in.data(), vin, gd.data(), &fo, &vo);
        expect("dv_level1_prefilter_step", {fo, vo}, {want_f, want_v});
    }
    std::printf("%d failures\n", failures);
    return failures;
}
