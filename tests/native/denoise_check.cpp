// denoise_check.cpp — rray_amd/csrc/denoise_tap.hpp (the denoiser's definition, rray.h RR_HAS_DENOISE) on small frames
// whose results are derived by hand: weights are products of h = (1/16, 1/4, 3/8, 1/4, 1/16), so the sums below are exact
// dyadic fractions and each expectation is one correctly rounded division.  Built and run by tests/test_denoise_host.py
// with g++ (no device); prints "ok <name>" per case and returns the number of failures.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "denoise_tap.hpp"

namespace {

int failures = 0;
const double INF = std::numeric_limits<double>::infinity();
const double QNAN = std::numeric_limits<double>::quiet_NaN();

struct Frame {
    int64_t W, H;
    std::vector<double> in, depth, normal, albedo;
    std::vector<int32_t> object;
};

// the whole filter with the header's functions, as rr_denoise_reference runs it
template <int C>
std::vector<double> run(const Frame& f, int iterations, bool object, double sc, double sn, double sz, double sa) {
    const int64_t n = f.W * f.H;
    std::vector<rr::DnGuide> g((size_t)n);
    for (int64_t p = 0; p < n; ++p)
        g[(size_t)p] = rr::dn_guide(p, f.depth.empty() ? nullptr : f.depth.data(), f.normal.empty() ? nullptr : f.normal.data(),
                                    f.object.empty() ? nullptr : f.object.data(), f.albedo.empty() ? nullptr : f.albedo.data());
    const int32_t terms = (object ? rr::DN_T_OBJECT : 0) | (sc > 0.0 ? rr::DN_T_COLOR : 0) | (sn > 0.0 ? rr::DN_T_NORMAL : 0) |
                          (sz > 0.0 ? rr::DN_T_DEPTH : 0) | (sa > 0.0 ? rr::DN_T_ALBEDO : 0);
    std::vector<double> src = f.in, dst((size_t)n * C);
    for (int i = 0; i < iterations; ++i) {
        const rr::DnLevel L = rr::dn_level(terms, i, sc, sn, sz, sa);
        for (int64_t y = 0; y < f.H; ++y)
            for (int64_t x = 0; x < f.W; ++x) rr::dn_pixel<C>(L, f.W, f.H, x, y, src.data(), g.data(), dst.data() + C * (y * f.W + x));
        src = dst;
    }
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
    // a single pixel: the centre tap alone, (9/64 * v) / (9/64)
    {
        Frame f{1, 1, {2.0}, {}, {}, {}, {}};
        expect("one_pixel", run<1>(f, 8, false, 0.5, 0.0, 0.0, 0.0), {2.0});
        Frame c{1, 1, {2.0, 0.5, 64.0}, {}, {}, {}, {}};
        expect("one_pixel_rgb", run<3>(c, 3, false, 0.0, 0.0, 0.0, 0.0), {2.0, 0.5, 64.0});
    }
    // a row of five, no term on: only dy == 0 lies inside, so w = 3/8 * h[dx+2].  x = 0 sees dx = 0..2: ws = 3/8 * 11/16,
    // acc = 3/128 * 16; x = 1 sees dx = -1..2: ws = 3/8 * 15/16, acc = 3/32 * 16; x = 2 sees all five: ws = 3/8, acc = 9/64 * 16
    {
        Frame f{5, 1, {0.0, 0.0, 16.0, 0.0, 0.0}, {}, {}, {}, {}};
        const double e0 = 0.375 / (33.0 / 128.0), e1 = 1.5 / (45.0 / 128.0), e2 = 2.25 / 0.375;
        expect("row5_level0", run<1>(f, 1, false, 0.0, 0.0, 0.0, 0.0), {e0, e1, e2, e1, e0});
        // the column of five is the same by symmetry (dx == 0 only)
        Frame c{1, 5, f.in, {}, {}, {}, {}};
        expect("col5_level0", run<1>(c, 1, false, 0.0, 0.0, 0.0, 0.0), {e0, e1, e2, e1, e0});
        // level 1 has holes of 2: x = 2 sees x = 0, 2, 4 (dx = -1, 0, 1), x = 0 sees x = 0, 2, 4 (dx = 0, 1, 2),
        // x = 1 sees x = 1, 3 (dx = 0, 1)
        const double w0 = 0.375 * 0.375, w1 = 0.375 * 0.25, w2 = 0.375 * 0.0625;
        const double l2 = ((w1 * e0 + w0 * e2) + w1 * e0) / ((w1 + w0) + w1);
        const double l0 = ((w0 * e0 + w1 * e2) + w2 * e0) / ((w0 + w1) + w2);
        const double l1 = (w0 * e1 + w1 * e1) / (w0 + w1);
        // x = 3 sees x = 1, 3 as dx = -1, 0 and x = 4 sees x = 0, 2, 4 as dx = -2, -1, 0: the sums run the other way
        const double l3 = (w1 * e1 + w0 * e1) / (w1 + w0);
        const double l4 = ((w2 * e0 + w1 * e2) + w0 * e0) / ((w2 + w1) + w0);
        expect("row5_level1", run<1>(f, 2, false, 0.0, 0.0, 0.0, 0.0), {l0, l1, l2, l3, l4});
    }
    // a void pixel keeps its value and is no tap: x = 0 sees dx = 0 and dx = 2, ws = 9/64 + 3/128, acc = 9/64 * 8; x = 2
    // sees dx = -2 and dx = 0, acc = 3/128 * 8
    {
        Frame f{3, 1, {8.0, 100.0, 0.0}, {1.0, INF, 1.0}, {}, {}, {}};
        expect("void_depth", run<1>(f, 1, false, 0.0, 0.0, 0.0, 0.0), {1.125 / (21.0 / 128.0), 100.0, 0.1875 / (21.0 / 128.0)});
        Frame o{3, 1, {8.0, 100.0, 0.0}, {}, {}, {}, {0, -1, 0}};
        expect("void_object", run<1>(o, 1, false, 0.0, 0.0, 0.0, 0.0), {1.125 / (21.0 / 128.0), 100.0, 0.1875 / (21.0 / 128.0)});
        Frame n{3, 1, {8.0, 100.0, 0.0}, {1.0, QNAN, 1.0}, {}, {}, {}};
        expect("void_nan_depth", run<1>(n, 1, false, 0.0, 0.0, 0.0, 0.0), {1.125 / (21.0 / 128.0), 100.0, 0.1875 / (21.0 / 128.0)});
        Frame big{3, 1, {8.0, 100.0, 0.0}, {1.0, 1e300, 1.0}, {}, {}, {}};  // rounds to +inf as a float
        expect("void_huge_depth", run<1>(big, 1, false, 0.0, 0.0, 0.0, 0.0), {1.125 / (21.0 / 128.0), 100.0, 0.1875 / (21.0 / 128.0)});
    }
    // two objects never mix with RR_DN_OBJECT, and do without
    {
        Frame f{4, 1, {1.0, 1.0, 5.0, 5.0}, {}, {}, {}, {0, 0, 1, 1}};
        expect("object_seam", run<1>(f, 3, true, 0.0, 0.0, 0.0, 0.0), {1.0, 1.0, 5.0, 5.0});
        const std::vector<double> mixed = run<1>(f, 1, false, 0.0, 0.0, 0.0, 0.0);
        if (mixed[1] > 1.0 && mixed[2] < 5.0)
            std::printf("ok object_off_mixes\n");
        else
            ++failures, std::printf("FAIL object_off_mixes\n");
    }
    // one term each on a pair of pixels, in = (0, 7) or (0, 1): the neighbour's weight is 3/32 * t^2 against 9/64
    {
        // depth: z = (4, 4.25), sigma 1/8: t = 1 - 0.25 / ((0.125 * 4) * 1) = 1/2 -> w = 3/128; out[0] = (3/128 * 7) / (21/128) = 1
        Frame z{2, 1, {0.0, 7.0}, {4.0, 4.25}, {}, {}, {}};
        const double t1 = 1.0 - 0.25 / ((0.125 * 4.25) * 1.0), w1 = (0.375 * 0.25) * (t1 * t1);
        expect("depth_term", run<1>(z, 1, false, 0.0, 0.0, 0.125, 0.0), {1.0, (0.140625 * 7.0) / (w1 + 0.140625)});
        // a larger step of depth is cut: t <= 0
        Frame zc{2, 1, {0.0, 7.0}, {4.0, 5.0}, {}, {}, {}};
        expect("depth_cut", run<1>(zc, 1, false, 0.0, 0.0, 0.125, 0.0), {0.0, 7.0});
        // a depth of exactly 0 divides by 0: the tap is skipped from the zero side (NaN or -inf), cut from the other
        Frame z0{2, 1, {0.0, 7.0}, {0.0, 0.0}, {}, {}, {}};
        expect("depth_zero", run<1>(z0, 1, false, 0.0, 0.0, 0.125, 0.0), {0.0, 7.0});
        // normal: (0,0,1) against (0,0,3/4), sigma 1/2: e = 1/4, t = 1/2 from both sides
        Frame n{2, 1, {0.0, 7.0}, {}, {0.0, 0.0, 1.0, 0.0, 0.0, 0.75}, {}, {}};
        expect("normal_term", run<1>(n, 1, false, 0.0, 0.5, 0.0, 0.0), {1.0, (0.140625 * 7.0) / (0.0234375 + 0.140625)});
        Frame nc{2, 1, {0.0, 7.0}, {}, {0.0, 0.0, 1.0, 0.0, 1.0, 0.0}, {}, {}};
        expect("normal_cut", run<1>(nc, 1, false, 0.0, 0.25, 0.0, 0.0), {0.0, 7.0});
        // normals of (0, 0, 0): dot = 0, e = 1, cut for sigma <= 1
        Frame n0{2, 1, {0.0, 7.0}, {}, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, {}, {}};
        expect("normal_zero", run<1>(n0, 1, false, 0.0, 0.25, 0.0, 0.0), {0.0, 7.0});
        // colour: d = 1, sigma 1: t = 2, w = 3/32 / 4 = 3/128: out = (3/128) / (21/128) and (9/64) / (21/128)
        Frame c{2, 1, {0.0, 1.0}, {}, {}, {}, {}};
        expect("colour_term", run<1>(c, 1, false, 1.0, 0.0, 0.0, 0.0), {0.0234375 / 0.1640625, 0.140625 / 0.1640625});
        // albedo: (0,0,0) against (1/2,0,0), sigma 1: t = 3/4, w = 3/32 * 9/16 = 27/512; ws = 99/512
        Frame a{2, 1, {0.0, 1.0}, {}, {}, {0.0, 0.0, 0.0, 0.5, 0.0, 0.0}, {}};
        expect("albedo_term", run<1>(a, 1, false, 0.0, 0.0, 0.0, 1.0), {(27.0 / 512.0) / (99.0 / 512.0), 0.140625 / (99.0 / 512.0)});
    }
    // a NaN colour stays where it is under the colour term and spreads without it
    {
        Frame f{2, 1, {QNAN, 1.0}, {}, {}, {}, {}};
        expect("nan_stays", run<1>(f, 2, false, 0.5, 0.0, 0.0, 0.0), {QNAN, 1.0});
        expect("nan_spreads", run<1>(f, 1, false, 0.0, 0.0, 0.0, 0.0), {QNAN, QNAN});
    }
    // guides are rounded to float when packed
    {
        const double d = 0.1, nrm[3] = {0.3, -0.7, 1e-50}, alb[3] = {1.0 / 3.0, 2.0 / 3.0, 1e39};
        const int32_t id = 7;
        const rr::DnGuide g = rr::dn_guide(0, &d, nrm, &id, alb);
        const bool ok = g.z == 0.1f && g.n[0] == 0.3f && g.n[1] == -0.7f && g.n[2] == 0.0f && g.a[0] == (float)(1.0 / 3.0) &&
                        g.a[1] == (float)(2.0 / 3.0) && std::isinf(g.a[2]) && g.id == 7 && !rr::dn_void(g);
        if (ok)
            std::printf("ok guide_rounding\n");
        else
            ++failures, std::printf("FAIL guide_rounding\n");
    }
    std::printf("%d failures\n", failures);
    return failures;
}
