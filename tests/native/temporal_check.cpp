// temporal_check.cpp — rray_amd/csrc/temporal_tap.hpp (temporal accumulation's definition, rray.h RR_HAS_TEMPORAL) on
// frames whose results are derived by hand.  Built and run by tests/test_temporal_host.py with g++ (no device); prints
// "ok <name>" per case and returns the number of failures.
//
// The wall: a camera at the origin looking down -z with the identity transform sees the plane z = -D.  Pixel x has
// wx = half_width - (x + 0.5) ps and its hit is (wx D, wy D, -D).  A previous camera with the transform translate(tx, 0,
// 0) sees that point at camera-space x = wx D + tx, so sx = wx + tx / D and fx = (half_width - sx) / ps - 0.5 =
// x - tx / (D ps): with tx = k ps D the history arrives shifted by exactly k pixels, fx = x - k, fy = y.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "temporal_tap.hpp"

namespace {

int failures = 0;
const double INF = std::numeric_limits<double>::infinity();

void report(const char* name, bool ok) {
    if (ok) {
        std::printf("ok %s\n", name);
        return;
    }
    ++failures;
    std::printf("FAIL %s\n", name);
}

bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// world -> camera translate(tx, ty, tz), optionally turned half round about y first (it then looks down +z)
void set_prev(rr::TpConst& K, double tx, bool turned, double hw, double hh, double ps) {
    const double s = turned ? -1.0 : 1.0;
    const double T[16] = {s, 0, 0, tx, 0, 1, 0, 0, 0, 0, s, 0, 0, 0, 0, 1};
    const double inv[16] = {s, 0, 0, -s * tx, 0, 1, 0, 0, 0, 0, s, 0, 0, 0, 0, 1};
    for (int i = 0; i < 12; ++i) K.T[i] = T[i];
    K.prev = rr::tp_camera(inv, hw, hh, ps);
}

struct Wall {
    static constexpr int64_t W = 8, H = 3;
    static constexpr double ps = 0.125, hw = 0.5, hh = 0.1875, D = 4.0;
    rr::TpConst K{};
    std::vector<double> in, depth, normal, hist, hist2;
    std::vector<int32_t> object, count;
    rr::TpFrame cur{}, prev{};

    Wall(double tx, bool turned = false) {
        const double id[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        K.cur = rr::tp_camera(id, hw, hh, ps);
        set_prev(K, tx, turned, hw, hh, ps);
        K.alpha = 0.0;
        K.sigma_plane = 0.01;
        K.sigma_normal = 0.1;
        K.W = W;
        K.H = H;
        K.terms = rr::TP_T_OBJECT | rr::TP_T_NORMAL | rr::TP_T_PLANE;
        K.max_history = 1 << 20;
        K.is_static = 0;
        const size_t n = (size_t)(W * H);
        in.assign(n, 0.0);
        depth.resize(n);
        normal.resize(3 * n);
        hist.resize(n);
        hist2.resize(n);
        object.assign(n, 0);
        count.assign(n, 1);
        for (int64_t y = 0; y < H; ++y)
            for (int64_t x = 0; x < W; ++x) {
                const size_t p = (size_t)(y * W + x);
                double d[3];
                rr::tp_ray_dir(K.cur, x, y, d);  // both cameras look the same way: one depth plane serves both
                depth[p] = D / -d[2];
                normal[3 * p] = 0.0, normal[3 * p + 1] = 0.0, normal[3 * p + 2] = 1.0;
                hist[p] = 10.0 * (double)x + (double)y + 1.0;
                hist2[p] = hist[p] * hist[p];
            }
        cur = rr::TpFrame{in.data(), depth.data(), normal.data(), object.data(), nullptr, nullptr};
        prev = rr::TpFrame{hist.data(), depth.data(), normal.data(), object.data(), count.data(), hist2.data()};
    }
};

// in = 0 and every count 1: n = 2, a = 1/2, out = h / 2 where a history arrives; out = 0 and n = 1 where none does
void wall_shift(const char* name, int k) {
    Wall w((double)k * Wall::ps * Wall::D);
    bool ok = true, left = true;
    for (int64_t y = 0; y < Wall::H; ++y)
        for (int64_t x = 0; x < Wall::W; ++x) {
            double out, m2;
            int32_t n;
            rr::tp_pixel<1, true>(w.K, w.cur, w.prev, x, y, &out, &n, &m2);
            if (x >= k) {
                const double want = w.hist[(size_t)(y * Wall::W + (x - k))];
                ok = ok && n == 2 && std::fabs(2.0 * out - want) <= 1e-12 * want && std::fabs(2.0 * m2 - want * want) <= 1e-12 * want * want;
            } else if (x <= k - 2) {
                left = left && n == 1 && same(out, 0.0) && same(m2, 0.0);
            } else {
                // fx = -1 up to rounding: no candidate, or column 0 with a weight of an ulp — its value either way
                const double want = w.hist[(size_t)(y * Wall::W)];
                left = left && ((n == 1 && same(out, 0.0)) || (n == 2 && std::fabs(2.0 * out - want) <= 1e-12 * want));
            }
        }
    report(name, ok);
    if (k == 3) report("wall_left_columns", left);
}

}  // namespace

int main() {
    wall_shift("wall_shift_0", 0);
    wall_shift("wall_shift_1", 1);
    wall_shift("wall_shift_3", 3);
    // half a pixel: the mean of two neighbours
    {
        Wall w(0.5 * Wall::ps * Wall::D);
        double out, m2;
        int32_t n;
        rr::tp_pixel<1, true>(w.K, w.cur, w.prev, 4, 1, &out, &n, &m2);
        const double want = 0.5 * (w.hist[8 + 3] + w.hist[8 + 4]);
        report("wall_half_pixel", n == 2 && std::fabs(2.0 * out - want) <= 1e-12 * want);
        // the shorter history of the two taps counts
        w.count[8 + 3] = 7, w.count[8 + 4] = 2;
        rr::tp_pixel<1, true>(w.K, w.cur, w.prev, 4, 1, &out, &n, &m2);
        report("min_count", n == 3 && std::fabs(out - want * (1.0 - 1.0 / 3.0)) <= 1e-12 * want);
        // a tap on another object, with a turned normal, off the tangent plane, void or without history is skipped:
        // the other tap alone is the history
        const double other = w.hist[8 + 4];
        w.count[8 + 3] = 1, w.count[8 + 4] = 1;
        std::vector<int32_t> ids = w.object;
        ids[8 + 3] = 5;
        w.prev.object = ids.data();
        rr::tp_pixel<1, true>(w.K, w.cur, w.prev, 4, 1, &out, &n, &m2);
        report("object_tap", n == 2 && std::fabs(2.0 * out - other) <= 1e-12 * other);
        w.prev.object = w.object.data();
        std::vector<double> nrm = w.normal, z = w.depth;
        nrm[3 * (8 + 3) + 2] = 0.8;  // 1 - dot = 0.2 > 0.1
        w.prev.normal = nrm.data();
        rr::tp_pixel<1, true>(w.K, w.cur, w.prev, 4, 1, &out, &n, &m2);
        report("normal_tap", n == 2 && std::fabs(2.0 * out - other) <= 1e-12 * other);
        w.prev.normal = w.normal.data();
        z[8 + 3] = w.depth[8 + 3] * 1.02;  // 0.08 behind the wall; sigma_plane te = 0.04
        w.prev.depth = z.data();
        rr::tp_pixel<1, true>(w.K, w.cur, w.prev, 4, 1, &out, &n, &m2);
        report("plane_tap", n == 2 && std::fabs(2.0 * out - other) <= 1e-12 * other);
        z[8 + 3] = w.depth[8 + 3] * 1.005;  // 0.02 behind it: inside the tolerance
        rr::tp_pixel<1, true>(w.K, w.cur, w.prev, 4, 1, &out, &n, &m2);
        report("plane_pass", n == 2 && std::fabs(2.0 * out - want) <= 1e-12 * want);
        z[8 + 3] = INF;
        rr::tp_pixel<1, true>(w.K, w.cur, w.prev, 4, 1, &out, &n, &m2);
        report("void_tap", n == 2 && std::fabs(2.0 * out - other) <= 1e-12 * other);
        w.prev.depth = w.depth.data();
        w.count[8 + 3] = 0;
        rr::tp_pixel<1, true>(w.K, w.cur, w.prev, 4, 1, &out, &n, &m2);
        report("zero_count_tap", n == 2 && std::fabs(2.0 * out - other) <= 1e-12 * other);
        w.count[8 + 4] = 0;
        w.in[8 + 4] = 3.0;
        rr::tp_pixel<1, true>(w.K, w.cur, w.prev, 4, 1, &out, &n, &m2);
        report("no_history", n == 1 && same(out, 3.0) && same(m2, 9.0));
    }
    // a void pixel: out = in, n = 1, m2 = in^2, whatever the history
    {
        Wall w(0.0);
        w.in[5] = -2.5;
        w.depth[5] = INF;
        double out, m2;
        int32_t n;
        rr::tp_pixel<1, true>(w.K, w.cur, w.prev, 5, 0, &out, &n, &m2);
        bool ok = n == 1 && same(out, -2.5) && same(m2, 6.25);
        w.depth[5] = 4.0;
        std::vector<int32_t> ids = w.object;
        ids[5] = -1;
        w.cur.object = ids.data();
        rr::tp_pixel<1, true>(w.K, w.cur, w.prev, 5, 0, &out, &n, &m2);
        report("void_pixel", ok && n == 1 && same(out, -2.5) && same(m2, 6.25));
    }
    // a previous camera that looks the other way: every point lies behind it
    {
        Wall w(0.0, true);
        bool ok = true;
        for (int64_t x = 0; x < Wall::W; ++x) {
            double out, m2;
            int32_t n;
            w.in[(size_t)x] = 1.5;
            rr::tp_pixel<1, true>(w.K, w.cur, w.prev, x, 0, &out, &n, &m2);
            ok = ok && n == 1 && same(out, 1.5) && same(m2, 2.25);
        }
        report("behind_camera", ok);
    }
    // a static camera over N calls, three channels: n counts 1..N up to max_history and out follows the recurrence term
    // by term (h = (0 + 1 * prev) / (0 + 1) = prev exactly)
    for (int pass = 0; pass < 2; ++pass) {
        Wall w(0.0);
        w.K.is_static = 1;
        w.K.max_history = pass ? 3 : 1 << 20;
        w.K.alpha = pass ? 0.4 : 0.0;
        const size_t n_px = (size_t)(Wall::W * Wall::H);
        std::vector<double> img(3 * n_px), acc(3 * n_px, 0.0), acc2(3 * n_px, 0.0), out(3 * n_px), out2(3 * n_px), want(3 * n_px),
            want2(3 * n_px);
        std::vector<int32_t> cnt(n_px, 0), cnt_out(n_px);
        bool ok = true;
        for (int k = 1; k <= 6; ++k) {
            for (size_t i = 0; i < img.size(); ++i) img[i] = std::sin(0.37 * (double)i + 1.3 * k);
            w.cur.image = img.data();
            w.prev.image = acc.data();
            w.prev.m2 = acc2.data();
            w.prev.count = cnt.data();
            const int32_t n = k < w.K.max_history ? k : w.K.max_history;
            double a = 1.0 / (double)n;
            if (a < w.K.alpha) a = w.K.alpha;
            for (int64_t y = 0; y < Wall::H; ++y)
                for (int64_t x = 0; x < Wall::W; ++x) {
                    const size_t p = (size_t)(y * Wall::W + x);
                    rr::tp_pixel<3, true>(w.K, w.cur, w.prev, x, y, &out[3 * p], &cnt_out[p], &out2[3 * p]);
                    for (int c = 0; c < 3; ++c) {
                        const size_t i = 3 * p + (size_t)c;
                        want[i] = k == 1 ? img[i] : acc[i] + (img[i] - acc[i]) * a;
                        want2[i] = k == 1 ? img[i] * img[i] : acc2[i] + (img[i] * img[i] - acc2[i]) * a;
                        ok = ok && same(out[i], want[i]) && same(out2[i], want2[i]);
                    }
                    ok = ok && cnt_out[p] == n;
                }
            acc = out, acc2 = out2, cnt = cnt_out;
        }
        report(pass ? "static_cap" : "static_recurrence", ok);
    }
    std::printf("%d failures\n", failures);
    return failures;
}
