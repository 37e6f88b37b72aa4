// device_core.inc — device-side restatement of the reference's per-ray arithmetic, included by
// render.hip only.  Reference (src/raytracer/): object.rs:45-218, object/{sphere,plane,group,
// triangle,smooth_triangle}.rs, scene.rs:234-259, intersection.rs:50-95, computations.rs:39-54,
// light.rs:47-140, material.rs:77-80, material/pattern.rs:145-215.
//
// All arithmetic is f64 with -ffp-contract=off: rustc never fuses a*b+c, so neither do we, and
// every discrete decision (disc < 0, t >= 0, hit.t < distance, floor parity ...) matches the
// reference bit-for-bit.  Node loops are wave-uniform: all 64 lanes test the same flattened node,
// so node records arrive as scalar (SMEM) broadcast loads; lanes only differ in their masks.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "rr_device.hpp"
#include "quartic.inc"

namespace rr {

#define RR_EPS 0.00001  // main.rs:10

struct V3 {
    double x, y, z;
};
struct Ray {
    V3 o, d;
};

__device__ __forceinline__ V3 mk(double x, double y, double z) { return {x, y, z}; }
__device__ __forceinline__ V3 vadd(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 vsub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 vmul(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 vprod(V3 a, V3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
__device__ __forceinline__ V3 vneg(V3 a) { return {-a.x, -a.y, -a.z}; }
// (x*x' + y*y') + z*z' ; the reference's 4th (w) term is +-0 here and adding it is exact.
__device__ __forceinline__ double dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross3(V3 a, V3 b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// Several quotients with one positive divisor, each bit-identical to the IEEE division n / d (round
// to nearest): y = RN(1 / d) once, then Markstein's correction per numerator — q0 = RN(n y) is within
// an ulp of n / d, the residual n - d q0 is exact in one fma, and RN(q0 + (n - d q0) y) = RN(n / d).
// Written as q0 - RN(d q0 - n) y so that n = +-0 keeps its sign (d > 0).  Valid without overflow or
// underflow on the way: d in [2^-400, 2^400] and numerators 0 or >= 2^-500 in magnitude (vectors
// normalised here have |v| = d; scenes would need coordinates beyond 1e120 or differences below
// 1e-150 to leave the range).  3 ops per quotient instead of the ~11-instruction division sequence.
__device__ __forceinline__ double div_y(double n, double d, double y) {
    const double q0 = n * y;
    return __builtin_fma(-__builtin_fma(d, q0, -n), y, q0);
}
__device__ __forceinline__ V3 div3(V3 v, double d) {  // (v.x / d, v.y / d, v.z / d), d > 0
    const double y = 1.0 / d;
    return {div_y(v.x, d, y), div_y(v.y, d, y), div_y(v.z, d, y)};
}
__device__ __forceinline__ V3 normalize3(V3 a) {  // tuple.rs:95-98
    double m = sqrt(dot3(a, a));
    return div3(a, m);
}
__device__ __forceinline__ V3 reflect3(V3 v, V3 n) { return vsub(v, vmul(n, 2.0 * dot3(v, n))); }  // tuple.rs:115

// point (w = 1): row . (x, y, z, 1) = ((m0*x + m1*y) + m2*z) + m3   (matrix.rs:234-240)
template <class P>
__device__ __forceinline__ V3 xf_point(P m, V3 p) {
    return {m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3], m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7],
            m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11]};
}
// vector (w = +-0): the m3*w term is +-0 and dropped
template <class P>
__device__ __forceinline__ V3 xf_vec(P m, V3 v) {
    return {m[0] * v.x + m[1] * v.y + m[2] * v.z, m[4] * v.x + m[5] * v.y + m[6] * v.z,
            m[8] * v.x + m[9] * v.y + m[10] * v.z};
}
// inverse().transpose() * n (object.rs:131): column i of the inverse
template <class P>
__device__ __forceinline__ V3 xf_normal(P m, V3 n) {
    return {m[0] * n.x + m[4] * n.y + m[8] * n.z, m[1] * n.x + m[5] * n.y + m[9] * n.z,
            m[2] * n.x + m[6] * n.y + m[10] * n.z};
}
template <class P>
__device__ __forceinline__ Ray xf_ray(P m, const Ray& r) {
    return {xf_point(m, r.o), xf_vec(m, r.d)};
}
// NF_DIAG nodes: the off-diagonal terms of the sums above are +-0 products, which leave every
// non-zero sum unchanged (a zero result may differ in sign only; nothing downstream divides by a
// transformed component or tells the zeros apart: the tests compare, square and add them)
template <class P>
__device__ __forceinline__ Ray xf_ray_diag(P m, const Ray& r) {
    return {{m[0] * r.o.x + m[3], m[5] * r.o.y + m[7], m[10] * r.o.z + m[11]}, {m[0] * r.d.x, m[5] * r.d.y, m[10] * r.d.z}};
}
// a node's object-space ray (object.rs:45-48): identity, diagonal or full inverse (flags are wave-uniform)
template <class P>
__device__ __forceinline__ Ray xf_ray_node(int flags, P m, const Ray& r) {
    if (flags & NF_IDENT) return r;
    if (flags & NF_DIAG) return xf_ray_diag(m, r);
    return xf_ray(m, r);
}

// Wave-uniform records live in the constant address space: with a uniform index the loads become
// scalar (s_load) broadcasts instead of 64 identical vector loads.
#if defined(__HIP_DEVICE_COMPILE__)
#define RR_AS4 __attribute__((address_space(4)))
#else
#define RR_AS4
#endif
template <class T>
using cptr = const RR_AS4 T*;
template <class T>
__device__ __forceinline__ cptr<T> cp(const T* p) {
    return (cptr<T>)p;
}
template <class T>
__device__ __forceinline__ T ldc(const T* p, int i) {
    return cp(p)[i];
}
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
// this lane's index in the wave, recomputed at every use (a volatile asm is neither hoisted nor merged): a
// value derived from threadIdx.x would be held in a VGPR across a whole loop (chain_kernel)
__device__ __forceinline__ int lane_id() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
// Counter-based replacement of thread_rng (light.rs:57-59), identical to the oracle's orc_jitter:
// one 64-bit mix per shading event (global sample id, recursion path), then one 32-bit mix per
// value (light, cell sample, u/v) — the per-sample part has 2 integer multiplies instead of the 21
// quarter-rate 32-bit multiplies of three chained 64-bit mixes.
__device__ __forceinline__ uint32_t jitter_base(uint64_t seed, uint64_t sample, uint32_t path) {
    return (uint32_t)(splitmix64(seed ^ splitmix64(sample ^ ((uint64_t)path << 40))) >> 32);
}
__device__ __forceinline__ double jitter_value(uint32_t base, uint32_t light, uint32_t s, uint32_t which) {
    return (double)lowbias32(base ^ ((light << 21) | (s << 1) | which)) * (1.0 / 4294967296.0);
}

// Wave-uniform counters (ballot popcounts), flushed by lane 0 with no cross-lane reduction.
struct Counters {
    // 32-bit where one wave's counts over one tile of events (flushed per tile) stay far below 2^32
    // (the kernels keep these in SGPRs for their whole run); the flop count can exceed it
    uint32_t rays, shadow, shade, n1n2, gtests, ghits, tests;
    uint64_t flops;   // exact-test f64 flops (lane-level)
    uint32_t visits;  // wave-level candidate visits
    uint32_t nan;     // lanes whose walk met a NaN t in a list of >= 2 entries (sort_by(partial_cmp).unwrap())
};
__device__ __forceinline__ uint32_t popc_ballot(bool b) { return (uint32_t)__popcll(__ballot(b)); }
// The counters are wave-uniform; a count added under divergent control flow can leave the compiler holding it
// in a VGPR.  Loops that carry Counters across iterations (chain_kernel) pass them through readfirstlane at the
// back edge, so they stay scalar there.
__device__ __forceinline__ uint32_t uniform_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ void uniform_counters(Counters& c) {
    c.rays = uniform_u32(c.rays);
    c.shadow = uniform_u32(c.shadow);
    c.shade = uniform_u32(c.shade);
    c.n1n2 = uniform_u32(c.n1n2);
    c.gtests = uniform_u32(c.gtests);
    c.ghits = uniform_u32(c.ghits);
    c.tests = uniform_u32(c.tests);
    c.flops = ((uint64_t)uniform_u32((uint32_t)(c.flops >> 32)) << 32) | uniform_u32((uint32_t)c.flops);
    c.visits = uniform_u32(c.visits);
    c.nan = uniform_u32(c.nan);
}
// SURVEY.md §8(d) flop model per exact test (ray transform + local intersect; FMA = 2)
__device__ __forceinline__ uint64_t test_flops(int kind) {  // torus: coefficients + classification
    return kind == RR_SPHERE ? 57u : kind == RR_PLANE ? 13u : kind == RR_TORUS ? 320u : 45u;
}

// Ray expressed in the space of node `parent` (group chain root-first, object.rs:45-48 per level).
// `parent` is wave-uniform (it comes from a node record).
__device__ __forceinline__ Ray ray_in_space(const DevScene& S, const Ray& rw, int parent) {
    if (parent < 0) return rw;
    cptr<DevGroup> g = cp(S.groups) + cp(S.nodes)[parent].aux;
    Ray r = rw;
    const int depth = g->depth;
    for (int k = 0; k < depth; ++k) r = xf_ray(cp(S.nodes)[g->anc[k]].inv, r);
    return r;
}

// AABB::intersect (object.rs:178-218)
__device__ __forceinline__ void check_axis(double origin, double direction, double mn, double mx, double& tmin,
                                           double& tmax) {
    double a = mn - origin, b = mx - origin;
    if (fabs(direction) >= RR_EPS) {
        tmin = a / direction;
        tmax = b / direction;
    } else {
        tmin = a * __builtin_inf();
        tmax = b * __builtin_inf();
    }
    if (tmin > tmax) {
        double t = tmin;
        tmin = tmax;
        tmax = t;
    }
}
template <class P>
__device__ __forceinline__ bool aabb_hit(P bx, const Ray& r) {
    double x0, x1, y0, y1, z0, z1;
    check_axis(r.o.x, r.d.x, bx[0], bx[3], x0, x1);
    check_axis(r.o.y, r.d.y, bx[1], bx[4], y0, y1);
    check_axis(r.o.z, r.d.z, bx[2], bx[5], z0, z1);
    double tmin = fmax(x0, fmax(y0, z0));
    double tmax = fmin(x1, fmin(y1, z1));
    return tmin <= tmax;
}

// Leaf local_intersect: up to two entries (t, u, v) in local order.
// Leaf local_intersect: up to four entries in the leaf's own list order (cylinder / cone: two side
// entries then the caps), each with its index k in that list (tie-break key and n1/n2 equality).
// M = 2 for scenes of spheres, planes and triangles; M = 4 (the kernels' G = 2 variant) when
// cubes, cylinders, cones or CSGs are present — the common path keeps its registers.
template <int M>
struct EntriesT {
    int n;
    double t[M];
    int k[M];
    double u, v;  // triangles (one entry)
};
// append with constant indices only (a lane-varying index would put the arrays in scratch)
template <int M>
__device__ __forceinline__ void push_entry(EntriesT<M>& e, double t) {
#pragma unroll
    for (int q = 0; q < M; ++q)
        if (e.n == q) e.t[q] = t;
    e.n++;
}
// FWD (closest-hit and shadow walks, which use only entries with t >= 0): a sphere's t2 is computed only
// where t1 < 0.  With a = d.d > 0 and s = sqrt(disc) >= 0, -b - s <= -b + s, and rounding and the division
// by 2a > 0 are monotonic, so t1 <= t2: when t1 >= 0 the sphere's first usable entry is t1 (a tie goes to
// the smaller local index, t1's), and t1 < distance decides a shadow whatever t2 is.  Elsewhere t2 = t1 (a
// duplicate of an entry already there: neither query's answer changes).  A NaN t1 (a = 0) leaves both
// entries unusable, as the reference's two NaN entries are.
// Möller-Trumbore (triangle.rs:72-94 / smooth_triangle.rs:75-97) on p1, e1, e2 at P[0..8]; e arrives empty
template <int M>
__device__ __forceinline__ void tri_intersect(const RR_AS4 double* P, const Ray& lr, EntriesT<M>& e) {
    V3 e1 = mk(P[3], P[4], P[5]), e2 = mk(P[6], P[7], P[8]);
    V3 dce2 = cross3(lr.d, e2);
    double det = dot3(e1, dce2);
    if (!(fabs(det) < RR_EPS)) {
        double f = 1.0 / det;
        V3 p1o = vsub(lr.o, mk(P[0], P[1], P[2]));
        double u = f * dot3(p1o, dce2);
        if (!(u < 0.0 || u > 1.0)) {
            V3 oce1 = cross3(p1o, e1);
            double v = f * dot3(lr.d, oce1);
            if (!(v < 0.0 || (u + v) > 1.0)) {
                e.n = 1;
                e.t[0] = f * dot3(e2, oce1);
                e.u = u;
                e.v = v;
            }
        }
    }
}
// plane.rs:51-58; e arrives empty
template <int M>
__device__ __forceinline__ void plane_intersect(const Ray& lr, EntriesT<M>& e) {
    if (!(fabs(lr.d.y) < RR_EPS)) {
        e.n = 1;
        e.t[0] = -lr.o.y / lr.d.y;
    }
}
// sphere.rs:64-78 (sphere_to_ray = origin - point(0,0,0) = origin); e arrives empty
template <int M, bool FWD>
__device__ __forceinline__ void sphere_intersect(const Ray& lr, EntriesT<M>& e) {
    double a = dot3(lr.d, lr.d);
    double b = 2.0 * dot3(lr.d, lr.o);
    double c = dot3(lr.o, lr.o) - 1.0;
    double disc = b * b - 4.0 * a * c;
    if (!(disc < 0.0)) {  // a NaN discriminant gives two NaN entries, as in the reference
        double s = sqrt(disc);
        e.n = 2;
        e.t[0] = (-b - s) / (2.0 * a);
        e.t[1] = e.t[0];
        if (!FWD || e.t[0] < 0.0) e.t[1] = (-b + s) / (2.0 * a);
    }
}
template <int M>
__device__ __forceinline__ EntriesT<M> empty_entries() {
    EntriesT<M> e;
    e.n = 0;
    e.u = 0.0;
    e.v = 0.0;
    for (int q = 0; q < M; ++q) {
        e.t[q] = 0.0;
        e.k[q] = q;
    }
    return e;
}
template <int M, bool FWD = false>
__device__ __forceinline__ EntriesT<M> leaf_intersect(const DevScene& S, cptr<DevNode> nd, int kind, int aux,
                                                      const Ray& lr) {
    EntriesT<M> e;
    e.n = 0;
    e.u = 0.0;
    e.v = 0.0;
    for (int q = 0; q < M; ++q) {
        e.t[q] = 0.0;
        e.k[q] = q;
    }
    if (kind == RR_SPHERE) {
        sphere_intersect<M, FWD>(lr, e);
    } else if (kind == RR_PLANE) {
        plane_intersect(lr, e);
    } else if (kind == RR_TRIANGLE || kind == RR_SMOOTH_TRIANGLE) {  // triangle.rs:72-94 / smooth_triangle.rs:75-97
        // p1, e1, e2 (9 doubles): inline in the node record (NF_TRI_INLINE, no dependent load) or DevTri
        tri_intersect((S.tri_inline || (nd->flags & NF_TRI_INLINE)) ? nd->inv : (cp(S.tris) + aux)->p1, lr, e);
    } else if (M == 4 && kind == RR_TORUS) {  // torus.rs:37-95 (roots 0.0.8 find_roots_quartic)
        const double r = (cp(S.shapes) + aux)->minimum;
        const V3 o = lr.o, d = lr.d;
        const double r_sq = r * r;
        const double sum_d_sq = d.x * d.x + d.y * d.y + d.z * d.z;
        const double ee = o.x * o.x + o.y * o.y + o.z * o.z - r_sq + 1.0;
        const double f = dot3(o, d) + 0.0;  // Tuple::dot: + w*w (1 * 0)
        const double four = 4.0;
        const double a4 = sum_d_sq * sum_d_sq;
        const double a3 = 4.0 * sum_d_sq * f;
        const double a2 = 2.0 * sum_d_sq * ee + 4.0 * f * f - four * (d.x * d.x + d.y * d.y);
        const double a1 = 4.0 * ee * f - 2.0 * four * (o.x * d.x + o.y * d.y);
        const double a0 = ee * ee - four * (o.x * o.x + o.y * o.y);
        const RqRoots rs = rq_quartic(a4, a3, a2, a1, a0);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < rs.n && rs.v[q] > 0.0) push_entry(e, rs.v[q]);
    } else if (M == 4 && kind == RR_CUBE) {  // cube.rs:64-78 with check_axis cube.rs:49-61
        double x0, x1, y0, y1, z0, z1;
        check_axis(lr.o.x, lr.d.x, -1.0, 1.0, x0, x1);
        check_axis(lr.o.y, lr.d.y, -1.0, 1.0, y0, y1);
        check_axis(lr.o.z, lr.d.z, -1.0, 1.0, z0, z1);
        const double tmin = fmax(fmax(x0, y0), z0), tmax = fmin(fmin(x1, y1), z1);
        if (!(tmin > tmax)) {
            e.n = 2;
            e.t[0] = tmin;
            e.t[1] = tmax;
        }
    } else if (M == 4 && kind == RR_CYLINDER) {  // cylinder.rs:85-111, caps :48-73, check_cap :40-46
        cptr<DevShape> P = cp(S.shapes) + aux;
        const double mn = P->minimum, mx = P->maximum;
        const V3 d = lr.d, o = lr.o;
        double a = d.x * d.x + d.z * d.z;
        bool miss = false;
        if (fabs(a) > RR_EPS) {
            double b = 2.0 * o.x * d.x + 2.0 * o.z * d.z;
            double c = o.x * o.x + o.z * o.z - 1.0;
            double disc = b * b - 4.0 * a * c;
            if (disc < 0.0) {
                miss = true;  // returns vec![] before the caps
            } else {
                double t0 = (-b - sqrt(disc)) / (2.0 * a);
                double t1 = (-b + sqrt(disc)) / (2.0 * a);
                if (t0 > t1) {
                    double tt = t0;
                    t0 = t1;
                    t1 = tt;
                }
                double ya = o.y + t0 * d.y;
                if (mn < ya && ya < mx) push_entry(e, t0);
                double yb = o.y + t1 * d.y;
                if (mn < yb && yb < mx) push_entry(e, t1);
            }
        }
        if (!miss && P->closed && !(fabs(d.y) < RR_EPS)) {
            double t = (mn - o.y) / d.y;
            double x = o.x + t * d.x, z = o.z + t * d.z;
            if ((x * x + z * z) <= 1.0) push_entry(e, t);
            t = (mx - o.y) / d.y;
            x = o.x + t * d.x;
            z = o.z + t * d.z;
            if ((x * x + z * z) <= 1.0) push_entry(e, t);
        }
    } else if (M == 4 && kind == RR_CONE) {  // cone.rs:75-135, caps :46-73, check_cap :36-44
        cptr<DevShape> P = cp(S.shapes) + aux;
        const double mn = P->minimum, mx = P->maximum;
        const V3 d = lr.d, o = lr.o;
        double a = d.x * d.x - d.y * d.y + d.z * d.z;
        double b = 2.0 * o.x * d.x - 2.0 * o.y * d.y + 2.0 * o.z * d.z;
        bool sides = true, caps = true;
        if (fabs(a) < RR_EPS && fabs(b) < RR_EPS) {
            sides = false;  // caps only
        } else {
            double c = o.x * o.x - o.y * o.y + o.z * o.z;
            if (fabs(a) < RR_EPS) {
                double t = -c / (2.0 * b);
                double y = o.y + t * d.y;
                if (mn < y && y < mx) {
                    push_entry(e, t);
                    sides = false;
                    caps = false;  // cone.rs:101-103 returns without the caps
                }
            }
            if (sides) {
                double disc = b * b - 4.0 * a * c;
                if (disc < 0.0) {
                    caps = false;  // returns vec![]
                } else {
                    double t0 = (-b - sqrt(disc)) / (2.0 * a);
                    double t1 = (-b + sqrt(disc)) / (2.0 * a);
                    if (t0 > t1) {
                        double tt = t0;
                        t0 = t1;
                        t1 = tt;
                    }
                    double ya = o.y + t0 * d.y;
                    if (mn < ya && ya < mx) push_entry(e, t0);
                    double yb = o.y + t1 * d.y;
                    if (mn < yb && yb < mx) push_entry(e, t1);
                }
            }
        }
        if (caps && P->closed && !(fabs(d.y) < RR_EPS)) {
            double t = (mn - o.y) / d.y;
            double x = o.x + t * d.x, y = o.y + t * d.y, z = o.z + t * d.z;
            if ((x * x + z * z) <= y * y) push_entry(e, t);
            t = (mx - o.y) / d.y;
            x = o.x + t * d.x;
            y = o.y + t * d.y;
            z = o.z + t * d.z;
            if ((x * x + z * z) <= y * y) push_entry(e, t);
        }
    }
    return e;
}

struct Hit {
    double t, u, v;
    int node, k;  // node index, local entry index (0/1)
    int rank;     // the node's reference DFS position (tie-break)
    int mat;      // the node's material (trace_closest; read with the node's record in the walk, so the shading
                  // code's material load does not wait for a per-lane node load first)
    bool found;
};

// ---------------------------------------------------------------- exact-preserving culling
// A wave's 64 rays are bounded by a "fat cone": every origin lies within rho of o, every direction
// within angle T of the axis a.  Lane j then tests node base+j's world-space bounding sphere
// against that bundle (the test is transposed: 64 nodes per pass), a ballot yields the candidate
// nodes, and only those get the per-lane f32 line test and the exact f64 test, still in flattened
// order.  Every cull is conservative (a node the f64 test could report as hit always passes), so
// the result is bit-identical to the full scan (DESIGN.md §3.5).
struct Bundle {
    float o[3], a[3];
    float rho, tanT, secT;
    int ok;   // 0: rays too spread (or non-finite) -> every node is a candidate
    int two;  // some lane's origin was moved forward along its ray: its segment starts behind the cone's
              // apex ball, so the node tests use both nappes
};
struct LaneRay {  // this lane's ray in f32 for the per-lane line test
    float o[3], d[3];
    float dd;   // |d|^2
    float dl;   // |d| (approximate: every use carries relative margins far above its error)
    float eo;   // radius slack for the f32 rounding of the origin
};

// Wave reductions on the DPP crossbar (no LDS traffic): quad swaps, half-row / row mirrors, then
// row_bcast15 / row_bcast31 fold the four 16-lane rows into lane 63, which is broadcast (wave_max_u).
__device__ __forceinline__ uint32_t wave_max_u(uint32_t v);
// Float wave minimum / maximum through an order-preserving map to unsigned integers (negative floats:
// all bits but the sign flipped; then the sign bit flipped), so every DPP step is one integer max with no
// NaN canonicalisation.  Inputs must not be NaN (callers pass finite values or +-inf).
__device__ __forceinline__ uint32_t f2ord(float v) {
    const uint32_t b = __float_as_uint(v);
    return ((int32_t)b < 0 ? b ^ 0x7fffffffu : b) ^ 0x80000000u;
}
__device__ __forceinline__ float ord2f(uint32_t u) {
    const uint32_t b = u ^ 0x80000000u;
    return __uint_as_float((int32_t)b < 0 ? b ^ 0x7fffffffu : b);
}
__device__ __forceinline__ float wave_min_f(float v) { return ord2f(~wave_max_u(~f2ord(v))); }
__device__ __forceinline__ float wave_max_f(float v) { return ord2f(wave_max_u(f2ord(v))); }
// Non-negative floats order like their bit patterns as unsigned integers, so their wave maximum is an
// integer reduction: one v_max_u32_dpp per step, no NaN-quieting canonicalisation (float min / max DPP
// steps cost 4 VALU each).  Lanes of rows a row_bcast step does not write keep their value (max identity).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_u(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ uint32_t wave_max_u(uint32_t v) {
    v = max(v, dpp_u<0xB1, 0xf>(v));
    v = max(v, dpp_u<0x4E, 0xf>(v));
    v = max(v, dpp_u<0x141, 0xf>(v));
    v = max(v, dpp_u<0x140, 0xf>(v));
    v = max(v, dpp_u<0x142, 0xa>(v));
    v = max(v, dpp_u<0x143, 0xc>(v));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// maximum over the wave of values >= +0 (squares, slacks; not NaN)
__device__ __forceinline__ float wave_max_nonneg(float v) { return __uint_as_float(wave_max_u(__float_as_uint(v))); }
// minimum over the wave of max(v, +0): negative values (and -0) count as +0; used where only a minimum
// above a positive threshold matters (the bundle's smallest cosine must exceed 0.2)
__device__ __forceinline__ float wave_min_clamp0(float v) {
    uint32_t b = __float_as_uint(v);
    b = (int32_t)b < 0 ? 0u : b;
    return __uint_as_float(~wave_max_u(~b));
}
__device__ __forceinline__ float uniform_f(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

__device__ __forceinline__ float lane_f(float v, int k);

// The fat cone around the live lanes' rays: centre = the midpoint of the first and last live
// lanes' origins, axis = the normalised sum of their unit directions (the opposite corners of a
// sample tile), then three reductions for the exact radius and half-angle around them.  Any centre
// and axis give a valid cone; these cost two readlanes instead of nine more reductions.
// want == false (scenes of a few nodes, where the reductions cost more than the node tests they
// could save): only the lane rays, and no bundle (every node is a candidate).
// Far origins (the floor at the horizon: t ~ 1e6 and beyond) would make the f32 origin's rounding
// slack eo, and the bundle's origin ball, as large as the scene, so every node would be a candidate
// for every lane (C4's horizon tiles: 1 % of the waves held 48 % of the kernel's cycles).  A lane
// whose origin lies more than 16 (R + 1) from the centre of the scene's bounded content is culled from
// o' = o + s d instead, s = (C - o).d / |d|^2 (the same line, next to the scene; returned in s): the
// line tests are unchanged, the forward test's far bound becomes tmax - s (walk_nodes, with a 1e-6
// relative slack for the rounding of both), its near bound is dropped when s > 0 (the segment starts
// behind o'), and the bundle tests both nappes when some s > 0.
// SHIFT: only the shadow walks of scenes with groups (their origins are hit points, which reach the
// horizon; camera rays start at the camera) — the trace walks and flat scenes keep their registers.
// cam_tile (level-0 camera rays of a full 8x8 tile, affine camera; wave-uniform): every lane's origin is
// the camera's (the same f64 value, so the same f32 value) and the directions are normalize(P - O) for
// points P on a regular grid in one plane (camera.rs:75-93, affine in the pixel offsets).  Then rho = 0
// exactly, and the largest angle between the axis and a ray is attained at a corner of the tile: the rays
// within angle theta of the axis meet the plane in a convex set (a section of one nappe of a solid cone),
// so the angle is quasi-convex over the tile and peaks at a vertex of its convex hull — lanes 0, 7, 56, 63.
// Four readlanes replace the three wave reductions (the f32 rounding of the directions, ~1e-7, sits far
// inside the 2e-4 margin on tan theta).
// cam_tile's bundle from a tile's camera origin (f32) and the f32 directions of its corner rays (lanes 0, 7,
// 56, 63): the same operations as make_bundle's cam_tile path (tile_bundle_kernel builds the table with it).
__device__ __forceinline__ Bundle cam_corner_bundle(const float o[3], const float dc[4][3]) {
    Bundle B;
    B.ok = 0;
    B.two = 0;
    for (int k = 0; k < 3; ++k) B.o[k] = B.a[k] = 0.0f;
    B.rho = B.tanT = B.secT = 0.0f;
    float u[4][3];
    for (int j = 0; j < 4; ++j) {
        const float dd = dc[j][0] * dc[j][0] + dc[j][1] * dc[j][1] + dc[j][2] * dc[j][2];
        const bool fin = isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]) && isfinite(dd) && dd > 1e-30f && dd < 1e30f &&
                         4e-7f * (fabsf(o[0]) + fabsf(o[1]) + fabsf(o[2])) < 1e30f;
        if (!fin) return B;
        const float il = __builtin_amdgcn_rsqf(dd);
        for (int k = 0; k < 3; ++k) u[j][k] = dc[j][k] * il;
    }
    float c[3], sv[3];
    for (int k = 0; k < 3; ++k) {
        c[k] = 0.5f * o[k] + 0.5f * o[k];
        sv[k] = u[0][k] + u[3][k];
    }
    const float sl2 = sv[0] * sv[0] + sv[1] * sv[1] + sv[2] * sv[2];
    if (!(sl2 > 1e-6f)) return B;
    const float isl = __builtin_amdgcn_rsqf(sl2);
    const float a[3] = {sv[0] * isl, sv[1] * isl, sv[2] * isl};
    float cosv[4], sn[4];
    for (int j = 0; j < 4; ++j) {
        cosv[j] = a[0] * u[j][0] + a[1] * u[j][1] + a[2] * u[j][2];
        const float x0 = a[1] * u[j][2] - a[2] * u[j][1], x1 = a[2] * u[j][0] - a[0] * u[j][2],
                    x2 = a[0] * u[j][1] - a[1] * u[j][0];
        sn[j] = x0 * x0 + x1 * x1 + x2 * x2;
    }
    const float cosm = fminf(fminf(cosv[0], cosv[1]), fminf(cosv[2], cosv[3]));
    const float sin2m = fmaxf(fmaxf(sn[0], sn[1]), fmaxf(sn[2], sn[3]));
    if (!(cosm > 0.2f)) return B;
    const float rho = 0.0f;
    B.rho = rho * 1.0001f + 2e-6f * (fabsf(c[0]) + fabsf(c[1]) + fabsf(c[2]) + rho) + 1e-30f;
    B.tanT = (__builtin_amdgcn_sqrtf(sin2m) * __builtin_amdgcn_rcpf(cosm)) * 1.001f + 2e-4f;
    B.secT = __builtin_amdgcn_sqrtf(1.0f + B.tanT * B.tanT) * 1.0001f;
    for (int k = 0; k < 3; ++k) {
        B.o[k] = c[k];
        B.a[k] = a[k];
    }
    B.ok = 1;
    return B;
}

// cam_bundle: cam_tile's bundle from the per-frame tile table (tile_bundle_kernel computes exactly the values
// the cam_tile path below would), read with scalar loads; the lane rays are still built here.
__device__ __forceinline__ Bundle load_tile_bundle(const float* p) {
    const RR_AS4 float* q = (const RR_AS4 float*)p;
    Bundle B;
    for (int k = 0; k < 3; ++k) {
        B.o[k] = q[k];
        B.a[k] = q[3 + k];
    }
    B.rho = q[6];
    B.tanT = q[7];
    B.secT = q[8];
    B.ok = __float_as_int(q[9]);
    B.two = 0;
    return B;
}
template <bool SHIFT>
__device__ __forceinline__ Bundle make_bundle(const DevScene& S, const Ray& rw, bool live, LaneRay& L, bool want,
                                              float& s_out, bool cam_tile = false, const float* cam_bundle = nullptr) {
    float o[3] = {(float)rw.o.x, (float)rw.o.y, (float)rw.o.z};
    float d[3] = {(float)rw.d.x, (float)rw.d.y, (float)rw.d.z};
    float dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    s_out = 0.0f;
    float eo_shift = 0.0f;
    bool shifted = false;
    if (SHIFT && S.bs_r >= 0.0f) {
        const float cx = S.bs_c[0] - o[0], cy = S.bs_c[1] - o[1], cz = S.bs_c[2] - o[2];
        const float lim = 16.0f * (S.bs_r + 1.0f);
        const bool far = live && cx * cx + cy * cy + cz * cz > lim * lim && dd > 1e-30f && dd < 1e30f;
        if (__ballot(far) != 0) {  // wave-uniform: coherent near waves skip this
            const float sf = far ? (cx * d[0] + cy * d[1] + cz * d[2]) / dd : 0.0f;
            const double s = (double)sf;
            const double ox = rw.o.x + s * rw.d.x, oy = rw.o.y + s * rw.d.y, oz = rw.o.z + s * rw.d.z;
            if (far) {
                // o' carries the f64 rounding of s d (<= 2^-52 |s| |d|_1 per component) into eo
                eo_shift = 1e-15f * (fabsf(o[0]) + fabsf(o[1]) + fabsf(o[2]) + fabsf(sf) * (fabsf(d[0]) + fabsf(d[1]) + fabsf(d[2])));
                o[0] = (float)ox;
                o[1] = (float)oy;
                o[2] = (float)oz;
                s_out = sf;
                shifted = sf > 0.0f;
            }
        }
    }
    for (int k = 0; k < 3; ++k) {
        L.o[k] = o[k];
        L.d[k] = d[k];
    }
    L.dd = dd;
    L.dl = __builtin_amdgcn_sqrtf(dd);
    L.eo = 4e-7f * (fabsf(o[0]) + fabsf(o[1]) + fabsf(o[2])) + eo_shift;
    if (cam_bundle && want) return load_tile_bundle(cam_bundle);
    Bundle B;
    B.ok = 0;
    B.two = __ballot(shifted) != 0 ? 1 : 0;
    for (int k = 0; k < 3; ++k) B.o[k] = B.a[k] = 0.0f;
    B.rho = B.tanT = B.secT = 0.0f;
    if (!want) return B;
    const bool fin = isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]) && isfinite(dd) && dd > 1e-30f &&
                     dd < 1e30f && L.eo < 1e30f;
    const uint64_t lm = __ballot(live);
    if (lm == 0 || __ballot(live && !fin) != 0) return B;
    const int f0 = __ffsll((long long)lm) - 1, f1 = 63 - __clzll((long long)lm);
    // the bundle only needs bounds (every margin below is >= 1e-4 relative), so the hardware's
    // approximate v_rsq / v_sqrt / v_rcp (~1 ulp) replace the correctly rounded f32 sequences
    const float il = __builtin_amdgcn_rsqf(dd);
    float u[3] = {d[0] * il, d[1] * il, d[2] * il};
    float c[3], s[3];
    for (int k = 0; k < 3; ++k) {
        c[k] = 0.5f * __int_as_float(__builtin_amdgcn_readlane(__float_as_int(o[k]), f0)) +
               0.5f * __int_as_float(__builtin_amdgcn_readlane(__float_as_int(o[k]), f1));
        s[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(u[k]), f0)) +
               __int_as_float(__builtin_amdgcn_readlane(__float_as_int(u[k]), f1));
    }
    const float sl2 = s[0] * s[0] + s[1] * s[1] + s[2] * s[2];
    if (!(sl2 > 1e-6f)) return B;
    const float isl = __builtin_amdgcn_rsqf(sl2);
    float a[3] = {s[0] * isl, s[1] * isl, s[2] * isl};
    const float ex = o[0] - c[0], ey = o[1] - c[1], ez = o[2] - c[2];
    const float cosv = a[0] * u[0] + a[1] * u[1] + a[2] * u[2];
    const float x0 = a[1] * u[2] - a[2] * u[1], x1 = a[2] * u[0] - a[0] * u[2], x2 = a[0] * u[1] - a[1] * u[0];
    float rho2, cosm, sin2m;
    if (cam_tile && lm == ~0ull) {
        const float sn = x0 * x0 + x1 * x1 + x2 * x2;
        rho2 = 0.0f;
        cosm = fminf(fminf(lane_f(cosv, 0), lane_f(cosv, 7)), fminf(lane_f(cosv, 56), lane_f(cosv, 63)));
        sin2m = fmaxf(fmaxf(lane_f(sn, 0), lane_f(sn, 7)), fmaxf(lane_f(sn, 56), lane_f(sn, 63)));
    } else {
        rho2 = uniform_f(wave_max_nonneg(live ? ex * ex + ey * ey + ez * ez : 0.0f));
        cosm = uniform_f(wave_min_clamp0(live ? cosv : 1.0f));
        sin2m = uniform_f(wave_max_nonneg(live ? x0 * x0 + x1 * x1 + x2 * x2 : 0.0f));
    }
    if (!(cosm > 0.2f)) return B;  // half-angle above ~78 degrees: not worth a bundle
    const float rho = __builtin_amdgcn_sqrtf(rho2);
    B.rho = rho * 1.0001f + 2e-6f * (fabsf(c[0]) + fabsf(c[1]) + fabsf(c[2]) + rho) + 1e-30f;
    B.tanT = (__builtin_amdgcn_sqrtf(sin2m) * __builtin_amdgcn_rcpf(cosm)) * 1.001f + 2e-4f;
    B.secT = __builtin_amdgcn_sqrtf(1.0f + B.tanT * B.tanT) * 1.0001f;
    for (int k = 0; k < 3; ++k) {
        B.o[k] = c[k];
        B.a[k] = a[k];
    }
    B.ok = 1;
    return B;
}

// Shadow rays toward one point light (wave-uniform position L): every ray's segment from its origin
// to L lies in the cone with apex L spanned by the origins, so the bundle is that cone — apex exact
// (rho covers only f32 rounding) instead of a ball around the spread origins, which widened the
// camera-tile shadow bundles by the whole tile's extent.  Two reductions instead of three.  The lane
// rays are the same as make_bundle's.  Forward nappe from L toward the origins (the segments end at L).
// SEG (the group scenes' shadow walks): the lane rays are the segments' lines through L (the SEG lane
// test of lane_may_hit), so a horizon origin's f32 rounding (up to 4e-7 |o|_1) does not widen its line
// tests; the cone is spanned by the origins, and their f32 rounding becomes an angular slack at L instead
// of a ball: seen from L, every point of a segment lies in the direction of its origin.
template <bool SEG>
__device__ __forceinline__ Bundle make_bundle_apex(const DevScene& S, const Ray& rw, bool live, LaneRay& L,
                                                   const float* apex) {
    Bundle B;
    if constexpr (SEG) {
        B.ok = 0;
        B.two = 0;
        for (int k = 0; k < 3; ++k) B.o[k] = B.a[k] = 0.0f;
        B.rho = B.tanT = B.secT = 0.0f;
        const float d[3] = {(float)rw.d.x, (float)rw.d.y, (float)rw.d.z};
        for (int k = 0; k < 3; ++k) {
            L.o[k] = apex[k];
            L.d[k] = d[k];
        }
        L.dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        L.dl = __builtin_amdgcn_sqrtf(L.dd);
        // the f32 rounding of L, and the f64 segment's end o + distance d against L (a few ulps of |L - o|)
        L.eo = 4e-7f * (fabsf(apex[0]) + fabsf(apex[1]) + fabsf(apex[2])) +
               1e-14f * (fabsf((float)rw.o.x) + fabsf((float)rw.o.y) + fabsf((float)rw.o.z));
    } else {
        float s_out;
        B = make_bundle<false>(S, rw, live, L, false, s_out);  // lane rays only, B.ok = 0
    }
    const float o[3] = {(float)rw.o.x, (float)rw.o.y, (float)rw.o.z};
    const float v[3] = {o[0] - apex[0], o[1] - apex[1], o[2] - apex[2]};
    const float vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    const float scale = fabsf(apex[0]) + fabsf(apex[1]) + fabsf(apex[2]);
    const bool fin = isfinite(vv) && vv > 1e-12f * (1.0f + scale * scale) && vv < 1e30f && L.eo < 1e30f &&
                     isfinite(scale) && isfinite(o[0] + o[1] + o[2]) && (!SEG || (L.dd > 1e-30f && L.dd < 1e30f));
    const uint64_t lm = __ballot(live);
    if (lm == 0 || __ballot(live && !fin) != 0) return B;
    const int f0 = __ffsll((long long)lm) - 1, f1 = 63 - __clzll((long long)lm);
    const float il = __builtin_amdgcn_rsqf(vv);
    const float u[3] = {v[0] * il, v[1] * il, v[2] * il};
    float sdir[3];
    for (int k = 0; k < 3; ++k)
        sdir[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(u[k]), f0)) +
                  __int_as_float(__builtin_amdgcn_readlane(__float_as_int(u[k]), f1));
    const float sl2 = sdir[0] * sdir[0] + sdir[1] * sdir[1] + sdir[2] * sdir[2];
    if (!(sl2 > 1e-6f)) return B;
    const float isl = __builtin_amdgcn_rsqf(sl2);
    const float a[3] = {sdir[0] * isl, sdir[1] * isl, sdir[2] * isl};
    const float cosv = a[0] * u[0] + a[1] * u[1] + a[2] * u[2];
    const float x0 = a[1] * u[2] - a[2] * u[1], x1 = a[2] * u[0] - a[0] * u[2], x2 = a[0] * u[1] - a[1] * u[0];
    const float cosm = uniform_f(wave_min_clamp0(live ? cosv : 1.0f));
    const float sin2m = uniform_f(wave_max_nonneg(live ? x0 * x0 + x1 * x1 + x2 * x2 : 0.0f));
    if (!(cosm > 0.2f)) return B;
    float tanT = __builtin_amdgcn_sqrtf(sin2m) * __builtin_amdgcn_rcpf(cosm);
    if constexpr (SEG) {
        // origin rounding as an angle at L: tan(theta + e) = (t + tan e) / (1 - t tan e), tan e <= 1.01 e
        const float eo0 = 4e-7f * (fabsf(o[0]) + fabsf(o[1]) + fabsf(o[2]));
        const float e = 1.01f * uniform_f(wave_max_nonneg(live ? eo0 * il * 1.01f : 0.0f));
        if (!(tanT * e < 0.5f)) return B;
        tanT = (tanT + e) / (1.0f - tanT * e);
        B.rho = 2e-6f * scale + 1e-30f;
    } else {
        // rho: the f32 rounding of L and of the origins (eo), as make_bundle's origin-ball slack
        const float eom = uniform_f(wave_max_nonneg(live ? L.eo : 0.0f));
        B.rho = eom + 2e-6f * scale + 1e-30f;
    }
    B.tanT = tanT * 1.001f + 2e-4f;
    B.secT = __builtin_amdgcn_sqrtf(1.0f + B.tanT * B.tanT) * 1.0001f;
    for (int k = 0; k < 3; ++k) {
        B.o[k] = apex[k];
        B.a[k] = a[k];
    }
    B.two = 0;
    B.ok = 1;
    return B;
}

// The culling tests are conservative f32 bounds, so they use explicit fmaf (the exact f64 tests keep
// the reference's unfused operations); the margins dominate either rounding.
// Radial distances are taken from cross products, whose f32 error is linear in the distance |v| from the
// line's origin (each component within ~4u |v| |d| of the exact one, u = 2^-24; with the f32 rounding of
// the direction, |v x d| within ~9u |v| |d|): the tests allow 2e-6 |v| (~30u) on top of the radius, with
// |v| <= q + |p| / |d| (q the radial, p the axial distance) and q <= the bound itself where it decides, so
// the slack is 2e-6 |p| / |d| and the bound's own (1 - 2e-6) factor sits inside the 1e-4 one.  (A radial
// distance squared as |v|^2 - p^2 cancels, with an error ~u |v|^2 that needed a 4e-6 |v|^2 term: for a
// node of radius r at distance |v| that widened r to sqrt(r^2 + 4e-6 |v|^2), doubling a 0.03-unit
// triangle's radius 17 units from the light — C4's teapot seen from its light: C4 0.766 -> 0.713 ms per
// frame.)  LIN: the bundle test with the cross product too (the kernels of scenes with groups, whose meshes
// hold many small nodes, and of small scenes, culls in LDS: C5 2.23 -> 2.17 ms); the large flat scenes' bundle
// tests keep the quadratic term, cheaper by the cross product (their nodes are large next to it: C2 +1.5 %
// with the cross product).
constexpr float RR_CULL_KAPPA = 2e-6f;
// sphere (c, r) vs the bundle's fat cone (forward nappe, or both nappes for line queries)
template <bool TWO_SIDED, bool LIN>
__device__ __forceinline__ bool bundle_may_hit(const Bundle& B, const DevCull& cl) {
    if (!(cl.r < __builtin_inff())) return true;
    const float vx = cl.c[0] - B.o[0], vy = cl.c[1] - B.o[1], vz = cl.c[2] - B.o[2];
    const float L2 = fmaf(vx, vx, fmaf(vy, vy, vz * vz));
    const float p = fmaf(B.a[0], vx, fmaf(B.a[1], vy, B.a[2] * vz));
    const float Rp = cl.r + B.rho;
    if (L2 <= Rp * Rp * 1.0001f) return true;  // the origin ball touches the sphere
    const float pp = (TWO_SIDED || B.two) ? fabsf(p) : p;
    const float rhs = fmaf(pp, B.tanT, Rp * B.secT);  // cone radius at depth pp, widened by Rp
    if (rhs < 0.0f) return false;
    if (!LIN) return fmaf(-pp, pp, L2) <= fmaf(rhs * rhs, 1.0001f, 4e-6f * L2);
    // radial distance from the axis: |a x v| (a unit up to ~1e-7, inside the 1e-4 factor)
    const float qx = fmaf(B.a[1], vz, -B.a[2] * vy), qy = fmaf(B.a[2], vx, -B.a[0] * vz),
                qz = fmaf(B.a[0], vy, -B.a[1] * vx);
    const float lim = fmaf(RR_CULL_KAPPA, fabsf(p), rhs);
    return fmaf(qx, qx, fmaf(qy, qy, qz * qz)) <= lim * lim * 1.0001f;
}

// this lane's ray line vs the sphere (f32 with rounding slack).  FWD (queries that only use entries
// with t >= 0): also the sphere's extent along the ray, (p -+ s) / |d|^2 with p = (c - o).d and
// s = (r + e_o + 1e-4 |c - o|_1) |d| (the 1e-4 term dominates the f32 rounding of p, ~4u L |d|), must
// reach [0, tmax]: spheres behind the origin, or beyond the lane's closest hit so far / the light,
// are skipped.  tmax is +inf or a value the query no longer needs entries beyond (an entry at tmax
// itself still passes: relative margin 1e-5 on top of s).
// SEG (shadow segments toward a point light, make_bundle_apex<true>): R.o is the light L and tmax the
// segment's length, so the segment is the line's parameter range [-tmax, 0] (t - distance): the node must
// not lie entirely beyond L (p - s > 1e-5 tmax |d|^2, the same relative margin as the far bound below) or
// entirely behind the origin (p + s < -tmax |d|^2 (1 + 1e-5)).
template <bool FWD, bool SEG = false>
__device__ __forceinline__ bool lane_may_hit(const LaneRay& R, const DevCull& cl, float tmax, bool near = true) {
    if (!(cl.r < __builtin_inff())) return true;
    const float vx = cl.c[0] - R.o[0], vy = cl.c[1] - R.o[1], vz = cl.c[2] - R.o[2];
    const float cx = fmaf(vy, R.d[2], -vz * R.d[1]), cy = fmaf(vz, R.d[0], -vx * R.d[2]),
                cz = fmaf(vx, R.d[1], -vy * R.d[0]);
    const float re = cl.r + R.eo;
    const float p = fmaf(vx, R.d[0], fmaf(vy, R.d[1], vz * R.d[2]));
    const float lim = fmaf(RR_CULL_KAPPA, fabsf(p), re * R.dl);  // |d| (r + e_o + 2e-6 |p| / |d|), see RR_CULL_KAPPA
    // written as "not provably outside": a NaN anywhere (a non-finite ray) passes every test, so such
    // rays get every node's exact test, as Scene::intersect gives them (their NaN entries: nan_census)
    const bool line = !(fmaf(cx, cx, fmaf(cy, cy, cz * cz)) > lim * lim * 1.0001f);
    if (!FWD) return line;
    const float sl = fmaf(1e-4f, fabsf(vx) + fabsf(vy) + fabsf(vz), re) * R.dl;
    if (SEG) return line && !(p + sl < -(tmax * R.dd * 1.00001f)) && !(p - sl > 1e-5f * tmax * R.dd);
    return line && !(near && p < -sl) && !(p - sl > tmax * R.dd * 1.00001f);
}

// lane k's value / ray data, as seen by every lane (ray-major chunk tests)
__device__ __forceinline__ float lane_f(float v, int k) {  // lane k's value, as seen by every lane
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}
__device__ __forceinline__ LaneRay lane_ray(const LaneRay& R, int k) {
    LaneRay r;
    for (int q = 0; q < 3; ++q) {
        r.o[q] = lane_f(R.o[q], k);
        r.d[q] = lane_f(R.d[q], k);
    }
    r.dd = lane_f(R.dd, k);
    r.dl = lane_f(R.dl, k);
    r.eo = lane_f(R.eo, k);
    return r;
}
__device__ __forceinline__ uint64_t lane_u64(uint64_t v, int k) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, k);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), k);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ DevCull lane_cull(const DevCull& c, int k) {
    DevCull r;
    r.c[0] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c.c[0]), k));
    r.c[1] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c.c[1]), k));
    r.c[2] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c.c[2]), k));
    r.r = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c.r), k));
    return r;
}

// Dynamic LDS of the walking kernels: the scene's node culls, then its chunk records, copied once
// per workgroup.
extern __shared__ DevCull rr_lds_culls[];
__device__ __forceinline__ DevChunk* lds_chunks(const DevScene& S) {
    return reinterpret_cast<DevChunk*>(rr_lds_culls + S.n_nodes);
}
__device__ __forceinline__ void stage_culls(const DevScene& S) {
    for (int j = threadIdx.x; j < S.n_nodes; j += 256) rr_lds_culls[j] = S.culls[j];  // 256-thread blocks
    DevChunk* ch = lds_chunks(S);
    for (int j = threadIdx.x; j < S.n_chunks; j += 256) ch[j] = S.chunks[j];
    __syncthreads();
}
template <bool LDS>
__device__ __forceinline__ DevCull load_cull(const DevScene& S, int j) {
    if (LDS) return rr_lds_culls[j];
    return S.culls[j];
}
template <bool LDS>
__device__ __forceinline__ DevChunk load_chunk(const DevScene& S, int j) {
    if (LDS) return lds_chunks(S)[j];
    return S.chunks[j];
}
__device__ __forceinline__ int lane_int(int v, int k) { return __builtin_amdgcn_readlane(v, k); }

// ---------------------------------------------------------------- CSG (csg.rs)
// One CSG subtree evaluated for one lane: every leaf's entries in the subtree's (reference) order,
// each group's list sorted after its AABB test (group.rs:80-91), each CSG's list
// left ++ right, stably sorted by t and filtered by its rule (csg.rs:67-113) — post-order over
// the contiguous subtree with an explicit stack.  The CSG subtree keeps the reference order
// (flatten.cpp), so list order == reference order.
struct CsgEntry {
    double t, u, v;
    int node, k;
};
__device__ __forceinline__ bool csg_allowed(int op, bool lhit, bool inl, bool inr) {
    if (op == RR_CSG_UNION) return (lhit && !inr) || (!lhit && !inl);
    if (op == RR_CSG_INTERSECTION) return (lhit && inr) || (!lhit && inl);
    return (lhit && !inr) || (!lhit && inl);
}
// nan: some sort of the evaluation (group.rs:88, csg.rs:231) saw a NaN t among >= 2 entries.
__device__ int csg_eval(const DevScene& S, const Ray& rw, int csg, CsgEntry* buf, uint64_t& tests, bool& nan) {
    cptr<DevNode> nodes = cp(S.nodes);
    int stk[RR_MAX_GROUP_DEPTH + 1], start[RR_MAX_GROUP_DEPTH + 1];
    int sp = 0, n = 0, raw = 0;
    bool nan_seen = false;
    stk[sp] = csg;
    start[sp] = 0;
    ++sp;
    int j = csg + 1;
    while (sp > 0) {
        const int top = stk[sp - 1];
        if (j >= nodes[top].skip) {  // close `top`: sort its segment (stable insertion), filter a CSG
            --sp;
            const int s0 = start[sp];
            for (int a = s0 + 1; a < n; ++a) {
                CsgEntry x = buf[a];
                int b = a;
                while (b > s0 && buf[b - 1].t > x.t) {
                    buf[b] = buf[b - 1];
                    --b;
                }
                buf[b] = x;
            }
            if (nodes[top].kind == RR_CSG) {
                cptr<DevGroup> g = cp(S.groups) + nodes[top].aux;
                const int op = g->csg_op, pos = g->depth - 1;  // position of `top` in a leaf's chain
                bool inl = false, inr = false;
                int m = s0;
                for (int a = s0; a < n; ++a) {
                    const bool lhit = (nodes[buf[a].node].flags >> (8 + pos)) & 1;
                    if (csg_allowed(op, lhit, inl, inr)) buf[m++] = buf[a];
                    if (lhit)
                        inl = !inl;
                    else
                        inr = !inr;
                }
                n = m;
            }
            continue;
        }
        cptr<DevNode> nd = nodes + j;
        const int kind = nd->kind;
        if (is_container(kind)) {
            if (kind == RR_GROUP) {
                const Ray rg = xf_ray(nd->inv, ray_in_space(S, rw, nd->parent));
                if (!aabb_hit(cp(S.groups)[nd->aux].aabb, rg)) {  // group.rs:82: no entries
                    j = nd->skip;
                    continue;
                }
            }
            stk[sp] = j;
            start[sp] = n;
            ++sp;
            ++j;
            continue;
        }
        const Ray lr = (nd->flags & NF_IDENT) ? ray_in_space(S, rw, nd->parent)
                                              : xf_ray(nd->inv, ray_in_space(S, rw, nd->parent));
        const EntriesT<4> e = leaf_intersect<4>(S, nd, kind, nd->aux, lr);
        ++tests;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < e.n) {
                nan_seen = nan_seen || isnan(e.t[q]);
                ++raw;
                if (n < RR_MAX_CSG_ENTRIES) buf[n++] = {e.t[q], e.u, e.v, j, e.k[q]};
            }
        ++j;
    }
    nan = nan_seen && raw >= 2;
    return n;
}

// Visits every node that some live lane's ray may reach, in increasing node index, with the ray in
// the node's parent space: fn(node_index, rank, entries) per leaf for the lanes that pass the line
// test (entries = the leaf's local_intersect, or its entries surviving a CSG filter); fn returns
// false to retire the lane (any-hit).  Two culling levels: lane j tests chunk j's bounding sphere
// against the wave's bundle (64 chunks per pass), then, inside a candidate chunk, lane j tests
// node start+j.  G = 0 flat scene, 1 groups, 2 groups and CSGs.  Groups are entered per lane
// through their exact AABB test (group.rs:80-91), whose miss skips the lane past the subtree; a CSG
// node is evaluated whole per lane (csg_eval) and its subtree is never visited directly.
// TWO_SIDED: the query needs entries at t < 0 too (the n1/n2 walk), so cull against the line.
template <int G>
constexpr int entries_max() {
    return G == 2 ? 4 : 2;
}
// kernels whose walks read across lanes (XL, walk_nodes); build.py fails the build if one spills VGPRs
constexpr bool cross_lane_ok(int G, bool CP, bool AR) { return G < 2 && !CP && !AR; }
// Scene::intersect sorts with partial_cmp().unwrap() (scene.rs:104; group.rs:88, csg.rs:231 inside):
// a NaN t in a list of >= 2 entries panics the reference.  Exact tests of a finite ray against the
// scene's finite geometry give no NaN t, so only a ray with a non-finite origin or direction needs
// the census: every node's exact test in Scene::intersect's order (group boxes and CSG evaluation as
// the reference runs them), counting entries and NaNs.  Run for such lanes only (wave-uniform branch);
// returns whether this lane's list would panic.
template <int G>
__device__ bool nan_census(const DevScene& S, const Ray& rw, bool bad) {
    constexpr int M = entries_max<G>();
    cptr<DevNode> nodes = cp(S.nodes);
    int n = 0, skip_until = 0;
    bool nan = false, panic = false;
    for (int j = 0; j < S.n_nodes;) {  // storage order: entry counts do not depend on it
        cptr<DevNode> nd = nodes + j;
        const int kind = nd->kind;
        if (G == 2 && (nd->flags & NF_IN_CSG)) {  // reached through its CSG
            ++j;
            continue;
        }
        const bool part = bad && j >= skip_until;
        const Ray rp = ray_in_space(S, rw, nd->parent);
        if (kind == RR_GROUP) {  // group.rs:80-91: the children only when the box is hit
            const bool hit = part && aabb_hit(cp(S.groups)[nd->aux].aabb, xf_ray(nd->inv, rp));
            if (part && !hit) skip_until = nd->skip;
            j = __ballot(hit) != 0 ? j + 1 : nd->skip;
            continue;
        }
        if (kind == RR_CSG) {
            if constexpr (G == 2) {
                CsgEntry buf[RR_MAX_CSG_ENTRIES];
                uint64_t lt = 0;
                bool csg_nan = false;
                if (part) {
                    const int ne = csg_eval(S, rw, j, buf, lt, csg_nan);
                    for (int a = 0; a < ne; ++a) nan = nan || isnan(buf[a].t);
                    n += ne;
                    panic = panic || csg_nan;
                }
            }
            j = nd->skip;
            continue;
        }
        if (part) {
            const Ray lr = (nd->flags & NF_IDENT) ? rp : xf_ray(nd->inv, rp);
            const EntriesT<M> e = leaf_intersect<M>(S, nd, kind, nd->aux, lr);
#pragma unroll
            for (int q = 0; q < M; ++q) nan = nan || (q < e.n && isnan(e.t[q]));
            n += e.n;
        }
        ++j;
    }
    return bad && (panic || (nan && n >= 2));
}

// tmax: per-lane bound for the forward culls (lane_may_hit<FWD>; ignored when TWO_SIDED), which fn
// may lower as the query progresses (closest hit so far).
// XL: the walk may read other lanes' registers (v_readlane of the chunk / cull records a lane loaded,
// ray-major tests).  Only kernels the build proves free of VGPR spills get it (build.py checks
// cross_lane_ok kernels for "VGPRs Spill: 0"): a spilled register reloaded under a partial exec mask
// holds stale data in the inactive lanes, which v_readlane returns — squeezed G = 2 builds (~300
// spills) rendered wrong, run-to-run different pixels that way, and reloading the records with a
// uniform address instead removed them (tools/diag_variants.sh, DESIGN.md §3.6).  Other kernels
// reload the chunk / cull records from LDS or memory and skip the ray-major test.
// ORD (closest-hit walks of incoherent waves): candidate chunks in increasing entry distance along the
// bundle axis instead of storage order, so the closest hit is found early and tmax culls the chunks
// behind it (the result is the minimum (t, rank, k) over all entries either way).  Cross-lane (XL) only.
// OWN (shadow walks): `own` is a node this lane's query provably gets no answer from (own_node: its hit object); its
// exact test is skipped for the lane, and a node whose passing lanes all own it is not visited.
// AWAY (forward queries of the chain kernels): the identity planes are skipped for lanes whose origin and direction lie
// strictly on one side of them (C3 6.10 -> 6.02 ms; C2's shade kernel measured 0.6 % slower with it, so it keeps none)
template <int G, bool TWO_SIDED, bool LDS, bool RM, bool XL, bool SHIFT = false, bool ORD = false, bool APEX = false,
          bool OWN = false, bool AWAY = false, class Fn>
__device__ __forceinline__ void walk_nodes(const DevScene& S, const Ray& rw, bool live, Counters& cnt, const float& tmax,
                                           Fn&& fn, const float* apex = nullptr, bool cam_tile = false,
                                           const float* cam_bundle = nullptr, uint32_t node_mask = ~0u, int own = -1) {
    const auto other = [&](int i) { return !OWN || i != own; };
    constexpr bool GROUPS = G > 0;
    constexpr int M = entries_max<G>();
    constexpr bool SEG = APEX && G > 0;  // lane rays through the light (make_bundle_apex<true>)
    constexpr bool LIN = G > 0 || LDS;   // bundle tests with the linear slack (RR_CULL_KAPPA)
    if (__ballot(live) == 0) return;
    {  // NaN t can only come from a non-finite ray (the f32 sum is non-finite for inf / NaN components)
        const float sum = (float)rw.o.x + (float)rw.o.y + (float)rw.o.z + (float)rw.d.x + (float)rw.d.y + (float)rw.d.z;
        const bool bad = live && !isfinite(sum);
        if (__ballot(bad) != 0) cnt.nan += popc_ballot(nan_census<G>(S, rw, bad));
    }
    cptr<DevNode> nodes = cp(S.nodes);
    LaneRay LR;
    if constexpr (G == 0 && LDS) {
        // Flat scenes of a few nodes (C5's plane and sphere, the README scene): no bundle, no chunk
        // passes — node by node, the lane's line test on the node's cull record (an LDS broadcast),
        // then the exact test for the lanes that pass.  The chunk machinery (chunk records, candidate
        // ballots, cull-record loads per chunk) cost more than it could cull here: C5 2.82 -> 2.30 ms,
        // C1 0.227 -> 0.216 ms.  Only the LDS-culls kernels carry it (every such scene stages its few
        // culls): the large scenes' kernels keep their code and registers.
        // node_mask (area-light walks): bit i clear = the light-hull pre-test proved node i cannot shadow this lane's
        // segment, so its exact test is skipped (the answer, some entry with 0 <= t < distance, is unchanged)
        if (S.n_nodes <= RR_BUNDLE_MIN_NODES) {
            float shift;
            (void)make_bundle<false>(S, rw, live, LR, false, shift);  // lane rays only
            constexpr int M = entries_max<G>();
            for (int i = 0; i < S.n_nodes; ++i) {
                const DevCull cl = rr_lds_culls[i];
                const bool part = live && ((node_mask >> i) & 1u) && other(i) && lane_may_hit<!TWO_SIDED>(LR, cl, tmax);
                const uint64_t np = popc_ballot(part);
                if (np == 0) continue;
                cptr<DevNode> nd = nodes + i;
                cnt.visits++;
                const int kind = nd->kind, aux = nd->aux, rank = nd->rank;
                cnt.tests += np;
                cnt.flops += np * test_flops(kind);
                if (part) {
                    Ray lr = xf_ray_node(nd->flags, nd->inv, rw);
                    live = fn(i, rank, leaf_intersect<M, !TWO_SIDED>(S, nd, kind, aux, lr));
                }
                if (__ballot(live) == 0) break;
            }
            return;
        }
    }
    float shift = 0.0f;
    Bundle B;
    if constexpr (APEX) {
        B = make_bundle_apex<SEG>(S, rw, live, LR, apex);
    } else {
        B = make_bundle<SHIFT>(S, rw, live, LR, S.n_nodes > RR_BUNDLE_MIN_NODES, shift, cam_tile, cam_bundle);
    }
    // SHIFT walks have a fixed tmax (the light distance): bound in the moved origin's frame, with the
    // near bound dropped for lanes moved forward (their segment starts behind o')
    const float tm_shift = SHIFT ? (tmax - shift) + 1e-6f * (fabsf(tmax) + fabsf(shift)) : 0.0f;
    const bool near = !SHIFT || !(shift > 0.0f);
    const float& TM = SHIFT ? tm_shift : tmax;
    const int lane = lane_id();
    Ray rc = rw;
    int cur = -1;
    int skip_until = 0;
    const DevCull none = {{0.0f, 0.0f, 0.0f}, -1.0f};
    const int nch = S.n_chunks - S.n_free;
    // global chunk records: the first pass's, loaded before the plane tests so the load overlaps them (C2 -1.5 %;
    // LDS records are near, and the registers cost the small scenes' area-light kernels 4 %)
    DevChunk chl0;
    if (!LDS && lane < nch) {
        chl0 = load_chunk<LDS>(S, lane);
    } else {
        chl0.cull = none;
        chl0.start = chl0.count = 0;
    }
    {
        // the scene's planes (lone unbounded top-level leaves, stored last) before the chunk passes: no
        // cull can reject them, and a closest-hit walk that finds the floor first culls what lies behind
        // it.  Top-level: the node's inverse applies to the world ray (no group ancestors, no CSG).
        const int nf = S.n_free;
        constexpr int M = entries_max<G>();
        // AWAY: a lane whose origin and direction lie strictly on one side of the identity planes (every free plane is
        // y = 0 when S.free_planes) gets t = -o.y / d.y < 0 from each, never a usable entry of a forward query
        // (plane.rs:51-58); the bounds keep the quotient away from underflow (-0.0 would pass t >= 0)
        const bool away = AWAY && !TWO_SIDED && !RM && S.free_planes &&
                          ((rw.o.y > 0x1p-900 && rw.d.y > 0.0 && rw.d.y < 0x1p100) ||
                           (rw.o.y < -0x1p-900 && rw.d.y < 0.0 && rw.d.y > -0x1p100));
        for (int i = S.n_nodes - nf; i < S.n_nodes; ++i) {
            if (OWN && __ballot(live) == 0) break;
            const bool part = live && other(i) && !away;
            const uint64_t np = popc_ballot(part);
            if (np == 0) {
                if (OWN) continue;
                break;
            }
            cptr<DevNode> nd = nodes + i;
            cnt.visits++;
            cnt.tests += np;
            if (!RM && S.free_planes) {  // identity planes (DevScene.free_planes): no dispatch (the ray-major
                                         // kernels spill with both paths)
                const int rank = nd->rank;
                cnt.flops += np * 13u;  // test_flops(RR_PLANE)
                if (part) {
                    EntriesT<M> e = empty_entries<M>();
                    plane_intersect(rw, e);
                    live = fn(i, rank, e);
                }
                continue;
            }
            const int kind = nd->kind, aux = nd->aux, rank = nd->rank;
            cnt.flops += np * test_flops(kind);
            if (part) {
                Ray lr = xf_ray_node(nd->flags, nd->inv, rw);
                live = fn(i, rank, leaf_intersect<M, !TWO_SIDED>(S, nd, kind, aux, lr));
            }
        }
        if (__ballot(live) == 0) {
            return;
        }
    }
    for (int cb = 0; cb < nch; cb += 64) {
        const bool cin = cb + lane < nch;
        DevChunk chl;
        if (!LDS && cb == 0) {
            chl = chl0;
        } else if (cin) {
            chl = load_chunk<LDS>(S, cb + lane);
        } else {
            chl.cull = none;
            chl.start = chl.count = 0;
        }
        uint64_t cmask = __ballot(cin && (!B.ok || bundle_may_hit<TWO_SIDED, LIN>(B, chl.cull)));
        constexpr bool ORDERED = ORD && XL;
        float key = __builtin_inff();  // ORDERED: entry distance of this lane's chunk along the bundle axis
        if (ORDERED && B.ok) {
            const float p = B.a[0] * (chl.cull.c[0] - B.o[0]) + B.a[1] * (chl.cull.c[1] - B.o[1]) +
                            B.a[2] * (chl.cull.c[2] - B.o[2]);
            key = (chl.cull.r < __builtin_inff()) ? p - chl.cull.r : -__builtin_inff();
        }
        while (cmask) {
            int kc = __ffsll((long long)cmask) - 1;
            if (ORDERED && B.ok && (cmask & (cmask - 1))) {  // the nearest remaining candidate
                const float kmin = uniform_f(wave_min_f(((cmask >> lane) & 1ull) ? key : __builtin_inff()));
                const uint64_t at = __ballot(((cmask >> lane) & 1ull) && key == kmin);
                if (at) kc = __ffsll((long long)at) - 1;
            }
            cmask &= ~(1ull << kc);
            // chunk kc's record: read across lanes (XL) or reloaded with a uniform address (see XL above)
            const DevChunk chk = XL ? DevChunk{lane_cull(chl.cull, kc), lane_int(chl.start, kc), lane_int(chl.count, kc),
                                               lane_int(chl.run, kc), 0}
                                    : load_chunk<LDS>(S, cb + kc);
            // the lanes whose line reaches the chunk: the ray-major test needs them; elsewhere the per-node line
            // tests below decide alone (a chunk-level line test cost more than the node passes it saved)
            uint64_t reach = ~0ull;
            if constexpr (RM) {
                reach = __ballot(live && lane_may_hit<!TWO_SIDED, SEG>(LR, chk.cull, TM, near));
                if (reach == 0) continue;
            }
            const int start = chk.start, count = chk.count;
            const bool in = lane < count;
            const DevCull mine = in ? load_cull<LDS>(S, start + lane) : none;
            uint64_t mask = __ballot(in && (!B.ok || bundle_may_hit<TWO_SIDED, LIN>(B, mine)));
            // Incoherent waves (few of the rays reach this chunk, many of its nodes survive the bundle):
            // test ray-major — each reaching ray against all of the chunk's nodes at once, lane j holding
            // node j — which gives per node the lanes whose line passes it.  The same f32 test, with each
            // ray's tmax as of now (tmax only decreases, so the result stays conservative).
            uint64_t rays = 0;  // lane j: lanes whose ray may hit node start + j (ray-major only)
            const bool ray_major = XL && RM && 4 * __popcll(reach) < 3 * __popcll(mask);
            if (ray_major) {
                const uint64_t near_m = __ballot(near);
                uint64_t rm = reach;
                while (rm) {
                    const int k = __ffsll((long long)rm) - 1;
                    rm &= rm - 1;
                    if (in && lane_may_hit<!TWO_SIDED, SEG>(lane_ray(LR, k), mine, lane_f(TM, k), ((near_m >> k) & 1ull) != 0))
                        rays |= 1ull << k;
                }
                mask &= __ballot(rays != 0);
            }
            if (GROUPS && chk.run >= 0) {
                // a mesh run (DevChunk.run): inline triangles of one parent, so no per-node kind, flag or transform
                // dispatch — each candidate's p1 / e1 / e2 and rank load together, with one wait (C4 0.697 -> 0.590
                // ms per frame, example1 28.2 -> 18.5 ms)
                const int parent = chk.run;
                while (mask) {
                    const int k = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const int i = start + k;
                    const bool line = ray_major ? ((lane_u64(rays, k) >> lane) & 1ull) != 0
                                                : lane_may_hit<!TWO_SIDED, SEG>(LR, XL ? lane_cull(mine, k) : load_cull<LDS>(S, i), TM, near);
                    const bool part = live && i >= skip_until && line;
                    const uint64_t np = popc_ballot(part);
                    if (np == 0) continue;
                    cptr<DevNode> nd = nodes + i;
                    const int rank = nd->rank;
                    cnt.visits++;
                    cnt.tests += np;
                    cnt.flops += np * 45u;  // test_flops(RR_TRIANGLE)
                    if (part) {
                        if (parent != cur) {
                            rc = ray_in_space(S, rw, parent);
                            cur = parent;
                        }
                        EntriesT<M> e = empty_entries<M>();
                        tri_intersect(nd->inv, rc, e);
                        live = fn(i, rank, e);
                    }
                    if (__ballot(live) == 0) return;
                }
                continue;
            }
            if (!GROUPS && chk.run == CR_SPHERE_DIAG) {  // a run of top-level spheres with diagonal inverses
                while (mask) {
                    const int k = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const int i = start + k;
                    const bool line = ray_major ? ((lane_u64(rays, k) >> lane) & 1ull) != 0
                                                : lane_may_hit<!TWO_SIDED, SEG>(LR, XL ? lane_cull(mine, k) : load_cull<LDS>(S, i), TM, near);
                    const bool part = live && line && other(i);
                    const uint64_t np = popc_ballot(part);
                    if (np == 0) continue;
                    cptr<DevNode> nd = nodes + i;
                    const int rank = nd->rank;
                    cnt.visits++;
                    cnt.tests += np;
                    cnt.flops += np * 57u;  // test_flops(RR_SPHERE)
                    if (part) {
                        EntriesT<M> e = empty_entries<M>();
                        sphere_intersect<M, !TWO_SIDED>(xf_ray_diag(nd->inv, rw), e);
                        live = fn(i, rank, e);
                    }
                    if (__ballot(live) == 0) return;
                }
                continue;
            }
            while (mask) {
                const int k = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const int i = start + k;
                cptr<DevNode> nd = nodes + i;
                if (G == 2 && (nd->flags & NF_IN_CSG)) continue;  // reached only through its CSG
                const bool line = ray_major ? ((lane_u64(rays, k) >> lane) & 1ull) != 0
                                            : lane_may_hit<!TWO_SIDED, SEG>(LR, XL ? lane_cull(mine, k) : load_cull<LDS>(S, i), TM, near);
                const bool part = live && (!GROUPS || i >= skip_until) && line && other(i);
                const uint64_t np = popc_ballot(part);
                if (np == 0) continue;
                cnt.visits++;
                const int kind = nd->kind, aux = nd->aux, rank = nd->rank;
                if (!GROUPS) {
                    cnt.tests += np;
                    cnt.flops += np * test_flops(kind);
                    if (part) {
                        Ray lr = xf_ray_node(nd->flags, nd->inv, rw);
                        live = fn(i, rank, leaf_intersect<M, !TWO_SIDED>(S, nd, kind, aux, lr));
                    }
                } else {
                    const int parent = nd->parent;
                    if (kind == RR_GROUP) {
                        cnt.gtests += np;
                    } else if (kind != RR_CSG) {
                        cnt.tests += np;
                    }
                    cnt.flops += np * test_flops(kind);
                    bool ghit = false;
                    if (part) {
                        if (kind == RR_CSG) {
                            if constexpr (G == 2) {
                                CsgEntry buf[RR_MAX_CSG_ENTRIES];
                                uint64_t lt = 0;
                                bool csg_nan = false;  // finite rays give no NaN t (nan_census)
                                const int ne = csg_eval(S, rw, i, buf, lt, csg_nan);
                                // deliver each leaf's surviving entries (in their list order)
                                for (int j = i + 1; j < nd->skip && live; ++j) {
                                    EntriesT<M> e;
                                    e.n = 0;
                                    e.u = 0.0;
                                    e.v = 0.0;
                                    for (int q = 0; q < M; ++q) {
                                        e.t[q] = 0.0;
                                        e.k[q] = 0;
                                    }
                                    for (int a = 0; a < ne; ++a)
                                        if (buf[a].node == j && e.n < M) {
#pragma unroll
                                            for (int q = 0; q < M; ++q)
                                                if (e.n == q) {
                                                    e.t[q] = buf[a].t;
                                                    e.k[q] = buf[a].k;
                                                }
                                            e.u = buf[a].u;
                                            e.v = buf[a].v;
                                            e.n++;
                                        }
                                    if (e.n > 0) live = fn(j, nodes[j].rank, e);
                                }
                            }
                        } else {
                            if (parent != cur) {
                                rc = ray_in_space(S, rw, parent);
                                cur = parent;
                            }
                            if (kind == RR_GROUP) {  // group.rs:80-91: ray into group space, AABB, then children
                                Ray rg = xf_ray(nd->inv, rc);
                                if (aabb_hit(cp(S.groups)[aux].aabb, rg)) {
                                    ghit = true;
                                    rc = rg;
                                    cur = i;
                                } else {
                                    skip_until = nd->skip;
                                }
                            } else {
                                Ray lr = xf_ray_node(nd->flags, nd->inv, rc);
                                live = fn(i, rank, leaf_intersect<M, !TWO_SIDED>(S, nd, kind, aux, lr));
                            }
                        }
                    }
                    if (kind == RR_GROUP) cnt.ghits += popc_ballot(ghit);
                }
                if (__ballot(live) == 0) {
                    return;
                }
            }
        }
    }
}

// Closest hit == first entry with t >= 0 of the stably sorted list (scene.rs:128-136): the minimum
// of (t, rank, local index) over all entries with t >= 0, whatever order the nodes are visited in.
// MAT: also the hit node's material (h.mat)
// OWN / own: a node the lane's ray provably has no entry t >= 0 in (reflect_own), skipped for the lane
template <int G, bool LDS, bool RM, bool XL, bool MAT = false, bool OWN = false, bool AWAY = false>
__device__ __forceinline__ void trace_closest(const DevScene& S, const Ray& rw, bool active, Hit& h, Counters& cnt,
                                              bool cam_tile = false, const float* cam_bundle = nullptr, int own = -1) {
    h.found = false;
    h.t = 0.0;
    h.u = 0.0;
    h.v = 0.0;
    h.node = -1;
    h.k = 0;
    h.rank = 0x7fffffff;
    h.mat = 0;
    float tmax = __builtin_inff();  // nodes entirely beyond the closest hit so far are skipped
    // ordered candidate chunks on incoherent levels of flat scenes (C3 level >= 1: 11.76 -> 11.71 ms; the
    // group scenes' mesh walks lost 3 % to the ordering overhead)
    walk_nodes<G, false, LDS, RM, XL, false, RM && G == 0, false, OWN, AWAY>(S, rw, active, cnt, tmax, [&](int i, int rank, const auto& e) {
        constexpr int M = entries_max<G>();
#pragma unroll
        for (int q = 0; q < M; ++q) {
            const double t = e.t[q];
            if (q < e.n && t >= 0.0 &&
                (!h.found || t < h.t || (t == h.t && (rank < h.rank || (rank == h.rank && e.k[q] < h.k))))) {
                h.found = true;
                h.t = t;
                h.u = e.u;
                h.v = e.v;
                h.node = i;
                h.k = e.k[q];
                h.rank = rank;
                if (MAT) h.mat = cp(S.nodes)[i].material;  // wave-uniform, next to the walk's own loads of the record
                tmax = (float)t;
            }
        }
        return true;
    }, nullptr, cam_tile, cam_bundle, ~0u, own);
}

// Scene::is_shadowed (scene.rs:234-245): shadowed <=> some entry with 0 <= t < distance (the
// minimum t >= 0 is below distance iff any t >= 0 is).  Lanes retire at their first occluder and
// the wave stops when every lane has its answer.
// dir / distance: normalize(light_pos - p) and its magnitude (scene.rs:235-237).
// own (OWN): own_node of the lane's hit, or -1; honoured for lights within 1e6 (own_node's bound)
template <int G, bool LDS, bool RM, bool XL, bool POINT = false, bool OWN = false, bool AWAY = false>
__device__ __forceinline__ bool shadowed_dir(const DevScene& S, V3 p, V3 dir, double distance, V3 light_pos, bool active,
                                             Counters& cnt, uint32_t node_mask = ~0u, int own = -1) {
    Ray rw = {p, dir};
    bool hit = false;
    cnt.shadow += popc_ballot(active);
    const float tmax = (float)distance;  // entries at t >= distance do not shadow
    // POINT (light_pos wave-uniform): the apex bundle of make_bundle_apex; in scenes with groups also the
    // lane rays through the light (SEG), which keeps horizon origins' line tests tight (meshes make their
    // all-node walks expensive, C4).  Area-light walks of group scenes take the far-origin shift
    // (make_bundle<true>) instead; flat scenes keep the lean walk.
    constexpr bool APEX = POINT;
    const float apex[3] = {(float)light_pos.x, (float)light_pos.y, (float)light_pos.z};
    if (OWN && !(distance < 1e6)) own = -1;
    walk_nodes<G, false, LDS, RM, XL, (G > 0) && !APEX, false, APEX, OWN, AWAY>(S, rw, active, cnt, tmax, [&](int, int, const auto& e) {
        constexpr int M = entries_max<G>();
        bool any = false;
#pragma unroll
        for (int q = 0; q < M; ++q) any = any || (q < e.n && e.t[q] >= 0.0 && e.t[q] < distance);
        if (any) {
            hit = true;
            return false;
        }
        return true;
    }, apex, false, nullptr, node_mask, own);
    return hit;
}
template <int G, bool LDS, bool RM, bool XL, bool POINT = false, bool OWN = false, bool AWAY = false>
__device__ __forceinline__ bool shadowed(const DevScene& S, V3 p, V3 light_pos, bool active, Counters& cnt,
                                         uint32_t node_mask = ~0u, int own = -1) {
    const V3 v = vsub(light_pos, p);
    const double distance = sqrt(dot3(v, v));
    return shadowed_dir<G, LDS, RM, XL, POINT, OWN, AWAY>(S, p, div3(v, distance), distance, light_pos, active, cnt,
                                                          node_mask, own);
}

// prepare_computations' n1/n2 container walk (intersection.rs:61-92) without a sorted list.  The
// loop has no break: n1 / n2 are set at every entry equal by value to the hit (same t, object, u,
// v), so the LAST such entry e* decides — the hit node's entry with t == hit.t and the largest
// local index.  Before e* (key (t, rank, k) < key(e*)) the containers hold exactly the objects
// with an odd number of entries, ordered by their latest such entry; n1 = the last of them, and
// after e* toggles the hit object n2 = the hit object if it is now inside, else the last of the
// others.  h.rank must be the hit node's rank.  (Subsumes the tangent-sphere duplicate.)
template <int G, bool LDS, bool RM, bool XL>
__device__ __forceinline__ void n1n2_walk(const DevScene& S, const Ray& rw, const Hit& h, bool active, double& n1,
                                          double& n2, Counters& cnt) {
    int best_all = -1, best_ex = -1;  // node indices
    int br_all = 0, br_ex = 0;        // their ranks
    double bt_all = 0.0, bt_ex = 0.0;
    int bk_all = 0, bk_ex = 0;        // local index of that latest entry (ties within one t)
    int ch = 0;                       // hit node's entries before e*
    cnt.n1n2 += popc_ballot(active);
    const float tmax = __builtin_inff();
    walk_nodes<G, true, LDS, RM, XL>(S, rw, active, cnt, tmax, [&](int i, int rank, const auto& e) {
        constexpr int M = entries_max<G>();
        const bool hitnode = i == h.node;
        int kmax = -1;  // e*: the hit node's last entry (list order) equal to the hit
        if (hitnode) {
#pragma unroll
            for (int q = 0; q < M; ++q)
                if (q < e.n && e.t[q] == h.t && e.k[q] > kmax) kmax = e.k[q];
        }
        int cnt_before = 0;
        double last_t = 0.0;
        int last_k = -1;
#pragma unroll
        for (int q = 0; q < M; ++q) {
            if (q >= e.n) continue;
            const double t = e.t[q];
            const int k = e.k[q];
            const bool before = hitnode ? (t < h.t || (t == h.t && k < kmax))
                                        : (t < h.t || (t == h.t && rank < h.rank));
            if (before) {
                cnt_before++;
                if (last_k < 0 || t > last_t || (t == last_t && k > last_k)) {  // latest (t, k) of the node
                    last_t = t;
                    last_k = k;
                }
            }
        }
        if (hitnode) ch = cnt_before;
        if (cnt_before & 1) {  // max of (t, rank, k): a later key sorts after
            if (best_all < 0 || last_t > bt_all || (last_t == bt_all && (rank > br_all || (rank == br_all && last_k > bk_all)))) {
                best_all = i;
                br_all = rank;
                bt_all = last_t;
                bk_all = last_k;
            }
            if (!hitnode &&
                (best_ex < 0 || last_t > bt_ex || (last_t == bt_ex && (rank > br_ex || (rank == br_ex && last_k > bk_ex))))) {
                best_ex = i;
                br_ex = rank;
                bt_ex = last_t;
                bk_ex = last_k;
            }
        }
        return true;
    });
    if (!active) return;
    auto ri = [&](int node) -> double {
        if (node < 0) return 1.0;
        return S.mats[S.nodes[node].material].refractive_index;
    };
    n1 = ri(best_all);
    n2 = (ch & 1) ? ri(best_ex) : ri(h.node);  // e* pushes the hit object iff its count was even
}

// world_to_object (object.rs:102-109): parents first, then the object itself.  nd: the node's record (loaded
// once by the caller).
__device__ __forceinline__ V3 world_to_object(const DevScene& S, const DevNode& nd, V3 p) {
    if (nd.parent >= 0) {
        // through a pointer: a copied DevGroup indexed by the loop counter would live in scratch
        cptr<DevGroup> g = cp(S.groups) + cp(S.nodes)[nd.parent].aux;
        const int depth = g->depth;
        for (int k = 0; k < depth; ++k) p = xf_point(cp(S.nodes)[g->anc[k]].inv, p);
    }
    if (nd.flags & NF_IDENT) return p;
    if (nd.flags & NF_DIAG) return {nd.inv[0] * p.x + nd.inv[3], nd.inv[5] * p.y + nd.inv[7], nd.inv[10] * p.z + nd.inv[11]};
    return xf_point(nd.inv, p);
}
__device__ __forceinline__ V3 world_to_object(const DevScene& S, int node, V3 p) {
    const DevNode nd = S.nodes[node];
    return world_to_object(S, nd, p);
}

// normal_to_world (object.rs:129-138): object first, normalize at every level, then parents.  nd0: the
// node's own record (loaded once by the caller; the loop loads only the ancestors').
__device__ __forceinline__ V3 normal_level(const DevNode& nd, V3 n) {
    if (nd.flags & NF_TRI_INLINE) {  // identity inverse (the slots hold the triangle): the same products
        const double I[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
        return normalize3(xf_normal(I, n));
    }
    return normalize3((nd.flags & NF_DIAG) ? mk(nd.inv[0] * n.x, nd.inv[5] * n.y, nd.inv[10] * n.z) : xf_normal(nd.inv, n));
}
__device__ __forceinline__ V3 normal_to_world(const DevScene& S, const DevNode& nd0, V3 n) {
    n = normal_level(nd0, n);
    for (int cur = nd0.parent; cur >= 0;) {
        const DevNode nd = S.nodes[cur];
        n = normal_level(nd, n);
        cur = nd.parent;
    }
    return n;
}

// saturating `as i32`
__device__ __forceinline__ int sat_i32(double v) {
    if (v != v) return 0;
    if (v >= 2147483647.0) return 2147483647;
    if (v <= -2147483648.0) return (int)(-2147483647 - 1);
    return (int)v;
}

// noise.rs:11-29 over fastnoise-lite 1.1.1 Perlin (crate feature "f64"; seed 1337, frequency
// 0.01f32 widened to f64, no fractal / rotation).  Lattice math in f64 and wrapping i32, the
// fractional parts and the whole interpolation in f32 (compiled without contraction, so each
// f32 operation rounds like rustc's).  Oracle: oracle/rray_oracle.cpp namespace fnl.
__constant__ float c_grad3[192] = {  // GRADIENTS_3D without its always-zero 4th column
    0, 1, 1, 0, -1, 1, 0, 1, -1, 0, -1, -1, 1, 0, 1, -1, 0, 1, 1, 0, -1, -1, 0, -1,
    1, 1, 0, -1, 1, 0, 1, -1, 0, -1, -1, 0, 0, 1, 1, 0, -1, 1, 0, 1, -1, 0, -1, -1,
    1, 0, 1, -1, 0, 1, 1, 0, -1, -1, 0, -1, 1, 1, 0, -1, 1, 0, 1, -1, 0, -1, -1, 0,
    0, 1, 1, 0, -1, 1, 0, 1, -1, 0, -1, -1, 1, 0, 1, -1, 0, 1, 1, 0, -1, -1, 0, -1,
    1, 1, 0, -1, 1, 0, 1, -1, 0, -1, -1, 0, 0, 1, 1, 0, -1, 1, 0, 1, -1, 0, -1, -1,
    1, 0, 1, -1, 0, 1, 1, 0, -1, -1, 0, -1, 1, 1, 0, -1, 1, 0, 1, -1, 0, -1, -1, 0,
    0, 1, 1, 0, -1, 1, 0, 1, -1, 0, -1, -1, 1, 0, 1, -1, 0, 1, 1, 0, -1, -1, 0, -1,
    1, 1, 0, -1, 1, 0, 1, -1, 0, -1, -1, 0, 1, 1, 0, 0, -1, 1, -1, 1, 0, 0, -1, -1};

__device__ __forceinline__ int32_t fnl_floor(double f) {  // FastFloor: `as i32` (saturating)
    int32_t i = sat_i32(f);
    return f >= 0 ? i : (int32_t)((uint32_t)i - 1u);
}
__device__ __forceinline__ float fnl_quintic(float t) { return t * t * t * (t * (t * 6.0f - 15.0f) + 10.0f); }
__device__ __forceinline__ float fnl_lerp(float a, float b, float t) { return a + t * (b - a); }
__device__ __forceinline__ float fnl_grad(int32_t xp, int32_t yp, int32_t zp, float xd, float yd, float zd) {
    uint32_t h = (uint32_t)(1337 ^ xp ^ yp ^ zp) * 0x27d4eb2du;
    int32_t hash = (int32_t)h;
    hash ^= hash >> 15;
    int g = ((hash >> 2) & 63) * 3;
    return xd * c_grad3[g] + yd * c_grad3[g + 1] + zd * c_grad3[g + 2];
}
__device__ float fnl_perlin(double x, double y, double z) {  // get_noise_3d -> single_perlin
    const double freq = (double)0.01f;
    x *= freq;
    y *= freq;
    z *= freq;
    int32_t x0 = fnl_floor(x), y0 = fnl_floor(y), z0 = fnl_floor(z);
    float xd0 = (float)(x - (double)x0), yd0 = (float)(y - (double)y0), zd0 = (float)(z - (double)z0);
    float xd1 = xd0 - 1.0f, yd1 = yd0 - 1.0f, zd1 = zd0 - 1.0f;
    float xs = fnl_quintic(xd0), ys = fnl_quintic(yd0), zs = fnl_quintic(zd0);
    const uint32_t PX = 501125321u, PY = 1136930381u, PZ = 1720413743u;
    int32_t xa = (int32_t)((uint32_t)x0 * PX), ya = (int32_t)((uint32_t)y0 * PY), za = (int32_t)((uint32_t)z0 * PZ);
    int32_t xb = (int32_t)((uint32_t)xa + PX), yb = (int32_t)((uint32_t)ya + PY), zb = (int32_t)((uint32_t)za + PZ);
    float xf00 = fnl_lerp(fnl_grad(xa, ya, za, xd0, yd0, zd0), fnl_grad(xb, ya, za, xd1, yd0, zd0), xs);
    float xf10 = fnl_lerp(fnl_grad(xa, yb, za, xd0, yd1, zd0), fnl_grad(xb, yb, za, xd1, yd1, zd0), xs);
    float xf01 = fnl_lerp(fnl_grad(xa, ya, zb, xd0, yd0, zd1), fnl_grad(xb, ya, zb, xd1, yd0, zd1), xs);
    float xf11 = fnl_lerp(fnl_grad(xa, yb, zb, xd0, yd1, zd1), fnl_grad(xb, yb, zb, xd1, yd1, zd1), xs);
    float yf0 = fnl_lerp(xf00, xf10, ys);
    float yf1 = fnl_lerp(xf01, xf11, ys);
    return fnl_lerp(yf0, yf1, zs) * 0.964921414852142333984375f;
}
__device__ double octave_perlin(double x, double y, double z, int octaves, double persistence) {
    double total = 0.0, frequency = 1.0, amplitude = 1.0, max_value = 0.0;
    for (int i = 0; i < octaves; ++i) {
        total += (double)fnl_perlin(x * frequency, y * frequency, z * frequency) * amplitude;
        max_value += amplitude;
        amplitude *= persistence;
        frequency *= 2.0;
    }
    return total / max_value;
}

// Texture pattern (pattern.rs:209-213): Object::uv_mapping of the shaded object at the pattern
// point, then Texture::sample_texture (texture.rs:31-55).  uv per kind: sphere.rs:126-132,
// plane.rs:105-113, cube.rs:132-175, cylinder.rs:181-197, cone.rs:232-257, triangle.rs:148-170
// (smooth_triangle.rs:151-173 identical; v0 = p2 - p1 is exactly e1, v1 = e2); containers keep the
// trait default (0, 0).  Out of line: atan2 / acos stay off the shading kernels' register budget.
__device__ __forceinline__ uint32_t sat_u32(double f) {  // `as u32`
    if (!(f > 0.0)) return 0u;
    if (f >= 4294967295.0) return 4294967295u;
    return (uint32_t)f;
}
__device__ __attribute__((noinline)) V3 texture_at(const DevScene& S, int tex, int node, V3 p) {
    const double PI = 3.141592653589793;
    double u = 0.0, v = 0.0;
    const DevNode& nd = S.nodes[node];
    switch (nd.kind) {
        case RR_SPHERE: {
            double theta = atan2(p.z, p.x);
            double phi = acos(p.y / sqrt(p.x * p.x + p.y * p.y + p.z * p.z));
            u = (theta + PI) / (2.0 * PI);
            v = 1.0 - (phi / PI);
            break;
        }
        case RR_PLANE:
            u = fmod(p.x, 1.0);
            v = fmod(p.z, 1.0);
            if (u < 0.0) u = 1.0 + u;
            if (v < 0.0) v = 1.0 + v;
            break;
        case RR_CUBE: {
            double ax = fabs(p.x), ay = fabs(p.y), az = fabs(p.z);
            if (ax >= ay && ax >= az) {
                u = p.x > 0.0 ? (p.z + 1.0) * 0.5 : (1.0 - p.z) * 0.5;
                v = (p.y + 1.0) * 0.5;
            } else if (ay >= ax && ay >= az) {
                u = (p.x + 1.0) * 0.5;
                v = p.y > 0.0 ? (1.0 - p.z) * 0.5 : (p.z + 1.0) * 0.5;
            } else {
                u = p.z > 0.0 ? (p.x + 1.0) * 0.5 : (1.0 - p.x) * 0.5;
                v = (p.y + 1.0) * 0.5;
            }
            break;
        }
        case RR_CYLINDER: {
            const DevShape sh = S.shapes[nd.aux];
            if (sh.closed && (p.y <= sh.minimum || p.y >= sh.maximum)) {
                u = (p.x + 1.0) / 2.0;
                v = (p.z + 1.0) / 2.0;
            } else {
                u = (atan2(p.z, p.x) + PI) / (2.0 * PI);
                v = fmod(p.y, 1.0);
                if (v < 0.0) v = 1.0 + v;
            }
            break;
        }
        case RR_CONE: {
            const DevShape sh = S.shapes[nd.aux];
            double dmin = fabs(p.y - sh.minimum), dmax = fabs(p.y - sh.maximum);
            if (sh.closed && (dmin <= RR_EPS || dmax <= RR_EPS)) {
                double radius = fabs(p.y);
                u = (p.x / radius + 1.0) / 2.0;
                v = (p.z / radius + 1.0) / 2.0;
            } else {
                v = (atan2(p.z, p.x) + PI) / (2.0 * PI);
                u = (p.y - sh.minimum) / (sh.maximum - sh.minimum);
            }
            break;
        }
        case RR_TORUS: {  // torus.rs:150-161
            u = (atan2(p.y, p.x) + PI) / (2.0 * PI);
            const double dist_to_center = sqrt(p.x * p.x + p.y * p.y) - 1.0;
            v = (atan2(p.z, dist_to_center) + PI) / (2.0 * PI);
            break;
        }
        case RR_TRIANGLE:
        case RR_SMOOTH_TRIANGLE: {
            const DevTri& T = S.tris[nd.aux];
            V3 v0 = mk(T.e1[0], T.e1[1], T.e1[2]), v1 = mk(T.e2[0], T.e2[1], T.e2[2]);
            V3 v2 = mk(p.x - T.p1[0], p.y - T.p1[1], p.z - T.p1[2]);
            double d00 = dot3(v0, v0) + 0.0, d01 = dot3(v0, v1) + 0.0, d11 = dot3(v1, v1) + 0.0;  // + w*w (= +0)
            double d20 = dot3(v2, v0) + 0.0, d21 = dot3(v2, v1) + 0.0;
            double denom = d00 * d11 - d01 * d01;
            u = (d11 * d20 - d01 * d21) / denom;
            v = (d00 * d21 - d01 * d20) / denom;
            break;
        }
        default:
            break;
    }
    const DevTexture T = S.textures[tex];
    if (u < 0.0) u = 0.0;  // f64::clamp (NaN passes through)
    if (u > 1.0) u = 1.0;
    if (v < 0.0) v = 0.0;
    if (v > 1.0) v = 1.0;
    uint32_t x = min(sat_u32(u * (double)T.width), T.width - 1u);
    uint32_t y = min(sat_u32(v * (double)T.height), T.height - 1u);
    y = T.height - y - 1u;
    uint32_t px = S.texels[T.offset + (uint64_t)y * T.width + x];
    return mk((double)(px & 255u) / 255.0, (double)((px >> 8) & 255u) / 255.0, (double)((px >> 16) & 255u) / 255.0);
}

// Pattern::pattern_at (pattern.rs:145-215) for trees with Gradient/Blend/Perturbed/Noise nodes:
// explicit stack (post-order); its arrays live in scratch, touched only by such scenes.
__device__ __attribute__((noinline)) V3 pattern_tree(const DevScene& S, int root, V3 p, int node) {
    int tn[2 * RR_MAX_PATTERN_DEPTH + 2];
    int tph[2 * RR_MAX_PATTERN_DEPTH + 2];
    V3 tp[2 * RR_MAX_PATTERN_DEPTH + 2];
    V3 vs[2 * RR_MAX_PATTERN_DEPTH + 2];
    double tf[2 * RR_MAX_PATTERN_DEPTH + 2];
    int ts = 0, vn = 0;
    tn[0] = root;
    tph[0] = 0;
    tp[0] = p;
    ts = 1;
    while (ts > 0) {
        --ts;
        int ni = tn[ts];
        int ph = tph[ts];
        V3 q = tp[ts];
        DevPattern P = S.pats[ni];
        if (ph == 2) {  // Noise: scale the selected sub-pattern's colour (pattern.rs:204-207)
            V3 v = vs[--vn];
            vs[vn++] = vmul(v, tf[ts]);
            continue;
        }
        if (ph == 1) {  // combine a, b (already evaluated)
            V3 b = vs[--vn];
            V3 a = vs[--vn];
            if (P.kind == RR_PAT_GRADIENT) {
                V3 dist = vsub(b, a);
                double fraction = q.x - floor(q.x);
                vs[vn++] = vadd(a, vmul(dist, fraction));
            } else {  // Blend
                vs[vn++] = vadd(vmul(a, 1.0 - P.scale), vmul(b, P.scale));
            }
            continue;
        }
        if (P.kind == RR_PAT_SOLID) {  // its own transform does not affect the colour
            vs[vn++] = mk(P.color[0], P.color[1], P.color[2]);
            continue;
        }
        V3 pp = (P.flags & NF_IDENT) ? q : xf_point(P.inv, q);
        switch (P.kind) {
            case RR_PAT_TEST: vs[vn++] = pp; break;
            case RR_PAT_TEXTURE: vs[vn++] = texture_at(S, P.a, node, pp); break;
            case RR_PAT_STRIPE:
                tn[ts] = (sat_i32(floor(pp.x)) % 2 == 0) ? P.a : P.b;
                tph[ts] = 0;
                tp[ts++] = pp;
                break;
            case RR_PAT_RING:
                tn[ts] = (sat_i32(floor(sqrt(pp.x * pp.x + pp.z * pp.z))) % 2 == 0) ? P.a : P.b;
                tph[ts] = 0;
                tp[ts++] = pp;
                break;
            case RR_PAT_CHECKER:
                tn[ts] = (sat_i32(floor(pp.x) + floor(pp.y) + floor(pp.z)) % 2 == 0) ? P.a : P.b;
                tph[ts] = 0;
                tp[ts++] = pp;
                break;
            case RR_PAT_PERTURBED: {  // pattern.rs:187-199
                double nx = octave_perlin(pp.x, pp.y, pp.z, P.octaves, P.persistence) * P.scale;
                double ny = octave_perlin(pp.x, pp.y, pp.z + 1.0, P.octaves, P.persistence) * P.scale;
                double nz = octave_perlin(pp.x, pp.y, pp.z + 2.0, P.octaves, P.persistence) * P.scale;
                tn[ts] = P.a;
                tph[ts] = 0;
                tp[ts++] = mk(pp.x + nx, pp.y + ny, pp.z + nz);
                break;
            }
            case RR_PAT_NOISE: {  // pattern.rs:200-208
                double n = octave_perlin(pp.x, pp.y, pp.z, P.octaves, P.persistence) * P.scale;
                tn[ts] = ni;
                tph[ts] = 2;
                tf[ts] = n <= 0.0 ? -n : n;
                tp[ts++] = pp;
                tn[ts] = n <= 0.0 ? P.a : P.b;
                tph[ts] = 0;
                tp[ts++] = pp;
                break;
            }
            default:  // Gradient / Blend: evaluate a then b, then combine
                tn[ts] = ni;
                tph[ts] = 1;
                tp[ts++] = pp;
                tn[ts] = P.b;
                tph[ts] = 0;
                tp[ts++] = pp;
                tn[ts] = P.a;
                tph[ts] = 0;
                tp[ts++] = pp;
                break;
        }
    }
    return vs[0];
}

// Pattern::pattern_at (pattern.rs:145-215): Stripe / Ring / Checker select one child, so chains of
// them (down to Solid or Test) need no stack; a Gradient / Blend / Perturbed / Noise / Texture
// subtree goes to pattern_tree (out of line, so none of it weighs on the shading kernels' registers).
template <bool CP>
__device__ __forceinline__ V3 pattern_at(const DevScene& S, int root, V3 p, int node) {
    if (root < 0) return mk(1.0, 1.0, 1.0);  // Material::default pattern: solid white
    int ni = root;
    bool tree = false;
#pragma unroll 1
    for (int lvl = 0; lvl <= RR_MAX_PATTERN_DEPTH; ++lvl) {
        const DevPattern& P = S.pats[ni];
        const int kind = P.kind;
        if (kind == RR_PAT_SOLID) return mk(P.color[0], P.color[1], P.color[2]);
        if (kind == RR_PAT_GRADIENT || kind == RR_PAT_BLEND || kind >= RR_PAT_PERTURBED) {
            tree = true;
            break;
        }
        V3 pp = (P.flags & NF_IDENT) ? p : xf_point(P.inv, p);
        if (kind == RR_PAT_TEST) return pp;
        bool even;
        if (kind == RR_PAT_STRIPE) {
            even = sat_i32(floor(pp.x)) % 2 == 0;
        } else if (kind == RR_PAT_RING) {
            even = sat_i32(floor(sqrt(pp.x * pp.x + pp.z * pp.z))) % 2 == 0;
        } else {  // checker
            even = sat_i32(floor(pp.x) + floor(pp.y) + floor(pp.z)) % 2 == 0;
        }
        if (P.flags & (even ? PF_A_SOLID : PF_B_SOLID))
            return even ? mk(P.ca[0], P.ca[1], P.ca[2]) : mk(P.cb[0], P.cb[1], P.cb[2]);
        ni = even ? P.a : P.b;
        p = pp;
    }
    if (CP && tree) return pattern_tree(S, ni, p, node);
    return mk(0.0, 0.0, 0.0);  // unreachable: flatten_scene bounds the nesting depth
}

// Material::pattern_at_object's colour with the root inlined in the material record (DevMaterial.root)
template <bool CP>
__device__ __forceinline__ V3 material_color(const DevScene& S, const DevMaterial& m, int node, V3 over) {
    if (m.root == 1) return mk(m.color[0], m.color[1], m.color[2]);
    return pattern_at<CP>(S, m.pattern, world_to_object(S, node, over), node);  // material.rs:77-80
}

struct Comps {
    V3 point, eyev, normalv, over, under, reflectv;
    double n1, n2;
    bool own_ok;  // NF_OWN_SAFE node hit from outside: its shadow rays may skip it (own_node)
    bool inside;  // Computations.inside (intersection.rs:57-60); read by hit_kernel only
};

// a plane's record in the table behind the node records (rr_device.hpp DevScene.nodes): its world normal, which
// depends on the node alone, and [3] != 0 when normal_to_world(nd, (0, 1, 0)) returns exactly these bits here
// (flat_normal.hpp: the host evaluates this file's sequence next to the reference's)
__device__ __forceinline__ const double* flat_normal_of(const DevScene& S, int node) {
    return reinterpret_cast<const double*>(S.nodes + S.n_nodes) + 4 * (int64_t)node;
}
// Intersection::prepare_computations (intersection.rs:50-60)
__device__ __forceinline__ void prepare(const DevScene& S, const Ray& r, const Hit& h, Comps& c) {
    c.point = vadd(r.o, vmul(r.d, h.t));
    c.eyev = vneg(r.d);
    DevNode nd = S.nodes[h.node];
    V3 lp = world_to_object(S, nd, c.point);
    V3 ln;
    if (nd.kind == RR_SPHERE) {
        ln = lp;  // local_point - point(0,0,0)
    } else if (nd.kind == RR_PLANE) {
        ln = mk(0.0, 1.0, 0.0);
    } else if (nd.kind == RR_CUBE) {  // cube.rs:81-90
        const double ax = fabs(lp.x), ay = fabs(lp.y), az = fabs(lp.z);
        const double maxc = fmax(fmax(ax, ay), az);
        ln = maxc == ax ? mk(lp.x, 0.0, 0.0) : maxc == ay ? mk(0.0, lp.y, 0.0) : mk(0.0, 0.0, lp.z);
    } else if (nd.kind == RR_TORUS) {  // torus.rs:97-107 (normalized here, and again by normal_at)
        const double mr = S.shapes[nd.aux].minimum;
        const double sum_squared = lp.x * lp.x + lp.y * lp.y + lp.z * lp.z;
        const double param_squared = 1.0 + mr * mr;
        ln = normalize3(mk(4.0 * lp.x * (sum_squared - param_squared), 4.0 * lp.y * (sum_squared - param_squared),
                           4.0 * lp.z * (sum_squared - param_squared + 2.0)));
    } else if (nd.kind == RR_CYLINDER || nd.kind == RR_CONE) {  // cylinder.rs:113-124, cone.rs:137-155
        const DevShape P = S.shapes[nd.aux];
        const double dist = lp.x * lp.x + lp.z * lp.z;
        if (dist < 1.0 && lp.y >= P.maximum - RR_EPS) {
            ln = mk(0.0, 1.0, 0.0);
        } else if (dist < 1.0 && lp.y <= P.minimum + RR_EPS) {
            ln = mk(0.0, -1.0, 0.0);
        } else if (nd.kind == RR_CYLINDER) {
            ln = mk(lp.x, 0.0, lp.z);
        } else {
            double y = sqrt(dist);
            if (lp.y > 0.0) y = -y;
            ln = mk(lp.x, y, lp.z);
        }
    } else {
        DevTri T = S.tris[nd.aux];
        if (T.smooth) {  // n2*u + n3*v + n1*(1-u-v)
            double w = 1.0 - h.u - h.v;
            V3 a = vmul(mk(T.n2[0], T.n2[1], T.n2[2]), h.u);
            V3 b = vmul(mk(T.n3[0], T.n3[1], T.n3[2]), h.v);
            V3 cc = vmul(mk(T.n1[0], T.n1[1], T.n1[2]), w);
            ln = vadd(vadd(a, b), cc);
        } else {
            ln = mk(T.normal[0], T.normal[1], T.normal[2]);
        }
    }
    V3 nrm = normal_to_world(S, nd, ln);
    bool inside = dot3(nrm, c.eyev) < 0.0;
    c.inside = inside;
    c.normalv = inside ? vneg(nrm) : nrm;
    c.over = vadd(c.point, vmul(c.normalv, RR_EPS));
    c.under = vsub(c.point, vmul(c.normalv, RR_EPS));
    c.reflectv = reflect3(r.d, c.normalv);
    c.n1 = 1.0;
    c.n2 = 1.0;
    // the hit's T = t |d|_inf within the node's limit (mark_own_safe: the hit point's own rounding)
    c.own_ok = !inside && (nd.flags & NF_OWN_SAFE) &&
               h.t * fmax(fmax(fabs(r.d.x), fabs(r.d.y)), fabs(r.d.z)) <= (double)__int_as_float(nd.aux);
}

// Hit-uniform tiles (shade_body.inc, the flat fused kernels): all 64 lanes of the wave hit node `node`, a top-level
// plane (uniform_hit_node; one-sphere tiles measured no separable gain and keep the per-lane code, DESIGN.md §4,
// tools/patches/uniform_hit_sphere_tiles.patch) whose table entry has the bits this file's normal_to_world gives, so
// its record, its material and the material's root pattern are read through the constant address space with a uniform index: scalar loads, the records in SGPRs and every kind / flag dispatch
// a scalar branch, where prepare / material_color gather the same record once per lane.  Per lane the arithmetic is
// prepare's, material_color's and pattern_at's: the same operations in the same order on the same operands.
__device__ __forceinline__ bool uniform_hit_node(const DevScene& S, int node) {
    cptr<DevNode> nd = cp(S.nodes) + node;
    const int kind = nd->kind;
    return kind == RR_PLANE && nd->parent < 0 && cp(flat_normal_of(S, node))[3] != 0.0;
}
// world_to_object of a top-level node
__device__ __forceinline__ V3 world_to_object_uniform(cptr<DevNode> nd, V3 p) {
    const int flags = nd->flags;
    if (flags & NF_IDENT) return p;
    if (flags & NF_DIAG) return {nd->inv[0] * p.x + nd->inv[3], nd->inv[5] * p.y + nd->inv[7], nd->inv[10] * p.z + nd->inv[11]};
    return xf_point(nd->inv, p);
}
__device__ __forceinline__ void prepare_uniform(const DevScene& S, const Ray& r, const Hit& h, int node, Comps& c) {
    cptr<DevNode> nd = cp(S.nodes) + node;
    c.point = vadd(r.o, vmul(r.d, h.t));
    c.eyev = vneg(r.d);
    const int flags = nd->flags;
    cptr<double> fn = cp(flat_normal_of(S, node));  // normal_to_world(nd, (0, 1, 0)), from the table
    const V3 nrm = mk(fn[0], fn[1], fn[2]);
    const bool inside = dot3(nrm, c.eyev) < 0.0;
    c.inside = inside;
    c.normalv = inside ? vneg(nrm) : nrm;
    c.over = vadd(c.point, vmul(c.normalv, RR_EPS));
    c.under = vsub(c.point, vmul(c.normalv, RR_EPS));
    c.reflectv = reflect3(r.d, c.normalv);
    c.n1 = 1.0;
    c.n2 = 1.0;
    c.own_ok = !inside && (flags & NF_OWN_SAFE) &&
               h.t * fmax(fmax(fabs(r.d.x), fabs(r.d.y)), fabs(r.d.z)) <= (double)__int_as_float(nd->aux);
}
// prepare of one lane of a UH kernel's tile: a hit-uniform tile reads the node through scalar loads, any other tile
// takes prepare.  UH false: prepare, as every other kernel calls it.  (A plane lane of a mixed tile reading its normal
// from the table too measured no gain on C2, DESIGN.md §4, and is not built.)
template <bool UH>
__device__ __forceinline__ void prepare_tile(const DevScene& S, const Ray& r, const Hit& h, Comps& c, bool uni, int unode) {
    if constexpr (UH) {
        if (uni) {
            prepare_uniform(S, r, h, unode, c);
            return;
        }
    }
    prepare(S, r, h, c);
}
// the material record light_terms reads: on a hit-uniform tile its four fields from scalar loads
template <bool UH>
__device__ __forceinline__ DevMaterial tile_material(const DevScene& S, int mat, bool uni, int umat) {
    if constexpr (UH) {
        if (uni) {
            cptr<DevMaterial> sm = cp(S.mats) + umat;
            DevMaterial m;
            m.ambient = sm->ambient;
            m.diffuse = sm->diffuse;
            m.specular = sm->specular;
            m.shininess = sm->shininess;
            return m;
        }
    }
    return S.mats[mat];
}
// material_color for material `mat` of node `node`.  A Stripe / Ring / Checker root whose two children are inline
// Solids ends here; any other chain goes on per lane, through pattern_at from the root (the same value).
template <bool CP>
__device__ __forceinline__ V3 material_color_uniform(const DevScene& S, int mat, int node, V3 over) {
    cptr<DevMaterial> m = cp(S.mats) + mat;
    if (m->root == 1) return mk(m->color[0], m->color[1], m->color[2]);
    const int root = m->pattern;
    const V3 p = world_to_object_uniform(cp(S.nodes) + node, over);
    if (root < 0) return mk(1.0, 1.0, 1.0);
    cptr<DevPattern> P = cp(S.pats) + root;
    const int kind = P->kind, pf = P->flags;
    if (kind == RR_PAT_SOLID) return mk(P->color[0], P->color[1], P->color[2]);
    if ((kind == RR_PAT_STRIPE || kind == RR_PAT_RING || kind == RR_PAT_CHECKER) && (pf & PF_A_SOLID) && (pf & PF_B_SOLID)) {
        const V3 pp = (pf & NF_IDENT) ? p : xf_point(P->inv, p);
        bool even;
        if (kind == RR_PAT_STRIPE) {
            even = sat_i32(floor(pp.x)) % 2 == 0;
        } else if (kind == RR_PAT_RING) {
            even = sat_i32(floor(sqrt(pp.x * pp.x + pp.z * pp.z))) % 2 == 0;
        } else {
            even = sat_i32(floor(pp.x) + floor(pp.y) + floor(pp.z)) % 2 == 0;
        }
        return even ? mk(P->ca[0], P->ca[1], P->ca[2]) : mk(P->cb[0], P->cb[1], P->cb[2]);
    }
    return pattern_at<CP>(S, root, p, node);
}
template <bool UH, bool CP>
__device__ __forceinline__ V3 tile_color(const DevScene& S, const DevMaterial& m, int node, V3 over, bool uni, int umat) {
    if constexpr (UH) {
        if (uni) return material_color_uniform<CP>(S, umat, uniform(node), over);
    }
    return material_color<CP>(S, m, node, over);
}

// The hit node a lane's shadow rays toward a light may skip, or -1.  A convex leaf (sphere, plane) hit from outside
// (not `inside`: the over point lies on the outer side of the tangent plane at the hit point, EPS along the normal)
// cannot hold an entry with 0 <= t < distance on a ray whose direction d has d . normalv >= 0: every point
// over + t d, t >= 0, stays at least EPS beyond that tangent plane, which the convex object lies behind.  In
// floating point the same holds with orders of magnitude to spare when the object's transform is well conditioned
// and the hit itself was found from near enough (NF_OWN_SAFE and prepare()'s limit on the hit's t |d|: flatten.cpp
// mark_own_safe bounds the rounding of the hit point, the object-space origin, direction and the quadratic by 1e-3
// of the margin for |over| <= 1e5), and a light within 1e6: the computed roots are both negative or absent
// (sphere.rs:64-78), the plane's t negative or absent (plane.rs:51-58).  tests/test_own_skip.py checks the rule
// against the oracle's own entries on the fuzz and benchmark scenes.  Point lights: the caller walks only lanes whose
// diffuse + specular term is non-zero, so d . normalv = lighting's light_dot_normal >= 0 (the same expression,
// light.rs:104-112) or NaN (a degenerate light direction: every entry NaN, none shadows).  Area lights: every corner
// of the light beyond the tangent plane (render_levels.inc area_beyond_tangent).
__device__ __forceinline__ int own_node(const Comps& c, int node) {
    const double m = fmax(fmax(fabs(c.over.x), fabs(c.over.y)), fabs(c.over.z));
    return (c.own_ok && m <= 1e5) ? node : -1;
}
// The reflected ray's closest-hit walk may skip the same object (own = own_node of the hit): its direction reflectv
// leaves the surface, reflectv . normalv >= 1e-6 (|reflectv| ~ 1; a clear margin, so the ray never comes back to the
// tangent plane, at any distance), and over lies beyond the tangent plane: the object's entries on it are all negative
// or absent, which the closest hit ignores (scene.rs:128-136 hit() takes t >= 0).
__device__ __forceinline__ int reflect_own(const Comps& c, int own) {
    return (own >= 0 && dot3(c.reflectv, c.normalv) >= 1e-6) ? own : -1;
}

// lighting (light.rs:98-140) split around the shadow query: light_terms gives the ambient and the
// diffuse + specular terms, light_final = ambient + (diffuse + specular) * (1 - in_shadow) — the
// same operations in the same order, so the shadow walk can run without eyev / normalv / colour
// live.  `color` = pattern_at_object(obj, over_point).
// f64::powf(x, y) (libm pow: correctly rounded but for rare near-halfway cases) for the specular factor.
// For the lanes with 0 < x <= 2^500 and the wave's integer exponent n in [1, 512] (shininess 200 in the
// benchmark scenes): x = m 2^e (frexp, m in [0.5, 1)), m^n by squaring in double-double with fma
// (relative error < 2^-98, so the rounded high part is the correctly rounded m^n but for inputs within
// 2^-98 of a rounding midpoint), scaled by 2^(e n) (exact unless the result is subnormal, < 2.2e-308).
// ~65 vector instructions instead of OCML's ~200, and closer to libm (OCML pow is within 1 ulp).
// Other lanes take OCML pow.
__device__ __forceinline__ void dd_mul(double& ah, double& al, double bh, double bl) {
    const double p = ah * bh;
    double e = __builtin_fma(ah, bh, -p);
    e = __builtin_fma(ah, bl, e);
    e = __builtin_fma(al, bh, e);
    const double s = p + e;
    al = e - (s - p);
    ah = s;
}
__device__ __forceinline__ void dd_sqr(double& ah, double& al) {
    const double p = ah * ah;
    double e = __builtin_fma(ah, ah, -p);
    e = __builtin_fma(ah + ah, al, e);
    const double s = p + e;
    al = e - (s - p);
    ah = s;
}
__device__ __forceinline__ double pow_int_dd(double x, int n0) {  // x in (0, 2^500], n0 in [1, 512] wave-uniform
    int e;
    const double m = frexp(x, &e);
    double rh = 1.0, rl = 0.0, bh = m, bl = 0.0;
    bool first = true;
    for (int k = n0;;) {  // wave-uniform exponent: scalar control
        // the first factor is a copy: dd_mul(1, 0, bh, bl) gives (bh, bl) up to the sign of a zero low part, which
        // never reaches a high part (every high part is p + e with p != 0)
        if (k & 1) {
            if (first) {
                rh = bh;
                rl = bl;
                first = false;
            } else {
                dd_mul(rh, rl, bh, bl);
            }
        }
        k >>= 1;
        if (k == 0) break;
        dd_sqr(bh, bl);
    }
    return ldexp(rh, e * n0);
}
__device__ __forceinline__ double pow_shininess(double x, double y) {
    const int n0 = __builtin_amdgcn_readfirstlane((int)fmin(fmax(y, 0.0), 1024.0));
    const bool fast = x > 0.0 && x <= 0x1p500 && y == (double)n0 && n0 >= 1 && n0 <= 512;
    if (__ballot(!fast) == 0) return pow_int_dd(x, n0);
    // a lane outside the fast domain (a NaN or infinite x beside ordinary lanes: the NaN normal at a cone's apex)
    // takes OCML pow by itself; the other lanes of its wave keep the correctly rounded power
    const double p = pow(x, y);
    if (__ballot(fast) == 0) return p;
    const double r = pow_int_dd(fast ? x : 1.0, n0);
    return fast ? r : p;
}

// dir_out (optional, LDS [4][256] doubles at this thread): normalize(light - point) and |light - point| — is_shadowed's
// direction and distance when point is the over_point (scene.rs:235-237: the same operations), stored as soon as
// they exist so that they hold no registers through the `pow` below
template <bool TINY = true>
__device__ __forceinline__ void light_terms(const DevMaterial& m, const DevLight& L, V3 color, V3 point, V3 eyev,
                                            V3 normalv, V3& ambient, V3& dspec, double* dir_out = nullptr) {
    V3 I = mk(L.intensity[0], L.intensity[1], L.intensity[2]);
    V3 eff = vprod(color, I);
    const V3 tl = vsub(mk(L.position[0], L.position[1], L.position[2]), point);
    const double mag = sqrt(dot3(tl, tl));
    V3 lightv = div3(tl, mag);  // normalize3 (tuple.rs:95-98)
    if (dir_out) {
        dir_out[0] = lightv.x;
        dir_out[256] = lightv.y;
        dir_out[512] = lightv.z;
        dir_out[768] = mag;
    }
    ambient = vmul(eff, m.ambient);
    double ldn = dot3(lightv, normalv);
    V3 diffuse = mk(0, 0, 0), specular = mk(0, 0, 0);
    if (!(ldn < 0.0)) {
        diffuse = vmul(vmul(eff, m.diffuse), ldn);
        V3 reflectv = reflect3(vneg(lightv), normalv);
        double rde = dot3(reflectv, eyev);
        if (!(rde <= 0.0)) {
            // specular == 0: (I * 0) * factor with factor = rde^shininess finite and >= 0 (0 < rde <= 1 + a few
            // ulps, 0 <= shininess <= 1e6) is exactly I * specular, signed zeros included — a wave whose lanes
            // all have specular-free materials skips the pow
            const bool free_spec = m.specular == 0.0 && m.shininess >= 0.0 && m.shininess <= 1e6;
            // tiny specular (TINY): shininess * log2(rde) <= -71 in f32 (rde >= 2^-100 and shininess <= 1e4 keep the
            // f32 log's error under 0.2 of the 1-unit margin) bounds the factor rde^shininess by 2^-70 (pow is within an
            // ulp), so each channel of (I * specular) * factor is below (|Ix| + |Iy| + |Iz|) |specular| 2^-69.9 <
            // |diffuse_c| 2^-54.9: under half an ulp of diffuse_c, so diffuse + specular rounds to diffuse exactly
            // (light.rs:138) and the lane needs no pow.  Written so that a NaN anywhere keeps the pow.  Lit sphere lanes
            // away from the highlight (reflect . eye below ~0.78 at shininess 200) qualify, so most waves skip the pow
            const double dlim = (fabs(I.x) + fabs(I.y) + fabs(I.z)) * fabs(m.specular) * 0x1p-15;
            const float rf = (float)rde;
            const bool tiny = TINY && rf >= 0x1p-100f && m.shininess <= 1e4 &&
                              (float)m.shininess * __builtin_amdgcn_logf(rf) <= -71.0f && dlim < fabs(diffuse.x) &&
                              dlim < fabs(diffuse.y) && dlim < fabs(diffuse.z);
            const bool need = !free_spec && !tiny;
            // factor 1 for specular-free lanes ((I * 0) * 1 = I * 0), 0 for tiny ones ((I * specular) * 0 = +-0, I *
            // specular finite: diffuse + +-0 = diffuse, diffuse != 0)
            double factor = 1.0;
            if (__ballot(need) != 0) factor = pow_shininess(need ? rde : 1.0, m.shininess);
            if constexpr (TINY)
                specular = vmul(vmul(I, m.specular), need ? factor : free_spec ? 1.0 : 0.0);
            else
                specular = need ? vmul(vmul(I, m.specular), factor) : vmul(I, m.specular);
        }
    }
    dspec = vadd(diffuse, specular);
}
__device__ __forceinline__ V3 light_final(V3 ambient, V3 dspec, double in_shadow) {
    return vadd(ambient, vmul(dspec, 1.0 - in_shadow));
}
__device__ __forceinline__ V3 lighting(const DevMaterial& m, const DevLight& L, V3 color, V3 point, V3 eyev,
                                       V3 normalv, double in_shadow) {
    V3 a, ds;
    light_terms(m, L, color, point, eyev, normalv, a, ds);
    return light_final(a, ds, in_shadow);
}

// Computations::schlick (computations.rs:39-54)
__device__ __forceinline__ double schlick(const Comps& c) {
    double cs = dot3(c.eyev, c.normalv);
    if (c.n1 > c.n2) {
        double n = c.n1 / c.n2;
        double sin2_t = n * n * (1.0 - cs * cs);
        if (sin2_t > 1.0) return 1.0;
        cs = sqrt(1.0 - sin2_t);
    }
    double q = (c.n1 - c.n2) / (c.n1 + c.n2);
    double r0 = q * q;
    double m = 1.0 - cs;
    double m2 = m * m;
    double m5 = m * (m2 * m2);  // powi(5)
    return r0 + (1.0 - r0) * m5;
}


}  // namespace rr
