// render_levels.inc — the per-level kernels (trace, n1n2, fused shade) and their launch template
// launch_level_t<G, LC>.  Each render_levels_g<G>_<lds|gl>.hip instantiates one (G, LC) pair, so the
// kernel variants compile in parallel translation units.  Included inside namespace rr, after
// render_common.inc.
template <int G, bool LC, bool RM>
__global__ void __launch_bounds__(256) trace_kernel(DevScene S, LevelArgs A) {
    load_prologue_args(A);
    const int64_t n_live = live_count(A);
    if ((int64_t)blockIdx.x * RR_BLOCK >= n_live) return;
    zero_next_counters(A);
    if (LC) stage_culls(S);
    const int64_t i = (int64_t)blockIdx.x * RR_BLOCK + threadIdx.x;
    const bool valid = i < n_live;
    Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    Ray r = valid ? event_ray<true>(A, i) : Ray{mk(0, 0, 0), mk(0, 0, 1)};
    Hit h;
    trace_closest<G, LC, RM, cross_lane_ok(G, false, false)>(S, r, valid, h, cnt, cam_tile(A), cam_bundle_of(A));
    cnt.rays += popc_ballot(valid);
    if (valid) {
        HitRec hr;
        hr.t = h.t;
        hr.u = h.u;
        hr.v = h.v;
        hr.node = h.found ? h.node : -1;
        hr.k = h.k;
        A.hit[i] = hr;
    }
    bool want = false;
    if (S.has_transparent && valid && h.found) {
        DevMaterial m = S.mats[S.nodes[h.node].material];
        want = needs_n1n2(m, A.rem);
    }
    if (S.has_transparent) {  // uniform: the whole block appends
        unsigned int* const ctr[1] = {A.lcount + LC_N1N2};
        const bool wq[1] = {want};
        int32_t slot[1];
        block_append<1>(ctr, wq, slot);
        if (want) A.n1n2_list[slot[0]] = (int32_t)i;
    }
    flush(cnt, A.counters, W_TRACE);
}

template <int G, bool LC, bool RM>
__global__ void __launch_bounds__(256) n1n2_kernel(DevScene S, LevelArgs A) {
    const int64_t cnt_n = (int64_t)A.lcount[LC_N1N2];
    if ((int64_t)blockIdx.x * RR_BLOCK >= cnt_n) return;
    if (LC) stage_culls(S);
    const int64_t j = (int64_t)blockIdx.x * RR_BLOCK + threadIdx.x;
    const bool valid = j < cnt_n;
    Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int64_t i = valid ? A.n1n2_list[j] : 0;
    Ray r = valid ? event_ray<false>(A, i) : Ray{mk(0, 0, 0), mk(0, 0, 1)};
    Hit h;
    h.found = valid;
    h.t = 0.0;
    h.node = -1;
    h.k = 0;
    h.rank = 0;
    if (valid) {
        HitRec hr = A.hit[i];
        h.t = hr.t;
        h.u = hr.u;
        h.v = hr.v;
        h.node = hr.node;
        h.k = hr.k;
        h.rank = S.nodes[hr.node].rank;
    }
    double n1 = 1.0, n2 = 1.0;
    n1n2_walk<G, LC, RM, cross_lane_ok(G, false, false)>(S, r, h, valid, n1, n2, cnt);
    if (valid) {
        A.n12[2 * i] = n1;
        A.n12[2 * i + 1] = n2;
    }
    flush(cnt, A.counters, W_N1N2);
}


// floor(n / d) for a wave-uniform d >= 1, given rd = 1.0f / d, wherever the quotient is below 2^22 and n + 2 d below
// 2^32: (float)n, rd and their product each round once (relative 2^-24), so the f32 quotient is off by less than
// 3 * 2^-24 * 2^22 < 1, its truncation within one of the true floor, and two integer corrections make it exact.  n itself
// may pass 2^24: area_shadow_block's pairs reach 2^28 with quotients of at most 256 (the block's events) and its cell
// indices 2^20 with quotients below 1024 (tests/test_division.py tries both call sites' whole domain)
__device__ __forceinline__ uint32_t small_div(uint32_t n, uint32_t d, float rd) {
    uint32_t q = (uint32_t)((float)n * rd);
    if (q * d > n) --q;
    if ((q + 1u) * d <= n) ++q;
    return q;
}

// Area-light staging in the shade kernels' dynamic LDS (after the culls and the prelit terms):
// the block's shading events compacted, with their shadowed-sample totals.  8 KB.
struct AreaStage {
    double o[3][256];     // over_point
    uint32_t key[256];    // jitter_base(seed, global sample id, recursion path)
    uint32_t total[256];  // shadowed samples so far
    uint32_t nodes[256];  // the nodes (bit i: node i < 32) the light-hull pre-test could not rule out for the event
};
static_assert(sizeof(AreaStage) == RR_AREA_STAGE_BYTES, "AreaStage layout");

// Whether any of an area light's sample rays from `o` may be shadowed (a conservative pre-test; false = none can).
// Every sample point lies in the light's parallelogram corner + [0,1] u + [0,1] v (the cell offsets
// (col + jitter) / level are in [0, 1)), so every shadow segment from o to a sample lies in the convex hull of o and
// the parallelogram, and that hull lies in the cone {o + t (qc - o) + t e : |e| <= qr, t in [0, 1]} (qc its centre,
// qr half its longer diagonal).  A bounded node whose cull sphere (which holds every point the kernel's exact test
// can report, DESIGN.md §2) keeps min over t of |c - o - t (qc - o)| - t qr (convex in t: evaluated at the clamped
// stationary point) above its radius gives none of the samples a hit at t < distance; a top-level plane gives
// none when o and the four corners lie strictly on one side of it (its object-space y is affine, so the whole
// hull does).  Containers are entered when any lane's cone meets their
// cull; anything else unbounded answers "may".  Margins cover the rounding of the sample points, the segment ends
// and the plane values.  Wave-uniform node loop over scenes of at most RR_AREA_PRETEST_NODES nodes; larger scenes
// always walk.
// With want_bits (scenes walked node by node, at most RR_BUNDLE_MIN_NODES nodes: C5) every node is decided and bit i
// of `bits` says whether node i may shadow some sample; the walks then skip the others' exact tests (C5: the floor
// plane, which no segment from a point above it to the light above it crosses, was half of the exact tests).
constexpr int RR_AREA_PRETEST_NODES = 64;
template <int G, bool LC>
__device__ __forceinline__ bool area_may_shadow(const DevScene& S, const DevLight& Lt, V3 o, bool live, bool want_bits,
                                                uint32_t& bits) {
    const V3 corner = mk(Lt.corner[0], Lt.corner[1], Lt.corner[2]);
    const V3 lu = mk(Lt.u[0], Lt.u[1], Lt.u[2]), lv = mk(Lt.v[0], Lt.v[1], Lt.v[2]);
    const V3 qc = vadd(corner, vadd(vmul(lu, 0.5), vmul(lv, 0.5)));
    const V3 dp = vadd(lu, lv), dm = vsub(lu, lv);
    const double qr = 0.5 * sqrt(fmax(dp.x * dp.x + dp.y * dp.y + dp.z * dp.z, dm.x * dm.x + dm.y * dm.y + dm.z * dm.z));
    const V3 ax = vsub(qc, o);
    const double len2 = ax.x * ax.x + ax.y * ax.y + ax.z * ax.z;
    const double L = sqrt(len2), cone = sqrt(fmax(len2 - qr * qr, 0.0));  // |qc - o|, L cos(half angle)
    const bool narrow = L > 1.001 * qr;  // otherwise o is about as close to the light as it is wide: always walk
    const double scale = fabs(o.x) + fabs(o.y) + fabs(o.z) + fabs(qc.x) + fabs(qc.y) + fabs(qc.z) + qr;
    const double slack = 1e-6 * (1.0 + scale);  // sample-point, segment-end and cull-centre rounding
    bool may = false;
    bits = 0u;
    const int n = uniform(S.n_nodes);
    for (int i = 0; i < n;) {
        if (!want_bits && __ballot(live && !may) == 0) break;  // every lane already walks
        const DevCull cl = LC ? rr_lds_culls[i] : S.culls[i];
        cptr<DevNode> nd = cp(S.nodes) + i;
        const int kind = nd->kind;
        bool pass;
        if (cl.r == INFINITY) {
            if (kind == RR_PLANE && nd->parent < 0) {
                // object-space y (row 1 of the inverse) at o and at the corners: one strict side -> no crossing
                const double* w = nd->inv + 4;
                const auto yv = [&](V3 p) { return w[0] * p.x + w[1] * p.y + w[2] * p.z + w[3]; };
                const auto mg = [&](V3 p) {
                    return 1e-9 * (fabs(w[0] * p.x) + fabs(w[1] * p.y) + fabs(w[2] * p.z) + fabs(w[3])) + 1e-300;
                };
                const V3 c1 = vadd(corner, lu), c2 = vadd(corner, lv), c3 = vadd(c1, lv);
                const double y0 = yv(o), y1 = yv(corner), y2 = yv(c1), y3 = yv(c2), y4 = yv(c3);
                const bool above = y0 > mg(o) && y1 > mg(corner) && y2 > mg(c1) && y3 > mg(c2) && y4 > mg(c3);
                const bool below = y0 < -mg(o) && y1 < -mg(corner) && y2 < -mg(c1) && y3 < -mg(c2) && y4 < -mg(c3);
                pass = !(above || below);
            } else {
                pass = true;  // unbounded otherwise (groups holding planes, open cylinders / cones)
            }
        } else {
            // the cone's distance to the cull centre along t, minimised at the stationary point
            // t* = (p + qr h / (L cos)) / L (p, h: the centre's axial / radial offsets), clamped to [0, 1]
            const V3 wv = vsub(mk(cl.c[0], cl.c[1], cl.c[2]), o);
            const double pa = (wv.x * ax.x + wv.y * ax.y + wv.z * ax.z) / L;
            const double h = sqrt(fmax(wv.x * wv.x + wv.y * wv.y + wv.z * wv.z - pa * pa, 0.0));
            const double t = narrow ? fmin(fmax((pa + qr * h / cone) / L, 0.0), 1.0) : 0.0;
            const V3 dv = vsub(wv, vmul(ax, t));
            pass = !narrow || sqrt(dv.x * dv.x + dv.y * dv.y + dv.z * dv.z) - t * qr <= (double)cl.r + slack;
        }
        if (is_container(kind)) {  // enter the subtree if any deciding lane's cone meets it
            i = __ballot(live && !may && pass) != 0 ? i + 1 : nd->skip;
            continue;
        }
        may = may || pass;
        if (pass && i < 32) bits |= 1u << i;
        ++i;
    }
    if (!want_bits) bits = ~0u;
    return may;
}

// intensity_at for an area light (light.rs:67-96 with sample_point light.rs:47-65): the fraction of
// its level^2 jittered cell samples from which over_point is shadowed, for every shading event of
// the workgroup at once.  The block's (event, sample) pairs are numbered event-major and dealt out
// over its 256 threads, so a wave walks ~64 consecutive pairs — a few origins, each toward the whole
// cell grid of the light (a narrow bundle) — and lanes without a hit hold no work (before, each hit
// lane walked its level^2 rays itself, and the idle lanes of sparse waves waited).  The per-event
// total is an integer (LDS atomics), so the walking order does not matter: the result is the same
// `total as f64 / amount as f64`.  Every thread of the block must call it (block-uniform).
// own_node's skip for an area light: every sample point lies in the light's parallelogram (corner + uf u + vf v, uf and
// vf in [0, 1]), so when all four corners lie beyond the tangent plane at over (margin 1e-6 of the coordinates'
// size, which covers the sample points' rounding) every sample's direction d has d . nrm > 0, and the own object holds
// no shadowing entry on any of the level^2 rays (own_node; its light-distance bound 1e6 checked per corner)
__device__ __forceinline__ bool area_beyond_tangent(const DevLight& Lt, V3 over, V3 nrm) {
    const V3 corner = mk(Lt.corner[0], Lt.corner[1], Lt.corner[2]);
    const V3 lu = mk(Lt.u[0], Lt.u[1], Lt.u[2]), lv = mk(Lt.v[0], Lt.v[1], Lt.v[2]);
    const V3 c1 = vadd(corner, lu), c2 = vadd(corner, lv), c3 = vadd(c1, lv);
    const auto beyond = [&](V3 c) {
        const V3 w = vsub(c, over);
        const double size = fabs(w.x) + fabs(w.y) + fabs(w.z);
        const double scale = size + fabs(over.x) + fabs(over.y) + fabs(over.z) + fabs(c.x) + fabs(c.y) + fabs(c.z);
        return dot3(w, nrm) > 1e-6 * scale && size < 1e6;
    };
    return beyond(corner) && beyond(c1) && beyond(c2) && beyond(c3);
}

// The umbra (node-by-node walks): whether every sample ray of the area light from o certainly has an entry with
// 0 <= t < distance on some node, so the event's level^2 walks would all report shadowed and its total is level^2.
// A node with an inner ball (S.inner: centre C, radius r inside the set its exact test reports) shadows every sample
// point p whose segment from o passes through the ball and ends beyond the node: the line o -> p within r of C
// (|v x w|^2 < r^2 |v|^2, v = p - o, w = C - o) and p past the node's outer bound along w (v . w > |w| (|w| + r_cull)).
// Both conditions hold for the whole parallelogram when they hold at its four corners: the first is a convex cone
// around w, the second a half-space.  The exact test's entry is then in [0, distance): for o outside the node (|w| >
// r) the entry precedes the closest approach, and both roots precede the node's far side, which precedes p.  Margins of
// 1e-6 relative (and |w| <= 1e3 r, which bounds the quadratic's cancellation) keep every rounding — the sample points',
// the directions', the test's own — far inside them.  `bits`: the nodes the pre-test left for the event.
template <bool LC>
__device__ __forceinline__ bool area_in_umbra(const DevScene& S, const DevLight& Lt, V3 o, uint32_t bits) {
    const V3 corner = mk(Lt.corner[0], Lt.corner[1], Lt.corner[2]);
    const V3 lu = mk(Lt.u[0], Lt.u[1], Lt.u[2]), lv = mk(Lt.v[0], Lt.v[1], Lt.v[2]);
    const V3 q[4] = {corner, vadd(corner, lu), vadd(corner, lv), vadd(vadd(corner, lu), lv)};
    const int n = uniform(S.n_nodes) < 32 ? uniform(S.n_nodes) : 32;
    for (int i = 0; i < n; ++i) {
        const DevCull in = ldc(S.inner, i);
        if (!(in.r > 0.0f)) continue;  // wave-uniform: no inner ball
        if (!((bits >> i) & 1u)) continue;
        const double r = (double)in.r, rc = LC ? (double)rr_lds_culls[i].r : (double)S.culls[i].r;
        const V3 w = vsub(mk(in.c[0], in.c[1], in.c[2]), o);
        const double L = sqrt(dot3(w, w));
        if (!(L > r * (1.0 + 1e-6) && L < 1e3 * r)) continue;
        bool all = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const V3 v = vsub(q[k], o);
            const V3 x = cross3(v, w);
            all = all && dot3(x, x) < (r * r) * dot3(v, v) * (1.0 - 1e-6) && dot3(v, w) > L * (L + rc) * (1.0 + 1e-6);
        }
        if (all) return true;
    }
    return false;
}

// own / nrm (node-by-node walks): the event's own_node and its normalv; area_beyond_tangent clears own's node bit
template <int G, bool LC, bool RM>
__device__ double area_shadow_block(const DevScene& S, const LevelArgs& A, const DevLight& Lt, int li, V3 over,
                                    bool has_hit, uint64_t sample, uint32_t path, AreaStage& st, Counters& cnt,
                                    int own = -1, V3 nrm = {0.0, 0.0, 0.0}) {
    __shared__ uint32_t s_wcnt[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // events whose light hull no node can reach skip their level^2 walks (total 0, as the walks would find); in scenes
    // walked node by node the walks also skip the nodes the pre-test ruled out for the event
    constexpr bool NODE_MASK = G == 0 && LC;  // walk_nodes' node-by-node path (n_nodes <= RR_BUNDLE_MIN_NODES)
    const bool per_node = NODE_MASK && S.n_nodes <= RR_BUNDLE_MIN_NODES;
    uint32_t node_bits = ~0u;
    bool may = S.n_nodes > RR_AREA_PRETEST_NODES || area_may_shadow<G, LC>(S, Lt, over, has_hit, per_node, node_bits);
    if (per_node && own >= 0 && own < 32 && area_beyond_tangent(Lt, over, nrm)) {  // per_node: flat, every node a leaf
        node_bits &= ~(1u << own);
        may = node_bits != 0u;
    }
    // the umbra: every sample certainly shadowed — the walks' total would be level^2 (scenes walked node by node)
    const bool umbra = per_node && has_hit && may && area_in_umbra<LC>(S, Lt, over, node_bits);
    const bool walk = has_hit && may && !umbra;
    const uint64_t m = __ballot(walk);
    if (lane == 0) s_wcnt[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t base = 0, nh = 0;
    for (int k = 0; k < 4; ++k) {
        const uint32_t c = s_wcnt[k];
        base += k < w ? c : 0u;
        nh += c;
    }
    const uint64_t below = lane == 0 ? 0ull : ((~0ull) >> (64 - lane));
    const uint32_t mine = base + (uint32_t)__popcll(m & below);
    if (walk) {
        st.o[0][mine] = over.x;
        st.o[1][mine] = over.y;
        st.o[2][mine] = over.z;
        st.key[mine] = A.jitter_mode == 0 ? jitter_base(A.seed, sample, path) : 0u;
        st.total[mine] = 0u;
        st.nodes[mine] = node_bits;
    }
    __syncthreads();
    const uint32_t level = (uint32_t)Lt.level, amount = level * level;
    cnt.shadow += popc_ballot(has_hit && !walk) * amount;  // skipped walks: the reference still casts their rays
    const float r_amount = 1.0f / (float)amount, r_level = 1.0f / (float)level;
    const uint32_t npairs = nh * amount;
    const double dlevel = (double)level, rlevel = 1.0 / dlevel;
    const V3 corner = mk(Lt.corner[0], Lt.corner[1], Lt.corner[2]);
    const V3 lu = mk(Lt.u[0], Lt.u[1], Lt.u[2]), lv = mk(Lt.v[0], Lt.v[1], Lt.v[2]);
    for (uint32_t j0 = (uint32_t)w * 64u; j0 < npairs; j0 += 256u) {  // wave-uniform; no barrier inside
        const uint32_t j = j0 + (uint32_t)lane;
        const bool live = j < npairs;
        const uint32_t h = live ? small_div(j, amount, r_amount) : 0u;
        const uint32_t s = j - h * amount;
        const uint32_t row = small_div(s, level, r_level), col = s - row * level;
        double ur = 0.5, vr = 0.5;
        if (A.jitter_mode == 0) {
            const uint32_t key = st.key[h];
            ur = jitter_value(key, (uint32_t)li, s, 0);
            vr = jitter_value(key, (uint32_t)li, s, 1);
        }
        // ((col + u) / level, (row + v) / level): numerators >= +0 and < 2^21, divisor an integer in
        // [1, 2^10]: div_y's conditions hold, with y = RN(1 / level) computed once per light
        const double uf = div_y((double)col + ur, dlevel, rlevel);
        const double vf = div_y((double)row + vr, dlevel, rlevel);
        const V3 target = vadd(vadd(corner, vmul(lu, uf)), vmul(lv, vf));
        const V3 o = mk(st.o[0][h], st.o[1][h], st.o[2][h]);
        const uint32_t nodes = NODE_MASK ? st.nodes[h] : ~0u;
        if (shadowed<G, LC, RM, false>(S, o, target, live, cnt, nodes) && live) atomicAdd(&st.total[h], 1u);
    }
    __syncthreads();
    const double r = has_hit ? (double)(int)(walk ? st.total[mine] : umbra ? amount : 0u) / (double)(int)amount : 0.0;
    __syncthreads();  // the stage is reused by the next light
    return r;
}

// intensity_at (light.rs:67-96): 1 - in_shadow from is_shadowed toward the light (point) or the
// fraction of its level^2 jittered cell samples that are shadowed (area, light.rs:47-65).
// Block-uniform (the area path synchronises the workgroup).
// AR: the scene has an area light (only those kernels carry the area path: inlined into the others it
// cost the C2 kernel 23 spilled VGPRs).
// `counted` lanes cast the light's shadow ray(s) in the reference; `active` (a subset) walk them.  A lane
// whose diffuse + specular term for this light is exactly zero (the light is behind the surface: ldn < 0,
// light.rs:112-116) gets ambient + (+-0) * (1 - in_shadow) == ambient + (+-0) whatever in_shadow is, so its
// walk is skipped — the rays are still counted, as the reference casts them (scene.rs:181-214).
// pdir (point lights, optional): this lane's normalize(light - over) and its magnitude, parked in LDS by the prelit
// stage ([4][256] doubles: x, y, z, distance) — lighting's lightv is the same expression (light.rs:104 on over_point,
// scene.rs:188) as is_shadowed's direction and distance (scene.rs:235-237), so the walk does not recompute them
// OWN / own: the lane's own_node, skipped by its point-light walk (`active` lanes have a non-zero diffuse + specular
// term, so their shadow direction points out of the surface: see own_node)
template <int G, bool LC, bool RM, bool AR, bool XL, bool OWN = false, bool AWAY = false>
__device__ __forceinline__ double shadow_amount(const DevScene& S, const LevelArgs& A, const DevLight& Lt, int li,
                                                V3 over, bool active, bool counted, uint64_t sample, uint32_t path,
                                                AreaStage* ast, Counters& cnt, const double* pdir = nullptr,
                                                int own = -1, V3 nrm = {0.0, 0.0, 0.0}) {
    if (!AR || Lt.kind == RR_LIGHT_POINT) {
        cnt.shadow += popc_ballot(counted && !active);
        const V3 L = mk(Lt.position[0], Lt.position[1], Lt.position[2]);
        if (pdir)
            return shadowed_dir<G, LC, RM, XL, true, OWN, AWAY>(S, over, mk(pdir[0], pdir[256], pdir[512]), pdir[768], L, active,
                                                           cnt, ~0u, own)
                       ? 1.0
                       : 0.0;
        return shadowed<G, LC, RM, XL, true, OWN, AWAY>(S, over, L, active, cnt, ~0u, own) ? 1.0 : 0.0;
    }
    if constexpr (AR) {
        cnt.shadow += popc_ballot(counted && !active) * (uint32_t)(Lt.level * Lt.level);
        return area_shadow_block<G, LC, RM>(S, A, Lt, li, over, active, sample, path, *ast, cnt, own, nrm);
    }
    return 0.0;
}

// The prelit terms follow the cull records in the walking kernels' dynamic LDS:
// [light][6 doubles][256 threads] (SoA: lanes of a wave read consecutive doubles).
__device__ __forceinline__ double* prelit_lds(const DevScene& S, bool lc) {
    char* base = reinterpret_cast<char*>(rr_lds_culls);
    const size_t off = lc ? (size_t)S.n_nodes * sizeof(DevCull) + (size_t)S.n_chunks * sizeof(DevChunk) : 0;
    return reinterpret_cast<double*>(base + off);
}
// doubles per light and thread in the prelit stage: ambient, diffuse+specular; the shade kernels without area lights
// also park the shadow direction and distance (shadow_amount pdir)
__host__ __device__ constexpr int prelit_per_light(bool area) { return area ? 6 : 10; }
// the area-light stage follows the prelit terms (PRE) or the culls
__device__ __forceinline__ AreaStage* area_lds(const DevScene& S, bool lc, bool pre) {
    char* base = reinterpret_cast<char*>(prelit_lds(S, lc));
    const size_t off = pre ? (size_t)S.n_lights * 6 * 256 * sizeof(double) : 0;
    return reinterpret_cast<AreaStage*>(base + off);
}
// Per-thread shading state parked in LDS (SoA, 9 doubles x 256 threads = 18 KB) while the shadow
// walks run, so the walks do not compete with it for VGPRs: eyev, normalv, pattern colour.
struct ShadeStash {
    double v[9][256];
};
__device__ __forceinline__ void stash_put(ShadeStash& s, V3 eyev, V3 normalv, V3 pcol) {
    const int t = threadIdx.x;
    s.v[0][t] = eyev.x;
    s.v[1][t] = eyev.y;
    s.v[2][t] = eyev.z;
    s.v[3][t] = normalv.x;
    s.v[4][t] = normalv.y;
    s.v[5][t] = normalv.z;
    s.v[6][t] = pcol.x;
    s.v[7][t] = pcol.y;
    s.v[8][t] = pcol.z;
}

// one light of shade_hit's sum: surface += lighting(material, light, colour, over, eyev, normalv,
// intensity_at(light, over)) — the shadow walk first, then the lighting terms from the stash
template <int G, bool LC, bool RM, bool AR, bool XL>
__device__ __forceinline__ void light_step(const DevScene& S, const LevelArgs& A, int li, bool has_hit, int mat,
                                           V3 over, uint64_t sample, uint32_t path, const ShadeStash& st,
                                           AreaStage* ast, V3& surface, Counters& cnt) {
    const DevLight Lt = ldc(S.lights, li);
    const double in_shadow = shadow_amount<G, LC, RM, AR, XL>(S, A, Lt, li, over, has_hit, has_hit, sample, path, ast, cnt);
    if (has_hit) {
        const int t = threadIdx.x;
        const V3 eyev = mk(st.v[0][t], st.v[1][t], st.v[2][t]);
        const V3 normalv = mk(st.v[3][t], st.v[4][t], st.v[5][t]);
        const V3 pcol = mk(st.v[6][t], st.v[7][t], st.v[8][t]);
        surface = vadd(surface, lighting(S.mats[mat], Lt, pcol, over, eyev, normalv, in_shadow));
    }
}

// Fused shade_hit for every event of the level (scene.rs:159-177):
//   prepare_computations + pattern (intersection.rs:50-60, material.rs:77-80), the children rays
//   (reflected_color scene.rs:281-290, refracted_color scene.rs:310-336) appended to level d+1,
//   then surface = 0 + lighting(L0, intensity_at(L0)) + ... with every is_shadowed walk
//   (scene.rs:181-214, 234-245; area lights sample level^2 jittered points, light.rs:47-65).
// The 64 lanes of a wave walk their shadow rays for the same light sample together, so the walk's
// ray bundle stays tight.  Events without children are finished here (deliver); events with
// children store their pending sum and are finished by combine_kernel after their children.
// FUSED (scenes without transparency, where no n1/n2 walk sits between trace and shade): the
// kernel first runs the closest-hit walk itself, so the hit and the ray stay in registers.
// PRE (scenes with <= RR_PRELIT_LIGHTS lights): every light's ambient and diffuse+specular terms
// (the `pow`-heavy part of lighting) are computed right after prepare_computations and parked in
// LDS, so the shadow walks run with only the walk state live; otherwise eyev / normalv / colour
// are parked and lighting runs after each walk.
// The prelit variant is held to 4 waves/SIMD (<= 128 VGPRs, measured faster than 3 waves: C2 0.258 vs
// 0.288 ms/frame when it was introduced).  The general variant (G = 2) is not held to 4 waves: squeezed into
// 128 VGPRs it spills ~300 registers (2 % slower on example1), and spilled cross-lane walks are unsafe
// (DESIGN.md §3.6).  Group (G = 1) kernels run at 3 waves/SIMD, which keeps the far-origin shift spill-free
// (cross-lane walks, build.py check; C4 1.44 -> 1.00 ms with both).
#ifdef RR_G1_WAVES_EXP  // experiment builds (build.py variant) only
constexpr int RR_PRE_WAVES = 4, RR_RM_WAVES = 4, RR_G2_WAVES = 2, RR_G1_WAVES = RR_G1_WAVES_EXP;
#else
constexpr int RR_PRE_WAVES = 4, RR_RM_WAVES = 4, RR_G2_WAVES = 2, RR_G1_WAVES = 3;
#endif
#define RR_SHADE_ATTR(PRE, G, RM)                                                                     \
    __attribute__((amdgpu_waves_per_eu(                                                                \
        ((PRE) && (G) < 2) ? ((RM) && (G) == 0 ? RR_RM_WAVES : (G) == 1 ? RR_G1_WAVES : RR_PRE_WAVES)   \
                           : (G) == 2 ? RR_G2_WAVES : 2)))
// CP: the scene has Gradient / Blend / Perturbed / Noise / Texture patterns, evaluated by the
// out-of-line pattern_tree.  Without CP the kernel carries no call at all: the call graph's register
// demand (atan2 / acos / Perlin in the callee) otherwise costs the common scenes their occupancy.
template <int G, bool LC, bool FUSED, bool PRE, bool CP, bool RM, bool AR>
__global__ void __launch_bounds__(256) RR_SHADE_ATTR(PRE, G, RM) shade_kernel(DevScene S, LevelArgs A) {
    // event index: below 2^31 (rr_render_device caps every level's queue, RR_E_LIMIT), so it is carried in
    // one 32-bit register (a 64-bit index held for the whole kernel cost the group kernels their 4th wave)
    uint32_t iu;
    bool valid;
    // (the camera levels' kernels and the group scenes': C2 -1.7 %, C4 -1 %; the flat scenes' secondary-level
    // and area-light kernels measured slower with it, C3 +0.8 %, C5 +3 %)
    if constexpr (!AR && (G > 0 || !RM)) load_prologue_args(A);
    if (FUSED && A.nseg > 1) {  // segmented level (wavefront.hpp): block b reads segment b % nseg
        const uint32_t seg = blockIdx.x % (uint32_t)A.nseg, chunk = blockIdx.x / (uint32_t)A.nseg;
        const int64_t cs = (int64_t)A.seg_count[seg];
        if ((int64_t)chunk * 256 >= cs) return;
        const int64_t off = (int64_t)chunk * 256 + threadIdx.x;
        iu = (uint32_t)((int64_t)seg * A.seg_cap + off);
        valid = off < cs;
        if (A.pad_children && valid) valid = A.ev[iu].parent != -2;  // a hole of a padded wave block
    } else {
        const int64_t n_live = live_count(A);
        if ((int64_t)blockIdx.x * RR_BLOCK >= n_live) return;
        iu = blockIdx.x * RR_BLOCK + threadIdx.x;
        valid = (int64_t)iu < n_live;
    }
    const int64_t i = iu;
    // cost-ordered level-0 tiles (LevelArgs.tile_perm / tile_cost): the group scenes' fused kernels
    constexpr bool ORD = FUSED && G == 1;
    // level 0 with a cost array: this wave's clock at entry (its tile's cost is stored at the end)
    const uint64_t clk0 = (ORD && A.tile_cost) ? __builtin_amdgcn_s_memtime() : 0;
    zero_next_counters(A);
    if (LC) stage_culls(S);
    Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t trace_flops = 0;
    uint32_t trace_visits = 0;
    constexpr int64_t tile = -1;  // the tile of the wave's launch slot
#include "shade_body.inc"
    if (FUSED && A.level > 0)  // secondary levels: unbalanced waves, no barrier at the end
        flush<true>(cnt, A.counters, W_SHADOW, trace_flops, trace_visits);
    else
        flush(cnt, A.counters, W_SHADOW, trace_flops, trace_visits);
}


// ---------------------------------------------------------------- in-kernel reflection chains
// Scenes without transparency (fused levels) whose materials reflect: an event has at most one child, its
// reflection, so color_at(ray, rem) is a chain  v_d = (surface_d + v_{d+1} * reflective_d) + black  ending at a
// miss, a non-reflective hit or rem == 0 (scene.rs:128-136,167-177, reflected_color :281-290).  chain_kernel runs
// the whole chain of a camera sample inside the level-0 wave: trace, shade, then the wave loops on its reflected
// lanes (the others idle) until none is left — the same lanes a tile-pure secondary level's wave holds, without
// the 64 B event and 48 B chain record per reflection through HBM, the per-level launches of worst-case grids
// and the deep levels' latency floor.  The chain is folded bottom-up exactly as shade_hit sums it.
// LDS (after the culls, prelit terms and area stage): the reflected ray, parked while the pattern, `pow` and
// shadow walks run (queued to HBM at that point before, for the same register reason), and the level-0 record,
// which becomes the lane's final colour when its chain ends.  Deeper records live in private memory (one
// lane's own stack; few lanes reach it).
struct ChainStage {
    double ray[6][256];  // over_point, reflectv of the pending reflection
    double rec[4][256];  // level 0: surface xyz, reflective; then the finished colour (xyz)
    uint32_t ls[256], lrow[256], px[256];  // camera lanes: the sample's Px0 (lrow's top bit: the lane holds a sample)
    int32_t own[256];  // the parked reflection's origin object, which its closest-hit walk skips (reflect_own), or -1
};
static_assert(sizeof(ChainStage) == RR_CHAIN_STAGE_BYTES, "ChainStage layout");
__device__ __forceinline__ ChainStage* chain_lds(const DevScene& S, bool lc, bool pre, bool ar) {
    char* base = reinterpret_cast<char*>(area_lds(S, lc, pre));
    return reinterpret_cast<ChainStage*>(base + (ar ? sizeof(AreaStage) : 0));
}
// area-light chain kernels (block-synchronised area walks): 2 waves/SIMD, no VGPR spilled (76 spilled at 4, 20 at 3):
// C5 1.40 -> 1.30 ms per frame (1.33 at 3; profiles/r04/ab_ar_waves.txt)
#ifdef RR_CHAIN_AR_WAVES_EXP  // experiment builds (build.py variant) only
constexpr int RR_CHAIN_AR_WAVES = RR_CHAIN_AR_WAVES_EXP;
#else
constexpr int RR_CHAIN_AR_WAVES = 2;
#endif
#define RR_CHAIN_ATTR(PRE, G, AR) \
    __attribute__((amdgpu_waves_per_eu(((PRE) && (G) < 2) ? ((G) == 1 ? RR_G1_WAVES : (AR) ? RR_CHAIN_AR_WAVES : RR_RM_WAVES) : 2)))
// blocks per deep-queue segment: block b works on chunks b / nseg + k * RR_DEEP_SPREAD (C3: ~14 chunks of 256 per
// segment; one block per segment walked them one after the other and left the GPU latency-bound, 2.15 ms)
constexpr int RR_DEEP_SPREAD = 1;
// Deep chains: a camera wave's lanes that are still reflecting after depth A.deep_from - 1 leave the wave — by
// then most of its lanes have finished, and every further depth would cost the whole wave for a few lanes (C3:
// depths 2-5 hold 5.6 M of 124 M rays and took 1.6 of 6.6 ms in the camera waves).  Each leaving lane appends a
// DeepRec (its ray, its chain's records, its output sample) to segment blockIdx % RR_NSEG of a packed queue, one
// atomic per wave; the deep launch (DEEP) then runs those chains from depth deep_from on in dense waves, one block
// per segment walking its segment's chunks, and delivers the finished colours.  Only frames whose samples are
// delivered one by one (canvas or aa == 1) spill; the in-wave AA average needs every sample in its wave.
//
// RM0 / RMD: ray-major chunk tests (walk_nodes) at depth 0 / at depths >= 1 (incoherent rays).  XL (cross-lane
// record reads) only in the flat kernels: the group kernels' loop spills VGPRs, and a spilled register read across
// lanes is unsafe (DESIGN.md §3.6; build.py checks).
template <int G, bool LC, bool PRE, bool CP, bool AR, bool RM0, bool RMD, bool DEEP>
__global__ void __launch_bounds__(256) RR_CHAIN_ATTR(PRE, G, AR) chain_kernel(DevScene S, LevelArgs A) {
    constexpr bool XL = G == 0 && cross_lane_ok(G, CP, AR);
    if constexpr (!AR) load_prologue_args(A);
    // camera launch: one lane per level-0 event; deep launch: block b walks chunks b / nseg, b / nseg + RR_DEEP_SPREAD,
    // ... of segment b % nseg of the deep queue
    const uint32_t seg = DEEP ? blockIdx.x % (uint32_t)A.nseg : 0u;
#ifdef RR_LISTED  // listed pixels: launched for the capacity, the live count is on the device (blocks past it leave)
    const int64_t n_live = DEEP ? (int64_t)A.seg_count[seg] : live_count(A);
#else
    const int64_t n_live = DEEP ? (int64_t)A.seg_count[seg] : A.n;
#endif
    const int64_t first = DEEP ? (int64_t)(blockIdx.x / (uint32_t)A.nseg) * RR_BLOCK : 0;
    if ((DEEP ? first : (int64_t)blockIdx.x * RR_BLOCK) >= n_live) return;
    if (!DEEP) zero_next_counters(A);
    if (LC) stage_culls(S);
    ChainStage& cs = *chain_lds(S, LC, PRE, AR);
    // the thread index, rebuilt at each use from the wave's index (a scalar) and lane_id(): threadIdx.x itself would
    // be held in a VGPR through the whole chain loop
    const uint32_t wave64 = (uint32_t)uniform((int)(threadIdx.x & ~63u));
    const auto tid = [&]() { return (int)(wave64 + (uint32_t)lane_id()); };
    // every walk's exact-test flops and visits stay in cnt (flushed as the shadow walk's): per-walk totals carried
    // through the chain loop took VGPRs there
    Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double stk[RR_MAX_DEPTH][4];  // this lane's own records of depths >= 1 (private memory)
    // REC1: the depth-1 and depth-2 records in registers instead (area-light kernels, which run at 2 waves per SIMD with registers to
    // spare: 217 VGPRs, none spilled): private-memory records are written back to HBM — 35 of C5's 86 MB of writes per
    // frame (profiles/r05/attrib_c5.txt); with them in registers C5 moves 70 instead of 107 MB per frame for +0.7 % time
    // (profiles/r05/ab_rec12_adopted.txt).  The kernels at 4 waves per SIMD have no 16 VGPRs to spare.
#ifdef RR_NO_REC1_EXP  // experiment builds only
    constexpr bool REC1 = false;
#else
    constexpr bool REC1 = AR;
#endif
    double r1[4] = {0.0, 0.0, 0.0, 0.0}, r2[4] = {0.0, 0.0, 0.0, 0.0};  // depths 1 and 2
    __shared__ ShadeStash stash;  // more than RR_PRELIT_LIGHTS lights: eyev / normalv / colour during the walks
    const int nlights = uniform(S.n_lights);  // a scalar loop bound (compared in VALU registers otherwise)
    const V3 zero = mk(0.0, 0.0, 0.0);
    const int d0 = DEEP ? A.deep_from : 0;  // the first depth of this launch's chains
    // cost-ordered camera waves (A.tile_cost / A.tile_perm, as the group scenes' level 0): each wave stores its tile's
    // clock-cycle cost; later frames launch the costliest tiles (the deepest chains) first, so the launch does not
    // end on a few long chains
    const uint64_t clk0 = (!DEEP && A.tile_cost) ? __builtin_amdgcn_s_memtime() : 0;
    for (int64_t base = first; DEEP ? base < n_live : base == 0; base += RR_DEEP_SPREAD * RR_BLOCK) {
        // this lane's event: camera sample blockIdx * 256 + tid, or deep-queue entry seg * seg_cap + base + tid
        const auto ev_index = [&]() -> int64_t {
            return DEEP ? (int64_t)seg * A.seg_cap + base + tid() : (int64_t)(blockIdx.x * RR_BLOCK + (uint32_t)tid());
        };
        // camera lanes: the sample (tile or pixel-wave layout, A.pw), computed once and kept in LDS for the delivery
        // (held in registers through the chain loop it would cost VGPRs; recomputed, VALU)
        Px0 q_cam = {0u, 0u, 0u, 0u};
        bool valid;
        if constexpr (DEEP) {
            valid = base + tid() < n_live;
        } else {
            bool in_px = true;
            q_cam = level0_px<true, true, true>(A, ev_index(), (int)(wave64 >> 6), &in_px);
            valid = (int64_t)(blockIdx.x * RR_BLOCK + (uint32_t)tid()) < n_live && in_px;
            cs.ls[tid()] = q_cam.ls;
            cs.lrow[tid()] = q_cam.lrow | (valid ? 0x80000000u : 0u);
            cs.px[tid()] = q_cam.px;
        }
        uint64_t sample = 0;  // jitter identity of the camera sample (area lights)
        if (AR && valid) {
            if constexpr (DEEP) {
                const uint32_t ls = A.deep[ev_index()].ls;
                const uint32_t hs = (uint32_t)A.hs, lrow = ls / hs, px = ls - lrow * hs;
                sample = A.rays0 ? (uint64_t)ls : (uint64_t)canvas_row(A, lrow) * (uint64_t)A.hs + px;  // as event_key
            } else {
                uint64_t s0 = 0;
                (void)event_ray(A, ev_index(), q_cam, s0);
                sample = A.rays0 ? (uint64_t)q_cam.ls : s0;
            }
        }
        bool active = valid;
        uint32_t path = 1u << d0;  // recursion path code: root 1, reflected child 2p
        // one chain step at `depth` for the active lanes: trace, shade, park the reflection, fold finished chains.
        // The first step (camera rays and RM0 walks, or the deep queue's rays) is peeled off the loop, so the loop
        // body holds only the secondary-ray code and nothing of the first step is hoisted across it.  Returns
        // whether any lane reflects on.
        auto step = [&](auto rm_tag, const int depth) -> bool {
            constexpr bool RM = decltype(rm_tag)::value;
            Ray r = {mk(0, 0, 0), mk(0, 0, 1)};
            Hit th;
            if (!DEEP && depth == 0) {
                if (valid) {
                    uint64_t s0 = 0;
                    r = event_ray(A, ev_index(), q_cam, s0);
                }
                // camera bundles from the per-tile / per-pixel-wave table (tile_bundles), when there is one
                const float* cb = A.pw ? (A.tile_bundles ? A.tile_bundles + (size_t)own_tile<true>(A, (int)(wave64 >> 6)) *
                                                               RR_TILE_BUNDLE_FLOATS
                                                         : nullptr)
                                       : cam_bundle_of<true>(A, (int)(wave64 >> 6));
                trace_closest<G, LC, RM, XL, !AR>(S, r, active, th, cnt, A.pw ? cb != nullptr : cam_tile(A), cb);
            } else {
                if (DEEP && depth == d0) {
                    if (active) {
                        const DeepRec& e = A.deep[ev_index()];
                        r = {mk(e.o[0], e.o[1], e.o[2]), mk(e.d[0], e.d[1], e.d[2])};
                    }
                } else if (active) {
                    r = {mk(cs.ray[0][tid()], cs.ray[1][tid()], cs.ray[2][tid()]),
                         mk(cs.ray[3][tid()], cs.ray[4][tid()], cs.ray[5][tid()])};
                }
                const int own_in = (!DEEP || depth > d0) && active ? cs.own[tid()] : -1;
                trace_closest<G, LC, RM, XL, !AR, true, true>(S, r, active, th, cnt, false, nullptr, own_in);
            }
            cnt.rays += popc_ballot(active);
            const bool has_hit = active && th.found;
            cnt.shade += popc_ballot(has_hit);
            V3 over = zero, eyev = mk(0, 0, 1), normalv = mk(0, 0, 1);
            int32_t mat = 0, own = -1;
            double refl = 0.0;
            bool do_refl = false;
            if (has_hit) {
                Hit h = th;
                h.found = true;
                mat = AR ? S.nodes[th.node].material : th.mat;
                const DevMaterial m = S.mats[mat];
                Comps c;
                prepare(S, r, h, c);  // intersection.rs:50-60
                over = c.over;
                eyev = c.eyev;
                normalv = c.normalv;
                own = own_node(c, th.node);
                do_refl = A.rem - depth > 0 && m.reflective != 0.0;
                if (do_refl) {  // parked: the child ray is dead through the pattern / pow / shadow code below
                    cs.ray[0][tid()] = c.over.x;
                    cs.ray[1][tid()] = c.over.y;
                    cs.ray[2][tid()] = c.over.z;
                    cs.ray[3][tid()] = c.reflectv.x;
                    cs.ray[4][tid()] = c.reflectv.y;
                    cs.ray[5][tid()] = c.reflectv.z;
                    cs.own[tid()] = reflect_own(c, own);
                }
                refl = m.reflective;
            }
            V3 surface = zero;  // surface = 0 + L0 + L1 + ... (scene.rs:159-166)
            if (has_hit) {
                const DevMaterial m = S.mats[mat];
                const V3 pcol = material_color<CP>(S, m, th.node, over);  // material.rs:77-80
                if (PRE) {
                    double* pl = prelit_lds(S, LC);
                    for (int li = 0; li < nlights; ++li) {
                        V3 amb, dsp;
                        light_terms(m, ldc(S.lights, li), pcol, over, eyev, normalv, amb, dsp);
                        const double v6[6] = {amb.x, amb.y, amb.z, dsp.x, dsp.y, dsp.z};
                        for (int k = 0; k < 6; ++k) pl[(li * 6 + k) * 256 + tid()] = v6[k];
                    }
                } else {
                    stash_put(stash, eyev, normalv, pcol);
                }
            }
            if constexpr (PRE) {
                const double* pl = prelit_lds(S, LC);
                for (int li = 0; li < nlights; ++li) {
                    const DevLight Lt = ldc(S.lights, li);
                    const double* q = pl + li * 6 * 256 + tid();
                    const bool lit = has_hit && !(q[768] == 0.0 && q[1024] == 0.0 && q[1280] == 0.0);  // see shadow_amount
                    // (the area-light kernels keep their code: measured +0.5 % on C5 with the point-light skip compiled in)
                    const double in_shadow = shadow_amount<G, LC, RM, AR, XL, !AR, !AR>(S, A, Lt, li, over, lit, has_hit, sample,
                                                                                    path, area_lds(S, LC, true), cnt, nullptr,
                                                                                    own, normalv);
                    if (has_hit) {
                        const V3 amb = mk(q[0], q[256], q[512]), dsp = mk(q[768], q[1024], q[1280]);
                        surface = vadd(surface, light_final(amb, dsp, in_shadow));
                    }
                }
            } else {
                for (int li = 0; li < nlights; ++li)
                    light_step<G, LC, RM, AR, XL>(S, A, li, has_hit, mat, over, sample, path, stash,
                                                  area_lds(S, LC, false), surface, cnt);
            }
            if (do_refl) {  // pending: park (surface, reflective) at this depth
                if (!DEEP && depth == 0) {
                    cs.rec[0][tid()] = surface.x;
                    cs.rec[1][tid()] = surface.y;
                    cs.rec[2][tid()] = surface.z;
                    cs.rec[3][tid()] = refl;
                } else if (REC1 && depth == 1) {  // wave-uniform
                    r1[0] = surface.x;
                    r1[1] = surface.y;
                    r1[2] = surface.z;
                    r1[3] = refl;
                } else if (REC1 && depth == 2) {
                    r2[0] = surface.x;
                    r2[1] = surface.y;
                    r2[2] = surface.z;
                    r2[3] = refl;
                } else {
                    stk[depth][0] = surface.x;
                    stk[depth][1] = surface.y;
                    stk[depth][2] = surface.z;
                    stk[depth][3] = refl;
                }
            } else if (active) {  // the chain ends here: fold every ancestor innermost-first (scene.rs:172-177)
                V3 v = has_hit ? shade_sum(surface, zero, zero, refl, 0.0, 0.0) : zero;
                for (int lv = depth - 1; lv >= (DEEP ? d0 : 1); --lv) {  // wave-uniform: every lane here has them
                    if (REC1 && lv <= 2) {
                        const double* r = lv == 1 ? r1 : r2;
                        v = shade_sum(mk(r[0], r[1], r[2]), vmul(v, r[3]), zero, r[3], 0.0, 0.0);
                        continue;
                    }
                    const double rf = stk[lv][3];
                    v = shade_sum(mk(stk[lv][0], stk[lv][1], stk[lv][2]), vmul(v, rf), zero, rf, 0.0, 0.0);
                }
                if constexpr (DEEP) {  // the camera wave's records, carried in the queue entry
                    const DeepRec& e = A.deep[ev_index()];
                    for (int lv = d0 - 1; lv >= 0; --lv) {
                        const double rf = e.rec[lv][3];
                        v = shade_sum(mk(e.rec[lv][0], e.rec[lv][1], e.rec[lv][2]), vmul(v, rf), zero, rf, 0.0, 0.0);
                    }
                } else if (depth >= 1) {
                    const double rf = cs.rec[3][tid()];
                    v = shade_sum(mk(cs.rec[0][tid()], cs.rec[1][tid()], cs.rec[2][tid()]), vmul(v, rf), zero, rf, 0.0,
                                  0.0);
                }
                cs.rec[0][tid()] = v.x;  // the finished colour (its level-0 record is consumed)
                cs.rec[1][tid()] = v.y;
                cs.rec[2][tid()] = v.z;
            }
            active = do_refl;
            uniform_counters(cnt);
            // area lights synchronise the block inside the shadow walks, so their loop is block-uniform
            return AR ? __syncthreads_or(active) != 0 : __ballot(active) != 0;
        };
        bool more = step(std::integral_constant<bool, DEEP ? RMD : RM0>{}, d0);
        bool spilled = false;  // this lane's chain went on to the deep queue
        for (int depth = d0 + 1; more; ++depth) {
            if (!DEEP && depth == A.deep_from) {  // the lanes still reflecting leave for the deep queue
                spilled = active;
                const uint32_t dseg = blockIdx.x >> RR_DEEP_SHIFT;  // neighbouring camera blocks share a segment
                const int32_t slot = wave_append(A.seg_out_count + dseg, spilled);
                if (spilled) {
                    DeepRec& e = A.deep[(int64_t)dseg * A.seg_cap_out + slot];
                    for (int k = 0; k < 3; ++k) e.o[k] = cs.ray[k][tid()];
                    for (int k = 0; k < 3; ++k) e.d[k] = cs.ray[3 + k][tid()];
                    for (int k = 0; k < 4; ++k) e.rec[0][k] = cs.rec[k][tid()];
                    for (int lv = 1; lv < RR_DEEP_FROM; ++lv)
                        for (int k = 0; k < 4; ++k) e.rec[lv][k] = (REC1 && lv == 1) ? r1[k] : stk[lv][k];
                    e.ls = cs.ls[tid()];
                }
                break;
            }
            path *= 2u;
            more = step(std::integral_constant<bool, RMD>{}, depth);
        }
        // deliver the finished samples: the averaged image (aa == 1, or in the wave for aa in {2, 4, 8}) and/or the
        // canvas (ls = the sample's part-local row-major index)
        const bool valid2 = (DEEP ? base + tid() < n_live : (cs.lrow[tid()] >> 31) != 0u) && !spilled;
        const V3 v = valid2 ? mk(cs.rec[0][tid()], cs.rec[1][tid()], cs.rec[2][tid()]) : zero;
        if constexpr (DEEP) {
            if (valid2) deliver(0, ev_index(), -1, 0, v, A.out, A.avg, A.avg_f32, nullptr, nullptr, A.deep[ev_index()].ls);
        } else {
            Px0 q0;
            q0.ls = cs.ls[tid()];
            q0.lrow = cs.lrow[tid()] & 0x7fffffffu;
            q0.px = cs.px[tid()];
            q0.py = 0u;
            if (A.pw) {  // aa = 3: the pixel's 9 samples are in this wave
                if (A.out && valid2) {
                    double* o = A.out + 3 * (int64_t)q0.ls;
                    o[0] = v.x;
                    o[1] = v.y;
                    o[2] = v.z;
                }
                deliver_pixel_wave(A, cs.rec, wave64, q0, valid2);
            } else if (A.aa_wave) {
                if (A.out && valid2) {
                    double* o = A.out + 3 * (int64_t)q0.ls;
                    o[0] = v.x;
                    o[1] = v.y;
                    o[2] = v.z;
                }
                deliver_wave_avg(A, v, q0, valid2);
            } else if (valid2) {
                deliver(0, ev_index(), -1, 0, v, A.out, A.avg, A.avg_f32, nullptr, nullptr, q0.ls);
            }
        }
    }
    if (!DEEP && A.tile_cost) {  // the wave's tile cost in clock cycles, from lane 0 (a vector store)
        const uint64_t dt = __builtin_amdgcn_s_memtime() - clk0;
        if (lane_id() == 0) A.tile_cost[own_tile<true>(A, (int)(wave64 >> 6))] = dt > 0xffffffffull ? 0xffffffffu : (uint32_t)dt;
    }
    if (AR)
        flush(cnt, A.counters, W_SHADOW);
    else  // no workgroup barrier in the non-area kernels: a finished wave leaves at once
        flush<true>(cnt, A.counters, W_SHADOW, 0, 0, (int)(wave64 >> 6));
}

template <int G, bool LC, bool PRE, bool CP, bool DEEP>
static void launch_chain_ar(const DevScene& S, const LevelArgs& A, hipStream_t st, size_t lds) {
    // camera launch: one lane per level-0 event; deep launch: RR_DEEP_SPREAD blocks per segment of the deep queue
    const dim3 grid(DEEP ? (unsigned)A.nseg * RR_DEEP_SPREAD : blocks_for(A.n)), block(256);
    constexpr bool RM0 = G > 0, RMD = true;  // ray-major tests at depth 0 / at depths >= 1 (incoherent rays)
    if (S.has_area)
        hipLaunchKernelGGL((chain_kernel<G, LC, PRE, CP, true, RM0, RMD, DEEP>), grid, block, lds, st, S, A);
    else
        hipLaunchKernelGGL((chain_kernel<G, LC, PRE, CP, false, RM0, RMD, DEEP>), grid, block, lds, st, S, A);
}

template <int G, bool LC, bool DEEP>
static void launch_chain_deep(const DevScene& S, const LevelArgs& A, hipStream_t st, size_t lds) {
    const bool pre = S.n_lights <= RR_PRELIT_LIGHTS;
    if (S.complex_patterns) {
        if (pre)
            launch_chain_ar<G, LC, true, true, DEEP>(S, A, st, lds);
        else
            launch_chain_ar<G, LC, false, true, DEEP>(S, A, st, lds);
    } else {
        if (pre)
            launch_chain_ar<G, LC, true, false, DEEP>(S, A, st, lds);
        else
            launch_chain_ar<G, LC, false, false, DEEP>(S, A, st, lds);
    }
}

template <int G, bool LC>
void launch_chain_t(const DevScene& S, const LevelArgs& A, hipStream_t st, KernelProf* prof, bool deep) {
    const bool pre = S.n_lights <= RR_PRELIT_LIGHTS;
    const size_t lds = cull_lds(S) + (pre ? (size_t)S.n_lights * 6 * 256 * sizeof(double) : 0) +
                       (S.has_area ? sizeof(AreaStage) : 0) + sizeof(ChainStage);
    Span s(prof, deep ? K_DEEP : K_CHAIN, st);
#if !defined(RR_LISTED) && !defined(RR_VIEWS)  // listed pixels and batched views never leave their camera wave for the deep queue
    if (deep)
        launch_chain_deep<G, LC, true>(S, A, st, lds);
    else
#endif
        launch_chain_deep<G, LC, false>(S, A, st, lds);
}


template <int G, bool LC, bool FUSED, bool RM, bool PRE, bool CP>
static void launch_shade_ar(const DevScene& S, const LevelArgs& A, hipStream_t st, size_t lds) {
    const dim3 grid(blocks_for(A.n)), block(256);
    if (S.has_area)
        hipLaunchKernelGGL((shade_kernel<G, LC, FUSED, PRE, CP, RM, true>), grid, block, lds, st, S, A);
    else
        hipLaunchKernelGGL((shade_kernel<G, LC, FUSED, PRE, CP, RM, false>), grid, block, lds, st, S, A);
}
template <int G, bool LC, bool FUSED, bool RM>
static void launch_shade_rm(const DevScene& S, const LevelArgs& A, hipStream_t st, bool pre, size_t lds) {
    if (S.complex_patterns) {
        if (pre)
            launch_shade_ar<G, LC, FUSED, RM, true, true>(S, A, st, lds);
        else
            launch_shade_ar<G, LC, FUSED, RM, false, true>(S, A, st, lds);
    } else {
        if (pre)
            launch_shade_ar<G, LC, FUSED, RM, true, false>(S, A, st, lds);
        else
            launch_shade_ar<G, LC, FUSED, RM, false, false>(S, A, st, lds);
    }
}
// RM (ray-major chunk tests, walk_nodes) for the secondary levels, whose waves are often
// incoherent, and for every level of scenes with groups (a mesh chunk holds many small triangles:
// C4 teapot 1.65 -> 1.35 ms per frame with it at level 0).  Level 0 of flat scenes (camera tiles and
// their shadow rays) runs without it, which keeps the camera kernels' registers (C2 0.172 vs
// 0.177 ms with it).
template <int G, bool LC, bool FUSED>
static void launch_shade(const DevScene& S, const LevelArgs& A, hipStream_t st, bool pre, size_t lds) {
    if constexpr (G > 0) {
        launch_shade_rm<G, LC, FUSED, true>(S, A, st, pre, lds);
    } else {
        if (A.level > 0)
            launch_shade_rm<G, LC, FUSED, true>(S, A, st, pre, lds);
        else
            launch_shade_rm<G, LC, FUSED, false>(S, A, st, pre, lds);
    }
}

// LevelArgs.uniform_hit of a launch: on unless RRAY_NO_UNIFORM_HIT=1 (read at every launch, like RRAY_NO_PERSIST)
static inline uint32_t uniform_hit_on() {
    const char* off = std::getenv("RRAY_NO_UNIFORM_HIT");
    return (off && std::atoi(off) == 1) ? 0u : 1u;
}

template <int G, bool LC>
void launch_level_t(const DevScene& S, const LevelArgs& A, hipStream_t st, KernelProf* prof) {
    const bool pre = S.n_lights <= RR_PRELIT_LIGHTS;
    const size_t shade_lds = cull_lds(S) + (pre ? (size_t)S.n_lights * prelit_per_light(S.has_area) * 256 * sizeof(double) : 0) +
                             (S.has_area ? sizeof(AreaStage) : 0);
    if (fused_levels(S)) {  // trace + shade in one kernel
        Span s(prof, K_TRACE_SHADE, st);
        if constexpr (G == 0 && !LC) {  // the kernels that read it (shade_body.inc UH)
            LevelArgs B = A;
            B.uniform_hit = uniform_hit_on();
            launch_shade<G, LC, true>(S, B, st, pre, shade_lds);
        } else {
            launch_shade<G, LC, true>(S, A, st, pre, shade_lds);
        }
        return;
    }
#if !defined(RR_LISTED) && !defined(RR_VIEWS)  // the listed-pixel and view-batch kernels serve the production dispatches only: no unfused level kernels
    {
        Span s(prof, K_TRACE, st);
        if (A.level > 0)
            hipLaunchKernelGGL((trace_kernel<G, LC, true>), dim3(blocks_for(A.n)), dim3(256), cull_lds(S), st, S, A);
        else
            hipLaunchKernelGGL((trace_kernel<G, LC, false>), dim3(blocks_for(A.n)), dim3(256), cull_lds(S), st, S, A);
    }
    if (S.has_transparent) {
        Span s(prof, K_N1N2, st);
        if (A.level > 0)
            hipLaunchKernelGGL((n1n2_kernel<G, LC, true>), dim3(blocks_for(A.n)), dim3(256), cull_lds(S), st, S, A);
        else
            hipLaunchKernelGGL((n1n2_kernel<G, LC, false>), dim3(blocks_for(A.n)), dim3(256), cull_lds(S), st, S, A);
    }
    {
        Span s(prof, K_SHADE, st);
        launch_shade<G, LC, false>(S, A, st, pre, shade_lds);
    }
#endif
}

