// render_tree.inc — the color_at recursion of scenes with transparent materials inside the camera wave (tree_kernel).
// Included inside namespace rr after render_common.inc and render_levels.inc (it shares the chain kernels' LDS stage,
// shading steps and delivery).
//
// With a transparent material shade_hit has two children (scene.rs:159-178): reflected_color (scene.rs:281-290) and
// refracted_color (scene.rs:310-336), so a camera sample's color_at is a binary tree of depth <= remaining.  The per-level
// path ran it breadth first through HBM queues: trace, n1n2 and shade launches per level and a bottom-up combine pass
// per level (23 launches for a C1 frame, most of them worst-case grids whose waves exit at once).  tree_kernel runs the
// whole tree of each sample in its camera lane, depth first, with an explicit per-lane stack:
//
//   * one iteration of the wave loop = one color_at call per active lane: the closest-hit walk, the n1/n2 container walk
//     for the lanes that need it (intersection.rs:61-92), prepare_computations, the children, the pattern and every
//     light's is_shadowed walk + lighting (scene.rs:159-166) — the lanes of a wave are at different depths of their
//     trees, but they all run the same code on one ray each;
//   * a shading event with children pushes a frame {surface, reflective, transparency, Schlick R, reflected result,
//     the refracted ray while its reflected sibling runs} and descends into its first child (reflected, else refracted);
//     the current ray is parked in LDS while the pattern, `pow` and shadow code run (ChainStage.ray, as the chains);
//   * a finished color_at (a miss, an event without children) unwinds: the value becomes the parent's reflected slot
//     (v * reflective) — the parent then descends into its waiting refracted ray — or its refracted slot
//     (v * transparency), which completes the parent with shade_hit's own sum (shade_sum: Schlick weighting when the
//     material both reflects and refracts, scene.rs:172-177); completed parents unwind further;
//   * a sample whose root completes leaves its colour in LDS (ChainStage.rec) for the delivery the chain kernels use
//     (the averaged image, in-wave AA for aa 2/4/8, pixel waves for aa 3, or the canvas).
// The frames live in the lane's private memory (scratch): only the lanes that hit a transparent or reflective
// material push one, and a frame is written once and read once or twice.  The value of every node is computed with
// the same operations as shade_hit, and the children's order does not change any value (the area-light jitter is keyed
// by the node's path code: root 1, reflected child 2p, refracted child 2p + 1, as the per-level path and the oracle),
// so frames are bit-identical to the per-level kernels' (RRAY_NO_TREE=1 selects those).  One launch per frame.
struct TreeFrame {
    double surf[3], acc[3];  // the light sum; the reflected slot (color_at(reflected) * reflective, or black)
    double rr[6];            // the refracted ray (under_point, direction) waiting for its reflected sibling
    double refl, transp, R;  // material.reflective, material.transparency, schlick() (0 unless both > 0)
    uint32_t flags;          // TF_* below
};
constexpr uint32_t TF_REFR_STAGE = 1u;    // the frame's child in progress is its refracted one (else reflected)
constexpr uint32_t TF_REFR_WAITING = 2u;  // the refracted child is still to run (after the reflected one)

// the tree kernels' occupancy, the most waves per SIMD without a VGPR spill (kernel-resource-usage): 4 (128 VGPRs) for the
// flat scenes' point-light kernels without tree-evaluated patterns (the README scene: 106 VGPRs), 3 for the group scenes'
// ones (2 to 18 spilled at 4), 2 for the rest (general shapes, area lights, complex patterns: 60-260
// spilled at 4).  The walks do not read across lanes (XL off), so a spill would only cost time, never correctness.
#define RR_TREE_ATTR(G, CP, AR) \
    __attribute__((amdgpu_waves_per_eu(((G) == 0 && !(CP) && !(AR)) ? 4 : ((G) == 1 && !(CP) && !(AR)) ? 3 : 2)))

template <int G, bool LC, bool PRE, bool CP, bool AR, bool RM0, bool RMD>
__global__ void __launch_bounds__(256) RR_TREE_ATTR(G, CP, AR) tree_kernel(DevScene S, LevelArgs A) {
    constexpr bool XL = false;
    if constexpr (!AR) load_prologue_args(A);
#ifdef RR_LISTED  // listed pixels: launched for the capacity, the live count is on the device (blocks past it leave)
    const int64_t n_live = live_count(A);
#else
    const int64_t n_live = A.n;
#endif
    if ((int64_t)blockIdx.x * RR_BLOCK >= n_live) return;
    zero_next_counters(A);
    if (LC) stage_culls(S);
    ChainStage& cs = *chain_lds(S, LC, PRE, AR);
    const uint32_t wave64 = (uint32_t)uniform((int)(threadIdx.x & ~63u));
    const auto tid = [&]() { return (int)(wave64 + (uint32_t)lane_id()); };
    const auto ev_index = [&]() -> int64_t { return (int64_t)(blockIdx.x * RR_BLOCK + (uint32_t)tid()); };
    Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    __shared__ ShadeStash stash;  // more than RR_PRELIT_LIGHTS lights: eyev / normalv / colour during the walks
    const int nlights = uniform(S.n_lights);
    const V3 zero = mk(0.0, 0.0, 0.0);
    const uint64_t clk0 = A.tile_cost ? __builtin_amdgcn_s_memtime() : 0;
    bool in_px = true;
    const Px0 q_cam = level0_px<true, true, true>(A, ev_index(), (int)(wave64 >> 6), &in_px);
    const bool valid = ev_index() < n_live && in_px;
    cs.ls[tid()] = q_cam.ls;
    cs.lrow[tid()] = q_cam.lrow | (valid ? 0x80000000u : 0u);
    cs.px[tid()] = q_cam.px;
    uint64_t sample = 0;  // jitter identity of the camera sample (area lights)
    if (AR && valid) {
        uint64_t s0 = 0;
        (void)event_ray(A, ev_index(), q_cam, s0);
        sample = A.rays0 ? (uint64_t)q_cam.ls : s0;
    }
    TreeFrame stk[RR_MAX_DEPTH];  // this lane's pending shade_hit frames, one per depth (private memory)
    int depth = 0;                // the current ray's depth: remaining = A.rem - depth
    uint32_t path = 1u;           // its path code (root 1, reflected child 2p, refracted child 2p + 1)
    bool active = valid;
    // One color_at call per active lane.  The first (camera rays, or rr_color_at's rays) is peeled off the loop, as in
    // chain_kernel.  Returns whether any lane has a ray left.
    auto step = [&](auto rm_tag, auto first_tag) -> bool {
        constexpr bool RM = decltype(rm_tag)::value;
        constexpr bool FIRST = decltype(first_tag)::value;
        Ray r = {mk(0, 0, 0), mk(0, 0, 1)};
        Hit th;
        if constexpr (FIRST) {
            if (valid) {
                uint64_t s0 = 0;
                r = event_ray(A, ev_index(), q_cam, s0);
            }
            const float* cb = A.pw ? (A.tile_bundles ? A.tile_bundles + (size_t)own_tile<true>(A, (int)(wave64 >> 6)) *
                                                           RR_TILE_BUNDLE_FLOATS
                                                     : nullptr)
                                   : cam_bundle_of<true>(A, (int)(wave64 >> 6));
            trace_closest<G, LC, RM, XL, !AR>(S, r, active, th, cnt, A.pw ? cb != nullptr : cam_tile(A), cb);
        } else {
            if (active)
                r = {mk(cs.ray[0][tid()], cs.ray[1][tid()], cs.ray[2][tid()]),
                     mk(cs.ray[3][tid()], cs.ray[4][tid()], cs.ray[5][tid()])};
            const int own_in = active ? cs.own[tid()] : -1;
            trace_closest<G, LC, RM, XL, !AR, true, true>(S, r, active, th, cnt, false, nullptr, own_in);
        }
        cnt.rays += popc_ballot(active);
        const bool has_hit = active && th.found;
        cnt.shade += popc_ballot(has_hit);
        const int rem = A.rem - depth;
        int32_t mat = 0;
        bool need12 = false;
        if (has_hit) {
            mat = AR ? S.nodes[th.node].material : th.mat;
            need12 = needs_n1n2(S.mats[mat], rem);
        }
        // prepare_computations' containers (intersection.rs:61-92) for the lanes whose refraction or Schlick term reads
        // n1 / n2 (th.rank is the hit node's rank, as the walk needs)
        double n1 = 1.0, n2 = 1.0;
        if (__ballot(need12) != 0) n1n2_walk<G, LC, RM, XL>(S, r, th, need12, n1, n2, cnt);
        V3 over = zero, eyev = mk(0, 0, 1), normalv = mk(0, 0, 1);
        int32_t own = -1;
        double refl = 0.0, transp = 0.0, R = 0.0;
        bool do_refl = false, do_refr = false;
        if (has_hit) {
            const DevMaterial m = S.mats[mat];
            Comps c;
            prepare(S, r, th, c);  // intersection.rs:50-60
            if (need12) {
                c.n1 = n1;
                c.n2 = n2;
            }
            over = c.over;
            eyev = c.eyev;
            normalv = c.normalv;
            own = own_node(c, th.node);
            refl = m.reflective;
            transp = m.transparency;
            R = (m.reflective > 0.0 && m.transparency > 0.0) ? schlick(c) : 0.0;  // computations.rs:39-54
            do_refl = rem > 0 && m.reflective != 0.0;  // reflected_color (scene.rs:281-290)
            if (do_refl) {  // parked: the child ray is dead through the pattern / pow / shadow code below
                cs.ray[0][tid()] = c.over.x;
                cs.ray[1][tid()] = c.over.y;
                cs.ray[2][tid()] = c.over.z;
                cs.ray[3][tid()] = c.reflectv.x;
                cs.ray[4][tid()] = c.reflectv.y;
                cs.ray[5][tid()] = c.reflectv.z;
                cs.own[tid()] = reflect_own(c, own);
            }
            if (rem > 0 && m.transparency != 0.0) {  // refracted_color (scene.rs:310-336)
                const double n_ratio = c.n1 / c.n2;
                const double cos_i = dot3(c.eyev, c.normalv);
                const double sin2_t = (n_ratio * n_ratio) * (1.0 - cos_i * cos_i);
                if (!(sin2_t > 1.0)) {  // else total internal reflection: black
                    const double cos_t = sqrt(1.0 - sin2_t);
                    const V3 d = vsub(vmul(c.normalv, n_ratio * cos_i - cos_t), vmul(c.eyev, n_ratio));
                    do_refr = true;
                    if (do_refl) {  // runs after its reflected sibling: framed below
                        TreeFrame& f = stk[depth];
                        f.rr[0] = c.under.x;
                        f.rr[1] = c.under.y;
                        f.rr[2] = c.under.z;
                        f.rr[3] = d.x;
                        f.rr[4] = d.y;
                        f.rr[5] = d.z;
                    } else {  // the first child: parked like a reflected ray, no object skipped (it enters its object)
                        cs.ray[0][tid()] = c.under.x;
                        cs.ray[1][tid()] = c.under.y;
                        cs.ray[2][tid()] = c.under.z;
                        cs.ray[3][tid()] = d.x;
                        cs.ray[4][tid()] = d.y;
                        cs.ray[5][tid()] = d.z;
                        cs.own[tid()] = -1;
                    }
                }
            }
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
                light_step<G, LC, RM, AR, XL>(S, A, li, has_hit, mat, over, sample, path, stash, area_lds(S, LC, false),
                                              surface, cnt);
        }
        if (do_refl || do_refr) {  // shade_hit waits for its children: push its frame, descend into the first child
            TreeFrame& f = stk[depth];
            f.surf[0] = surface.x;
            f.surf[1] = surface.y;
            f.surf[2] = surface.z;
            f.acc[0] = f.acc[1] = f.acc[2] = 0.0;  // reflected_color is black unless the reflected child delivers
            f.refl = refl;
            f.transp = transp;
            f.R = R;
            f.flags = do_refl ? (do_refr ? TF_REFR_WAITING : 0u) : TF_REFR_STAGE;
            depth += 1;
            path = 2u * path + (do_refl ? 0u : 1u);
        } else if (active) {  // color_at finished: shade_hit with black children, or black on a miss
            V3 v = has_hit ? shade_sum(surface, zero, zero, refl, transp, R) : zero;
            bool next = false;
            while (depth > 0 && !next) {  // unwind: deliver v into the parent's slot
                TreeFrame& f = stk[depth - 1];
                if (!(f.flags & TF_REFR_STAGE)) {  // the reflected child: v * reflective (scene.rs:289)
                    f.acc[0] = v.x * f.refl;
                    f.acc[1] = v.y * f.refl;
                    f.acc[2] = v.z * f.refl;
                    if (f.flags & TF_REFR_WAITING) {  // now the refracted sibling (path 2p + 1)
                        for (int k = 0; k < 6; ++k) cs.ray[k][tid()] = f.rr[k];
                        cs.own[tid()] = -1;
                        f.flags = TF_REFR_STAGE;
                        path += 1u;
                        next = true;
                        break;
                    }
                    v = shade_sum(mk(f.surf[0], f.surf[1], f.surf[2]), mk(f.acc[0], f.acc[1], f.acc[2]), zero, f.refl,
                                  f.transp, f.R);
                } else {  // the refracted child: v * transparency (scene.rs:335), then shade_hit's sum
                    const V3 b = vmul(v, f.transp);
                    v = shade_sum(mk(f.surf[0], f.surf[1], f.surf[2]), mk(f.acc[0], f.acc[1], f.acc[2]), b, f.refl,
                                  f.transp, f.R);
                }
                depth -= 1;
                path >>= 1;
            }
            if (!next) {  // the root: the sample's colour
                cs.rec[0][tid()] = v.x;
                cs.rec[1][tid()] = v.y;
                cs.rec[2][tid()] = v.z;
                active = false;
            }
        }
        uniform_counters(cnt);
        // area lights synchronise the block inside the shadow walks, so their loop is block-uniform
        return AR ? __syncthreads_or(active) != 0 : __ballot(active) != 0;
    };
    bool more = step(std::integral_constant<bool, RM0>{}, std::true_type{});
    while (more) more = step(std::integral_constant<bool, RMD>{}, std::false_type{});
    // deliver the finished samples (as chain_kernel): the averaged image (aa == 1, or in the wave for aa in {2, 4, 8}),
    // pixel waves (aa == 3) and/or the canvas (ls = the sample's part-local row-major index)
    const bool valid2 = (cs.lrow[tid()] >> 31) != 0u;
    const V3 v = valid2 ? mk(cs.rec[0][tid()], cs.rec[1][tid()], cs.rec[2][tid()]) : zero;
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
    if (A.tile_cost) {  // the wave's tile cost in clock cycles, from lane 0 (a vector store)
        const uint64_t dt = __builtin_amdgcn_s_memtime() - clk0;
        if (lane_id() == 0) A.tile_cost[own_tile<true>(A, (int)(wave64 >> 6))] = dt > 0xffffffffull ? 0xffffffffu : (uint32_t)dt;
    }
    if (AR)
        flush(cnt, A.counters, W_SHADOW);
    else  // no workgroup barrier in the non-area kernels: a finished wave leaves at once
        flush<true>(cnt, A.counters, W_SHADOW, 0, 0, (int)(wave64 >> 6));
}

template <int G, bool LC, bool PRE, bool CP>
static void launch_tree_ar(const DevScene& S, const LevelArgs& A, hipStream_t st, size_t lds) {
    const dim3 grid(blocks_for(A.n)), block(256);
    constexpr bool RM0 = G > 0, RMD = true;  // ray-major tests for the first rays / the secondary (incoherent) rays
    if (S.has_area)
        hipLaunchKernelGGL((tree_kernel<G, LC, PRE, CP, true, RM0, RMD>), grid, block, lds, st, S, A);
    else
        hipLaunchKernelGGL((tree_kernel<G, LC, PRE, CP, false, RM0, RMD>), grid, block, lds, st, S, A);
}

template <int G, bool LC>
void launch_tree_t(const DevScene& S, const LevelArgs& A, hipStream_t st, KernelProf* prof) {
    const bool pre = S.n_lights <= RR_PRELIT_LIGHTS;
    const size_t lds = cull_lds(S) + (pre ? (size_t)S.n_lights * 6 * 256 * sizeof(double) : 0) +
                       (S.has_area ? sizeof(AreaStage) : 0) + sizeof(ChainStage);
    Span s(prof, K_CHAIN, st);
    if (S.complex_patterns) {
        if (pre)
            launch_tree_ar<G, LC, true, true>(S, A, st, lds);
        else
            launch_tree_ar<G, LC, false, true>(S, A, st, lds);
    } else {
        if (pre)
            launch_tree_ar<G, LC, true, false>(S, A, st, lds);
        else
            launch_tree_ar<G, LC, false, false>(S, A, st, lds);
    }
}
