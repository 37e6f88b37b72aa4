// shade_body.inc — the body of shade_kernel (render_levels.inc) for one wave's 64 events, from the level-0 canvas
// mapping to the tile's cost record: included inside shade_kernel and inside shade_tile (render_persist.inc, the
// persistent level-0 loop), so both compile the same statements.  It is shared as text and not as a function
// because shade_kernel built around a call of an always-inlined function allocated registers differently in 118 of
// its instantiations (2-4 VGPRs more); included, every one of them keeps the code it had.
// The including scope provides: template parameters G, LC, FUSED, PRE, CP, RM, AR; S, A; the event index iu / i and
// `valid`; ORD; clk0 (the wave's clock at entry, cost-ordered kernels); cnt, trace_flops, trace_visits (zero); and
// `tile`: the level-0 tile the wave renders, or -1 for the tile of its launch slot.
    // UH: the C2 family (flat scene, global culls, fused, prelit point lights, no tree pattern: persist_kernel and the
    // level-0 shade_kernel it mirrors) shades a tile whose 64 lanes hit one node from scalar records, a plane's normal
    // from the table behind S.nodes (device_core.inc prepare_tile / tile_material / tile_color); every other
    // instantiation compiles to the code it had
#ifdef RR_LISTED
    constexpr bool UH = false;
#else
    constexpr bool UH = G == 0 && !LC && FUSED && PRE && !CP && !RM && !AR;
#endif
#ifdef RR_VIEWS  // a view's events past its samples (sizes that are no multiple of 8) hold none
    bool in_view = true;
    const Px0 q0 = A.level > 0 ? Px0{0u, 0u, 0u, 0u} : level0_px<true, ORD>(A, i, -1, &in_view, tile);
    valid = valid && in_view;
#else
    const Px0 q0 = level0_px_if<true, ORD>(A, i, tile);
#endif
    const uint32_t ls0 = q0.ls;
    HitRec hr;
    hr.node = -1;
    int32_t hmat = 0;  // FUSED: the hit node's material, from the walk
    Ray r0 = {mk(0, 0, 0), mk(0, 0, 1)};  // FUSED: the event's ray, traced here
    uint64_t s0 = 0;  // level-0 sample id from event_ray
    if (FUSED) {
        if (valid) r0 = event_ray(A, i, q0, s0);
        Hit th;
        // the hit's material from the walk (C2 -1 %; the area-light kernels measured slower with it)
        trace_closest<G, LC, RM, cross_lane_ok(G, CP, AR), !AR>(S, r0, valid, th, cnt, cam_tile(A), cam_bundle_of<ORD>(A, -1, tile));
        cnt.rays += popc_ballot(valid);
        hr.t = th.t;
        hr.u = th.u;
        hr.v = th.v;
        hr.node = th.found ? th.node : -1;
        hr.k = th.k;
        hmat = th.mat;
        trace_flops = cnt.flops;
        trace_visits = cnt.visits;
        cnt.flops = cnt.visits = 0;
    } else if (valid) {
        hr = A.hit[i];
    }
    const bool has_hit = valid && hr.node >= 0;
    // UH: every lane of the wave is valid and hit the same top-level plane (partial and mixed tiles keep
    // the per-lane code); unode / umat are wave-uniform then
    bool uni = false;
    int unode = 0, umat = 0;
    if constexpr (UH) {
        unode = uniform(hr.node);
        umat = uniform(hmat);
        uni = A.uniform_hit && __ballot(has_hit && hr.node == unode) == ~0ull && uniform_hit_node(S, unode);
    }
    int32_t parent = -1, slot = 0;
    if (valid && A.level > 0) {
        parent = A.ev[i].parent;
        slot = A.ev[i].slot;
    }
    cnt.shade += popc_ballot(has_hit);
    V3 over = mk(0, 0, 0), eyev = mk(0, 0, 1), normalv = mk(0, 0, 1), pcol = mk(0, 0, 0);
    int32_t mat = 0, own = -1;
    double refl = 0.0, transp = 0.0, R = 0.0;
    bool do_refl = false, do_refr = false;
    Ray rr = {mk(0, 0, 0), mk(0, 0, 1)}, refr = rr;
    uint64_t sample = 0;
    uint32_t path = 1u;
    if (has_hit) {
        const Ray r = FUSED ? r0 : event_ray(A, i, q0, s0);
        Hit h;
        h.found = true;
        h.t = hr.t;
        h.u = hr.u;
        h.v = hr.v;
        h.node = hr.node;
        h.k = hr.k;
        mat = (FUSED && !AR) ? hmat : S.nodes[hr.node].material;
        const DevMaterial m = S.mats[mat];
        Comps c;
        prepare_tile<UH>(S, r, h, c, uni, unode);  // intersection.rs:50-60
        if (S.has_transparent && needs_n1n2(m, A.rem)) {
            c.n1 = A.n12[2 * i];
            c.n2 = A.n12[2 * i + 1];
        }
        over = c.over;
        eyev = c.eyev;
        normalv = c.normalv;
        own = own_node(c, hr.node);
        do_refl = A.rem > 0 && m.reflective != 0.0;
        if (do_refl) {
            rr.o = c.over;
            rr.d = c.reflectv;
        }
        // FUSED: no material of the scene is transparent (fused_levels), so neither a refracted child nor
        // Schlick's term exists — compiled out, which keeps their registers out of the fused kernels
        if (!FUSED && A.rem > 0 && m.transparency != 0.0) {
            double n_ratio = c.n1 / c.n2;
            double cos_i = dot3(c.eyev, c.normalv);
            double sin2_t = (n_ratio * n_ratio) * (1.0 - cos_i * cos_i);
            if (!(sin2_t > 1.0)) {
                double cos_t = sqrt(1.0 - sin2_t);
                refr.o = c.under;
                refr.d = vsub(vmul(c.normalv, n_ratio * cos_i - cos_t), vmul(c.eyev, n_ratio));
                do_refr = true;
            }
        }
        refl = m.reflective;
        transp = FUSED ? 0.0 : m.transparency;
        R = (!FUSED && m.reflective > 0.0 && m.transparency > 0.0) ? schlick(c) : 0.0;
        event_key(A, i, q0, s0, sample, path);
    }
    // children of this level -> next level queue; parents -> this level's pending list (FUSED: no
    // list — without transparency an event has at most one child, and that chain's leaf finishes it)
    const bool pending = do_refl || do_refr;
    const uint32_t ls = A.level > 0 ? A.ev[valid ? i : 0].sample : ls0;  // the camera sample's output index
    if (A.next) {  // null when no material is reflective or transparent (or at the last level)
        int32_t slots[3];
        if constexpr (FUSED) {  // segment blockIdx % nseg_out of the next level, one atomic per wave
            const uint32_t seg = blockIdx.x % (uint32_t)A.nseg_out;
            if (A.pad_children) {  // the wave's children keep their lanes in a 64-slot block (tile-pure waves)
                const uint64_t m = __ballot(do_refl);
                if (m) {
                    const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
                    unsigned int base = 0;
                    if (lane == leader) base = atomicAdd(A.seg_out_count + seg, 64u);
                    base = (unsigned int)__builtin_amdgcn_readlane((int)base, leader);
                    const int64_t at = (int64_t)seg * A.seg_cap_out + base + lane;
                    slots[0] = (int32_t)at;
                    if (!do_refl) A.next[at].parent = -2;
                }
            } else {
                const int32_t s1 = wave_append(A.seg_out_count + seg, do_refl);
                slots[0] = (int32_t)((int64_t)seg * A.seg_cap_out + s1);
            }
        } else {
            unsigned int* const ctr[3] = {A.lcount + LC_CHILDREN, A.lcount + LC_CHILDREN, A.lcount + LC_PENDING};
            const bool wq[3] = {do_refl, do_refr, pending};
            block_append<3>(ctr, wq, slots);
        }
        if (do_refl) {
            Event e;
            e.o[0] = rr.o.x;
            e.o[1] = rr.o.y;
            e.o[2] = rr.o.z;
            e.d[0] = rr.d.x;
            e.d[1] = rr.d.y;
            e.d[2] = rr.d.z;
            e.sample = ls;
            e.path = path * 2u;
            e.parent = (int32_t)i;
            e.slot = 0;
            A.next[slots[0]] = e;
        }
        if (do_refr) {
            Event e;
            e.o[0] = refr.o.x;
            e.o[1] = refr.o.y;
            e.o[2] = refr.o.z;
            e.d[0] = refr.d.x;
            e.d[1] = refr.d.y;
            e.d[2] = refr.d.z;
            e.sample = ls;
            e.path = path * 2u + 1u;
            e.parent = (int32_t)i;
            e.slot = 1;
            A.next[slots[1]] = e;
        }
        if (!FUSED && pending) A.pending[slots[2]] = (int32_t)i;
    }
    // the surface colour and (PRE) every light's ambient / diffuse+specular terms, after the children
    // are queued: point / under / reflectv and the child rays are dead by now, which keeps the
    // pattern and `pow` code below the 128-VGPR budget without spilling
    constexpr int NPL = prelit_per_light(AR);
    if (has_hit) {
        const DevMaterial m = tile_material<UH>(S, mat, uni, umat);
        pcol = tile_color<UH, CP>(S, m, hr.node, over, uni, umat);  // material.rs:77-80
        if (PRE) {
            double* pl = prelit_lds(S, LC);
            for (int li = 0; li < S.n_lights; ++li) {
                V3 amb, dsp;
                // the small scenes' LDS-cull kernels keep the pow for every lit lane (the tiny-specular test spilled 2
                // of their VGPRs)
                light_terms<!LC>(m, ldc(S.lights, li), pcol, over, eyev, normalv, amb, dsp,
                                 NPL == 10 ? pl + (li * NPL + 6) * 256 + threadIdx.x : nullptr);
                const double v6[6] = {amb.x, amb.y, amb.z, dsp.x, dsp.y, dsp.z};
                for (int k = 0; k < 6; ++k) pl[(li * NPL + k) * 256 + threadIdx.x] = v6[k];
            }
        }
    }
    // surface = 0 + L0 + L1 + ... (scene.rs:159-166)
    V3 surface = mk(0, 0, 0);
    if constexpr (PRE) {
        const double* pl = prelit_lds(S, LC);
        for (int li = 0; li < S.n_lights; ++li) {
            const DevLight Lt = ldc(S.lights, li);
            const int t = threadIdx.x;
            const double* q = pl + li * NPL * 256 + t;
            const bool lit = has_hit && !(q[768] == 0.0 && q[1024] == 0.0 && q[1280] == 0.0);  // see shadow_amount
            const double in_shadow =
                shadow_amount<G, LC, RM, AR, cross_lane_ok(G, CP, AR), !AR>(S, A, Lt, li, over, lit, has_hit, sample, path,
                                                                             area_lds(S, LC, true), cnt,
                                                                             NPL == 10 ? q + 6 * 256 : nullptr, own,
                                                                             normalv);
            if (has_hit) {
                const V3 amb = mk(q[0], q[256], q[512]), dsp = mk(q[768], q[1024], q[1280]);
                surface = vadd(surface, light_final(amb, dsp, in_shadow));
            }
        }
    } else {
        __shared__ ShadeStash stash;
        stash_put(stash, eyev, normalv, pcol);
        for (int li = 0; li < S.n_lights; ++li)
            light_step<G, LC, RM, AR, cross_lane_ok(G, CP, AR)>(S, A, li, has_hit, mat, over, sample, path, stash,
                                                                 area_lds(S, LC, false), surface,
                                  cnt);
    }
    if constexpr (FUSED) {
        // Reflection chains (no transparency in the scene, so no refracted child): a pending event parks
        // its surface sum; a finished event (leaf) completes every ancestor on its chain, innermost
        // first, with shade_hit's own sum c_parent = (surface + c * reflective) + black (scene.rs:172-177,
        // reflected_color scene.rs:281-290), and writes the level-0 value — no combine pass, and no
        // partial writes into the parents' records.
        if (A.aa_wave) {  // level 0 of a frame without secondary rays: average inside the wave
            const V3 zero = mk(0.0, 0.0, 0.0);
            const V3 v = has_hit ? shade_sum(surface, zero, zero, refl, 0.0, 0.0) : zero;
            if (A.out && valid) {  // the supersampled canvas too, when the caller asked for it
                double* o = A.out + 3 * (int64_t)ls0;
                o[0] = v.x;
                o[1] = v.y;
                o[2] = v.z;
            }
            deliver_wave_avg(A, v, q0, valid);
        } else if (pending) {
            ChainRec cr;
            cr.surf[0] = surface.x;
            cr.surf[1] = surface.y;
            cr.surf[2] = surface.z;
            cr.refl = refl;
            cr.parent = parent;
            A.chain[A.level][i] = cr;
        } else if (valid) {
            const V3 zero = mk(0.0, 0.0, 0.0);
            V3 v = has_hit ? shade_sum(surface, zero, zero, refl, 0.0, 0.0) : zero;
            int32_t p = parent;
            for (int lv = A.level - 1; lv >= 0; --lv) {  // every leaf of this level has the same chain length
                const ChainRec c = A.chain[lv][p];
                v = shade_sum(mk(c.surf[0], c.surf[1], c.surf[2]), vmul(v, c.refl), zero, c.refl, 0.0, 0.0);
                p = c.parent;
            }
            deliver(0, i, -1, 0, v, A.out, A.avg, A.avg_f32, nullptr, nullptr, ls);
        }
    } else if (pending) {
        CombRec cr;
        cr.surf[0] = surface.x;
        cr.surf[1] = surface.y;
        cr.surf[2] = surface.z;
        cr.refl_res[0] = cr.refl_res[1] = cr.refl_res[2] = 0.0;
        cr.refl = refl;
        cr.parent = parent;
        cr.flags = CF_HIT | (slot ? CF_REFRACT_CHILD : 0);
        A.comb[i] = cr;
        if (A.comb_ext) {
            CombExt ce;
            ce.refr_res[0] = ce.refr_res[1] = ce.refr_res[2] = 0.0;
            ce.transp = transp;
            ce.R = R;
            A.comb_ext[i] = ce;
        }
    } else if (valid) {  // finished: color_at = shade_hit with black children, or black on a miss
        const V3 zero = mk(0.0, 0.0, 0.0);
        const V3 v = has_hit ? shade_sum(surface, zero, zero, refl, transp, R) : zero;
        deliver(A.level, i, parent, slot, v, A.out, A.avg, A.avg_f32, A.parent_comb, A.parent_ext, ls0);
    }
    if (ORD && A.tile_cost) {  // level 0 (host-set): the tile's cost in clock cycles, from lane 0 (a vector store)
        const uint64_t dt = __builtin_amdgcn_s_memtime() - clk0;
        if ((threadIdx.x & 63) == 0) A.tile_cost[own_tile<ORD>(A, -1, tile)] = dt > 0xffffffffull ? 0xffffffffu : (uint32_t)dt;
    }
