// render_hit.inc — first-hit queries: Scene::intersect -> hit -> prepare_computations of one ray per lane
// (scene.rs:97-106,128-136; intersection.rs:50-92) with no shading (hit_kernel).  Included inside namespace rr after
// render_common.inc; instantiated per (G, LC) in render_hit_g<G>_<lds|gl>.hip.
//
// The kernel runs exactly the steps the colour kernels run for every ray before they shade — trace_closest, the
// n1/n2 container walk, prepare, material_color (device_core.inc) — on the same rays, and stores their results
// instead of consuming them:
//   * CAM: the lane is a canvas sample.  Lanes are laid out as the level-0 lanes of chain_kernel / tree_kernel
//     (level0_px: 8x8 tiles, one wave per tile when every tile is full), the ray is event_ray's camera ray and the
//     walk is culled with the context's cached tile bundle (cam_bundle_of), so a sample's hit is the colour frame's
//     hit bit for bit.  When the frame has partial tiles the lanes run in tile_to_local order and only the last wave
//     is short: its lanes past the frame stay in the walk inactive and store nothing (as the colour kernels').
//     Requested planes are written per sample, row-major; the frame runs without the n1/n2 walk (N12 off).
//   * !CAM: the lane reads its ray from the caller's batch (A.rays0, as rr_color_at's level 0) and stores the whole
//     record, one plane per field (HitOut.rec_i / rec_d); the batch's last wave is short.  N12: the container walk
//     runs for EVERY lane that hit, as the reference computes n1 / n2 for every hit (intersection.rs:61-92), not only
//     for the transparent materials whose shading reads them.
// Why it is exact: every value stored is the value the colour kernels compute from the same inputs with the same
// device functions (tests/test_gpu_fuzz.py holds their frames to the oracle bit for bit), and the culls only skip
// nodes whose exact test cannot report an entry (DESIGN.md §3.5).  The walks do not read across lanes (XL off, as
// the tree kernels), so a VGPR spill could only cost time, never a result.
// RR_VIEWS (namespace rr::views, render_views_hit_g<G>_<lds|gl>.hip: rr_render_views_aov): the CAM kernels once more
// with the camera-table source.  A pass is whole views of whole waves; a lane is valid when it is inside the launch
// and holds a sample of its view (level0_px's ok), q.ls is its slot in the pass's stacked planes, and there is no
// cached bundle (A.tile_bundles == null): full tiles of an affine view build the corner bundle in the walk (cam_tile
// from the table), every other wave its bundle from its own rays.  Waves of the last block past the events read the
// table's padding (RR_VIEW_TABLE_PAD) for their flag.
// CP: material_color may meet a tree-evaluated pattern (gradient / blend / perturbed / noise / texture: the scene's
// complex_patterns); only the albedo plane reads it.
//
// Occupancy: the walk's state (ray, hit record, bundle, lane ray, the node's inverse) plus prepare's chain of
// transforms need 101-128 VGPRs in the flat and group kernels: 4 waves per SIMD (128 VGPRs) is the most they take
// without a VGPR spill, but for the group scenes' batch kernel with the n1/n2 walk (2 spilled at 4, so it gets 3).
// The general (G = 2) kernels (CSG evaluation buffers in scratch) and the tree-pattern variants (pattern_tree is a
// call) get 2 (256 VGPRs) like their colour counterparts.  DESIGN.md §3.14 has the table (tools/kernel_resources.py).
#define RR_HIT_ATTR(G, CAM, CP) \
    __attribute__((amdgpu_waves_per_eu(((G) == 2 || (CP)) ? 2 : ((G) == 1 && !(CAM)) ? 3 : 4)))

template <int G, bool LC, bool CAM, bool N12, bool CP = false>
__global__ void __launch_bounds__(256) RR_HIT_ATTR(G, CAM, CP) hit_kernel(DevScene S, LevelArgs A, HitOut O) {
    constexpr bool XL = false;
    constexpr bool RM = CAM ? G > 0 : true;  // ray-major tests: the colour kernels' choice for camera / incoherent rays
    load_prologue_args(A);
    const int64_t n_live = A.n;
    if ((int64_t)blockIdx.x * RR_BLOCK >= n_live) return;
    if (LC) stage_culls(S);
    const uint32_t wave64 = (uint32_t)uniform((int)(threadIdx.x & ~63u));
    const int wave = (int)(wave64 >> 6);
    const int64_t i = (int64_t)(blockIdx.x * RR_BLOCK + wave64 + (uint32_t)lane_id());
#ifdef RR_VIEWS
    // a batch of views (rr_render_views_aov): every view takes whole waves, so a ragged view's last wave has idle
    // lanes inside the launch, not only at its end (level0_px's ok); q.ls is the slot in the pass's stacked planes
    bool in_px = true;
    const Px0 q = level0_px<true>(A, i, wave, &in_px);
    const bool valid = i < n_live && in_px;
    Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#else
    const bool valid = i < n_live;
    Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const Px0 q = level0_px<true>(A, i, wave);
#endif
    Ray r = {mk(0, 0, 0), mk(0, 0, 1)};
    if (valid) {
        uint64_t s0 = 0;
        r = event_ray(A, i, q, s0);
    }
    Hit th;
    trace_closest<G, LC, RM, XL, true>(S, r, valid, th, cnt, cam_tile(A), cam_bundle_of(A, wave));
    cnt.rays += popc_ballot(valid);
    const bool has_hit = valid && th.found;
    double n1 = 1.0, n2 = 1.0;
    if constexpr (N12) {
        if (__ballot(has_hit) != 0) n1n2_walk<G, LC, RM, XL>(S, r, th, has_hit, n1, n2, cnt);
    }
    Comps c;
    c.point = c.eyev = c.normalv = c.over = c.under = c.reflectv = mk(0.0, 0.0, 0.0);
    c.inside = false;
    if (has_hit) prepare(S, r, th, c);  // intersection.rs:50-60
    const int32_t object = has_hit ? O.node_object[th.node] : -1;
    if constexpr (CAM) {
        if (valid) {
            const int64_t ls = (int64_t)q.ls;
            if (O.depth) __builtin_nontemporal_store(has_hit ? th.t : (double)__builtin_inf(), O.depth + ls);
            if (O.normal) {
                double* o = O.normal + 3 * ls;
                __builtin_nontemporal_store(c.normalv.x, o);
                __builtin_nontemporal_store(c.normalv.y, o + 1);
                __builtin_nontemporal_store(c.normalv.z, o + 2);
            }
            if (O.object) __builtin_nontemporal_store(object, O.object + ls);
        }
        if (O.albedo) {  // material.rs:77-80, as shade_hit's lighting reads it
            V3 pcol = mk(0.0, 0.0, 0.0);
            if (has_hit) pcol = material_color<CP>(S, S.mats[th.mat], th.node, c.over);
            if (valid) {
                double* o = O.albedo + 3 * (int64_t)q.ls;
                __builtin_nontemporal_store(pcol.x, o);
                __builtin_nontemporal_store(pcol.y, o + 1);
                __builtin_nontemporal_store(pcol.z, o + 2);
            }
        }
    } else {
        if (valid) {
            const int64_t j = A.base + i;
            O.rec_i[j] = object;
            O.rec_i[O.stride + j] = c.inside ? 1 : 0;
            const double f[RR_HIT_DOUBLES] = {has_hit ? th.t : 0.0, has_hit ? th.u : 0.0, has_hit ? th.v : 0.0,
                                              c.point.x, c.point.y, c.point.z, c.eyev.x, c.eyev.y, c.eyev.z,
                                              c.normalv.x, c.normalv.y, c.normalv.z, c.over.x, c.over.y, c.over.z,
                                              c.under.x, c.under.y, c.under.z, c.reflectv.x, c.reflectv.y, c.reflectv.z,
                                              has_hit ? n1 : 0.0, has_hit ? n2 : 0.0};
#pragma unroll
            for (int k = 0; k < RR_HIT_DOUBLES; ++k) O.rec_d[(int64_t)k * O.stride + j] = f[k];
        }
    }
    uniform_counters(cnt);
    flush<true>(cnt, A.counters, W_TRACE, 0, 0, wave);  // no workgroup barrier: a finished wave leaves at once
}

template <int G, bool LC>
void launch_hit_t(const DevScene& S, const LevelArgs& A, const HitOut& O, hipStream_t st) {
    const dim3 grid(blocks_for(A.n)), block(256);
    const size_t lds = cull_lds(S);
#ifdef RR_LISTED  // ordered ray batches only (launch_hit_ordered refuses anything else): the one !CAM instantiation
    hipLaunchKernelGGL((hit_kernel<G, LC, false, true>), grid, block, lds, st, S, A, O);
#else
#ifdef RR_VIEWS  // camera samples only (launch_hit_views refuses a ray batch): the CAM instantiations
    if (O.albedo && S.complex_patterns) {
#else
    if (A.rays0) {
        hipLaunchKernelGGL((hit_kernel<G, LC, false, true>), grid, block, lds, st, S, A, O);
    } else if (O.albedo && S.complex_patterns) {
#endif
        hipLaunchKernelGGL((hit_kernel<G, LC, true, false, true>), grid, block, lds, st, S, A, O);
    } else {
        hipLaunchKernelGGL((hit_kernel<G, LC, true, false, false>), grid, block, lds, st, S, A, O);
    }
#endif
}
