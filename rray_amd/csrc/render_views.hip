// render_views.hip — the launches of a batch of views (rr_render_views): one pass's level-0 events
// through the scene's own in-wave kernel family, compiled with the camera-table source in namespace rr::views
// (the units render_views_{levels,chain,tree}_g<G>_<lds|gl>: unit_*.hip with the views source), and a pass of
// rr_render_views_aov (§3.17) through the first-hit kernel compiled the same way (render_views_hit_g<G>_<lds|gl>).
// Only the argument checks and the (G, LC) dispatch (kernels.hpp dispatch_glc) live here: the pass's level-0 launch,
// by the scene's kernel family as launch_level / launch_chain / launch_tree.
#include "kernels.hpp"

namespace rr {

// what every rr::views kernel relies on: a camera table, whole waves per view, level 0, camera rays, none of the
// single frame's per-camera tables (cached bundles, cost order, pixel waves, the resident loop's queue)
static bool views_args_ok(const LevelArgs& A) {
    return A.views && A.view_e >= 64 && A.view_e % 64 == 0 && A.level == 0 && !A.rays0 && !A.list && !A.n_dev &&
           !A.tile_bundles && !A.tile_perm && !A.tile_cost && !A.pw && !A.deep_from && A.n % A.view_e == 0 &&
           (int64_t)A.view_e >= A.hs * A.lrows;
}

hipError_t launch_level_views(const DevScene& S, const LevelArgs& A, hipStream_t st, KernelProf* prof) {
    if (A.n <= 0) return hipSuccess;
    if (!views_args_ok(A) || !fused_levels(S)) return hipErrorInvalidValue;
    dispatch_glc(S, [&](auto g, auto lc) { views::launch_level_t<g(), lc()>(S, A, st, prof); });
    return hipGetLastError();
}

hipError_t launch_chain_views(const DevScene& S, const LevelArgs& A, hipStream_t st, KernelProf* prof) {
    if (A.n <= 0) return hipSuccess;
    if (!views_args_ok(A)) return hipErrorInvalidValue;
    dispatch_glc(S, [&](auto g, auto lc) { views::launch_chain_t<g(), lc()>(S, A, st, prof, false); });
    return hipGetLastError();
}

hipError_t launch_tree_views(const DevScene& S, const LevelArgs& A, hipStream_t st, KernelProf* prof) {
    if (A.n <= 0) return hipSuccess;
    if (!views_args_ok(A)) return hipErrorInvalidValue;
    dispatch_glc(S, [&](auto g, auto lc) { views::launch_tree_t<g(), lc()>(S, A, st, prof); });
    return hipGetLastError();
}

// one pass of rr_render_views_aov: the first-hit kernel over the pass's views (the units render_views_hit_g<G>_<lds|gl>).
// It counts into the query buffer and clears nothing (no counters_zero); the planes it writes are the ones O names
hipError_t launch_hit_views(const DevScene& S, const LevelArgs& A, const HitOut& O, hipStream_t st) {
    if (A.n <= 0) return hipSuccess;
    if (!views_args_ok(A) || A.base != 0 || A.n >= ((int64_t)1 << 31) || A.counters_zero || !O.node_object ||
        !(O.depth || O.normal || O.object || O.albedo))
        return hipErrorInvalidValue;
    dispatch_glc(S, [&](auto g, auto lc) { views::launch_hit_t<g(), lc()>(S, A, O, st); });
    return hipGetLastError();
}

}  // namespace rr
