// render_views_hit_g2_lds.hip — the first-hit kernel with the view-batch source (rr_render_views_aov: a table of
// cameras, render_common.inc level0_px / event_ray under RR_VIEWS) for G = 2 (general scenes: CSG, 4-entry leaves), culls staged in LDS.
// The same sources as render_hit_g2_lds.hip, compiled into namespace rr::views: the production kernels stay as they are.
#include <cstdlib>

#include "device_core.inc"
#include "kernels.hpp"
#include "wavefront.hpp"

#define RR_VIEWS 1
namespace rr {
namespace views {
#include "render_common.inc"
#include "render_hit.inc"

template void launch_hit_t<2, true>(const DevScene&, const LevelArgs&, const HitOut&, hipStream_t);
}  // namespace views
}  // namespace rr
