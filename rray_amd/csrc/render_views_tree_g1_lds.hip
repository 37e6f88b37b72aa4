// render_views_tree_g1_lds.hip — the color_at tree kernels with the view-batch source (rr_render_views: a table of cameras,
// render_common.inc level0_px / event_ray under RR_VIEWS) for G = 1 (scenes with groups), culls staged in LDS.  The same sources
// as render_tree_g1_lds.hip and built like it, compiled into namespace rr::views: the production kernels stay as they are.
#include <cstdlib>

#include "device_core.inc"
#include "kernels.hpp"
#include "wavefront.hpp"

#define RR_VIEWS 1
namespace rr {
namespace views {
#include "render_common.inc"
#include "render_levels.inc"
#include "render_tree.inc"

template void launch_tree_t<1, true>(const DevScene&, const LevelArgs&, hipStream_t, KernelProf*);
}  // namespace views
}  // namespace rr
