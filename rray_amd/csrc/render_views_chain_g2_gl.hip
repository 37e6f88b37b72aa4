// render_views_chain_g2_gl.hip — the reflection-chain kernels with the view-batch source (rr_render_views: a table of cameras,
// render_common.inc level0_px / event_ray under RR_VIEWS) for G = 2 (general scenes), culls read from global memory.  The same sources
// as render_chain_g2_gl.hip and built like it, compiled into namespace rr::views: the production kernels stay as they are.
#include <cstdlib>

#include "device_core.inc"
#include "kernels.hpp"
#include "wavefront.hpp"

#define RR_VIEWS 1
namespace rr {
namespace views {
#include "render_common.inc"
#include "render_levels.inc"

template void launch_chain_t<2, false>(const DevScene&, const LevelArgs&, hipStream_t, KernelProf*, bool);
}  // namespace views
}  // namespace rr
