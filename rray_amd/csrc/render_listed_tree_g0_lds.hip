// render_listed_tree_g0_lds.hip — the color_at tree kernels with the listed-pixel source (adaptive frames' refine
// pass, render_common.inc level0_px under RR_LISTED) for G = 0 (flat scenes), culls staged in LDS.  The same sources
// as render_tree_g0_lds.hip and built like it, compiled into namespace rr::listed.
#include <cstdlib>

#include "device_core.inc"
#include "kernels.hpp"
#include "wavefront.hpp"

#define RR_LISTED 1
namespace rr {
namespace listed {
#include "render_common.inc"
#include "render_levels.inc"
#include "render_tree.inc"

template void launch_tree_t<0, true>(const DevScene&, const LevelArgs&, hipStream_t, KernelProf*);
}  // namespace listed
}  // namespace rr
