// render_listed_levels_g1_lds.hip — the fused level-0 kernel with the listed-pixel source (adaptive frames' refine
// pass, render_common.inc level0_px under RR_LISTED) for G = 1 (scenes with groups), culls staged in LDS.  The same sources
// as render_levels_g1_lds.hip, compiled into namespace rr::listed: the production kernels stay as they are.
#include <cstdlib>

#include "device_core.inc"
#include "kernels.hpp"
#include "wavefront.hpp"

#define RR_LISTED 1
namespace rr {
namespace listed {
#include "render_common.inc"
#include "render_levels.inc"

template void launch_level_t<1, true>(const DevScene&, const LevelArgs&, hipStream_t, KernelProf*);
}  // namespace listed
}  // namespace rr
