// render_listed_levels_g2_gl.hip — the fused level-0 kernel with the listed-pixel source (adaptive frames' refine
// pass, render_common.inc level0_px under RR_LISTED) for G = 2 (general scenes), culls read from global memory.  The same sources
// as render_levels_g2_gl.hip, compiled into namespace rr::listed: the production kernels stay as they are.
#include <cstdlib>

#include "device_core.inc"
#include "kernels.hpp"
#include "wavefront.hpp"

#define RR_LISTED 1
namespace rr {
namespace listed {
#include "render_common.inc"
#include "render_levels.inc"

template void launch_level_t<2, false>(const DevScene&, const LevelArgs&, hipStream_t, KernelProf*);
}  // namespace listed
}  // namespace rr
