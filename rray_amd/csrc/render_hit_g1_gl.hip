// render_hit_g1_gl.hip — first-hit kernels (render_hit.inc hit_kernel: rr_hit_at, rr_render_aov) for G = 1
// (scenes with groups), culls read from global memory.
#include <cstdlib>

#include "device_core.inc"
#include "kernels.hpp"
#include "wavefront.hpp"

namespace rr {
#include "render_common.inc"
#include "render_hit.inc"

template void launch_hit_t<1, false>(const DevScene&, const LevelArgs&, const HitOut&, hipStream_t);
}  // namespace rr
