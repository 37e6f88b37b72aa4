// render_hit_g2_lds.hip — first-hit kernels (render_hit.inc hit_kernel: rr_hit_at, rr_render_aov) for G = 2
// (general scenes (CSG, 4-entry leaves)), culls staged in LDS.
#include <cstdlib>

#include "device_core.inc"
#include "kernels.hpp"
#include "wavefront.hpp"

namespace rr {
#include "render_common.inc"
#include "render_hit.inc"

template void launch_hit_t<2, true>(const DevScene&, const LevelArgs&, const HitOut&, hipStream_t);
}  // namespace rr
