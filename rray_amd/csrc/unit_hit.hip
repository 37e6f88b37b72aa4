// unit_hit.hip — the first-hit kernels (render_hit.inc hit_kernel: rr_hit_at, rr_render_aov, rr_render_views_aov) of
// one (G, LC, level-0 source) variant: unit_select.inc.  Objects render[_views]_hit_g<G>_<lds|gl>.  The views variants
// hold the camera kernels only and carry no cached bundles; there is no listed-pixel first-hit query (the ordered ray
// batches' first-hit kernel, the one listed instantiation, is built in the listed level units: unit_levels.hip).
#include <cstdlib>

#include "device_core.inc"
#include "kernels.hpp"
#include "wavefront.hpp"

#include "unit_select.inc"
#if RR_UNIT_SRC == 1
#error "unit_hit.hip: RR_UNIT_SRC 0 (production) or 2 (views)"
#endif
RR_UNIT_OPEN
#include "render_common.inc"
#include "render_hit.inc"

template void launch_hit_t<RR_UNIT_G, RR_UNIT_LC != 0>(const DevScene&, const LevelArgs&, const HitOut&, hipStream_t);
RR_UNIT_CLOSE
