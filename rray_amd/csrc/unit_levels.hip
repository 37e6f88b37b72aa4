// unit_levels.hip — the level kernels (render_levels.inc) of one (G, LC, level-0 source) variant: unit_select.inc.
// One variant per compile so the kernel variants build in parallel; the build names the objects
// render[_listed|_views]_levels_g<G>_<lds|gl>.  The listed and views variants serve level 0 only (the fused kernel).
// The listed variants also hold the first-hit kernel of ordered ray batches (render_hit.inc under RR_LISTED: the one
// ray-batch instantiation, rr_hit_at_device_ordered), so the unit table keeps its rows.
#include <cstdlib>

#include "device_core.inc"
#include "kernels.hpp"
#include "wavefront.hpp"

#include "unit_select.inc"
RR_UNIT_OPEN
#include "render_common.inc"
#include "render_levels.inc"

template void launch_level_t<RR_UNIT_G, RR_UNIT_LC != 0>(const DevScene&, const LevelArgs&, hipStream_t, KernelProf*);
#if RR_UNIT_SRC == 1
#include "render_hit.inc"

template void launch_hit_t<RR_UNIT_G, RR_UNIT_LC != 0>(const DevScene&, const LevelArgs&, const HitOut&, hipStream_t);
#endif
RR_UNIT_CLOSE
