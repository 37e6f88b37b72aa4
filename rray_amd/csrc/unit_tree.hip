// unit_tree.hip — the color_at tree kernels of scenes with transparent materials (render_tree.inc tree_kernel) of one
// (G, LC, level-0 source) variant: unit_select.inc.  Objects render[_listed|_views]_tree_g<G>_<lds|gl>, built like the
// chain units (no machine LICM: the loop's constants are rematerialised rather than hoisted and spilled).
#include <cstdlib>

#include "device_core.inc"
#include "kernels.hpp"
#include "wavefront.hpp"

#include "unit_select.inc"
RR_UNIT_OPEN
#include "render_common.inc"
#include "render_levels.inc"
#include "render_tree.inc"

template void launch_tree_t<RR_UNIT_G, RR_UNIT_LC != 0>(const DevScene&, const LevelArgs&, hipStream_t, KernelProf*);
RR_UNIT_CLOSE
