// unit_chain.hip — the reflection-chain kernels (render_levels.inc chain_kernel) of one (G, LC, level-0 source)
// variant: unit_select.inc.  Units of their own (objects render[_listed|_views]_chain_g<G>_<lds|gl>): the build compiles
// these without machine LICM, which otherwise hoists constant materialisations (OCML pow's coefficients) out of the
// chain loop and spills them.
#include <cstdlib>

#include "device_core.inc"
#include "kernels.hpp"
#include "wavefront.hpp"

#include "unit_select.inc"
RR_UNIT_OPEN
#include "render_common.inc"
#include "render_levels.inc"

template void launch_chain_t<RR_UNIT_G, RR_UNIT_LC != 0>(const DevScene&, const LevelArgs&, hipStream_t, KernelProf*, bool);
RR_UNIT_CLOSE
