// render_listed_chain_g1_lds.hip — the reflection-chain kernels with the listed-pixel source (adaptive frames' refine
// pass, render_common.inc level0_px under RR_LISTED) for G = 1 (scenes with groups), culls staged in LDS.  The same sources
// as render_chain_g1_lds.hip and built like it, compiled into namespace rr::listed.
#include <cstdlib>

#include "device_core.inc"
#include "kernels.hpp"
#include "wavefront.hpp"

#define RR_LISTED 1
namespace rr {
namespace listed {
#include "render_common.inc"
#include "render_levels.inc"

template void launch_chain_t<1, true>(const DevScene&, const LevelArgs&, hipStream_t, KernelProf*, bool);
}  // namespace listed
}  // namespace rr
