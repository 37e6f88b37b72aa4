// render_persist_g0_gl.hip — the persistent level-0 loop (render_persist.inc) for G = 0 (flat scenes), culls read
// from global memory: the fused camera kernel of frames without secondary rays as one resident launch.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "device_core.inc"
#include "kernels.hpp"
#include "wavefront.hpp"

namespace rr {
#include "render_common.inc"
#include "render_levels.inc"
#include "render_persist.inc"

PersistPlan persist_plan(const DevScene& S, const LevelArgs& A, int* resident) {
    if (S.general || S.has_groups || S.lds_culls) return {0, 0};
    return persist_plan_t<0, false>(S, A, resident);
}

hipError_t launch_persist(const DevScene& S, const LevelArgs& A, const PersistPlan& plan, hipStream_t st, KernelProf* prof) {
    launch_persist_t<0, false>(S, A, plan, st, prof);
    return hipGetLastError();
}
}  // namespace rr
