// render_hit.hip — launch of the first-hit kernels (render_hit.inc hit_kernel): picks the (G, LC) variant of the
// uploaded scene, as launch_level / launch_chain / launch_tree do.  The kernels themselves are instantiated in
// render_hit_g<G>_<lds|gl>.hip.
#include "kernels.hpp"

namespace rr {

hipError_t launch_hit(const DevScene& S, const LevelArgs& A, const HitOut& O, hipStream_t st) {
    if (A.n <= 0) return hipSuccess;
    const int g = S.general ? 2 : S.has_groups ? 1 : 0;  // G: flat / groups / general (CSG, 4-entry leaves)
    if (g == 2) {
        if (S.lds_culls)
            launch_hit_t<2, true>(S, A, O, st);
        else
            launch_hit_t<2, false>(S, A, O, st);
    } else if (g == 1) {
        if (S.lds_culls)
            launch_hit_t<1, true>(S, A, O, st);
        else
            launch_hit_t<1, false>(S, A, O, st);
    } else {
        if (S.lds_culls)
            launch_hit_t<0, true>(S, A, O, st);
        else
            launch_hit_t<0, false>(S, A, O, st);
    }
    return hipGetLastError();
}

}  // namespace rr
