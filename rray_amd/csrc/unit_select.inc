// unit_select.inc — the selectors of a kernel-variant unit (unit_levels.hip, unit_chain.hip, unit_tree.hip,
// unit_hit.hip).  rray_amd/build.py compiles each of those files once per row of its unit table and gives every
// compile its variant as defines:
//   RR_UNIT_G    0 flat scenes, 1 scenes with groups, 2 general scenes (CSG, 4-entry leaves)
//   RR_UNIT_LC   1 culls staged in LDS, 0 culls read from global memory
//   RR_UNIT_SRC  the level-0 source: 0 production (the frame's camera; namespace rr), 1 listed pixels (adaptive
//                frames' refine pass, render_common.inc level0_px under RR_LISTED; namespace rr::listed), 2 a batch of
//                views (a table of cameras, level0_px / event_ray under RR_VIEWS; namespace rr::views)
// Included after the common headers and before the kernel .inc files: RR_LISTED / RR_VIEWS must not reach the headers.
// The unit then writes RR_UNIT_OPEN, its .inc files, one explicit instantiation <RR_UNIT_G, RR_UNIT_LC != 0> and
// RR_UNIT_CLOSE.  The production kernels stay as they are whatever the other sources add.
#if !defined(RR_UNIT_G) || !defined(RR_UNIT_LC) || !defined(RR_UNIT_SRC)
#error "a kernel-variant unit needs -DRR_UNIT_G=, -DRR_UNIT_LC= and -DRR_UNIT_SRC= (rray_amd/build.py UNITS)"
#endif
#if RR_UNIT_G < 0 || RR_UNIT_G > 2
#error "RR_UNIT_G: 0 (flat), 1 (groups) or 2 (general)"
#endif
#if RR_UNIT_LC < 0 || RR_UNIT_LC > 1
#error "RR_UNIT_LC: 0 (global culls) or 1 (LDS culls)"
#endif

#if RR_UNIT_SRC == 0
#define RR_UNIT_OPEN namespace rr {
#define RR_UNIT_CLOSE }
#elif RR_UNIT_SRC == 1
#define RR_LISTED 1
#define RR_UNIT_OPEN namespace rr { namespace listed {
#define RR_UNIT_CLOSE } }
#elif RR_UNIT_SRC == 2
#define RR_VIEWS 1
#define RR_UNIT_OPEN namespace rr { namespace views {
#define RR_UNIT_CLOSE } }
#else
#error "RR_UNIT_SRC: 0 (production), 1 (listed pixels) or 2 (views)"
#endif
