// kernels.hpp — host-visible launch interface of render.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>
#include <vector>

#include "persist_map.hpp"
#include "rr_device.hpp"
#include "wavefront.hpp"

namespace rr {

// One camera of a batch of views (LevelArgs.views): the camera and whether its inverse's row 3 is (0, 0, 0, 1)
// (LevelArgs.cam_affine of a single frame).
struct DevView {
    DevCamera cam;
    int32_t affine;
    int32_t pad;
};
// the table's records past the last view: a launch's last block may hold up to three waves past its events, which
// read their (unused) view's affine flag
constexpr int RR_VIEW_TABLE_PAD = 4;

// Arguments of one wavefront level (see wavefront.hpp).
struct LevelArgs {
    DevCamera cam;           // level-0 ray source (when rays0 == nullptr)
    int64_t hs;              // supersampled width
    int64_t lrows;           // part-local supersampled rows (level-0 camera rays run in 8x8 tiles)
    int32_t aa, part, nparts, block_rows;
    uint32_t aa_magic, br_magic;  // floor(2^32 / d) for d = aa, block_rows (>= 2; 0 when d == 1)
    int32_t tile_fast;       // level-0 tiles all full 8x8 and the batch tile-aligned: wave = one tile
    uint32_t tiles_per_row;  // hs / 8 (tile_fast)
    int32_t cam_affine;      // camera inverse row 3 == (0, 0, 0, 1)
    int64_t base;            // first local sample of this batch
    const double* rays0;     // level-0 explicit rays (o xyz, d xyz); nullptr: camera rays
    int32_t level, rem;      // level d and `remaining` = max_depth - d
    int64_t n;               // events at this level (n_dev == null) or this level's capacity (the grid)
    const unsigned int* n_dev;  // level >= 1: the live event count, written by the previous level's appends
    // segmented queues (fused levels, wavefront.hpp): this level's events are seg_count[s] events at
    // s * seg_cap (nseg > 1; level 0 has one segment), its children go to segment blockIdx % nseg_out of
    // the next level at s * seg_cap_out, counted in seg_out_count[s]
    int32_t nseg, nseg_out;
    int64_t seg_cap, seg_cap_out;
    const unsigned int* seg_count;
    unsigned int* seg_out_count;
    const Event* ev;         // level >= 1 input queue
    HitRec* hit;
    double* n12;
    CombRec* comb;           // this level's pending sums (indexed by event)
    CombRec* parent_comb;    // level - 1 (children deliver into their parent's slot)
    CombExt* comb_ext;       // refraction halves (null when no material is transparent)
    CombExt* parent_ext;
    ChainRec* chain[RR_MAX_DEPTH + 1];  // FUSED levels: each level's pending surface sums (in the comb buffers)
    double* out;             // level 0: canvas / color_at results (3 doubles per local sample), or null
    void* avg;               // aa == 1: the averaged image written directly (canvas.rs:85-96 with aa = 1)
    const float* tile_bundles;  // level 0, tile_fast, affine camera: per-tile camera-ray bundles (tile_bundle_kernel,
                                // RR_TILE_BUNDLE_FLOATS each, indexed by tile), or null: built in the walk
    // fused level 0 of a one-batch tile_fast frame (group scenes' kernels): the tile each wave renders (launch slot -> tile, the costliest
    // first: tile_order_kernel), or null (launch order); and where each wave stores its tile's cost in clock
    // cycles (or null).  The order changes only which wave renders which tile, never a result.
    const uint32_t* tile_perm;
    uint32_t* tile_cost;
    int32_t order_group;     // tile_perm's units: 1 (one wave's tile each) or 4 (a block's four tiles)
    int32_t pad_children;    // fused levels: children in per-wave 64-slot blocks (holes: Event.parent == -2)
    // chain kernels (chain_kernel): the deep queue (segmented like the fused levels' queues: the camera launch
    // appends to seg_out_count / seg_cap_out, the deep launch reads seg_count / seg_cap) and the depth at which
    // chains leave their camera wave for it (0: they never do)
    DeepRec* deep;
    int32_t deep_from;
    // pixel waves (aa == 3, chain kernels, render_common.inc pixel_wave): level-0 waves of 7 whole pixels, averaged in
    // the wave; pw_wpb waves per band of two output rows, pw_rows the part's output rows
    int32_t pw;
    uint32_t pw_wpb;
    int32_t pw_rows;
    int32_t aa_wave;         // 2 / 4 / 8: every pixel's aa x aa samples lie in one wave's 8x8 tile and no
                             // sample has a secondary ray: the wave box-averages and writes avg (0: off)
    int32_t avg_f32;         // avg holds floats (RR_OUT_AVG_F32)
    Event* next;
    int32_t* pending;        // this level's events with children
    int32_t* n1n2_list;
    unsigned int* lcount;    // LC_* (zeroed per level)
    uint64_t seed;
    int32_t jitter_mode;
    unsigned long long* counters;  // C_* totals
    unsigned long long* counters_zero;  // the next frame's counter buffer, zeroed by this frame's kernels (or null)
    // persistent level-0 loop (render_persist.inc; persist_map.hpp): the frame's tiles (0: the frame does not
    // qualify, per-tile launch), the number of queue heads (a power of two <= RR_CNT_SLOTS) and head 0 — head h is
    // persist_head[h * RR_CNT_STRIDE], the C_WORK word of counter slot h of this frame's buffer, zero at the frame's start
    uint32_t persist_tiles;
    uint32_t persist_heads;
    unsigned long long* persist_head;
    // listed pixels (adaptive frames' refine pass; the rr::listed kernels only, render_listed_*.hip): level-0 event i is
    // sample i % aa^2 (dy outer, dx inner) of output pixel list[i / aa^2] (row-major index into the list_w-wide
    // frame); n_dev holds the live event count (aa^2 x the listed pixels), the launch covers the capacity.  Last in
    // the struct, so that no other field moves in the kernels that never read them.
    // (with rays0, the rr::listed kernels read list as the order of an ordered ray batch instead, DESIGN.md §3.19: level-0
    // slot base + i works on ray list[base + i]; n_dev null and n the host's count, or — one batch, base 0, the indirect
    // frames' live list — n the capacity, n_dev the live count the kernels' live_count reads, and every one of the n
    // list slots a ray of the batch)
    const uint32_t* list;
    uint32_t list_w;
    // the flat fused level-0 kernels (shade_body.inc UH): the scalar path for hit-uniform tiles, planes' normals from
    // the table behind DevScene.nodes.  Set by their launches (render_levels.inc uniform_hit_on); RRAY_NO_UNIFORM_HIT=1
    // keeps the per-lane code, for tests and same-binary timing.  In the struct's tail padding: no field moves.
    uint32_t uniform_hit;
    // a batch of views (rr_render_views; the rr::views kernels only, render_views_*.hip): level-0 event i is event
    // i % view_e of view i / view_e of the pass, view_e = ceil(hs * lrows / 64) * 64 events per view, so a wave holds
    // samples of one view only and reads that view's camera with a wave-uniform index; hs x lrows is one view's
    // canvas.  At the struct's end: no other field moves.
    const DevView* views;
    uint32_t view_e;
};

struct CombArgs {
    int32_t level;
    int64_t n;                 // capacity of this level's pending list (sizes the grid)
    const unsigned int* n_dev; // the live pending count (LC_PENDING of the level)
    int64_t base;
    const int32_t* pending;
    const CombRec* comb;
    CombRec* parent_comb;
    const CombExt* comb_ext;  // as LevelArgs
    CombExt* parent_ext;
    double* out;  // level 0: canvas (3 doubles per local sample), or null
    void* avg;    // as LevelArgs
    int32_t avg_f32;
    int64_t hs, lrows;  // lrows > 0: level-0 events are in tile order (tile_to_local)
};

// The walking kernels' dynamic LDS (render_levels.inc): the scene's culls (when staged), then with <=
// RR_PRELIT_LIGHTS lights (PRE) every light's prelit terms ([light][6][256] doubles) and the area-light
// stage (scenes with an area light).
constexpr int RR_PRELIT_LIGHTS = 2;
constexpr size_t RR_AREA_STAGE_BYTES = 3 * 256 * 8 + 3 * 256 * 4;
constexpr size_t RR_CHAIN_STAGE_BYTES = 10 * 256 * 8 + 4 * 256 * 4;  // chain kernels: parked ray, level-0 record, Px0, own

// Level-0 camera events run in 8x8-sample tiles of the part-local supersampled canvas (8-row bands,
// 8-column tiles inside a band; the last band / column may be narrower) so that a wave's 64 rays
// form a tight bundle for the culling in walk_nodes.  Maps tile-order index t to the row-major
// local sample index (a bijection on [0, hs*lrows)).
__host__ __device__ inline int64_t tile_to_local(int64_t t, int64_t hs, int64_t lrows) {
    const int64_t band = t / (8 * hs);
    int64_t k = t - band * 8 * hs;
    const int64_t y0 = band * 8;
    const int64_t hb = lrows - y0 < 8 ? lrows - y0 : 8;
    const int64_t tc = k / (8 * hb);
    k -= tc * 8 * hb;
    const int64_t x0 = tc * 8;
    const int64_t wc = hs - x0 < 8 ? hs - x0 : 8;
    const int64_t dy = k / wc;
    return (y0 + dy) * hs + x0 + (k - dy * wc);
}
// the same in 32 bits (device: parts hold < 2^31 samples)
__host__ __device__ inline uint32_t tile_to_local_u32(uint32_t t, uint32_t hs, uint32_t lrows) {
    const uint32_t band = t / (8u * hs);
    uint32_t k = t - band * 8u * hs;
    const uint32_t y0 = band * 8u;
    const uint32_t hb = lrows - y0 < 8u ? lrows - y0 : 8u;
    const uint32_t tc = k / (8u * hb);
    k -= tc * 8u * hb;
    const uint32_t x0 = tc * 8u;
    const uint32_t wc = hs - x0 < 8u ? hs - x0 : 8u;
    const uint32_t dy = k / wc;
    return (y0 + dy) * hs + x0 + (k - dy * wc);
}

// Optional per-kernel timing: when `prof` is non-null every launch is bracketed by HIP events on
// the launch stream and appended to it (resolved on the host after a synchronise).
enum KernelId { K_TRACE = 0, K_N1N2, K_SHADE, K_SHADOW, K_FINISH, K_COMBINE, K_AA, K_TRACE_SHADE, K_CHAIN, K_DEEP, K_COUNT };
struct KernelProf {
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> marks;
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    hipEvent_t get();
};

hipError_t launch_level(const DevScene& S, const LevelArgs& A, hipStream_t stream, KernelProf* prof = nullptr);
// One camera-ray bundle per full 8x8 tile of the part (A: level-0 tile_fast arguments of the whole part), into
// out (n_tiles x RR_TILE_BUNDLE_FLOATS floats): exactly the bundle make_bundle's cam_tile path builds in the walk.
constexpr int RR_TILE_BUNDLE_FLOATS = 12;
hipError_t launch_tile_bundles(const DevScene& S, const LevelArgs& A, float* out, int64_t n_tiles, hipStream_t stream);
// the same per pixel wave (A.pw): the bundle of the wave's 12 x 6-sample footprint from its corner rays
hipError_t launch_pixel_wave_bundles(const LevelArgs& A, float* out, int64_t n_waves, hipStream_t stream);
// cost = a guess of each tile's cost from its camera bundle (the nodes of the chunks it may reach), for a layout's
// first frame, before any tile has been timed
hipError_t launch_tile_guess(const DevScene& S, const float* bundles, uint32_t* cost, int64_t n_tiles, hipStream_t stream);
// perm = tiles by decreasing recorded cost (LevelArgs.tile_cost), for the next frames' level-0 launches;
// scratch = 256 u32 of device memory (bucket counters)
constexpr int RR_ORDER_GROUP = 4;
// group: the sort's unit, 1 tile or RR_ORDER_GROUP consecutive tiles (one launch block's waves; perm then maps a launch
// block to a tile group)
hipError_t launch_tile_order(const uint32_t* cost, uint32_t* perm, uint32_t* scratch, int64_t n_tiles, int group,
                             hipStream_t stream);
// trace + shade run as one kernel per level (no transparent material, so no n1/n2 walk between them);
// those levels finish their reflection chains themselves and need no combine pass
bool fused_levels(const DevScene& S);
// The scene's kernel variant: G = 0 flat, 1 groups, 2 general (CSG, 4-entry leaves); LC = culls staged in LDS.
// dispatch_glc calls f(G, LC) with the pair as std::integral_constant values, so the callee names an instantiation:
//   dispatch_glc(S, [&](auto g, auto lc) { launch_level_t<g(), lc()>(S, A, st, prof); });
// Every launch_* that picks a <G, LC> instantiation goes through it.
template <class F>
inline void dispatch_glc(const DevScene& S, F&& f) {
    using std::integral_constant;
    const int g = S.general ? 2 : S.has_groups ? 1 : 0;
    if (g == 2)
        S.lds_culls ? f(integral_constant<int, 2>{}, std::true_type{}) : f(integral_constant<int, 2>{}, std::false_type{});
    else if (g == 1)
        S.lds_culls ? f(integral_constant<int, 1>{}, std::true_type{}) : f(integral_constant<int, 1>{}, std::false_type{});
    else
        S.lds_culls ? f(integral_constant<int, 0>{}, std::true_type{}) : f(integral_constant<int, 0>{}, std::false_type{});
}
// one (G, LC) variant of a level's kernels (render_levels.inc), instantiated in its own translation
// unit render_levels_g<G>_<lds|gl> (unit_levels.hip, compiled once per variant: build.py UNITS)
template <int G, bool LC>
void launch_level_t(const DevScene& S, const LevelArgs& A, hipStream_t stream, KernelProf* prof);
hipError_t launch_combine(const CombArgs& C, hipStream_t stream, KernelProf* prof = nullptr);
// Level-0 fused frames of flat scenes as one resident launch (render_persist.inc persist_kernel): the grid covers the
// GPU's resident capacity whatever the frame's size, and every wave loops over tiles it takes from the sharded queue
// A.persist_head.  persist_plan: the launch that serves (S, A) that way, decided once per launch (blocks 0: the
// per-tile launch_level) — A.persist_tiles set (api.cpp: one level, one batch, full tiles), a flat scene with global
// culls, at most RR_PRELIT_LIGHTS point lights and no complex pattern (the one kernel instantiated), not
// RRAY_NO_PERSIST=1, and at least as many tiles as resident wave slots unless RRAY_PERSIST_BLOCKS=n sets the grid.
// *resident caches the blocks the GPU holds at once for this scene (the caller's, per context and scene; < 0: not
// asked yet): the occupancy query runs once, and a launch costs two getenv reads on top of the per-tile one.
struct PersistPlan {
    int blocks;      // the grid; 0: per-tile launch
    uint32_t heads;  // queue heads in use: A.persist_heads, and no more than the grid has waves
};
PersistPlan persist_plan(const DevScene& S, const LevelArgs& A, int* resident);
hipError_t launch_persist(const DevScene& S, const LevelArgs& A, const PersistPlan& plan, hipStream_t stream,
                          KernelProf* prof);
// Fused scenes whose materials reflect: the whole reflection chain of every level-0 event inside its wave
// (render_levels.inc chain_kernel), one launch per batch with no recursion queues
bool chain_levels(const DevScene& S, int max_children, int max_depth);
template <int G, bool LC>
void launch_chain_t(const DevScene& S, const LevelArgs& A, hipStream_t stream, KernelProf* prof, bool deep);
// deep: the deep queue's launch (one block per segment, A.nseg segments), else the camera launch
hipError_t launch_chain(const DevScene& S, const LevelArgs& A, hipStream_t stream, KernelProf* prof = nullptr,
                        bool deep = false);
// Scenes with a transparent material: every camera sample's whole color_at tree (reflected and refracted children,
// shade_hit's sums) inside its camera lane with an explicit per-lane stack (render_tree.inc tree_kernel), one launch
// per batch with no recursion queues and no combine passes.  RRAY_NO_TREE=1 keeps the per-level kernels.
bool tree_levels(const DevScene& S);
template <int G, bool LC>
void launch_tree_t(const DevScene& S, const LevelArgs& A, hipStream_t stream, KernelProf* prof);
hipError_t launch_tree(const DevScene& S, const LevelArgs& A, hipStream_t stream, KernelProf* prof = nullptr);
hipError_t launch_aa(const double* canvas, double* out, int64_t width, int64_t rows, int32_t aa, hipStream_t stream,
                     KernelProf* prof = nullptr);
hipError_t launch_aa_f32(const double* canvas, float* out, int64_t width, int64_t rows, int32_t aa, hipStream_t stream,
                         KernelProf* prof = nullptr);
hipError_t launch_shadow_query(const DevScene& S, const double* pts, const double* lps, int64_t n, int32_t* out,
                               unsigned long long* counters, hipStream_t stream);

// Adaptive anti-aliasing (render_adapt.hip).  The refine pass renders the samples of a device-side
// list of pixels (LevelArgs.list) with the level kernels compiled a second time, in namespace rr::listed with
// RR_LISTED defined (the units render_listed_*_g<G>_<lds|gl>): the production instantiations above do not carry the listed
// source.  Every production dispatch is served: the fused level 0, the chain kernels and the tree kernels.
namespace listed {
template <int G, bool LC>
void launch_level_t(const DevScene& S, const LevelArgs& A, hipStream_t stream, KernelProf* prof);
template <int G, bool LC>
void launch_chain_t(const DevScene& S, const LevelArgs& A, hipStream_t stream, KernelProf* prof, bool deep);
template <int G, bool LC>
void launch_tree_t(const DevScene& S, const LevelArgs& A, hipStream_t stream, KernelProf* prof);
}  // namespace listed
hipError_t launch_level_listed(const DevScene& S, const LevelArgs& A, hipStream_t stream, KernelProf* prof = nullptr);
hipError_t launch_chain_listed(const DevScene& S, const LevelArgs& A, hipStream_t stream, KernelProf* prof = nullptr);
hipError_t launch_tree_listed(const DevScene& S, const LevelArgs& A, hipStream_t stream, KernelProf* prof = nullptr);
// Batches of views (rr_render_views): many cameras of one scene in one launch per pass.  The level,
// chain and tree kernels compiled a third time, in namespace rr::views with RR_VIEWS defined
// (the units render_views_{levels,chain,tree}_g<G>_<lds|gl>): level-0 events come from the camera table LevelArgs.views.
// The production and listed instantiations do not carry the source.  launch_*_views (render_views.hip) pick the
// scene's (G, LC) variant as launch_level / launch_chain / launch_tree do.
namespace views {
template <int G, bool LC>
void launch_level_t(const DevScene& S, const LevelArgs& A, hipStream_t stream, KernelProf* prof);
template <int G, bool LC>
void launch_chain_t(const DevScene& S, const LevelArgs& A, hipStream_t stream, KernelProf* prof, bool deep);
template <int G, bool LC>
void launch_tree_t(const DevScene& S, const LevelArgs& A, hipStream_t stream, KernelProf* prof);
}  // namespace views
hipError_t launch_level_views(const DevScene& S, const LevelArgs& A, hipStream_t stream, KernelProf* prof = nullptr);
hipError_t launch_chain_views(const DevScene& S, const LevelArgs& A, hipStream_t stream, KernelProf* prof = nullptr);
hipError_t launch_tree_views(const DevScene& S, const LevelArgs& A, hipStream_t stream, KernelProf* prof = nullptr);
// The passes around the adaptive refine pass, all on the caller's stream with their counts in HBM:
//   mask     rule: pixel p is refined iff some q of its clipped 3x3 neighbourhood has !(max_c |F[p][c] - F[q][c]| <= thr);
//            writes flags (and mask, when not null) and one count per block of RR_ADAPT_BLOCK pixels
//   scan     exclusive scan of the block counts (in place); n_list = refined pixels, n_events = n_list * aa^2,
//            n_refined (int64, or null) = n_list
//   scatter  list = the refined pixels' indices in ascending raster order (ballot + popcount inside the wave)
//   resolve  per listed pixel: r = 0.0; r += sample (dy outer, dx inner); avg[p] = r / (double)(aa * aa)
constexpr int RR_ADAPT_BLOCK = 256;
struct AdaptArgs {
    const double* frame;  // the aa 1 frame (3 doubles per pixel), overwritten at the listed pixels by resolve
    int64_t w, h;
    int32_t aa;
    double thr;
    uint8_t* flags;         // w * h
    uint8_t* mask;          // the caller's, or null
    uint32_t* block_count;  // ceil(w * h / RR_ADAPT_BLOCK): counts, then exclusive offsets
    uint32_t* counts;       // [0] n_list, [1] n_events
    int64_t* n_refined;     // the caller's, or null
    uint32_t* list;         // w * h
    const double* samples;  // the refine pass's colours: 3 doubles per level-0 event
    double* avg;            // == frame
};
hipError_t launch_adapt_select(const AdaptArgs& P, hipStream_t stream);   // mask, scan, scatter
hipError_t launch_adapt_resolve(const AdaptArgs& P, hipStream_t stream);

// hit_kernel (render_hit.inc): hit() + prepare_computations of one ray per lane (scene.rs:128-136,
// intersection.rs:50-92), no shading.  The rays are a level's level-0 rays: the camera's samples in 8x8 tiles
// (A.rays0 == null: an AOV frame, rr_render_aov) or a caller's batch (A.rays0: rr_hit_at).  Not a KernelId: it is
// timed by the frame's event pair only.
struct HitOut {
    const int32_t* node_object;  // node index -> rr_scene_desc object id (the context's table, built at upload)
    // camera samples: the requested planes, row-major over the part's supersampled canvas (null: not requested)
    double* depth;    // t, +inf on a miss
    double* normal;   // 3 per sample: normalv
    int32_t* object;  // object id, -1 on a miss
    double* albedo;   // 3 per sample: material_color at over_point
    // ray batches: the rr_hit fields as planes of `stride` entries each — ints {object, inside}, doubles {t, u, v,
    // point, eyev, normalv, over_point, under_point, reflectv (3 each), n1, n2} (RR_HIT_DOUBLES planes)
    int32_t* rec_i;
    double* rec_d;
    int64_t stride;
};
constexpr int RR_HIT_DOUBLES = 23;
template <int G, bool LC>
void launch_hit_t(const DevScene& S, const LevelArgs& A, const HitOut& O, hipStream_t stream);
hipError_t launch_hit(const DevScene& S, const LevelArgs& A, const HitOut& O, hipStream_t stream);
// First-hit planes of a batch of views (rr_render_views_aov): hit_kernel's camera variants compiled
// once more in namespace rr::views (the units render_views_hit_g<G>_<lds|gl>).  One pass of whole views per launch: A.views
// and O's planes start at the pass's first view, A.n = the pass's views * A.view_e, A.base 0, no cached bundles.
namespace views {
template <int G, bool LC>
void launch_hit_t(const DevScene& S, const LevelArgs& A, const HitOut& O, hipStream_t stream);
}  // namespace views
hipError_t launch_hit_views(const DevScene& S, const LevelArgs& A, const HitOut& O, hipStream_t stream);

// Device-resident ray queries (render_rays.hip).
// camera_rays_kernel: the n = cam.hsize * cam.vsize (< 2^32) rays of a camera, row-major, six doubles each (origin,
// direction: LevelArgs.rays0's layout), by the frames' camera_ray on the frames' DevCamera / affine flag (api.cpp
// set_camera).
hipError_t launch_camera_rays(const DevCamera& cam, bool affine, int64_t n, double* out, hipStream_t stream);
// hit_records_kernel: the first n entries of hit_kernel's ray-batch planes (O.rec_i / O.rec_d, O.stride entries per
// plane) as n rr_hit records at `out`; n <= 2^24 (one pass of rr_hit_at_device holds at most 2^22).
hipError_t launch_hit_records(const HitOut& O, int64_t n, void* out, hipStream_t stream);

// Ordered ray batches (render_order.inc in render_rays.hip).
// launch_ray_order: perm = argsort(key, stable) of the n (< 2^32) rays at `rays` (six doubles each), key the 32-bit
// origin-major Morton code of rray_amd.ray_order_keys (bounds over the batch's valid rays, then 6 + 6 + 6 origin bits
// over 7 + 7 octahedral direction bits; 0xFFFFFFFF for a ray with a non-finite component or no direction).  Five kernels
// and four 8-bit stable radix passes, all on `stream`.  scratch: ray_order_scratch_bytes(n) bytes the call owns while it runs.
size_t ray_order_scratch_bytes(int64_t n);
hipError_t launch_ray_order(const double* rays, int64_t n, uint32_t* perm, void* scratch, hipStream_t stream);
// the first-hit kernel's ray-batch instantiation with the listed source (in the units render_listed_levels_g<G>_<lds|gl>): slot j
// of the pass (A.base 0, A.n slots) works on ray A.rays0[A.list[j]] and writes its planes at slot j
namespace listed {
template <int G, bool LC>
void launch_hit_t(const DevScene& S, const LevelArgs& A, const HitOut& O, hipStream_t stream);
}  // namespace listed
hipError_t launch_hit_ordered(const DevScene& S, const LevelArgs& A, const HitOut& O, hipStream_t stream);
// hit_records_kernel with a scattered destination: the record of pass slot j goes to out + 192 * perm[j], whole
hipError_t launch_hit_records_ordered(const HitOut& O, int64_t n, const uint32_t* perm, void* out, hipStream_t stream);

// Lens frames (render_lens.inc in render_rays.hip; the definition is rray.h's RR_HAS_LENS block).
// What lens_rays_kernel reads of the camera and the lens: the affine rows of the frames' camera inverse (api.cpp
// set_camera), the image plane, the lens and the frame's geometry.  A kernel argument of its own, never part of LevelArgs.
struct DevLens {
    double inv[12];  // rows 0..2 of DevCamera.inv (row 3 is 0, 0, 0, 1: host-checked)
    double half_width, half_height, pixel_size;
    double aperture, focal_distance;
    uint64_t seed;
    uint32_t samples, width;  // S and W; ray i is sample i % S of pixel i / S, pixel p at (p % W, p / W)
    int32_t pixel_jitter, pad;
};
// lens_rays_kernel: the rays [first_ray, first_ray + n) of the frame (first_ray + n <= 2^32), ray first_ray + j at
// out + 6 * j
hipError_t launch_lens_rays(const DevLens& L, int64_t first_ray, int64_t n, double* out, hipStream_t stream);
// lens_resolve_kernel: out[p] = (((c[p*S] + c[p*S + 1]) + ...) + c[p*S + S - 1]) / (double)S per channel, p < n_pixels
hipError_t launch_lens_resolve(const double* colours, int32_t samples, int64_t n_pixels, double* out, hipStream_t stream);

// Ambient occlusion (render_ao.inc in render_rays.hip; the definition is rray.h's RR_HAS_AO block).
// The rr_ao parameters as ao_pairs_kernel reads them: a kernel argument of their own, never part of LevelArgs or DevScene.
struct DevAo {
    double radius;
    uint64_t seed;
    uint32_t samples, pad;  // K
};
// Where the points and unit normals of a launch lie: component r of point i at points[i * point_stride + r *
// comp_stride] (normals alike) — (3, 1) for the caller's n x 3 arrays (rr_ao_at_device), (1, plane stride) for the
// over_point / normalv planes of hit_kernel's ray-batch records (HitOut.rec_d; rr_render_ao_device).  object: the
// records' object plane (a point with object < 0 is a miss and takes part in no walk), or null: every point is
// evaluated.  first: the hash index of point 0 (its index in the batch or the frame).
struct AoPoints {
    const double* points;
    const double* normals;
    int64_t point_stride, comp_stride;
    const int32_t* object;
    int64_t first;
};
// ao_pairs_kernel: count[i] = the occluded ones of point i's K segments, i < n (n * K < 2^32); the walks' counters go
// to `counters` (shadow rays: K per evaluated point).  Clears count first when K does not divide 64.
hipError_t launch_ao_pairs(const DevScene& S, const DevAo& P, const AoPoints& I, int64_t n, int32_t* count,
                           unsigned long long* counters, hipStream_t stream);
// camera_rays_window_kernel: rays [first, first + n) of launch_camera_rays' batch (first + n <= hsize * vsize < 2^32),
// ray first + j at out + 6 * j, by the same camera_ray: one pass of an occlusion frame
hipError_t launch_camera_rays_window(const DevCamera& cam, bool affine, int64_t first, int64_t n, double* out,
                                     hipStream_t stream);
// ao_resolve_kernel: out[i] = (double)(K - count[i]) / (double)K, i < n
hipError_t launch_ao_resolve(const int32_t* count, int32_t samples, int64_t n, double* out, hipStream_t stream);

// One-bounce indirect light (render_indirect.inc in render_rays.hip; the definition is rray.h's
// RR_HAS_INDIRECT block).  The rr_indirect parameters as indirect_rays_kernel reads them (`remaining` is the trace's).
struct DevIndirect {
    uint64_t seed;
    uint32_t samples, pad;  // K
};
// indirect_rays_kernel over n points in AoPoints' form (I.first: the hash index of point 0; (I.first + n) * K < 2^32):
// ray (I.first + i) * K + k at rays + 6 * (i * K + k).  list null (the point query): every point is evaluated and
// I.object is not read.  list non-null (the frames; I.object required): the pairs of a miss write no ray, and
// list[0 .. live) holds the global indices (I.first + i) * K + k of the other pairs in increasing order and
// list[live .. n * K) the pass's first ray index (slots a launch for the capacity may read but never trace); block_count
// (one uint32 per 256 pairs) is scratch, counts[0] = live and counts[1 + b] = the live entries among list slots
// [b * chunk, (b + 1) * chunk), b < ceil(n * K / chunk): all computed on the device, nothing waits.
hipError_t launch_indirect_rays(const DevIndirect& P, const AoPoints& I, int64_t n, double* rays, uint32_t* list,
                                uint32_t* block_count, uint32_t* counts, int64_t chunk, hipStream_t stream);
// indirect_resolve_kernel: out[i] = (((c[i*K] + c[i*K + 1]) + ...) + c[i*K + K - 1]) / (double)K per channel, i < n;
// object non-null: zeros where object[i] < 0, whose colours are not read
hipError_t launch_indirect_resolve(const double* colours, const int32_t* object, int32_t samples, int64_t n, double* out,
                                   hipStream_t stream);

// The edge-avoiding denoiser (render_denoise.inc in render_rays.hip; the definition is rray.h's
// RR_HAS_DENOISE block, its arithmetic denoise_tap.hpp's).
struct DnGuide;
struct DnLevel;
// denoise_pack_kernel: guides[p] = dn_guide(p, ...) for p < n (n < 2^31); a null plane packs as zeros
hipError_t launch_denoise_pack(int64_t n, const double* depth, const double* normal, const int32_t* object,
                               const double* albedo, DnGuide* guides, hipStream_t stream);
// denoise_level_kernel<channels>: dst = one level of the filter over src (W x H x channels doubles, channels 1 or 3,
// W * H < 2^31, src != dst) with the records of launch_denoise_pack.  lds: levels with holes of 1 or 2 pixels run
// denoise_level_lds_kernel (tile and halo staged in LDS; the same result bit for bit), wider ones the direct kernel.
constexpr int RR_DN_LDS_MAX_STEP = 2;
hipError_t launch_denoise_level(const DnLevel& L, bool lds, int32_t channels, int64_t W, int64_t H, const double* src,
                                const DnGuide* guides, double* dst, hipStream_t stream);

// Variance-guided denoising (render_denoise_var.inc in render_rays.hip; the definition is rray.h's
// RR_HAS_DENOISE_VAR block, its arithmetic denoise_var_tap.hpp's).  Both read the records of launch_denoise_pack.
// variance_kernel<channels>: var[p] = dv_variance of every pixel of `in` (W x H x channels doubles, channels 1 or 3,
// W * H < 2^31).  G: dv_guide_level(terms, 1, ...); m2 and count: rr_temporal's planes, both or neither.
hipError_t launch_variance(const DnLevel& G, int32_t min_history, int32_t channels, int64_t W, int64_t H, const double* in,
                           const double* m2, const int32_t* count, const DnGuide* guides, double* var, hipStream_t stream);
// denoise_var_level_kernel<channels>: dst and vdst = one level of the filter over src and vsrc (src != dst, vsrc !=
// vdst; vdst may be null: the level's variance is not stored).  L: dv_level(...).
hipError_t launch_denoise_var_level(const DnLevel& L, double epsilon, int32_t channels, int64_t W, int64_t H,
                                    const double* src, const double* vsrc, const DnGuide* guides, double* dst, double* vdst,
                                    hipStream_t stream);

// Temporal accumulation (render_temporal.inc in render_rays.hip; the definition is rray.h's
// RR_HAS_TEMPORAL block, its arithmetic temporal_tap.hpp's).
struct TpConst;
struct TpFrame;
// temporal_kernel<channels, m2_out != null, tile width>: out, n_out and m2_out of every pixel of a K.W x K.H frame
// (W * H < 2^31, channels 1 or 3; every plane a term of K.terms reads must be given).  rows: the row-major lane map
// (a block is 256 x 1 pixels) instead of the 32 x 8 tile; the same result bit for bit.
hipError_t launch_temporal(const TpConst& K, int32_t channels, const TpFrame& cur, const TpFrame& prev, bool rows,
                           double* out, int32_t* n_out, double* m2_out, hipStream_t stream);

}  // namespace rr
