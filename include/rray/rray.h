/*
 * rray.h — C ABI of the MI355X (gfx950) render path for davelpz/rray.
 *
 * Drop-in boundary for the reference's per-pixel render loop:
 *   Camera::render(&self, &Scene) -> Canvas        src/raytracer/camera.rs:107-121
 *     -> Scene::color_at / intersect / shade_hit / is_shadowed / reflected_color /
 *        refracted_color                           src/raytracer/scene.rs:97-336
 *     -> Object::intersect (+ local_intersect)     src/raytracer/object.rs:45-48
 * and its YAML/CLI front-end
 *   render_scene_from_file(path, w, h, png, aa)    src/raytracer/scene_builder_yaml.rs:429-436
 *
 * Everything is extern "C" with plain pointers and sizes so a Rust host binds it with
 * an `extern "C"` block.  Return codes: 0 = OK, < 0 = error
 * (the reference's panics, scene_builder_yaml.rs / db.rs, become codes); the message is
 * available from rr_last_error().  Never aborts or throws across the ABI.
 *
 * There is no CPU fallback: every render entry point runs the HIP kernels and fails with
 * RR_E_HIP when no gfx950 device is usable.
 */
#ifndef RRAY_RRAY_H
#define RRAY_RRAY_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RR_ABI_VERSION 11

/* error codes */
#define RR_OK 0
#define RR_E_ARG (-1)        /* invalid argument / inconsistent descriptor */
#define RR_E_HIP (-2)        /* HIP runtime error (no device, launch failure, ...) */
#define RR_E_SCENE (-3)      /* scene the reference would panic on (scene_builder_yaml.rs) */
#define RR_E_NONAFFINE (-4)  /* inverse transform with row 3 != (0,0,0,1) */
#define RR_E_LIMIT (-5)      /* exceeds a compiled limit (depth, pattern nesting) */
#define RR_E_IO (-6)         /* file missing / unreadable / unwritable */
#define RR_E_NAN (-7)        /* NaN intersection t in a list of >= 2 entries: the reference panics in
                                Vec::sort_by(partial_cmp().unwrap()) (scene.rs:104, group.rs:88, csg.rs:231).
                                rr_render / rr_color_at return it after writing their outputs; for
                                rr_render_device see rr_stats.nan_rays. */

/* object kinds — Sphere, Plane, Group, Triangle, SmoothTriangle, Cube, Cylinder, Cone, Csg, Torus
 * (src/raytracer/object/) */
enum { RR_SPHERE = 0, RR_PLANE = 1, RR_GROUP = 2, RR_TRIANGLE = 3, RR_SMOOTH_TRIANGLE = 4,
       RR_CUBE = 5, RR_CYLINDER = 6, RR_CONE = 7, RR_CSG = 8, RR_TORUS = 9 };
/* CSG operations — CsgOperation (csg.rs:13-17) */
enum { RR_CSG_UNION = 0, RR_CSG_INTERSECTION = 1, RR_CSG_DIFFERENCE = 2 };
/* pattern kinds — PatternType (src/raytracer/material/pattern.rs:10-21), in-scope subset */
enum { RR_PAT_TEST = 0, RR_PAT_SOLID = 1, RR_PAT_STRIPE = 2, RR_PAT_GRADIENT = 3,
       RR_PAT_RING = 4, RR_PAT_CHECKER = 5, RR_PAT_BLEND = 6, RR_PAT_PERTURBED = 7, RR_PAT_NOISE = 8,
       RR_PAT_TEXTURE = 9 /* pat_a = texture index */ };
/* light kinds — LightType (src/raytracer/light.rs:10-14) */
enum { RR_LIGHT_POINT = 0, RR_LIGHT_AREA = 1 };

#define RR_MAX_DEPTH 8          /* max `remaining` (render uses 5, camera.rs:113) */
#define RR_MAX_GROUP_DEPTH 6    /* nested group levels */
#define RR_MAX_AREA_LEVEL 1024  /* area light `level` (level^2 jittered samples per shading event; the
                                   reference takes any usize, scene_builder_yaml.rs:137).  Bound by the
                                   kernels' cell arithmetic: (col + u) / level is the proven shared-divisor
                                   quotient (tests/test_division.py, every level 1..1024) and the cell index
                                   s < level^2 <= 2^20 fits the jitter key's 20-bit field.  The YAML front-end
                                   and rr_scene_upload both refuse larger levels (RR_E_LIMIT / RR_E_SCENE). */
#define RR_MAX_PATTERN_DEPTH 8  /* nested pattern levels */
#define RR_MAX_CSG_ENTRIES 32   /* intersections one CSG subtree can produce for one ray */
#define RR_MAX_OCTAVES 64       /* octave_perlin octaves (noise.rs:11-29) */

/*
 * The scene exactly as the reference's object registry holds it (object/db.rs:11-13 +
 * Scene{light, ids}, scene.rs:24-27).  All arrays are caller-owned and copied by
 * rr_scene_upload.  Object ids index every per-object array.
 */
typedef struct {
    int32_t n_objects;
    const int32_t* kind;         /* RR_SPHERE.. per object */
    const int32_t* parent;       /* parent group id or -1 (Object::get_parent_id) */
    const double* transform;     /* n_objects x 16, row-major (Matrix.data, matrix.rs:20-25) */
    const double* inverse;       /* optional n_objects x 16; NULL: computed like matrix.rs:389-412 */
    const int32_t* material;     /* material index per object (ignored for groups) */
    const double* tri;           /* n_objects x 18: p1,p2,p3,n1,n2,n3 (triangles; NULL if none) */
    const int32_t* child_start;  /* per object: offset into children[] (groups) */
    const int32_t* child_count;  /* per object: number of children (Group.child_ids order) */
    const int32_t* children;
    int32_t n_top;               /* Scene.ids (tie-break order of the stable sort) */
    const int32_t* top;

    int32_t n_materials;         /* Material (material.rs:35-44) */
    const double* mat;           /* n_materials x 7: ambient, diffuse, specular, shininess,
                                    reflective, transparency, refractive_index */
    const int32_t* mat_pattern;  /* root pattern per material */

    int32_t n_patterns;          /* Pattern tree nodes (pattern.rs:23-27) */
    const int32_t* pat_kind;
    const int32_t* pat_a;        /* child pattern ids (-1 if none) */
    const int32_t* pat_b;
    const double* pat_color;     /* n_patterns x 3 (Solid) */
    const double* pat_scale;     /* n_patterns (Blend) */
    const double* pat_transform; /* n_patterns x 16 */

    int32_t n_lights;            /* Light (light.rs:17-21) */
    const int32_t* light_kind;
    const double* light;         /* n_lights x 15: position, intensity, corner, u, v */
    const int32_t* light_level;  /* area light sample level (light.rs:13) */

    /* ABI 3 */
    const double* shape;         /* optional n_objects x 3: minimum, maximum, closed (cylinder.rs:29-37,
                                    cone.rs:30-38); NULL: -inf, +inf, open.  Torus (ABI 4):
                                    shape[0] = minor_radius (torus.rs:23-31; major radius 1) */
    const int32_t* csg_op;       /* optional per object: RR_CSG_* (CSG objects; their two children,
                                    left then right, are the group child lists) */
    /* ABI 4: Perturbed / Noise patterns (pattern.rs:16-19); pat_scale is their scale, pat_a the
       perturbed pattern, pat_a / pat_b the noise's two sub-patterns */
    const int32_t* pat_octaves;      /* optional per pattern (`usize`, <= RR_MAX_OCTAVES); NULL: 1 */
    const double* pat_persistence;   /* optional per pattern; NULL: 1.0 */
    /* ABI 4: image textures (texture.rs:6-11, Texture::new decodes + to_rgba8) */
    int32_t n_textures;
    const int32_t* tex_size;         /* n_textures x 2: width, height (>= 1 each) */
    const uint8_t* texels;           /* RGBA8 rows top to bottom, textures back to back */
} rr_scene_desc;

/* Camera (camera.rs:18-27): hsize/vsize are the SUPERSAMPLED sizes (W*aa, H*aa). */
typedef struct {
    int64_t hsize, vsize;
    double field_of_view, pixel_size, half_width, half_height;
    double transform[16];
} rr_camera;

/* render options */
typedef struct {
    int32_t aa;            /* anti-aliasing level; camera sizes are W*aa x H*aa */
    int32_t max_depth;     /* reflect/refract recursion budget (5 in camera.rs:113) */
    uint64_t seed;         /* area-light jitter seed (replaces thread_rng, light.rs:57-59) */
    int32_t jitter_mode;   /* 0 = counter hash jitter, 1 = cell centre */
    int32_t part, nparts;  /* row sharding: output rows y with (y/block_rows)%nparts == part */
    int32_t block_rows;    /* rows per interleaved block (default 8) */
    int32_t flags;         /* RR_OUT_* */
    /* ABI 10: a contiguous band of output rows [row_begin, row_end) instead of an interleaved part (part 0 of 1
       only; row_begin == row_end == 0: no band, and any other pair with row_end <= row_begin is refused).  Rows, pixels and the area-light jitter are the full frame's, so a band equals
       those rows of the whole frame bit for bit. */
    int32_t row_begin, row_end;
} rr_render_opts;
#define RR_OUT_CANVAS 1    /* write the supersampled canvas (Canvas.pixels layout) */
#define RR_OUT_AVG 2       /* write the AA-averaged image (canvas.rs:76-96, before `as u8`) */
#define RR_OUT_AVG_F32 4   /* rr_render_device only: the AA-averaged image rounded to float (3 floats per
                              pixel; the average itself is computed in f64) — compact tiles for gathers */
#define RR_NO_FRAME_TIMING 8 /* rr_render_device only: no HIP event pair around the frame (each event
                                record costs the stream a few microseconds); rr_stats.kernel_ms is 0 */
#define RR_PART_INTERLEAVE 16 /* ABI 10, multi-device contexts: interleaved row tiles, a staging buffer and placement
                                 kernels on rank 0 (the ABI 9 transfer) instead of cost-balanced bands */

typedef struct {
    uint64_t rays;          /* closest-hit rays (primary + reflected + refracted) */
    uint64_t shadow_rays;   /* is_shadowed rays */
    uint64_t shade_events;  /* shade_hit calls */
    uint64_t n1n2_scans;    /* prepare_computations container walks (transparent hits) */
    uint64_t group_tests, group_hits;
    uint64_t samples;       /* pixel x AA samples rendered */
    uint64_t prim_tests;    /* exact f64 leaf tests executed (lane-level, after culling) */
    double kernel_ms;       /* render + AA kernels, HIP events (0 with RR_NO_FRAME_TIMING) */
    uint64_t exact_flops[3];  /* f64 flops of those tests (SURVEY §8d model) per walk: trace, shadow, n1n2 */
    uint64_t wave_visits[3];  /* wave-level node visits (exact test issued for a 64-lane wave), same order */
    /* ABI 6: rays whose intersection list (as far as the walk computed it) held a NaN t among >= 2
       entries — where the reference panics; > 0 makes rr_render return RR_E_NAN */
    uint64_t nan_rays;
} rr_stats;

typedef struct rr_ctx rr_ctx;
typedef struct rr_scene rr_scene;

/* ---- library ---- */
int32_t rr_abi_version(void);
const char* rr_last_error(void);            /* thread-local message of the last failure */
int rr_device_count(int* out);

/* ---- context: one device, one stream (not thread-safe; one render at a time) ---- */
int rr_create(int device, rr_ctx** out);
void rr_destroy(rr_ctx* ctx);
/* flattens (DFS order, 3x4 inverses, group AABBs) and uploads to HBM (scene.rs, group.rs);
 * a multi-device context replicates the scene to every device */
int rr_scene_upload(rr_ctx* ctx, const rr_scene_desc* desc);

/* ---- multi-device contexts (ABI 5): one frame across several GPUs (camera.rs:107-121 spreads one
 * frame over every rayon worker).  ABI 10 default: global rank r renders a contiguous band of output rows
 * [bounds[r], bounds[r+1]) as an f64 AA-averaged tile; the bands are balanced by cost on the first frame of a
 * layout (rank 0 renders that frame once as 64 timed bands, rr_balance_bands, and broadcasts the bounds to every
 * rank: one ncclBroadcast per layout), and rank 0's band is kept lighter by its own transfer work.  One RCCL group
 * per frame (over xGMI): every other rank sends its tile to rank 0 in one ncclSend, which rank 0 receives straight
 * into the frame's rows; rank 0 copies its own tile there.  No staging buffer, no placement kernel.
 * With RR_PART_INTERLEAVE (the ABI 9 transfer): rank r renders the output rows {y : (y/block_rows) % N == r};
 * every rank sends its whole tile to rank 0 in one ncclSend, and rank 0 receives every part's tile (its own from
 * itself) back to back into a staging buffer of `height` rows, one ncclRecv per part (part p at row
 * rr_stage_row_offset); one copy kernel per part then places the tile's rows into their frame rows.  The context
 * owns a render and a transfer stream per device and the RCCL communicator.  rr_render (blocking; out_avg filled on rank 0 only) and
 * rr_render_gather_device (asynchronous) take part 0 of 1: the context does the split.  Only the
 * f64 averaged image is produced (no RR_OUT_CANVAS / RR_OUT_AVG_F32).  rr_color_at / rr_is_shadowed /
 * rr_kernel_times act on the context's first local device; rr_last_stats sums its local devices. */
#define RR_RCCL_ID_BYTES 128
/* this process drives n devices (ncclCommInitAll); images are bit-identical to one device's */
int rr_create_multi(int n_devices, const int* device_ids, rr_ctx** out);
/* one process per GPU: rank 0 makes an id with rr_rccl_unique_id, the host shares it (any channel),
 * every rank calls rr_create_rank with it (ncclCommInitRank; collective) */
int rr_rccl_unique_id(uint8_t* out, int32_t n_bytes);
int rr_create_rank(int device, int nranks, int rank, const uint8_t* unique_id, rr_ctx** out);
/* nranks in the group, this context's first global rank, devices this context drives (1/0/1 for rr_create) */
int rr_context_info(const rr_ctx* ctx, int32_t* nranks, int32_t* rank, int32_t* ndevices);
/* ABI 7: nparts VIRTUAL ranks on one device — the N > 1 path of a real group (per-part contexts and
 * streams, tiles, double buffering, the staging buffer at the same per-part offsets and the same placement
 * kernels) with only the ncclSend / ncclRecv pairs replaced by device-local copies of each tile into the
 * staging buffer.  For exercising / testing the multi-GPU frame assembly on one GPU; images are
 * bit-identical to one part's. */
int rr_create_virtual(int device, int nparts, rr_ctx** out);
/* ABI 10: band bounds from per-row costs: bounds[0] = 0 <= bounds[1] <= ... <= bounds[nparts] = height, every inner
 * bound a multiple of `align`, such that part p's cost sum(row_cost[bounds[p] .. bounds[p+1]-1]) (plus root_extra
 * for part 0, the same unit) is as even as the alignment allows.  Host only.  Returns RR_OK. */
int rr_balance_bands(const double* row_cost, int64_t height, int32_t nparts, double root_extra, int32_t align,
                     int64_t* bounds);
/* ABI 10: the band bounds of a multi-device context (nranks + 1 values; n >= nranks + 1) once its first band frame
 * has calibrated them, and rr_group_set_bands to impose bounds (every rank the same; skips the calibration until the
 * frame layout changes).  rr_group_bands returns the number of bounds written (0: not calibrated yet). */
int rr_group_bands(rr_ctx* ctx, int64_t* bounds, int32_t n);
int rr_group_set_bands(rr_ctx* ctx, const int64_t* bounds, int32_t n);
/* ABI 9: first row of part `part`'s tile in the staging buffer (the rows of parts 0 .. part-1; partition.hpp
 * stage_row_offset).  part == nparts gives height. */
int64_t rr_stage_row_offset(int64_t height, int32_t part, int32_t nparts, int32_t block_rows);
/* ABI 9 (was ABI 7 with padded tiles): the frame from tiles a caller transferred itself (e.g. torch.distributed
 * send / recv; the same layout and run arithmetic as the device transfer): staged = the nparts tiles back to back,
 * unpadded, part p's rows (increasing y) at row rr_stage_row_offset(height, p, nparts, block_rows), height rows of
 * width*3 doubles in all -> frame = height rows in frame order.  No device needed (CPU rehearsals of the N > 1 path
 * use it).  The buffers are not checked: both must hold height * width * 3 doubles (rray_amd.unshuffle checks its
 * array's shape before the call). */
int rr_unshuffle_host(const double* staged, double* frame, int64_t width, int64_t height, int32_t nparts,
                      int32_t block_rows);
/* ABI 8: build provenance — the sha256 prefix of the product sources this library was built from
 * (rray_amd/build.py source_digest(): rray_amd/csrc/*, this header, the build script).  Static string. */
const char* rr_build_digest(void);
/* Whole frame -> d_frame (W*H*3 doubles on rank 0's device; ignored on other ranks), enqueued after
 * the work already on `hip_stream` (NULL: no ordering with the caller) and completed in its order;
 * not synchronised.  Collective: every rank calls it for every frame.  Tiles are double-buffered, so
 * frame k+1 renders while frame k is being gathered.  On a single-device context it is
 * rr_render_device(d_avg = d_frame). */
int rr_render_gather_device(rr_ctx* ctx, const rr_camera* cam, const rr_render_opts* opts, void* d_frame,
                            void* hip_stream);

/* Camera::new (camera.rs:41-63) */
int rr_camera_new(int64_t hsize, int64_t vsize, double field_of_view, const double transform[16], rr_camera* out);

/* Camera::render (camera.rs:107-121).  Host buffers:
 *   out_canvas: hsize*vsize_part*3 doubles (RR_OUT_CANVAS) — identical layout to Canvas.pixels;
 *   out_avg:    W*rows_part*3 doubles (RR_OUT_AVG).
 * Rows are this part's rows in increasing order (see rr_part_rows).  Blocking. */
int rr_render(rr_ctx* ctx, const rr_camera* cam, const rr_render_opts* opts, double* out_canvas, double* out_avg,
              rr_stats* stats);
/* Same, into DEVICE buffers on the context's device, enqueued on `hip_stream` (NULL: ctx stream)
 * and NOT synchronised — for collectives that consume the tile straight from HBM.  d_avg holds
 * doubles, or floats with RR_OUT_AVG_F32. */
int rr_render_device(rr_ctx* ctx, const rr_camera* cam, const rr_render_opts* opts, void* d_canvas, void* d_avg,
                     void* hip_stream);
/* AA-averaged rows owned by `part` of `nparts` (interleaved blocks of block_rows output rows). */
int64_t rr_part_rows(int64_t height, int32_t part, int32_t nparts, int32_t block_rows, int64_t* rows_out);
/* Per-kernel HIP-event timing on the context's stream.  rr_kernel_profile(ctx, 1) resets and enables
 * it; rr_kernel_times fills accumulated milliseconds and launch counts per kernel in the order
 * trace, n1n2, shade, shadow, finish, combine, aa, trace_shade, chain, deep (returns the number of kernels,
 * 10; the shadow walks and the light sum run inside shade, so shadow and finish stay 0; scenes without
 * transparent materials run trace and shade as one trace_shade kernel, and those whose materials reflect run
 * every reflection chain in one chain kernel — deep only with RRAY_DEEP=1). */
int rr_kernel_profile(rr_ctx* ctx, int enable);
int rr_kernel_times(rr_ctx* ctx, double* ms, uint64_t* launches, int32_t n);
/* How the last rr_render_device / rr_render_adaptive_device frame on this context launched its level-0 kernel
 * (additive, ABI 11; no synchronisation): *blocks is the grid of the resident tile-loop launch and *heads the
 * queue heads it used, both 0 when the frame ran the per-tile launch (or launched nothing).  Either may be NULL. */
int rr_resident_launch(rr_ctx* ctx, int32_t* blocks, int32_t* heads);
/* stats of the last rr_render/rr_render_device on this context (synchronises) */
int rr_last_stats(rr_ctx* ctx, rr_stats* stats);

/* Scene::color_at (scene.rs:128-136) for a batch of rays (rr_color_at), and
 * Scene::is_shadowed (scene.rs:234-245) for a batch of point/light pairs.  Host buffers. */
int rr_color_at(rr_ctx* ctx, int64_t n, const double* origins, const double* directions, int32_t remaining,
                uint64_t seed, int32_t jitter_mode, double* out_rgb);
int rr_is_shadowed(rr_ctx* ctx, int64_t n, const double* points, const double* light_positions, int32_t* out);

/* ---- ABI 11: first-hit queries and depth / normal / object-id / albedo frames ----
 * hit() + prepare_computations of one ray (scene.rs:128-136, intersection.rs:50-92): the first entry with t >= 0 of
 * Scene::intersect's sorted list and the Computations the reference builds from it, every field bit for bit; n1 / n2
 * are computed for every hit, as the reference does (not only for transparent materials). */
typedef struct {
    int32_t object;   /* rr_scene_desc id of the hit leaf (a CSG's or group's leaf, as Intersection.object); -1: no entry with t >= 0 */
    int32_t inside;
    double t, u, v;
    double point[3], eyev[3], normalv[3], over_point[3], under_point[3], reflectv[3];
    double n1, n2;
} rr_hit;             /* 192 bytes; a miss has object -1 and every other field 0 */

/* A batch of rays -> one rr_hit each.  Host buffers (origins / directions: n x 3 doubles), blocking; n == 0 is
 * RR_OK.  Returns RR_E_NAN after writing `out` when a ray met a NaN t among >= 2 entries.  rr_last_stats then
 * reports rays == samples == n, n1n2_scans == the number of hits, no shadow rays and no shading events.  A
 * multi-device context answers on its first local device. */
int rr_hit_at(rr_ctx* ctx, int64_t n, const double* origins, const double* directions, rr_hit* out);

#define RR_AOV_DEPTH  1  /* double per sample: the hit's t (+inf: miss) */
#define RR_AOV_NORMAL 2  /* 3 doubles: normalv (0,0,0: miss) */
#define RR_AOV_OBJECT 4  /* int32: object id (-1: miss) */
#define RR_AOV_ALBEDO 8  /* 3 doubles: material.pattern_at_object(object, over_point) as shade_hit reads it
                            (material.rs:77-80; 0,0,0: miss) */
/* The camera rays' first hits as image planes (arbitrary output values: a depth, normal, object-id or albedo pass
 * for picking, compositing or a denoiser's guides).  `planes` ORs the RR_AOV_* wanted; each requested plane needs
 * its buffer (NULL: RR_E_ARG), an unrequested plane's pointer is ignored.  Planes are per canvas SAMPLE —
 * cam->vsize x cam->hsize, row-major, the layout of RR_OUT_CANVAS — and never averaged (ids and depths do not
 * average); opts->aa only has to be consistent with the camera sizes, as in rr_render.  The rays are the colour
 * frame's rays bit for bit.  Only part 0 of 1 without a band (else RR_E_ARG); max_depth, seed, jitter_mode and flags
 * are ignored.  rr_render_aov: host buffers, blocking, RR_E_NAN after writing the planes when nan_rays > 0.
 * rr_render_aov_device: device buffers on the context's device, enqueued on `hip_stream` (NULL: ctx stream) and
 * NOT synchronised.  rr_last_stats after either: rays == samples, n1n2_scans == shadow_rays == shade_events == 0.
 * A multi-device context renders the planes on its first local device. */
int rr_render_aov(rr_ctx* ctx, const rr_camera* cam, const rr_render_opts* opts, int32_t planes,
                  double* depth, double* normal, int32_t* object, double* albedo, rr_stats* stats);
int rr_render_aov_device(rr_ctx* ctx, const rr_camera* cam, const rr_render_opts* opts, int32_t planes,
                         void* d_depth, void* d_normal, void* d_object, void* d_albedo, void* hip_stream);

/* ---- adaptive anti-aliasing (additive to ABI 11; test RR_HAS_ADAPTIVE) ----
 * Supersamples only the pixels whose aa 1 colour differs from a neighbour's.  Inputs are rr_render's (a camera of
 * W*aa x H*aa, opts->aa, max_depth, seed, jitter_mode) and a threshold:
 *   1. probe   F1 = the aa 1 frame of the same view: what rr_render returns as out_avg for opts->aa = 1 and the camera
 *              rr_camera_new(cam->hsize / aa, cam->vsize / aa, cam->field_of_view, cam->transform).  The library
 *              derives that camera itself: cam's field_of_view and transform define it, not cam's pixel_size / half_*.
 *   2. mask    pixel p is refined iff some pixel q of its 3x3 neighbourhood, clipped to the frame (q = p included),
 *              has !(max_c |F1[p][c] - F1[q][c]| <= threshold) in plain f64.  So a NaN colour refines its
 *              neighbourhood, threshold < 0 refines every pixel and +inf none (unless a colour is NaN).
 *   3. refine  a refined pixel gets the pixel rr_render returns at opts->aa, bit for bit: the same aa*aa camera rays
 *              with the full frame's area-light jitter identity, summed in canvas.rs:85-96 order and divided by
 *              (double)(aa*aa).
 *   4. result  out_avg = where(mask, that pixel, F1) (H*W*3 doubles); out_mask (H*W bytes, 0 / 1) and n_refined
 *              are optional.  With aa == 1 the result is F1 and the mask is still the criterion's.
 * RR_E_ARG: a null ctx / cam / opts / out_avg, a NaN threshold, part != 0, nparts != 1, a row band, any flag other
 * than RR_NO_FRAME_TIMING, a multi-device or virtual context.  RR_E_LIMIT: (W*aa)*(H*aa) >= 2^32, or more samples
 * than one pass of the context holds (2^27 unless RRAY_BATCH says otherwise).  Other errors are rr_render's;
 * RR_E_NAN is returned after the outputs are written.  The RRAY_UNFUSED / RRAY_NO_TREE / RRAY_NO_CHAIN per-level
 * paths do not serve the refine pass (RR_E_ARG).
 * rr_last_stats / stats afterwards: samples = W*H + aa*aa*n_refined; the ray, shading and walk counters are the
 * probe's plus the refine pass's; kernel_ms is one event pair around everything.
 * rr_render_adaptive: host buffers, blocking.  rr_render_adaptive_device: device buffers on the context's device
 * (d_avg doubles, d_mask bytes, d_n_refined one int64), everything enqueued on `hip_stream` (NULL: ctx stream) and
 * NOT synchronised; no count visits the host between the passes. */
#define RR_HAS_ADAPTIVE 1
int rr_render_adaptive(rr_ctx* ctx, const rr_camera* cam, const rr_render_opts* opts, double threshold,
                       double* out_avg, uint8_t* out_mask, int64_t* n_refined, rr_stats* stats);
int rr_render_adaptive_device(rr_ctx* ctx, const rr_camera* cam, const rr_render_opts* opts, double threshold,
                              void* d_avg, void* d_mask, void* d_n_refined, void* hip_stream);

/* ---- batches of views (additive to ABI 11; test RR_HAS_VIEWS) ----
 * Many cameras of the uploaded scene in one call: stereo pairs, cube-map faces, turntables, light fields, training
 * sets.  `cams` is a host array of n_views cameras that share hsize and vsize (each has its own transform, field of
 * view and derived fields); it is read before the call returns.  `opts` holds for the whole batch (aa, max_depth,
 * seed, jitter_mode, flags).  An output is requested by its flag and then needs its buffer: RR_OUT_AVG n_views x H x W
 * x 3 doubles, RR_OUT_CANVAS n_views x vsize x hsize x 3 doubles; view k is slice k of each, so a caller can wrap
 * either as one tensor.  An unrequested output's pointer is ignored.
 * Definition: slice k is what rr_render(ctx, &cams[k], opts, ...) writes, bit for bit — area lights included: a
 * sample's jitter identity is py * hsize + px within its own view, so a view does not depend on its place in the
 * batch.
 * The batch runs in passes of whole views (as many as fit one pass of the context, 2^27 samples unless RRAY_BATCH
 * says otherwise), each pass one launch of the scene's kernel family; a view's samples take whole 64-lane waves.
 * The call leaves the context's single-frame state alone (cached camera bundles, tile order): an rr_render before
 * and after it returns the same image and the same counters.  rr_resident_launch after a batch reports 0 / 0.
 * rr_last_stats / stats afterwards: rays, shadow_rays, shade_events, n1n2_scans, samples and nan_rays are the sums of
 * the single frames' values; prim_tests, exact_flops and wave_visits are reproducible but may differ from those sums
 * (the culling bundles differ); kernel_ms is one event pair around the batch (0 with RR_NO_FRAME_TIMING).
 * n_views == 0: RR_OK, nothing written.  RR_E_ARG: a null ctx / cams / opts, n_views < 0, a requested output with a
 * null pointer, cameras of differing sizes, sizes inconsistent with aa, part != 0, nparts != 1, a row band,
 * RR_OUT_AVG_F32, RR_PART_INTERLEAVE, a multi-device or virtual context, the RRAY_UNFUSED / RRAY_NO_TREE /
 * RRAY_NO_CHAIN per-level paths.  RR_E_LIMIT: one view holds more samples than one pass (render it with rr_render).
 * Other errors are rr_render's; RR_E_NAN is returned after the outputs are written.
 * rr_render_views: host buffers, blocking.  rr_render_views_device: device buffers on the context's device,
 * everything enqueued on `hip_stream` (NULL: ctx stream) and NOT synchronised. */
#define RR_HAS_VIEWS 1
int rr_render_views(rr_ctx* ctx, const rr_camera* cams, int32_t n_views, const rr_render_opts* opts,
                    double* out_canvas, double* out_avg, rr_stats* stats);
int rr_render_views_device(rr_ctx* ctx, const rr_camera* cams, int32_t n_views, const rr_render_opts* opts,
                           void* d_canvas, void* d_avg, void* hip_stream);

/* ---- first-hit planes of batches of views (additive to ABI 11; test RR_HAS_VIEWS_AOV) ----
 * The guide planes that go with a batch of views: depth, normal, object id and albedo of n_views cameras of the
 * uploaded scene in one call.  `cams` and its rules are rr_render_views' (a host array of cameras that share hsize and
 * vsize, read before the call returns); `planes` and the plane buffers are rr_render_aov's, stacked: depth n_views x
 * vsize x hsize doubles, normal and albedo n_views x vsize x hsize x 3 doubles, object n_views x vsize x hsize int32.
 * View k is slice k of each plane, so a caller can wrap a plane as one tensor.  Each requested plane needs its buffer
 * (NULL: RR_E_ARG), an unrequested plane's pointer is ignored.
 * Definition: slice k of each requested plane is what rr_render_aov(ctx, &cams[k], opts, planes, ...) writes, bit for
 * bit.  Planes are per canvas sample and never averaged; opts->aa only has to be consistent with the camera sizes;
 * max_depth, seed, jitter_mode and flags are ignored.
 * The batch runs in passes of whole views (as many as fit one pass of the context, 2^27 samples unless RRAY_BATCH says
 * otherwise), each pass one launch of the first-hit kernel; a view's samples take whole 64-lane waves.  The
 * RRAY_UNFUSED / RRAY_NO_TREE / RRAY_NO_CHAIN switches do not concern the first-hit kernel and are not refused.
 * The call leaves the context's single-frame state (cached camera bundles, tile order, rr_resident_launch) and the
 * colour batches alone: an rr_render, rr_render_aov or rr_render_views before and after it returns the same outputs
 * and the same counters.
 * rr_last_stats / stats afterwards: rays == samples == n_views * hsize * vsize, shadow_rays == shade_events ==
 * n1n2_scans == 0, nan_rays is the sum of the single frames' values; prim_tests, exact_flops and wave_visits are
 * reproducible but may differ from those sums (the culling bundles differ); kernel_ms is one event pair around the batch.
 * n_views == 0: RR_OK, nothing written.  RR_E_ARG: a null ctx / cams / opts, n_views < 0, `planes` empty or with
 * unknown bits, a requested plane with a null buffer, cameras of differing sizes, sizes inconsistent with aa,
 * part != 0, nparts != 1, a row band, a multi-device or virtual context, no scene uploaded.  RR_E_LIMIT: one view holds
 * more samples than one pass (render it with rr_render_aov).
 * rr_render_views_aov: host buffers, blocking, RR_E_NAN after writing the planes when nan_rays > 0.
 * rr_render_views_aov_device: device buffers on the context's device, everything enqueued on `hip_stream` (NULL: ctx
 * stream) and NOT synchronised; NaN rays are reported through rr_last_stats' nan_rays. */
#define RR_HAS_VIEWS_AOV 1
int rr_render_views_aov(rr_ctx* ctx, const rr_camera* cams, int32_t n_views, const rr_render_opts* opts, int32_t planes,
                        double* depth, double* normal, int32_t* object, double* albedo, rr_stats* stats);
int rr_render_views_aov_device(rr_ctx* ctx, const rr_camera* cams, int32_t n_views, const rr_render_opts* opts,
                               int32_t planes, void* d_depth, void* d_normal, void* d_object, void* d_albedo,
                               void* hip_stream);

/* ---- device-resident ray queries (additive to ABI 11; test RR_HAS_RAYS_DEVICE) ----
 * The ray queries for callers whose rays live in HBM: lenses that are not a pinhole (fisheye, panorama, thin lens,
 * distortion), rays sampled by a network, picking rays, visibility between point pairs.  Device buffers on the context's
 * device; the work is enqueued on `hip_stream` (NULL: ctx stream) and NOT synchronised, with the stream claim of the
 * other _device entries.  Inputs are read in place — no copy, no pack kernel — and must stay valid until the stream
 * reaches the end of the call's work; outputs must not overlap inputs.
 * Ray layout: ray i is six doubles at d_rays + 6 * i, origin xyz then direction xyz (torch.cat([origins, directions],
 * 1) of two n x 3 tensors).
 * rr_camera_rays_device: the hsize * vsize rays of `cam`, row-major (ray py * hsize + px is Camera::ray_for_pixel(px,
 *   py), camera.rs:75-93), computed by the device function the frames use: the colour frame's rays bit for bit.  Needs
 *   no scene.  RR_E_ARG: a null ctx / cam / d_rays, hsize or vsize < 1.  RR_E_LIMIT: hsize * vsize >= 2^32.
 * rr_color_at_device: d_rgb[i] (3 doubles) is what rr_color_at writes for ray i of the same batch, bit for bit.  Ray
 *   i's area-light jitter identity is sample i, path 1, under `seed` — the identity of sample i of a camera frame, so
 *   rr_color_at_device over rr_camera_rays_device(cam) is the canvas of rr_render(cam) with the same remaining / seed /
 *   jitter_mode.
 * rr_hit_at_device: d_hits holds n rr_hit records (192 bytes each, the host struct's layout: word 0 = {object, inside},
 *   words 1..23 = t, u, v, point, eyev, normalv, over_point, under_point, reflectv, n1, n2); record i equals the one
 *   rr_hit_at writes, every field bit for bit.  The batch runs in passes of at most min(context batch, 2^22) rays, so the
 *   context's staging planes stay below 2^22 * 192 bytes whatever n is.
 * rr_is_shadowed_device: d_points and d_light_positions are two n x 3 double arrays, d_out n int32; d_out[i] equals
 *   rr_is_shadowed's value.  rr_last_stats is not touched.
 * The three queries.  n == 0: RR_OK, nothing enqueued.  RR_E_ARG: a null ctx, a null buffer when n > 0, n < 0, no scene
 * uploaded, a multi-device or virtual context (the buffers belong to one device).  RR_E_LIMIT: `remaining` outside
 * 0..RR_MAX_DEPTH, n >= 2^32 (the sample index is 32-bit).  They never return RR_E_NAN: NaN rays are reported through
 * rr_last_stats' nan_rays (the count rr_color_at / rr_hit_at would have turned into RR_E_NAN).
 * rr_last_stats after rr_color_at_device / rr_hit_at_device: samples == n and the call's own counters (for hits: rays
 * == n, n1n2_scans == the number of hits, shadow_rays == shade_events == 0); kernel_ms is one event pair around the
 * call's work.
 * The calls leave the context's frame state alone (cached camera bundles, tile order, rr_resident_launch, the frames'
 * counter buffers): an rr_render or rr_render_views before and after them returns the same image and counters. */
#define RR_HAS_RAYS_DEVICE 1
int rr_camera_rays_device(rr_ctx* ctx, const rr_camera* cam, void* d_rays, void* hip_stream);
int rr_color_at_device(rr_ctx* ctx, int64_t n, const void* d_rays, int32_t remaining, uint64_t seed,
                       int32_t jitter_mode, void* d_rgb, void* hip_stream);
int rr_hit_at_device(rr_ctx* ctx, int64_t n, const void* d_rays, void* d_hits, void* hip_stream);
int rr_is_shadowed_device(rr_ctx* ctx, int64_t n, const void* d_points, const void* d_light_positions, void* d_out,
                          void* hip_stream);

/* ---- ordered ray batches (additive to ABI 11; test RR_HAS_RAY_ORDER) ----
 * Device ray batches are incoherent by nature (lens samples, proposed rays, picking rays), and a wave of 64 unrelated
 * rays culls nothing.  One call puts a batch into a coherent order and the two ordered queries walk the batch in that
 * order; they still answer ray i in slot i, bit for bit what the plain entries write.
 * rr_ray_order_device: writes n uint32 to d_perm; d_perm[j] is the index of the ray at position j of the order.  Needs
 *   no scene.  Deterministic: d_perm == argsort(keys, stable) with the 32-bit keys of rray_amd.ray_order_keys — bounds of
 *   ox, oy, oz and of the octahedral direction (u, v) over the batch's valid rays, six bits per origin axis and seven
 *   per direction axis, morton3(origin) << 14 | morton2(direction); a ray with a NaN or infinite component or a zero
 *   direction has the key 0xFFFFFFFF and sorts to the end.  Directions need not be normalised.
 * rr_color_at_device_ordered / rr_hit_at_device_ordered: the plain entries with wave slot t working on ray d_perm[t].
 *   d_rgb[i] / d_hits[i] are what rr_color_at_device / rr_hit_at_device write for the same batch, bit for bit; ray
 *   d_perm[t]'s area-light jitter identity is sample d_perm[t], path 1.  (One value of the plain entries themselves
 *   depends on which rays share a wave: in a wave that mixes shininess values, the lanes whose shininess is not the
 *   wave's first lane's take the library pow instead of the correctly rounded one, so a specular term may move by an
 *   ulp with the batch's order — between two plain calls as well.  Hits never do.)  d_perm == NULL: the library computes the order
 *   itself into context-owned scratch, then traces, all on the caller's stream.  A non-null d_perm (from
 *   rr_ray_order_device or the caller's own) must hold each of 0..n-1 exactly once.  It is NOT CHECKED: an index >= n
 *   reads and writes out of bounds, a repeated index leaves some slot unwritten.
 * Stream claim, device guard, refusals, n == 0, the n < 2^32 limit, NaN-ray reporting and rr_last_stats are the plain
 * device entries' (rr_ray_order_device refuses a null ctx / buffer, n < 0, n >= 2^32 and a multi-device or virtual
 * context, and leaves rr_last_stats alone).  rr_last_stats after an ordered query: the same rays, shadow_rays,
 * shade_events, n1n2_scans, samples and nan_rays as after the plain call; prim_tests, exact_flops and wave_visits are
 * reproducible but differ — fewer wave visits is what the order is for.  The hit query runs in passes of at most
 * min(context batch, 2^22) positions of the order.  RR_E_ARG under RRAY_UNFUSED / RRAY_NO_TREE / RRAY_NO_CHAIN: the
 * ordered colour query is served by the in-wave kernels only.  RR_E_HIP: the scratch (about 16 bytes per ray, grown
 * on demand, freed with the context) could not be allocated.  Frame state is left alone, as by the plain entries. */
#define RR_HAS_RAY_ORDER 1
int rr_ray_order_device(rr_ctx* ctx, int64_t n, const void* d_rays, void* d_perm, void* hip_stream);
int rr_color_at_device_ordered(rr_ctx* ctx, int64_t n, const void* d_rays, const void* d_perm, int32_t remaining,
                               uint64_t seed, int32_t jitter_mode, void* d_rgb, void* hip_stream);
int rr_hit_at_device_ordered(rr_ctx* ctx, int64_t n, const void* d_rays, const void* d_perm, void* d_hits,
                             void* hip_stream);

/* ---- lens frames: depth of field and jittered samples per pixel (additive to ABI 11; test RR_HAS_LENS) ----
 * A frame with S rays per pixel through a finite aperture, with optional sub-pixel jitter: depth of field, and S
 * decorrelated area-light samples per pixel, in one call with an exact, repeatable definition.  `cam` is the camera at
 * OUTPUT size W x H (cam->hsize x cam->vsize); opts->aa must be 1 (the S samples take aa's place).  Pixel p = py * W +
 * px; sample s of pixel p is ray i = p * S + s of the frame's batch (W * H * S < 2^32).
 * The rays (rr_lens_rays_device writes those of pixels [first_pixel, first_pixel + n_pixels): rr_camera_rays_device's
 * layout, six doubles per ray, ray i at d_rays + 6 * (i - first_pixel * S); no scene needed; ordered on the stream, not
 * synchronised).  Plain f64 in exactly this order, no contraction; rray_amd.lens_rays is the same in numpy:
 *   base = jitter_base(lens.seed, i, 0) (path 0 is free: shading paths start at 1); u(k) = jitter_value(base, 0, k >> 1,
 *     k & 1) = lowbias32(base ^ k) * 2^-32 in [0, 1)
 *   jx, jy = pixel_jitter ? (u(0), u(1)) : (0.5, 0.5)
 *   wx = half_width - ((double)px + jx) * pixel_size;  wy = half_height - ((double)py + jy) * pixel_size
 *   X(x, y, z)[r] = ((M[4r] * x + M[4r+1] * y) + M[4r+2] * z) + M[4r+3] * 1.0, M the camera's inverse as the frames
 *     compute it (rr_camera_inverse returns those 16 doubles; host only)
 *   aperture == 0 (a pinhole): o = X(0, 0, 0), f = X(wx, wy, -1)
 *   aperture > 0 (a thin lens): for a = 0..7: A = 2 * u(2 + 2a) - 1, B = 2 * u(3 + 2a) - 1; the first pair with
 *     A * A + B * B <= 1 is taken, A = B = 0 if there is none (probability (1 - pi/4)^8, about 4.5e-6 per ray; the
 *     rejection loop needs no sin / cos); o = X(aperture * A, aperture * B, 0.0), f = X(wx * fd, wy * fd, -fd) with
 *     fd = focal_distance: every sample of a pixel without jitter passes the same point of the plane in focus
 *   d = f - o, mag = sqrt((dx * dx + dy * dy) + dz * dz), direction d / mag by IEEE division
 * With samples == 1, no jitter and no aperture the rays are rr_camera_rays_device's bit for bit.  A camera whose inverse
 * is not affine (last row other than 0, 0, 0, 1) is refused with RR_E_NONAFFINE.
 * The frame: avg[p][c] = (((c_0 + c_1) + ...) + c_{S-1}) / (double)S per channel, c_s what rr_color_at_device writes
 * for ray p * S + s of the whole frame's batch with remaining = opts->max_depth, opts->seed and opts->jitter_mode (the
 * area-light jitter identity of sample p * S + s, path 1).  out_avg / d_avg: H x W x 3 doubles.
 * The frame runs in passes of whole pixels; every pass but the last holds a multiple of 64 pixels, so a pass starts at
 * a ray index that is a multiple of 64 and its waves are the one-shot batch's.  Default pass: the largest such count
 * with at most 2^22 rays (at least 64 pixels); RRAY_LENS_PASS=<pixels> overrides it (rounded up to a multiple of 64, read
 * at context creation).  Context-owned scratch holds one pass's rays and colours (48 + 24 bytes per ray), grows on
 * demand and is freed with the context (RR_E_HIP when it cannot be allocated).
 * rr_last_stats / stats after a frame: samples == W * H * S; rays, shadow_rays, shade_events, n1n2_scans and nan_rays
 * are what one rr_color_at_device over the whole batch reports; kernel_ms is one event pair around the frame (0 with
 * RR_NO_FRAME_TIMING).  Frame state is left alone, as by the ray entries.
 * rr_render_lens: host buffer, blocking, RR_E_NAN after writing when nan_rays > 0.  rr_render_lens_device: a device
 * buffer, enqueued on `hip_stream` (NULL: ctx stream) and NOT synchronised, stream claim and device guard of the other
 * _device entries; NaN rays are reported through nan_rays.
 * RR_E_ARG: a null pointer, samples outside 1..RR_MAX_LENS_SAMPLES, aperture negative or not finite, focal_distance
 * not finite and positive while aperture > 0, aa != 1, part != 0, nparts != 1, a row band, any flag but
 * RR_NO_FRAME_TIMING, a first_pixel / n_pixels window outside the frame, a multi-device or virtual context, no scene
 * uploaded (frames only).  RR_E_LIMIT: W * H * S >= 2^32, max_depth outside 0..RR_MAX_DEPTH.  n_pixels == 0: RR_OK,
 * nothing enqueued. */
#define RR_HAS_LENS 1
#define RR_MAX_LENS_SAMPLES 4096
typedef struct {
    int32_t samples;        /* S: rays per pixel, 1..RR_MAX_LENS_SAMPLES */
    int32_t pixel_jitter;   /* 0: every sample through the pixel centre (camera.rs's +0.5); 1: uniform in the pixel */
    double aperture;        /* lens radius in camera space; 0: a pinhole.  Finite, >= 0 */
    double focal_distance;  /* camera-space distance of the plane in focus (z = -focal_distance); finite, > 0; ignored when aperture == 0 */
    uint64_t seed;          /* seed of the pixel / lens samples (opts->seed stays the area lights') */
} rr_lens;
int rr_camera_inverse(const rr_camera* cam, double inv[16]);
int rr_lens_rays_device(rr_ctx* ctx, const rr_camera* cam, const rr_lens* lens, int64_t first_pixel, int64_t n_pixels,
                        void* d_rays, void* hip_stream);
int rr_render_lens(rr_ctx* ctx, const rr_camera* cam, const rr_render_opts* opts, const rr_lens* lens, double* out_avg,
                   rr_stats* stats);
int rr_render_lens_device(rr_ctx* ctx, const rr_camera* cam, const rr_render_opts* opts, const rr_lens* lens,
                          void* d_avg, void* hip_stream);

/* ---- ambient occlusion: queries and frames (additive to ABI 11; test RR_HAS_AO) ----
 * How open the surface is at a point: K short occlusion segments over the hemisphere of the normal, each answered as
 * Scene::is_shadowed (scene.rs:234-245) answers a (point, light position) pair, and the share of them that are free.
 * For point i (its index in the batch, or canvas sample py * hsize + px in a frame), with position P, unit normal N
 * and k = 0..K-1, in plain f64 in exactly this order, no contraction (rray_amd.ao_directions / ao_targets / ao_resolve
 * are the same in numpy):
 *   hash: base = jitter_base(ao.seed, i, 0); u(k, j) = lowbias32(base ^ ((k << 21) | j)) * 2^-32 in [0, 1).  For k = 0
 *     these are the lens frames' counters u(j): a caller who combines the two gives them different seeds.
 *   disc point: for a = 0..7: A = 2 * u(k, 2a) - 1, B = 2 * u(k, 2a + 1) - 1; the first pair with A * A + B * B <= 1 is
 *     taken, A = B = 0 if there is none (probability (1 - pi/4)^8, about 4.5e-6, the thin lens's rule; all eight rounds
 *     run in every lane).  c = sqrt(1.0 - (A * A + B * B))
 *   frame around N (Duff et al.'s branch-free basis): s = copysign(1.0, N.z); q = -1.0 / (s + N.z); b = (N.x * N.y) * q;
 *     T = (1.0 + (s * (N.x * N.x)) * q, s * b, -(s * N.x)); Bv = (b, s + (N.y * N.y) * q, -N.y)
 *   direction (Malley's method: cosine-weighted, never below the surface): w[r] = (A * T[r] + B * Bv[r]) + c * N[r]
 *   segment: target[r] = P[r] + radius * w[r]; occluded(i, k) = is_shadowed(P, target), exactly what
 *     rr_is_shadowed_device answers for that pair
 *   value: ao(i) = (double)(K - sum_k occluded(i, k)) / (double)K.  The sum is an integer: the value does not depend on
 *     the order in which the walks finish.
 * rr_ao_directions: host only, no context: w of points first .. first + n - 1 (their hash indices) from n x 3 normals,
 * as (n, K, 3) doubles, by the very function the kernel calls.
 * rr_ao_at_device: two n x 3 double device arrays in (points, unit normals), n doubles out.  Every point is evaluated
 * and normals are taken as unit.  rr_is_shadowed_device's conventions: enqueued on `hip_stream` (NULL: ctx stream) and
 * NOT synchronised; frame state and rr_last_stats are left alone; n == 0 returns RR_OK; a multi-device or virtual
 * context is RR_E_ARG; n * K >= 2^32 is RR_E_LIMIT.
 * rr_render_ao / rr_render_ao_device: one double per canvas sample, vsize x hsize, row-major, never averaged; the rules
 * of `opts` and the refusals are rr_render_aov's (whole frames; max_depth, seed, jitter_mode and flags are ignored),
 * but a multi-device or virtual context is RR_E_ARG.  P and N are over_point and normalv of the sample's first hit, bit
 * for bit rr_hit_at_device's over rr_camera_rays_device(cam); a miss writes 1.0.  The frame runs in passes of at most
 * 2^22 pairs and at most the context's batch of points, every pass but the last a multiple of 64 points
 * (RRAY_AO_PASS=<points> overrides, rounded up to a multiple of 64, read at context creation), in context-owned scratch
 * that grows on demand.  Stats: samples == rays == hsize * vsize, shadow_rays == K * hits, shade_events == 0, kernel_ms
 * one event pair around the frame.  rr_render_ao: host buffer, blocking.  rr_render_ao_device: a device buffer, enqueued
 * and NOT synchronised, as the other _device entries.
 * RR_E_ARG for every entry: a null pointer, samples outside 1..RR_MAX_AO_SAMPLES, reserved != 0, radius not finite or
 * <= 0 (and n < 0, first < 0). */
#define RR_HAS_AO 1
#define RR_MAX_AO_SAMPLES 1024
typedef struct {
    int32_t samples;   /* K: occlusion rays per point, 1..RR_MAX_AO_SAMPLES */
    int32_t reserved;  /* must be 0 */
    double radius;     /* length of each occlusion segment; finite, > 0 */
    uint64_t seed;
} rr_ao;
int rr_ao_directions(const rr_ao* ao, int64_t first, int64_t n, const double* normals, double* out_w);
int rr_ao_at_device(rr_ctx* ctx, int64_t n, const void* d_points, const void* d_normals, const rr_ao* ao, void* d_ao,
                    void* hip_stream);
int rr_render_ao(rr_ctx* ctx, const rr_camera* cam, const rr_render_opts* opts, const rr_ao* ao, double* out_ao,
                 rr_stats* stats);
int rr_render_ao_device(rr_ctx* ctx, const rr_camera* cam, const rr_render_opts* opts, const rr_ao* ao, void* d_ao,
                        void* hip_stream);

/* ---- edge-avoiding denoiser for lens and occlusion frames (additive to ABI 11; test RR_HAS_DENOISE) ----
 * An a-trous (hole-dilated) edge-avoiding wavelet filter over an image that is already on the device, guided by the
 * first-hit planes of rr_render_aov.  Aimed at soft shadows, jittered pixels and occlusion planes.  Caveat: first-hit
 * planes are the pinhole's, so with a wide aperture the filter sharpens out-of-focus edges.
 * Inputs: the image `in`, H x W x C doubles, C in {1, 3} (an occlusion plane or a colour frame); optional guide planes
 * of the same H x W in rr_render_aov's layouts: depth (doubles, +inf for a miss), normal (H x W x 3 doubles), object
 * (int32, -1 for a miss), albedo (H x W x 3 doubles).
 * Rounding: guides are rounded to float when read and widened again: z = (double)(float)depth[p], and so every normal
 *   and albedo component.  This is part of the definition (a pixel's guides pack into 7 floats and an int32 without
 *   changing a bit of the result).  All arithmetic is f64 in exactly the order written, no contraction.
 * void(p): a depth plane is given and !(z_p < +inf), or an object plane is given and id_p < 0.
 * Levels: F_0 = in.  For level i = 0..I-1: s = 2^i, sc = sigma_color * 2^-i (exact), h = (1/16, 1/4, 3/8, 1/4, 1/16).
 * For pixel p = (x, y):
 *   if void(p): F_{i+1}[p] = F_i[p]
 *   else acc[c] = 0.0, ws = 0.0; for dy = -2..2 (outer), dx = -2..2 (inner), q = (x + dx * s, y + dy * s):
 *     skip the tap if q lies outside the frame (no clamping, no mirroring), or if void(q)
 *     w = h[dy+2] * h[dx+2]
 *     if (dx, dy) != (0, 0), the terms that are switched on, in this order; a term whose t is not > 0.0 skips the tap
 *     (so a NaN anywhere skips it):
 *       1. object (RR_DN_OBJECT): id_q != id_p skips the tap
 *       2. colour (sigma_color > 0): d_c = F_i[p][c] - F_i[q][c]; dc = (d_0 * d_0 + d_1 * d_1) + d_2 * d_2, or d_0 * d_0
 *          for C = 1; t = 1.0 + dc / (sc * sc); w = w * (1.0 / (t * t)).  Never zero: a bright outlier is still pulled in
 *       3. normal (sigma_normal > 0): dot = (nx_p * nx_q + ny_p * ny_q) + nz_p * nz_q; e = 1.0 - dot; if e < 0.0 then
 *          e = 0.0; t = 1.0 - e / sigma_normal; w = w * (t * t)
 *       4. depth (sigma_depth > 0): r = (double)(max(|dx|, |dy|) * s);
 *          t = 1.0 - fabs(z_p - z_q) / ((sigma_depth * fabs(z_p)) * r); w = w * (t * t).  The depth change allowed
 *          grows with the tap's distance in pixels, so a floor seen at a glancing angle is still filtered
 *       5. albedo (sigma_albedo > 0): da = (a_0 * a_0 + a_1 * a_1) + a_2 * a_2 of the component differences;
 *          t = 1.0 - da / (sigma_albedo * sigma_albedo); w = w * (t * t)
 *     skip the tap unless w > 0.0
 *     acc[c] = acc[c] + w * F_i[q][c]; ws = ws + w
 *   F_{i+1}[p][c] = acc[c] / ws.  The centre tap always contributes 9/64, so ws > 0.  The output is F_I.
 * (rray_amd.denoise_filter is the same in numpy.)
 * A term that is switched on needs its plane: a null plane is RR_E_ARG.  A plane whose term is off is used only for
 * void (depth, object) or ignored.  RR_E_ARG also: a null ctx, desc, in or out; C not 1 or 3; W or H < 1; iterations
 * outside 1..RR_MAX_DENOISE_ITERATIONS; a sigma that is negative or not finite; unknown flag bits; `out` overlapping an
 * input; a multi-device or virtual context.  RR_E_LIMIT: W * H >= 2^31.  No scene is needed.
 * rr_denoise_reference: host only, no context: the definition, by the very function the kernel calls (single thread:
 *   for small frames).
 * rr_denoise: host buffers, runs on the device, blocking.
 * rr_denoise_device: device buffers on the context's device, enqueued on `hip_stream` (NULL: ctx stream) and NOT
 *   synchronised; the stream claim and device guard of the other _device entries.  One pack kernel per call, one level
 *   kernel per iteration, through two context-owned scratch images that grow on demand (none for iterations == 1).
 *   Frame state and rr_last_stats are left alone, as by rr_is_shadowed_device. */
#define RR_HAS_DENOISE 1
#define RR_MAX_DENOISE_ITERATIONS 8
#define RR_DN_OBJECT 1 /* taps on another object id are skipped (off for meshes: every triangle is an object) */
typedef struct {
    int32_t iterations; /* I: 1..RR_MAX_DENOISE_ITERATIONS; level i uses holes of 2^i pixels */
    int32_t flags;      /* RR_DN_OBJECT or 0; other bits: RR_E_ARG */
    double sigma_color; /* each sigma finite and >= 0; 0 switches the term off */
    double sigma_normal;
    double sigma_depth; /* allowed relative depth change per pixel of distance */
    double sigma_albedo;
} rr_denoise_desc; /* 40 bytes */
int rr_denoise_reference(const rr_denoise_desc* desc, int64_t width, int64_t height, int32_t channels, const double* in,
                         const double* depth, const double* normal, const int32_t* object, const double* albedo,
                         double* out);
int rr_denoise(rr_ctx* ctx, const rr_denoise_desc* desc, int64_t width, int64_t height, int32_t channels,
               const double* in, const double* depth, const double* normal, const int32_t* object, const double* albedo,
               double* out);
int rr_denoise_device(rr_ctx* ctx, const rr_denoise_desc* desc, int64_t width, int64_t height, int32_t channels,
                      const void* d_in, const void* d_depth, const void* d_normal, const void* d_object,
                      const void* d_albedo, void* d_out, void* hip_stream);

/* ---- one-bounce indirect light: gathered radiance at points and frames (additive to ABI 11; test RR_HAS_INDIRECT) ----
 * What the surroundings send to a diffuse surface: the mean of the colours that K cosine-weighted rays from the point
 * bring back, each answered as rr_color_at_device answers any ray.  (rr_render_gather_device is the multi-device frame
 * gather; this feature is called "indirect" everywhere.)  For point i (its index in the batch, or canvas sample
 * py * hsize + px in a frame), with position P, unit normal N and k = 0..K-1 (rray_amd.indirect_rays /
 * indirect_resolve are the same in numpy):
 *   direction: w(i, k) = ao_direction(ao_base(ind.seed, i), k, N): the very function the ambient-occlusion block above
 *     defines and calls — same hash, same disc rejection, same basis, same operation order.  (A caller who combines
 *     the two, or the lens frames, gives them different seeds.)
 *   ray: ray j = i * K + k has origin P and direction w(i, k), taken as it is, with no renormalisation; six doubles in
 *     rr_camera_rays_device's layout.
 *   radiance: L(i, k) is what rr_color_at_device writes for ray j of that batch with remaining = ind.remaining and the
 *     call's seed and jitter_mode: the area lights' jitter identity is sample j, path 1.
 *   value: G(i)[c] = (((L(i,0)[c] + L(i,1)[c]) + ...) + L(i,K-1)[c]) / (double)K, three doubles, plain f64 in this
 *     order.  With cosine-weighted directions this is the irradiance divided by pi.  It is NOT multiplied by the
 *     surface's own albedo, which is what rr_denoise wants; rray_amd.indirect_compose adds it to a colour frame.
 *   The plain ray entries' caveat (the ordered-batch block above) carries over: in a wave that mixes shininess values a
 *   specular term may move by an ulp with the wave's composition, and a frame's waves hold only the rays of the samples
 *   that hit.  In a scene whose materials share one shininess every value is bit for bit the composition's.
 * rr_indirect_at_device: two n x 3 double device arrays in (points, unit normals), n x 3 doubles out.  Every point is
 *   evaluated and normals are taken as unit.  rr_ao_at_device's conventions: enqueued on `hip_stream` (NULL: ctx
 *   stream) and NOT synchronised; frame state is left alone; n == 0 returns RR_OK; a multi-device or virtual context
 *   is RR_E_ARG; n * K >= 2^32 is RR_E_LIMIT.  rr_last_stats afterwards is rr_color_at_device's over the n * K rays,
 *   with samples == n.  The batch runs in passes of whole points (at most 2^22 rays and at most the context's batch
 *   of points, a multiple of 64 points each but the last; RRAY_INDIRECT_PASS=<points> overrides, rounded up to a
 *   multiple of 64, read at context creation) through context-owned scratch that grows on demand and never exceeds one
 *   pass: 48 + 24 bytes per ray.
 * rr_render_indirect / rr_render_indirect_device: vsize x hsize x 3 doubles, one value per canvas sample, row-major,
 *   never averaged.  The rules of `opts` and the refusals are rr_render_ao's (whole frames; a multi-device or virtual
 *   context is RR_E_ARG); opts->seed and opts->jitter_mode are the trace's; max_depth and flags are ignored.  P and N
 *   are over_point and normalv of the sample's first hit, bit for bit rr_hit_at_device's over
 *   rr_camera_rays_device(cam).  A miss writes (0, 0, 0) and traces nothing: the gathered rays of a pass are listed on
 *   the device, only the samples that hit, and their number never visits the host.  hsize * vsize * K >= 2^32 is
 *   RR_E_LIMIT.  Passes as above (a frame's scratch adds 4 bytes per ray for the list).  Stats: samples == hsize *
 *   vsize; rays, shadow_rays, shade_events, n1n2_scans and nan_rays are each what rr_hit_at_device reports over the
 *   camera's rays plus what rr_color_at_device reports over the K rays of the samples that hit, and only those;
 *   kernel_ms is one event pair around the frame.  rr_render_indirect: host buffer, blocking, RR_E_NAN after writing
 *   when nan_rays > 0.  rr_render_indirect_device: a device buffer, enqueued and NOT synchronised; NaN rays are
 *   reported through the stats only.  The frames are served by the in-wave kernels only: RR_E_ARG under RRAY_UNFUSED /
 *   RRAY_NO_TREE / RRAY_NO_CHAIN, as rr_color_at_device_ordered; the point query has no list and serves there too.
 * RR_E_ARG for every entry: a null pointer, samples outside 1..RR_MAX_INDIRECT_SAMPLES (and n < 0).  RR_E_LIMIT:
 * remaining outside 0..RR_MAX_DEPTH. */
#define RR_HAS_INDIRECT 1
#define RR_MAX_INDIRECT_SAMPLES 1024
typedef struct {
    int32_t samples;   /* K: gathered rays per point, 1..RR_MAX_INDIRECT_SAMPLES */
    int32_t remaining; /* the gathered rays' `remaining` (reflection / refraction budget), 0..RR_MAX_DEPTH */
    uint64_t seed;     /* seed of the directions (the area lights keep the call's own seed) */
} rr_indirect;         /* 16 bytes */
int rr_indirect_at_device(rr_ctx* ctx, int64_t n, const void* d_points, const void* d_normals, const rr_indirect* ind,
                          uint64_t seed, int32_t jitter_mode, void* d_out, void* hip_stream);
int rr_render_indirect(rr_ctx* ctx, const rr_camera* cam, const rr_render_opts* opts, const rr_indirect* ind,
                       double* out, rr_stats* stats);
int rr_render_indirect_device(rr_ctx* ctx, const rr_camera* cam, const rr_render_opts* opts, const rr_indirect* ind,
                              void* d_out, void* hip_stream);

/* ---- temporal accumulation: reproject a frame's history (additive to ABI 11; test RR_HAS_TEMPORAL) ----
 * Blends a frame's image with the accumulated image of the previous frame of the same static scene, seen from another
 * (or the same) camera: each pixel's first hit is projected into the previous camera, the history is gathered there
 * bilinearly from the taps that show the same surface, and the two are blended by the history's length.  One
 * image-space kernel; everything it reads is what rr_render_aov_device and the stochastic frames write.
 * Frames: `cur` holds the current frame's image (`in`, H x W x C doubles, C in {1, 3}) and first-hit planes, `prev` the
 * previous call's outputs (out as image, n_out as count, m2_out as m2) with the previous frame's planes.  Planes are
 * H x W in rr_render_aov's layouts.  Outputs: out (H x W x C doubles), n_out (int32 history lengths), m2_out (H x W x C
 * running second moments, or NULL together with prev.m2).  A history whose counts are all 0 is "no history": that is
 * how the first frame is passed.
 * Plain f64 in exactly the order written, no contraction; the only functions are sqrt, fabs and floor
 * (rray_amd.temporal_filter is the same in numpy):
 *   M = rr_camera_inverse(cam), M' = rr_camera_inverse(prev_cam), T' = prev_cam->transform
 *   X_M(x, y, z)[r] = ((M[4r] * x + M[4r+1] * y) + M[4r+2] * z) + M[4r+3] * 1.0
 *   ray(cam, x, y), the pinhole ray of the lens block above at the pixel centre: wx = half_width - ((double)x + 0.5) *
 *     pixel_size, wy = half_height - ((double)y + 0.5) * pixel_size; o = X_M(0, 0, 0), f = X_M(wx, wy, -1), d = f - o,
 *     mag = sqrt((dx * dx + dy * dy) + dz * dz), direction d / mag
 *   void(p) in a frame: !(depth[p] < +inf), or that frame's object plane is given and its id < 0
 * For pixel p = (x, y) with z = cur.depth[p]:
 *   1. void(p): out = in, n_out = 1, m2_out[c] = in[c] * in[c]
 *   2. world point: (o, d) = ray(cam, x, y); P[r] = o[r] + z * d[r]
 *   3. static cameras (every field of the two rr_camera compares ==, so a NaN anywhere makes them unequal): the only
 *      candidate tap is q = p with w = 1.0, and te = z: progressive accumulation under a fixed camera is exact
 *   4. moving cameras: c[r] = ((T'[4r] * Px + T'[4r+1] * Py) + T'[4r+2] * Pz) + T'[4r+3] * 1.0; no candidate if
 *      !(c[2] < 0.0); m = -c[2]; sx = c[0] / m; sy = c[1] / m; fx = (half_width' - sx) / pixel_size' - 0.5;
 *      fy = (half_height' - sy) / pixel_size' - 0.5; no candidate if !(fx > -1.0 && fx < W && fy > -1.0 && fy < H);
 *      x0 = floor(fx), ax = fx - x0, y0 = floor(fy), ay = fy - y0; candidates for j = 0..1 (outer), i = 0..1 (inner):
 *      q = (x0 + i, y0 + j), w = (i ? ax : 1.0 - ax) * (j ? ay : 1.0 - ay); o' = X_M'(0, 0, 0), e = P - o',
 *      te = sqrt((e0 * e0 + e1 * e1) + e2 * e2)
 *   5. a candidate is skipped when any of these holds, tested in this order (each written so that a NaN skips it):
 *      q outside the frame; void(q) in the previous planes; prev.count[q] < 1; RR_TP_OBJECT and the ids differ;
 *      sigma_normal > 0 and !(1.0 - ((nx_p * nx_q + ny_p * ny_q) + nz_p * nz_q) <= sigma_normal);
 *      sigma_plane > 0 and, with (o', d_q) = ray(prev_cam, q), Q[r] = o'[r] + z_q * d_q[r],
 *      g = (n0 * (Q0 - P0) + n1 * (Q1 - P1)) + n2 * (Q2 - P2) over the current normal n: !(fabs(g) <= sigma_plane * te)
 *      (the tap must lie on the current pixel's tangent plane: a floor seen at a glancing angle keeps its history,
 *      which no relative depth tolerance allows); !(w > 0.0)
 *   6. for each surviving tap: acc[c] = acc[c] + w * prev.image[q][c] (accm2 likewise over prev.m2); ws = ws + w;
 *      nmin = min(nmin, prev.count[q])
 *   7. if any tap survived: h[c] = acc[c] / ws, hm2[c] = accm2[c] / ws; n = min(nmin + 1, max_history);
 *      a = 1.0 / (double)n; if a < alpha then a = alpha; out[c] = h[c] + (in[c] - h[c]) * a;
 *      m2_out[c] = hm2[c] + (in[c] * in[c] - hm2[c]) * a; n_out = n.  Otherwise as for a void pixel.
 * RR_E_ARG: a null desc, camera, frame, out or n_out; C not 1 or 3; W or H < 1; either camera's hsize / vsize not W / H;
 * a missing image, depth or previous count plane (cur.count and cur.m2 are ignored); sigma_plane > 0 without cur.normal,
 * sigma_normal > 0 without both normal planes, RR_TP_OBJECT without both object planes; m2_out without prev.m2 or
 * prev.m2 without m2_out; max_history outside 1..RR_MAX_TEMPORAL_HISTORY; alpha outside 0..1 or a sigma negative or
 * not finite; unknown flag bits; an output overlapping an input or another output; a multi-device or virtual context.
 * RR_E_LIMIT: W * H >= 2^31.  A camera whose inverse rr_camera_inverse refuses returns that code.  No scene is needed.
 * rr_temporal_reference: host only, no context: the definition, by the very function the kernel calls.
 * rr_temporal: host buffers, runs on the device, blocking.
 * rr_temporal_device: device buffers on the context's device, enqueued on `hip_stream` (NULL: ctx stream) and NOT
 *   synchronised; the stream claim and device guard of the other _device entries; one kernel launch, no scratch.  Frame
 *   state and rr_last_stats are left alone, as by rr_denoise_device. */
#define RR_HAS_TEMPORAL 1
#define RR_TP_OBJECT 1 /* a tap on another object id is skipped */
#define RR_MAX_TEMPORAL_HISTORY 1048576
typedef struct {
    int32_t flags;       /* RR_TP_OBJECT or 0; other bits: RR_E_ARG */
    int32_t max_history; /* 1..RR_MAX_TEMPORAL_HISTORY: n_out never exceeds it */
    double alpha;        /* 0..1: floor of the blend factor (0: a running mean up to max_history) */
    double sigma_plane;  /* >= 0, finite; 0 switches the term off; needs the current normal plane */
    double sigma_normal; /* >= 0, finite; 0 switches the term off; needs both normal planes */
} rr_temporal_desc;      /* 32 bytes */
typedef struct {         /* one frame's planes, H x W, rr_render_aov's layouts; host or device pointers by entry */
    const void* image;   /* H x W x C doubles: `in` for the current frame, the accumulated `out` of the previous one */
    const void* depth;   /* doubles, +inf: miss.  Required */
    const void* normal;  /* H x W x 3 doubles or NULL */
    const void* object;  /* int32 or NULL */
    const void* count;   /* previous frame only: int32 history lengths (its n_out); NULL in the current frame */
    const void* m2;      /* previous frame only: H x W x C second moments (its m2_out) or NULL */
} rr_temporal_frame;     /* 48 bytes */
int rr_temporal_reference(const rr_temporal_desc* desc, int64_t width, int64_t height, int32_t channels,
                          const rr_camera* cam, const rr_temporal_frame* cur, const rr_camera* prev_cam,
                          const rr_temporal_frame* prev, double* out, int32_t* n_out, double* m2_out);
int rr_temporal(rr_ctx* ctx, const rr_temporal_desc* desc, int64_t width, int64_t height, int32_t channels,
                const rr_camera* cam, const rr_temporal_frame* cur, const rr_camera* prev_cam,
                const rr_temporal_frame* prev, double* out, int32_t* n_out, double* m2_out);
int rr_temporal_device(rr_ctx* ctx, const rr_temporal_desc* desc, int64_t width, int64_t height, int32_t channels,
                       const rr_camera* cam, const rr_temporal_frame* cur, const rr_camera* prev_cam,
                       const rr_temporal_frame* prev, void* d_out, void* d_n_out, void* d_m2_out, void* hip_stream);

/* ---- variance-guided denoising: a per-pixel noise estimate steers the filter (additive to ABI 11; test
 * RR_HAS_DENOISE_VAR) ----
 * Two composable entries that join rr_temporal to an a-trous filter (spatiotemporal variance-guided filtering): rr_variance
 * turns an image — with rr_temporal's moments where there is history, from a guided window where there is none — into a
 * per-pixel variance plane, and rr_denoise_var is rr_denoise's filter with the colour tolerance of each pixel
 * following that plane, which it carries through the levels.  The chain rr_render_*_device -> rr_temporal_device ->
 * rr_variance_device -> rr_denoise_var_device leaves nothing on the host.
 * Guides, their rounding to float, void(p) and the frames' layouts are rr_denoise's (the RR_HAS_DENOISE block above).
 * All arithmetic is f64 in exactly the order written, no contraction; the only functions are fabs and the comparisons.
 * Guide terms: for an off-centre tap q seen from p, the object (1), normal (3), depth (4) and albedo (5) terms of
 *   rr_denoise in that order and with its arithmetic, r = (double)(max(|dx|, |dy|) * step), applied to the starting
 *   weight w; a term whose t is not > 0.0 skips the tap.  The colour term is not among them.
 *
 * rr_variance: `in` (H x W x C doubles, C in {1, 3}), optional m2 (H x W x C) and count (int32 H x W) — rr_temporal's
 * m2_out and n_out, both or neither — and the optional guide planes give var, H x W doubles.  For pixel p = (x, y):
 *   if void(p): V = 0.0
 *   else if count is given and count[p] >= min_history (the temporal branch):
 *     v_c = m2[p][c] - in[p][c] * in[p][c]; if !(v_c > 0.0) then v_c = 0.0
 *     V = ((v_0 + v_1) + v_2) / (double)count[p], or v_0 / (double)count[p] for C = 1.  Divided by the history length, V
 *     is the variance of the accumulated mean: what the difference of two accumulated pixels is measured against.
 *     Under rr_temporal's `alpha` floor the mean weighs recent frames more than 1 / count, so V under-estimates the
 *     noise there.  (min_history = 0 with count[p] = 0 divides by zero as written.)
 *   else (the spatial branch): s1[c] = s2[c] = 0.0, ws = 0.0; for dy = -3..3 (outer), dx = -3..3 (inner),
 *     q = (x + dx, y + dy):
 *       skip the tap if q lies outside the frame, or if void(q)
 *       w = 1.0; if (dx, dy) != (0, 0), the guide terms with step 1; skip the tap unless w > 0.0
 *       s1[c] = s1[c] + w * in[q][c]; s2[c] = s2[c] + w * (in[q][c] * in[q][c]); ws = ws + w
 *     m_c = s1[c] / ws; v_c = s2[c] / ws - m_c * m_c; if !(v_c > 0.0) then v_c = 0.0
 *     V = (v_0 + v_1) + v_2, or v_0 for C = 1, not divided
 * (rray_amd.variance_estimate is the same in numpy.)
 *
 * rr_denoise_var: `in` (H x W x C), var (H x W doubles, required: rr_variance's output or the caller's own estimate)
 * and the guide planes give `out` and, when var_out is not NULL, var_out (H x W): the variance of the filtered image.
 * sigma_color is NOT halved per level: sc2 = sigma_color * sigma_color at every level, and the shrinking variance does
 * the narrowing.  F_0 = in, V_0 = var.  For level i = 0..I-1, s = 2^i, and pixel p = (x, y):
 *   if void(p): F_{i+1}[p] = F_i[p], V_{i+1}[p] = V_i[p]
 *   else the prefiltered variance: ga = gs = 0.0; for ey = -1..1 (outer), ex = -1..1 (inner), q = (x + ex, y + ey)
 *     (step 1 at every level): skip q outside the frame or void; gw = g[ey+1] * g[ex+1] with g = (1/4, 1/2, 1/4);
 *     ga = ga + gw * V_i[q]; gs = gs + gw
 *     gv = ga / gs; den = sc2 * gv + epsilon (two roundings)
 *     acc[c] = 0.0, va = 0.0, ws = 0.0; for dy = -2..2 (outer), dx = -2..2 (inner), q = (x + dx * s, y + dy * s):
 *       skip the tap if q lies outside the frame, or if void(q)
 *       w = h[dy+2] * h[dx+2], h as in rr_denoise
 *       if (dx, dy) != (0, 0): the guide terms with step s; then, if sigma_color > 0: dc as in rr_denoise's colour
 *         term; t = 1.0 + dc / den; skip the tap unless t > 0.0; w = w * (1.0 / (t * t))
 *       skip the tap unless w > 0.0
 *       acc[c] = acc[c] + w * F_i[q][c]; va = va + (w * w) * V_i[q]; ws = ws + w
 *     F_{i+1}[p][c] = acc[c] / ws; V_{i+1}[p] = va / (ws * ws).  The centre tap always contributes, so ws > 0.
 *   Where V is 0, den is epsilon, t * t may overflow and the tap then drops out by `w > 0.0`: a noise-free pixel keeps
 *   its value.  The outputs are F_I and V_I.
 * (rray_amd.denoise_var_filter is the same in numpy.)
 *
 * Refusals, rr_denoise's: RR_E_ARG for a null ctx, desc, in or out (var for rr_variance); C not 1 or 3; W or H < 1;
 * iterations outside 1..RR_MAX_DENOISE_ITERATIONS; a sigma that is negative or not finite; unknown flag bits; a term
 * that is switched on without its plane; an output overlapping an input or another output; a multi-device or virtual
 * context.  RR_E_LIMIT: W * H >= 2^31.  In addition RR_E_ARG: m2 without count or count without m2; min_history outside
 * 0..RR_MAX_TEMPORAL_HISTORY; an epsilon that is not finite or not > 0; a null var for rr_denoise_var.  No scene is
 * needed.
 * The _reference entries: host only, no context: the definition, by the very functions the kernels call.
 * rr_variance, rr_denoise_var: host buffers, run on the device, blocking.
 * rr_variance_device, rr_denoise_var_device: device buffers on the context's device, enqueued on `hip_stream` (NULL: ctx
 *   stream) and NOT synchronised; the stream claim and device guard of the other _device entries.  One pack kernel per
 *   call, then one variance kernel, or one level kernel per iteration through rr_denoise_device's two scratch images
 *   and two context-owned variance planes that grow on demand (none for iterations == 1).  Frame state and
 *   rr_last_stats are left alone, as by rr_denoise_device. */
#define RR_HAS_DENOISE_VAR 1
typedef struct {
    int32_t flags;       /* RR_DN_OBJECT or 0; other bits: RR_E_ARG */
    int32_t min_history; /* 0..RR_MAX_TEMPORAL_HISTORY: a pixel with count >= min_history takes the temporal branch */
    double sigma_normal; /* the spatial branch's guide terms: each sigma finite and >= 0; 0 switches the term off */
    double sigma_depth;
    double sigma_albedo;
} rr_variance_desc; /* 32 bytes */
typedef struct {
    int32_t iterations; /* the fields of rr_denoise_desc, with its meanings and ranges */
    int32_t flags;
    double sigma_color; /* in standard deviations of the pixel's noise: t = 1 + dc / (sigma_color^2 * gv + epsilon) */
    double sigma_normal;
    double sigma_depth;
    double sigma_albedo;
    double epsilon; /* finite and > 0: the colour tolerance (squared) of a pixel whose variance is 0 */
} rr_denoise_var_desc; /* 48 bytes */
int rr_variance_reference(const rr_variance_desc* desc, int64_t width, int64_t height, int32_t channels, const double* in,
                          const double* m2, const int32_t* count, const double* depth, const double* normal,
                          const int32_t* object, const double* albedo, double* var);
int rr_variance(rr_ctx* ctx, const rr_variance_desc* desc, int64_t width, int64_t height, int32_t channels,
                const double* in, const double* m2, const int32_t* count, const double* depth, const double* normal,
                const int32_t* object, const double* albedo, double* var);
int rr_variance_device(rr_ctx* ctx, const rr_variance_desc* desc, int64_t width, int64_t height, int32_t channels,
                       const void* d_in, const void* d_m2, const void* d_count, const void* d_depth, const void* d_normal,
                       const void* d_object, const void* d_albedo, void* d_var, void* hip_stream);
int rr_denoise_var_reference(const rr_denoise_var_desc* desc, int64_t width, int64_t height, int32_t channels,
                             const double* in, const double* var, const double* depth, const double* normal,
                             const int32_t* object, const double* albedo, double* out, double* var_out);
int rr_denoise_var(rr_ctx* ctx, const rr_denoise_var_desc* desc, int64_t width, int64_t height, int32_t channels,
                   const double* in, const double* var, const double* depth, const double* normal, const int32_t* object,
                   const double* albedo, double* out, double* var_out);
int rr_denoise_var_device(rr_ctx* ctx, const rr_denoise_var_desc* desc, int64_t width, int64_t height, int32_t channels,
                          const void* d_in, const void* d_var, const void* d_depth, const void* d_normal,
                          const void* d_object, const void* d_albedo, void* d_out, void* d_var_out, void* hip_stream);

/* Host-only inspection of the flattening (no device needed): per-object inverse transforms as the
 * kernels use them (4x4, row 3 == 0,0,0,1), group bounding boxes (group.rs:128-149; zeros for
 * non-groups) and each object's index in the flattened depth-first order (-1: not in the tree).
 * Any output pointer may be NULL. */
int rr_scene_inspect(const rr_scene_desc* desc, double* inverses, double* group_aabbs, int32_t* node_of_object);

/* ---- front-end: scene_builder_yaml.rs / load_obj.rs / canvas.rs / main.rs ---- */
/* render_scene_from_str up to camera.render: parse YAML (first document), build the scene.
 * obj_root: directory relative OBJ paths are resolved against (NULL: current directory). */
int rr_scene_from_yaml(const char* yaml_text, const char* obj_root, int64_t width, int64_t height, int32_t aa,
                       rr_scene** out_scene, rr_camera* out_camera);
const rr_scene_desc* rr_scene_desc_of(const rr_scene* scene);
void rr_scene_free(rr_scene* scene);
/* canvas.rs:76-105 + write_to_file: AA-averaged f64 image -> RGBA8 (`as u8`) -> PNG */
int rr_quantize(const double* avg, int64_t n_pixels, uint8_t* rgba);
int rr_write_png(const char* path, const uint8_t* rgba, int64_t width, int64_t height);
/* render_scene_from_file (scene_builder_yaml.rs:429-436) on `device` */
int rr_render_scene_from_file(const char* path, int64_t width, int64_t height, const char* png_file, int32_t aa,
                              int device);
/* the same on n devices of this process (rr_create_multi) */
int rr_render_scene_from_file_devices(const char* path, int64_t width, int64_t height, const char* png_file,
                                      int32_t aa, int n_devices, const int* device_ids);

#ifdef __cplusplus
}
#endif
#endif /* RRAY_RRAY_H */
