// render_common.inc — device helpers shared by every render translation unit (render.hip and the
// per-variant level units render_levels_*.hip): canvas mapping, camera rays, event keys, block
// appends, counter flushes and the delivery of finished color_at values.  Included inside
// namespace rr, after device_core.inc / kernels.hpp / wavefront.hpp.
// floor(n / d) for d >= 1 given magic = floor(2^32 / d) (d >= 2; unused for d == 1): the high
// product is the quotient or one less for every 32-bit n, so one correction makes it exact.
// (Branch-free: the kernels' prologue would otherwise wait for d before loading what follows.)
__device__ __forceinline__ uint32_t magic_div(uint32_t n, uint32_t d, uint32_t magic) {
    uint32_t q = __umulhi(n, magic);
    q += (n - q * d >= d) ? 1u : 0u;
    return d == 1u ? n : q;
}

// A level-0 event's canvas position: ls = part-local row-major sample index (the output index),
// (px, py) = supersampled canvas pixel.  Camera events run in tile order (tile_to_local); when every
// tile is a full 8x8 and the batch is tile-aligned (A.tile_fast, host-checked) a wave is exactly one
// tile, so the tile arithmetic is wave-uniform (scalar) and a lane only adds its (lane & 7, lane >> 3)
// offset — the same bijection as tile_to_local_u32 without its three per-lane divisions.
struct Px0 {
    uint32_t ls, px, py;
    uint32_t lrow;  // part-local supersampled row (ls = lrow * hs + px)
};
// part-local supersampled row -> canvas row: interleaved row blocks of the part (32-bit: rr_render_device rejects
// parts of 2^31 samples or more).  A band render (rr_render_opts row_begin / row_end) is part row_begin / block of 1
// with a block that divides row_begin (api.cpp rr_render_device), so the same arithmetic gives its frame rows.
__device__ __forceinline__ uint32_t canvas_row(const LevelArgs& A, uint32_t lrow) {
    const uint32_t aa = (uint32_t)A.aa, br = (uint32_t)A.block_rows;
    const uint32_t k = magic_div(lrow, aa, A.aa_magic), sub = lrow - k * aa;
    const uint32_t bi = magic_div(k, br, A.br_magic), kb = k - bi * br;
    const uint32_t y = (bi * (uint32_t)A.nparts + (uint32_t)A.part) * br + kb;
    return y * aa + sub;
}
// Pixel waves (A.pw, aa = 3): a level-0 wave holds 7 whole pixels (63 samples, lane 63 idle), so it can box-average
// its own samples (deliver_pixel_wave) — 3 does not divide the 8x8 tile.  The part's output rows go in bands of two;
// a band's pixels are numbered column-major (p -> column p / r, row p % r for a band of r rows) and wave w of the band
// takes p = 7w .. 7w + 6: a 4 x 2-pixel (12 x 6-sample) footprint.  Lane l: pixel l / 9 of the wave, sample (dx, dy) =
// (s % 3, s / 3) for s = l % 9 — the reference's dy-outer, dx-inner order within the pixel.
struct PixelWave {
    uint32_t band, w, rb;  // band, wave in the band, output rows in the band (1 or 2)
};
__device__ __forceinline__ PixelWave pixel_wave(const LevelArgs& A, uint32_t g) {
    PixelWave pw;
    pw.band = g / A.pw_wpb;
    pw.w = g - pw.band * A.pw_wpb;
    const uint32_t left = (uint32_t)A.pw_rows - 2u * pw.band;
    pw.rb = left < 2u ? left : 2u;
    return pw;
}
// sample (px, lrow) of lane `lane` in pixel wave pw; false for idle lanes
__device__ __forceinline__ bool pixel_wave_sample(const LevelArgs& A, const PixelWave& pw, uint32_t lane, uint32_t& px,
                                                  uint32_t& lrow) {
    const uint32_t q = (lane * 57u) >> 9;  // lane / 9 for lane < 64
    const uint32_t sm = lane - 9u * q, dy = (sm * 11u) >> 5, dx = sm - 3u * dy;  // sm / 3 for sm < 9
    const uint32_t p = 7u * pw.w + q;
    const uint32_t col = pw.rb == 2u ? p >> 1 : p, prow = pw.rb == 2u ? p & 1u : 0u;
    px = 3u * col + dx;
    lrow = 3u * (2u * pw.band + prow) + dy;
    return q < 7u && px < (uint32_t)A.hs;
}
// OWN: i is this thread's own index (blockIdx.x * 256 + threadIdx.x), so the wave's tile is uniform;
// otherwise (events from a list) the same mapping is computed per lane from i.
// the tile of this wave's launch slot (level 0, tile_fast, OWN indexing): the slot itself, or the tile the
// cost order puts there (ORDER kernels: A.tile_perm, wave-uniform scalar load).  Only the group scenes' fused
// kernels carry the order (the flat scenes' kernels measured 1-1.5 % slower with the code in them, unused)
// (wave: the wave's index in the block when the caller holds it as a scalar, else -1)
// The cost order permutes single tiles (A.order_group == 1: chain frames, whose blocks then hold waves of like cost and
// release their LDS together) or groups of four consecutive tiles (a block's waves: horizontally adjacent tiles, whose
// output rows join into whole cache lines; A.tile_perm then maps the launch block to a tile group).  One-batch frames,
// base 0.
// tile >= 0: the caller's own tile (the persistent level-0 loop takes its tiles from a queue, queue_request below)
template <bool ORDER = false>
__device__ __forceinline__ uint32_t own_tile(const LevelArgs& A, int wave = -1, int64_t tile = -1) {
    if (tile >= 0) return (uint32_t)tile;
    const uint32_t w = wave >= 0 ? (uint32_t)wave : (uint32_t)uniform((int)threadIdx.x) >> 6;
    const uint32_t T0 = (uint32_t)(A.base >> 6) + blockIdx.x * 4u + w;
    if constexpr (ORDER) {
        if (!A.tile_perm) return T0;
        return A.order_group == 1 ? ldc(A.tile_perm, (int)T0) : ldc(A.tile_perm, (int)blockIdx.x) * 4u + w;
    }
    return T0;
}
// PW: the kernel may run pixel waves (A.pw; the chain kernels); ok (PW) = the lane holds a sample
template <bool OWN, bool ORDER = false, bool PW = false>
__device__ __forceinline__ Px0 level0_px(const LevelArgs& A, int64_t i, int wave = -1, bool* ok = nullptr,
                                         int64_t tile = -1) {
    Px0 r;
    if (A.rays0) {
#ifdef RR_LISTED
        // An ordered ray batch (the rr::listed kernels, rr_*_at_device_ordered): slot t works on ray list[t], a
        // permutation of the batch; ls is the ray's own index, so its jitter identity is sample ls and its result
        // lands in slot ls.  Slots past the launch's events (i >= A.n: the last wave) hold no ray (ok) and read nothing.
        if (A.list) {
            const bool in = i < A.n;
            if (ok) *ok = in;
            r.ls = in ? A.list[A.base + i] : 0u;
            r.px = r.py = r.lrow = 0u;
            return r;
        }
#endif
        r.ls = (uint32_t)(A.base + i);
        r.px = r.py = r.lrow = 0u;
        return r;
    }
#ifdef RR_LISTED
    // Listed pixels (the rr::listed kernels, adaptive frames' refine pass): event t is sample t % aa^2 (dy outer, dx
    // inner: canvas.rs:85-96) of output pixel list[t / aa^2]; ls = t, the event's slot in the compact sample buffer.
    // Whole frames only (part 0 of 1), so the canvas row is the sample row.  Events past the live count (A.n_dev)
    // hold no sample (ok).
    if (A.list) {
        const uint32_t t = (uint32_t)(A.base + i);
        const bool in = t < *A.n_dev;
        if (ok) *ok = in;
        const uint32_t aa = (uint32_t)A.aa, aa2 = aa * aa;
        const uint32_t k = t / aa2, sm = t - k * aa2, dy = sm / aa, dx = sm - dy * aa;
        const uint32_t p = in ? A.list[k] : 0u;
        const uint32_t y = p / A.list_w, x = p - y * A.list_w;
        r.ls = t;
        r.px = x * aa + dx;
        r.py = r.lrow = y * aa + dy;
        return r;
    }
#endif
#ifdef RR_VIEWS
    // A batch of views (the rr::views kernels): event t is event t % view_e of view t / view_e, view_e a multiple of
    // 64, so the wave's view and its tile within the view are wave-uniform (scalar); hs x lrows is one view's canvas.
    // Full tiles (tile_fast) take the wave-uniform tile arithmetic, other sizes tile_to_local_u32 within the view, and
    // events past the view's samples hold none (ok).  lrow counts the rows of the stacked canvases (view * lrows +
    // the view's row), so ls = lrow * hs + px is the sample's slot in the batch's output and deliver_wave_avg's pixel
    // arithmetic holds as it is (lrows is a multiple of aa); py is the view's own canvas row, the camera's and the
    // jitter identity's.
    {
        const uint32_t t = (uint32_t)(A.base + i);
        const uint32_t w = OWN ? (uint32_t)uniform((int)(t >> 6)) : t >> 6;
        const uint32_t e64 = A.view_e >> 6, view = w / e64, tw = w - view * e64;
        const uint32_t hs = (uint32_t)A.hs, vs = (uint32_t)A.lrows;
        const uint32_t lane = OWN ? (uint32_t)lane_id() : t & 63u;
        bool in = true;
        if (A.tile_fast) {
            const uint32_t band = tw / A.tiles_per_row, tc = tw - band * A.tiles_per_row;
            r.py = band * 8u + (lane >> 3);
            r.px = tc * 8u + (lane & 7u);
        } else {
            const uint32_t tl = tw * 64u + lane;
            in = tl < hs * vs;
            const uint32_t l = tile_to_local_u32(in ? tl : 0u, hs, vs);
            r.py = l / hs;
            r.px = l - r.py * hs;
        }
        if (ok) *ok = in;
        r.lrow = view * vs + r.py;
        r.ls = r.lrow * hs + r.px;
        return r;
    }
#else
    const uint32_t hs = (uint32_t)A.hs;
    uint32_t lrow;
    if (PW && A.pw) {  // OWN indexing, one batch (base 0): the wave's slot, or the wave the cost order puts there
        const PixelWave pw = pixel_wave(A, own_tile<ORDER>(A, wave, tile));
        const bool in = pixel_wave_sample(A, pw, (uint32_t)lane_id(), r.px, lrow);
        if (ok) *ok = in;
        if (!in) r.px = lrow = 0u;
        r.ls = lrow * hs + r.px;
        r.py = canvas_row(A, lrow);
        r.lrow = lrow;
        return r;
    }
    if (A.tile_fast) {
        const uint32_t t = (uint32_t)(A.base + i);
        const uint32_t T = OWN ? own_tile<ORDER>(A, wave, tile) : ((ORDER && A.tile_perm) ? (A.order_group == 1 ? A.tile_perm[t >> 6] : A.tile_perm[t >> 8] * 4u + ((t >> 6) & 3u))
                                                                          : t >> 6);
        const uint32_t band = T / A.tiles_per_row;
        const uint32_t tc = T - band * A.tiles_per_row;
        const uint32_t lane = OWN ? (uint32_t)lane_id() : t & 63u;
        lrow = band * 8u + (lane >> 3);
        r.px = tc * 8u + (lane & 7u);
        r.ls = lrow * hs + r.px;
    } else {
        const uint32_t t = (uint32_t)(A.base + i);
        r.ls = A.lrows <= 0 ? t : tile_to_local_u32(t, hs, (uint32_t)A.lrows);
        lrow = r.ls / hs;
        r.px = r.ls - lrow * hs;
    }
    r.py = canvas_row(A, lrow);
    r.lrow = lrow;
    return r;
#endif
}
template <bool OWN, bool ORDER = false>
__device__ __forceinline__ Px0 level0_px_if(const LevelArgs& A, int64_t i, int64_t tile = -1) {
    if (A.level > 0) return {0u, 0u, 0u, 0u};
    return level0_px<OWN, ORDER>(A, i, -1, nullptr, tile);
}

// Camera::ray_for_pixel (camera.rs:75-93).  The camera inverse's 4th row is (0, 0, 0, 1) for every
// view_transform (checked on the host, A.cam_affine), so pixel.w == 1 == origin.w and the w terms of
// the subtraction and of the magnitude are exactly +0 (adding +0 to a sum of squares is exact).
__device__ __forceinline__ Ray camera_ray(const DevCamera& C, bool affine, uint32_t px, uint32_t py) {
    double xoffset = ((double)px + 0.5) * C.pixel_size;
    double yoffset = ((double)py + 0.5) * C.pixel_size;
    double wx = C.half_width - xoffset;
    double wy = C.half_height - yoffset;
    const double* M = C.inv;
    const double* ow = C.origin;  // M * point(0, 0, 0): pixel-independent, computed on the host
    if (affine) {
        double pw[3];
        for (int r = 0; r < 3; ++r) pw[r] = M[4 * r] * wx + M[4 * r + 1] * wy + M[4 * r + 2] * -1.0 + M[4 * r + 3] * 1.0;
        double dx = pw[0] - ow[0], dy = pw[1] - ow[1], dz = pw[2] - ow[2];
        double mag = sqrt(dx * dx + dy * dy + dz * dz);
        return {mk(ow[0], ow[1], ow[2]), div3(mk(dx, dy, dz), mag)};
    }
    double pw[4];
    for (int r = 0; r < 4; ++r) pw[r] = M[4 * r] * wx + M[4 * r + 1] * wy + M[4 * r + 2] * -1.0 + M[4 * r + 3] * 1.0;
    double dx = pw[0] - ow[0], dy = pw[1] - ow[1], dz = pw[2] - ow[2], dw = pw[3] - ow[3];
    double mag = sqrt(dx * dx + dy * dy + dz * dz + dw * dw);
    return {mk(ow[0], ow[1], ow[2]), mk(dx / mag, dy / mag, dz / mag)};
}

// level-0 camera rays of full 8x8 tiles through an affine camera: one origin, a planar grid of directions
// (make_bundle's cam_tile bundle)
#ifdef RR_VIEWS
// the view of this wave's launch slot (OWN indexing, as own_tile): wave-uniform, a scalar
__device__ __forceinline__ uint32_t own_view(const LevelArgs& A) {
    const uint32_t w = (uint32_t)(A.base >> 6) + blockIdx.x * 4u + ((uint32_t)uniform((int)threadIdx.x) >> 6);
    return w / (A.view_e >> 6);
}
// full tiles of the wave's own view, when its camera is affine (its flag from the camera table: a scalar load)
__device__ __forceinline__ bool cam_tile(const LevelArgs& A) {
    return A.level == 0 && !A.rays0 && A.tile_fast && cp(A.views)[own_view(A)].affine != 0;
}
#else
__device__ __forceinline__ bool cam_tile(const LevelArgs& A) {
    return A.level == 0 && !A.rays0 && A.tile_fast && A.cam_affine;
}
#endif

// this wave's entry of the per-frame tile-bundle table (level 0, tile_fast, OWN indexing), or null
template <bool ORDER = false>
__device__ __forceinline__ const float* cam_bundle_of(const LevelArgs& A, int wave = -1, int64_t tile = -1) {
    if (!A.tile_bundles || !cam_tile(A)) return nullptr;
    return A.tile_bundles + (size_t)own_tile<ORDER>(A, wave, tile) * RR_TILE_BUNDLE_FLOATS;
}

// the ray of event i at this level; q = level0_px(A, i) (used at level 0 only); camera rays also
// return their global sample id (the jitter key, as event_key) in s0
__device__ __forceinline__ Ray event_ray(const LevelArgs& A, int64_t i, const Px0& q, uint64_t& s0) {
    if (A.level > 0) {
        const Event& e = A.ev[i];
        return {mk(e.o[0], e.o[1], e.o[2]), mk(e.d[0], e.d[1], e.d[2])};
    }
    if (A.rays0) {
#ifdef RR_LISTED  // an ordered ray batch reads ray q.ls = list[base + i]: a 48-byte gather per lane
        const double* p = A.list ? A.rays0 + 6 * (int64_t)q.ls : A.rays0 + 6 * (A.base + i);
#else
        const double* p = A.rays0 + 6 * (A.base + i);
#endif
        return {mk(p[0], p[1], p[2]), mk(p[3], p[4], p[5])};
    }
    s0 = (uint64_t)q.py * (uint64_t)A.hs + q.px;
#ifdef RR_VIEWS
    // the wave's own camera: the view index is wave-uniform (every rr::views kernel indexes its events by launch
    // slot), so the record is read through the constant address space into scalar registers, and camera_ray itself is
    // the single frame's
    {
        const uint32_t view = (uint32_t)uniform((int)((uint32_t)(A.base + i) >> 6)) / (A.view_e >> 6);
        const cptr<DevView> V = cp(A.views) + view;
        DevCamera C;
        C.hsize = C.vsize = 0;  // not read by camera_ray
        C.half_width = V->cam.half_width;
        C.half_height = V->cam.half_height;
        C.pixel_size = V->cam.pixel_size;
        for (int k = 0; k < 16; ++k) C.inv[k] = V->cam.inv[k];
        for (int k = 0; k < 4; ++k) C.origin[k] = V->cam.origin[k];
        return camera_ray(C, V->affine != 0, q.px, q.py);
    }
#else
    return camera_ray(A.cam, A.cam_affine, q.px, q.py);
#endif
}
template <bool OWN>
__device__ __forceinline__ Ray event_ray(const LevelArgs& A, int64_t i) {
    uint64_t s0 = 0;
    return event_ray(A, i, level0_px_if<OWN>(A, i), s0);
}
// jitter identity of event i: (global sample id, recursion path); q as for event_ray
// (s0: event_ray's sample id of a level-0 camera ray)
__device__ __forceinline__ void event_key(const LevelArgs& A, int64_t i, const Px0& q, uint64_t s0, uint64_t& sample,
                                          uint32_t& path) {
    path = A.level > 0 ? A.ev[i].path : 1u;
    if (A.level == 0) {
        sample = A.rays0 ? (uint64_t)q.ls : s0;
        return;
    }
    const uint32_t ls = A.ev[i].sample;
    if (A.rays0) {
        sample = (uint64_t)ls;
        return;
    }
    // level >= 1: the event carries its camera sample's local index (row-major)
    const uint32_t hs = (uint32_t)A.hs;
    const uint32_t lrow = ls / hs, px = ls - lrow * hs;
    sample = (uint64_t)canvas_row(A, lrow) * (uint64_t)A.hs + px;
}

// Block-aggregated queue appends: the 4 waves' ballots are summed in LDS and one lane per queue
// does a single device-scope atomicAdd for the whole block (device-scope atomics are performed
// memory-side and serialise per address, so one per wave per queue was the kernels' bottleneck).
// Every thread of the (256-thread) block must call it.  Returns this lane's slot where want[q].
template <int NQ>
__device__ __forceinline__ void block_append(unsigned int* const (&ctr)[NQ], const bool (&want)[NQ],
                                             int32_t (&slot)[NQ]) {
    __shared__ unsigned int s_cnt[NQ][4];
    __shared__ unsigned int s_base[NQ][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t m[NQ];
    for (int q = 0; q < NQ; ++q) {
        m[q] = __ballot(want[q]);
        if (lane == 0) s_cnt[q][w] = (unsigned int)__popcll(m[q]);
    }
    __syncthreads();
    if (threadIdx.x < NQ) {
        const int q = threadIdx.x;
        unsigned int total = s_cnt[q][0] + s_cnt[q][1] + s_cnt[q][2] + s_cnt[q][3];
        unsigned int run = total ? atomicAdd(ctr[q], total) : 0u;
        for (int k = 0; k < 4; ++k) {
            s_base[q][k] = run;
            run += s_cnt[q][k];
        }
    }
    __syncthreads();
    const uint64_t below_mask = lane == 0 ? 0ull : ((~0ull) >> (64 - lane));
    for (int q = 0; q < NQ; ++q) slot[q] = (int32_t)(s_base[q][w] + (unsigned int)__popcll(m[q] & below_mask));
}

// Wave-level queue append (segmented fused levels): one device atomic per wave on the segment's counter,
// no workgroup barrier, so a block's fast waves never wait for its slow ones.  Returns this lane's slot
// where want (else -1).
__device__ __forceinline__ int32_t wave_append(unsigned int* ctr, bool want) {
    const uint64_t m = __ballot(want);
    if (m == 0) return -1;
    const int lane = lane_id(), leader = __ffsll((long long)m) - 1;
    unsigned int base = 0;
    if (lane == leader) base = atomicAdd(ctr, (unsigned int)__popcll(m));
    base = (unsigned int)__builtin_amdgcn_readlane((int)base, leader);
    const uint64_t below = lane == 0 ? 0ull : ((~0ull) >> (64 - lane));
    return want ? (int32_t)(base + (unsigned int)__popcll(m & below)) : -1;
}

// Sharded work queue (persist_map.hpp; the persistent level-0 loop, render_persist.inc): H heads, head h at
// head[h * RR_CNT_STRIDE], each counting the tickets handed out.  Accesses to one head serialise memory-side (about
// 11 ns each, loads included): a wave touches only its home head, once per tile.  queue_request takes the next ticket of head h for the
// wave — one returning device atomic from lane 0 (a vector instruction); the ticket stays in lane 0's register until
// queue_ticket broadcasts it, so the request can be issued ahead of the work that hides its latency.
__device__ __forceinline__ uint32_t queue_request(unsigned long long* head, uint32_t h) {
    uint32_t k = 0;
    if (lane_id() == 0) k = (uint32_t)atomicAdd(head + (size_t)h * RR_CNT_STRIDE, 1ull);
    return k;
}
__device__ __forceinline__ uint32_t queue_ticket(uint32_t requested) {
    return (uint32_t)__builtin_amdgcn_readlane((int)requested, 0);
}

// The live event count of a level.  Levels >= 1 are launched with their worst-case grid (the
// previous level's capacity x max children, known on the host) and read the real count the previous
// level's appends produced from HBM, so the host never waits for a level to finish (rray.h:
// rr_render_device is asynchronous).  Blocks past the count exit at once (block-uniform).
__device__ __forceinline__ int64_t live_count(const LevelArgs& A) {
    return A.n_dev ? (int64_t)*A.n_dev : A.n;
}

enum WalkKind { W_NONE = -1, W_TRACE = 0, W_SHADOW = 1, W_N1N2 = 2 };
// Counter flush, aggregated per workgroup: the 4 waves' totals are summed in LDS and one thread per
// counter does a single device-scope atomic (slot = blockIdx % RR_CNT_SLOTS), 4x fewer memory-side
// atomics than per-wave flushes (they were ~14 % of a C2 frame's HBM writes).  `extra` adds the fused
// kernels' closest-hit walk flops / visits.  Every thread of the (256-thread) block must call it.
constexpr int RR_FLUSH_N = 12;
// the counter slot of flush value k (k < RR_FLUSH_N, a lane index) as a chain of selects: a constant table indexed by
// the lane is a private array, and every wave wrote its 48 B per lane to scratch memory before the atomics (1.19 M
// waves x 3 KB per C3 frame: most of the chain kernel's 2.0 GB of HBM writes, profiles/r05)
__device__ __forceinline__ int flush_slot(int k, int walk) {
    const int wk = walk >= 0 ? walk : 0;
    int s = C_NAN;
    s = k == 10 ? (int)C_VISITS_TRACE : s;
    s = k == 9 ? (int)C_FLOPS_TRACE : s;
    s = k == 8 ? (int)C_VISITS_TRACE + wk : s;
    s = k == 7 ? (int)C_FLOPS_TRACE + wk : s;
    s = k == 6 ? (int)C_PRIM_TESTS : s;
    return k < 6 ? k : s;  // C_RAYS .. C_GROUP_HITS are 0 .. 5
}
static_assert(C_RAYS == 0 && C_SHADOW == 1 && C_SHADE == 2 && C_N1N2 == 3 && C_GROUP_TESTS == 4 && C_GROUP_HITS == 5,
              "flush_slot: the first six flush values map to counters 0..5");
// WAVE (fused kernels, which have no other workgroup barrier): one atomic per counter per wave, so a
// finished wave leaves at once instead of waiting at a barrier for the block's slowest wave.
// wave: this wave's index in the block when the caller holds it (a scalar), or -1 (taken from threadIdx.x)
// Always inlined: an out-of-line flush takes the Counters by address, and the kernel then keeps them in private
// memory for its whole run — every count became a scratch load and store (the C5 chain kernel: 106 scratch stores)
template <bool WAVE = false>
__device__ __forceinline__ void flush(const Counters& cnt, unsigned long long* counters, int walk = W_NONE,
                      uint64_t trace_flops = 0, uint64_t trace_visits = 0, int wave = -1) {
    if constexpr (WAVE) {
        const int lane = lane_id();
        const uint64_t v[RR_FLUSH_N] = {cnt.rays, cnt.shadow, cnt.shade, cnt.n1n2, cnt.gtests, cnt.ghits, cnt.tests,
                                        walk >= 0 ? (uint64_t)cnt.flops : 0ull, walk >= 0 ? (uint64_t)cnt.visits : 0ull,
                                        trace_flops, trace_visits, cnt.nan};
        const uint32_t w = wave >= 0 ? (uint32_t)wave : (uint32_t)uniform((int)threadIdx.x) >> 6;
        const int slot = (int)((blockIdx.x * 4u + w) & (RR_CNT_SLOTS - 1));
        if (lane < RR_FLUSH_N) {
            unsigned long long t = 0;
#pragma unroll
            for (int k = 0; k < RR_FLUSH_N; ++k) t = lane == k ? v[k] : t;
            if (t) atomicAdd(counters + slot * RR_CNT_STRIDE + flush_slot(lane, walk), t);
        }
        return;
    }
    __shared__ unsigned long long s_acc[4][RR_FLUSH_N];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {  // every field is wave-uniform
        const uint64_t v[RR_FLUSH_N] = {cnt.rays, cnt.shadow, cnt.shade, cnt.n1n2, cnt.gtests, cnt.ghits, cnt.tests,
                                        walk >= 0 ? (uint64_t)cnt.flops : 0ull, walk >= 0 ? (uint64_t)cnt.visits : 0ull,
                                        trace_flops, trace_visits, cnt.nan};
        for (int k = 0; k < RR_FLUSH_N; ++k) s_acc[w][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < RR_FLUSH_N) {
        const int k = threadIdx.x;
        const unsigned long long t = s_acc[0][k] + s_acc[1][k] + s_acc[2][k] + s_acc[3][k];
        if (t) atomicAdd(counters + (blockIdx.x & (RR_CNT_SLOTS - 1)) * RR_CNT_STRIDE + flush_slot(k, walk), t);
    }
}

__device__ __forceinline__ bool needs_n1n2(const DevMaterial& m, int rem) {
    // n1/n2 feed refracted_color (rem > 0, transparency != 0) and schlick (reflective > 0 &&
    // transparency > 0); both need transparency != 0.
    return m.transparency != 0.0 && (rem > 0 || m.reflective > 0.0);
}

// Counters are double-buffered per frame: the first level's kernels clear the buffer the next
// frame will count into, so no memset sits between frames.
// The kernels' prologue (segment / live count, counter clearing, the level-0 canvas mapping and camera ray)
// branches on kernel arguments one after the other, and the compiler loads each argument where the branch
// needs it: a chain of ~15 dependent scalar loads before the first ray.  Naming them in an empty asm
// statement at entry makes them all load together (one wait).
__device__ __forceinline__ void load_prologue_args(const LevelArgs& A) {
    asm volatile("" ::"s"(A.level), "s"(A.rays0), "s"(A.tile_fast), "s"(A.base), "s"(A.tiles_per_row), "s"(A.hs));
    asm volatile("" ::"s"(A.aa), "s"(A.part), "s"(A.nparts), "s"(A.block_rows), "s"(A.aa_magic), "s"(A.br_magic));
    asm volatile("" ::"s"(A.cam_affine), "s"(A.n), "s"(A.n_dev), "s"(A.nseg), "s"(A.counters_zero), "s"(A.lrows));
}
// The level kernels run 256-thread blocks on a grid of blocks_for(A.n) (launch_level_t): the block and grid
// sizes are taken from those instead of blockDim / gridDim, which read the dispatch's hidden arguments with a
// vector load that every wave waited for at its start.
constexpr uint32_t RR_BLOCK = 256;
__device__ __forceinline__ uint32_t level_grid(const LevelArgs& A) { return (uint32_t)((A.n + 255) / 256); }
__device__ __forceinline__ void zero_next_counters(const LevelArgs& A) {
    if (!A.counters_zero) return;
    const uint32_t total = RR_CNT_SLOTS * RR_CNT_STRIDE, stride = level_grid(A) * RR_BLOCK;
    for (uint32_t j = blockIdx.x * RR_BLOCK + threadIdx.x; j < total; j += stride) A.counters_zero[j] = 0ull;
}


// shade_hit's final sum (scene.rs:172-177) for given child results a (reflected) and b (refracted)
__device__ __forceinline__ V3 shade_sum(V3 s, V3 a, V3 b, double refl, double transp, double R) {
    if (refl > 0.0 && transp > 0.0) return vadd(vadd(s, vmul(a, R)), vmul(b, 1.0 - R));
    return vadd(vadd(s, a), b);
}

// A finished color_at value v of event i: level 0 writes the canvas; deeper levels become the
// parent's reflected_color (v * reflective, scene.rs:281-290) or refracted_color (v * transparency,
// scene.rs:310-336) slot.  Each slot has exactly one writer.
// With aa == 1 the box average of canvas.rs:85-96 is r = 0.0; r += p; r /= 1.0, written here
// directly (same operations) instead of through the canvas and aa_kernel.
// The averaged f64 image is written with nontemporal stores (here, deliver_wave_avg, deliver_pixel_wave): nothing in the
// frame reads it back, and streaming it past the caches measured C2 0.1186 -> 0.1173 ms and C4 0.508 -> 0.497 ms per
// frame (profiles/r05/ab_nt_output.txt; C3 and C5 unchanged)
__device__ __forceinline__ void deliver(int32_t level, int64_t i, int32_t parent, int32_t slot, V3 v, double* out,
                                        void* avg, int32_t avg_f32, CombRec* parent_comb, CombExt* parent_ext,
                                        int64_t out_index) {
    if (level == 0) {
        if (out) {
            double* o = out + 3 * out_index;
            o[0] = v.x;
            o[1] = v.y;
            o[2] = v.z;
        }
        if (avg) {
            const double a0 = (0.0 + v.x) / 1.0, a1 = (0.0 + v.y) / 1.0, a2 = (0.0 + v.z) / 1.0;
            if (avg_f32) {
                float* o = static_cast<float*>(avg) + 3 * out_index;
                o[0] = (float)a0;
                o[1] = (float)a1;
                o[2] = (float)a2;
            } else {
                double* o = static_cast<double*>(avg) + 3 * out_index;
                __builtin_nontemporal_store(a0, o);
                __builtin_nontemporal_store(a1, o + 1);
                __builtin_nontemporal_store(a2, o + 2);
            }
        }
        return;
    }
    if (slot) {  // a refracted child: the scene has transparency, so the parent has its CombExt
        CombExt& e = parent_ext[parent];
        const double t = e.transp;
        e.refr_res[0] = v.x * t;
        e.refr_res[1] = v.y * t;
        e.refr_res[2] = v.z * t;
    } else {
        CombRec& p = parent_comb[parent];
        const double t = p.refl;
        p.refl_res[0] = v.x * t;
        p.refl_res[1] = v.y * t;
        p.refl_res[2] = v.z * t;
    }
}

// canvas.rs:85-96 inside the wave (A.aa_wave = aa in {2, 4, 8}): a level-0 wave is one full 8x8 tile of the
// supersampled canvas (A.tile_fast), lane = 8 * row + column, and a tile holds whole aa x aa pixels (it
// starts on a multiple of 8 in both directions).  Every lane gathers its pixel's samples in the
// reference's order — r = 0.0; r += p (dy outer, dx inner) — and the pixel's first lane divides by aa^2
// and writes the averaged image: no supersampled canvas round trip through HBM, no aa_kernel.  Every lane
// of the wave must call it (shuffles); ls = the lane's part-local row-major sample index.
// a double moved across lanes by one DPP control (both halves); lanes without a source read 0
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// aa = 2: the pixel's samples sit at lanes +0, +1, +8, +9 of its first lane (even column, even row of the
// tile, so lanes 0-7 of a 16-lane DPP row): quad_perm [1,0,3,2] brings lane + 1, row_shl:8 lane + 8
__device__ __forceinline__ double box2(double p) {
    const double p1 = dpp_d<0xB1>(p);
    double r = 0.0;
    r += p;
    r += p1;
    r += dpp_d<0x108>(p);
    r += dpp_d<0x108>(p1);
    return r;
}
__device__ __forceinline__ void deliver_wave_avg(const LevelArgs& A, V3 v, const Px0& q, bool valid) {
    const int aa = A.aa_wave, m = aa - 1;
    const int lane = lane_id(), lx = lane & 7, ly = lane >> 3;
    double r = 0.0, g = 0.0, b = 0.0;
    if (aa == 2) {
        r = box2(v.x);
        g = box2(v.y);
        b = box2(v.z);
    } else {
        const int base = (ly & ~m) * 8 + (lx & ~m);
        for (int dy = 0; dy < aa; ++dy)
            for (int dx = 0; dx < aa; ++dx) {
                const int src = base + dy * 8 + dx;
                r += __shfl(v.x, src, 64);
                g += __shfl(v.y, src, 64);
                b += __shfl(v.z, src, 64);
            }
    }
    if (valid && (lx & m) == 0 && (ly & m) == 0) {
        // r / aa^2 with aa^2 a power of two: the same real number as r * 2^-2k, so both round alike (no division)
        const int sh = aa == 2 ? 1 : aa == 4 ? 2 : 3;
        const double inv_total = aa == 2 ? 0.25 : aa == 4 ? 0.0625 : 0.015625;
        const int64_t oi = (int64_t)(q.lrow >> sh) * (int64_t)((uint32_t)A.hs >> sh) + (q.px >> sh);
        if (A.avg_f32) {
            float* o = static_cast<float*>(A.avg) + 3 * oi;
            o[0] = (float)(r * inv_total);
            o[1] = (float)(g * inv_total);
            o[2] = (float)(b * inv_total);
        } else {
            double* o = static_cast<double*>(A.avg) + 3 * oi;
            __builtin_nontemporal_store(r * inv_total, o);
            __builtin_nontemporal_store(g * inv_total, o + 1);
            __builtin_nontemporal_store(b * inv_total, o + 2);
        }
    }
}

// canvas.rs:85-96 inside a pixel wave (A.pw): the pixel's 9 samples sit at lanes 9q .. 9q + 8 in the reference's order;
// its first lane sums them (r = 0.0; r += p) and writes r / 9.0.  The samples' colours are read from LDS (fin: the
// wave's [3][256]-double colour stage, this wave's slots at wave64), where the chain kernel leaves them.  The quotient
// is div_y's exact one (RN(r / 9) by Markstein's correction of r * RN(1/9), DESIGN.md §3) when every pixel's sums
// are 0 or of magnitude in [2^-500, 2^1000], else the IEEE division.  Every lane of the wave must call it.
__device__ __forceinline__ void deliver_pixel_wave(const LevelArgs& A, const double (*fin)[256], uint32_t wave64,
                                                   const Px0& q0, bool valid) {
    const int lane = lane_id();
    const int q = (lane * 57) >> 9, first = 9 * q;
    const bool mine = valid && lane == first;
    double r = 0.0, g = 0.0, b = 0.0;
    if (mine) {
        const int t0 = (int)wave64 + first;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            r += fin[0][t0 + k];
            g += fin[1][t0 + k];
            b += fin[2][t0 + k];
        }
    }
    const auto in_range = [](double v) {
        const double a = fabs(v);
        return v == 0.0 || (a >= 0x1p-500 && a <= 0x1p1000);
    };
    const bool exact_ok = !mine || (in_range(r) && in_range(g) && in_range(b));
    double qr, qg, qb;
    if (__ballot(!exact_ok) == 0) {
        const double y = 1.0 / 9.0;
        qr = div_y(r, 9.0, y);
        qg = div_y(g, 9.0, y);
        qb = div_y(b, 9.0, y);
    } else {
        const double total = 9.0;
        qr = r / total;
        qg = g / total;
        qb = b / total;
    }
    if (mine) {
        const int64_t oi = (int64_t)(q0.lrow / 3u) * (int64_t)((uint32_t)A.hs / 3u) + (q0.px / 3u);
        if (A.avg_f32) {
            float* o = static_cast<float*>(A.avg) + 3 * oi;
            o[0] = (float)qr;
            o[1] = (float)qg;
            o[2] = (float)qb;
        } else {
            double* o = static_cast<double*>(A.avg) + 3 * oi;
            __builtin_nontemporal_store(qr, o);
            __builtin_nontemporal_store(qg, o + 1);
            __builtin_nontemporal_store(qb, o + 2);
        }
    }
}

// ------------------------------------------------------------------ host-side launchers
static inline unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }
static inline size_t cull_lds(const DevScene& S) {
    return S.lds_culls ? (size_t)S.n_nodes * sizeof(DevCull) + (size_t)S.n_chunks * sizeof(DevChunk) : 0;
}

namespace {
struct Span {  // brackets one launch with events when profiling
    KernelProf* p;
    int id;
    hipStream_t st;
    hipEvent_t a = nullptr;
    Span(KernelProf* p_, int id_, hipStream_t st_) : p(p_), id(id_), st(st_) {
        if (p) {
            a = p->get();
            (void)hipEventRecord(a, st);
        }
    }
    ~Span() {
        if (p) {
            hipEvent_t b = p->get();
            (void)hipEventRecord(b, st);
            p->marks.push_back({id, {a, b}});
        }
    }
};
}  // namespace
