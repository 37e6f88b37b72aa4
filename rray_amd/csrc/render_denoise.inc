// render_denoise.inc — the kernels of the edge-avoiding denoiser (DESIGN.md §3.22; rray.h RR_HAS_DENOISE holds the
// definition):
//   denoise_pack_kernel      once per call: a pixel's depth, normal, albedo and object id, rounded to float as the
//                            definition reads them, into one 32-byte DnGuide record whose id < 0 is the void flag
//   denoise_level_kernel<C>  once per level: one lane per pixel runs dn_pixel<C> (denoise_tap.hpp, the host entry
//                            rr_denoise_reference's own function) on the level's source image and the records
//   denoise_level_lds_kernel<C, S>  the same level for holes of S = 1 or 2 pixels with the tile and its halo of 2 S
//                            pixels staged in LDS first (the A/B of DESIGN.md §3.22; chosen per level by the host)
// Included by render_rays.hip inside namespace rr.  None reads the scene.
//
// Lanes: a block is a tile of DN_TW x DN_TH = 32 x 8 pixels and a wave two rows of 32, so every tap of a wave is two
// runs of 32 consecutive pixels (768 bytes of colour at C = 3, 1 KiB of records) whatever the level's hole.  The taps
// of neighbouring pixels overlap, and those re-reads are served by the vector L1 and L2; what a level must move from
// HBM is its image and the records once.  Tiles are numbered row-major in a 1-D grid (W * H < 2^31, so at most 2^28
// tiles of a one-pixel-wide frame), and a lane outside the frame leaves at once.

constexpr int DN_TW = 32, DN_TH = 8;
static_assert(DN_TW * DN_TH == (int)RR_BLOCK, "a denoiser tile is one block");

__global__ void __launch_bounds__(256) denoise_pack_kernel(int64_t n, const double* __restrict__ depth,
                                                           const double* __restrict__ normal,
                                                           const int32_t* __restrict__ object,
                                                           const double* __restrict__ albedo, DnGuide* __restrict__ g) {
    const int64_t p = (int64_t)blockIdx.x * RR_BLOCK + threadIdx.x;
    if (p >= n) return;
    g[p] = dn_guide(p, depth, normal, object, albedo);
}

template <int C>
__global__ void __launch_bounds__(256) denoise_level_kernel(DnLevel L, int64_t W, int64_t H, uint32_t tiles_x,
                                                            const double* __restrict__ src,
                                                            const DnGuide* __restrict__ g, double* __restrict__ dst) {
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int64_t x = (int64_t)tx * DN_TW + (threadIdx.x & (DN_TW - 1));
    const int64_t y = (int64_t)ty * DN_TH + (threadIdx.x / DN_TW);
    if (x >= W || y >= H) return;
    double out[C];
    dn_pixel<C>(L, W, H, x, y, src, g, out);
    double* o = dst + C * (y * W + x);
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = out[c];
}

// The LDS form.  A block stages its 32 x 8 tile with a halo of 2 S pixels on every side — (32 + 4 S) x (8 + 4 S) pixels:
// 36 x 12 at S = 1, 40 x 16 at S = 2 — and every lane then takes its 25 taps from the stage through the same dn_pixel_at.
// Layout: structure of arrays, one plane of doubles per channel and the 32-byte record as two planes of 16-byte halves.
// A wave's tap is two rows of 32 consecutive pixels: the 32 lanes of a half-wave read 32 consecutive doubles (256 bytes:
// every bank once, whatever the row's start) and 32 consecutive 16-byte halves (each 16-lane group of ds_read_b128 its 16
// consecutive slots), so no read is 2-way; records kept whole at their 32-byte stride would put two lanes of every
// 16-lane group on each slot, and a whole 56-byte pixel would not even keep them 16-byte aligned.  Pixels of the halo outside the frame are staged as void and never read (dn_pixel_at asks only for
// pixels inside the frame).  LDS: (8 C + 32) bytes per staged pixel: 24,192 bytes at S = 1 and 35,840 at S = 2 for C = 3.
template <int C, int S>
__global__ void __launch_bounds__(256) denoise_level_lds_kernel(DnLevel L, int64_t W, int64_t H, uint32_t tiles_x,
                                                                const double* __restrict__ src,
                                                                const DnGuide* __restrict__ g, double* __restrict__ dst) {
    constexpr int SW = DN_TW + 4 * S, SH = DN_TH + 4 * S, SN = SW * SH;
    __shared__ double s_col[C][SN];
    __shared__ float4 s_g0[SN], s_g1[SN];
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int64_t x0 = (int64_t)tx * DN_TW - 2 * S, y0 = (int64_t)ty * DN_TH - 2 * S;  // the stage's corner in the frame
    for (int k = threadIdx.x; k < SN; k += (int)RR_BLOCK) {
        const int sy = k / SW, sx = k - sy * SW;
        const int64_t qx = x0 + sx, qy = y0 + sy;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
        b.w = __int_as_float(-1);  // void
        double col[C];
#pragma unroll
        for (int c = 0; c < C; ++c) col[c] = 0.0;
        if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
            const int64_t q = qy * W + qx;
            const float4* gq = reinterpret_cast<const float4*>(g + q);
            a = gq[0];
            b = gq[1];
#pragma unroll
            for (int c = 0; c < C; ++c) col[c] = src[C * q + c];
        }
        s_g0[k] = a;
        s_g1[k] = b;
#pragma unroll
        for (int c = 0; c < C; ++c) s_col[c][k] = col[c];
    }
    __syncthreads();
    const int64_t x = (int64_t)tx * DN_TW + (threadIdx.x & (DN_TW - 1));
    const int64_t y = (int64_t)ty * DN_TH + (threadIdx.x / DN_TW);
    if (x >= W || y >= H) return;
    const auto img = [&](int64_t qx, int64_t qy, int c) -> double { return s_col[c][(int)(qy - y0) * SW + (int)(qx - x0)]; };
    const auto guide = [&](int64_t qx, int64_t qy) -> DnGuide {
        const int k = (int)(qy - y0) * SW + (int)(qx - x0);
        const float4 a = s_g0[k], b = s_g1[k];
        DnGuide r;
        r.z = a.x;
        r.n[0] = a.y;
        r.n[1] = a.z;
        r.n[2] = a.w;
        r.a[0] = b.x;
        r.a[1] = b.y;
        r.a[2] = b.z;
        r.id = __float_as_int(b.w);
        return r;
    };
    DnLevel Ls = L;
    Ls.step = S;  // a constant: the taps' stage offsets fold
    double out[C];
    dn_pixel_at<C>(Ls, W, H, x, y, img, guide, out);
    double* o = dst + C * (y * W + x);
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = out[c];
}

hipError_t launch_denoise_pack(int64_t n, const double* depth, const double* normal, const int32_t* object,
                               const double* albedo, DnGuide* guides, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!guides || n >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(denoise_pack_kernel, dim3(blocks_for(n)), dim3(RR_BLOCK), 0, st, n, depth, normal, object, albedo,
                       guides);
    return hipGetLastError();
}

template <int C>
static void launch_denoise_level_t(const DnLevel& L, bool lds, int64_t W, int64_t H, uint32_t tiles, uint32_t tiles_x,
                                   const double* src, const DnGuide* guides, double* dst, hipStream_t st) {
    if (lds && L.step == 1)
        hipLaunchKernelGGL((denoise_level_lds_kernel<C, 1>), dim3(tiles), dim3(RR_BLOCK), 0, st, L, W, H, tiles_x, src, guides, dst);
    else if (lds && L.step == 2)
        hipLaunchKernelGGL((denoise_level_lds_kernel<C, 2>), dim3(tiles), dim3(RR_BLOCK), 0, st, L, W, H, tiles_x, src, guides, dst);
    else
        hipLaunchKernelGGL(denoise_level_kernel<C>, dim3(tiles), dim3(RR_BLOCK), 0, st, L, W, H, tiles_x, src, guides, dst);
}

hipError_t launch_denoise_level(const DnLevel& L, bool lds, int32_t channels, int64_t W, int64_t H, const double* src,
                                const DnGuide* guides, double* dst, hipStream_t st) {
    if (!src || !guides || !dst || src == dst || W < 1 || H < 1 || W > ((int64_t)1 << 31) / H || W * H >= ((int64_t)1 << 31) ||
        L.step < 1 || L.step > 128 || (channels != 1 && channels != 3))
        return hipErrorInvalidValue;
    const int64_t tiles_x = (W + DN_TW - 1) / DN_TW, tiles_y = (H + DN_TH - 1) / DN_TH;
    const int64_t tiles = tiles_x * tiles_y;  // at most 2^28 (a frame one pixel wide): W * H < 2^31
    if (tiles >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    if (channels == 3)
        launch_denoise_level_t<3>(L, lds, W, H, (uint32_t)tiles, (uint32_t)tiles_x, src, guides, dst, st);
    else
        launch_denoise_level_t<1>(L, lds, W, H, (uint32_t)tiles, (uint32_t)tiles_x, src, guides, dst, st);
    return hipGetLastError();
}
