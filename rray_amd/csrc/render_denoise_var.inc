// render_denoise_var.inc — the kernels of variance-guided denoising (DESIGN.md §3.25; rray.h RR_HAS_DENOISE_VAR holds
// the definition):
//   variance_kernel<C>            once per rr_variance call: one lane per pixel runs dv_variance<C> (denoise_var_tap.hpp,
//                                 the host entry rr_variance_reference's own function) on the image, the moments and
//                                 counts of rr_temporal where they are given, and the records of denoise_pack_kernel
//   denoise_var_level_kernel<C>   once per level of rr_denoise_var: one lane per pixel runs dv_pixel<C> on the level's
//                                 source image and variance plane and writes both of the next level
// Included by render_rays.hip inside namespace rr, behind render_denoise.inc, whose pack kernel, tile and lane map they
// share: a block is a tile of 32 x 8 pixels numbered row-major in a 1-D grid, a wave two rows of 32, and a lane outside
// the frame leaves at once.  None reads the scene.  Direct forms only: the taps' re-reads are served by the vector L1
// and L2 as in denoise_level_kernel, whose levels §3.22 found bound by f64 division and not by memory.
//
// variance_kernel: a lane whose pixel has enough history takes the short branch (three loads, one division); the others
// walk the 7 x 7 window.  A wave that holds both runs the window for its spatial lanes only, under their exec mask, and
// the lanes are not compacted: after the first frames only disoccluded pixels are spatial, they come in clusters along
// silhouettes, and a compaction would cost every frame a scan and a list for them (DESIGN.md §3.25).

template <int C>
__global__ void __launch_bounds__(256) variance_kernel(DnLevel G, int32_t min_history, int64_t W, int64_t H,
                                                       uint32_t tiles_x, const double* __restrict__ in,
                                                       const double* __restrict__ m2, const int32_t* __restrict__ count,
                                                       const DnGuide* __restrict__ g, double* __restrict__ var) {
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int64_t x = (int64_t)tx * DN_TW + (threadIdx.x & (DN_TW - 1));
    const int64_t y = (int64_t)ty * DN_TH + (threadIdx.x / DN_TW);
    if (x >= W || y >= H) return;
    var[y * W + x] = dv_variance<C>(G, min_history, W, H, x, y, in, g, m2, count);
}

// vdst may be null (the last level of a call without var_out): the variance of the filtered image is then not stored
template <int C>
__global__ void __launch_bounds__(256) denoise_var_level_kernel(DnLevel L, double epsilon, int64_t W, int64_t H,
                                                                uint32_t tiles_x, const double* __restrict__ src,
                                                                const double* __restrict__ vsrc,
                                                                const DnGuide* __restrict__ g, double* __restrict__ dst,
                                                                double* __restrict__ vdst) {
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int64_t x = (int64_t)tx * DN_TW + (threadIdx.x & (DN_TW - 1));
    const int64_t y = (int64_t)ty * DN_TH + (threadIdx.x / DN_TW);
    if (x >= W || y >= H) return;
    double out[C], vout;
    dv_pixel<C>(L, epsilon, W, H, x, y, src, vsrc, g, out, &vout);
    double* o = dst + C * (y * W + x);
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = out[c];
    if (vdst) vdst[y * W + x] = vout;
}

// the row-major 1-D grid of 32 x 8 tiles of a W x H frame (W * H < 2^31: at most 2^28 tiles of a one-pixel-wide frame)
static bool dv_tiles(int64_t W, int64_t H, uint32_t* tiles, uint32_t* tiles_x) {
    if (W < 1 || H < 1 || W > ((int64_t)1 << 31) / H || W * H >= ((int64_t)1 << 31)) return false;
    const int64_t nx = (W + DN_TW - 1) / DN_TW, ny = (H + DN_TH - 1) / DN_TH;
    if (nx * ny >= ((int64_t)1 << 31)) return false;
    *tiles = (uint32_t)(nx * ny);
    *tiles_x = (uint32_t)nx;
    return true;
}

hipError_t launch_variance(const DnLevel& G, int32_t min_history, int32_t channels, int64_t W, int64_t H, const double* in,
                           const double* m2, const int32_t* count, const DnGuide* guides, double* var, hipStream_t st) {
    uint32_t tiles = 0, tiles_x = 0;
    if (!in || !guides || !var || (m2 != nullptr) != (count != nullptr) || G.step != 1 || (G.terms & DN_T_COLOR) ||
        (channels != 1 && channels != 3) || !dv_tiles(W, H, &tiles, &tiles_x))
        return hipErrorInvalidValue;
    if (channels == 3)
        hipLaunchKernelGGL(variance_kernel<3>, dim3(tiles), dim3(RR_BLOCK), 0, st, G, min_history, W, H, tiles_x, in, m2, count,
                           guides, var);
    else
        hipLaunchKernelGGL(variance_kernel<1>, dim3(tiles), dim3(RR_BLOCK), 0, st, G, min_history, W, H, tiles_x, in, m2, count,
                           guides, var);
    return hipGetLastError();
}

hipError_t launch_denoise_var_level(const DnLevel& L, double epsilon, int32_t channels, int64_t W, int64_t H,
                                    const double* src, const double* vsrc, const DnGuide* guides, double* dst, double* vdst,
                                    hipStream_t st) {
    uint32_t tiles = 0, tiles_x = 0;
    if (!src || !vsrc || !guides || !dst || src == dst || vsrc == vdst || L.step < 1 || L.step > 128 ||
        (channels != 1 && channels != 3) || !dv_tiles(W, H, &tiles, &tiles_x))
        return hipErrorInvalidValue;
    if (channels == 3)
        hipLaunchKernelGGL(denoise_var_level_kernel<3>, dim3(tiles), dim3(RR_BLOCK), 0, st, L, epsilon, W, H, tiles_x, src, vsrc,
                           guides, dst, vdst);
    else
        hipLaunchKernelGGL(denoise_var_level_kernel<1>, dim3(tiles), dim3(RR_BLOCK), 0, st, L, epsilon, W, H, tiles_x, src, vsrc,
                           guides, dst, vdst);
    return hipGetLastError();
}
