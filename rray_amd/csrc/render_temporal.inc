// render_temporal.inc — the kernel of temporal accumulation (DESIGN.md §3.24; rray.h RR_HAS_TEMPORAL holds the
// definition):
//   temporal_kernel<C, HAS_M2, TW>  one lane per pixel runs tp_pixel<C, HAS_M2> (temporal_tap.hpp, the host entry
//                                   rr_temporal_reference's own function) and writes out, n_out and m2_out
// Included by render_rays.hip inside namespace rr.  It reads no scene and needs no scratch: one launch per call.
//
// Lanes: a block is a tile of TW x (256 / TW) pixels, numbered row-major in a 1-D grid (W * H < 2^31, so at most 2^28
// tiles of a one-pixel-wide frame); a lane outside the frame leaves at once.  TW = 32 is the denoiser's 32 x 8 tile: a
// wave is two rows of 32, so under a small camera move its 2 x 2 gathers from the previous planes fall into three or
// four rows of about 33 pixels.  TW = 256 is the row-major map: a wave is 64 consecutive pixels, which suits the loads
// and stores of the pixel itself, and its gathers fall into two rows of about 65.  The host chooses (DESIGN.md §3.24).
// The constants are a by-value argument: uniform, so they are read with scalar loads into SGPRs.

template <int C, bool HAS_M2, int TW>
__global__ void __launch_bounds__(256) temporal_kernel(TpConst K, TpFrame cur, TpFrame prev, uint32_t tiles_x,
                                                       double* __restrict__ out, int32_t* __restrict__ n_out,
                                                       double* __restrict__ m2_out) {
    constexpr int TH = (int)RR_BLOCK / TW;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int64_t x = (int64_t)tx * TW + (threadIdx.x & (TW - 1));
    const int64_t y = (int64_t)ty * TH + (threadIdx.x / TW);
    if (x >= K.W || y >= K.H) return;
    double o[C], m2[C];
    int32_t n;
    tp_pixel<C, HAS_M2>(K, cur, prev, x, y, o, &n, m2);
    const int64_t p = y * K.W + x;
#pragma unroll
    for (int c = 0; c < C; ++c) out[C * p + c] = o[c];
    n_out[p] = n;
    if (HAS_M2) {
#pragma unroll
        for (int c = 0; c < C; ++c) m2_out[C * p + c] = m2[c];
    }
}

template <int C, bool HAS_M2>
static void launch_temporal_t(const TpConst& K, const TpFrame& cur, const TpFrame& prev, bool rows, double* out,
                              int32_t* n_out, double* m2_out, hipStream_t st) {
    if (rows) {
        const int64_t tiles_x = (K.W + 255) / 256;
        hipLaunchKernelGGL((temporal_kernel<C, HAS_M2, 256>), dim3((uint32_t)(tiles_x * K.H)), dim3(RR_BLOCK), 0, st, K, cur,
                           prev, (uint32_t)tiles_x, out, n_out, m2_out);
    } else {
        const int64_t tiles_x = (K.W + 31) / 32, tiles_y = (K.H + 7) / 8;
        hipLaunchKernelGGL((temporal_kernel<C, HAS_M2, 32>), dim3((uint32_t)(tiles_x * tiles_y)), dim3(RR_BLOCK), 0, st, K, cur,
                           prev, (uint32_t)tiles_x, out, n_out, m2_out);
    }
}

hipError_t launch_temporal(const TpConst& K, int32_t channels, const TpFrame& cur, const TpFrame& prev, bool rows,
                           double* out, int32_t* n_out, double* m2_out, hipStream_t st) {
    // W * H < 2^31 pixels, so either map has fewer than 2^31 tiles (at most W * H of them: a frame one pixel wide)
    if (K.W < 1 || K.H < 1 || K.W > ((int64_t)1 << 31) / K.H || K.W * K.H >= ((int64_t)1 << 31) ||
        (channels != 1 && channels != 3) || !cur.image || !cur.depth || !prev.image || !prev.depth || !prev.count || !out ||
        !n_out || (m2_out != nullptr) != (prev.m2 != nullptr) || ((K.terms & TP_T_OBJECT) && (!cur.object || !prev.object)) ||
        ((K.terms & TP_T_NORMAL) && (!cur.normal || !prev.normal)) || ((K.terms & TP_T_PLANE) && !cur.normal))
        return hipErrorInvalidValue;
    if (channels == 3) {
        if (m2_out)
            launch_temporal_t<3, true>(K, cur, prev, rows, out, n_out, m2_out, st);
        else
            launch_temporal_t<3, false>(K, cur, prev, rows, out, n_out, m2_out, st);
    } else {
        if (m2_out)
            launch_temporal_t<1, true>(K, cur, prev, rows, out, n_out, m2_out, st);
        else
            launch_temporal_t<1, false>(K, cur, prev, rows, out, n_out, m2_out, st);
    }
    return hipGetLastError();
}
