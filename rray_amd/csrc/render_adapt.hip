// render_adapt.hip — adaptive anti-aliasing around the level kernels (rr_render_adaptive):
//   adapt_mask_kernel     which pixels of the aa 1 frame differ from a neighbour by more than the threshold
//   adapt_scan_kernel     exclusive scan of the per-block counts; the totals, left on the device
//   adapt_scatter_kernel  the refined pixels' indices in ascending raster order (ballot + popcount in the wave)
//   adapt_resolve_kernel  canvas.rs:85-96 over each listed pixel's aa x aa samples, written over its aa 1 colour
// and the dispatch of the refine pass to the listed-pixel level kernels (namespace rr::listed: the units
// render_listed_*_g<G>_<lds|gl>, unit_*.hip compiled with the listed source).  Everything runs on the caller's stream; no count ever visits the host, and the list's order
// does not depend on which block runs first, so the refine pass's waves hold the same samples in every run.
#include <algorithm>
#include <cstdlib>

#include "device_core.inc"
#include "kernels.hpp"
#include "wavefront.hpp"

namespace rr {

static_assert(RR_ADAPT_BLOCK == 256, "the adapt kernels run four 64-lane waves per block");

// this lane's rank among the set lanes of its block's flags, and the block's total: the waves' ballots are
// summed through LDS.  Every thread of the (256-thread) block must call it.
__device__ __forceinline__ uint32_t block_rank(bool flag, uint32_t& total) {
    __shared__ uint32_t s_cnt[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t m = __ballot(flag);
    if (lane == 0) s_cnt[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0;
    for (int k = 0; k < 4; ++k) before += k < w ? s_cnt[k] : 0u;
    total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    const uint64_t below = lane == 0 ? 0ull : ((~0ull) >> (64 - lane));
    return before + (uint32_t)__popcll(m & below);
}

// Pixel p is refined iff some q of its 3x3 neighbourhood, clipped to the frame (q = p included), has
// !(max_c |F[p][c] - F[q][c]| <= thr).  The maximum propagates a NaN, so it is taken as "some channel fails the
// comparison": a NaN colour refines its whole neighbourhood, and a negative threshold refines every pixel (q = p).
__global__ void __launch_bounds__(RR_ADAPT_BLOCK) adapt_mask_kernel(AdaptArgs P) {
    const int64_t n = P.w * P.h;
    const int64_t p = (int64_t)blockIdx.x * RR_ADAPT_BLOCK + threadIdx.x;
    bool flag = false;
    if (p < n) {
        const int64_t y = p / P.w, x = p - y * P.w;
        const double* f = P.frame + 3 * p;
        const double a0 = f[0], a1 = f[1], a2 = f[2];
        const int64_t y0 = y > 0 ? y - 1 : y, y1 = y + 1 < P.h ? y + 1 : y;
        const int64_t x0 = x > 0 ? x - 1 : x, x1 = x + 1 < P.w ? x + 1 : x;
        for (int64_t qy = y0; qy <= y1; ++qy)
            for (int64_t qx = x0; qx <= x1; ++qx) {
                const double* g = P.frame + 3 * (qy * P.w + qx);
                const bool same = fabs(a0 - g[0]) <= P.thr && fabs(a1 - g[1]) <= P.thr && fabs(a2 - g[2]) <= P.thr;
                flag = flag || !same;
            }
        P.flags[p] = flag ? 1 : 0;
        if (P.mask) P.mask[p] = flag ? 1 : 0;
    }
    uint32_t total;
    (void)block_rank(flag, total);
    if (threadIdx.x == 0) P.block_count[blockIdx.x] = total;
}

// block_count -> exclusive prefix, in place, by one block: 256 counts at a time (Hillis-Steele in LDS) behind a
// running total.  32 400 counts for a 3840 x 2160 frame: 127 rounds.
__global__ void __launch_bounds__(256) adapt_scan_kernel(AdaptArgs P, int64_t n_blocks) {
    __shared__ uint32_t v[256];
    const int t = threadIdx.x;
    uint32_t carry = 0;
    for (int64_t b0 = 0; b0 < n_blocks; b0 += 256) {
        const uint32_t c = b0 + t < n_blocks ? P.block_count[b0 + t] : 0u;
        v[t] = c;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const uint32_t a = t >= off ? v[t - off] : 0u;
            __syncthreads();
            v[t] += a;
            __syncthreads();
        }
        if (b0 + t < n_blocks) P.block_count[b0 + t] = carry + v[t] - c;
        carry += v[255];
        __syncthreads();
    }
    if (t == 0) {
        P.counts[0] = carry;
        P.counts[1] = carry * (uint32_t)(P.aa * P.aa);  // < 2^32: the frame's samples fit one pass (api.cpp)
        if (P.n_refined) *P.n_refined = (int64_t)carry;
    }
}

__global__ void __launch_bounds__(RR_ADAPT_BLOCK) adapt_scatter_kernel(AdaptArgs P) {
    const int64_t n = P.w * P.h;
    const int64_t p = (int64_t)blockIdx.x * RR_ADAPT_BLOCK + threadIdx.x;
    const bool flag = p < n && P.flags[p] != 0;
    uint32_t total;
    const uint32_t rank = block_rank(flag, total);
    if (flag) P.list[P.block_count[blockIdx.x] + rank] = (uint32_t)p;
}

// canvas.rs:85-96 for listed pixel j: its samples are events j * aa^2 .. of the refine pass, in the reference's
// order (dy outer, dx inner): r = 0.0; r += p; r / (aa * aa) as f64 (an IEEE division)
__global__ void __launch_bounds__(256) adapt_resolve_kernel(AdaptArgs P) {
    const int64_t n_list = (int64_t)P.counts[0];
    const int64_t aa2 = (int64_t)P.aa * P.aa;
    const double total = (double)(P.aa * P.aa);
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_list; j += (int64_t)gridDim.x * blockDim.x) {
        const double* s = P.samples + 3 * j * aa2;
        double r = 0.0, g = 0.0, b = 0.0;
        for (int64_t k = 0; k < aa2; ++k) {
            r += s[3 * k];
            g += s[3 * k + 1];
            b += s[3 * k + 2];
        }
        double* o = P.avg + 3 * (int64_t)P.list[j];
        o[0] = r / total;
        o[1] = g / total;
        o[2] = b / total;
    }
}

hipError_t launch_adapt_select(const AdaptArgs& P, hipStream_t st) {
    const int64_t n = P.w * P.h;
    if (n <= 0) return hipErrorInvalidValue;
    const int64_t n_blocks = (n + RR_ADAPT_BLOCK - 1) / RR_ADAPT_BLOCK;
    hipLaunchKernelGGL(adapt_mask_kernel, dim3((unsigned)n_blocks), dim3(RR_ADAPT_BLOCK), 0, st, P);
    hipLaunchKernelGGL(adapt_scan_kernel, dim3(1), dim3(256), 0, st, P, n_blocks);
    hipLaunchKernelGGL(adapt_scatter_kernel, dim3((unsigned)n_blocks), dim3(RR_ADAPT_BLOCK), 0, st, P);
    return hipGetLastError();
}

hipError_t launch_adapt_resolve(const AdaptArgs& P, hipStream_t st) {
    const int64_t n = P.w * P.h;
    if (n <= 0) return hipErrorInvalidValue;
    // grid-stride over the live count: the capacity (every pixel) is usually far above it
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(adapt_resolve_kernel, dim3(grid), dim3(256), 0, st, P);
    return hipGetLastError();
}

// the refine pass's level-0 launch, by the scene's kernel family as launch_level / launch_chain / launch_tree; an
// ordered ray batch (A.rays0 with A.list its permutation) takes the same launches with a host count
hipError_t launch_level_listed(const DevScene& S, const LevelArgs& A, hipStream_t st, KernelProf* prof) {
    if (A.n <= 0) return hipSuccess;
    if (!A.list || (!A.n_dev && !A.rays0) || A.level != 0 || !fused_levels(S)) return hipErrorInvalidValue;
    dispatch_glc(S, [&](auto g, auto lc) { listed::launch_level_t<g(), lc()>(S, A, st, prof); });
    return hipGetLastError();
}

hipError_t launch_chain_listed(const DevScene& S, const LevelArgs& A, hipStream_t st, KernelProf* prof) {
    if (A.n <= 0) return hipSuccess;
    if (!A.list || (!A.n_dev && !A.rays0) || A.level != 0) return hipErrorInvalidValue;
    dispatch_glc(S, [&](auto g, auto lc) { listed::launch_chain_t<g(), lc()>(S, A, st, prof, false); });
    return hipGetLastError();
}

hipError_t launch_tree_listed(const DevScene& S, const LevelArgs& A, hipStream_t st, KernelProf* prof) {
    if (A.n <= 0) return hipSuccess;
    if (!A.list || (!A.n_dev && !A.rays0) || A.level != 0) return hipErrorInvalidValue;
    dispatch_glc(S, [&](auto g, auto lc) { listed::launch_tree_t<g(), lc()>(S, A, st, prof); });
    return hipGetLastError();
}

}  // namespace rr
