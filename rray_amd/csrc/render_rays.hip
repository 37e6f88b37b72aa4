// render_rays.hip — the two kernels of the device-resident ray queries:
//   camera_rays_kernel  Camera::ray_for_pixel (camera.rs:75-93) of every canvas sample into a caller's ray buffer
//                       (rr_camera_rays_device), by render_common.inc's camera_ray: the frames' own arithmetic
//   hit_records_kernel  one pass of hit_kernel's ray-batch planes (HitOut.rec_i / rec_d) -> rr_hit records in the
//                       caller's buffer (rr_hit_at_device)
//   hit_records_ordered_kernel  the same with a scattered destination: the record of pass slot j goes to ray
//                       perm[j]'s place (rr_hit_at_device_ordered)
//   render_order.inc    the coherent order of a ray batch: bounds, keys and a stable radix sort (rr_ray_order_device)
//   render_lens.inc     the lens frames' ray generator and resolve step (rr_lens_rays_device, rr_render_lens_device)
//   render_ao.inc       the ambient-occlusion pairs and resolve kernels (rr_ao_at_device, rr_render_ao_device): the one
//                       part of this unit that walks the scene, with shadow_query_kernel's shadowed<> instantiation
//   render_denoise.inc  the edge-avoiding denoiser's pack and level kernels (rr_denoise_device), by denoise_tap.hpp
//   render_indirect.inc the one-bounce indirect rays, their live list and the resolve step (rr_indirect_at_device,
//                       rr_render_indirect_device)
//   render_temporal.inc temporal accumulation's one kernel (rr_temporal_device), by temporal_tap.hpp
//   render_denoise_var.inc  the per-pixel noise estimate and the variance-guided levels (rr_variance_device,
//                       rr_denoise_var_device), by denoise_var_tap.hpp
// None of the others reads the scene.  The queries' walks are the existing kernels' (hit_kernel's ray-batch instantiation, the
// colour families with A.rays0, shadow_query_kernel), launched on the caller's buffers as they are.
#include <algorithm>
#include <cstdlib>

#include "ao_dir.hpp"
#include "denoise_tap.hpp"
#include "denoise_var_tap.hpp"
#include "device_core.inc"
#include "kernels.hpp"
#include "temporal_tap.hpp"
#include "wavefront.hpp"

namespace rr {
#include "render_common.inc"

// One lane per ray, row-major: ray i is sample (i % hsize, i / hsize) in 32-bit arithmetic (n < 2^32, host-checked).
// The last wave may be short.  A lane's six doubles are 48 consecutive bytes and a wave's rays 3 KiB of consecutive
// cache lines, each written whole by the wave's six stores.
__global__ void __launch_bounds__(256) camera_rays_kernel(DevCamera C, int32_t affine, uint32_t hsize, int64_t n,
                                                          double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * RR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = (uint32_t)i;
    const uint32_t py = t / hsize, px = t - py * hsize;
    const Ray r = camera_ray(C, affine != 0, px, py);
    double* o = out + 6 * i;
    o[0] = r.o.x;
    o[1] = r.o.y;
    o[2] = r.o.z;
    o[3] = r.d.x;
    o[4] = r.d.y;
    o[5] = r.d.z;
}

// rr_hit as 8-byte words: word 0 = {object (low), inside (high)}, words 1..23 = the RR_HIT_DOUBLES planes in the
// struct's order.  A block turns RR_REC_TILE consecutive records of the pass into records: the planes are read 64
// consecutive entries per wave (whole 512-byte runs of one plane; the int planes 256-byte runs) into an LDS tile, and
// the tile goes out as RR_REC_TILE * 24 consecutive words, lane after lane, so every store instruction of a wave covers
// four whole cache lines.  The tile is field-major with rows padded by one word: the plane-side writes are
// conflict-free, the record-side reads at most two-way.  Any pass size >= 1: a short last tile reads and writes only
// its n - first records.
constexpr int RR_REC_WORDS = 1 + RR_HIT_DOUBLES;  // 24
constexpr int RR_REC_TILE = 64;
constexpr int RR_REC_ROW = RR_REC_TILE + 1;
static_assert(RR_REC_WORDS * 8 == 192, "rr_hit is 24 words of 8 bytes (rray.h)");
static_assert(RR_REC_WORDS % 4 == 0 && (RR_REC_TILE * RR_REC_WORDS) % (int)RR_BLOCK == 0, "whole block iterations");

// ORD: record r of the tile goes to out + RR_REC_WORDS * perm[first + r] (whole records still: 24 consecutive words
// each, so a wave's store covers whole 64-byte runs of 2 to 3 records), else to out + RR_REC_WORDS * (first + r).
template <bool ORD>
__device__ __forceinline__ void hit_records_body(const int32_t* __restrict__ rec_i, const double* __restrict__ rec_d,
                                                 int64_t stride, int64_t n, const uint32_t* __restrict__ perm,
                                                 unsigned long long* __restrict__ out) {
    __shared__ unsigned long long tile[RR_REC_WORDS * RR_REC_ROW];
    __shared__ uint32_t dest[ORD ? RR_REC_TILE : 1];
    const int64_t first = (int64_t)blockIdx.x * RR_REC_TILE;
    const int64_t left = n - first;
    const int m = left < RR_REC_TILE ? (int)left : RR_REC_TILE;  // records of this tile (>= 1: the grid is ceil)
    const int r = (int)(threadIdx.x & 63u), w4 = (int)(threadIdx.x >> 6);
    if constexpr (ORD) {
        if (w4 == 0 && r < m) dest[r] = perm[first + r];
    }
#pragma unroll
    for (int it = 0; it < RR_REC_WORDS / 4; ++it) {  // four planes per step, one per wave
        const int f = it * 4 + w4;
        unsigned long long v = 0ull;
        if (r < m) {
            const int64_t j = first + r;
            if (f == 0) {
                const uint32_t object = (uint32_t)rec_i[j], inside = (uint32_t)rec_i[stride + j];
                v = (unsigned long long)object | ((unsigned long long)inside << 32);
            } else {
                v = (unsigned long long)__double_as_longlong(rec_d[(int64_t)(f - 1) * stride + j]);
            }
        }
        tile[f * RR_REC_ROW + r] = v;
    }
    __syncthreads();
    unsigned long long* o = out + first * RR_REC_WORDS;
    const int words = m * RR_REC_WORDS;
#pragma unroll
    for (int it = 0; it < RR_REC_TILE * RR_REC_WORDS / (int)RR_BLOCK; ++it) {
        const int w = it * (int)RR_BLOCK + (int)threadIdx.x;
        const int rec = w / RR_REC_WORDS, f = w - rec * RR_REC_WORDS;
        if (w < words) {
            if constexpr (ORD)
                out[(int64_t)dest[rec] * RR_REC_WORDS + f] = tile[f * RR_REC_ROW + rec];
            else
                o[w] = tile[f * RR_REC_ROW + rec];
        }
    }
}

__global__ void __launch_bounds__(256) hit_records_kernel(const int32_t* __restrict__ rec_i,
                                                          const double* __restrict__ rec_d, int64_t stride, int64_t n,
                                                          unsigned long long* __restrict__ out) {
    hit_records_body<false>(rec_i, rec_d, stride, n, nullptr, out);
}

// perm: the pass's entries of the order (perm[j]: the ray of pass slot j), each < the batch's n — not checked
__global__ void __launch_bounds__(256) hit_records_ordered_kernel(const int32_t* __restrict__ rec_i,
                                                                  const double* __restrict__ rec_d, int64_t stride,
                                                                  int64_t n, const uint32_t* __restrict__ perm,
                                                                  unsigned long long* __restrict__ out) {
    hit_records_body<true>(rec_i, rec_d, stride, n, perm, out);
}

#include "render_order.inc"
#include "render_lens.inc"
#include "render_ao.inc"
#include "render_indirect.inc"
#include "render_denoise.inc"
#include "render_denoise_var.inc"
#include "render_temporal.inc"

hipError_t launch_camera_rays(const DevCamera& cam, bool affine, int64_t n, double* out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!out || cam.hsize < 1 || cam.vsize < 1 || n != cam.hsize * cam.vsize || n >= ((int64_t)1 << 32))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(camera_rays_kernel, dim3(blocks_for(n)), dim3(RR_BLOCK), 0, st, cam, affine ? 1 : 0,
                       (uint32_t)cam.hsize, n, out);
    return hipGetLastError();
}

hipError_t launch_hit_records(const HitOut& O, int64_t n, void* out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!O.rec_i || !O.rec_d || !out || O.stride < n || n > ((int64_t)1 << 24)) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((n + RR_REC_TILE - 1) / RR_REC_TILE);
    hipLaunchKernelGGL(hit_records_kernel, dim3(grid), dim3(RR_BLOCK), 0, st, O.rec_i, O.rec_d, O.stride, n,
                       static_cast<unsigned long long*>(out));
    return hipGetLastError();
}

hipError_t launch_hit_records_ordered(const HitOut& O, int64_t n, const uint32_t* perm, void* out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!O.rec_i || !O.rec_d || !out || !perm || O.stride < n || n > ((int64_t)1 << 24)) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((n + RR_REC_TILE - 1) / RR_REC_TILE);
    hipLaunchKernelGGL(hit_records_ordered_kernel, dim3(grid), dim3(RR_BLOCK), 0, st, O.rec_i, O.rec_d, O.stride, n, perm,
                       static_cast<unsigned long long*>(out));
    return hipGetLastError();
}

// one pass of an ordered ray batch through the first-hit kernel's listed instantiation (render_hit.inc under RR_LISTED)
hipError_t launch_hit_ordered(const DevScene& S, const LevelArgs& A, const HitOut& O, hipStream_t st) {
    if (A.n <= 0) return hipSuccess;
    if (!A.rays0 || !A.list || A.n_dev || A.level != 0 || A.base != 0 || !O.rec_i || !O.rec_d || O.stride < A.n)
        return hipErrorInvalidValue;
    dispatch_glc(S, [&](auto g, auto lc) { listed::launch_hit_t<g(), lc()>(S, A, O, st); });
    return hipGetLastError();
}

}  // namespace rr
