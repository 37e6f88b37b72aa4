// render_ao.inc — the kernels of the ambient-occlusion queries and frames (DESIGN.md §3.21; rray.h RR_HAS_AO holds the
// definition):
//   camera_rays_window_kernel  a pass's window of the camera's rays (the frames only)
//   ao_pairs_kernel<G, LC>  one lane per (point, k) pair, pair j = i * K + k: the lane builds occlusion ray k of point i
//                           with ao_dir.hpp (the host entry rr_ao_directions' own functions) and walks the segment with
//                           shadowed<G, LC, true, cross_lane_ok(G, false, false)>, the instantiation shadow_query_kernel
//                           uses, so a pair's answer is rr_is_shadowed_device's by construction; the occluded pairs of
//                           a point are counted into count[i]
//   ao_resolve_kernel       count -> (double)(K - c) / (double)K (a miss took part in no walk: count 0, value 1.0)
// Included by render_rays.hip inside namespace rr.  The K rays of a point sit in adjacent lanes, share their origin and
// are at most `radius` long, so the walk's f32 bundle cull sees a ball around the wave's few points.

// One lane per pair.  n_pairs = n * K < 2^32 (host-checked), so the point and sample indices are 32-bit divisions.
// A lane whose point is a miss (I.object[i] < 0) or that lies past the batch stays in the walk inactive, with
// shadow_query_kernel's placeholder segment.  Counting: when K divides 64 a point's K lanes are one aligned segment of
// one wave (blocks of 256 lanes start at a multiple of 64 pairs, and i * K is a multiple of K), so the segment's first
// lane stores the popcount of its part of the ballot — no atomic, no cleared buffer; otherwise every occluded lane adds
// 1 to count[i] with a vector atomic (the host clears count first).  The sum is an integer either way: the value does
// not depend on the order in which the walks finish.
template <int G, bool LC>
__global__ void __launch_bounds__(256) ao_pairs_kernel(DevScene S, DevAo P, AoPoints I, int64_t n_pairs,
                                                       int32_t* __restrict__ count, unsigned long long* counters) {
    if (LC) stage_culls(S);
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = j < n_pairs;
    const uint32_t K = P.samples;
    const uint32_t jj = valid ? (uint32_t)j : 0u;
    const uint32_t i = jj / K, k = jj - i * K;
    bool active = valid;
    if (valid && I.object) active = I.object[i] >= 0;
    Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    V3 p = mk(0, 0, 0), l = mk(0, 0, 1);
    if (active) {
        const double* pp = I.points + (int64_t)i * I.point_stride;
        const double* np = I.normals + (int64_t)i * I.point_stride;
        const double N[3] = {np[0], np[I.comp_stride], np[2 * I.comp_stride]};
        double w[3];
        ao_direction(ao_base(P.seed, (uint64_t)I.first + i), k, N, w);
        p = mk(pp[0], pp[I.comp_stride], pp[2 * I.comp_stride]);
        l = mk(p.x + P.radius * w[0], p.y + P.radius * w[1], p.z + P.radius * w[2]);
    }
    const bool sh = shadowed<G, LC, true, cross_lane_ok(G, false, false)>(S, p, l, active, cnt) && active;
    const unsigned long long m = __ballot(sh);
    if (64u % K == 0u) {
        if (valid && k == 0u) {
            const unsigned long long seg = m >> (threadIdx.x & 63u);
            count[i] = __popcll(K == 64u ? seg : seg & ((1ull << K) - 1ull));
        }
    } else if (sh) {
        atomicAdd(count + i, 1);
    }
    flush(cnt, counters, W_SHADOW);
}

__global__ void __launch_bounds__(256) ao_resolve_kernel(const int32_t* __restrict__ count, uint32_t samples, int64_t n,
                                                         double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * RR_BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = (double)((int32_t)samples - count[i]) / (double)samples;
}

// camera_rays_kernel for a window of the frame: lane j writes ray first + j of the camera's row-major batch at
// out + 6 * j, with the same camera_ray on the same DevCamera, so a pass's rays are rr_camera_rays_device's bit for bit.
__global__ void __launch_bounds__(256) camera_rays_window_kernel(DevCamera C, int32_t affine, uint32_t hsize, int64_t first,
                                                                 int64_t n, double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * RR_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t t = (uint32_t)(first + j);
    const uint32_t py = t / hsize, px = t - py * hsize;
    const Ray r = camera_ray(C, affine != 0, px, py);
    double* o = out + 6 * j;
    o[0] = r.o.x;
    o[1] = r.o.y;
    o[2] = r.o.z;
    o[3] = r.d.x;
    o[4] = r.d.y;
    o[5] = r.d.z;
}

hipError_t launch_camera_rays_window(const DevCamera& cam, bool affine, int64_t first, int64_t n, double* out,
                                     hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!out || cam.hsize < 1 || cam.vsize < 1 || first < 0 || first + n > cam.hsize * cam.vsize ||
        cam.hsize * cam.vsize >= ((int64_t)1 << 32))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(camera_rays_window_kernel, dim3(blocks_for(n)), dim3(RR_BLOCK), 0, st, cam, affine ? 1 : 0,
                       (uint32_t)cam.hsize, first, n, out);
    return hipGetLastError();
}

template <int G, bool LC>
static void launch_ao_pairs_t(const DevScene& S, const DevAo& P, const AoPoints& I, int64_t n_pairs, int32_t* count,
                              unsigned long long* counters, hipStream_t st) {
    hipLaunchKernelGGL((ao_pairs_kernel<G, LC>), dim3(blocks_for(n_pairs)), dim3(256), cull_lds(S), st, S, P, I, n_pairs,
                       count, counters);
}

hipError_t launch_ao_pairs(const DevScene& S, const DevAo& P, const AoPoints& I, int64_t n, int32_t* count,
                           unsigned long long* counters, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!I.points || !I.normals || !count || !counters || P.samples < 1 || P.samples > 1024 || I.first < 0 ||
        n * (int64_t)P.samples >= ((int64_t)1 << 32))
        return hipErrorInvalidValue;
    if (64u % P.samples != 0u) {
        const hipError_t e = hipMemsetAsync(count, 0, (size_t)n * sizeof(int32_t), st);
        if (e != hipSuccess) return e;
    }
    dispatch_glc(S, [&](auto g, auto lc) {
        launch_ao_pairs_t<g(), lc()>(S, P, I, n * (int64_t)P.samples, count, counters, st);
    });
    return hipGetLastError();
}

hipError_t launch_ao_resolve(const int32_t* count, int32_t samples, int64_t n, double* out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!count || !out || samples < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ao_resolve_kernel, dim3(blocks_for(n)), dim3(RR_BLOCK), 0, st, count, (uint32_t)samples, n, out);
    return hipGetLastError();
}
