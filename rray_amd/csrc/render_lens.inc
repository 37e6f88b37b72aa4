// render_lens.inc — the two kernels of the lens frames (DESIGN.md §3.20; rray.h RR_HAS_LENS holds the definition):
//   lens_rays_kernel     sample s of pixel p as ray i = p * S + s: sub-pixel jitter and a thin lens from the counter
//                        hash of (lens.seed, i, path 0), through the frames' camera inverse, into a ray buffer in
//                        camera_rays_kernel's layout (rr_lens_rays_device; a pass of rr_render_lens_device)
//   lens_resolve_kernel  a pass's colours, S per pixel, summed in increasing s and divided by (double)S into the image
// Included by render_rays.hip inside namespace rr.  Neither reads the scene; the trace between them is the colour
// families' A.rays0 path on the pass's scratch.

// u(k) of ray i: jitter_value(base, 0, k >> 1, k & 1) = lowbias32(base ^ k) * 2^-32
__device__ __forceinline__ double lens_u(uint32_t base, uint32_t k) { return jitter_value(base, 0u, k >> 1, k & 1u); }

// X(x, y, z)[r] = ((M[4r] x + M[4r+1] y) + M[4r+2] z) + M[4r+3] * 1.0 (camera_ray's order; no contraction)
__device__ __forceinline__ V3 lens_xf(const double* M, double x, double y, double z) {
    return {M[0] * x + M[1] * y + M[2] * z + M[3] * 1.0, M[4] * x + M[5] * y + M[6] * z + M[7] * 1.0,
            M[8] * x + M[9] * y + M[10] * z + M[11] * 1.0};
}

// One lane per ray.  i < 2^32 (host-checked), so the pixel and sample indices are 32-bit divisions.  A lane's six
// doubles are 48 consecutive bytes and a wave's rays 3 KiB of consecutive cache lines, each written whole by the wave's
// stores (as camera_rays_kernel).  The rejection loop runs all eight rounds for every lane (sixteen 32-bit hashes: two
// integer multiplies each) and keeps the first pair inside the disc, so the waves do not diverge.
__global__ void __launch_bounds__(256) lens_rays_kernel(DevLens L, int64_t first_ray, int64_t n,
                                                        double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * RR_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = (uint32_t)(first_ray + j);
    const uint32_t p = i / L.samples;
    const uint32_t py = p / L.width, px = p - py * L.width;
    const uint32_t base = jitter_base(L.seed, (uint64_t)i, 0u);
    double jx = 0.5, jy = 0.5;
    if (L.pixel_jitter) {
        jx = lens_u(base, 0u);
        jy = lens_u(base, 1u);
    }
    const double wx = L.half_width - ((double)px + jx) * L.pixel_size;
    const double wy = L.half_height - ((double)py + jy) * L.pixel_size;
    V3 o, f;
    if (L.aperture == 0.0) {
        o = lens_xf(L.inv, 0.0, 0.0, 0.0);
        f = lens_xf(L.inv, wx, wy, -1.0);
    } else {
        double A = 0.0, B = 0.0;
        bool found = false;
#pragma unroll
        for (uint32_t a = 0; a < 8u; ++a) {
            const double ca = 2.0 * lens_u(base, 2u + 2u * a) - 1.0;
            const double cb = 2.0 * lens_u(base, 3u + 2u * a) - 1.0;
            const bool in = ca * ca + cb * cb <= 1.0;
            if (!found && in) {
                A = ca;
                B = cb;
            }
            found = found || in;
        }
        const double fd = L.focal_distance;
        o = lens_xf(L.inv, L.aperture * A, L.aperture * B, 0.0);
        f = lens_xf(L.inv, wx * fd, wy * fd, -fd);
    }
    const double dx = f.x - o.x, dy = f.y - o.y, dz = f.z - o.z;
    const double mag = sqrt(dx * dx + dy * dy + dz * dz);
    double* r = out + 6 * j;
    r[0] = o.x;
    r[1] = o.y;
    r[2] = o.z;
    r[3] = dx / mag;
    r[4] = dy / mag;
    r[5] = dz / mag;
}

// One lane per pixel of the pass: its S colours are 24 * S consecutive bytes, read in increasing s, so the sum is the
// definition's.  Consecutive lanes read 24 * S bytes apart: a wave's loads are not coalesced, but each lane walks its own
// run of cache lines front to back and every line fetched is used whole (by one lane, or by the two whose runs meet in
// it), from L2 after its first touch.  A form that stages 64 pixels' colours through LDS with coalesced loads (as
// hit_records_kernel does) was measured and not kept: the frame took 1.271 against 1.274 ms on C2 with S = 8 and 1.093
// against 1.051 ms on C5 with S = 4 (DESIGN.md §3.20) — the step is bound by the bytes it reads once, not by their order.
__global__ void __launch_bounds__(256) lens_resolve_kernel(const double* __restrict__ colours, uint32_t samples,
                                                           int64_t n_pixels, double* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * RR_BLOCK + threadIdx.x;
    if (p >= n_pixels) return;
    const double* c = colours + 3 * p * (int64_t)samples;
    double r = c[0], g = c[1], b = c[2];
    for (uint32_t s = 1; s < samples; ++s) {
        c += 3;
        r = r + c[0];
        g = g + c[1];
        b = b + c[2];
    }
    const double S = (double)samples;
    double* o = out + 3 * p;
    o[0] = r / S;
    o[1] = g / S;
    o[2] = b / S;
}

hipError_t launch_lens_rays(const DevLens& L, int64_t first_ray, int64_t n, double* out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!out || L.samples < 1 || L.width < 1 || first_ray < 0 || first_ray + n > ((int64_t)1 << 32))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(lens_rays_kernel, dim3(blocks_for(n)), dim3(RR_BLOCK), 0, st, L, first_ray, n, out);
    return hipGetLastError();
}

hipError_t launch_lens_resolve(const double* colours, int32_t samples, int64_t n_pixels, double* out, hipStream_t st) {
    if (n_pixels <= 0) return hipSuccess;
    if (!colours || !out || samples < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lens_resolve_kernel, dim3(blocks_for(n_pixels)), dim3(RR_BLOCK), 0, st, colours, (uint32_t)samples,
                       n_pixels, out);
    return hipGetLastError();
}
