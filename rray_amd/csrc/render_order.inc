// render_order.inc — the coherent order of a device-resident ray batch (rr_ray_order_device, DESIGN.md §3.19), included
// by render_rays.hip inside namespace rr.  perm = argsort(key, stable), key the 32-bit code that
// rray_amd.ray_order_keys defines (the numpy mirror; the kernels equal it bit for bit):
//   order_bounds_kernel   per-block min / max of ox, oy, oz, u, v over the batch's valid rays
//   order_bounds_finish   the partials' min / max: the batch's bounds (min and max are exact, so any order serves)
//   order_key_kernel      one lane per ray: 48 bytes in, the key and the ray's own index out
//   four stable 8-bit LSD radix passes over the (key, index) pairs, each
//     order_hist_kernel     per-block digit histogram in LDS -> hist[digit][block]
//     order_scan_kernel     exclusive scan over the digit-major histograms, in place (one block)
//     order_scatter_kernel  stable scatter: ranks within a wave from __ballot digit matching, a block's waves and a
//                           wave's 64-key groups taken in index order
// Everything is f64 and integer arithmetic in the mirror's order of operations (-ffp-contract=off is global); nothing
// reads the scene, nothing visits the host.
constexpr int RR_ORDER_BLOCKS_MAX = 1024;  // sort blocks (the scan's columns); a block's tile grows with n instead
constexpr int RR_ORDER_BOUND_BLOCKS = 1024;
constexpr int RR_ORDER_OBITS = 6, RR_ORDER_DBITS = 7;

struct OrderCoords {
    double c[5];  // ox, oy, oz, u, v
    bool valid;
};
// The octahedral direction (u, v) of an unnormalised direction, and whether the ray takes part: its six components,
// u and v all finite (a zero direction gives 0 / 0).
__device__ __forceinline__ OrderCoords order_coords(const double* __restrict__ p) {
    OrderCoords r;
    const double ox = p[0], oy = p[1], oz = p[2], dx = p[3], dy = p[4], dz = p[5];
    const double s = (fabs(dx) + fabs(dy)) + fabs(dz);
    const double px = dx / s, py = dy / s;
    double u = px, v = py;
    if (dz < 0.0) {
        u = (1.0 - fabs(py)) * copysign(1.0, px);
        v = (1.0 - fabs(px)) * copysign(1.0, py);
    }
    r.c[0] = ox;
    r.c[1] = oy;
    r.c[2] = oz;
    r.c[3] = u;
    r.c[4] = v;
    r.valid = isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(dx) && isfinite(dy) && isfinite(dz) &&
              isfinite(u) && isfinite(v);
    return r;
}

// min over the block of lo[k], max of hi[k] -> out[k], out[5 + k] (thread 0).  Every thread of the block calls it.
__device__ __forceinline__ void order_block_minmax(double (&lo)[5], double (&hi)[5], double* __restrict__ out) {
    __shared__ double s_lo[4][5], s_hi[4][5];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        for (int off = 32; off > 0; off >>= 1) {
            const double a = __shfl_xor(lo[k], off), b = __shfl_xor(hi[k], off);
            lo[k] = a < lo[k] ? a : lo[k];
            hi[k] = b > hi[k] ? b : hi[k];
        }
        if (lane == 0) {
            s_lo[w][k] = lo[k];
            s_hi[w][k] = hi[k];
        }
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int k = threadIdx.x;
        double a = s_lo[0][k], b = s_hi[0][k];
        for (int q = 1; q < 4; ++q) {
            a = s_lo[q][k] < a ? s_lo[q][k] : a;
            b = s_hi[q][k] > b ? s_hi[q][k] : b;
        }
        out[k] = a;
        out[5 + k] = b;
    }
}

__global__ void __launch_bounds__(256) order_bounds_kernel(const double* __restrict__ rays, int64_t n,
                                                           double* __restrict__ partial) {
    double lo[5], hi[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        lo[k] = (double)__builtin_inf();
        hi[k] = -(double)__builtin_inf();
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const OrderCoords q = order_coords(rays + 6 * i);
        if (q.valid) {
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                lo[k] = q.c[k] < lo[k] ? q.c[k] : lo[k];
                hi[k] = q.c[k] > hi[k] ? q.c[k] : hi[k];
            }
        }
    }
    order_block_minmax(lo, hi, partial + 10 * (int64_t)blockIdx.x);
}

__global__ void __launch_bounds__(256) order_bounds_finish(const double* __restrict__ partial, int blocks,
                                                           double* __restrict__ bounds) {
    double lo[5], hi[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        lo[k] = (double)__builtin_inf();
        hi[k] = -(double)__builtin_inf();
    }
    for (int b = threadIdx.x; b < blocks; b += 256) {
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const double a = partial[10 * b + k], c = partial[10 * b + 5 + k];
            lo[k] = a < lo[k] ? a : lo[k];
            hi[k] = c > hi[k] ? c : hi[k];
        }
    }
    order_block_minmax(lo, hi, bounds);
}

// q = clamp(floor((c - lo) / (hi - lo) * 2^b), 0, 2^b - 1); a non-finite quotient (hi == lo, an overflowed extent) gives 0
__device__ __forceinline__ uint32_t order_quant(double c, double lo, double hi, int bits) {
    const double t = (c - lo) / (hi - lo);
    if (!isfinite(t)) return 0u;
    const double top = (double)((1 << bits) - 1);
    double f = floor(t * (double)(1 << bits));
    f = f < 0.0 ? 0.0 : f > top ? top : f;
    return (uint32_t)f;
}
// bit k of x -> bit 3k (six bits) / bit 2k (seven bits)
__device__ __forceinline__ uint32_t order_spread3(uint32_t x) {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < RR_ORDER_OBITS; ++k) r |= ((x >> k) & 1u) << (3 * k);
    return r;
}
__device__ __forceinline__ uint32_t order_spread2(uint32_t x) {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < RR_ORDER_DBITS; ++k) r |= ((x >> k) & 1u) << (2 * k);
    return r;
}

__global__ void __launch_bounds__(256) order_key_kernel(const double* __restrict__ rays, int64_t n,
                                                        const double* __restrict__ bounds, uint32_t* __restrict__ keys,
                                                        uint32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const OrderCoords q = order_coords(rays + 6 * i);
    uint32_t key = 0xFFFFFFFFu;
    if (q.valid) {
        const uint32_t qx = order_quant(q.c[0], bounds[0], bounds[5], RR_ORDER_OBITS);
        const uint32_t qy = order_quant(q.c[1], bounds[1], bounds[6], RR_ORDER_OBITS);
        const uint32_t qz = order_quant(q.c[2], bounds[2], bounds[7], RR_ORDER_OBITS);
        const uint32_t qu = order_quant(q.c[3], bounds[3], bounds[8], RR_ORDER_DBITS);
        const uint32_t qv = order_quant(q.c[4], bounds[4], bounds[9], RR_ORDER_DBITS);
        const uint32_t m3 = order_spread3(qx) | (order_spread3(qy) << 1) | (order_spread3(qz) << 2);
        const uint32_t m2 = order_spread2(qu) | (order_spread2(qv) << 1);
        key = (m3 << (2 * RR_ORDER_DBITS)) | m2;
    }
    keys[i] = key;
    idx[i] = (uint32_t)i;
}

// The radix passes.  Block b owns the 256 * groups consecutive pairs from b * 256 * groups on; its wave w the
// 64 * groups consecutive pairs from there + w * 64 * groups on, in groups of 64 (one per lane).  So the pairs' input
// order is (block, wave, group, lane), and a pass keeps the pairs of equal digit in that order: stable.
__global__ void __launch_bounds__(256) order_hist_kernel(const uint32_t* __restrict__ keys, int64_t n, int groups,
                                                         int shift, uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_h[256];
    s_h[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * 256 * groups;
    for (int g = 0; g < groups; ++g) {  // any order inside the block: the counts are sums
        const int64_t i = first + (int64_t)g * 256 + threadIdx.x;
        if (i < n) atomicAdd(&s_h[(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = s_h[threadIdx.x];
}

// Exclusive scan of the m digit-major counts in place, by one block of 1024 lanes: lane t owns the run
// [t * run, (t + 1) * run); the runs' sums are scanned through the waves (shuffles) and LDS.
__global__ void __launch_bounds__(1024) order_scan_kernel(uint32_t* __restrict__ hist, int m) {
    __shared__ uint32_t s_w[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int run = (m + 1023) / 1024;
    const int a = t * run < m ? t * run : m, b = a + run < m ? a + run : m;
    uint32_t sum = 0u;
    for (int j = a; j < b; ++j) sum += hist[j];
    uint32_t inc = sum;  // inclusive scan inside the wave
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(inc, off);
        if (lane >= off) inc += v;
    }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t before = 0u;
    for (int k = 0; k < 16; ++k) before += k < w ? s_w[k] : 0u;
    uint32_t at = before + inc - sum;
    for (int j = a; j < b; ++j) {
        const uint32_t c = hist[j];
        hist[j] = at;
        at += c;
    }
}

// hist: the scanned counts, hist[digit][block] = where this block's first pair of that digit goes.  keys_out may be
// null (the last pass: only the indices are wanted).
__global__ void __launch_bounds__(256) order_scatter_kernel(const uint32_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ idx, int64_t n, int groups,
                                                            int shift, const uint32_t* __restrict__ hist,
                                                            uint32_t* __restrict__ keys_out,
                                                            uint32_t* __restrict__ idx_out) {
    __shared__ uint32_t s_off[4][256];  // per wave and digit: its count, then where its next pair goes
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 4; ++q) s_off[q][threadIdx.x] = 0u;
    __syncthreads();
    const int64_t first = ((int64_t)blockIdx.x * 4 + w) * 64 * groups;
    for (int g = 0; g < groups; ++g) {
        const int64_t i = first + (int64_t)g * 64 + lane;
        if (i < n) atomicAdd(&s_off[w][(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    {
        const int d = threadIdx.x;
        uint32_t at = hist[(int64_t)d * gridDim.x + blockIdx.x];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t c = s_off[q][d];
            s_off[q][d] = at;
            at += c;
        }
    }
    __syncthreads();
    volatile uint32_t* off = s_off[w];  // this wave's row: read and advanced by this wave only, group after group
    const uint64_t below = lane == 0 ? 0ull : ((~0ull) >> (64 - lane));
    for (int g = 0; g < groups; ++g) {
        const int64_t i = first + (int64_t)g * 64 + lane;
        const bool in = i < n;
        const uint32_t key = in ? keys[i] : 0u, id = in ? idx[i] : 0u;
        const uint32_t d = (key >> shift) & 255u;
        uint64_t m = __ballot(in);  // the lanes of this group with this lane's digit
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (d >> bit) & 1u;
            const uint64_t bm = __ballot(one);
            m &= one ? bm : ~bm;
        }
        const uint32_t rank = (uint32_t)__popcll(m & below);
        uint32_t pos = 0u;
        if (in) pos = off[d] + rank;
        __builtin_amdgcn_wave_barrier();
        if (in && rank == 0u) off[d] = pos + (uint32_t)__popcll(m);  // one lane per digit of the group
        __builtin_amdgcn_wave_barrier();
        if (in) {
            if (keys_out) keys_out[pos] = key;
            idx_out[pos] = id;
        }
    }
}

// tile geometry of the radix passes for n pairs: 64-key groups per wave, and the blocks
static inline int order_groups(int64_t n) {
    const int64_t per = (int64_t)256 * RR_ORDER_BLOCKS_MAX;
    const int64_t g = (n + per - 1) / per;
    return (int)(g < 4 ? 4 : g);
}
static inline int order_blocks(int64_t n) {
    const int64_t tile = (int64_t)256 * order_groups(n);
    return (int)((n + tile - 1) / tile);
}
static inline size_t order_align(size_t b) { return (b + 255) & ~(size_t)255; }

// scratch: keys A | keys B | indices A | indices B | histograms | bounds partials | bounds
size_t ray_order_scratch_bytes(int64_t n) {
    if (n <= 0) return 0;
    return 4 * order_align((size_t)n * sizeof(uint32_t)) + order_align((size_t)256 * order_blocks(n) * sizeof(uint32_t)) +
           order_align((size_t)RR_ORDER_BOUND_BLOCKS * 10 * sizeof(double)) + order_align(10 * sizeof(double));
}

hipError_t launch_ray_order(const double* rays, int64_t n, uint32_t* perm, void* scratch, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!rays || !perm || !scratch || n >= ((int64_t)1 << 32)) return hipErrorInvalidValue;
    char* p = static_cast<char*>(scratch);
    const size_t nb = order_align((size_t)n * sizeof(uint32_t));
    uint32_t* keys[2] = {reinterpret_cast<uint32_t*>(p), reinterpret_cast<uint32_t*>(p + nb)};
    uint32_t* idx[2] = {reinterpret_cast<uint32_t*>(p + 2 * nb), reinterpret_cast<uint32_t*>(p + 3 * nb)};
    const int groups = order_groups(n), blocks = order_blocks(n);
    uint32_t* hist = reinterpret_cast<uint32_t*>(p + 4 * nb);
    double* partial = reinterpret_cast<double*>(p + 4 * nb + order_align((size_t)256 * blocks * sizeof(uint32_t)));
    double* bounds = partial + RR_ORDER_BOUND_BLOCKS * 10;
    const int bblocks = (int)std::min<int64_t>((n + 255) / 256, RR_ORDER_BOUND_BLOCKS);
    hipLaunchKernelGGL(order_bounds_kernel, dim3(bblocks), dim3(256), 0, st, rays, n, partial);
    hipLaunchKernelGGL(order_bounds_finish, dim3(1), dim3(256), 0, st, partial, bblocks, bounds);
    hipLaunchKernelGGL(order_key_kernel, dim3(blocks_for(n)), dim3(256), 0, st, rays, n, bounds, keys[0], idx[0]);
    for (int pass = 0; pass < 4; ++pass) {
        const int in = pass & 1, out = in ^ 1, shift = 8 * pass;
        const bool last = pass == 3;
        hipLaunchKernelGGL(order_hist_kernel, dim3(blocks), dim3(256), 0, st, keys[in], n, groups, shift, hist);
        hipLaunchKernelGGL(order_scan_kernel, dim3(1), dim3(1024), 0, st, hist, 256 * blocks);
        hipLaunchKernelGGL(order_scatter_kernel, dim3(blocks), dim3(256), 0, st, keys[in], idx[in], n, groups, shift, hist,
                           last ? (uint32_t*)nullptr : keys[out], last ? perm : idx[out]);
    }
    return hipGetLastError();
}
