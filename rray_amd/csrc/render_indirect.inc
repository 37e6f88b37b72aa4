// render_indirect.inc — the kernels of the one-bounce indirect queries and frames (DESIGN.md §3.23; rray.h
// RR_HAS_INDIRECT holds the definition):
//   indirect_count_kernel    how many of each block's 256 (point, k) pairs belong to a point that hit (the frames only)
//   indirect_scan_kernel     those counts -> exclusive offsets, the pass's live count and each trace chunk's share of it,
//                            all left on the device (the frames only)
//   indirect_rays_kernel     one lane per pair, pair j = i * K + k: gathered ray k of point i — origin P, direction
//                            ao_direction(ao_base(seed, i), k, N), the very functions ao_pairs_kernel calls — into the
//                            pass's ray scratch in camera_rays_kernel's layout; for the frames also the live list: the
//                            global indices of the pairs of points that hit, in pair order
//   indirect_resolve_kernel  a pass's colours, K per point, summed in increasing k and divided by (double)K; zeros where
//                            the object plane says miss
// Included by render_rays.hip inside namespace rr.  None of them reads the scene: the trace between rays and resolve is
// the colour families' A.rays0 path on the pass's scratch (the frames: the rr::listed kernels' ordered source over the
// live list, with the live count on the device, so that a miss costs no ray and nothing visits the host).

// This lane's rank among the set flags of its block and the block's total (render_adapt.hip's block_rank: the waves'
// ballots summed through LDS).  Every thread of the 256-thread block must call it.
__device__ __forceinline__ uint32_t indirect_block_rank(bool flag, uint32_t& total) {
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

// n_pairs = n * K < 2^32 (host-checked), so the point index is a 32-bit division.  A wave reads at most 64 / K + 2
// consecutive ints of the object plane.
__global__ void __launch_bounds__(256) indirect_count_kernel(const int32_t* __restrict__ object, uint32_t K,
                                                             int64_t n_pairs, uint32_t* __restrict__ block_count) {
    const int64_t j = (int64_t)blockIdx.x * RR_BLOCK + threadIdx.x;
    const bool live = j < n_pairs && object[(uint32_t)j / K] >= 0;
    uint32_t total;
    (void)indirect_block_rank(live, total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// block_count -> exclusive prefix, in place, by one block: 256 counts at a time (Hillis-Steele in LDS) behind a running
// total, as adapt_scan_kernel; a pass of 2^22 pairs has 16 384 counts, 64 rounds.  counts[0] = the pass's live pairs;
// counts[1 + b] = those of them in slots [b * chunk, (b + 1) * chunk) of the live list, the live count of trace chunk b.
__global__ void __launch_bounds__(256) indirect_scan_kernel(uint32_t* __restrict__ block_count, int64_t n_blocks,
                                                            uint32_t* __restrict__ counts, int64_t chunk,
                                                            int32_t n_chunks) {
    __shared__ uint32_t v[256];
    const int t = threadIdx.x;
    uint32_t carry = 0;
    for (int64_t b0 = 0; b0 < n_blocks; b0 += 256) {
        const uint32_t c = b0 + t < n_blocks ? block_count[b0 + t] : 0u;
        v[t] = c;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const uint32_t a = t >= off ? v[t - off] : 0u;
            __syncthreads();
            v[t] += a;
            __syncthreads();
        }
        if (b0 + t < n_blocks) block_count[b0 + t] = carry + v[t] - c;
        carry += v[255];
        __syncthreads();
    }
    if (t == 0) counts[0] = carry;
    for (int32_t b = t; b < n_chunks; b += 256) {
        const int64_t left = (int64_t)carry - (int64_t)b * chunk;
        counts[1 + b] = (uint32_t)(left < 0 ? 0 : left > chunk ? chunk : left);
    }
}

// One lane per pair.  A lane's six doubles are 48 consecutive bytes and a wave's rays 3 KiB of consecutive cache lines
// (as lens_rays_kernel); the K lanes of a point read the same six doubles of the point planes (one request's worth: the
// loads of a wave touch 64 / K + 1 points).  The pair of a miss (I.object[i] < 0) writes no ray and enters no list: its
// scratch slot is never read.  list (the frames): entry block_off[block] + rank = first_ray + j for the live pairs, so the
// list is in pair order whatever block runs first; first_ray = I.first * K, the global index of the pass's pair 0.  The
// slots behind the live ones (one per pair of a miss) are filled with first_ray, a ray inside the pass's scratch: the
// trace launches for the capacity and the lanes of its last live block read their slot before they learn that they
// hold no ray.  No lane leaves before the rank's barrier.
__global__ void __launch_bounds__(256) indirect_rays_kernel(DevIndirect P, AoPoints I, int64_t n_pairs,
                                                            double* __restrict__ rays,
                                                            const uint32_t* __restrict__ block_off,
                                                            const uint32_t* __restrict__ counts,
                                                            uint32_t* __restrict__ list, uint32_t first_ray) {
    const int64_t j = (int64_t)blockIdx.x * RR_BLOCK + threadIdx.x;
    const bool valid = j < n_pairs;
    const uint32_t K = P.samples;
    const uint32_t jj = valid ? (uint32_t)j : 0u;
    const uint32_t i = jj / K, k = jj - i * K;
    bool live = valid;
    if (valid && I.object) live = I.object[i] >= 0;
    if (live) {
        const double* pp = I.points + (int64_t)i * I.point_stride;
        const double* np = I.normals + (int64_t)i * I.point_stride;
        const double N[3] = {np[0], np[I.comp_stride], np[2 * I.comp_stride]};
        double w[3];
        ao_direction(ao_base(P.seed, (uint64_t)I.first + i), k, N, w);
        double* r = rays + 6 * j;
        r[0] = pp[0];
        r[1] = pp[I.comp_stride];
        r[2] = pp[2 * I.comp_stride];
        r[3] = w[0];
        r[4] = w[1];
        r[5] = w[2];
    }
    if (list) {  // kernel-uniform
        uint32_t total;
        const uint32_t rank = indirect_block_rank(live, total);
        const uint32_t before = block_off[blockIdx.x] + rank;  // live pairs before pair j
        if (live)
            list[before] = first_ray + jj;
        else if (valid)
            list[counts[0] + (jj - before)] = first_ray;
    }
}

// One lane per point of the pass, lens_resolve_kernel's walk: the point's K colours are 24 * K consecutive bytes, read in
// increasing k, so the sum is the definition's.  A miss (object[i] < 0) writes zeros and reads none of its K slots, which
// no kernel wrote.  Reads: for K = 1 a wave reads 1536 consecutive bytes (three strided loads over the same twelve
// lines); for K = 4 / 16 / 64 consecutive lanes are 96 / 384 / 1536 bytes apart, so a load instruction touches 64 lines
// at K >= 16 — but each lane walks its own run front to back and every line fetched is used whole by the one or two
// lanes whose runs meet in it, from L2 after its first touch: the step is bound by the bytes it reads once (DESIGN.md
// §3.20's measurement of the LDS-staged form of lens_resolve_kernel, not kept).
__global__ void __launch_bounds__(256) indirect_resolve_kernel(const double* __restrict__ colours,
                                                               const int32_t* __restrict__ object, uint32_t samples,
                                                               int64_t n, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * RR_BLOCK + threadIdx.x;
    if (i >= n) return;
    double* o = out + 3 * i;
    if (object && object[i] < 0) {
        o[0] = 0.0;
        o[1] = 0.0;
        o[2] = 0.0;
        return;
    }
    const double* c = colours + 3 * i * (int64_t)samples;
    double r = c[0], g = c[1], b = c[2];
    for (uint32_t s = 1; s < samples; ++s) {
        c += 3;
        r = r + c[0];
        g = g + c[1];
        b = b + c[2];
    }
    const double S = (double)samples;
    o[0] = r / S;
    o[1] = g / S;
    o[2] = b / S;
}

hipError_t launch_indirect_rays(const DevIndirect& P, const AoPoints& I, int64_t n, double* rays, uint32_t* list,
                                uint32_t* block_count, uint32_t* counts, int64_t chunk, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int64_t n_pairs = n * (int64_t)P.samples;
    if (!I.points || !I.normals || !rays || P.samples < 1 || P.samples > 1024 || I.first < 0 ||
        (I.first + n) * (int64_t)P.samples >= ((int64_t)1 << 32))
        return hipErrorInvalidValue;
    const int64_t n_blocks = (n_pairs + RR_BLOCK - 1) / RR_BLOCK;
    if (list) {
        if (!I.object || !block_count || !counts || chunk < 1 || (n_pairs + chunk - 1) / chunk > ((int64_t)1 << 20))
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(indirect_count_kernel, dim3((unsigned)n_blocks), dim3(RR_BLOCK), 0, st, I.object, P.samples,
                           n_pairs, block_count);
        hipLaunchKernelGGL(indirect_scan_kernel, dim3(1), dim3(256), 0, st, block_count, n_blocks, counts, chunk,
                           (int32_t)((n_pairs + chunk - 1) / chunk));
    }
    hipLaunchKernelGGL(indirect_rays_kernel, dim3((unsigned)n_blocks), dim3(RR_BLOCK), 0, st, P, I, n_pairs, rays,
                       block_count, counts, list, (uint32_t)(I.first * (int64_t)P.samples));
    return hipGetLastError();
}

hipError_t launch_indirect_resolve(const double* colours, const int32_t* object, int32_t samples, int64_t n, double* out,
                                   hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!colours || !out || samples < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(indirect_resolve_kernel, dim3(blocks_for(n)), dim3(RR_BLOCK), 0, st, colours, object,
                       (uint32_t)samples, n, out);
    return hipGetLastError();
}
