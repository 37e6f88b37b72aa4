// render_persist.inc — the persistent level-0 loop: a fused camera frame of a flat scene as one resident launch.
// The grid covers the GPU's resident capacity, whatever the frame's size; every wave loops: it takes a tile from the
// sharded queue (persist_map.hpp, render_common.inc queue_*), renders it exactly as a wave of shade_kernel does
// (shade_tile) and stores its pixels.  What shade_kernel pays per tile is paid once per wave here: the kernel-argument
// prologue, the clearing of the next frame's counters, the counter flush, and the workgroup's launch and teardown.
// There is no workgroup barrier: a block's four waves run independently.  A wave's home head is its global wave index
// mod H, and it leaves when that head is exhausted; the launch uses no more heads than it has waves, so any grid size
// renders the whole frame (nothing depends on co-residency).  Waves do not steal from other heads: a wave that
// scanned the heads for a non-empty one before leaving made the frame 10 % slower than the per-tile launch (every
// wave's loads of the same H words serialise memory-side, DESIGN.md §4), and with 32 waves per head the heads run dry
// within a tile's time of each other.  Included inside namespace rr,
// after render_levels.inc, by render_persist_g<G>_<lds|gl>.hip.
//
// Instantiated for the kernels without a workgroup barrier in shade_tile: no area light (AR: the area walks
// synchronise the block).
struct PersistArgs {
    const DevScene* S;
    const LevelArgs* A;
};
// the kernel's two arguments in its kernel-argument segment (DevScene first, LevelArgs at its alignment after it),
// through an address the compiler cannot see through
__device__ __forceinline__ PersistArgs persist_args() {
    typedef const __attribute__((address_space(4))) char* KernArg;
    KernArg ka = (KernArg)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    constexpr size_t a_off = (sizeof(DevScene) + alignof(LevelArgs) - 1) / alignof(LevelArgs) * alignof(LevelArgs);
    return {(const DevScene*)ka, (const LevelArgs*)(ka + a_off)};
}
// One tile of the loop: shade_kernel's body (shade_body.inc) for the 64 events of level-0 tile `tile`, counted into
// cnt and the closest-hit walk's trace_flops / trace_visits (all zero on entry)
template <int G, bool LC, bool FUSED, bool PRE, bool CP, bool RM, bool AR>
__device__ __forceinline__ void shade_tile(const DevScene& S, const LevelArgs& A, const int64_t tile, Counters& cnt,
                                           uint64_t& trace_flops, uint32_t& trace_visits) {
    const uint32_t iu = (uint32_t)tile * 64u + (uint32_t)lane_id();  // as the per-tile launch numbers the tile's events
    const int64_t i = iu;
    const bool valid = true;  // full tiles (A.tile_fast)
    constexpr bool ORD = FUSED && G == 1;
    const uint64_t clk0 = 0;
#include "shade_body.inc"
}

template <int G, bool LC, bool FUSED, bool PRE, bool CP, bool RM, bool AR>
__global__ void __launch_bounds__(256) RR_SHADE_ATTR(PRE, G, RM) persist_kernel(DevScene S_, LevelArgs A_) {
    static_assert(FUSED && !AR && !LC, "persist_kernel: the barrier-free fused kernels");
    // The arguments are read through the kernel-argument segment's address, made opaque once per iteration
    // (persist_args): loads of loop-invariant arguments then stay inside the iteration, where they are scalar loads
    // next to their uses, as in shade_kernel.  Hoisted out of the loop they are held in registers across the whole
    // tile body, which has none to spare (the kernel spilled 112 VGPRs and 223 SGPRs that way).
    const PersistArgs P0 = persist_args();
    const DevScene& S = *P0.S;
    const LevelArgs& A = *P0.A;
    (void)S_;
    (void)A_;
    load_prologue_args(A);
    if (A.counters_zero) {  // as zero_next_counters, over this launch's grid
        const uint32_t total = RR_CNT_SLOTS * RR_CNT_STRIDE, stride = gridDim.x * RR_BLOCK;
        for (uint32_t j = blockIdx.x * RR_BLOCK + threadIdx.x; j < total; j += stride) A.counters_zero[j] = 0ull;
    }
    const uint32_t w = (uint32_t)uniform((int)threadIdx.x) >> 6;
    const uint32_t home = (blockIdx.x * 4u + w) & (A.persist_heads - 1u);  // the wave's home head
    // the wave's totals: a tile's counts are 32-bit (Counters), so the totals are flushed every RR_PERSIST_FLUSH tiles
    // (a wave of a full-size grid renders about eight and flushes once, when it leaves)
    constexpr uint32_t RR_PERSIST_FLUSH = 64;
    Counters acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t acc_flops = 0;
    uint32_t acc_visits = 0, since = 0;
    // the home head's next ticket is requested a tile ahead and read after that tile's work, which hides the
    // atomic's round trip (one VGPR: lane 0 holds the ticket).  A wave leaves when its home head is exhausted: the
    // launch gives every head a wave (persist_plan_t), so every tile is rendered whatever the grid.
    uint32_t req = queue_request(A.persist_head, home);
    for (;;) {
        const PersistArgs P = persist_args();
        uint32_t tile = 0;
        if (!persist_ticket_tile(P.A->persist_tiles, P.A->persist_heads, home, queue_ticket(req), &tile)) break;
        req = queue_request(P.A->persist_head, home);
        Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        uint64_t trace_flops = 0;
        uint32_t trace_visits = 0;
        shade_tile<G, LC, FUSED, PRE, CP, RM, AR>(*P.S, *P.A, (int64_t)tile, cnt, trace_flops, trace_visits);
        acc.rays += cnt.rays;
        acc.shadow += cnt.shadow;
        acc.shade += cnt.shade;
        acc.n1n2 += cnt.n1n2;
        acc.gtests += cnt.gtests;
        acc.ghits += cnt.ghits;
        acc.tests += cnt.tests;
        acc.flops += cnt.flops;
        acc.visits += cnt.visits;
        acc.nan += cnt.nan;
        acc_flops += trace_flops;
        acc_visits += trace_visits;
        uniform_counters(acc);
        if (++since == RR_PERSIST_FLUSH) {
            flush<true>(acc, A.counters, W_SHADOW, acc_flops, acc_visits, (int)w);
            acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            acc_flops = 0;
            acc_visits = since = 0;
        }
    }
    flush<true>(acc, A.counters, W_SHADOW, acc_flops, acc_visits, (int)w);
}

// The launch's dynamic LDS: as launch_level_t's fused kernels (the prelit terms; the culls are global)
static size_t persist_lds(const DevScene& S) {
    return cull_lds(S) + (size_t)S.n_lights * prelit_per_light(false) * 256 * sizeof(double);
}

// Blocks the GPU holds at once: blocks per compute unit (the occupancy query with the launch's dynamic LDS, capped at
// the kernel's waves per SIMD — a 256-thread block is one wave on each SIMD — which the query can exceed by one) x
// compute units of the current device.  persist_plan_t asks once per context and scene (its caller keeps the answer).
template <int G, bool LC>
static int persist_resident_blocks(size_t lds) {
    int dev = 0, per_cu = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, persist_kernel<G, LC, true, true, false, false, false>, 256,
                                                     lds) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return 0;
    return std::max(std::min(per_cu, RR_PRE_WAVES), 0) * std::max(cus, 0);
}

// The launch of (S, A), decided once (kernels.hpp persist_plan).  RRAY_PERSIST_BLOCKS=n sets the grid (any n >= 1
// renders the whole frame); every head needs a wave of its own, so the launch uses no more heads than it has waves.
template <int G, bool LC>
PersistPlan persist_plan_t(const DevScene& S, const LevelArgs& A, int* resident) {
    const PersistPlan per_tile = {0, 0};
    if (A.persist_tiles == 0 || A.level != 0 || A.rays0 || A.pw || A.list || !A.tile_fast || A.next) return per_tile;
    if (S.has_area || S.complex_patterns || S.n_lights > RR_PRELIT_LIGHTS || !fused_levels(S)) return per_tile;
    const char* off = std::getenv("RRAY_NO_PERSIST");
    if (off && std::atoi(off) == 1) return per_tile;
    const char* forced = std::getenv("RRAY_PERSIST_BLOCKS");
    int blocks = forced ? std::max(0, std::atoi(forced)) : 0;
    if (blocks <= 0) {
        if (*resident < 0) *resident = persist_resident_blocks<G, LC>(persist_lds(S));
        // frames with fewer tiles than resident wave slots keep the per-tile launch
        if (*resident <= 0 || (int64_t)A.persist_tiles < 4 * (int64_t)*resident) return per_tile;
        blocks = *resident;
    }
    uint32_t heads = A.persist_heads;
    while ((int64_t)heads > 4 * (int64_t)blocks) heads >>= 1;
    return {blocks, heads};
}

template <int G, bool LC>
void launch_persist_t(const DevScene& S, const LevelArgs& A, const PersistPlan& plan, hipStream_t st, KernelProf* prof) {
    // persist_args finds the arguments by their places in the kernel-argument segment: exactly these two, by value, in
    // this order (a third argument would be harmless, another order or a pointer not); the units are built without
    // kernel-argument preloading, which would leave the first words of the segment unread but still in place
    static_assert(std::is_same<decltype(&persist_kernel<G, LC, true, true, false, false, false>),
                               void (*)(DevScene, LevelArgs)>::value,
                  "persist_args reads (DevScene, LevelArgs) from the kernel-argument segment");
    static_assert(std::is_trivially_copyable<DevScene>::value && std::is_trivially_copyable<LevelArgs>::value &&
                      alignof(DevScene) <= 16 && alignof(LevelArgs) <= 16,
                  "persist_args: plain structures at their natural offsets");
    LevelArgs B = A;
    B.persist_heads = plan.heads;
    B.uniform_hit = uniform_hit_on();
    Span s(prof, K_TRACE_SHADE, st);
    hipLaunchKernelGGL((persist_kernel<G, LC, true, true, false, false, false>), dim3((unsigned)plan.blocks), dim3(256),
                       persist_lds(S), st, S, B);
}
