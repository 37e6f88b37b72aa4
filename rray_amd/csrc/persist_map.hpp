// persist_map.hpp — the tile queue of the persistent level-0 loop (render_persist.inc), host and device.
// A frame's n_tiles tiles are dealt over H sharded heads (H a power of two): ticket k of head h is tile k * H + h, so
// the tiles being rendered at any moment stay a compact region of the image, as in launch order.  A head is a counter
// that starts at zero; a wave takes a ticket with one atomic add and renders the ticket's tile, and a ticket at or past
// the head's count is refused.  Every tile belongs to exactly one (head, ticket) pair below its head's count.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RR_PERSIST_HD __host__ __device__
#else
#define RR_PERSIST_HD
#endif

namespace rr {

constexpr uint32_t RR_PERSIST_MAX_HEADS = 256;  // one per counter slot (rr_device.hpp RR_CNT_SLOTS, C_WORK)

// tickets of head h that hold a tile
RR_PERSIST_HD inline uint32_t persist_head_count(uint32_t n_tiles, uint32_t H, uint32_t h) {
    return h < n_tiles ? (n_tiles - h + H - 1u) / H : 0u;
}

// the tile of ticket k of head h, or false when the head holds no such ticket (k may be any value an
// over-subscribed head reaches: the product is taken in 64 bits)
RR_PERSIST_HD inline bool persist_ticket_tile(uint32_t n_tiles, uint32_t H, uint32_t h, uint64_t k, uint32_t* tile) {
    const uint64_t t = k * (uint64_t)H + h;
    if (t >= (uint64_t)n_tiles) return false;
    *tile = (uint32_t)t;
    return true;
}

}  // namespace rr
