// persist_map_check.cpp — the persistent level-0 loop's ticket -> tile mapping (rray_amd/csrc/persist_map.hpp, the
// header the device code includes) on the host: for every (n_tiles, H) the tickets below each head's count enumerate
// every tile exactly once, and every ticket at or past the count is refused.  Prints one line per case:
//   n_tiles H tiles_hit doubles refused_below accepted_past count_sum
#include <cstdint>
#include <cstdio>
#include <vector>

#include "persist_map.hpp"

int main() {
    const uint32_t tiles[] = {1, 15, 64, 32400, 129600};
    const uint32_t heads[] = {1, 8, 32, 256};
    for (uint32_t n : tiles)
        for (uint32_t H : heads) {
            std::vector<uint32_t> hit(n, 0);
            uint64_t doubles = 0, refused_below = 0, accepted_past = 0, count_sum = 0;
            for (uint32_t h = 0; h < H; ++h) {
                const uint32_t cnt = rr::persist_head_count(n, H, h);
                count_sum += cnt;
                for (uint32_t k = 0; k < cnt; ++k) {
                    uint32_t t = 0;
                    if (!rr::persist_ticket_tile(n, H, h, k, &t) || t >= n)
                        ++refused_below;
                    else if (hit[t]++)
                        ++doubles;
                }
                // past the count: the next tickets, and values an over-subscribed head's counter could reach
                const uint64_t past[] = {cnt, (uint64_t)cnt + 1, (uint64_t)cnt + 4096, 0xffffffffull, 0x100000000ull / H,
                                         0x100000000ull};
                for (uint64_t k : past) {
                    uint32_t t = 0;
                    if (k >= cnt && rr::persist_ticket_tile(n, H, h, k, &t)) ++accepted_past;
                }
            }
            uint64_t tiles_hit = 0;
            for (uint32_t v : hit) tiles_hit += v != 0;
            std::printf("%u %u %llu %llu %llu %llu %llu\n", n, H, (unsigned long long)tiles_hit, (unsigned long long)doubles,
                        (unsigned long long)refused_below, (unsigned long long)accepted_past, (unsigned long long)count_sum);
        }
    return 0;
}
