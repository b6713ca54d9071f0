// keyset_policy.h -- when a device-resident key set (keyset.h) is rehashed and into what capacity.  Host-only
// plain C++17, no HIP include (tests/test_txpool_host.py pins every rule without a GPU), in the manner of
// key_cache.h; the device side that will call these methods is not built yet.
//
// The insert kernel never reuses a tombstone and its probe loop is bounded by the capacity, so the table must
// never fill: the host keeps `bound`, an upper bound of the occupied slots (live keys plus tombstones).  It grows
// by n for every insert batch of n keys (whether or not they were new) and never shrinks on erase (an erased
// key leaves a tombstone).  Before a batch of `incoming` keys:
//   bound + incoming <= capacity / 2   nothing happens: no read of the device, no synchronisation;
//   otherwise                          the caller reads the true live count (the one synchronisation this policy
//                                      costs) and rehashes into capacity_for(live, incoming), the smallest power
//                                      of two >= 4 (live + incoming) and >= 8; the bound becomes the live count.
// After the batch the bound is therefore at most capacity / 2: a probe always meets an EMPTY slot.
#pragma once
#include <cstdint>

namespace bcosgpu {

constexpr uint64_t kKeySetMinCapacity = 8;

// the smallest power of two >= want and >= 8
inline uint64_t keyset_round_capacity(uint64_t want) {
    uint64_t c = kKeySetMinCapacity;
    while (c < want) c <<= 1;
    return c;
}

struct KeySetPolicy {
    uint64_t capacity = kKeySetMinCapacity;
    uint64_t bound = 0;     // >= live keys + tombstones
    uint64_t rehashes = 0;

    explicit KeySetPolicy(uint64_t initial_capacity = 0) : capacity(keyset_round_capacity(initial_capacity)) {}

    // must the live count be read (and the set rehashed) before a batch of `incoming` keys?
    bool must_rehash(uint64_t incoming) const { return bound + incoming > capacity / 2; }
    static uint64_t capacity_for(uint64_t live, uint64_t incoming) { return keyset_round_capacity(4 * (live + incoming)); }
    // the set was rehashed into `new_capacity` and holds `live` keys, no tombstones
    void rehashed(uint64_t new_capacity, uint64_t live) {
        capacity = new_capacity;
        bound = live;
        ++rehashes;
    }
    // an insert batch of n keys was enqueued
    void inserted(uint64_t n) { bound += n; }
    // an erase batch: tombstones keep their slots
    void erased(uint64_t) {}
};

}  // namespace bcosgpu
