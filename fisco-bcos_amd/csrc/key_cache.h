// key_cache.h -- the bookkeeping of the registered-key cache (ecc_keyed.hip): which key has which table, what a
// call builds, when a sighted key is promoted.  Host-only plain C++17, no HIP include: every rule below is a
// method on plain containers (tests/test_key_cache.py pins them without a GPU).  A slip in one of them changes
// no verdict -- it routes sealer signatures to the generic kernels, or hands out an id of an unbuilt table --
// so no parity test would notice.  ecc_keyed.hip owns the device side (arena, streams, the table kernel) and
// calls these methods under its mutex.
//
// Keys get a table in one of two ways, never evicted until clear():
//   registration (bcosgpu_register_keys: the consensus node list) builds synchronously: plan_registration says
//     which keys to build at which arena indices, registration_done publishes them, so the ids it returns name
//     built tables.  A key repeated in the call gets one index.  A full arena leaves the key uncached (-1).
//   promotion (the coalesced verify calls): lookup counts a sighting of each uncached key, once per call however
//     often the key occurs in it, and only for calls that name their keys (SM2 recover -- admission, the
//     sender's own key -- never counts).  A key seen in `promote_after` calls is handed to an asynchronous
//     build: at most kPromoteBuildsPerCall keys a build, one build in flight (while it is, lookups count
//     nothing), promoted keys in at most half the capacity (the rest stays for registrations).  The sightings
//     live in a bounded sketch, dropped whole once it holds more than kSeenMax keys.  build_started /
//     build_finished bracket the build; finished(ok) publishes its keys, finished(failed) drops them, and
//     either way their indices stay consumed.
// Slot ids carry 15 bits of the cache generation, which clear() bumps: an id from before a clear fails in the
// kernel instead of naming whichever key now has its index.
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace bcosgpu {

using Key64 = std::array<uint8_t, 64>;
struct Key64Hash {
    size_t operator()(const Key64& k) const {
        uint64_t h;
        std::memcpy(&h, k.data() + 24, 8);  // low bits of x: uniformly distributed for valid keys
        uint64_t g;
        std::memcpy(&g, k.data() + 56, 8);
        return static_cast<size_t>(h ^ (g * 0x9E3779B97F4A7C15ull));
    }
};
inline Key64 key_at(const uint8_t* pubs, size_t stride, size_t i) {
    Key64 k;
    std::memcpy(k.data(), pubs + stride * i, 64);
    return k;
}

// the 15-bit generation tag of public slot ids: id = (tag << 16) | index (capacity <= 65536 keys)
inline uint32_t gen_tag(uint64_t gen) { return static_cast<uint32_t>(gen & 0x7FFFu); }
inline int32_t slot_id(uint64_t gen, int32_t index) { return static_cast<int32_t>((gen_tag(gen) << 16) | uint32_t(index)); }

constexpr int kPromoteBuildsPerCall = 16;  // tables built by one promotion build at most
constexpr size_t kSeenMax = size_t{1} << 16;

// the tables one call builds: keys[q] at arena index idx[q]
struct KeyBuild {
    std::vector<Key64> keys;
    std::vector<int32_t> idx;
    std::vector<size_t> at;  // (registration) the call's positions that take a key of `keys`, repeats included
};

struct KeyCacheBook {
    using Map = std::unordered_map<Key64, int32_t, Key64Hash>;
    const int cap;            // tables the arena holds
    const int promote_after;  // calls that must see a key before it is promoted (0 = never)
    Map slot_of;              // published: table built
    Map pending;              // promoted, table being built
    std::unordered_map<Key64, uint32_t, Key64Hash> seen;
    int32_t next = 0;  // arena indices handed out this generation (published, pending, failed builds)
    int promoted = 0, registered = 0;
    uint64_t gen = 0;  // bumped by clear
    bool building = false;
    std::vector<Key64> build_keys;  // of the build in flight
    uint64_t hits = 0, misses = 0, builds = 0;

    KeyCacheBook(int capacity, int promote_after_calls) : cap(capacity), promote_after(promote_after_calls) {}
    int32_t id_of(const Key64& k) const {  // -1: no table
        const auto it = slot_of.find(k);
        return it != slot_of.end() ? slot_id(gen, it->second) : -1;
    }

    // Ids of the n keys at pubs + stride * i into out (-1: no table) and whether every key has one.  With
    // `promote` (the call names its keys and a build can start) it counts sightings, and `b` lists the build to
    // start now, if any: after launching it call build_started(b); if that fails, nothing (its indices stay
    // consumed).  An empty cache that cannot promote answers false at once and leaves out and the counters alone.
    bool lookup(const uint8_t* pubs, size_t stride, size_t n, int32_t* out, bool promote, KeyBuild& b) {
        b = KeyBuild{};
        promote = promote && promote_after > 0;
        if (slot_of.empty() && !promote) return false;
        std::unordered_set<Key64, Key64Hash> counted;
        bool every = true;
        for (size_t i = 0; i < n; ++i) {
            const Key64 k = key_at(pubs, stride, i);
            if ((out[i] = id_of(k)) >= 0) continue;
            every = false;
            if (!promote || building || pending.count(k) || !counted.insert(k).second) continue;
            if (promoted + static_cast<int>(b.keys.size()) >= cap / 2 ||
                static_cast<int>(b.keys.size()) >= kPromoteBuildsPerCall)
                continue;
            if (seen.size() > kSeenMax) seen.clear();
            if (++seen[k] < static_cast<uint32_t>(promote_after) || next >= cap) continue;  // or the arena is full
            b.keys.push_back(k);
            b.idx.push_back(next++);
        }
        (every ? hits : misses) += n;
        return every;
    }
    void build_started(const KeyBuild& b) {
        for (size_t q = 0; q < b.keys.size(); ++q) pending.emplace(b.keys[q], b.idx[q]);
        build_keys = b.keys;
        building = true;
    }
    void build_finished(bool ok) {
        building = false;
        for (const Key64& k : build_keys) {
            const auto it = pending.find(k);
            if (it == pending.end()) continue;
            if (ok) {
                slot_of.emplace(k, it->second);
                seen.erase(k);
                ++builds;
                ++promoted;
            }
            pending.erase(it);
        }
        build_keys.clear();
    }

    // A registration, with no build in flight: fills out for the keys that have a table and returns what to build
    // (`arena`: there is one to build into).  After a successful build, registration_done publishes it, fills the
    // positions b.at, counts the call and says whether every key has a table; with nothing to build it is called
    // at once; after a failed build it is not called (the indices stay consumed).
    KeyBuild plan_registration(const uint8_t* pubs, size_t stride, size_t n, int32_t* out, bool arena) {
        KeyBuild b;
        std::unordered_set<Key64, Key64Hash> first;
        for (size_t i = 0; i < n; ++i) {
            const Key64 k = key_at(pubs, stride, i);
            if ((out[i] = id_of(k)) >= 0) continue;
            if (first.count(k)) {  // a repeat within this call: it follows its first occurrence
                b.at.push_back(i);
                continue;
            }
            if (!arena || next >= cap) continue;  // the cache is full: not cached
            first.insert(k);
            b.keys.push_back(k);
            b.idx.push_back(next++);
            b.at.push_back(i);
        }
        return b;
    }
    bool registration_done(const KeyBuild& b, const uint8_t* pubs, size_t stride, size_t n, int32_t* out) {
        for (size_t q = 0; q < b.keys.size(); ++q) {
            slot_of.emplace(b.keys[q], b.idx[q]);
            seen.erase(b.keys[q]);
        }
        builds += b.keys.size();
        registered += static_cast<int>(b.keys.size());
        for (size_t i : b.at) out[i] = id_of(key_at(pubs, stride, i));
        bool every = true;
        for (size_t i = 0; i < n; ++i) every = every && out[i] >= 0;
        (every ? hits : misses) += n;
        return every;
    }

    // Forget every key (the device has drained): a build in flight is dropped unpublished, indices restart at 0
    // under a new generation.
    void clear() {
        slot_of.clear();
        pending.clear();
        seen.clear();
        build_keys.clear();
        building = false;
        next = 0;
        promoted = registered = 0;
        ++gen;
    }
    // keys cached, capacity, lookups with every key cached (by keys), the others, tables built
    void info(int64_t out[5]) const {
        out[0] = static_cast<int64_t>(slot_of.size());
        out[1] = cap;
        out[2] = static_cast<int64_t>(hits);
        out[3] = static_cast<int64_t>(misses);
        out[4] = static_cast<int64_t>(builds);
    }
};

}  // namespace bcosgpu
