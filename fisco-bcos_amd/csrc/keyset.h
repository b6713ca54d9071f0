// keyset.h -- the slot arithmetic of a set of 32-byte keys kept in an open-addressing table (power-of-two
// capacity >= 8, linear probing, one state word per slot, a separate key array): the slot hash, the probe walk
// and the slot states.  Plain C++17 without a HIP include, host-tested (tests/test_txpool_host.py); it is the
// groundwork of the device-resident sets transaction admission needs and no kernel uses it yet.
//
// The slot hash mixes the key's eight words with a 128-bit per-set seed: nonces are chosen by the sender, so the
// seed is meant to be random unless a caller fixes it for reproducible tests.
//
// Three rules the table's kernels will have to keep, which this arithmetic is shaped for:
//  1. No lane waits for another lane or wave: every probe loop runs at most `capacity` steps (probe_slot visits
//     every slot exactly once in steps 0 .. mask) and one that gets there sets kErrProbeBound.
//  2. Within one kernel only the result of an atomic read-modify-write on a state word is relied on: an insert
//     claims EMPTY -> BUSY, writes the key, and a later launch turns BUSY into FULL.
//  3. An insert never reuses a tombstone; a rehash reclaims them (keyset_policy.h says when).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KS_HD __host__ __device__ inline
#else
#define KS_HD inline
#endif

namespace bcosgpu {
namespace keyset {

enum : uint32_t { kEmpty = 0, kBusy = 1, kFull = 2, kTomb = 3 };
constexpr uint32_t kNone = 0xFFFFFFFFu;  // "no slot" / "no index"
constexpr uint32_t kErrProbeBound = 1;   // a probe loop ran `capacity` steps

struct Key {
    uint32_t w[8];
};

KS_HD uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

// the slot hash: the key's eight words folded under seed0, finished (the 64-bit finaliser of MurmurHash3) under seed1
KS_HD uint64_t hash_key(const Key& k, uint64_t seed0, uint64_t seed1) {
    uint64_t h = seed0;
    for (int i = 0; i < 4; ++i) {
        const uint64_t x = static_cast<uint64_t>(k.w[2 * i]) | (static_cast<uint64_t>(k.w[2 * i + 1]) << 32);
        h = rotl64((h ^ x) * 0x9E3779B97F4A7C15ull, 29);
    }
    h ^= seed1;
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 33;
    return h;
}

// linear probing: the slot of probe step `step` (0 .. mask); steps 0 .. mask visit every slot exactly once
KS_HD uint64_t probe_slot(uint64_t h, uint64_t step, uint64_t mask) { return (h + step) & mask; }

KS_HD bool key_eq(const Key& a, const Key& b) {
    uint32_t d = 0;
    for (int i = 0; i < 8; ++i) d |= a.w[i] ^ b.w[i];
    return d == 0;
}

}  // namespace keyset
}  // namespace bcosgpu
