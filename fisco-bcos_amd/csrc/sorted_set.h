// sorted_set.h -- a set of 32-byte keys in HBM as a strictly ascending array plus a device-side count, and the
// kernel bodies of its three operations (contains, union with a batch, difference with a batch).  Every body is
// a __host__ __device__ function of (thread index, arguments) with no intrinsics in it, in the manner of
// tars_decode.h: csrc/txpool_kernels.hip wraps each one in a __global__ kernel, tests/cpp/txpool_sets_test.cpp
// runs each one for every thread index of its grid, serially, under ASan / UBSan, with every buffer malloc'ed at
// exactly its stated capacity.
//
// Order: a key is a big-endian 256-bit number; "ascending" is ascending as that number, everywhere (the set
// arrays, the sorted batches, the dumps).  Each set is double-buffered: a mutation reads one buffer (and its
// count) and writes the other; the host flips which one is current after the call.
//
// The rules every kernel of the transaction pool obeys (this header and txpool_admit.h):
//
//  1. No lane waits for another lane, wave or workgroup: no spin, no flag, no hand-off inside a kernel.  What one
//     kernel writes the next one reads only across the kernel boundary, on the pool's one stream.
//  2. No atomic touches set storage.  The single atomic anywhere is the atomicOr on the pool's error word
//     (set_error below).
//  3. Every loop is bounded by a count that comes from the host; a binary search takes at most kMaxSearchSteps
//     = 64 steps (a range below 2^32 halves to nothing in 33).
//  4. Every kernel takes the capacity of each buffer it writes as an argument.  A count read from device memory
//     is clamped to the capacity of the buffer it counts before it is used (clamp_count).  A store whose index is
//     not below the capacity is skipped and sets the error word, which the host reports as an engine error after
//     the call's synchronisation.
//  5. Growth happens only between calls, on the host: it keeps an upper bound of every set's count (old bound
//     plus the batch size for a union, unchanged by a difference, refreshed from the true count whenever it has
//     synchronised anyway); a bound above the capacity allocates both buffers anew, at least doubled, and copies.
//
// A union is, on one stream: records (key, index) of the batch -> sort by (skip, key, index) (a library merge
// sort with RecLess; std::sort in the host test) -> union_flag_body marks the first record of every run of equal
// keys that the set does not hold -> exclusive scan of the marks -> compact_body writes the marked keys B' (sorted,
// distinct, disjoint from the set) and their count -> merge_body: A[i] goes to i + lower_bound(B', A[i]), B'[k]
// to k + lower_bound(A, B'[k]); every element computes its own destination, the destinations are a permutation
// of [0, |A| + |B'|) because A and B' share no key.  A difference: sort the batch E the same way (duplicates may
// stay: a lower bound over a non-decreasing array finds a key all the same) -> diff_keep_body: keep[i] = A[i] not
// in E -> exclusive scan -> diff_scatter_body.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SSET_HD __host__ __device__ inline
#else
#define SSET_HD inline
#endif

namespace bcosgpu {
namespace sset {

constexpr uint32_t kKeyBytes = 32;
constexpr uint32_t kMaxSearchSteps = 64;
// bits of the pool's error word
constexpr uint32_t kErrStore = 1;  // a store's index was not below its buffer's capacity (the store was skipped)
constexpr uint32_t kErrCount = 2;  // a device-side count was above its buffer's capacity or the host's bound
constexpr uint32_t kErrInput = 4;  // a field of a decoded transaction points outside the encoded bytes

// One element of a batch on its way through the sort: the key, its index in the caller's batch, and whether it
// takes part at all (skip != 0 sorts behind every record that does).
struct Rec {
    uint8_t key[kKeyBytes];
    uint32_t idx;
    uint32_t skip;
};
static_assert(sizeof(Rec) == 40 && offsetof(Rec, key) == 0, "Rec layout");

// rule 2's one exception
SSET_HD void set_error(uint32_t* err, uint32_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(err, bits);
#else
    *err |= bits;
#endif
}

SSET_HD uint64_t load_be64(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i) v = (v << 8) | p[i];
    return v;
}

// -1 / 0 / 1 as a < b, a == b, a > b for two big-endian 256-bit numbers
SSET_HD int key_cmp(const uint8_t* a, const uint8_t* b) {
    for (int w = 0; w < 4; ++w) {
        const uint64_t x = load_be64(a + 8 * w), y = load_be64(b + 8 * w);
        if (x != y) return x < y ? -1 : 1;
    }
    return 0;
}

SSET_HD void key_copy(uint8_t* dst, const uint8_t* src) {
    for (uint32_t i = 0; i < kKeyBytes; ++i) dst[i] = src[i];
}

// the sort's order: records that take part first, by key, then by index
struct RecLess {
    SSET_HD bool operator()(const Rec& a, const Rec& b) const {
        if ((a.skip != 0) != (b.skip != 0)) return a.skip == 0;
        const int c = key_cmp(a.key, b.key);
        return c != 0 ? c < 0 : a.idx < b.idx;
    }
};

// rule 4: a count from device memory, never above the capacity of what it counts
SSET_HD uint32_t clamp_count(const uint32_t* count, uint32_t cap, uint32_t* err) {
    uint32_t c = *count;
    if (c > cap) {
        set_error(err, kErrCount);
        c = cap;
    }
    return c;
}

// the first index in [0, n) of an ascending key array whose key is >= key (n when none)
SSET_HD uint32_t lower_bound_keys(const uint8_t* keys, uint32_t n, const uint8_t* key) {
    uint32_t lo = 0, hi = n;
    for (uint32_t s = 0; s < kMaxSearchSteps && lo < hi; ++s) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (key_cmp(keys + static_cast<size_t>(mid) * kKeyBytes, key) < 0) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

SSET_HD bool contains_key(const uint8_t* keys, uint32_t n, const uint8_t* key) {
    const uint32_t p = lower_bound_keys(keys, n, key);
    return p < n && key_cmp(keys + static_cast<size_t>(p) * kKeyBytes, key) == 0;
}

// the same over records sorted with RecLess: a skipped record counts as above every key
SSET_HD uint32_t lower_bound_recs(const Rec* recs, uint32_t n, const uint8_t* key) {
    uint32_t lo = 0, hi = n;
    for (uint32_t s = 0; s < kMaxSearchSteps && lo < hi; ++s) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (recs[mid].skip == 0 && key_cmp(recs[mid].key, key) < 0) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

SSET_HD bool recs_contain(const Rec* recs, uint32_t n, const uint8_t* key) {
    const uint32_t p = lower_bound_recs(recs, n, key);
    return p < n && recs[p].skip == 0 && key_cmp(recs[p].key, key) == 0;
}

// A set as a kernel reads it: the current buffer, its count, the buffer's capacity in keys.
struct SetView {
    const uint8_t* keys;
    const uint32_t* count;
    uint32_t cap;
};

// ---- contains: out[i] = keys_in[i] in the set, i < n
SSET_HD void contains_body(uint64_t i, uint32_t n, const uint8_t* keys_in, SetView a, uint8_t* out, uint32_t out_cap,
                           uint32_t* err) {
    if (i >= n) return;
    if (i >= out_cap) {
        set_error(err, kErrStore);
        return;
    }
    const uint32_t na = clamp_count(a.count, a.cap, err);
    out[i] = contains_key(a.keys, na, keys_in + i * kKeyBytes) ? 1 : 0;
}

// ---- the records of a batch of n keys, every one taking part
SSET_HD void records_body(uint64_t i, uint32_t n, const uint8_t* keys_in, Rec* recs, uint32_t recs_cap, uint32_t* err) {
    if (i >= n) return;
    if (i >= recs_cap) {
        set_error(err, kErrStore);
        return;
    }
    key_copy(recs[i].key, keys_in + i * kKeyBytes);
    recs[i].idx = static_cast<uint32_t>(i);
    recs[i].skip = 0;
}

// ---- union, step 1: flag[i] = record i (of m, sorted) is the first of its run of equal keys, takes part, and
// its key is not in the set
SSET_HD void union_flag_body(uint64_t i, uint32_t m, const Rec* recs, SetView a, uint32_t* flag, uint32_t flag_cap,
                             uint32_t* err) {
    if (i >= m) return;
    if (i >= flag_cap) {
        set_error(err, kErrStore);
        return;
    }
    const uint32_t na = clamp_count(a.count, a.cap, err);
    bool f = recs[i].skip == 0;
    if (f && i > 0) f = key_cmp(recs[i - 1].key, recs[i].key) != 0;  // (a record before one that takes part does too)
    if (f) f = !contains_key(a.keys, na, recs[i].key);
    flag[i] = f ? 1u : 0u;
}

// ---- union, step 2 (after the exclusive scan pos of flag): the flagged keys, in order, to out; thread m - 1
// writes their count
SSET_HD void compact_body(uint64_t i, uint32_t m, const Rec* recs, const uint32_t* flag, const uint32_t* pos,
                          uint8_t* out, uint32_t out_cap, uint32_t* out_count, uint32_t* err) {
    if (i >= m) return;
    const uint32_t p = pos[i], f = flag[i];
    if (f) {
        if (p < out_cap) key_copy(out + static_cast<size_t>(p) * kKeyBytes, recs[i].key);
        else set_error(err, kErrStore);
    }
    if (i == m - 1) {
        uint64_t c = static_cast<uint64_t>(p) + f;
        if (c > out_cap) {
            set_error(err, kErrStore);
            c = out_cap;
        }
        *out_count = static_cast<uint32_t>(c);
    }
}

// ---- union, step 3: the rank merge of the set A (threads [0, bound_a), bound_a the host's bound of its count)
// and the compacted batch B' (threads [bound_a, bound_a + m)) into dst; thread 0 writes dst's count
SSET_HD void merge_body(uint64_t t, uint32_t bound_a, uint32_t m, SetView a, SetView b, uint8_t* dst, uint32_t dst_cap,
                        uint32_t* dst_count, uint32_t* err) {
    if (t >= static_cast<uint64_t>(bound_a) + m) return;
    const uint32_t na = clamp_count(a.count, a.cap, err), nb = clamp_count(b.count, b.cap, err);
    if (t == 0) {
        uint64_t total = static_cast<uint64_t>(na) + nb;
        if (na > bound_a || nb > m) set_error(err, kErrCount);  // elements no thread of this grid moves
        if (total > dst_cap) total = dst_cap;                    // (the refused stores below set the error word)
        *dst_count = static_cast<uint32_t>(total);
    }
    const uint8_t* src;
    uint64_t d;
    if (t < bound_a) {
        if (t >= na) return;
        src = a.keys + t * kKeyBytes;
        d = t + lower_bound_keys(b.keys, nb, src);
    } else {
        const uint64_t k = t - bound_a;
        if (k >= nb) return;
        src = b.keys + k * kKeyBytes;
        d = k + lower_bound_keys(a.keys, na, src);
    }
    if (d < dst_cap) key_copy(dst + d * kKeyBytes, src);
    else set_error(err, kErrStore);
}

// ---- difference, step 1: keep[i] = A[i] exists and is not among the m sorted records of E; i < bound_a
SSET_HD void diff_keep_body(uint64_t i, uint32_t bound_a, SetView a, const Rec* recs, uint32_t m, uint32_t* keep,
                            uint32_t keep_cap, uint32_t* err) {
    if (i >= bound_a) return;
    if (i >= keep_cap) {
        set_error(err, kErrStore);
        return;
    }
    const uint32_t na = clamp_count(a.count, a.cap, err);
    keep[i] = i < na && !recs_contain(recs, m, a.keys + i * kKeyBytes) ? 1u : 0u;
}

// ---- difference, step 2 (after the exclusive scan pos of keep): the kept keys to dst; thread bound_a - 1
// writes dst's count
SSET_HD void diff_scatter_body(uint64_t i, uint32_t bound_a, SetView a, const uint32_t* keep, const uint32_t* pos,
                               uint8_t* dst, uint32_t dst_cap, uint32_t* dst_count, uint32_t* err) {
    if (i >= bound_a) return;
    const uint32_t p = pos[i], f = keep[i];
    if (f) {
        if (p < dst_cap && i < a.cap) key_copy(dst + static_cast<size_t>(p) * kKeyBytes, a.keys + i * kKeyBytes);
        else set_error(err, kErrStore);
    }
    if (i == bound_a - 1) {
        uint64_t c = static_cast<uint64_t>(p) + f;
        if (clamp_count(a.count, a.cap, err) > bound_a) set_error(err, kErrCount);  // keys no thread looked at
        if (c > dst_cap) {
            set_error(err, kErrStore);
            c = dst_cap;
        }
        *dst_count = static_cast<uint32_t>(c);
    }
}

}  // namespace sset
}  // namespace bcosgpu
