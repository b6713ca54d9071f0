// mismatch_record.h -- what the concurrent tests (concurrent_test.cpp, coalesce_mix_test.cpp) write down about
// a wrong result, so that a mismatch that cannot be made to order explains itself the one time it happens:
// who called, what was expected, what came back, and one class for the bytes that came back --
//   other_item   the bytes are the expected value of another item of the data file (with that item's index):
//                staging, scatter or the queue handed a caller somebody else's result
//   zeros        all zero where a value was expected
//   untouched    still the guard byte the caller filled its buffer with: nothing was written
//   verdict_only the bytes are right (or there are none to look at), only the verdict differs
//   garbage      none of these
#pragma once
#include <stdint.h>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace mismatch {

constexpr uint8_t kGuard = 0xA5;
constexpr size_t kMaxRecords = 32;

// the expected values of one output field over the data file: `count` entries of `width` bytes
struct Table {
    const uint8_t* values;
    size_t width, count;
};

inline bool all_bytes(const uint8_t* p, size_t n, uint8_t v) {
    for (size_t i = 0; i < n; ++i)
        if (p[i] != v) return false;
    return n > 0;
}

// got / want: `width` bytes of the field (got may be null: the interface returned no bytes)
inline std::string classify(const uint8_t* got, const uint8_t* want, size_t width, const std::vector<Table>& tables,
                            long* other) {
    *other = -1;
    if (!got || (want && std::memcmp(got, want, width) == 0)) return "verdict_only";
    if (all_bytes(got, width, kGuard)) return "untouched";
    if (all_bytes(got, width, 0)) return "zeros";
    for (const Table& t : tables) {
        if (t.width != width) continue;
        for (size_t i = 0; i < t.count; ++i)
            if (std::memcmp(t.values + width * i, got, width) == 0 && !all_bytes(got, width, 0)) {
                *other = static_cast<long>(i);
                return "other_item";
            }
    }
    return "garbage";
}

struct Log {
    std::mutex mu;
    std::vector<std::string> records;
    std::vector<Table> tables;

    // op: the entry point; field: which output; item: index in the data file
    void add(int thread, long call, const char* op, const char* field, long item, int want_ok, int got_ok,
             const uint8_t* got, const uint8_t* want, size_t width) {
        std::lock_guard<std::mutex> g(mu);
        if (records.size() >= kMaxRecords) return;
        long other = -1;
        const std::string cls = classify(got, want, width, tables, &other);
        std::string hex;
        for (size_t i = 0; got && i < width; ++i) {
            char b[3];
            snprintf(b, sizeof b, "%02x", got[i]);
            hex += b;
        }
        char buf[256];
        snprintf(buf, sizeof buf,
                 "{\"thread\": %d, \"call\": %ld, \"op\": \"%s\", \"field\": \"%s\", \"item\": %ld, \"want_ok\": %d, "
                 "\"got_ok\": %d, \"class\": \"%s\", \"other_item\": %ld, \"got\": \"",
                 thread, call, op, field, item, want_ok, got_ok, cls.c_str(), other);
        records.push_back(std::string(buf) + hex + "\"}");
    }
    std::string json() {
        std::lock_guard<std::mutex> g(mu);
        std::string s = "[";
        for (size_t i = 0; i < records.size(); ++i) s += (i ? ", " : "") + records[i];
        return s + "]";
    }
};

inline std::string stats_json(const uint64_t st[10]) {
    std::string s = "[";
    for (int i = 0; i < 10; ++i) s += (i ? ", " : "") + std::to_string(st[i]);
    return s + "]";
}

}  // namespace mismatch
