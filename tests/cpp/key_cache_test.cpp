// Runs scripted scenarios on KeyCacheBook (csrc/key_cache.h, host-only) and prints one JSON line per argument
//   CAPACITY:PROMOTE_AFTER:STEP;STEP;...
// Keys are named by integers (K: a comma list of N or N..M, inclusive).  Steps:
//   L+K / L-K  lookup, promotion allowed / not           -> all, ids, build [[key, index], ...]
//   S          build_started(the last lookup's build)
//   F1 / F0    build_finished(ok / failed)
//   RK         plan_registration + registration_done     -> all, ids, build, at (positions filled when done)
//   RxK        plan_registration alone (the build failed) -> ids, build, at
//   RnK        a registration with no arena              -> as R
//   C          clear
//   I          -> info's five numbers and the book's other counts (seen: keys in the sketch, sightings: their sum)
//   Tgen,index -> slot_id(gen, index)
// ids are left out of calls of more than 32 keys; -7 marks an id the call did not write.
// tests/test_key_cache.py compiles this with g++ and pins the answers.
#include <cstdio>
#include <cstdlib>
#include <string>
#include "../../fisco-bcos_amd/csrc/key_cache.h"

using namespace bcosgpu;

static std::vector<uint64_t> parse_keys(const std::string& s) {
    std::vector<uint64_t> v;
    size_t p = 0;
    while (p < s.size()) {
        size_t e = s.find(',', p);
        if (e == std::string::npos) e = s.size();
        const std::string t = s.substr(p, e - p);
        const size_t dd = t.find("..");
        const uint64_t a = std::strtoull(t.c_str(), nullptr, 10);
        const uint64_t b = dd == std::string::npos ? a : std::strtoull(t.c_str() + dd + 2, nullptr, 10);
        for (uint64_t k = a; k <= b; ++k) v.push_back(k);
        p = e + 1;
    }
    return v;
}
static std::vector<uint8_t> key_bytes(const std::vector<uint64_t>& ks) {
    std::vector<uint8_t> b(64 * ks.size() + 1, 0);
    for (size_t i = 0; i < ks.size(); ++i)
        for (size_t at : {size_t{0}, size_t{24}, size_t{56}}) std::memcpy(b.data() + 64 * i + at, &ks[i], 8);
    return b;
}
static uint64_t key_name(const Key64& k) {
    uint64_t v;
    std::memcpy(&v, k.data(), 8);
    return v;
}
static void print_call(const char* op, int all, const std::vector<int32_t>& ids, const KeyBuild& b) {
    std::printf("{\"op\": \"%s\"", op);
    if (all >= 0) std::printf(", \"all\": %s", all ? "true" : "false");
    if (ids.size() <= 32) {
        std::printf(", \"ids\": [");
        for (size_t i = 0; i < ids.size(); ++i) std::printf("%s%d", i ? ", " : "", ids[i]);
        std::printf("]");
    }
    std::printf(", \"build\": [");
    for (size_t q = 0; q < b.keys.size(); ++q)
        std::printf("%s[%llu, %d]", q ? ", " : "", static_cast<unsigned long long>(key_name(b.keys[q])), b.idx[q]);
    std::printf("], \"at\": [");
    for (size_t q = 0; q < b.at.size(); ++q) std::printf("%s%zu", q ? ", " : "", b.at[q]);
    std::printf("]}");
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        int cap = 0, after = 0, used = 0;
        if (std::sscanf(argv[a], "%d:%d:%n", &cap, &after, &used) != 2) return 2;
        KeyCacheBook book(cap, after);
        KeyBuild last;
        std::string rest = argv[a] + used;
        std::printf("[");
        for (bool head = true; !rest.empty(); head = false) {
            const std::string step = rest.substr(0, rest.find(';'));
            rest.erase(0, step.size() + 1);
            if (step.empty()) return 2;
            if (!head) std::printf(", ");
            const char op = step[0];
            if (op == 'L') {
                const std::vector<uint64_t> ks = parse_keys(step.substr(2));
                const std::vector<uint8_t> pubs = key_bytes(ks);
                std::vector<int32_t> ids(ks.size(), -7);
                const bool all = book.lookup(pubs.data(), 64, ks.size(), ids.data(), step[1] == '+', last);
                print_call("lookup", all, ids, last);
            } else if (op == 'S') {
                book.build_started(last);
                std::printf("{\"op\": \"started\"}");
            } else if (op == 'F') {
                book.build_finished(step[1] == '1');
                std::printf("{\"op\": \"finished\"}");
            } else if (op == 'R') {
                const bool plan_only = step.size() > 1 && step[1] == 'x', no_arena = step.size() > 1 && step[1] == 'n';
                const std::vector<uint64_t> ks = parse_keys(step.substr(plan_only || no_arena ? 2 : 1));
                const std::vector<uint8_t> pubs = key_bytes(ks);
                std::vector<int32_t> ids(ks.size(), -7);
                const KeyBuild b = book.plan_registration(pubs.data(), 64, ks.size(), ids.data(), !no_arena);
                int all = -1;
                if (!plan_only) all = book.registration_done(b, pubs.data(), 64, ks.size(), ids.data());
                print_call(plan_only ? "plan" : "register", all, ids, b);
            } else if (op == 'C') {
                book.clear();
                std::printf("{\"op\": \"clear\"}");
            } else if (op == 'I') {
                int64_t o[5];
                book.info(o);
                unsigned long long sightings = 0;
                for (const auto& kv : book.seen) sightings += kv.second;
                std::printf("{\"op\": \"info\", \"keys\": %lld, \"cap\": %lld, \"hits\": %lld, \"misses\": %lld, \"builds\": %lld, "
                            "\"promoted\": %d, \"registered\": %d, \"next\": %d, \"gen\": %llu, \"pending\": %zu, \"seen\": %zu, "
                            "\"sightings\": %llu, \"building\": %s}",
                            static_cast<long long>(o[0]), static_cast<long long>(o[1]), static_cast<long long>(o[2]),
                            static_cast<long long>(o[3]), static_cast<long long>(o[4]), book.promoted, book.registered,
                            book.next, static_cast<unsigned long long>(book.gen), book.pending.size(), book.seen.size(),
                            sightings, book.building ? "true" : "false");
            } else if (op == 'T') {
                unsigned long long gen = 0;
                int index = 0;
                if (std::sscanf(step.c_str() + 1, "%llu,%d", &gen, &index) != 2) return 2;
                std::printf("{\"op\": \"slot_id\", \"id\": %d}", slot_id(gen, index));
            } else {
                return 2;
            }
        }
        std::printf("]\n");
    }
    return 0;
}
