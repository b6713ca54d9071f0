// state_pack_check.cpp -- the state-entry packer (csrc/pack.cpp bcosgpu_pack_state_entries) on its edge
// views, as a host-only program to build with the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o state_pack_check
//       tools/state_pack_check.cpp csrc/pack.cpp -lpthread
// Buffers are sized exactly (no slack), so a byte written or read past an end is a report.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/bcos_gpu.h"

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                               \
        }                                                          \
    } while (0)

static bcosgpu_StateEntry view(const std::string& t, const std::string& k, const std::vector<uint8_t>& v, int status,
                               int flags) {
    bcosgpu_StateEntry e;
    std::memset(&e, 0, sizeof e);
    e.table = t.empty() ? nullptr : t.data();
    e.table_len = t.size();
    e.key = k.empty() ? nullptr : k.data();
    e.key_len = k.size();
    e.value = v.empty() ? nullptr : v.data();
    e.value_len = v.size();
    e.status = static_cast<int8_t>(status);
    e.flags = static_cast<uint8_t>(flags);
    return e;
}

static int pack(const std::vector<bcosgpu_StateEntry>& e, std::vector<uint8_t>& out, std::vector<uint64_t>& off,
                std::vector<uint8_t>& kind) {
    out.assign(bcosgpu_state_entries_size(e.data(), e.size()), 0xEE);
    off.assign(3 * e.size() + 1, ~0ull);
    kind.assign(e.size(), 0xEE);
    return bcosgpu_pack_state_entries(e.data(), e.size(), out.data(), out.size(), off.data(), kind.data());
}

int main() {
    const std::string t = "table!", k = "key!", none;
    const std::vector<uint8_t> v(12, 'v'), empty;
    std::vector<uint8_t> out, kind;
    std::vector<uint64_t> off;
    // empty table / key / value (null pointers with zero lengths), a DELETED entry with a stale value, clean ones
    std::vector<bcosgpu_StateEntry> e = {view(none, k, v, BCOSGPU_ENTRY_MODIFIED, 1), view(t, none, v, BCOSGPU_ENTRY_MODIFIED, 0),
                                         view(t, k, empty, BCOSGPU_ENTRY_MODIFIED, 1), view(t, k, v, BCOSGPU_ENTRY_DELETED, 1),
                                         view(t, k, v, BCOSGPU_ENTRY_NORMAL, 1), view(t, k, v, BCOSGPU_ENTRY_EMPTY, 0),
                                         view(none, none, empty, BCOSGPU_ENTRY_MODIFIED, 1)};
    CHECK(pack(e, out, off, kind) == BCOSGPU_OK);
    CHECK(out.size() == 4 + 12 + 6 + 12 + 10 + 10 + 10 + 10);
    CHECK(off[3 * 3 + 2] == off[3 * 3 + 3] && off.back() == out.size());
    CHECK(kind[3] == (BCOSGPU_ENTRY_DELETED | 1 << 4) && kind[5] == BCOSGPU_ENTRY_EMPTY);
    // a DELETED entry whose value pointer dangles: never dereferenced
    bcosgpu_StateEntry gone = view(t, k, empty, BCOSGPU_ENTRY_DELETED, 1);
    gone.value = reinterpret_cast<const uint8_t*>(16);
    gone.value_len = 1000;
    CHECK(pack({gone}, out, off, kind) == BCOSGPU_OK && out.size() == 10);
    // refusals: short cap, null with a length, status outside 0..3, an entry of 2^32 bytes
    CHECK(pack(e, out, off, kind) == BCOSGPU_OK);
    CHECK(bcosgpu_pack_state_entries(e.data(), e.size(), out.data(), out.size() - 1, off.data(), kind.data()) == BCOSGPU_E_ARG);
    bcosgpu_StateEntry bad = view(t, k, v, BCOSGPU_ENTRY_MODIFIED, 0);
    bad.value = nullptr;
    CHECK(pack({bad}, out, off, kind) == BCOSGPU_E_ARG);
    for (int s : {4, -1, 127, -128}) CHECK(pack({view(t, k, v, s, 0)}, out, off, kind) == BCOSGPU_E_ARG);
    bad = view(t, k, v, BCOSGPU_ENTRY_MODIFIED, 0);
    bad.value_len = (1ull << 32) - 10;  // table + key + value = 2^32
    off.assign(4, 0);
    kind.assign(1, 0);
    CHECK(bcosgpu_pack_state_entries(&bad, 1, out.data(), ~0ull, off.data(), kind.data()) == BCOSGPU_E_ARG);
    CHECK(bcosgpu_pack_state_entries(nullptr, 0, nullptr, 0, off.data(), nullptr) == BCOSGPU_OK && off[0] == 0);
    // the threaded path: 20000 entries over exact-size buffers
    std::vector<bcosgpu_StateEntry> many;
    for (int i = 0; i < 20000; ++i) many.push_back(e[i % e.size()]);
    CHECK(pack(many, out, off, kind) == BCOSGPU_OK && off.back() == out.size());
    for (size_t i = 0; i < many.size(); ++i) {
        const bcosgpu_StateEntry& x = many[i];
        const uint8_t* p = out.data() + off[3 * i];
        if (x.table_len && std::memcmp(p, x.table, x.table_len) != 0) ++fails;
        if (x.key_len && std::memcmp(p + x.table_len, x.key, x.key_len) != 0) ++fails;
    }
    if (fails) return 1;
    std::printf("state_pack_check: ok\n");
    return 0;
}
