// state_root_test.cpp -- StateStorage::hash / KeyPageStorage::hash (StateStorage.h:397-431,
// KeyPageStorage.cpp:351-406) through the C ABI and the C++ adapter (include/bcos_gpu.hpp calculateStateRoot):
// bcosgpu_StateEntry views over a fixture written by tests/test_state_root.py, whose expected packed layout
// and roots come from that file's restatement of Entry::hash (Entry.h:229-309).
// argv[1] = fixture.  The packer check runs everywhere; the root part exits 77 without a gfx950 device.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/bcos_gpu.hpp"

using namespace bcosgpu;

namespace {
struct Reader {
    std::vector<uint8_t> d;
    size_t at = 0;
    uint32_t u32() {
        uint32_t v;
        std::memcpy(&v, d.data() + at, 4);
        at += 4;
        return v;
    }
    std::pair<const uint8_t*, size_t> bytes() {
        const uint32_t n = u32();
        const uint8_t* p = d.data() + at;
        at += n;
        return {p, n};
    }
};
int fails = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);     \
            ++fails;                                                   \
        }                                                              \
    } while (0)
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    Reader r;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        std::fseek(f, 0, SEEK_END);
        r.d.resize(std::ftell(f));
        std::fseek(f, 0, SEEK_SET);
        if (std::fread(r.d.data(), 1, r.d.size(), f) != r.d.size()) return 2;
        std::fclose(f);
    }
    if (r.d.size() < 8 || std::memcmp(r.d.data(), "STRT", 4) != 0) return 2;
    r.at = 4;
    const size_t n = r.u32();
    // the views point into the fixture bytes; a DELETED or clean entry keeps its (stale) value pointer
    std::vector<bcosgpu_StateEntry> ent(n);
    for (size_t i = 0; i < n; ++i) {
        bcosgpu_StateEntry& e = ent[i];
        std::memset(&e, 0, sizeof e);
        auto t = r.bytes();
        e.table = reinterpret_cast<const char*>(t.first);
        e.table_len = t.second;
        auto k = r.bytes();
        e.key = reinterpret_cast<const char*>(k.first);
        e.key_len = k.second;
        auto v = r.bytes();
        e.value = v.first;
        e.value_len = v.second;
        e.status = static_cast<int8_t>(r.d[r.at]);
        e.flags = r.d[r.at + 1];
        r.at += 2;
    }
    // expected: packed data, off3[3n+1], kind[n], then per hasher (Keccak256, SM3) the 3.0 and the 3.1 root
    const auto want_data = r.bytes();
    std::vector<uint64_t> want_off(3 * n + 1);
    std::memcpy(want_off.data(), r.d.data() + r.at, 8 * want_off.size());
    r.at += 8 * want_off.size();
    const uint8_t* want_kind = r.d.data() + r.at;
    r.at += n;
    const uint8_t* want_root[2][2];
    for (int h = 0; h < 2; ++h)
        for (int v = 0; v < 2; ++v) {
            want_root[h][v] = r.d.data() + r.at;
            r.at += 32;
        }
    if (r.at != r.d.size()) {
        std::printf("fixture size mismatch\n");
        return 2;
    }

    // host packer against the restatement's layout
    const uint64_t total = bcosgpu_state_entries_size(ent.data(), n);
    CHECK(total == want_data.second);
    std::vector<uint8_t> packed(total + 1), kind(n + 1);
    std::vector<uint64_t> off(3 * n + 1);
    CHECK(bcosgpu_pack_state_entries(ent.data(), n, packed.data(), total, off.data(), kind.data()) == BCOSGPU_OK);
    CHECK(off == want_off);
    if (total == want_data.second && total) CHECK(std::memcmp(packed.data(), want_data.first, total) == 0);
    if (n) CHECK(std::memcmp(kind.data(), want_kind, n) == 0);
    if (total)
        CHECK(bcosgpu_pack_state_entries(ent.data(), n, packed.data(), total - 1, off.data(), kind.data()) == BCOSGPU_E_ARG);
    if (n) {
        uint64_t o2[4];
        uint8_t k2[1];
        bcosgpu_StateEntry bad = ent[0];
        bad.status = 4;  // outside Entry::Status
        CHECK(bcosgpu_pack_state_entries(&bad, 1, packed.data(), packed.size(), o2, k2) == BCOSGPU_E_ARG);
        bad = ent[0];
        bad.key = nullptr;  // a null pointer with a length
        bad.key_len = 2;
        CHECK(bcosgpu_pack_state_entries(&bad, 1, packed.data(), packed.size(), o2, k2) == BCOSGPU_E_ARG);
    }
    if (fails) return 1;
    if (bcosgpu_device_count() <= 0 || bcosgpu_init(0) != 0) {
        std::printf("packer ok; no gfx950 device: %s\n", bcosgpu_last_error());
        return 77;
    }
    const uint32_t versions[2] = {0u, 0x03010000u};
    for (int v = 0; v < 2; ++v) {
        CHECK(std::memcmp(calculateStateRoot<BCOSGPU_KECCAK256>(ent, versions[v]).data(), want_root[0][v], 32) == 0);
        CHECK(std::memcmp(calculateStateRoot<BCOSGPU_SM3>(ent, versions[v]).data(), want_root[1][v], 32) == 0);
    }
    CHECK(calculateStateRoot<BCOSGPU_KECCAK256>({}, 0x03010000u) == HashType{});
    {   // an engine error throws, as the other adapters do
        std::vector<bcosgpu_StateEntry> bad(1, ent.empty() ? bcosgpu_StateEntry{} : ent[0]);
        bad[0].status = 4;
        bool threw = false;
        try {
            calculateStateRoot<BCOSGPU_SM3>(bad, 0);
        } catch (const std::runtime_error&) {
            threw = true;
        }
        CHECK(threw);
    }
    if (fails) return 1;
    std::printf("state_root_test: ok (%zu entries)\n", n);
    return 0;
}
