// cipher_test.cpp -- DataEncryption over storage values (RocksDBStorage.cpp:348-353, :513-524, :106-108, :204-205)
// through the C++ adapter (include/bcos_gpu.hpp encryptStorageValues / decryptStorageValues): std::string_views
// over a fixture written by tests/test_gpu_cipher.py, whose expected ciphertexts come from the restatement
// tests/cipher_restatement.py.  argv[1] = fixture.  Exits 77 without a gfx950 device.
#include <cstdio>
#include <cstring>
#include <string>
#include <string_view>
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
    std::string_view bytes() {
        const uint32_t n = u32();
        const char* p = reinterpret_cast<const char*>(d.data()) + at;
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

template <int CIPHER>
void run(std::string_view key, const std::vector<std::string_view>& values, const std::vector<std::string_view>& want) {
    const size_t n = values.size();
    // asyncPrepare's shape: an empty value is left alone
    const std::vector<std::string> ct = encryptStorageValues<CIPHER>(key, values);
    CHECK(ct.size() == n);
    for (size_t i = 0; i < n; ++i) CHECK(values[i].empty() ? ct[i].empty() : ct[i] == want[i]);
    // setRows' shape: every value goes through, an empty one becomes a block
    const std::vector<std::string> all = encryptStorageValues<CIPHER>(key, values, false);
    for (size_t i = 0; i < n; ++i) CHECK(all[i] == want[i]);
    // the reads: what was stored comes back; an empty stored value stays empty
    std::vector<std::string_view> stored(ct.begin(), ct.end());
    DecryptedStorageValues back = decryptStorageValues<CIPHER>(key, stored);
    CHECK(back.values.size() == n && back.status.size() == n);
    for (size_t i = 0; i < n; ++i) CHECK(back.values[i] == values[i] && back.status[i] == BCOSGPU_CBC_OK);
    // a damaged row fails alone, where the reference throws DecryptException
    if (n >= 3) {
        std::string cut = all[1].substr(0, all[1].size() - 1), flipped = all[2];
        flipped.back() ^= 0x55;
        std::vector<std::string_view> rows = {all[0], cut, flipped};
        back = decryptStorageValues<CIPHER>(key, rows);
        CHECK(back.status[0] == BCOSGPU_CBC_OK && back.values[0] == values[0]);
        CHECK(back.status[1] == BCOSGPU_CBC_E_LENGTH && back.values[1].empty());
        CHECK(back.status[2] != BCOSGPU_CBC_OK || back.values[2] != values[2]);
    }
    CHECK(encryptStorageValues<CIPHER>(key, {}).empty());
    CHECK(decryptStorageValues<CIPHER>(key, {}).values.empty());
}
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
    if (r.d.size() < 8 || std::memcmp(r.d.data(), "CIPH", 4) != 0) return 2;
    r.at = 4;
    const std::string_view key = r.bytes();
    const size_t n = r.u32();
    std::vector<std::string_view> values(n), want[2];
    for (size_t i = 0; i < n; ++i) values[i] = r.bytes();
    for (int c = 0; c < 2; ++c)
        for (size_t i = 0; i < n; ++i) want[c].push_back(r.bytes());
    if (r.at != r.d.size()) {
        std::printf("fixture size mismatch\n");
        return 2;
    }
    if (bcosgpu_device_count() <= 0 || bcosgpu_init(0) != 0) {
        std::printf("no gfx950 device: %s\n", bcosgpu_last_error());
        return 77;
    }
    run<BCOSGPU_CIPHER_AES256>(key, values, want[0]);
    run<BCOSGPU_CIPHER_SM4>(key, values, want[1]);
    {   // an engine error throws, as the other adapters do
        bool threw = false;
        try {
            std::vector<uint64_t> off(2);
            uint8_t out[16];
            const bcosgpu_Bytes v{nullptr, 0};
            check(bcosgpu_cbc_encrypt_batch(7, nullptr, 0, nullptr, 0, &v, 1, out, 16, off.data()));
        } catch (const std::runtime_error&) {
            threw = true;
        }
        CHECK(threw);
    }
    if (fails) return 1;
    std::printf("cipher_test: ok (%zu values)\n", n);
    return 0;
}
