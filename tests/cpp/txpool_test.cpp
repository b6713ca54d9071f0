// bcosgpu::GpuTxPool (include/bcos_gpu.hpp) through the C ABI on the GPU: tests/test_gpu_txpool.py writes a
// fixture -- encoded transactions, what the restatement (tests/txpool_restatement.py) returns for them in mode
// FULL, a committed block, a removal, and the three sets after each step -- and this program replays it.
//   u32 suite | u32 n | n x (u32 len, bytes) | n x (hash 32, sender 20, nonce 32, u32 status) | sets
//   | i64 number, u32 nh, nh x 32, u32 nn, nn x 32 | sets | u32 nh, nh x 32, u32 nn, nn x 32 | sets
//   sets = 3 x (u32 count, count x 32)
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>

#include "../../include/bcos_gpu.hpp"

using namespace bcosgpu;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                   \
        }                                                               \
    } while (0)

struct In {
    bytes b;
    size_t pos = 0;
    template <class T>
    T get() {
        T v;
        if (pos + sizeof(T) > b.size()) throw std::runtime_error("fixture too short");
        std::memcpy(&v, b.data() + pos, sizeof(T));
        pos += sizeof(T);
        return v;
    }
    const uint8_t* take(size_t n) {
        if (pos + n > b.size()) throw std::runtime_error("fixture too short");
        pos += n;
        return b.data() + pos - n;
    }
    std::vector<HashType> keys() {
        std::vector<HashType> v(get<uint32_t>());
        for (HashType& k : v) std::memcpy(k.data(), take(32), 32);
        return v;
    }
};

static bool sets_equal(GpuTxPool& pool, In& in) {
    for (int which : {BCOSGPU_TXPOOL_HASHES, BCOSGPU_TXPOOL_NONCES, BCOSGPU_TXPOOL_LEDGER})
        if (pool.dump(which) != in.keys()) return false;
    return pool.info().errorWord == 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    In in{bytes(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>())};
    const int suite = static_cast<int>(in.get<uint32_t>());
    const uint32_t n = in.get<uint32_t>();
    std::vector<std::string_view> encoded;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t len = in.get<uint32_t>();
        encoded.emplace_back(reinterpret_cast<const char*>(in.take(len)), len);
    }
    check(bcosgpu_init(0));
    GpuTxPool pool(suite, "chain0", "group0", 10, 100, 8);
    CHECK(pool.admit({}).status.empty() && pool.info().hashes == 0);
    const TxAdmission r = pool.admit(encoded);
    CHECK(r.status.size() == n);
    for (uint32_t i = 0; i < n; ++i) {
        CHECK(std::memcmp(r.hashes[i].data(), in.take(32), 32) == 0);
        CHECK(std::memcmp(r.senders[i].data(), in.take(20), 20) == 0);
        CHECK(std::memcmp(r.nonces[i].data(), in.take(32), 32) == 0);
        CHECK(r.status[i] == in.get<uint32_t>());
    }
    CHECK(sets_equal(pool, in));
    const int64_t number = in.get<int64_t>();
    const std::vector<HashType> h1 = in.keys(), n1 = in.keys();
    pool.blockCommitted(number, h1, n1);
    CHECK(pool.info().blockNumber == static_cast<uint64_t>(number) && pool.info().blocks == 1);
    CHECK(sets_equal(pool, in));
    const std::vector<HashType> h2 = in.keys(), n2 = in.keys();
    pool.remove(h2, n2);
    CHECK(sets_equal(pool, in));
    pool.loadLedgerNonces({{number + 1, n2}});
    CHECK(pool.info().blocks == 2 && pool.info().ledger >= n2.size());
    CHECK(in.pos == in.b.size());
    std::printf("txpool_test: ok\n");
    return 0;
}
