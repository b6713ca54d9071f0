// header_check_test.cpp -- the block-header check through the C ABI and the C++ adapter (include/bcos_gpu.hpp
// calculateBlockHeaderHash, checkBlockHeaders): bcosgpu_BlockHeaderData views over fixtures written by
// tests/test_header_check.py, whose expected preimages, hashes, verdicts and links come from that file's
// restatement of TarsHashable.h:77-126, BlockValidator.cpp:28-182 and LedgerImpl.h:290-312.
// argv[1..] = fixtures (one per suite).  The packer check runs everywhere; the GPU part exits 77 without a
// gfx950 device.
#include <cstdio>
#include <cstring>
#include <deque>
#include <string>
#include <vector>
#include "../../include/bcos_gpu.hpp"

using namespace bcosgpu;

namespace {
struct Reader {
    std::vector<uint8_t> d;
    size_t at = 0;
    template <class T>
    T get() {
        T v;
        std::memcpy(&v, d.data() + at, sizeof v);
        at += sizeof v;
        return v;
    }
    const uint8_t* raw(size_t n) {
        const uint8_t* p = d.data() + at;
        at += n;
        return p;
    }
    std::pair<const uint8_t*, size_t> bytes() {
        const uint32_t n = get<uint32_t>();
        return {raw(n), n};
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

struct Expected {
    std::pair<const uint8_t*, size_t> data;
    std::vector<uint64_t> off;
    const uint8_t *hash, *check, *link;
    std::pair<const uint8_t*, size_t> sig_ok;
};

struct Fixture {
    Reader r;
    int32_t suite = 0;
    bcosgpu_ConsensusSet cs{};
    std::vector<uint64_t> weights;
    int64_t prev_number = 0;
    HashType prev_hash{};
    std::vector<bcosgpu_BlockHeaderData> headers;
    // the lists the views point to (deques: growing them moves nothing)
    std::deque<std::vector<bcosgpu_ParentInfo>> parents;
    std::deque<std::vector<bcosgpu_Bytes>> sealers;
    std::deque<std::vector<int64_t>> wlists;
    std::deque<std::vector<bcosgpu_HeaderSignature>> sigs;
    Expected want[2];  // dataHash used, recomputed
};

bool load(const char* path, Fixture& f) {
    Reader& r = f.r;
    FILE* fp = std::fopen(path, "rb");
    if (!fp) return false;
    std::fseek(fp, 0, SEEK_END);
    r.d.resize(std::ftell(fp));
    std::fseek(fp, 0, SEEK_SET);
    const bool read = std::fread(r.d.data(), 1, r.d.size(), fp) == r.d.size();
    std::fclose(fp);
    if (!read || r.d.size() < 8 || std::memcmp(r.d.data(), "HDRC", 4) != 0) return false;
    r.at = 4;
    f.suite = r.get<int32_t>();
    f.cs.n = r.get<uint32_t>();
    f.cs.node_ids64 = r.raw(64 * f.cs.n);
    f.weights.resize(f.cs.n);
    for (uint64_t& w : f.weights) w = r.get<uint64_t>();
    f.cs.weights = f.weights.data();
    f.cs.min_required_quorum = r.get<uint64_t>();
    f.cs.committed_index = r.get<int64_t>();
    f.prev_number = r.get<int64_t>();
    std::memcpy(f.prev_hash.data(), r.raw(32), 32);
    const size_t n = r.get<uint32_t>();
    f.headers.resize(n);
    for (bcosgpu_BlockHeaderData& h : f.headers) {
        std::memset(&h, 0, sizeof h);
        h.version = r.get<int32_t>();
        h.block_number = r.get<int64_t>();
        h.timestamp = r.get<int64_t>();
        h.sealer = r.get<int64_t>();
        h.tx_count = r.get<uint64_t>();
        auto b = r.bytes();
        h.txs_root = b.first, h.txs_root_len = b.second;
        b = r.bytes();
        h.receipt_root = b.first, h.receipt_root_len = b.second;
        b = r.bytes();
        h.state_root = b.first, h.state_root_len = b.second;
        b = r.bytes();
        h.gas_used = reinterpret_cast<const char*>(b.first), h.gas_used_len = b.second;
        b = r.bytes();
        h.extra_data = b.first, h.extra_data_len = b.second;
        b = r.bytes();
        h.data_hash = b.first, h.data_hash_len = b.second;
        f.parents.emplace_back(r.get<uint32_t>());
        for (bcosgpu_ParentInfo& p : f.parents.back()) {
            p.block_number = r.get<int64_t>();
            b = r.bytes();
            p.block_hash = b.first, p.block_hash_len = b.second;
        }
        h.parents = f.parents.back().data(), h.nparents = f.parents.back().size();
        f.sealers.emplace_back(r.get<uint32_t>());
        for (bcosgpu_Bytes& s : f.sealers.back()) {
            b = r.bytes();
            s.data = b.first, s.len = b.second;
        }
        h.sealer_list = f.sealers.back().data(), h.nsealer_list = f.sealers.back().size();
        f.wlists.emplace_back(r.get<uint32_t>());
        for (int64_t& w : f.wlists.back()) w = r.get<int64_t>();
        h.consensus_weights = f.wlists.back().data(), h.nconsensus_weights = f.wlists.back().size();
        f.sigs.emplace_back(r.get<uint32_t>());
        for (bcosgpu_HeaderSignature& s : f.sigs.back()) {
            s.sealer_index = r.get<int64_t>();
            b = r.bytes();
            s.signature = b.first, s.signature_len = b.second;
        }
        h.signatures = f.sigs.back().data(), h.nsignatures = f.sigs.back().size();
    }
    for (Expected& e : f.want) {
        e.data = r.bytes();
        e.off.resize(n + 1);
        std::memcpy(e.off.data(), r.raw(8 * (n + 1)), 8 * (n + 1));
        e.hash = r.raw(32 * n);
        e.check = r.raw(n);
        e.link = r.raw(n);
        e.sig_ok = r.bytes();
    }
    return r.at == r.d.size();
}

// the host packer against the restatement's bytes, with and without the recompute flag
void check_packer(const Fixture& f) {
    const size_t n = f.headers.size();
    for (int flags = 0; flags < 2; ++flags) {
        const Expected& e = f.want[flags];
        const uint64_t total = bcosgpu_header_preimage_size(f.headers.data(), n, flags);
        CHECK(total == e.data.second);
        std::vector<uint8_t> packed(total + 1);
        std::vector<uint64_t> off(n + 1);
        CHECK(bcosgpu_pack_header_preimages(f.headers.data(), n, flags, packed.data(), total, off.data()) == BCOSGPU_OK);
        CHECK(off == e.off);
        if (total == e.data.second && total) CHECK(std::memcmp(packed.data(), e.data.first, total) == 0);
        if (total)
            CHECK(bcosgpu_pack_header_preimages(f.headers.data(), n, flags, packed.data(), total - 1, off.data()) ==
                  BCOSGPU_E_ARG);
    }
    if (n) {
        uint64_t o2[2];
        uint8_t buf[8192];
        bcosgpu_BlockHeaderData bad = f.headers[0];
        bad.extra_data = nullptr;  // a null pointer with a length
        bad.extra_data_len = 2;
        CHECK(bcosgpu_pack_header_preimages(&bad, 1, 0, buf, sizeof buf, o2) == BCOSGPU_E_ARG);
        bad = f.headers[0];
        static const uint8_t long_hash[33] = {1};
        bad.data_hash = long_hash;  // a 33-byte dataHash
        bad.data_hash_len = 33;
        CHECK(bcosgpu_pack_header_preimages(&bad, 1, 0, buf, sizeof buf, o2) == BCOSGPU_E_ARG);
    }
}

template <int SUITE>
void check_gpu(const Fixture& f) {
    constexpr int HASHER = SUITE == BCOSGPU_SUITE_SM2 ? BCOSGPU_SM3 : BCOSGPU_KECCAK256;
    const size_t n = f.headers.size();
    for (int flags = 0; flags < 2; ++flags) {
        const Expected& e = f.want[flags];
        const std::vector<HashType> hashes = calculateBlockHeaderHash<HASHER>(f.headers, flags);
        CHECK(hashes.size() == n && (n == 0 || std::memcmp(hashes[0].data(), e.hash, 32 * n) == 0));
        const BlockHeaderCheck r = checkBlockHeaders<SUITE>(f.headers, f.cs, &f.prev_hash, f.prev_number, flags);
        CHECK(r.hashes == hashes);
        CHECK(r.check.size() == n && std::memcmp(r.check.data(), e.check, n) == 0);
        CHECK(r.link.size() == n && std::memcmp(r.link.data(), e.link, n) == 0);
        CHECK(r.sigOk.size() == e.sig_ok.second && std::memcmp(r.sigOk.data(), e.sig_ok.first, r.sigOk.size()) == 0);
        for (size_t i = 0; i < n; ++i) CHECK(r.accepted(i) == (e.check[i] < 16));
    }
    // without a previous hash the first link is not checked; the rest is unchanged
    const BlockHeaderCheck r = checkBlockHeaders<SUITE>(f.headers, f.cs);
    CHECK(n == 0 || r.link[0] == BCOSGPU_LINK_UNCHECKED);
    CHECK(n < 2 || std::memcmp(r.link.data() + 1, f.want[0].link + 1, n - 1) == 0);
    CHECK(checkBlockHeaders<SUITE>({}, f.cs).check.empty());
    {   // an engine error throws, as the other adapters do
        std::vector<bcosgpu_BlockHeaderData> bad(1, f.headers[0]);
        bad[0].signatures = nullptr;
        bad[0].nsignatures = 1;
        bool threw = false;
        try {
            checkBlockHeaders<SUITE>(bad, f.cs);
        } catch (const std::runtime_error&) {
            threw = true;
        }
        CHECK(threw);
    }
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::deque<Fixture> fx;
    for (int a = 1; a < argc; ++a) {
        fx.emplace_back();
        if (!load(argv[a], fx.back()) || fx.back().headers.empty()) {
            std::printf("bad fixture %s\n", argv[a]);
            return 2;
        }
        check_packer(fx.back());
    }
    if (fails) return 1;
    if (bcosgpu_device_count() <= 0 || bcosgpu_init(0) != 0) {
        std::printf("packer ok; no gfx950 device: %s\n", bcosgpu_last_error());
        return 77;
    }
    size_t total = 0;
    for (const Fixture& f : fx) {
        if (f.suite == BCOSGPU_SUITE_SM2) check_gpu<BCOSGPU_SUITE_SM2>(f);
        else check_gpu<BCOSGPU_SUITE_SECP256K1>(f);
        total += f.headers.size();
    }
    if (fails) return 1;
    std::printf("header_check_test: ok (%zu headers)\n", total);
    return 0;
}
