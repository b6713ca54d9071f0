// pbft_check_test.cpp -- the PBFT message check through the C ABI and the C++ adapter (include/bcos_gpu.hpp
// checkPBFTMessages): bcosgpu_PBFTMessageData views over fixtures written by tests/test_pbft_check.py, whose
// expected hashes, verdict bits, prepared-proposal codes and row verdicts come from that file's restatement of
// PBFTEngine.cpp:732-771, :1230-1271 and PBFTCacheProcessor.cpp:795-821.
// argv[1..] = fixtures (one per suite).  The argument checks run everywhere; the GPU part exits 77 without a
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

struct Fixture {
    Reader r;
    int32_t suite = 0;
    bcosgpu_ConsensusSet cs{};
    std::vector<uint64_t> weights;
    std::vector<bcosgpu_PBFTMessageData> msgs;
    std::vector<bcosgpu_PBFTGroup> groups;
    // the lists the views point to (deques: growing them moves nothing)
    std::deque<std::vector<bcosgpu_PrecommitProof>> prepared;
    std::deque<std::vector<bcosgpu_HeaderSignature>> proofs;
    const uint8_t* hash = nullptr;
    std::vector<uint32_t> flags;
    std::pair<const uint8_t*, size_t> prepared_check, sig_ok;
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
    if (!read || r.d.size() < 8 || std::memcmp(r.d.data(), "PBFT", 4) != 0) return false;
    r.at = 4;
    f.suite = r.get<int32_t>();
    f.cs.n = r.get<uint32_t>();
    f.cs.node_ids64 = r.raw(64 * f.cs.n);
    f.weights.resize(f.cs.n);
    for (uint64_t& w : f.weights) w = r.get<uint64_t>();
    f.cs.weights = f.weights.data();
    f.cs.min_required_quorum = r.get<uint64_t>();
    f.cs.committed_index = -1;
    const size_t n = r.get<uint32_t>();
    f.msgs.resize(n);
    for (bcosgpu_PBFTMessageData& m : f.msgs) {
        std::memset(&m, 0, sizeof m);
        m.generated_from = r.get<int64_t>();
        m.checks = r.get<uint32_t>();
        auto b = r.bytes();
        m.signed_data = b.first, m.signed_data_len = b.second;
        b = r.bytes();
        m.signature_hash = b.first, m.signature_hash_len = b.second;
        b = r.bytes();
        m.signature = b.first, m.signature_len = b.second;
        b = r.bytes();
        m.proposal_hash = b.first, m.proposal_hash_len = b.second;
        b = r.bytes();
        m.proposal_signature = b.first, m.proposal_signature_len = b.second;
        f.prepared.emplace_back(r.get<uint32_t>());
        for (bcosgpu_PrecommitProof& p : f.prepared.back()) {
            b = r.bytes();
            p.hash = b.first, p.hash_len = b.second;
            f.proofs.emplace_back(r.get<uint32_t>());
            for (bcosgpu_HeaderSignature& s : f.proofs.back()) {
                s.sealer_index = r.get<int64_t>();
                b = r.bytes();
                s.signature = b.first, s.signature_len = b.second;
            }
            p.proofs = f.proofs.back().data(), p.nproofs = f.proofs.back().size();
        }
        m.prepared = f.prepared.back().data(), m.nprepared = f.prepared.back().size();
    }
    f.groups.resize(r.get<uint32_t>());
    for (bcosgpu_PBFTGroup& g : f.groups) {
        g.parent = r.get<uint64_t>();
        g.first = r.get<uint64_t>();
        g.count = r.get<uint64_t>();
    }
    f.hash = r.raw(32 * n);
    f.flags.resize(n);
    std::memcpy(f.flags.data(), r.raw(4 * n), 4 * n);
    f.prepared_check = r.bytes();
    f.sig_ok = r.bytes();
    return r.at == r.d.size();
}

// what the host call refuses before it touches a device
void check_arguments(const Fixture& f) {
    std::vector<HashType> h(f.msgs.size());
    std::vector<uint32_t> fl(f.msgs.size());
    auto call = [&](const bcosgpu_PBFTMessageData* m, size_t n, const bcosgpu_PBFTGroup* g, size_t ng, int flags) {
        return bcosgpu_pbft_check(f.suite, m, n, g, ng, &f.cs, flags, h[0].data(), fl.data(), nullptr, nullptr);
    };
    CHECK(call(f.msgs.data(), 0, nullptr, 0, 0) == BCOSGPU_OK);  // n == 0 is a no-op
    CHECK(call(f.msgs.data(), 1, nullptr, 0, 1) == BCOSGPU_E_ARG);  // reserved flags
    CHECK(call(nullptr, 1, nullptr, 0, 0) == BCOSGPU_E_ARG);
    CHECK(call(f.msgs.data(), 1, nullptr, 1, 0) == BCOSGPU_E_ARG);
    bcosgpu_PBFTMessageData bad = f.msgs[0];
    bad.signed_data = nullptr, bad.signed_data_len = 2;  // a null pointer with a length
    CHECK(call(&bad, 1, nullptr, 0, 0) == BCOSGPU_E_ARG);
    static const uint8_t long_hash[33] = {1};
    bad = f.msgs[0];
    bad.signature_hash = long_hash, bad.signature_hash_len = 33;
    CHECK(call(&bad, 1, nullptr, 0, 0) == BCOSGPU_E_ARG);
    bad = f.msgs[0];
    bad.proposal_hash = long_hash, bad.proposal_hash_len = 33;
    CHECK(call(&bad, 1, nullptr, 0, 0) == BCOSGPU_E_ARG);
    bad = f.msgs[0];
    bad.prepared = nullptr, bad.nprepared = 1;
    CHECK(call(&bad, 1, nullptr, 0, 0) == BCOSGPU_E_ARG);
    const size_t n = f.msgs.size();
    const bcosgpu_PBFTGroup outside[3] = {{n, 0, 0}, {0, n + 1, 0}, {0, 1, n}};  // parent, first, first + count
    for (const bcosgpu_PBFTGroup& g : outside) CHECK(call(f.msgs.data(), n, &g, 1, 0) == BCOSGPU_E_ARG);
}

template <int SUITE>
void check_gpu(const Fixture& f) {
    const size_t n = f.msgs.size();
    const PBFTMessageCheck r = checkPBFTMessages<SUITE>(f.msgs, f.cs, f.groups);
    CHECK(r.hashes.size() == n && std::memcmp(r.hashes[0].data(), f.hash, 32 * n) == 0);
    CHECK(r.flags == f.flags);
    CHECK(r.preparedCheck.size() == f.prepared_check.second &&
          std::memcmp(r.preparedCheck.data(), f.prepared_check.first, r.preparedCheck.size()) == 0);
    CHECK(r.sigOk.size() == f.sig_ok.second && std::memcmp(r.sigOk.data(), f.sig_ok.first, r.sigOk.size()) == 0);
    for (size_t i = 0; i < n; ++i) CHECK(r.accepted(i) == (f.flags[i] == 0));
    // without the groups only bits 16 and 32 go
    const PBFTMessageCheck plain = checkPBFTMessages<SUITE>(f.msgs, f.cs);
    for (size_t i = 0; i < n; ++i) CHECK(plain.flags[i] == (f.flags[i] & 15u));
    CHECK(checkPBFTMessages<SUITE>({}, f.cs).flags.empty());
    {   // an engine error throws, as the other adapters do
        std::vector<bcosgpu_PBFTMessageData> bad(1, f.msgs[0]);
        bad[0].signature = nullptr;
        bad[0].signature_len = 64;
        bool threw = false;
        try {
            checkPBFTMessages<SUITE>(bad, f.cs);
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
        if (!load(argv[a], fx.back()) || fx.back().msgs.empty()) {
            std::printf("bad fixture %s\n", argv[a]);
            return 2;
        }
        check_arguments(fx.back());
    }
    if (fails) return 1;
    if (bcosgpu_device_count() <= 0 || bcosgpu_init(0) != 0) {
        std::printf("arguments ok; no gfx950 device: %s\n", bcosgpu_last_error());
        return 77;
    }
    size_t total = 0;
    for (const Fixture& f : fx) {
        if (f.suite == BCOSGPU_SUITE_SM2) check_gpu<BCOSGPU_SUITE_SM2>(f);
        else check_gpu<BCOSGPU_SUITE_SECP256K1>(f);
        total += f.msgs.size();
    }
    if (fails) return 1;
    std::printf("pbft_check_test: ok (%zu messages)\n", total);
    return 0;
}
