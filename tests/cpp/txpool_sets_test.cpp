// The kernel bodies of csrc/sorted_set.h and csrc/txpool_admit.h on the CPU (tests/test_txpool_sets.py builds
// this with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it alone).  Each "kernel" is its body
// called for every thread index of its grid, serially, grids rounded up to whole 256-thread blocks as the real
// launches are; the library sort is std::sort with the same comparator, the library scan std::exclusive_scan.
// Every buffer is malloc'ed at exactly the capacity the body is told, so an index out of range is an ASan report.
//
//   sets    the sets against std::set after every operation (the cases are listed in main_sets)
//   admit   verdict / rule / finalize against a literal loop of the reference's order (the C++ twin of
//           tests/txpool_restatement.py) on batches dense in repeated nonces and repeated whole transactions
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../../fisco-bcos_amd/csrc/sorted_set.h"
#include "../../fisco-bcos_amd/csrc/txpool_admit.h"

using namespace bcosgpu;
using sset::Rec;
using sset::SetView;
using Key = std::array<uint8_t, 32>;  // std::array compares lexicographically = as a big-endian number

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

// a buffer of exactly n elements (n == 0: one byte nobody may touch as a T)
template <class T>
struct Buf {
    T* p;
    uint32_t n;
    explicit Buf(uint32_t count) : p(static_cast<T*>(std::malloc(count ? sizeof(T) * count : 1))), n(count) {
        if (count) std::memset(p, 0xA5, sizeof(T) * count);
    }
    ~Buf() { std::free(p); }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
};

template <class F>
void launch(uint64_t threads, F body) {
    const uint64_t grid = (threads + 255) / 256 * 256;  // the spare threads of the last block run too
    for (uint64_t t = 0; t < grid; ++t) body(t);
}

struct HostSet {
    uint8_t* buf[2];
    uint32_t count[2] = {0, 0};
    int cur = 0;
    uint32_t cap, bound = 0;
    int growths = 0;
    explicit HostSet(uint32_t c) : cap(c) {
        for (auto& b : buf) b = static_cast<uint8_t*>(std::malloc(32 * static_cast<size_t>(cap)));
    }
    ~HostSet() {
        for (auto& b : buf) std::free(b);
    }
    SetView view() const { return SetView{buf[cur], &count[cur], cap}; }
    // rule 5: between calls, on the host
    void reserve(uint32_t incoming) {
        if (static_cast<uint64_t>(bound) + incoming <= cap) return;
        uint32_t want = std::max<uint32_t>(2 * cap, bound + incoming);
        uint8_t* a = static_cast<uint8_t*>(std::malloc(32 * static_cast<size_t>(want)));
        uint8_t* b = static_cast<uint8_t*>(std::malloc(32 * static_cast<size_t>(want)));
        std::memcpy(a, buf[cur], 32 * static_cast<size_t>(count[cur]));
        std::free(buf[0]);
        std::free(buf[1]);
        buf[0] = a;
        buf[1] = b;
        count[0] = count[cur];
        cur = 0;
        cap = want;
        ++growths;
    }
    std::vector<Key> dump() const {
        std::vector<Key> v(count[cur]);
        for (uint32_t i = 0; i < count[cur]; ++i) std::memcpy(v[i].data(), buf[cur] + 32 * static_cast<size_t>(i), 32);
        return v;
    }
};

static uint32_t g_err = 0;

// the union's chain after the sort: flags (general, or given), scan, compact, merge
static void union_sorted(HostSet& s, const Buf<Rec>& recs, uint32_t m, const uint32_t* given_flag) {
    Buf<uint32_t> flag(m), pos(m);
    Buf<uint8_t> bprime(32 * m);
    uint32_t nb = 0xFFFFFFFFu;
    if (given_flag) std::memcpy(flag.p, given_flag, 4 * static_cast<size_t>(m));
    else launch(m, [&](uint64_t t) { sset::union_flag_body(t, m, recs.p, s.view(), flag.p, m, &g_err); });
    std::exclusive_scan(flag.p, flag.p + m, pos.p, 0u);
    launch(m, [&](uint64_t t) { sset::compact_body(t, m, recs.p, flag.p, pos.p, bprime.p, m, &nb, &g_err); });
    const SetView b{bprime.p, &nb, m};
    const int o = 1 - s.cur;
    launch(static_cast<uint64_t>(s.bound) + m,
           [&](uint64_t t) { sset::merge_body(t, s.bound, m, s.view(), b, s.buf[o], s.cap, &s.count[o], &g_err); });
    s.cur = o;
    s.bound = s.count[o];  // ("whenever it has synchronised anyway": here always)
}

static void set_union(HostSet& s, const std::vector<Key>& batch, bool grow = true) {
    const uint32_t m = static_cast<uint32_t>(batch.size());
    if (m == 0) return;  // n == 0 changes nothing
    if (grow) s.reserve(m);
    Buf<uint8_t> in(32 * m);
    for (uint32_t i = 0; i < m; ++i) std::memcpy(in.p + 32 * static_cast<size_t>(i), batch[i].data(), 32);
    Buf<Rec> recs(m);
    launch(m, [&](uint64_t t) { sset::records_body(t, m, in.p, recs.p, m, &g_err); });
    std::sort(recs.p, recs.p + m, sset::RecLess());
    union_sorted(s, recs, m, nullptr);
}

static void set_diff(HostSet& s, const std::vector<Key>& batch) {
    const uint32_t m = static_cast<uint32_t>(batch.size()), na = s.bound;
    if (m == 0 || na == 0) return;
    Buf<uint8_t> in(32 * m);
    for (uint32_t i = 0; i < m; ++i) std::memcpy(in.p + 32 * static_cast<size_t>(i), batch[i].data(), 32);
    Buf<Rec> recs(m);
    launch(m, [&](uint64_t t) { sset::records_body(t, m, in.p, recs.p, m, &g_err); });
    std::sort(recs.p, recs.p + m, sset::RecLess());
    Buf<uint32_t> keep(na), pos(na);
    launch(na, [&](uint64_t t) { sset::diff_keep_body(t, na, s.view(), recs.p, m, keep.p, na, &g_err); });
    std::exclusive_scan(keep.p, keep.p + na, pos.p, 0u);
    const int o = 1 - s.cur;
    launch(na, [&](uint64_t t) {
        sset::diff_scatter_body(t, na, s.view(), keep.p, pos.p, s.buf[o], s.cap, &s.count[o], &g_err);
    });
    s.cur = o;
    s.bound = s.count[o];
}

static void expect(const HostSet& s, const std::set<Key>& want) {
    const std::vector<Key> got = s.dump();
    CHECK(got.size() == want.size());
    CHECK(std::equal(got.begin(), got.end(), want.begin()));  // ascending, strictly: std::set's own order
    CHECK(g_err == 0);
    // contains: every key of the set, and a neighbour of each
    std::vector<Key> probe(got);
    for (Key k : got) {
        k[31] ^= 1;
        probe.push_back(k);
    }
    const uint32_t n = static_cast<uint32_t>(probe.size());
    Buf<uint8_t> in(32 * n), out(n);
    for (uint32_t i = 0; i < n; ++i) std::memcpy(in.p + 32 * static_cast<size_t>(i), probe[i].data(), 32);
    launch(n, [&](uint64_t t) { sset::contains_body(t, n, in.p, s.view(), out.p, n, &g_err); });
    for (uint32_t i = 0; i < n; ++i) CHECK((out.p[i] != 0) == (want.count(probe[i]) != 0));
}

static Key small_key(uint32_t v) {
    Key k{};
    k[28] = static_cast<uint8_t>(v >> 24);
    k[29] = static_cast<uint8_t>(v >> 16);
    k[30] = static_cast<uint8_t>(v >> 8);
    k[31] = static_cast<uint8_t>(v);
    return k;
}

static Key random_key(std::mt19937_64& rng) {
    Key k;
    for (auto& b : k) b = static_cast<uint8_t>(rng());
    return k;
}

static int main_sets() {
    std::mt19937_64 rng(20260);
    std::set<Key> want;
    auto do_union = [&](HostSet& s, const std::vector<Key>& b) {
        set_union(s, b);
        want.insert(b.begin(), b.end());
        expect(s, want);
    };
    auto do_diff = [&](HostSet& s, const std::vector<Key>& b) {
        set_diff(s, b);
        for (const Key& k : b) want.erase(k);
        expect(s, want);
    };
    {
        HostSet s(8);
        expect(s, want);
        do_union(s, {});                                          // an empty batch
        do_diff(s, {small_key(1)});                               // erase from the empty set
        do_union(s, {small_key(7)});                              // a batch of one key
        do_union(s, std::vector<Key>(130, small_key(9)));         // all one key, 130 copies: crosses growth
        CHECK(s.growths >= 1 && s.count[s.cur] == 2);
        do_union(s, s.dump());                                    // a batch equal to the set
        std::vector<Key> big;
        for (uint32_t i = 0; i < 300; ++i) big.push_back(small_key(1000 + 3 * i));
        do_union(s, big);                                         // a batch larger than the set
        do_diff(s, {small_key(2), small_key(1001), small_key(5000)});  // erase of absent keys
        do_diff(s, std::vector<Key>(130, small_key(9)));          // erase by 130 copies of one key
        do_diff(s, {});
        Key zero{}, ones;
        ones.fill(0xFF);
        do_union(s, {ones, zero, ones, zero});                    // keys 0 and 2^256 - 1
        Key a = random_key(rng), b = a, c = a;
        b[31] = static_cast<uint8_t>(a[31] + 1);
        c[31] = static_cast<uint8_t>(a[31] + 2);
        do_union(s, {c, a, b});                                   // keys that differ only in the last byte
        do_diff(s, {b});
        do_diff(s, {zero, ones});
        do_diff(s, s.dump());                                     // erase of everything ...
        CHECK(want.empty());
        do_union(s, {small_key(3), small_key(1), small_key(2)});  // ... then insert
    }
    want.clear();
    {   // a union that lands exactly on capacity, then one key over it without the host's growth: the kernel
        // refuses the store and sets the error word
        HostSet s(16);
        std::vector<Key> b;
        for (uint32_t i = 0; i < 10; ++i) b.push_back(small_key(10 * i));
        do_union(s, b);
        b.clear();
        for (uint32_t i = 0; i < 6; ++i) b.push_back(small_key(10 * i + 5));
        do_union(s, b);
        CHECK(s.count[s.cur] == 16 && s.cap == 16 && s.growths == 0);
        set_union(s, {small_key(7)}, false);
        CHECK(g_err == sset::kErrStore);
        CHECK(s.count[s.cur] == 16);
        g_err = 0;
        // with the host's growth the same key goes in (the refused call's output buffer is abandoned)
        s.cur = 1 - s.cur;
        s.bound = s.count[s.cur];
        do_union(s, {small_key(7)});
        CHECK(s.growths == 1 && s.cap == 32);
    }
    want.clear();
    for (uint32_t cap0 : {1u, 8u, 64u}) {  // random operation sequences from a small universe (dense in repeats)
        want.clear();
        HostSet s(cap0);
        for (int step = 0; step < 300; ++step) {
            std::vector<Key> b(rng() % 40);
            for (auto& k : b) k = rng() % 8 ? small_key(static_cast<uint32_t>(rng() % 200)) : random_key(rng);
            if (rng() % 3) do_union(s, b);
            else do_diff(s, b);
        }
    }
    std::printf("sets: ok\n");
    return 0;
}

// ---------------------------------------------------------------- admission
struct Fields {  // the part of tars::TxFields the bodies read
    uint64_t off[8];
    uint32_t len[8];
    int32_t version;
    int64_t block_limit;
};

struct TestTx {
    bool decoded;
    std::string chain, group, nonce;
    int64_t limit;
    bool sig_ok;
    Key hash;  // a function of the preimage fields: equal hashes <=> equal preimages
};

static Key digest(const std::string& s) {  // 4 x FNV-1a with different offsets; collisions do not matter at this size
    Key k;
    for (int w = 0; w < 4; ++w) {
        uint64_t h = 1469598103934665603ull + 977u * static_cast<uint64_t>(w);
        for (unsigned char c : s) h = (h ^ c) * 1099511628211ull;
        for (int i = 0; i < 8; ++i) k[8 * w + i] = static_cast<uint8_t>(h >> (56 - 8 * i));
    }
    return k;
}

static bool canonical(const std::string& s, Key& out) {
    return parse_canonical_nonce(reinterpret_cast<const uint8_t*>(s.data()), static_cast<uint32_t>(s.size()), out.data());
}

struct LiteralPool {  // tests/txpool_restatement.py, line by line
    std::set<Key> hashes, nonces, ledger;
    std::string chain = "chain0", group = "group0";
    int64_t number = 100, range = 10;
    uint32_t verify_and_submit(const TestTx& t) {
        if (!t.decoded) return admit::kMalformed;
        if (hashes.count(t.hash)) return admit::kAlreadyInTxPool;
        if (t.group != group) return admit::kInvalidGroupId;
        if (t.chain != chain) return admit::kInvalidChainId;
        Key v;
        if (!canonical(t.nonce, v)) return admit::kNonceForHost;
        if (nonces.count(v)) return admit::kNonceCheckFail;
        if (ledger.count(v)) return admit::kNonceCheckFail;
        if (number >= t.limit || number + range < t.limit) return admit::kBlockLimitCheckFail;
        if (!t.sig_ok) return admit::kInvalidSignature;
        nonces.insert(v);
        hashes.insert(t.hash);
        return admit::kOk;
    }
    uint32_t enforce_submit(const TestTx& t) {
        if (!t.decoded) return admit::kMalformed;
        Key v;
        if (!canonical(t.nonce, v)) return admit::kNonceForHost;
        if (ledger.count(v)) return admit::kNonceCheckFail;
        if (!t.sig_ok) return admit::kInvalidSignature;
        hashes.insert(t.hash);
        return admit::kOk;
    }
};

static TestTx random_tx(std::mt19937_64& rng) {
    static const char* nonces[] = {"", "0", "1", "2", "3", "07", "7", "+1",
                                   "115792089237316195423570985008687907853269984665640564039457584007913129639935"};
    static const int64_t limits[] = {100, 101, 105, 110, 111};
    TestTx t;
    t.decoded = rng() % 20 != 0;
    t.group = rng() % 10 ? "group0" : "other";
    t.chain = rng() % 10 ? "chain0" : "other";
    t.nonce = nonces[rng() % 9];
    t.limit = limits[rng() % 5];
    t.sig_ok = rng() % 5 != 0;
    const std::string to = rng() % 2 ? "a" : "b";
    t.hash = digest(t.group + "|" + t.chain + "|" + t.nonce + "|" + std::to_string(t.limit) + "|" + to);
    if (!t.decoded) t.hash = Key{};
    return t;
}

static void load(HostSet& s, const std::set<Key>& keys) {
    s.reserve(static_cast<uint32_t>(keys.size()));
    uint32_t i = 0;
    for (const Key& k : keys) std::memcpy(s.buf[s.cur] + 32 * static_cast<size_t>(i++), k.data(), 32);
    s.count[s.cur] = s.bound = i;
}

// one admit call through the bodies, as txpool_kernels.hip chains them
static std::vector<uint32_t> admit_call(int mode, const std::vector<TestTx>& txs, HostSet& hashes, HostSet& nonces,
                                        HostSet& ledger, const LiteralPool& pool, std::vector<Key>& nonce_out,
                                        std::vector<std::array<uint8_t, 20>>& sender_out) {
    const uint32_t n = static_cast<uint32_t>(txs.size());
    std::string bytes;
    std::vector<Fields> fields(n);
    Buf<uint8_t> vstatus(n), txhash(32 * n), sender(20 * n), nonce32(32 * n);
    for (uint32_t j = 0; j < n; ++j) {
        std::memset(&fields[j], 0, sizeof(Fields));
        const std::string* f[3] = {&txs[j].chain, &txs[j].group, &txs[j].nonce};
        for (int k = 0; k < 3 && txs[j].decoded; ++k) {
            fields[j].off[k] = bytes.size();
            fields[j].len[k] = static_cast<uint32_t>(f[k]->size());
            bytes += *f[k];
        }
        fields[j].block_limit = txs[j].limit;
        vstatus.p[j] = !txs[j].decoded ? 2 : txs[j].sig_ok ? 0 : 1;
        std::memcpy(txhash.p + 32 * static_cast<size_t>(j), txs[j].hash.data(), 32);
        if (!txs[j].decoded) std::memset(txhash.p + 32 * static_cast<size_t>(j), 0xEE, 32);  // (the hash of nothing)
        std::memset(sender.p + 20 * static_cast<size_t>(j), 0x11, 20);
    }
    Buf<uint8_t> enc(static_cast<uint32_t>(bytes.size()));
    std::memcpy(enc.p, bytes.data(), bytes.size());
    Buf<uint8_t> chain(static_cast<uint32_t>(pool.chain.size())), group(static_cast<uint32_t>(pool.group.size()));
    std::memcpy(chain.p, pool.chain.data(), pool.chain.size());
    std::memcpy(group.p, pool.group.data(), pool.group.size());
    const admit::PoolParams pp{chain.p, group.p, chain.n, group.n, pool.number, pool.range};
    Buf<uint32_t> status(n);
    Buf<Rec> recs(n);
    launch(n, [&](uint64_t t) {
        admit::verdict_body(t, n, mode, enc.p, enc.n, fields.data(), vstatus.p, txhash.p, hashes.view(), nonces.view(),
                            ledger.view(), pp, status.p, nonce32.p, recs.p, n, &g_err);
    });
    if (mode == admit::kModeFull) {
        std::sort(recs.p, recs.p + n, sset::RecLess());
        Buf<uint32_t> ok(n), c(n), win(n);
        launch(n, [&](uint64_t t) { admit::run_ok_body(t, n, recs.p, status.p, ok.p, n, &g_err); });
        std::exclusive_scan(ok.p, ok.p + n, c.p, 0u);
        launch(n, [&](uint64_t t) {
            admit::run_rule_body(t, n, recs.p, ok.p, c.p, txhash.p, status.p, win.p, n, &g_err);
        });
        nonces.reserve(n);
        union_sorted(nonces, recs, n, win.p);
    }
    launch(n, [&](uint64_t t) { admit::finalize_body(t, n, status.p, txhash.p, sender.p, recs.p, n, &g_err); });
    std::sort(recs.p, recs.p + n, sset::RecLess());
    hashes.reserve(n);
    union_sorted(hashes, recs, n, nullptr);
    nonce_out.resize(n);
    sender_out.resize(n);
    for (uint32_t j = 0; j < n; ++j) {
        std::memcpy(nonce_out[j].data(), nonce32.p + 32 * static_cast<size_t>(j), 32);
        std::memcpy(sender_out[j].data(), sender.p + 20 * static_cast<size_t>(j), 20);
        if (!txs[j].decoded)
            for (int i = 0; i < 32; ++i) CHECK(txhash.p[32 * static_cast<size_t>(j) + i] == 0);
    }
    return std::vector<uint32_t>(status.p, status.p + n);
}

static int main_admit() {
    std::mt19937_64 rng(6);
    for (int trial = 0; trial < 600; ++trial) {
        LiteralPool lit;
        lit.ledger.insert(small_key(3));
        const int warm = static_cast<int>(rng() % 5);
        for (int i = 0; i < warm; ++i) lit.verify_and_submit(random_tx(rng));
        HostSet hashes(trial % 2 ? 8 : 1), nonces(trial % 3 ? 8 : 1), ledger(4);
        load(hashes, lit.hashes);
        load(nonces, lit.nonces);
        load(ledger, lit.ledger);
        // several calls against one pool, the sets carried over; sizes around the 256-thread block too
        for (int call = 0; call < 3; ++call) {
            const int mode = rng() % 4 ? admit::kModeFull : admit::kModeProposal;
            std::vector<TestTx> txs(trial % 50 == 0 ? 255 + rng() % 4 : 1 + rng() % 24);
            for (auto& t : txs) t = random_tx(rng);
            for (size_t j = 1; j < txs.size(); ++j)
                if (rng() % 6 == 0) txs[j] = txs[rng() % j];  // whole transactions again
            std::vector<uint32_t> want;
            for (const TestTx& t : txs)
                want.push_back(mode == admit::kModeFull ? lit.verify_and_submit(t) : lit.enforce_submit(t));
            std::vector<Key> nonce_out;
            std::vector<std::array<uint8_t, 20>> sender_out;
            const std::vector<uint32_t> got = admit_call(mode, txs, hashes, nonces, ledger, lit, nonce_out, sender_out);
            CHECK(g_err == 0);
            CHECK(got == want);
            for (size_t j = 0; j < txs.size(); ++j) {
                Key v{}, z{};
                const bool canon = txs[j].decoded && canonical(txs[j].nonce, v);
                CHECK(nonce_out[j] == (canon ? v : z));
                for (uint8_t b : sender_out[j]) CHECK(b == (got[j] == admit::kOk ? 0x11 : 0));
            }
            expect(hashes, lit.hashes);
            expect(nonces, lit.nonces);
            expect(ledger, lit.ledger);
        }
    }
    std::printf("admit: ok\n");
    return 0;
}

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "sets") return main_sets();
    if (what == "admit") return main_admit();
    std::printf("usage: txpool_sets_test sets|admit\n");
    return 2;
}
