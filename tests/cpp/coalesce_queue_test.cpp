// coalesce_queue_test.cpp -- the coalescer's queue protocol and staging layout (csrc/coalesce_queue.h) on the
// CPU, with a stand-in for the GPU batch.  tests/test_coalesce_queue.py builds this file with
// -fsanitize=thread and with -fsanitize=address,undefined and runs it as a child process.
//
//   coalesce_queue_test protocol <threads> <calls_per_thread> [seed]
//   coalesce_queue_test boundary [seed]      (BCOSGPU_COALESCE_SLOTS=1)
//   coalesce_queue_test quiesce <rounds> [seed]   (BCOSGPU_COALESCE_SLOTS=1)
//   coalesce_queue_test layout [seed]
// The BCOSGPU_COALESCE_* variables are read once per process, as in the library.  Prints one JSON line; exit 0
// iff nothing was violated, 1 with "violations" filled, 3 when a call did not return (the watchdog).
//
// The stand-in's "signature function": every output byte of an item is a pure function of that item's own
// input bytes (in the order the kind's kernel reads them) and the kind, so a result that belongs to another
// item, a stale one or an untouched buffer cannot pass.
#include "../../fisco-bcos_amd/csrc/coalesce_queue.h"

#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <memory>
#include <random>
#include <stdexcept>
#include <thread>

using namespace bcosgpu;
using namespace bcosgpu::coalesce;

namespace {

constexpr uint8_t kGuard = 0xA5;
constexpr int kStandInRc = -77;

struct NoPayload {};
using Queue = DeviceQueue<NoPayload>;
using QSlot = Slot<NoPayload>;

uint64_t mix(uint64_t h, const uint8_t* p, size_t len) {
    size_t i = 0;
    for (; i + 8 <= len; i += 8) {
        uint64_t w;
        std::memcpy(&w, p + i, 8);
        h = (h ^ w) * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
    }
    for (; i < len; ++i) {
        h = (h ^ p[i]) * 0x100000001B3ull;
        h ^= h >> 31;
    }
    return h;
}

// hash32, then the signature bytes the kind reads, then the key (verify kinds)
uint64_t item_fn(int kind, const uint8_t* hash32, const uint8_t* sig, const uint8_t* pub64) {
    uint64_t h = mix(0xC0A1E5CEull + static_cast<uint64_t>(kind), hash32, 32);
    h = mix(h, sig, kind == kSigJobRecoverK1 ? 65 : 64);
    if (kind != kSigJobRecoverK1) h = mix(h, pub64, 64);
    return h;
}
inline uint8_t out_byte(uint64_t h, int field, size_t b) {
    return static_cast<uint8_t>((h >> (8 * (b % 8))) + 131 * b + 17 * static_cast<unsigned>(field));
}
inline uint8_t ok_byte(uint64_t h) { return static_cast<uint8_t>(h >> 63); }

// The "kernel": reads the SoA input and writes the SoA output by the layout table of coalesce_queue.h
//   recover secp256k1: in  hash[32] .. | sig[65] ..          out pub[64] .. | addr[20] .. | ok ..
//   verify SM2:        in  hash[32] .. | r||s||pub[128] ..   out addr[20] .. | ok ..
//   verify secp256k1:  in  pub[64] .. | hash[32] .. | r||s[64] ..   out ok ..
void fake_kernel(int kind, size_t n, const uint8_t* in, uint8_t* out, bool want_pub, bool want_addr) {
    for (size_t i = 0; i < n; ++i) {
        if (kind == kSigJobRecoverK1) {
            const uint64_t h = item_fn(kind, in + 32 * i, in + 32 * n + 65 * i, nullptr);
            for (size_t b = 0; b < 64 && want_pub; ++b) out[64 * i + b] = out_byte(h, 0, b);
            for (size_t b = 0; b < 20 && want_addr; ++b) out[64 * n + 20 * i + b] = out_byte(h, 1, b);
            out[84 * n + i] = ok_byte(h);
        } else if (kind == kSigJobVerifySM2) {
            const uint64_t h = item_fn(kind, in + 32 * i, in + 32 * n + 128 * i, in + 32 * n + 128 * i + 64);
            for (size_t b = 0; b < 20 && want_addr; ++b) out[20 * i + b] = out_byte(h, 1, b);
            out[20 * n + i] = ok_byte(h);
        } else {
            out[i] = ok_byte(item_fn(kind, in + 64 * n + 32 * i, in + 96 * n + 64 * i, in + 64 * i));
        }
    }
}

// stage, "launch", scatter: what run_batch does around its kernel, in buffers of exactly the staged sizes
void run_layout(int kind, std::vector<SigJob*>& batch) {
    size_t n = 0;
    bool want_addr = false, want_pub = false;
    for (SigJob* j : batch) {
        n += j->n;
        want_addr = want_addr || j->out_addr20;
        want_pub = want_pub || j->out_pub64;
    }
    const bool verify = kind != kSigJobRecoverK1;
    const size_t in_bytes = kInPer[kind] * n + (verify ? 4 * n : 0), out_bytes = kOutPer[kind] * n;
    std::unique_ptr<uint8_t[]> in(new uint8_t[in_bytes]), out(new uint8_t[out_bytes]);
    std::memset(in.get(), 0xEE, in_bytes);
    std::memset(out.get(), 0xDD, out_bytes);
    stage_in(kind, batch, n, in.get());
    fake_kernel(kind, n, in.get(), out.get(), want_pub, want_addr);
    scatter_out(kind, batch, n, out.get());
}

std::mutex g_vmu;
std::vector<std::string> g_violations;
std::atomic<long> g_nviolations{0};
void violation(const std::string& s) {
    g_nviolations.fetch_add(1);
    std::lock_guard<std::mutex> g(g_vmu);
    if (g_violations.size() < 16) g_violations.push_back(s);
}
std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char* f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

// One call's arguments and caller-allocated outputs (exact sizes, guard-filled).
struct Call {
    int kind = 0;
    size_t n = 0, stride = 0;
    const uint8_t *hash = nullptr, *sig = nullptr, *pub = nullptr;
    std::unique_ptr<uint8_t[]> out_pub, out_addr, out_ok;
    void alloc_outputs(bool with_pub, bool with_addr) {
        if (with_pub) out_pub.reset(new uint8_t[64 * n]), std::memset(out_pub.get(), kGuard, 64 * n);
        if (with_addr) out_addr.reset(new uint8_t[20 * n]), std::memset(out_addr.get(), kGuard, 20 * n);
        out_ok.reset(new uint8_t[n]);
        std::memset(out_ok.get(), kGuard, n);
    }
    SigJob job() const {
        return sig_job(kind, n, hash, sig, stride, pub, out_pub.get(), out_addr.get(), out_ok.get());
    }
    const uint8_t* key_of(size_t i) const { return pub ? pub + 64 * i : sig + stride * i + 64; }
    // "" or what is wrong with the outputs of a successful call
    std::string check_values(const char* who) const {
        for (size_t i = 0; i < n; ++i) {
            const uint64_t h = item_fn(kind, hash + 32 * i, sig + stride * i, kind == kSigJobRecoverK1 ? nullptr : key_of(i));
            if (out_ok[i] != ok_byte(h)) return fmt("%s: kind %d item %zu of %zu: ok %u, want %u", who, kind, i, n, out_ok[i], ok_byte(h));
            for (size_t b = 0; b < 64 && out_pub; ++b)
                if (out_pub[64 * i + b] != out_byte(h, 0, b)) return fmt("%s: kind %d item %zu of %zu: pub byte %zu", who, kind, i, n, b);
            for (size_t b = 0; b < 20 && out_addr; ++b)
                if (out_addr[20 * i + b] != out_byte(h, 1, b)) return fmt("%s: kind %d item %zu of %zu: addr byte %zu", who, kind, i, n, b);
        }
        return "";
    }
    bool untouched() const {
        for (size_t i = 0; i < n; ++i)
            if (out_ok[i] != kGuard) return false;
        for (size_t i = 0; i < 64 * n && out_pub; ++i)
            if (out_pub[i] != kGuard) return false;
        for (size_t i = 0; i < 20 * n && out_addr; ++i)
            if (out_addr[i] != kGuard) return false;
        return true;
    }
};

// ------------------------------------------------------------------------------------------------ protocol

std::vector<uint8_t> g_pool;  // read-only random bytes every call's inputs point into
std::atomic<int> g_inflight{0}, g_max_inflight{0};
std::atomic<long> g_batches{0}, g_ok_batches{0}, g_ok_items{0}, g_cap_checked{0}, g_big_jobs{0};
// The cap of 2 batches in flight holds for a leader that chose its slot while `callers` was at or above
// BCOSGPU_COALESCE_DEEP; a batch chosen before may still be running.  `callers` itself can only be sampled,
// and a sample can miss a short dip, so the check rests on callers that are certain instead.  The owner of a
// job is inside run_on_queue from before the job's t_enq until after the stand-in batch that holds the job
// has returned (it is notified later still).  A leader chooses its slot at some moment between `chosen_after`
// -- the later of its own call's begin and the newest t_enq of its batch -- and the stand-in's start.  Over
// that whole span the owners of its own batch were inside, and so were the owners of those jobs of the other
// batches still running whose t_enq is not later than chosen_after.  If these number DEEP or more, the leader
// saw DEEP callers or more and its slot must be one of the first two; when that holds for every batch in
// flight, at most two are in flight.  No report can be false; how often the check engages depends on how the
// batches fall.
struct Running {
    bool on = false, held = false;
    std::vector<int64_t> t_enq;
};
std::mutex g_cap_mu;
Running g_running[kMaxSlots];  // under g_cap_mu
thread_local int64_t tl_call_begin = 0;
thread_local std::mt19937_64* tl_rng = nullptr;

int stand_in(int kind, QSlot& slot, std::vector<SigJob*>& batch, std::atomic<uint64_t>* stat) {
    struct Flight {
        int idx;
        explicit Flight(int i) : idx(i) {}
        ~Flight() {
            {
                std::lock_guard<std::mutex> g(g_cap_mu);
                g_running[idx].on = false;
            }
            g_inflight.fetch_sub(1);
        }
    } flight(slot.index);
    const int inflight = g_inflight.fetch_add(1) + 1;
    g_batches.fetch_add(1);
    int seen = g_max_inflight.load();
    while (inflight > seen && !g_max_inflight.compare_exchange_weak(seen, inflight)) {
    }
    if (inflight > slots_in_use()) violation(fmt("%d batches in flight with %d slots", inflight, slots_in_use()));
    if (slot.index >= slots_in_use() || !slot.busy) violation(fmt("slot %d of %d, busy %d", slot.index, slots_in_use(), slot.busy));
    {
        const int cap = std::min(2, slots_in_use()), deep = deep_callers();
        Running mine;
        mine.on = true;
        int64_t chosen_after = tl_call_begin;
        for (SigJob* j : batch) {
            mine.t_enq.push_back(j->t_enq);
            chosen_after = std::max(chosen_after, j->t_enq);
        }
        std::lock_guard<std::mutex> g(g_cap_mu);
        long sure = static_cast<long>(batch.size());
        for (const Running& r : g_running)
            for (size_t k = 0; r.on && k < r.t_enq.size(); ++k) sure += r.t_enq[k] <= chosen_after;
        mine.held = deep > 0 && cap < slots_in_use() && sure >= deep;
        g_running[slot.index] = mine;
        if (mine.held) {
            g_cap_checked.fetch_add(1);
            if (slot.index >= cap) violation(fmt("slot %d taken past the cap of %d", slot.index, cap));
            int running = 0, held = 0;
            for (const Running& r : g_running) running += r.on, held += r.on && r.held;
            if (running > cap && held == running) violation(fmt("%d batches in flight past the cap of %d", running, cap));
        }
    }
    // the batch itself: one kind, arrival order, over kMaxBatch items only alone
    size_t n = 0;
    for (size_t k = 0; k < batch.size(); ++k) {
        n += batch[k]->n;
        if (batch[k]->kind != kind) violation(fmt("a job of kind %d in a batch of kind %d", batch[k]->kind, kind));
        if (k && batch[k]->seq <= batch[k - 1]->seq)
            violation(fmt("batch out of arrival order: seq %" PRIu64 " after %" PRIu64, batch[k]->seq, batch[k - 1]->seq));
    }
    if (batch.empty()) violation("an empty batch");
    if (n > kMaxBatch && batch.size() != 1) violation(fmt("%zu items in a batch of %zu jobs", n, batch.size()));
    std::mt19937_64& rng = *tl_rng;
    std::this_thread::sleep_for(std::chrono::microseconds(20 + rng() % 201));
    const unsigned fate = rng() % 100;
    if (fate == 0) throw std::runtime_error("stand-in exception");
    if (fate == 1) return fail(batch, kStandInRc, "stand-in failure");
    run_layout(kind, batch);
    g_ok_batches.fetch_add(1);
    g_ok_items.fetch_add(static_cast<long>(n));
    stat[kStBatches].fetch_add(1, std::memory_order_relaxed);
    stat[kStItems].fetch_add(n, std::memory_order_relaxed);
    return 0;
}

int protocol(int threads, int calls, uint64_t seed) {
    Queue q;
    constexpr size_t kBig = 65537, kBigSpan = 500, kMaxStride = 200;
    g_pool.resize((kBig + kBigSpan) * kMaxStride + (1u << 20));
    {
        std::mt19937_64 r(seed);
        for (size_t i = 0; i + 8 <= g_pool.size(); i += 8) {
            const uint64_t w = r();
            std::memcpy(&g_pool[i], &w, 8);
        }
    }
    std::atomic<long> done_calls{0}, ok_calls{0}, failed_calls{0}, items_called{0};
    std::vector<std::atomic<int>> in_call(threads);
    for (auto& x : in_call) x.store(-1);
    std::atomic<int> finished{0};
    const int64_t t0 = now_ns();
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t) {
        pool.emplace_back([&, t] {
            std::mt19937_64 rng(seed * 1000003 + static_cast<uint64_t>(t));
            tl_rng = &rng;
            const size_t slack = 1u << 20;
            for (int c = 0; c < calls; ++c) {
                Call call;
                call.kind = static_cast<int>(rng() % kSigJobKinds);
                const unsigned size_draw = rng() % 1000;
                call.n = size_draw < 2 ? kBig + rng() % kBigSpan : size_draw < 100 ? 2 + rng() % 6 : 1;
                if (call.n >= kBig) g_big_jobs.fetch_add(1);
                bool named = false;
                if (call.kind == kSigJobRecoverK1) {
                    call.stride = rng() % 2 ? 65 : 70;
                } else if (call.kind == kSigJobVerifySM2) {
                    const unsigned v = rng() % 3;
                    call.stride = v == 0 ? 128 : v == 1 ? 64 : 200;
                    named = v != 0;
                } else {
                    call.stride = rng() % 2 ? 64 : 65;
                    named = true;
                }
                call.hash = g_pool.data() + rng() % slack;
                call.sig = g_pool.data() + rng() % slack;
                call.pub = named ? g_pool.data() + rng() % slack : nullptr;
                call.alloc_outputs(call.kind == kSigJobRecoverK1 && rng() % 2, call.kind != kSigJobVerifyK1 && rng() % 2);
                SigJob job = call.job();
                in_call[t].store(c);
                tl_call_begin = now_ns();
                const int rc = run_on_queue(q, job, stand_in);
                in_call[t].store(-1);
                items_called.fetch_add(static_cast<long>(call.n));
                if (rc != job.rc) violation(fmt("thread %d call %d: returned %d, job.rc %d", t, c, rc, job.rc));
                if (rc == 0) {
                    ok_calls.fetch_add(1);
                    const std::string bad = call.check_values(fmt("thread %d call %d", t, c).c_str());
                    if (!bad.empty()) violation(bad);
                } else {
                    failed_calls.fetch_add(1);
                    if (job.err.empty()) violation(fmt("thread %d call %d: rc %d without a message", t, c, rc));
                    if (rc != kStandInRc && rc != BCOSGPU_E_HIP) violation(fmt("thread %d call %d: rc %d", t, c, rc));
                    if (!call.untouched()) violation(fmt("thread %d call %d: failed (rc %d) with outputs written", t, c, rc));
                }
                done_calls.fetch_add(1);
            }
            finished.fetch_add(1);
        });
    }
    // the watchdog: every call returns.  No call completing for 10 s is a stranded caller
    long last = -1;
    int64_t last_t = now_ns();
    while (finished.load() < threads) {
        std::this_thread::sleep_for(std::chrono::milliseconds(20));
        const long d = done_calls.load();
        if (d != last) last = d, last_t = now_ns();
        if (now_ns() - last_t > 10000000000ll) {
            std::string who;
            for (int t = 0; t < threads; ++t)
                if (in_call[t].load() >= 0) who += fmt("%s[%d, %d]", who.empty() ? "" : ", ", t, in_call[t].load());
            printf("{\"mode\": \"protocol\", \"stranded\": [%s], \"done_calls\": %ld, \"calls\": %ld}\n", who.c_str(), d,
                   static_cast<long>(threads) * calls);
            fflush(stdout);
            _exit(3);
        }
    }
    for (auto& th : pool) th.join();
    const double dt = (now_ns() - t0) * 1e-9;
    const long total = static_cast<long>(threads) * calls;
    if (ok_calls.load() + failed_calls.load() != total) violation("calls lost");
    if (q.stat[kStJobs].load() != static_cast<uint64_t>(total))
        violation(fmt("kStJobs %" PRIu64 " for %ld calls", q.stat[kStJobs].load(), total));
    if (q.stat[kStItems].load() != static_cast<uint64_t>(g_ok_items.load()))
        violation(fmt("kStItems %" PRIu64 ", successful batches held %ld", q.stat[kStItems].load(), g_ok_items.load()));
    if (q.stat[kStBatches].load() != static_cast<uint64_t>(g_ok_batches.load())) violation("kStBatches differs");
    if (q.callers.load() != 0) violation(fmt("callers %d after the run", q.callers.load()));
    for (auto& p : q.pending)
        if (!p.empty()) violation("jobs left pending");
    if (q.incoming.load() != nullptr) violation("jobs left on the arrival stack");
    std::string v;
    for (auto& s : g_violations) v += (v.empty() ? "\"" : ", \"") + s + "\"";
    printf("{\"mode\": \"protocol\", \"threads\": %d, \"calls\": %ld, \"items\": %ld, \"batches\": %ld, \"ok_batches\": %ld, "
           "\"ok_calls\": %ld, \"failed_calls\": %ld, \"big_jobs\": %ld, \"max_inflight\": %d, \"slots\": %d, \"deep\": %d, "
           "\"lockfree\": %d, \"cap_checked\": %ld, \"stat_jobs\": %" PRIu64 ", \"stat_items\": %" PRIu64 ", \"ok_items\": %ld, "
           "\"nviolations\": %ld, \"violations\": [%s], \"seconds\": %.3f}\n",
           threads, total, items_called.load(), g_batches.load(), g_ok_batches.load(), ok_calls.load(), failed_calls.load(),
           g_big_jobs.load(), g_max_inflight.load(), slots_in_use(), deep_callers(), lockfree_arrivals() ? 1 : 0,
           g_cap_checked.load(), q.stat[kStJobs].load(), q.stat[kStItems].load(), g_ok_items.load(), g_nviolations.load(),
           v.c_str(), dt);
    return g_nviolations.load() == 0 ? 0 : 1;
}

// ------------------------------------------------------------------------------------------------ boundary

// The item limit of a batch, to the item: with one slot (BCOSGPU_COALESCE_SLOTS=1) a first call's batch is held
// inside the stand-in while two more calls of another kind arrive one after the other; released, the first of
// them leads.  kMaxBatch - 1 and 1 items are one batch, kMaxBatch and 1 are two, and a job over kMaxBatch
// runs alone.
std::atomic<bool> g_gate_open{false};
std::mutex g_seen_mu;
std::vector<std::vector<size_t>> g_seen;  // the sizes of the jobs of every batch of kind 1, in order

int gated_stand_in(int kind, QSlot&, std::vector<SigJob*>& batch, std::atomic<uint64_t>* stat) {
    if (kind == kSigJobRecoverK1) {
        while (!g_gate_open.load()) std::this_thread::sleep_for(std::chrono::microseconds(50));
    } else {
        std::lock_guard<std::mutex> g(g_seen_mu);
        g_seen.emplace_back();
        for (SigJob* j : batch) g_seen.back().push_back(j->n);
    }
    run_layout(kind, batch);
    stat[kStBatches].fetch_add(1, std::memory_order_relaxed);
    return 0;
}

int boundary(uint64_t seed) {
    if (slots_in_use() != 1 || !lockfree_arrivals()) {
        fprintf(stderr, "boundary needs BCOSGPU_COALESCE_SLOTS=1 and lock-free arrivals\n");
        return 2;
    }
    g_pool.resize((kMaxBatch + 2) * 128 + 64);
    std::mt19937_64 r(seed);
    for (auto& b : g_pool) b = static_cast<uint8_t>(r());
    const size_t cases[3][2] = {{kMaxBatch - 1, 1}, {kMaxBatch, 1}, {kMaxBatch + 1, 1}};
    std::string got;
    for (auto& sizes : cases) {
        Queue q;
        g_gate_open.store(false);
        g_seen.clear();
        auto make = [&](Call& c, int kind, size_t n) {
            c.kind = kind;
            c.n = n;
            c.stride = kind == kSigJobRecoverK1 ? 65 : 128;
            c.hash = c.sig = g_pool.data();
            c.alloc_outputs(false, true);
        };
        Call first, a, b;
        make(first, kSigJobRecoverK1, 1);
        make(a, kSigJobVerifySM2, sizes[0]);
        make(b, kSigJobVerifySM2, sizes[1]);
        SigJob jf = first.job(), ja = a.job(), jb = b.job();
        auto arrived = [&](SigJob* j) {  // pushed on the arrival stack, every slot busy: its owner sleeps
            const int64_t until = now_ns() + 10000000000ll;
            while (q.incoming.load() != j && now_ns() < until) std::this_thread::sleep_for(std::chrono::microseconds(50));
            return q.incoming.load() == j;
        };
        std::thread tf([&] { run_on_queue(q, jf, gated_stand_in); });
        const int64_t until = now_ns() + 10000000000ll;
        while (q.idle.load() != 0 && now_ns() < until) std::this_thread::sleep_for(std::chrono::microseconds(50));
        std::thread ta([&] { run_on_queue(q, ja, gated_stand_in); });
        const bool a_in = arrived(&ja);
        std::thread tb([&] { run_on_queue(q, jb, gated_stand_in); });
        const bool b_in = arrived(&jb);
        if (!a_in || !b_in || q.idle.load() != 0) violation("boundary: the arrivals were not queued behind the held batch");
        g_gate_open.store(true);
        tf.join();
        ta.join();
        tb.join();
        for (const Call* c : {&first, &a, &b}) {
            const std::string bad = c->check_values("boundary");
            if (!bad.empty()) violation(bad);
        }
        if (jf.rc || ja.rc || jb.rc) violation("boundary: a call failed");
        std::vector<std::vector<size_t>> want;
        if (sizes[0] + sizes[1] <= kMaxBatch) want = {{sizes[0], sizes[1]}};
        else want = {{sizes[0]}, {sizes[1]}};
        if (g_seen != want) violation(fmt("boundary: jobs of %zu and %zu items ran as %zu batch(es), want %zu", sizes[0], sizes[1], g_seen.size(), want.size()));
        got += fmt("%s[%zu, %zu, %zu]", got.empty() ? "" : ", ", sizes[0], sizes[1], g_seen.size());
    }
    std::string v;
    for (auto& s : g_violations) v += (v.empty() ? "\"" : ", \"") + s + "\"";
    printf("{\"mode\": \"boundary\", \"cases\": [%s], \"nviolations\": %ld, \"violations\": [%s]}\n", got.c_str(), g_nviolations.load(),
           v.c_str());
    return g_nviolations.load() == 0 ? 0 : 1;
}

// ------------------------------------------------------------------------------------------------- quiesce

// No arrival is stranded when the queue goes quiet.  With one slot, round after round: one call leads a batch,
// and a second call arrives just as that batch ends -- while the leader frees its slot, publishes q.idle and
// drains the arrivals -- after which nobody else calls.  Either the leader's drain sees the arrival or the
// arrival sees the free slot (see lockfree_arrivals in coalesce_queue.h); a round that does not end within
// 10 s is a stranded call (exit 3).
std::atomic<long> g_batch_ending{0};
thread_local long tl_round = 0;

int ending_stand_in(int kind, QSlot&, std::vector<SigJob*>& batch, std::atomic<uint64_t>* stat) {
    run_layout(kind, batch);
    stat[kStBatches].fetch_add(1, std::memory_order_relaxed);
    g_batch_ending.store(tl_round);
    return 0;
}

int quiesce(long rounds, uint64_t seed) {
    if (slots_in_use() != 1 || !lockfree_arrivals()) {
        fprintf(stderr, "quiesce needs BCOSGPU_COALESCE_SLOTS=1 and lock-free arrivals\n");
        return 2;
    }
    g_pool.resize(4096);
    std::mt19937_64 r(seed);
    for (auto& b : g_pool) b = static_cast<uint8_t>(r());
    Queue q;
    std::atomic<long> go{0}, done[2];
    done[0].store(0);
    done[1].store(0);
    std::atomic<bool> stop{false};
    auto body = [&](int who) {
        std::mt19937_64 rng(seed * 7919 + static_cast<uint64_t>(who));
        for (long round = 1; round <= rounds; ++round) {
            while (go.load() < round)
                if (stop.load()) return;
            tl_round = round;
            Call c;
            c.kind = static_cast<int>(rng() % kSigJobKinds);
            c.n = 1;
            c.stride = 128;
            c.hash = g_pool.data() + rng() % 1024;
            c.sig = g_pool.data() + rng() % 1024;
            c.pub = c.kind == kSigJobRecoverK1 ? nullptr : g_pool.data() + rng() % 1024;
            c.alloc_outputs(c.kind == kSigJobRecoverK1, c.kind != kSigJobVerifyK1);
            SigJob job = c.job();
            if (who == 1) {  // arrive as the first call's batch ends, give or take
                while (g_batch_ending.load() < round) {
                }
                for (volatile unsigned spin = static_cast<unsigned>(rng() % 600); spin > 0; --spin) {
                }
            }
            const int rc = run_on_queue(q, job, ending_stand_in);
            const std::string bad = rc ? fmt("quiesce: round %ld: rc %d", round, rc) : c.check_values("quiesce");
            if (!bad.empty()) violation(bad);
            done[who].store(round);
        }
    };
    std::thread a(body, 0), b(body, 1);
    for (long round = 1; round <= rounds; ++round) {
        go.store(round);
        const int64_t until = now_ns() + 10000000000ll;
        while (done[0].load() < round || done[1].load() < round) {
            if (now_ns() > until) {
                printf("{\"mode\": \"quiesce\", \"stranded\": [%d], \"round\": %ld, \"rounds\": %ld}\n",
                       done[0].load() < round ? 0 : 1, round, rounds);
                fflush(stdout);
                _exit(3);
            }
        }
    }
    a.join();
    b.join();
    if (q.stat[kStJobs].load() != static_cast<uint64_t>(2 * rounds)) violation("quiesce: kStJobs differs");
    std::string v;
    for (auto& s : g_violations) v += (v.empty() ? "\"" : ", \"") + s + "\"";
    printf("{\"mode\": \"quiesce\", \"rounds\": %ld, \"batches\": %" PRIu64 ", \"nviolations\": %ld, \"violations\": [%s]}\n", rounds,
           q.stat[kStBatches].load(), g_nviolations.load(), v.c_str());
    return g_nviolations.load() == 0 ? 0 : 1;
}

// -------------------------------------------------------------------------------------------------- layout

// Inputs of exactly the bytes a job may read: stride * (n - 1) + the item's length.
struct OwnedCall : Call {
    std::unique_ptr<uint8_t[]> hash_mem, sig_mem, pub_mem;
    void make(std::mt19937_64& rng, int kind_, int variant, size_t n_, bool with_pub, bool with_addr) {
        kind = kind_;
        n = n_;
        size_t item = 64;
        bool named = false;
        if (kind == kSigJobRecoverK1) {
            stride = variant % 2 ? 70 : 65;
            item = 65;
        } else if (kind == kSigJobVerifySM2) {
            stride = variant % 3 == 0 ? 128 : variant % 3 == 1 ? 64 : 200;
            named = variant % 3 != 0;
            item = named ? 64 : 128;
        } else {
            stride = variant % 2 ? 65 : 64;
            named = true;
        }
        auto fill = [&](std::unique_ptr<uint8_t[]>& m, size_t len) {
            m.reset(new uint8_t[len]);
            for (size_t i = 0; i < len; ++i) m[i] = static_cast<uint8_t>(rng());
            return m.get();
        };
        hash = fill(hash_mem, 32 * n);
        sig = fill(sig_mem, stride * (n - 1) + item);
        pub = named ? fill(pub_mem, 64 * n) : nullptr;
        alloc_outputs(kind == kSigJobRecoverK1 && with_pub, kind != kSigJobVerifyK1 && with_addr);
    }
};

int layout(uint64_t seed) {
    std::mt19937_64 rng(seed);
    const size_t sizes[] = {1, 2, 63, 64, 65};
    long batches = 0, jobs = 0;
    auto run = [&](int kind, std::vector<std::unique_ptr<OwnedCall>>& calls) {
        std::vector<std::unique_ptr<SigJob>> js;  // (a SigJob holds atomics: it is built in place, never moved)
        std::vector<SigJob*> batch;
        for (auto& c : calls) {
            js.emplace_back(new SigJob(c->job()));
            js.back()->rc = -99;
            batch.push_back(js.back().get());
        }
        run_layout(kind, batch);
        for (size_t k = 0; k < calls.size(); ++k) {
            if (js[k]->rc != 0) violation(fmt("layout: kind %d job %zu: rc %d", kind, k, js[k]->rc));
            const std::string bad = calls[k]->check_values(fmt("layout: job %zu of %zu", k, calls.size()).c_str());
            if (!bad.empty()) violation(bad);
        }
        ++batches;
        jobs += static_cast<long>(calls.size());
    };
    for (int kind = 0; kind < kSigJobKinds; ++kind) {
        const int variants = kind == kSigJobVerifySM2 ? 3 : 2;
        // every variant x size x outputs on its own, then as the first, middle and last job of a mixed batch
        for (int v = 0; v < variants; ++v)
            for (size_t sz : sizes)
                for (int outs = 0; outs < 4; ++outs) {
                    std::vector<std::unique_ptr<OwnedCall>> one;
                    one.emplace_back(new OwnedCall);
                    one[0]->make(rng, kind, v, sz, outs & 1, outs & 2);
                    run(kind, one);
                }
        for (int rep = 0; rep < 400; ++rep) {
            const size_t nj = 1 + rng() % 5;
            std::vector<std::unique_ptr<OwnedCall>> calls;
            for (size_t k = 0; k < nj; ++k) {
                calls.emplace_back(new OwnedCall);
                calls.back()->make(rng, kind, static_cast<int>(rng() % 6), sizes[rng() % 5], rng() % 2, rng() % 2);
            }
            run(kind, calls);
        }
    }
    std::string v;
    for (auto& s : g_violations) v += (v.empty() ? "\"" : ", \"") + s + "\"";
    printf("{\"mode\": \"layout\", \"batches\": %ld, \"jobs\": %ld, \"nviolations\": %ld, \"violations\": [%s]}\n", batches, jobs,
           g_nviolations.load(), v.c_str());
    return g_nviolations.load() == 0 ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 4 && std::string(argv[1]) == "protocol")
        return protocol(atoi(argv[2]), atoi(argv[3]), argc > 4 ? strtoull(argv[4], nullptr, 10) : 1);
    if (argc >= 2 && std::string(argv[1]) == "layout") return layout(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    if (argc >= 3 && std::string(argv[1]) == "quiesce") return quiesce(atol(argv[2]), argc > 3 ? strtoull(argv[3], nullptr, 10) : 1);
    if (argc >= 2 && std::string(argv[1]) == "boundary") return boundary(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    fprintf(stderr, "usage: %s protocol threads calls_per_thread [seed] | boundary [seed] | quiesce rounds [seed] | layout [seed]\n", argv[0]);
    return 2;
}
