// coalesce_queue.h -- the host side of the signature-call coalescer that needs no GPU: the job, the per-device
// queue and its leader / follower protocol, and the layout of a batch's staging buffers.  coalesce.hip
// instantiates the protocol with its HIP slot and run_batch; tests/cpp/coalesce_queue_test.cpp instantiates it
// with a CPU stand-in under ThreadSanitizer and AddressSanitizer.  No HIP header is included here, so a plain
// host compiler builds it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <deque>
#include <exception>
#include <mutex>
#include <string>
#include <vector>
#include <cstdlib>
#include <cstring>
#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>
#include "../../include/bcos_gpu.h"

namespace bcosgpu {

// The host-pointer signature calls as jobs of a per-device queue, coalesced into shared launches (see
// coalesce.hip's file header).  coalesced_run blocks until the job's results are written.
enum SigJobKind { kSigJobRecoverK1 = 0, kSigJobVerifySM2 = 1, kSigJobVerifyK1 = 2, kSigJobKinds = 3 };
struct SigJob {
    int kind = 0;
    size_t n = 0;
    const uint8_t* hash32 = nullptr;  // n x 32
    const uint8_t* sig = nullptr;     // item i at sig + sig_stride * i: r||s||v (recover), r||s[||pub] (verify)
    size_t sig_stride = 0;
    const uint8_t* pub64 = nullptr;   // verify: the known keys (SM2: null = the key is sig[64..128))
    uint8_t* out_pub64 = nullptr;     // recover only, nullable
    uint8_t* out_addr20 = nullptr;    // recover / SM2 verify, nullable
    uint8_t* out_ok = nullptr;        // n bytes: 1 valid, 0 invalid
    int rc = 0;                       // filled in by the engine: 0 or BCOSGPU_E_*, with err
    std::string err;
    bool queued = false, woken = false;  // under the device queue's mutex
    uint64_t seq = 0;                    // arrival order in its device queue
    int64_t t_enq = 0;                   // steady-clock ns: queued (coalescer statistics)
    std::atomic<int64_t> t_notify{0};    // ... last notified
    std::atomic<uint32_t> wake{0};       // the owner's futex word: bit 0 woken to lead, bit 1 done (notify_job)
    SigJob* next = nullptr;              // the device queue's lock-free arrival stack
};
// (an aggregate: the engine's fields keep their defaults)
inline SigJob sig_job(int kind, size_t n, const uint8_t* hash32, const uint8_t* sig, size_t sig_stride,
                      const uint8_t* pub64, uint8_t* out_pub64, uint8_t* out_addr20, uint8_t* out_ok) {
    return SigJob{kind, n, hash32, sig, sig_stride, pub64, out_pub64, out_addr20, out_ok};
}

namespace coalesce {

constexpr int kMaxSlots = 16;
constexpr size_t kMaxBatch = 65536;

// batches in flight per device: 4 (GPU_MAX_HW_QUEUES' default), BCOSGPU_COALESCE_SLOTS = 1..16 to tune
inline int slots_in_use() {
    static const int n = [] {
        const char* e = getenv("BCOSGPU_COALESCE_SLOTS");
        const int v = e ? atoi(e) : 4;
        return v < 1 ? 1 : v > kMaxSlots ? kMaxSlots : v;
    }();
    return n;
}

// How a leader waits for its batch (BCOSGPU_COALESCE_WAIT, read once): 0 hipStreamSynchronize (the
// runtime spins on the completion signal), 1 a blocking-sync event (the thread sleeps until the GPU's
// interrupt), 2 poll the event and yield the CPU between polls, 3 poll the event and sleep ~15 us between
// polls (1 us timer slack on the leader thread), 4 (default) as 3 until 25 us before the batch's expected
// end (a running average of the GPU time of the last batches of its kind, kernel family -- registered-key
// or not -- and size class), then poll without sleeping.
// hipStreamSynchronize and even a blocking-sync event spin on the CPU for a batch's whole ~0.13-0.35 ms
// (one core per batch in flight: a lone caller's process used 1.0 core); mode 4 keeps the spin's latency
// (p50 132.1 vs 132.0 us for one caller) on 0.26 of a core, and 1.6 / 3.9 cores instead of 4.1 / 6.2 at
// 16 / 64 callers -- cores a node's executor and consensus threads get back -- for throughput within
// 2-5 % (tools/callbench_sweep.py, profiles/r06_coalesce_wait_ab.jsonl)
inline int wait_mode() {
    static const int m = [] {
        const char* e = getenv("BCOSGPU_COALESCE_WAIT");
        const int v = e ? atoi(e) : 4;
        return v < 0 || v > 4 ? 4 : v;
    }();
    return m;
}

// Batches in flight: slots_in_use() while fewer than kDeepCallers callers are inside the device's queue,
// 2 beyond (with ~256 submitter threads on the box's 16 cores more concurrent leaders only add host CPU
// -- polling leaders, smaller batches, more wake-ups -- to a process already at its CPU quota:
// tools/callbench_sweep.py, profiles/r06_callbench_slots.jsonl: secp256k1 at 256 threads 245k calls/s
// with 4 slots, 347k with 2; at 16 / 64 threads 4 slots stay ahead, 80k / 266k against 72k / 254k;
// the cap against none on one box, profiles/r06_coalesce_deep_ab.json: 257-273k against 187-219k, p99
// 2 ms against 60 ms).  Measured before the lock-free arrivals below; with them the CPU is no longer the
// bound, the cap is neutral for secp256k1 and still worth ~6 % for SM2's longer batches at 256 threads
// (profiles/r06_coalesce_deep_ab2.json), so it stays.
// BCOSGPU_COALESCE_DEEP = the caller count (default 128; 0 keeps slots_in_use() always), read once.
inline int deep_callers() {
    static const int n = [] {
        const char* e = getenv("BCOSGPU_COALESCE_DEEP");
        return e ? atoi(e) : 128;
    }();
    return n;
}

// A launch slot of a device queue: the protocol's two fields and the runner's payload (coalesce.hip: the
// stream, the event and the staging buffers).
template <class Payload>
struct Slot : Payload {
    int index = 0;
    bool busy = false;
};

// Where a coalesced call's time goes (bcosgpu_coalesce_stats): per device, summed over calls / batches,
// in nanoseconds.  All updated under the queue mutex except the batch phases (one leader each, atomics).
enum CoalesceStat {
    kStBatches = 0,   // batches launched
    kStJobs,          // calls completed
    kStItems,         // signatures
    kStQueueNs,       // per call: enqueue -> its batch taken by a leader
    kStLeadNs,        // per batch: the leader's host work before the launch (staging, key lookup)
    kStGpuNs,         // per batch: first launch -> results synchronised (kernel + copies + queue)
    kStScatterNs,     // per batch: results copied out to the callers
    kStWakeNs,        // per woken follower / leader: notify -> running again (scheduler latency)
    kStWakes,         // wake-ups counted in kStWakeNs
    kStLockNs,        // per call: waiting for the queue mutex on entry
    kStCount
};

template <class Payload>
struct DeviceQueue {
    std::mutex mu;
    std::atomic<int> callers{0};  // callers inside coalesced_run on this device
    // arrivals push their job here without the mutex; whoever holds the mutex moves them to pending
    std::atomic<SigJob*> incoming{nullptr};
    std::atomic<int> idle{0};     // slots free within the current cap (written under mu)
    uint64_t next_seq = 0;
    std::deque<SigJob*> pending[kSigJobKinds];
    Slot<Payload> slots[kMaxSlots];
    std::atomic<uint64_t> stat[kStCount];
    DeviceQueue() {
        for (auto& x : stat) x.store(0, std::memory_order_relaxed);
        idle.store(slots_in_use(), std::memory_order_relaxed);
        for (int k = 0; k < kMaxSlots; ++k) slots[k].index = k;
    }
};

inline int64_t now_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

// Bytes per item of the staged input and output of each job kind (n = the batch's items; verify kinds stage
// the keys' cache slots, int32 per item, after the input: 4 n more bytes).
//   recover secp256k1: in  hash[32] .. | sig[65] ..          out pub[64] .. | addr[20] .. | ok ..
//   verify SM2:        in  hash[32] .. | r||s||pub[128] ..   out addr[20] .. | ok ..
//   verify secp256k1:  in  pub[64] .. | hash[32] .. | r||s[64] ..   out ok ..
constexpr size_t kInPer[kSigJobKinds] = {32 + 65, 32 + 128, 64 + 32 + 64};
constexpr size_t kOutPer[kSigJobKinds] = {64 + 20 + 1, 20 + 1, 1};

// assemble the SoA input of `batch` (all of `kind`, n items in all) at `in`
inline void stage_in(int kind, const std::vector<SigJob*>& batch, size_t n, uint8_t* in) {
    size_t at = 0;
    for (SigJob* j : batch) {
        const size_t m = j->n;
        if (kind == kSigJobRecoverK1) {
            std::memcpy(in + 32 * at, j->hash32, 32 * m);
            uint8_t* s = in + 32 * n + 65 * at;
            if (j->sig_stride == 65) std::memcpy(s, j->sig, 65 * m);
            else for (size_t i = 0; i < m; ++i) std::memcpy(s + 65 * i, j->sig + j->sig_stride * i, 65);
        } else if (kind == kSigJobVerifySM2) {
            std::memcpy(in + 32 * at, j->hash32, 32 * m);
            uint8_t* s = in + 32 * n + 128 * at;
            if (!j->pub64 && j->sig_stride == 128) {
                std::memcpy(s, j->sig, 128 * m);
            } else {
                for (size_t i = 0; i < m; ++i) {
                    std::memcpy(s + 128 * i, j->sig + j->sig_stride * i, 64);
                    std::memcpy(s + 128 * i + 64, j->pub64 ? j->pub64 + 64 * i : j->sig + j->sig_stride * i + 64, 64);
                }
            }
        } else {
            std::memcpy(in + 64 * at, j->pub64, 64 * m);
            std::memcpy(in + 64 * n + 32 * at, j->hash32, 32 * m);
            uint8_t* s = in + 96 * n + 64 * at;
            for (size_t i = 0; i < m; ++i) std::memcpy(s + 64 * i, j->sig + j->sig_stride * i, 64);
        }
        at += m;
    }
}

// copy the SoA output at `out` to the callers' buffers and complete every job of `batch` with rc 0
inline void scatter_out(int kind, const std::vector<SigJob*>& batch, size_t n, const uint8_t* out) {
    size_t at = 0;
    for (SigJob* j : batch) {
        const size_t m = j->n;
        if (kind == kSigJobRecoverK1) {
            if (j->out_pub64) std::memcpy(j->out_pub64, out + 64 * at, 64 * m);
            if (j->out_addr20) std::memcpy(j->out_addr20, out + 64 * n + 20 * at, 20 * m);
            std::memcpy(j->out_ok, out + 84 * n + at, m);
        } else if (kind == kSigJobVerifySM2) {
            if (j->out_addr20) std::memcpy(j->out_addr20, out + 20 * at, 20 * m);
            std::memcpy(j->out_ok, out + 20 * n + at, m);
        } else {
            std::memcpy(j->out_ok, out + at, m);
        }
        j->rc = 0;
        at += m;
    }
}

inline int fail(std::vector<SigJob*>& batch, int rc, const std::string& msg) {
    for (SigJob* j : batch) {
        j->rc = rc;
        j->err = msg;
    }
    return rc;
}

// Wake-ups are targeted, never broadcast: a finished batch wakes its own jobs' owners, and for every
// free slot the owner of the oldest queued job (of any kind) to lead the next batch.  (A broadcast on
// every completion woke all callers -- 256 submitter threads on the box's 16 cores -- per batch: at
// 256 threads secp256k1 single calls fell to 30k/s with a p99 of 87 ms, profiles/r04_bench_first.json.)
// An owner sleeps on its job's own futex word, and a leader marks its batch's jobs done and wakes their
// owners AFTER releasing the device queue's mutex: at 256 callers on 16 cores, notifying ~20 owners under
// that mutex held it ~0.1 ms per batch and every new call queued behind it (tools/callbench_sweep.py,
// profiles/r06_callbench_sweep.json: lock wait 0.17 -> 0.75 ms per call when only the wait moved).  The
// word, not a mutex + condition variable: a notify under the job's mutex woke the owner only for it to
// block again on that mutex (two context switches per wake-up).  The notifier's last access to the job is
// the release fetch_or that publishes the bit (rc, outputs and t_notify are written before it); the
// FUTEX_WAKE after it names only the word's address, so an owner that has already seen the bit and
// returned (its SigJob gone) costs at most a spurious wake-up of whatever waits there later, which every
// futex waiter tolerates.
constexpr uint32_t kSigWake = 1, kSigDone = 2;

inline void futex_wait(std::atomic<uint32_t>& a, uint32_t v) {
    (void)syscall(SYS_futex, reinterpret_cast<uint32_t*>(&a), FUTEX_WAIT_PRIVATE, v, nullptr, nullptr, 0);
}
inline void futex_wake(uint32_t* a) {
    (void)syscall(SYS_futex, a, FUTEX_WAKE_PRIVATE, 1, nullptr, nullptr, 0);
}

inline void notify_job(SigJob* j, bool done, int64_t t) {
    uint32_t* word = reinterpret_cast<uint32_t*>(&j->wake);
    if (!done) j->woken = true;  // (under q.mu: wake_leaders)
    j->t_notify.store(t, std::memory_order_relaxed);
    j->wake.fetch_or(done ? kSigDone : kSigWake, std::memory_order_release);  // last access to *j
    futex_wake(word);
}

template <class Payload>
int slots_now(const DeviceQueue<Payload>& q) {
    const int deep = deep_callers();
    return deep > 0 && q.callers.load(std::memory_order_relaxed) >= deep ? std::min(2, slots_in_use()) : slots_in_use();
}

// Arrivals without the queue mutex (BCOSGPU_COALESCE_LOCKFREE, default 1, read once): a caller pushes its
// job on q.incoming and takes the mutex only when a slot is free (q.idle > 0); otherwise it sleeps at once,
// and every holder of the mutex moves the arrivals to pending first.  No arrival is stranded: a leader
// stores q.idle after freeing its slot and only then drains, while an arrival pushes and only then reads
// q.idle (all sequentially consistent), so either the leader's drain sees the job or the arrival sees the
// free slot and comes to lead.  At 256 submitter threads every arrival used to queue on the mutex (tens of
// us per call under the box's CPU quota, its holders preempted).
inline bool lockfree_arrivals() {
    static const bool v = [] {
        const char* e = getenv("BCOSGPU_COALESCE_LOCKFREE");
        return !(e && e[0] == '0');
    }();
    return v;
}

template <class Payload>
void refresh_idle(DeviceQueue<Payload>& q) {  // under q.mu
    int free_slots = 0;
    for (int k = 0, cap = slots_now(q); k < cap; ++k) free_slots += !q.slots[k].busy;
    q.idle.store(free_slots, std::memory_order_seq_cst);
}

template <class Payload>
void drain(DeviceQueue<Payload>& q) {  // under q.mu: arrivals to pending, in arrival order
    SigJob* h = q.incoming.exchange(nullptr, std::memory_order_seq_cst);
    SigJob* fifo = nullptr;
    while (h) {
        SigJob* n = h->next;
        h->next = fifo;
        fifo = h;
        h = n;
    }
    for (SigJob* j = fifo; j; j = j->next) {
        j->queued = true;
        j->seq = q.next_seq++;
        q.pending[j->kind].push_back(j);
    }
}

template <class Payload>
void wake_leaders(DeviceQueue<Payload>& q) {  // under q.mu
    int free_slots = 0;
    for (int k = 0, cap = slots_now(q); k < cap; ++k) free_slots += !q.slots[k].busy;
    for (int pass = 0; pass < kSigJobKinds && free_slots > 0; ++pass) {
        // the kind whose front job has waited longest first (jobs carry their arrival order)
        SigJob* best = nullptr;
        for (int kd = 0; kd < kSigJobKinds; ++kd) {
            auto& pend = q.pending[kd];
            if (pend.empty() || pend.front()->woken) continue;
            if (!best || pend.front()->seq < best->seq) best = pend.front();
        }
        if (!best) return;
        notify_job(best, false, now_ns());
        --free_slots;
    }
}

// One call on queue `q`: `job` (a valid kind, n > 0) is queued, batched and completed.
// run(kind, slot, batch, q.stat) runs one batch of one kind on a slot this caller holds: it completes every
// job of the batch (rc 0 and the outputs, or fail()) and counts kStBatches / kStItems and the batch phases.
template <class Payload, class Runner>
int run_on_queue(DeviceQueue<Payload>& q, SigJob& job, Runner&& run) {
    struct Inside {
        std::atomic<int>& c;
        explicit Inside(std::atomic<int>& x) : c(x) { c.fetch_add(1, std::memory_order_relaxed); }
        ~Inside() { c.fetch_sub(1, std::memory_order_relaxed); }
    } inside(q.callers);
    job.wake.store(0, std::memory_order_relaxed);
    job.queued = false;
    job.woken = false;
    job.t_notify.store(0, std::memory_order_relaxed);
    job.t_enq = now_ns();
    std::unique_lock<std::mutex> lk(q.mu, std::defer_lock);
    bool sleep_first = false;
    if (lockfree_arrivals()) {
        SigJob* h = q.incoming.load(std::memory_order_relaxed);
        do {
            job.next = h;
        } while (!q.incoming.compare_exchange_weak(h, &job, std::memory_order_seq_cst, std::memory_order_relaxed));
        sleep_first = q.idle.load(std::memory_order_seq_cst) == 0;  // every slot busy: a leader will drain
    }
    if (!sleep_first) {
        const int64_t t_call = now_ns();
        lk.lock();
        q.stat[kStLockNs].fetch_add(static_cast<uint64_t>(now_ns() - t_call), std::memory_order_relaxed);
        if (lockfree_arrivals()) {
            drain(q);
        } else {
            job.queued = true;
            job.seq = q.next_seq++;
            q.pending[job.kind].push_back(&job);
        }
    }
    // A caller leads only while its own job is still queued (a caller whose job is in flight just waits
    // for its batch to finish).
    while (true) {
        Slot<Payload>* free_slot = nullptr;
        if (!sleep_first) {
            if (job.wake.load(std::memory_order_acquire) & kSigDone) return job.rc;  // (lk released on return)
            for (int k = 0, cap = slots_now(q); k < cap; ++k)
                if (!q.slots[k].busy) {
                    free_slot = &q.slots[k];
                    break;
                }
        }
        if (sleep_first || !free_slot || !job.queued) {
            if (!sleep_first) lk.unlock();
            sleep_first = false;
            uint32_t s;
            while (((s = job.wake.load(std::memory_order_acquire)) & (kSigWake | kSigDone)) == 0) futex_wait(job.wake, s);
            const int64_t tn = job.t_notify.exchange(0, std::memory_order_relaxed);
            if (tn) {  // a targeted wake-up: its scheduler latency
                q.stat[kStWakeNs].fetch_add(static_cast<uint64_t>(now_ns() - tn), std::memory_order_relaxed);
                q.stat[kStWakes].fetch_add(1, std::memory_order_relaxed);
            }
            if (s & kSigDone) return job.rc;
            job.wake.fetch_and(~kSigWake, std::memory_order_relaxed);
            lk.lock();
            drain(q);
            job.woken = false;  // (wake_leaders sets it under q.mu)
            continue;
        }
        // lead: take every queued job of this kind, oldest first, up to kMaxBatch items (at least one)
        drain(q);
        auto& pend = q.pending[job.kind];
        std::vector<SigJob*> batch;
        size_t items = 0;
        const int64_t t_take = now_ns();
        while (!pend.empty() && (batch.empty() || items + pend.front()->n <= kMaxBatch)) {
            items += pend.front()->n;
            pend.front()->queued = false;
            q.stat[kStQueueNs].fetch_add(static_cast<uint64_t>(t_take - pend.front()->t_enq), std::memory_order_relaxed);
            batch.push_back(pend.front());
            pend.pop_front();
        }
        free_slot->busy = true;
        refresh_idle(q);
        lk.unlock();
        // a host exception (std::bad_alloc from the staging vectors) fails this batch only: the slot is
        // released and every job of the batch is completed with the error, so no caller waits forever
        try {
            run(job.kind, *free_slot, batch, q.stat);
        } catch (const std::exception& e) {
            fail(batch, BCOSGPU_E_HIP, std::string("signature batch failed on the host: ") + e.what());
        } catch (...) {
            fail(batch, BCOSGPU_E_HIP, "signature batch failed on the host");
        }
        lk.lock();
        free_slot->busy = false;
        refresh_idle(q);  // before the drain (see lockfree_arrivals)
        drain(q);
        wake_leaders(q);
        lk.unlock();
        const int64_t t_done = now_ns();
        bool mine = false;
        for (SigJob* j : batch) {
            if (j == &job) {
                mine = true;
                continue;
            }
            notify_job(j, true, t_done);  // j's owner may return (and j go away) once the bit is set
        }
        q.stat[kStJobs].fetch_add(batch.size(), std::memory_order_relaxed);
        if (mine) return job.rc;
        lk.lock();  // the batch was full before this caller's own job: lead or wait again
        drain(q);
    }
}

}  // namespace coalesce
}  // namespace bcosgpu
