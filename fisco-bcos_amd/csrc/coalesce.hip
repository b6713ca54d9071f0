// coalesce.hip -- per-device coalescing of the host-pointer signature calls.
//
// The reference verifies one signature per call on its hot admission path: TxPool's submitter pool
// (hardware_concurrency threads, TxPool.h:48-49) runs TxValidator::verify -> Transaction::verify ->
// SignatureCrypto::recover once per transaction (TxValidator.cpp:56, Transaction.h:68-82).  A kernel
// launch per call would serialise those threads behind one latency-bound launch each.  Instead every
// host-pointer recover / verify call (single or batched) becomes a job in its device's queue; a caller
// that finds a free launch slot takes EVERY queued job of its kind (up to kMaxBatch items) and runs them
// as one batch -- assemble into pinned staging, one H2D copy, one launch (the same rounds x latency
// kernel choice as the tx path, ecc_txv.hip launch_verify), one D2H copy, synchronise, scatter -- while
// the other callers sleep, each on its own job (see notify_job and lockfree_arrivals in coalesce_queue.h,
// which holds the queue protocol and the staging layout, tested without a GPU).  No dispatcher
// thread: the callers themselves lead batches
// (leader / follower), so nothing runs when nobody calls and nothing needs shutting down.  Up to
// slots_in_use() batches can be in flight per device at once, each on its own stream: small
// latency-bound batches occupy a few CUs each, so they overlap on the device instead of queueing.
#include <string>
#include <vector>
#include <sched.h>
#include <sys/prctl.h>
#include <time.h>
#include "engine.h"

namespace bcosgpu {
namespace {

using namespace coalesce;

struct SlotGpu {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;  // wait modes 1 and 2
    PinnedBuf h_in{true}, h_out{true};  // device-mapped staging (hd: zero-copy small batches)
    DevBuf d_in, d_out;                 // batches past the zero-copy size (64 KiB floor, as the staging)
    SlotGpu() { d_in.min = d_out.min = 65536; }
};
using GpuSlot = Slot<SlotGpu>;
using GpuQueue = DeviceQueue<SlotGpu>;

std::mutex g_qmu;
GpuQueue* g_queues[64] = {};  // never freed: no teardown races with the HIP runtime at exit

GpuQueue* queue_of(int device) {
    std::lock_guard<std::mutex> g(g_qmu);
    if (!g_queues[device]) g_queues[device] = new GpuQueue();
    return g_queues[device];
}

// Batches up to this many items are read and written by the kernel in place, in the mapped staging
// (zero-copy: no copy dispatches, which cost a latency-bound single call ~2 x 20-60 us of queue time);
// larger ones are copied by the DMA engines.
constexpr size_t kZeroCopyMax = 2048;

#define BATCH_HIP(call)                                                                        \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) return fail(batch, BCOSGPU_E_HIP, hip_msg(e_, #call));           \
    } while (0)

// One coalesced launch for `batch` (all of one kind) on `slot` of `device`.
int run_batch(int device, int kind, GpuSlot& slot, std::vector<SigJob*>& batch, std::atomic<uint64_t>* stat) {
    const int64_t t_lead = now_ns();
    int64_t t_launch = 0, t_synced = 0;
    size_t n = 0;
    bool want_addr = false, want_pub = false;
    for (SigJob* j : batch) {
        n += j->n;
        want_addr = want_addr || j->out_addr20;
        want_pub = want_pub || j->out_pub64;
    }
    DeviceScope select_device(device);
    BATCH_HIP(select_device.err);
    if (!slot.stream) {
        // Streams of one priority share a few hardware queues (GPU_MAX_HW_QUEUES), and kernels on one
        // queue run in order, so slot k takes priority level k mod levels: each level brings its own
        // queues and the batches in flight really overlap (BCOSGPU_COALESCE_PRIO=0: all at the default).
        static const bool prio = !getenv("BCOSGPU_COALESCE_PRIO") || atoi(getenv("BCOSGPU_COALESCE_PRIO")) != 0;
        int least = 0, greatest = 0;
        if (prio) BATCH_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        const int levels = least >= greatest ? least - greatest + 1 : 1;
        BATCH_HIP(hipStreamCreateWithPriority(&slot.stream, hipStreamNonBlocking, least - slot.index % levels));
    }
    if (!slot.done && wait_mode() != 0)
        BATCH_HIP(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming |
                                                          (wait_mode() == 1 ? hipEventBlockingSync : 0u)));
    // verify kinds stage the keys' cache slots (int32 per item) after the input (registered-key path)
    const bool verify = kind == kSigJobVerifyK1 || kind == kSigJobVerifySM2;
    const size_t slots_at = kInPer[kind] * n;
    const size_t in_bytes = slots_at + (verify ? 4 * n : 0), out_bytes = kOutPer[kind] * n;
    BATCH_HIP(slot.h_in.ensure(in_bytes));
    BATCH_HIP(slot.h_out.ensure(out_bytes));
    static const size_t zero_copy_max = [] {
        const char* e = getenv("BCOSGPU_COALESCE_ZEROCOPY");  // items; tuning
        return e ? static_cast<size_t>(atol(e)) : kZeroCopyMax;
    }();
    const bool zero_copy = n <= zero_copy_max;
    if (!zero_copy) {
        BATCH_HIP(slot.d_in.ensure(in_bytes + 16));
        BATCH_HIP(slot.d_out.ensure(out_bytes + 16));
    }
    // assemble the SoA input
    uint8_t* in = slot.h_in.as<uint8_t>();
    stage_in(kind, batch, n, in);
    // every key of the batch registered (or promoted now): the registered-key kernel (ecc_keyed.hip)
    bool keyed = false;
    uint64_t gen = 0;
    const int vsuite = kind == kSigJobVerifySM2 ? BCOSGPU_SUITE_SM2 : BCOSGPU_SUITE_SECP256K1;
    if (verify) {
        const uint8_t* pubs = kind == kSigJobVerifySM2 ? in + 32 * n + 64 : in;
        // only calls that name their keys (SignatureCrypto::verify: the sealer path) promote keys; SM2 recover
        // (admission: the key is the sender's, embedded in the signature) only looks them up
        bool named = true;
        for (SigJob* j : batch) named = named && (kind == kSigJobVerifyK1 || j->pub64 != nullptr);
        const int krc = keyed_lookup(vsuite, pubs, kind == kSigJobVerifySM2 ? 128 : 64, n,
                                     reinterpret_cast<int32_t*>(in + slots_at), named, &keyed, &gen);
        if (krc) keyed = false;  // a failed table build leaves the generic path
    }
    // the slot goes back to the queue with its stream idle, whatever way the batch ends
    StreamDrain drain(slot.stream);
    if (!zero_copy) BATCH_HIP(hipMemcpyAsync(slot.d_in.p, in, in_bytes, hipMemcpyHostToDevice, slot.stream));
    const uint8_t* di = static_cast<const uint8_t*>(zero_copy ? slot.h_in.hd : slot.d_in.p);
    uint8_t* dout = static_cast<uint8_t*>(zero_copy ? slot.h_out.hd : slot.d_out.p);
    t_launch = now_ns();
    for (int attempt = 0; attempt < 2; ++attempt) {
        int rc;
        if (keyed && kind == kSigJobVerifySM2)
            rc = launch_sig_verify_keyed(BCOSGPU_SUITE_SM2, reinterpret_cast<const int32_t*>(di + slots_at), di,
                                         di + 32 * n, 128, n, dout + 20 * n, want_addr ? dout : nullptr, slot.stream);
        else if (keyed)
            rc = launch_sig_verify_keyed(BCOSGPU_SUITE_SECP256K1, reinterpret_cast<const int32_t*>(di + slots_at),
                                         di + 64 * n, di + 96 * n, 64, n, dout, nullptr, slot.stream);
        else if (kind == kSigJobRecoverK1)
            rc = launch_secp256k1_recover(di, di + 32 * n, 65, n, want_pub ? dout : nullptr,
                                          want_addr ? dout + 64 * n : nullptr, dout + 84 * n, slot.stream);
        else if (kind == kSigJobVerifySM2)
            rc = launch_sm2_verify(di, di + 32 * n, 128, n, want_addr ? dout : nullptr, dout + 20 * n, slot.stream);
        else
            rc = launch_sig_verify(BCOSGPU_SUITE_SECP256K1, di, di + 64 * n, di + 96 * n, 64, n, dout, slot.stream);
        if (rc) {
            hipError_t e = hipGetLastError();
            return fail(batch, rc, std::string("signature batch launch failed: ") + hipGetErrorString(e));
        }
        if (!zero_copy)
            BATCH_HIP(hipMemcpyAsync(slot.h_out.p, slot.d_out.p, out_bytes, hipMemcpyDeviceToHost, slot.stream));
        if (wait_mode() == 0) {
            BATCH_HIP(hipStreamSynchronize(slot.stream));
        } else {
            BATCH_HIP(hipEventRecord(slot.done, slot.stream));
            if (wait_mode() == 1) {
                BATCH_HIP(hipEventSynchronize(slot.done));
            } else {
                static thread_local bool slack = false;
                if (wait_mode() >= 3 && !slack) {
                    (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0);
                    slack = true;
                }
                // running average GPU time per (kind, registered-key kernel or not, batch size by powers of 2)
                static std::atomic<int64_t> expect[kSigJobKinds][2][18];
                int lg = 0;
                while (lg < 17 && (size_t{1} << (lg + 1)) <= n) ++lg;
                std::atomic<int64_t>& expect_ns = expect[kind][keyed ? 1 : 0][lg];
                const int64_t sleep_until = wait_mode() == 4 ? t_launch + expect_ns.load(std::memory_order_relaxed) - 25000
                                                             : INT64_MAX;
                const timespec nap{0, 15000};
                hipError_t qe;
                while ((qe = hipEventQuery(slot.done)) == hipErrorNotReady) {
                    if (wait_mode() == 2) sched_yield();
                    else if (now_ns() < sleep_until) nanosleep(&nap, nullptr);
                }
                BATCH_HIP(qe);
                if (wait_mode() == 4) {
                    const int64_t took = now_ns() - t_launch, e = expect_ns.load(std::memory_order_relaxed);
                    expect_ns.store(e == 0 ? took : e + (took - e) / 8, std::memory_order_relaxed);
                }
            }
        }
        // the key cache was cleared (bcosgpu_clear_keys) between the lookup and the launch: its slots may
        // have been rebuilt for other keys meanwhile, so this batch runs again on the generic kernels
        if (!keyed || keyed_generation(vsuite) == gen) break;
        keyed = false;
    }
    drain.dismiss();
    t_synced = now_ns();
    // scatter
    scatter_out(kind, batch, n, slot.h_out.as<uint8_t>());
    stat[kStBatches].fetch_add(1, std::memory_order_relaxed);
    stat[kStItems].fetch_add(n, std::memory_order_relaxed);
    stat[kStLeadNs].fetch_add(static_cast<uint64_t>(t_launch - t_lead), std::memory_order_relaxed);
    stat[kStGpuNs].fetch_add(static_cast<uint64_t>(t_synced - t_launch), std::memory_order_relaxed);
    stat[kStScatterNs].fetch_add(static_cast<uint64_t>(now_ns() - t_synced), std::memory_order_relaxed);
    return 0;
}

}  // namespace

// The queue protocol (arrivals, leaders and followers, wake-ups) is coalesce_queue.h's run_on_queue.
int coalesced_run(int device, SigJob& job) {
    if (device < 0 || device >= 64 || job.kind < 0 || job.kind >= kSigJobKinds) {
        job.err = "bad device or job kind";
        return job.rc = BCOSGPU_E_ARG;
    }
    if (job.n == 0) return job.rc = 0;
    GpuQueue& q = *queue_of(device);
    return run_on_queue(q, job, [device](int kind, GpuSlot& slot, std::vector<SigJob*>& batch, std::atomic<uint64_t>* stat) {
        return run_batch(device, kind, slot, batch, stat);
    });
}

int coalesce_stats(int device, uint64_t* out, int n, int reset) {
    if (device < 0 || device >= 64 || !out) return BCOSGPU_E_ARG;
    GpuQueue& q = *queue_of(device);
    for (int k = 0; k < kStCount; ++k) {
        const uint64_t v = reset ? q.stat[k].exchange(0, std::memory_order_relaxed) : q.stat[k].load(std::memory_order_relaxed);
        if (k < n) out[k] = v;
    }
    return 0;
}

}  // namespace bcosgpu
