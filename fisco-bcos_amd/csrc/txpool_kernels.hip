// txpool_kernels.hip -- transaction admission against the pool's own state, resident in HBM across calls
// (DESIGN.md 6e): the __global__ wrappers of the bodies in sorted_set.h and txpool_admit.h, the launch chains,
// the pool object with its growth, and the bcosgpu_txpool_* C ABI.  The five rules of sorted_set.h hold for every
// kernel here; the wrappers add nothing but the thread index.
//
// A pool owns three sorted key sets (hashes: m_txsTable's keys; nonces: TxPoolNonceChecker's; ledger:
// LedgerNonceChecker's), host copies of the per-block nonce lists (LedgerNonceChecker::m_blockNonceCache), the
// chain id, group id, block_limit_range and the current block number, one stream and one mutex.  Every call is a
// short chain of kernels on that stream and ends with one synchronisation that reads the error word and the true
// counts (which become the host's bounds).  Sets and scratch grow on the host only, with the stream drained.
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include "engine.h"
#include "tars_decode.h"
#include "txpool_admit.h"

namespace bcosgpu {
namespace txpool {

using sset::Rec;
using sset::SetView;

static_assert(admit::kFieldChain == tars::F_CHAIN && admit::kFieldGroup == tars::F_GROUP &&
                  admit::kFieldNonce == tars::F_NONCE,
              "txpool_admit.h reads TxFields by tars_decode.h's indices");
static_assert(admit::kModeFull == BCOSGPU_TXPOOL_FULL && admit::kModeProposal == BCOSGPU_TXPOOL_PROPOSAL, "modes");

#define TP_TID (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x)

__global__ __launch_bounds__(256) void txpool_records_kernel(uint32_t n, const uint8_t* keys, Rec* recs, uint32_t cap,
                                                             uint32_t* err) {
    sset::records_body(TP_TID, n, keys, recs, cap, err);
}
__global__ __launch_bounds__(256) void txpool_union_flag_kernel(uint32_t m, const Rec* recs, SetView a, uint32_t* flag,
                                                                uint32_t cap, uint32_t* err) {
    sset::union_flag_body(TP_TID, m, recs, a, flag, cap, err);
}
__global__ __launch_bounds__(256) void txpool_compact_kernel(uint32_t m, const Rec* recs, const uint32_t* flag,
                                                             const uint32_t* pos, uint8_t* out, uint32_t cap,
                                                             uint32_t* out_count, uint32_t* err) {
    sset::compact_body(TP_TID, m, recs, flag, pos, out, cap, out_count, err);
}
__global__ __launch_bounds__(256) void txpool_merge_kernel(uint32_t bound_a, uint32_t m, SetView a, SetView b,
                                                           uint8_t* dst, uint32_t cap, uint32_t* dst_count,
                                                           uint32_t* err) {
    sset::merge_body(TP_TID, bound_a, m, a, b, dst, cap, dst_count, err);
}
__global__ __launch_bounds__(256) void txpool_diff_keep_kernel(uint32_t bound_a, SetView a, const Rec* recs, uint32_t m,
                                                               uint32_t* keep, uint32_t cap, uint32_t* err) {
    sset::diff_keep_body(TP_TID, bound_a, a, recs, m, keep, cap, err);
}
__global__ __launch_bounds__(256) void txpool_diff_scatter_kernel(uint32_t bound_a, SetView a, const uint32_t* keep,
                                                                  const uint32_t* pos, uint8_t* dst, uint32_t cap,
                                                                  uint32_t* dst_count, uint32_t* err) {
    sset::diff_scatter_body(TP_TID, bound_a, a, keep, pos, dst, cap, dst_count, err);
}
__global__ __launch_bounds__(256) void txpool_verdict_kernel(uint32_t n, int mode, const uint8_t* enc, uint64_t enc_bytes,
                                                             const tars::TxFields* fields, const uint8_t* vstatus,
                                                             uint8_t* txhash, SetView hashes, SetView nonces,
                                                             SetView ledger, admit::PoolParams pp, uint32_t* status,
                                                             uint8_t* nonce_out, Rec* recs, uint32_t cap, uint32_t* err) {
    admit::verdict_body(TP_TID, n, mode, enc, enc_bytes, fields, vstatus, txhash, hashes, nonces, ledger, pp, status,
                        nonce_out, recs, cap, err);
}
__global__ __launch_bounds__(256) void txpool_run_ok_kernel(uint32_t n, const Rec* recs, const uint32_t* status,
                                                            uint32_t* ok, uint32_t cap, uint32_t* err) {
    admit::run_ok_body(TP_TID, n, recs, status, ok, cap, err);
}
__global__ __launch_bounds__(256) void txpool_run_rule_kernel(uint32_t n, const Rec* recs, const uint32_t* ok,
                                                              const uint32_t* c, const uint8_t* txhash, uint32_t* status,
                                                              uint32_t* win, uint32_t cap, uint32_t* err) {
    admit::run_rule_body(TP_TID, n, recs, ok, c, txhash, status, win, cap, err);
}
__global__ __launch_bounds__(256) void txpool_finalize_kernel(uint32_t n, const uint32_t* status, const uint8_t* txhash,
                                                              uint8_t* sender, Rec* recs, uint32_t cap, uint32_t* err) {
    admit::finalize_body(TP_TID, n, status, txhash, sender, recs, cap, err);
}

inline dim3 grid_of(uint64_t threads) { return dim3(static_cast<unsigned>((threads + 255) / 256)); }

constexpr uint32_t kMaxKeys = 0x7fffffffu;  // counts, indices and capacities are uint32 on the device
constexpr int kHashes = BCOSGPU_TXPOOL_HASHES, kNonces = BCOSGPU_TXPOOL_NONCES, kLedger = BCOSGPU_TXPOOL_LEDGER;
// the pool's device words: the error word, the count of the compacted batch B', the counts of set s's buffer b
constexpr int kMetaErr = 0, kMetaB = 1, kMetaWords = 8;
constexpr int meta_count(int s, int b) { return 2 + 2 * s + b; }

struct DevSet {
    uint8_t* buf[2] = {nullptr, nullptr};
    int cur = 0;
    uint32_t cap = 0;
    uint32_t bound = 0;  // rule 5: never below the true count
};

struct Pool {
    std::mutex mu;
    int dev = 0, suite = 0;
    hipStream_t st = nullptr;
    std::string chain, group;
    uint8_t* d_ids = nullptr;  // chain | group
    int64_t range = 0, number = 0;
    DevSet sets[3];
    uint32_t* d_meta = nullptr;
    uint32_t h_meta[kMetaWords] = {};
    bool broken = false;                               // an engine error was reported: the sets are not to be trusted
    std::map<int64_t, std::vector<uint8_t>> blocks;   // number -> its nonces, 32 bytes each
    // scratch (contents live within one chain): batch keys, records, flags, their scan, B', ok, its scan, library temp
    DevBuf keys_in, recs, flag, pos, bprime, okv, cscan, temp;
    // admit: the decode + verify buffers, and for the host call the inputs and outputs
    DevBuf pre, offs, sig, work, vstatus, enc, enc_off, out;

    SetView view(int s) const {
        return SetView{sets[s].buf[sets[s].cur], d_meta + meta_count(s, sets[s].cur), sets[s].cap};
    }
};

#define TP_HIP(call)                                                                          \
    do {                                                                                      \
        const hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) return api_set_err(BCOSGPU_E_HIP, hip_msg(e_, #call));          \
    } while (0)

// scratch grows with the stream drained (a growth frees the old buffer)
static int ensure(Pool& p, DevBuf& b, uint64_t bytes) {
    if (bytes <= b.cap) return 0;
    TP_HIP(hipStreamSynchronize(p.st));
    TP_HIP(b.ensure(bytes));
    return 0;
}

static size_t sort_temp_bytes(uint32_t m) {
    size_t t = 0;
    (void)hipcub::DeviceMergeSort::SortKeys(nullptr, t, static_cast<Rec*>(nullptr), static_cast<int>(m), sset::RecLess());
    return t;
}
static size_t scan_temp_bytes(uint32_t m) {
    size_t t = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t, static_cast<const uint32_t*>(nullptr),
                                           static_cast<uint32_t*>(nullptr), static_cast<int>(m));
    return t;
}

// scratch for a chain over a batch of m records and flag arrays of up to `flags` entries
static int ensure_scratch(Pool& p, uint32_t m, uint32_t flags) {
    flags = std::max(flags, m);
    const uint32_t big = std::max(flags, 1u);
    if (int rc = ensure(p, p.recs, static_cast<uint64_t>(m) * sizeof(Rec))) return rc;
    if (int rc = ensure(p, p.bprime, static_cast<uint64_t>(m) * 32)) return rc;
    if (int rc = ensure(p, p.flag, static_cast<uint64_t>(flags) * 4)) return rc;
    if (int rc = ensure(p, p.pos, static_cast<uint64_t>(flags) * 4)) return rc;
    return ensure(p, p.temp, std::max(sort_temp_bytes(std::max(m, 1u)), scan_temp_bytes(big)) + 256);
}

// rule 5: room for `incoming` more keys in set s, or both buffers anew (at least doubled) with the keys copied
static int reserve(Pool& p, int s, uint64_t incoming) {
    DevSet& d = p.sets[s];
    const uint64_t need = static_cast<uint64_t>(d.bound) + incoming;
    if (need <= d.cap) return 0;
    if (need > kMaxKeys) return api_set_err(BCOSGPU_E_ARG, "a key set would exceed 2^31 - 1 keys");
    const uint32_t want = static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>(2ull * d.cap, need), kMaxKeys));
    TP_HIP(hipStreamSynchronize(p.st));
    uint8_t *a = nullptr, *b = nullptr;
    TP_HIP(hipMalloc(&a, static_cast<size_t>(want) * 32));
    if (const hipError_t e = hipMalloc(&b, static_cast<size_t>(want) * 32); e != hipSuccess) {
        (void)hipFree(a);
        return api_set_err(BCOSGPU_E_HIP, hip_msg(e, "hipMalloc (key set)"));
    }
    hipError_t e = hipMemcpyAsync(a, d.buf[d.cur], static_cast<size_t>(d.bound) * 32, hipMemcpyDeviceToDevice, p.st);
    if (e == hipSuccess && d.cur != 0)
        e = hipMemcpyAsync(p.d_meta + meta_count(s, 0), p.d_meta + meta_count(s, 1), 4, hipMemcpyDeviceToDevice, p.st);
    if (e == hipSuccess) e = hipStreamSynchronize(p.st);
    if (e != hipSuccess) {
        (void)hipFree(a);
        (void)hipFree(b);
        return api_set_err(BCOSGPU_E_HIP, hip_msg(e, "key set growth"));
    }
    (void)hipFree(d.buf[0]);
    (void)hipFree(d.buf[1]);
    d.buf[0] = a;
    d.buf[1] = b;
    d.cur = 0;
    d.cap = want;
    return 0;
}

static int sort_recs(Pool& p, uint32_t m) {
    size_t t = p.temp.cap;
    TP_HIP(hipcub::DeviceMergeSort::SortKeys(p.temp.p, t, p.recs.as<Rec>(), static_cast<int>(m), sset::RecLess(), p.st));
    return 0;
}
static int scan(Pool& p, const uint32_t* in, uint32_t* out, uint32_t m) {
    size_t t = p.temp.cap;
    TP_HIP(hipcub::DeviceScan::ExclusiveSum(p.temp.p, t, in, out, static_cast<int>(m), p.st));
    return 0;
}

// The union's chain behind the sort: p.recs holds m sorted records; flags by union_flag_body, or `given` (the
// winners of run_rule_body).  The caller reserved room and scratch.
static int union_tail(Pool& p, int s, uint32_t m, const uint32_t* given) {
    DevSet& d = p.sets[s];
    uint32_t* err = p.d_meta + kMetaErr;
    const Rec* recs = p.recs.as<Rec>();
    const uint32_t* flag = given;
    if (!given) {
        hipLaunchKernelGGL(txpool_union_flag_kernel, grid_of(m), dim3(256), 0, p.st, m, recs, p.view(s),
                           p.flag.as<uint32_t>(), m, err);
        flag = p.flag.as<uint32_t>();
    }
    if (int rc = scan(p, flag, p.pos.as<uint32_t>(), m)) return rc;
    hipLaunchKernelGGL(txpool_compact_kernel, grid_of(m), dim3(256), 0, p.st, m, recs, flag, p.pos.as<uint32_t>(),
                       p.bprime.as<uint8_t>(), m, p.d_meta + kMetaB, err);
    const SetView b{p.bprime.as<uint8_t>(), p.d_meta + kMetaB, m};
    const int o = 1 - d.cur;
    hipLaunchKernelGGL(txpool_merge_kernel, grid_of(static_cast<uint64_t>(d.bound) + m), dim3(256), 0, p.st, d.bound, m,
                       p.view(s), b, d.buf[o], d.cap, p.d_meta + meta_count(s, o), err);
    TP_HIP(hipGetLastError());
    d.cur = o;
    d.bound += m;
    return 0;
}

// m host keys into the records, sorted
static int sorted_records(Pool& p, const uint8_t* keys, uint32_t m) {
    if (int rc = ensure(p, p.keys_in, static_cast<uint64_t>(m) * 32)) return rc;
    TP_HIP(hipMemcpyAsync(p.keys_in.p, keys, static_cast<size_t>(m) * 32, hipMemcpyHostToDevice, p.st));
    hipLaunchKernelGGL(txpool_records_kernel, grid_of(m), dim3(256), 0, p.st, m, p.keys_in.as<uint8_t>(), p.recs.as<Rec>(),
                       m, p.d_meta + kMetaErr);
    return sort_recs(p, m);
}

static int set_union(Pool& p, int s, const uint8_t* keys, uint64_t m64) {
    if (m64 == 0) return 0;
    if (m64 > kMaxKeys) return api_set_err(BCOSGPU_E_ARG, "batch too large");
    const uint32_t m = static_cast<uint32_t>(m64);
    if (int rc = reserve(p, s, m)) return rc;
    if (int rc = ensure_scratch(p, m, m)) return rc;
    if (int rc = sorted_records(p, keys, m)) return rc;
    return union_tail(p, s, m, nullptr);
}

static int set_difference(Pool& p, int s, const uint8_t* keys, uint64_t m64) {
    DevSet& d = p.sets[s];
    if (m64 == 0 || d.bound == 0) return 0;  // (a bound of 0 is an empty set)
    if (m64 > kMaxKeys) return api_set_err(BCOSGPU_E_ARG, "batch too large");
    const uint32_t m = static_cast<uint32_t>(m64), na = d.bound;
    if (int rc = ensure_scratch(p, m, na)) return rc;
    if (int rc = sorted_records(p, keys, m)) return rc;
    uint32_t* err = p.d_meta + kMetaErr;
    hipLaunchKernelGGL(txpool_diff_keep_kernel, grid_of(na), dim3(256), 0, p.st, na, p.view(s), p.recs.as<Rec>(), m,
                       p.flag.as<uint32_t>(), na, err);
    if (int rc = scan(p, p.flag.as<uint32_t>(), p.pos.as<uint32_t>(), na)) return rc;
    const int o = 1 - d.cur;
    hipLaunchKernelGGL(txpool_diff_scatter_kernel, grid_of(na), dim3(256), 0, p.st, na, p.view(s), p.flag.as<uint32_t>(),
                       p.pos.as<uint32_t>(), d.buf[o], d.cap, p.d_meta + meta_count(s, o), err);
    TP_HIP(hipGetLastError());
    d.cur = o;  // (the bound stays)
    return 0;
}

// the one synchronisation that ends a call: the error word, and the true counts as the new bounds
static int end_call(Pool& p, StreamDrain& drain) {
    TP_HIP(hipMemcpyAsync(p.h_meta, p.d_meta, sizeof(p.h_meta), hipMemcpyDeviceToHost, p.st));
    TP_HIP(hipStreamSynchronize(p.st));
    drain.dismiss();
    if (p.h_meta[kMetaErr]) {
        p.broken = true;
        return api_set_err(BCOSGPU_E_ENGINE, "txpool: a kernel refused a store or a count (error word " +
                                                 std::to_string(p.h_meta[kMetaErr]) + "); the pool must be rebuilt");
    }
    for (int s = 0; s < 3; ++s) p.sets[s].bound = p.h_meta[meta_count(s, p.sets[s].cur)];
    return 0;
}

// the admission chain on device buffers (all outputs n entries); nothing is synchronised here
static int admit_chain(Pool& p, int mode, const uint8_t* d_enc, const uint64_t* d_enc_off, uint32_t n, uint64_t enc_bytes,
                       uint8_t* d_txhash, uint8_t* d_sender, uint8_t* d_nonce, uint32_t* d_status) {
    if (mode == admit::kModeFull)
        if (int rc = reserve(p, kNonces, n)) return rc;
    if (int rc = reserve(p, kHashes, n)) return rc;
    if (int rc = ensure_scratch(p, n, n)) return rc;
    const uint64_t work = tars_decode_work_bytes(n);
    if (int rc = ensure(p, p.pre, enc_bytes + 12ull * n + 8)) return rc;
    if (int rc = ensure(p, p.offs, 2ull * (n + 1ull) * 8)) return rc;
    if (int rc = ensure(p, p.sig, enc_bytes + 8)) return rc;
    if (int rc = ensure(p, p.work, work)) return rc;
    if (int rc = ensure(p, p.vstatus, n)) return rc;
    if (int rc = ensure(p, p.okv, 4ull * n)) return rc;
    if (int rc = ensure(p, p.cscan, 4ull * n)) return rc;
    uint64_t* pre_off = p.offs.as<uint64_t>();
    // the existing decode + verify, unchanged: check_sig on, check_hash off; TxFields stay at the head of the work buffer
    if (int rc = bcosgpu_tars_tx_verify_batch_dev(p.suite, d_enc, d_enc_off, n, 1, 0, p.pre.as<uint8_t>(), pre_off,
                                                  p.sig.as<uint8_t>(), pre_off + (n + 1), p.work.p, work, d_txhash,
                                                  d_sender, p.vstatus.as<uint8_t>(), p.st))
        return rc;
    const tars::TxFields* fields = p.work.as<tars::TxFields>();
    uint32_t* err = p.d_meta + kMetaErr;
    Rec* recs = p.recs.as<Rec>();
    const admit::PoolParams pp{p.d_ids, p.d_ids + p.chain.size(), static_cast<uint32_t>(p.chain.size()),
                               static_cast<uint32_t>(p.group.size()), p.number, p.range};
    hipLaunchKernelGGL(txpool_verdict_kernel, grid_of(n), dim3(256), 0, p.st, n, mode, d_enc, enc_bytes, fields,
                       p.vstatus.as<uint8_t>(), d_txhash, p.view(kHashes), p.view(kNonces), p.view(kLedger), pp, d_status,
                       d_nonce, recs, n, err);
    if (mode == admit::kModeFull) {
        if (int rc = sort_recs(p, n)) return rc;
        hipLaunchKernelGGL(txpool_run_ok_kernel, grid_of(n), dim3(256), 0, p.st, n, recs, d_status, p.okv.as<uint32_t>(), n,
                           err);
        if (int rc = scan(p, p.okv.as<uint32_t>(), p.cscan.as<uint32_t>(), n)) return rc;
        hipLaunchKernelGGL(txpool_run_rule_kernel, grid_of(n), dim3(256), 0, p.st, n, recs, p.okv.as<uint32_t>(),
                           p.cscan.as<uint32_t>(), d_txhash, d_status, p.flag.as<uint32_t>(), n, err);
        if (int rc = union_tail(p, kNonces, n, p.flag.as<uint32_t>())) return rc;  // the winners' nonces
    }
    hipLaunchKernelGGL(txpool_finalize_kernel, grid_of(n), dim3(256), 0, p.st, n, d_status, d_txhash, d_sender, recs, n, err);
    if (int rc = sort_recs(p, n)) return rc;
    return union_tail(p, kHashes, n, nullptr);  // the accepted hashes
}

static void destroy(Pool* p) {
    if (!p) return;
    DeviceScope scope(p->dev);
    if (p->st) (void)hipStreamSynchronize(p->st);
    for (DevSet& d : p->sets)
        for (uint8_t* b : d.buf)
            if (b) (void)hipFree(b);
    for (DevBuf* b : {&p->keys_in, &p->recs, &p->flag, &p->pos, &p->bprime, &p->okv, &p->cscan, &p->temp, &p->pre, &p->offs,
                      &p->sig, &p->work, &p->vstatus, &p->enc, &p->enc_off, &p->out})
        if (b->p) (void)hipFree(b->p);
    if (p->d_ids) (void)hipFree(p->d_ids);
    if (p->d_meta) (void)hipFree(p->d_meta);
    if (p->st) (void)hipStreamDestroy(p->st);
    delete p;
}

}  // namespace txpool
}  // namespace bcosgpu

using namespace bcosgpu;
using namespace bcosgpu::txpool;

struct bcosgpu_txpool : Pool {};

// the head of every call on a live pool: the lock, the pool's device, the sticky engine error
#define TP_ENTER(h)                                                                                      \
    if (!(h)) return api_set_err(BCOSGPU_E_ARG, "null pool");                                            \
    Pool& p = *(h);                                                                                      \
    std::lock_guard<std::mutex> lock(p.mu);                                                              \
    DeviceScope scope(p.dev);                                                                            \
    if (scope.err != hipSuccess) return api_set_err(BCOSGPU_E_HIP, hip_msg(scope.err, "hipSetDevice")); \
    if (p.broken) return api_set_err(BCOSGPU_E_ENGINE, "txpool: the pool reported an engine error earlier")

extern "C" {

int bcosgpu_txpool_create(int device, int suite, const char* chain_id, size_t chain_len, const char* group_id,
                          size_t group_len, int64_t block_limit_range, int64_t block_number, uint64_t initial_capacity,
                          bcosgpu_txpool** out) {
    if (!out) return api_set_err(BCOSGPU_E_ARG, "null pointer");
    *out = nullptr;
    if (int rc = check_suite(suite)) return rc;
    if ((chain_len && !chain_id) || (group_len && !group_id)) return api_set_err(BCOSGPU_E_ARG, "null pointer");
    if (chain_len > 0xffffu || group_len > 0xffffu) return api_set_err(BCOSGPU_E_ARG, "chain / group id too long");
    constexpr int64_t kMaxNumber = int64_t(1) << 62;  // number + range then never overflows
    if (block_limit_range < 0 || block_limit_range > kMaxNumber || block_number < 0 || block_number > kMaxNumber)
        return api_set_err(BCOSGPU_E_ARG, "block number and block_limit_range must be in [0, 2^62]");
    if (initial_capacity > kMaxKeys) return api_set_err(BCOSGPU_E_ARG, "initial capacity too large");
    if (int rc = api_ready_device(device)) return rc;
    DeviceScope scope(device);
    if (scope.err != hipSuccess) return api_set_err(BCOSGPU_E_HIP, hip_msg(scope.err, "hipSetDevice"));
    bcosgpu_txpool* h = new bcosgpu_txpool();
    Pool& p = *h;
    p.dev = device;
    p.suite = suite;
    p.chain.assign(chain_id ? chain_id : "", chain_len);
    p.group.assign(group_id ? group_id : "", group_len);
    p.range = block_limit_range;
    p.number = block_number;
    const uint32_t cap = initial_capacity ? static_cast<uint32_t>(initial_capacity) : 4096u;
    const std::string ids = p.chain + p.group;
    hipError_t e = hipStreamCreateWithFlags(&p.st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&p.d_meta, sizeof(p.h_meta));
    if (e == hipSuccess) e = hipMemset(p.d_meta, 0, sizeof(p.h_meta));
    if (e == hipSuccess) e = hipMalloc(&p.d_ids, ids.size() + 1);
    if (e == hipSuccess && !ids.empty()) e = hipMemcpy(p.d_ids, ids.data(), ids.size(), hipMemcpyHostToDevice);
    for (DevSet& d : p.sets) {
        d.cap = cap;
        for (uint8_t*& b : d.buf)
            if (e == hipSuccess) e = hipMalloc(&b, static_cast<size_t>(cap) * 32);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        const int rc = api_set_err(BCOSGPU_E_HIP, hip_msg(e, "txpool create"));
        destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

int bcosgpu_txpool_destroy(bcosgpu_txpool* pool) {
    destroy(pool);
    return 0;
}

int bcosgpu_txpool_admit_dev(bcosgpu_txpool* pool, int mode, const uint8_t* d_enc, const uint64_t* d_enc_off, size_t n,
                             uint64_t enc_bytes, uint8_t* d_txhash32, uint8_t* d_sender20, uint8_t* d_nonce32,
                             uint32_t* d_status) {
    TP_ENTER(pool);
    if (mode != BCOSGPU_TXPOOL_FULL && mode != BCOSGPU_TXPOOL_PROPOSAL) return api_set_err(BCOSGPU_E_ARG, "bad mode");
    if (n == 0) return 0;
    if (!d_enc || !d_enc_off || !d_txhash32 || !d_sender20 || !d_nonce32 || !d_status)
        return api_set_err(BCOSGPU_E_ARG, "null pointer");
    if (n > kMaxKeys) return api_set_err(BCOSGPU_E_ARG, "batch too large");
    StreamDrain drain(p.st);
    if (int rc = admit_chain(p, mode, d_enc, d_enc_off, static_cast<uint32_t>(n), enc_bytes, d_txhash32, d_sender20,
                             d_nonce32, d_status))
        return rc;
    return end_call(p, drain);
}

int bcosgpu_txpool_admit(bcosgpu_txpool* pool, int mode, const uint8_t* enc, const uint64_t* enc_off, size_t n,
                         uint8_t* txhash32, uint8_t* sender20, uint8_t* nonce32, uint32_t* status) {
    TP_ENTER(pool);
    if (mode != BCOSGPU_TXPOOL_FULL && mode != BCOSGPU_TXPOOL_PROPOSAL) return api_set_err(BCOSGPU_E_ARG, "bad mode");
    if (n == 0) return 0;
    if (!enc || !enc_off || !txhash32 || !sender20 || !nonce32 || !status)
        return api_set_err(BCOSGPU_E_ARG, "null pointer");
    if (n > kMaxKeys) return api_set_err(BCOSGPU_E_ARG, "batch too large");
    for (size_t i = 0; i < n; ++i)
        if (enc_off[i + 1] < enc_off[i]) return api_set_err(BCOSGPU_E_ARG, "offsets must be non-decreasing");
    const uint64_t base = enc_off[0], bytes = enc_off[n] - base;
    std::vector<uint64_t> off(n + 1);  // (declared before the drain: it runs while this is alive)
    for (size_t i = 0; i <= n; ++i) off[i] = enc_off[i] - base;
    StreamDrain drain(p.st);
    if (int rc = ensure(p, p.enc, bytes + 8)) return rc;
    if (int rc = ensure(p, p.enc_off, (n + 1) * 8)) return rc;
    if (int rc = ensure(p, p.out, n * 88)) return rc;  // txhash 32 n | nonce 32 n | status 4 n | sender 20 n
    TP_HIP(hipMemcpyAsync(p.enc.p, enc + base, bytes, hipMemcpyHostToDevice, p.st));
    TP_HIP(hipMemcpyAsync(p.enc_off.p, off.data(), (n + 1) * 8, hipMemcpyHostToDevice, p.st));
    uint8_t* o = p.out.as<uint8_t>();
    if (int rc = admit_chain(p, mode, p.enc.as<uint8_t>(), p.enc_off.as<uint64_t>(), static_cast<uint32_t>(n), bytes, o,
                             o + 68 * n, o + 32 * n, reinterpret_cast<uint32_t*>(o + 64 * n)))
        return rc;
    TP_HIP(hipMemcpyAsync(txhash32, o, 32 * n, hipMemcpyDeviceToHost, p.st));
    TP_HIP(hipMemcpyAsync(nonce32, o + 32 * n, 32 * n, hipMemcpyDeviceToHost, p.st));
    TP_HIP(hipMemcpyAsync(status, o + 64 * n, 4 * n, hipMemcpyDeviceToHost, p.st));
    TP_HIP(hipMemcpyAsync(sender20, o + 68 * n, 20 * n, hipMemcpyDeviceToHost, p.st));
    return end_call(p, drain);
}

int bcosgpu_txpool_block_committed(bcosgpu_txpool* pool, int64_t number, const uint8_t* txhashes32, size_t nhashes,
                                   const uint8_t* nonces32, size_t nnonces) {
    TP_ENTER(pool);
    if ((nhashes && !txhashes32) || (nnonces && !nonces32)) return api_set_err(BCOSGPU_E_ARG, "null pointer");
    if (number < 0 || number > (int64_t(1) << 62)) return api_set_err(BCOSGPU_E_ARG, "block number out of range");
    StreamDrain drain(p.st);
    // MemoryStorage::batchRemove (MemoryStorage.cpp:435-498) + LedgerNonceChecker::batchInsert (:64-99), in the
    // order of tests/txpool_restatement.py
    if (int rc = set_difference(p, kHashes, txhashes32, nhashes)) return rc;
    if (p.number < number) p.number = number;
    if (int rc = set_union(p, kLedger, nonces32, nnonces)) return rc;
    if (int rc = set_difference(p, kNonces, nonces32, nnonces)) return rc;
    if (!p.blocks.count(number)) p.blocks[number].assign(nonces32, nonces32 + 32 * nnonces);
    const int64_t expired = number > p.range ? number - p.range : -1;
    const auto it = expired < 0 ? p.blocks.end() : p.blocks.find(expired);
    if (it != p.blocks.end()) {
        const std::vector<uint8_t> list = std::move(it->second);  // (alive until end_call's synchronisation)
        p.blocks.erase(it);
        if (int rc = set_difference(p, kLedger, list.data(), list.size() / 32)) return rc;
        return end_call(p, drain);
    }
    return end_call(p, drain);
}

int bcosgpu_txpool_remove(bcosgpu_txpool* pool, const uint8_t* txhashes32, size_t nhashes, const uint8_t* nonces32,
                          size_t nnonces) {
    TP_ENTER(pool);
    if ((nhashes && !txhashes32) || (nnonces && !nonces32)) return api_set_err(BCOSGPU_E_ARG, "null pointer");
    StreamDrain drain(p.st);
    if (int rc = set_difference(p, kHashes, txhashes32, nhashes)) return rc;
    if (int rc = set_difference(p, kNonces, nonces32, nnonces)) return rc;
    return end_call(p, drain);
}

int bcosgpu_txpool_load_ledger_nonces(bcosgpu_txpool* pool, const int64_t* numbers, const uint64_t* nonce_off,
                                      const uint8_t* nonces32, size_t nblocks) {
    TP_ENTER(pool);
    if (nblocks == 0) return 0;
    if (!numbers || !nonce_off) return api_set_err(BCOSGPU_E_ARG, "null pointer");
    for (size_t b = 0; b < nblocks; ++b)
        if (nonce_off[b + 1] < nonce_off[b]) return api_set_err(BCOSGPU_E_ARG, "offsets must be non-decreasing");
    const uint64_t base = nonce_off[0], total = nonce_off[nblocks] - base;
    if (total && !nonces32) return api_set_err(BCOSGPU_E_ARG, "null pointer");
    StreamDrain drain(p.st);
    // LedgerNonceChecker::initNonceCache (:26-34): every block's list is remembered, every nonce enters the set
    for (size_t b = 0; b < nblocks; ++b)
        p.blocks[numbers[b]].assign(nonces32 + 32 * nonce_off[b], nonces32 + 32 * nonce_off[b + 1]);
    if (int rc = set_union(p, kLedger, nonces32 + 32 * base, total)) return rc;
    return end_call(p, drain);
}

int bcosgpu_txpool_info(bcosgpu_txpool* pool, uint64_t out[BCOSGPU_TXPOOL_INFO_WORDS]) {
    if (!pool) return api_set_err(BCOSGPU_E_ARG, "null pool");
    if (!out) return api_set_err(BCOSGPU_E_ARG, "null pointer");
    Pool& p = *pool;
    std::lock_guard<std::mutex> lock(p.mu);
    DeviceScope scope(p.dev);
    if (scope.err != hipSuccess) return api_set_err(BCOSGPU_E_HIP, hip_msg(scope.err, "hipSetDevice"));
    TP_HIP(hipMemcpyAsync(p.h_meta, p.d_meta, sizeof(p.h_meta), hipMemcpyDeviceToHost, p.st));
    TP_HIP(hipStreamSynchronize(p.st));
    for (int s = 0; s < 3; ++s) {
        out[s] = p.h_meta[meta_count(s, p.sets[s].cur)];
        out[3 + s] = p.sets[s].cap;
    }
    out[6] = static_cast<uint64_t>(p.number);
    out[7] = p.blocks.size();
    out[8] = p.h_meta[kMetaErr];
    return 0;
}

int bcosgpu_txpool_dump(bcosgpu_txpool* pool, int which, uint8_t* keys32, uint64_t capacity, uint64_t* count) {
    TP_ENTER(pool);
    if (which < 0 || which > 2) return api_set_err(BCOSGPU_E_ARG, "bad set");
    if (!count) return api_set_err(BCOSGPU_E_ARG, "null pointer");
    const DevSet& d = p.sets[which];
    *count = d.bound;  // the true count: every call ends with the refresh
    if (d.bound == 0) return 0;
    if (!keys32 || capacity < d.bound) return api_set_err(BCOSGPU_E_ARG, "dump buffer too small");
    TP_HIP(hipMemcpyAsync(keys32, d.buf[d.cur], static_cast<size_t>(d.bound) * 32, hipMemcpyDeviceToHost, p.st));
    TP_HIP(hipStreamSynchronize(p.st));
    return 0;
}

}  // extern "C"
