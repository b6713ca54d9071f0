// api.hip -- the C ABI (include/bcos_gpu.h): argument checks, per-device workspaces for the
// host-pointer entry points, and the wedpr-shaped single-call shims.  No exceptions cross the ABI.
#include <atomic>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>
#include <cstring>
#include "engine.h"
#include "consensus_stage.h"

using namespace bcosgpu;

namespace {

thread_local std::string g_err;
int set_err(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int hip_err(hipError_t e, const char* what) { return set_err(BCOSGPU_E_HIP, hip_msg(e, what)); }
#define HIP_OK(call)                                   \
    do {                                               \
        hipError_t e_ = (call);                        \
        if (e_ != hipSuccess) return hip_err(e_, #call); \
    } while (0)

// One workspace per device for the synchronous host-pointer API; the mutex makes those entry
// points safe to call from the reference's concurrent verifier pools (TxPool.h:48-49).
struct Workspace {
    std::mutex mu;
    bool ready = false;
    hipStream_t stream = nullptr;
    DevBuf b[8];
    PinnedBuf h[2];  // staging for packers that write straight into DMA-able memory
};
std::mutex g_mu;
std::vector<Workspace*> g_ws;
std::atomic<bool> g_ready[64];  // device initialised (tables built): the single-call fast path

int current_device(int* dev) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return set_err(BCOSGPU_E_NODEV, "no HIP device visible");
    }
    HIP_OK(hipGetDevice(dev));
    return 0;
}

int get_ws(Workspace** out) {
    int dev = 0;
    int rc = current_device(&dev);
    if (rc) return rc;
    rc = bcosgpu_init(dev);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(g_mu);
    *out = g_ws[dev];
    return 0;
}

// One call on the workspace of the calling thread's device.  It owns, in this order, the workspace, its
// lock and the drain of its stream: whatever way the call returns before finish(), the stream is idle
// before the mutex is released, so nothing of a failed call writes the caller's memory or runs into the
// next call's buffers.  `if (c.rc) return c.rc;` follows the declaration.
struct WsCall {
    Workspace* w = nullptr;
    const int rc;
    std::unique_lock<std::mutex> lock;
    StreamDrain drain;
    WsCall()
        : rc(get_ws(&w)), lock(rc ? std::unique_lock<std::mutex>() : std::unique_lock<std::mutex>(w->mu)),
          drain(rc ? nullptr : w->stream) {}
    hipStream_t stream() const { return w->stream; }
    template <class T = uint8_t> T* buf(int i) const { return w->b[i].as<T>(); }
    // buffers 0, 1, ... of at least these sizes (0: not used by this call)
    hipError_t ensure(std::initializer_list<size_t> bytes) {
        int i = 0;
        for (size_t n : bytes)
            if (hipError_t e = w->b[i++].ensure(n)) return e;
        return hipSuccess;
    }
    hipError_t h2d(int i, const void* src, size_t bytes) {
        return hipMemcpyAsync(w->b[i].p, src, bytes, hipMemcpyHostToDevice, w->stream);
    }
    hipError_t d2h(void* dst, int i, size_t bytes) {
        return hipMemcpyAsync(dst, w->b[i].p, bytes, hipMemcpyDeviceToHost, w->stream);
    }
    int finish() {  // the synchronisation that ends the success path
        HIP_OK(hipStreamSynchronize(w->stream));
        drain.dismiss();
        return 0;
    }
};

inline hipStream_t as_stream(void* s) { return static_cast<hipStream_t>(s); }

int init_device(int device, int flags);

// The explicit-device entry points: initialise `device` once, without changing the calling thread's
// current device.
int ready_device(int device) {
    if (device >= 0 && device < 64 && g_ready[device].load(std::memory_order_acquire)) return 0;
    DeviceScope keep(device);  // (init_device selects the device itself and reports why it could not)
    return init_device(device, 0);
}

// A host-pointer signature call as a coalesced job (coalesce.hip) on `device`.
int run_job(int device, SigJob& job) {
    int rc = ready_device(device);
    if (rc) return rc;
    rc = coalesced_run(device, job);
    return rc ? set_err(rc, job.err) : 0;
}

int calling_device(int* dev) {
    int rc = current_device(dev);
    return rc ? rc : ready_device(*dev);
}

}  // namespace

// for the device-set entry points (multi.hip)
namespace bcosgpu {
int api_set_err(int code, const std::string& msg) { return set_err(code, msg); }
int api_ready_device(int device) { return ready_device(device); }
int api_run_job(int device, SigJob& job) { return run_job(device, job); }
}  // namespace bcosgpu

extern "C" {

int bcosgpu_version(void) { return BCOSGPU_VERSION; }

int bcosgpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

const char* bcosgpu_last_error(void) { return g_err.c_str(); }

uint64_t bcosgpu_merkle_size(uint64_t n, int width) {
    if (width < 2) return 0;
    return n == 1 ? 1 : merkle_size(n, width);
}

int bcosgpu_init(int device) { return bcosgpu_init_ex(device, 0); }

int bcosgpu_init_ex(int device, int flags) { return init_device(device, flags); }

}  // extern "C"

namespace {
// selects `device` on the calling thread and builds its tables once
int init_device(int device, int flags) {
    int n = bcosgpu_device_count();
    if (n <= 0) return set_err(BCOSGPU_E_NODEV, "no HIP device visible");
    if (device < 0 || device >= n) return set_err(BCOSGPU_E_ARG, "device index out of range");
    HIP_OK(hipSetDevice(device));
    std::lock_guard<std::mutex> g(g_mu);
    if (g_ws.size() < static_cast<size_t>(n)) g_ws.resize(n, nullptr);
    if (!g_ws[device]) g_ws[device] = new Workspace();
    Workspace* w = g_ws[device];
    if (!w->ready) {
        hipDeviceProp_t prop;
        HIP_OK(hipGetDeviceProperties(&prop, device));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return set_err(BCOSGPU_E_NODEV, std::string("device is ") + prop.gcnArchName + ", built for gfx950");
        HIP_OK(hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking));
        int rc = ecc_init_tables(device, (flags & BCOSGPU_INIT_SMALL_TABLES) != 0);
        if (rc) return set_err(rc, "ecc table setup failed");
        w->ready = true;
        if (device < 64) g_ready[device].store(true, std::memory_order_release);
    }
    return 0;
}
}  // namespace

extern "C" {

int bcosgpu_set_tx_kernel_policy(int split, int occupancy, int coop, int field) {
    set_tx_kernel_policy(split, occupancy, coop, field);
    return 0;
}

// ------------------------------------------------------------------ hashing
int bcosgpu_hash_batch_dev(int hasher, const uint8_t* d_data, const uint64_t* d_offsets, size_t n,
                           uint8_t* d_out32, void* stream) {
    if (int rc = check_hasher(hasher)) return rc;
    if (n && (!d_data || !d_offsets || !d_out32)) return set_err(BCOSGPU_E_ARG, "null pointer");
    int rc = launch_hash_batch(hasher, d_data, d_offsets, n, d_out32, as_stream(stream));
    return rc ? hip_err(hipGetLastError(), "hash_batch launch") : 0;
}

int bcosgpu_hash_batch(int hasher, const uint8_t* data, const uint64_t* offsets, size_t n,
                       uint8_t* out32) {
    if (int rc = check_hasher(hasher)) return rc;
    if (n == 0) return 0;
    if (!data || !offsets || !out32) return set_err(BCOSGPU_E_ARG, "null pointer");
    const uint64_t base = offsets[0], bytes = offsets[n] - base;
    for (size_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 0xFFFFFFFFull)
            return set_err(BCOSGPU_E_ARG, "offsets must be non-decreasing and messages < 4 GiB");
    std::vector<uint64_t> off(n + 1);  // (declared before the call: the drain runs while it is alive)
    for (size_t i = 0; i <= n; ++i) off[i] = offsets[i] - base;
    WsCall c;
    if (c.rc) return c.rc;
    HIP_OK(c.ensure({bytes + 8, (n + 1) * 8, n * 32}));
    HIP_OK(c.h2d(0, data + base, bytes));
    HIP_OK(c.h2d(1, off.data(), (n + 1) * 8));
    if (launch_hash_batch(hasher, c.buf(0), c.buf<uint64_t>(1), n, c.buf(2), c.stream()))
        return hip_err(hipGetLastError(), "hash_batch launch");
    HIP_OK(c.d2h(out32, 2, n * 32));
    return c.finish();
}

int bcosgpu_keccak256_batch(const uint8_t* data, const uint64_t* offsets, size_t n, uint8_t* out32) {
    return bcosgpu_hash_batch(BCOSGPU_KECCAK256, data, offsets, n, out32);
}
int bcosgpu_sm3_batch(const uint8_t* data, const uint64_t* offsets, size_t n, uint8_t* out32) {
    return bcosgpu_hash_batch(BCOSGPU_SM3, data, offsets, n, out32);
}

// ------------------------------------------------------------------ Merkle
int bcosgpu_merkle_root_dev(int hasher, int width, const uint8_t* d_leaves32, size_t n,
                            uint8_t* d_tree, uint8_t* d_root32, void* stream) {
    if (int rc = check_hasher(hasher)) return rc;
    if (n == 0) return set_err(BCOSGPU_E_EMPTY, "Empty input");
    if (int rc = check_width(width)) return rc;
    if (!d_leaves32 || !d_tree) return set_err(BCOSGPU_E_ARG, "null pointer");
    int rc = launch_merkle(hasher, width, d_leaves32, n, d_tree, d_root32, as_stream(stream));
    return rc ? hip_err(hipGetLastError(), "merkle launch") : 0;
}

uint64_t bcosgpu_merkle_bytes_size(uint64_t n, int width) {
    if (width < 2 || n == 0) return 0;
    return n == 1 ? 32 : 32 * merkle_size(n, width) - 28 * merkle_levels(n, width);
}

int bcosgpu_merkle_tree_bytes_dev(int width, const uint8_t* d_tree, size_t n, uint8_t* d_out, void* stream) {
    if (int rc = check_width(width)) return rc;
    if (n == 0) return set_err(BCOSGPU_E_EMPTY, "Empty input");
    if (!d_tree || !d_out) return set_err(BCOSGPU_E_ARG, "null pointer");
    int rc = launch_merkle_compact(d_tree, n, width, d_out, as_stream(stream));
    return rc ? hip_err(hipGetLastError(), "merkle compact launch") : 0;
}

int bcosgpu_merkle_root(int hasher, int width, int variant, const uint8_t* leaves32, size_t n,
                        uint8_t* root32, uint8_t* levels) {
    if (int rc = check_hasher(hasher)) return rc;
    if (!root32 || (n && !leaves32)) return set_err(BCOSGPU_E_ARG, "null pointer");
    const bool bytes_layout = variant == BCOSGPU_MERKLE_NEW_BYTES;
    if (bytes_layout) variant = BCOSGPU_MERKLE_NEW;
    if (variant == BCOSGPU_MERKLE_NEW) {
        if (n == 0) return set_err(BCOSGPU_E_EMPTY, "Empty input");
        if (int rc = check_width(width)) return rc;
    } else if (variant != BCOSGPU_MERKLE_OLD) {
        return set_err(BCOSGPU_E_ARG, "bad variant");
    }
    WsCall c;
    if (c.rc) return c.rc;
    const uint64_t tree = variant == BCOSGPU_MERKLE_NEW ? bcosgpu_merkle_size(n, width) : merkle_size(n, 16) + 1;
    const bool compact = levels && bytes_layout;
    HIP_OK(c.ensure({n * 32 + 32, tree * 32 + 32, 32, compact ? tree * 32 + 32 : 0}));
    if (n) HIP_OK(c.h2d(0, leaves32, n * 32));
    int rc;
    if (variant == BCOSGPU_MERKLE_NEW)
        rc = launch_merkle(hasher, width, c.buf(0), n, c.buf(1), c.buf(2), c.stream());
    else
        rc = launch_merkle_old(hasher, c.buf(0), n, c.buf(1), c.buf(2), c.stream());
    if (!rc && compact) rc = launch_merkle_compact(c.buf(1), n, width, c.buf(3), c.stream());
    if (rc) return rc == BCOSGPU_E_ARG ? set_err(rc, "bad merkle arguments") : hip_err(hipGetLastError(), "merkle launch");
    HIP_OK(c.d2h(root32, 2, 32));
    if (compact)
        HIP_OK(c.d2h(levels, 3, bcosgpu_merkle_bytes_size(n, width)));
    else if (levels && variant == BCOSGPU_MERKLE_NEW)
        HIP_OK(c.d2h(levels, 1, tree * 32));
    return c.finish();
}

int bcosgpu_merkle_frontier_dev(int hasher, int width, const uint8_t* d_leaves32, size_t n, int levels,
                                uint8_t* d_work, uint8_t* d_frontier, void* stream) {
    if (int rc = check_hasher(hasher)) return rc;
    if (n == 0) return set_err(BCOSGPU_E_EMPTY, "Empty input");
    if (width < 2 || width > 64 || levels < 1 || levels > 63) return set_err(BCOSGPU_E_ARG, "bad width/levels");
    if (!d_leaves32 || !d_work || !d_frontier) return set_err(BCOSGPU_E_ARG, "null pointer");
    int rc = launch_merkle_levels(hasher, width, d_leaves32, n, levels, d_work, d_frontier, as_stream(stream));
    return rc ? hip_err(hipGetLastError(), "merkle frontier launch") : 0;
}

uint64_t bcosgpu_merkle_roots_work_size(uint64_t total_leaves, size_t nblocks, int width) {
    if (width < 2 || width > 64) return 0;
    return merkle_roots_work_bytes(total_leaves, nblocks, width);
}

static int check_block_off(const uint64_t* block_off, size_t nblocks) {
    if (!block_off) return set_err(BCOSGPU_E_ARG, "null block offsets");
    for (size_t b = 0; b < nblocks; ++b)
        if (block_off[b + 1] < block_off[b] || block_off[b + 1] - block_off[b] > 0xFFFFFFFFull)
            return set_err(BCOSGPU_E_ARG, "block offsets must be non-decreasing, blocks < 2^32 leaves");
    return 0;
}

int bcosgpu_merkle_roots_batch_dev(int hasher, int width, const uint8_t* d_leaves32, const uint64_t* block_off,
                                   size_t nblocks, uint8_t* d_work, uint8_t* d_roots32, void* stream) {
    if (int rc = check_hasher(hasher)) return rc;
    if (int rc = check_width(width)) return rc;
    if (nblocks == 0) return 0;
    if (int rc = check_block_off(block_off, nblocks)) return rc;
    if (!d_work || !d_roots32 || (block_off[nblocks] > block_off[0] && !d_leaves32))
        return set_err(BCOSGPU_E_ARG, "null pointer");
    int rc = launch_merkle_roots_batch(hasher, width, d_leaves32, block_off, nblocks, d_work, d_roots32,
                                       as_stream(stream));
    return rc ? hip_err(hipGetLastError(), "merkle roots launch") : 0;
}

int bcosgpu_merkle_roots_batch(int hasher, int width, const uint8_t* leaves32, const uint64_t* block_off,
                               size_t nblocks, uint8_t* roots32) {
    if (int rc = check_hasher(hasher)) return rc;
    if (int rc = check_width(width)) return rc;
    if (nblocks == 0) return 0;
    if (int rc = check_block_off(block_off, nblocks)) return rc;
    const uint64_t total = block_off[nblocks] - block_off[0];
    if (!roots32 || (total && !leaves32)) return set_err(BCOSGPU_E_ARG, "null pointer");
    WsCall c;
    if (c.rc) return c.rc;
    HIP_OK(c.ensure({total * 32 + 32, merkle_roots_work_bytes(total, nblocks, width), nblocks * 32}));
    if (total) HIP_OK(c.h2d(0, leaves32, total * 32));
    if (launch_merkle_roots_batch(hasher, width, c.buf(0), block_off, nblocks, c.buf(1), c.buf(2), c.stream()))
        return hip_err(hipGetLastError(), "merkle roots launch");
    HIP_OK(c.d2h(roots32, 2, nblocks * 32));
    return c.finish();
}

// calculateReceiptRoot for many blocks (BlockImpl.h:156-183): the receipt preimages are packed
// (pack.cpp, TarsHashable.h:54-73) straight into pinned staging, one H2D, one hash launch, the dataHash
// short-circuits (TarsHashable.h:47-51) patched in, then the many-tree root kernel.
int bcosgpu_receipt_roots(int hasher, const bcosgpu_TransactionReceiptData* receipts, const uint64_t* block_off,
                          size_t nblocks, uint8_t* roots32, uint8_t* hashes32) {
    if (int rc = check_hasher(hasher)) return rc;
    if (nblocks == 0) return 0;
    if (int rc = check_block_off(block_off, nblocks)) return rc;
    if (block_off[0] != 0) return set_err(BCOSGPU_E_ARG, "block_off[0] must be 0");
    const uint64_t n = block_off[nblocks];
    if (!roots32 || (n && !receipts)) return set_err(BCOSGPU_E_ARG, "null pointer");
    WsCall c;
    if (c.rc) return c.rc;
    Workspace* w = c.w;
    const uint64_t bytes = bcosgpu_receipt_preimage_size(receipts, n);
    bool patched = false;
    for (uint64_t i = 0; i < n && !patched; ++i) patched = receipts[i].data_hash_len != 0;
    HIP_OK(w->h[0].ensure(bytes + 8 * (n + 1) + 16));
    if (patched) HIP_OK(w->h[1].ensure(32 * n + 32));
    uint64_t* off = w->h[0].as<uint64_t>();
    uint8_t* pre = reinterpret_cast<uint8_t*>(off + n + 1);
    if (bcosgpu_pack_receipt_preimages(receipts, n, pre, bytes, off))
        return set_err(BCOSGPU_E_ARG, "bad receipt view (null field with a length, or a dataHash over 32 bytes)");
    HIP_OK(c.ensure({bytes + 8 * (n + 1) + 16, 32 * n + 32, merkle_roots_work_bytes(n, nblocks, 2), nblocks * 32}));
    uint8_t* d_hash = c.buf(1);
    if (n) {
        HIP_OK(c.h2d(0, off, bytes + 8 * (n + 1)));
        const uint64_t* d_off = c.buf<uint64_t>(0);
        if (launch_hash_batch(hasher, reinterpret_cast<const uint8_t*>(d_off + n + 1), d_off, n, d_hash, c.stream()))
            return hip_err(hipGetLastError(), "receipt hash launch");
        if (patched) {  // the dataHash receipts: hashes round-trip through the host once
            uint8_t* h = w->h[1].as<uint8_t>();
            HIP_OK(c.d2h(h, 1, 32 * n));
            HIP_OK(hipStreamSynchronize(c.stream()));
            bcosgpu_apply_receipt_data_hashes(receipts, n, h);
            HIP_OK(c.h2d(1, h, 32 * n));
        }
    }
    if (launch_merkle_roots_batch(hasher, 2, d_hash, block_off, nblocks, c.buf(2), c.buf(3), c.stream()))
        return hip_err(hipGetLastError(), "merkle roots launch");
    HIP_OK(c.d2h(roots32, 3, nblocks * 32));
    if (hashes32 && n) HIP_OK(c.d2h(hashes32, 1, 32 * n));
    return c.finish();
}

// ------------------------------------------------------------------ state root
uint64_t bcosgpu_state_root_work_size(size_t n) { return state_root_work_bytes(n); }

int bcosgpu_state_root_dev(int hasher, uint32_t block_version, const uint8_t* d_data, const uint64_t* d_off3,
                           const uint8_t* d_kind, size_t n, void* d_work, uint64_t work_bytes, uint8_t* d_root32,
                           void* stream) {
    if (int rc = check_hasher(hasher)) return rc;
    if (!d_root32 || (n && (!d_data || !d_off3 || !d_kind || !d_work))) return set_err(BCOSGPU_E_ARG, "null pointer");
    const int rc = launch_state_root(hasher, block_version, d_data, d_off3, d_kind, n, d_work, work_bytes, d_root32,
                                     as_stream(stream));
    if (rc == BCOSGPU_E_ARG) return set_err(rc, "work buffer too small or batch too large");
    return rc ? hip_err(hipGetLastError(), "state root launch") : 0;
}

// StateStorage::hash / KeyPageStorage::hash (StateStorage.h:397-431, KeyPageStorage.cpp:351-406): the entries
// are packed (pack.cpp) straight into pinned staging as off3 | data | kind, one H2D, the fused kernel and its
// fold, 32 bytes back.
int bcosgpu_state_root(int hasher, uint32_t block_version, const bcosgpu_StateEntry* entries, size_t n,
                       uint8_t* root32) {
    if (int rc = check_hasher(hasher)) return rc;
    if (!root32 || (n && !entries)) return set_err(BCOSGPU_E_ARG, "null pointer");
    if (n == 0) {  // no dirty entry: the zero hash (StateStorage.h:399)
        std::memset(root32, 0, 32);
        return 0;
    }
    WsCall c;
    if (c.rc) return c.rc;
    Workspace* w = c.w;
    const uint64_t bytes = bcosgpu_state_entries_size(entries, n), offb = 8 * (3 * static_cast<uint64_t>(n) + 1);
    const uint64_t total = offb + bytes + n, work = state_root_work_bytes(n);
    HIP_OK(w->h[0].ensure(total + 16));
    uint64_t* off3 = w->h[0].as<uint64_t>();
    uint8_t* data = reinterpret_cast<uint8_t*>(off3) + offb;
    if (bcosgpu_pack_state_entries(entries, n, data, bytes, off3, data + bytes))
        return set_err(BCOSGPU_E_ARG, "bad state entry view (null field with a length, status outside 0..3, or an "
                                      "entry of 4 GiB or more)");
    HIP_OK(c.ensure({total + 16, work, 32}));
    HIP_OK(c.h2d(0, off3, total));
    const uint8_t* d_data = c.buf(0) + offb;
    const int rc = launch_state_root(hasher, block_version, d_data, c.buf<uint64_t>(0), d_data + bytes, n, c.buf<void>(1),
                                     work, c.buf(2), c.stream());
    if (rc == BCOSGPU_E_ARG) return set_err(rc, "batch too large");
    if (rc) return hip_err(hipGetLastError(), "state root launch");
    HIP_OK(c.d2h(root32, 2, 32));
    return c.finish();
}

}  // extern "C"

// ------------------------------------------------------------------ storage cipher (cipher_kernels.hip)
namespace {

// the checks every cipher entry point shares (0, or E_ARG with the message set); they need no device
int check_cipher_key(int cipher_id, const uint8_t* key, size_t key_len, const uint8_t* iv, size_t iv_len) {
    if (cipher_id != BCOSGPU_CIPHER_AES256 && cipher_id != BCOSGPU_CIPHER_SM4) return set_err(BCOSGPU_E_ARG, "bad cipher");
    if ((!key && key_len) || (!iv && iv_len)) return set_err(BCOSGPU_E_ARG, "null key or iv with a length");
    return 0;
}
int check_value_views(const bcosgpu_Bytes* values, size_t n) {
    if (n > 0xFFFFFFFFull) return set_err(BCOSGPU_E_ARG, "batch too large");
    if (n && !values) return set_err(BCOSGPU_E_ARG, "null pointer");
    for (size_t i = 0; i < n; ++i)
        if ((!values[i].data && values[i].len) || values[i].len > 0xFFFFFFFFull)
            return set_err(BCOSGPU_E_ARG, "bad value view (null data with a length, or a value of 4 GiB or more)");
    return 0;
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
uint64_t round16(uint64_t x) { return (x + 15) & ~15ull; }

}  // namespace

extern "C" {

uint64_t bcosgpu_cbc_padded_size(uint64_t len) { return cipher::cbc_padded_size(len); }
uint64_t bcosgpu_cbc_work_size(size_t n) { return cbc_work_bytes(n); }

int bcosgpu_cbc_encrypt_batch_dev(int cipher_id, const uint8_t* key, size_t key_len, const uint8_t* iv, size_t iv_len,
                                  const uint8_t* d_in, const uint64_t* d_in_off, size_t n, uint8_t* d_out,
                                  uint64_t* d_out_off, void* d_work, uint64_t work_bytes, void* stream) {
    if (int rc = check_cipher_key(cipher_id, key, key_len, iv, iv_len)) return rc;
    if (n == 0) return 0;
    if (!d_in || !d_in_off || !d_out || !d_out_off || !d_work) return set_err(BCOSGPU_E_ARG, "null pointer");
    if (!aligned16(d_out) || (reinterpret_cast<uintptr_t>(d_work) & 7u))
        return set_err(BCOSGPU_E_ARG, "d_out must be 16-byte aligned and d_work 8-byte aligned");
    const cipher::Schedule ck = cipher::make_schedule(cipher_id, false, key, key_len, iv, iv_len);
    const int rc = launch_cbc_encrypt(cipher_id, ck, d_in, d_in_off, n, d_out, d_out_off, d_work, work_bytes,
                                      as_stream(stream));
    if (rc == BCOSGPU_E_ARG) return set_err(rc, "work buffer too small or batch too large");
    return rc ? hip_err(hipGetLastError(), "cbc encrypt launch") : 0;
}

int bcosgpu_cbc_decrypt_batch_dev(int cipher_id, const uint8_t* key, size_t key_len, const uint8_t* iv, size_t iv_len,
                                  const uint8_t* d_in, const uint64_t* d_in_off, size_t n, uint8_t* d_out,
                                  uint32_t* d_out_len, uint8_t* d_status, void* stream) {
    if (int rc = check_cipher_key(cipher_id, key, key_len, iv, iv_len)) return rc;
    if (n == 0) return 0;
    if (!d_in || !d_in_off || !d_out || !d_out_len || !d_status) return set_err(BCOSGPU_E_ARG, "null pointer");
    if (d_in == d_out) return set_err(BCOSGPU_E_ARG, "input and output must not overlap");
    if (!aligned16(d_in) || !aligned16(d_out)) return set_err(BCOSGPU_E_ARG, "d_in and d_out must be 16-byte aligned");
    const cipher::Schedule ck = cipher::make_schedule(cipher_id, true, key, key_len, iv, iv_len);
    const int rc = launch_cbc_decrypt(cipher_id, ck, d_in, d_in_off, n, d_out, d_out_len, d_status, as_stream(stream));
    if (rc == BCOSGPU_E_ARG) return set_err(rc, "batch too large");
    return rc ? hip_err(hipGetLastError(), "cbc decrypt launch") : 0;
}

// DataEncryption::encrypt over the values of a commit (RocksDBStorage.cpp:348-353, :513-524): the values are
// gathered into pinned staging as off | data, one H2D, the kernels, the ciphertexts back in one copy.  The
// output offsets are also computed here: the cap check needs them before anything runs.
int bcosgpu_cbc_encrypt_batch(int cipher_id, const uint8_t* key, size_t key_len, const uint8_t* iv, size_t iv_len,
                              const bcosgpu_Bytes* values, size_t n, uint8_t* out, uint64_t cap, uint64_t* out_off) {
    if (int rc = check_cipher_key(cipher_id, key, key_len, iv, iv_len)) return rc;
    if (int rc = check_value_views(values, n)) return rc;
    if (n == 0) return 0;
    if (!out || !out_off) return set_err(BCOSGPU_E_ARG, "null pointer");
    uint64_t bytes = 0, total = 0;
    for (size_t i = 0; i < n; ++i) bytes += values[i].len, total += cipher::cbc_padded_size(values[i].len);
    if (cap < total) return set_err(BCOSGPU_E_ARG, "cap too small");
    const cipher::Schedule ck = cipher::make_schedule(cipher_id, false, key, key_len, iv, iv_len);
    WsCall c;
    if (c.rc) return c.rc;
    Workspace* w = c.w;
    const uint64_t offb = 8 * (static_cast<uint64_t>(n) + 1), in_bytes = offb + bytes, work = cbc_work_bytes(n);
    HIP_OK(w->h[0].ensure(in_bytes + 16));
    uint64_t* off = w->h[0].as<uint64_t>();
    uint8_t* data = reinterpret_cast<uint8_t*>(off) + offb;
    off[0] = out_off[0] = 0;
    for (size_t i = 0; i < n; ++i) {
        if (values[i].len) std::memcpy(data + off[i], values[i].data, values[i].len);
        off[i + 1] = off[i] + values[i].len;
        out_off[i + 1] = out_off[i] + cipher::cbc_padded_size(values[i].len);
    }
    HIP_OK(c.ensure({in_bytes + 16, total, offb, work}));
    HIP_OK(c.h2d(0, off, in_bytes));
    const int rc = launch_cbc_encrypt(cipher_id, ck, c.buf(0) + offb, c.buf<uint64_t>(0), n, c.buf(1), c.buf<uint64_t>(2),
                                      c.buf<void>(3), work, c.stream());
    if (rc) return hip_err(hipGetLastError(), "cbc encrypt launch");
    HIP_OK(c.d2h(out, 1, total));
    return c.finish();
}

// DataEncryption::decrypt over the values of a batched read (RocksDBStorage.cpp:106-108, :204-205): an item whose
// length is not a non-zero multiple of 16 fails here, the rest are packed (their offsets stay multiples of 16)
// and decrypted; the raw plaintext blocks, lengths and statuses come back in one copy and are compacted.
int bcosgpu_cbc_decrypt_batch(int cipher_id, const uint8_t* key, size_t key_len, const uint8_t* iv, size_t iv_len,
                              const bcosgpu_Bytes* values, size_t n, uint8_t* out, uint64_t cap, uint64_t* out_off,
                              uint8_t* status) {
    if (int rc = check_cipher_key(cipher_id, key, key_len, iv, iv_len)) return rc;
    if (int rc = check_value_views(values, n)) return rc;
    if (n == 0) return 0;
    if (!out_off || !status) return set_err(BCOSGPU_E_ARG, "null pointer");
    uint64_t bytes = 0, m = 0;  // of the well-formed items
    for (size_t i = 0; i < n; ++i)
        if (values[i].len && values[i].len % 16 == 0) bytes += values[i].len, ++m;
    if (cap < bytes || (bytes && !out)) return set_err(BCOSGPU_E_ARG, bytes && !out ? "null pointer" : "cap too small");
    if (m == 0) {
        for (size_t i = 0; i <= n; ++i) out_off[i] = 0;
        std::memset(status, BCOSGPU_CBC_E_LENGTH, n);
        return 0;
    }
    const cipher::Schedule ck = cipher::make_schedule(cipher_id, true, key, key_len, iv, iv_len);
    WsCall c;
    if (c.rc) return c.rc;
    Workspace* w = c.w;
    // staging in: data (16-byte aligned, first) | off[m+1]; back: plaintext blocks | out_len[m] | status[m]
    const uint64_t offb = 8 * (m + 1), in_bytes = bytes + offb, back = bytes + 4 * m + m;
    HIP_OK(w->h[0].ensure(in_bytes));
    HIP_OK(w->h[1].ensure(back));
    uint8_t* data = w->h[0].as<uint8_t>();
    uint64_t* off = reinterpret_cast<uint64_t*>(data + bytes);
    uint64_t at = 0, k = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!values[i].len || values[i].len % 16) continue;
        std::memcpy(data + at, values[i].data, values[i].len);
        off[k++] = at;
        at += values[i].len;
    }
    off[m] = at;
    HIP_OK(c.ensure({in_bytes, back}));
    HIP_OK(c.h2d(0, data, in_bytes));
    uint8_t* d_back = c.buf(1);
    const int rc = launch_cbc_decrypt(cipher_id, ck, c.buf(0), reinterpret_cast<const uint64_t*>(c.buf(0) + bytes), m,
                                      d_back, reinterpret_cast<uint32_t*>(d_back + bytes), d_back + bytes + 4 * m,
                                      c.stream());
    if (rc) return hip_err(hipGetLastError(), "cbc decrypt launch");
    HIP_OK(c.d2h(w->h[1].p, 1, back));
    HIP_OK(hipStreamSynchronize(c.stream()));
    const uint8_t* plain = w->h[1].as<uint8_t>();
    const uint32_t* len = reinterpret_cast<const uint32_t*>(plain + bytes);
    const uint8_t* st = plain + bytes + 4 * m;
    out_off[0] = 0;
    k = 0;
    for (size_t i = 0; i < n; ++i) {
        uint64_t got = 0;
        if (!values[i].len || values[i].len % 16) {
            status[i] = BCOSGPU_CBC_E_LENGTH;
        } else {
            status[i] = st[k];
            got = st[k] == BCOSGPU_CBC_OK ? len[k] : 0;
            if (got) std::memcpy(out + out_off[i], plain + off[k], got);
            ++k;
        }
        out_off[i + 1] = out_off[i] + got;
    }
    return c.finish();
}

}  // extern "C"

// ------------------------------------------------------------------ signature rows against a consensus set
namespace {

// The device half of a check's signature rows (ConsensusRows, consensus_stage.h, is the host half): the consensus
// keys are registered (a cached key is a lookup) and their slot ids handed to the stage's plan; no rows, or an
// empty set, registers nothing.  Constructed after the call's WsCall (the device is initialised by then).
struct ConsensusKeys {
    const int suite;
    const uint64_t gen;          // the key cache's generation before the registration
    std::vector<int32_t> slots;  // of the consensus keys, -1 = none
    ConsensusKeys(int suite_, const bcosgpu_ConsensusSet& cs, uint64_t rows)
        : suite(suite_), gen(keyed_generation(suite_)), slots(cs.n, -1) {
        if (rows && cs.n && keyed_register(suite, cs.node_ids64, cs.n, slots.data())) {
            (void)hipGetLastError();  // a failed table build leaves the key path
            slots.assign(cs.n, -1);
        }
    }
    bool stale() const { return keyed_generation(suite) != gen; }
};

int check_consensus_set(const bcosgpu_ConsensusSet& cs) {
    if (cs.n && (!cs.node_ids64 || !cs.weights)) return set_err(BCOSGPU_E_ARG, "null consensus set");
    if (cs.n > 0x7FFFFFFFull) return set_err(BCOSGPU_E_ARG, "consensus set too large");
    return 0;
}

// Runs the check's kernels over the arguments `a` (`launch`: launch_headers_check or launch_pbft_check) and the
// download of the out_bytes at dout into ho, on c's stream, and waits for them.  If the key cache was cleared
// (bcosgpu_clear_keys) between the registration and here, the ids may name other keys' tables by now: the run
// is repeated once with the keys in the rows (as coalesce.hip does), uploaded into workspace buffer 3.
template <class Args, class Launch>
int run_rows(WsCall& c, const ConsensusKeys& keys, ConsensusRows& cr, Args& a, Launch launch, const char* what,
             uint8_t* ho, const uint8_t* dout, uint64_t out_bytes) {
    for (int attempt = 0; attempt < 2; ++attempt) {
        const int rc = launch(keys.suite, a, c.stream());
        if (rc == BCOSGPU_E_ARG) return set_err(rc, "batch too large");
        if (rc) return hip_err(hipGetLastError(), what);
        HIP_OK(hipMemcpyAsync(ho, dout, out_bytes, hipMemcpyDeviceToHost, c.stream()));
        HIP_OK(hipStreamSynchronize(c.stream()));
        if (!a.d_row_slot || !keys.stale()) break;
        HIP_OK(c.w->b[3].ensure(64 * cr.rows));
        HIP_OK(c.h2d(3, cr.row_pubs(), 64 * cr.rows));
        a.d_row_slot = nullptr, a.d_row_pub64 = c.buf(3);
    }
    return 0;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ block headers (header_kernels.hip)
uint64_t bcosgpu_headers_check_work_size(size_t n, size_t rows) { return headers_check_work_bytes(n, rows); }

int bcosgpu_headers_check_dev(int suite, const uint8_t* d_pre, const uint64_t* d_pre_off, const uint8_t* d_given32,
                              const uint8_t* d_given_mask, const uint8_t* d_pre_status, const int64_t* d_number,
                              const int64_t* d_parent_number, const uint8_t* d_parent_hash32,
                              const uint8_t* d_parent_ok, const uint8_t* d_prev_hash32, int64_t prev_number,
                              const uint64_t* d_sig_off, const uint8_t* d_sig, const uint64_t* d_row_weight,
                              const int32_t* d_row_slot, const uint8_t* d_row_pub64, uint64_t quorum, size_t n,
                              size_t rows, uint8_t* d_hash32, uint8_t* d_check, uint8_t* d_link, uint8_t* d_sig_ok,
                              void* d_work, uint64_t work_bytes, void* stream) {
    if (int rc = check_suite(suite)) return rc;
    if (n == 0) return 0;
    if (!d_pre || !d_pre_off || !d_pre_status || !d_number || !d_parent_number || !d_parent_hash32 || !d_parent_ok ||
        !d_sig_off || !d_hash32 || !d_check || !d_link || !d_work || (rows && (!d_sig || !d_row_weight)))
        return set_err(BCOSGPU_E_ARG, "null pointer");
    if (rows && (d_row_slot != nullptr) == (d_row_pub64 != nullptr))
        return set_err(BCOSGPU_E_ARG, "exactly one of d_row_slot and d_row_pub64 must be given");
    HeadersCheckArgs a;
    a.d_pre = d_pre, a.d_pre_off = d_pre_off, a.d_given32 = d_given32, a.d_given_mask = d_given_mask;
    a.d_pre_status = d_pre_status, a.d_number = d_number, a.d_parent_number = d_parent_number;
    a.d_parent_hash32 = d_parent_hash32, a.d_parent_ok = d_parent_ok, a.d_prev_hash32 = d_prev_hash32;
    a.prev_number = prev_number, a.d_sig_off = d_sig_off, a.d_sig = d_sig, a.d_row_weight = d_row_weight;
    a.d_row_slot = d_row_slot, a.d_row_pub64 = d_row_pub64, a.quorum = quorum, a.n = n, a.rows = rows;
    a.d_hash32 = d_hash32, a.d_check = d_check, a.d_link = d_link, a.d_sig_ok = d_sig_ok;
    a.d_work = d_work, a.work_bytes = work_bytes;
    const int rc = launch_headers_check(suite, a, as_stream(stream));
    if (rc == BCOSGPU_E_ARG)
        return set_err(rc, "work buffer too small, batch too large, or no key registered on this device");
    return rc ? hip_err(hipGetLastError(), "headers check launch") : 0;
}

// BlockValidator::asyncCheckBlock and the ledger's parent check for a run of headers (see bcos_gpu.h): the
// early verdicts and the rows' keys and weights on the host, everything packed into pinned staging as one
// block (HeadersStage, consensus_stage.h), one H2D, the three phases, one D2H.
int bcosgpu_headers_check(int suite, const bcosgpu_BlockHeaderData* headers, size_t n,
                          const bcosgpu_ConsensusSet* consensus, const uint8_t* prev_hash32_or_null,
                          int64_t prev_number, int flags, uint8_t* hash32, uint8_t* check, uint8_t* link,
                          uint8_t* sig_ok_or_null) {
    if (int rc = check_suite(suite)) return rc;
    if (n == 0) return 0;
    if (!headers || !consensus || !hash32 || !check || !link) return set_err(BCOSGPU_E_ARG, "null pointer");
    const bcosgpu_ConsensusSet& cs = *consensus;
    if (int rc = check_consensus_set(cs)) return rc;
    HeadersStage st{headers, n, cs, prev_hash32_or_null, prev_number, flags};
    if (const char* bad = st.validate()) return set_err(BCOSGPU_E_ARG, bad);
    WsCall c;
    if (c.rc) return c.rc;
    Workspace* w = c.w;
    const ConsensusKeys keys(suite, cs, st.rows);
    st.plan(keys.slots);
    const HeadersStage::Plan& p = st.p;
    HIP_OK(w->h[0].ensure(p.total + 16));
    uint8_t* hs = w->h[0].as<uint8_t>();
    if (const char* bad = st.pack(hs)) return set_err(BCOSGPU_E_ARG, bad);
    const uint64_t work = headers_check_work_bytes(n, st.rows);
    HIP_OK(w->h[1].ensure(p.out_bytes + 16));
    HIP_OK(c.ensure({p.total + 16, work, p.out_bytes + 16}));
    HIP_OK(c.h2d(0, hs, p.total));
    uint8_t* ho = w->h[1].as<uint8_t>();
    HeadersCheckArgs a = st.args(c.buf(0), c.buf(2), c.buf<void>(1), work);
    if (int rc = run_rows(c, keys, st.cr, a, launch_headers_check, "headers check launch", ho, c.buf(2), p.out_bytes)) return rc;
    if (int rc = c.finish()) return rc;
    st.scatter(ho, hash32, check, link, sig_ok_or_null);
    return 0;
}

// ------------------------------------------------------------------ PBFT messages (pbft_kernels.hip)
uint64_t bcosgpu_pbft_check_work_size(size_t n, size_t rows) { return pbft_check_work_bytes(n, rows); }

int bcosgpu_pbft_check_dev(int suite, const uint8_t* d_data, const uint64_t* d_data_off, const uint8_t* d_given32,
                           const uint8_t* d_given_mask, const uint8_t* d_pre_flags, const uint64_t* d_msg_weight,
                           const uint8_t* d_checks, const int64_t* d_msg_row, const int64_t* d_prop_row,
                           const uint64_t* d_prep_off, const uint64_t* d_prep_row_off, size_t nprep,
                           uint8_t* d_row_hash32, const uint8_t* d_sig, const uint64_t* d_row_weight,
                           const int32_t* d_row_slot, const uint8_t* d_row_pub64, const uint64_t* d_groups,
                           size_t ngroups, uint64_t quorum, size_t n, size_t rows, uint8_t* d_msg_hash32,
                           uint32_t* d_msg_flags, uint8_t* d_prepared_check, uint8_t* d_sig_ok, void* d_work,
                           uint64_t work_bytes, void* stream) {
    if (int rc = check_suite(suite)) return rc;
    if (n == 0) return 0;
    if (!d_data || !d_data_off || !d_pre_flags || !d_checks || !d_msg_row || !d_prop_row || !d_prep_off ||
        !d_msg_hash32 || !d_msg_flags || !d_work || (nprep && (!d_prep_row_off || !d_prepared_check)) ||
        (rows && (!d_row_hash32 || !d_sig || !d_row_weight)) || (ngroups && (!d_groups || !d_msg_weight)))
        return set_err(BCOSGPU_E_ARG, "null pointer");
    if (rows && (d_row_slot != nullptr) == (d_row_pub64 != nullptr))
        return set_err(BCOSGPU_E_ARG, "exactly one of d_row_slot and d_row_pub64 must be given");
    PbftCheckArgs a;
    a.d_data = d_data, a.d_data_off = d_data_off, a.d_given32 = d_given32, a.d_given_mask = d_given_mask;
    a.d_pre_flags = d_pre_flags, a.d_msg_weight = d_msg_weight, a.d_checks = d_checks;
    a.d_msg_row = d_msg_row, a.d_prop_row = d_prop_row, a.d_prep_off = d_prep_off, a.d_prep_row_off = d_prep_row_off;
    a.nprep = nprep, a.d_row_hash32 = d_row_hash32, a.d_sig = d_sig, a.d_row_weight = d_row_weight;
    a.d_row_slot = d_row_slot, a.d_row_pub64 = d_row_pub64, a.d_groups = d_groups, a.ngroups = ngroups;
    a.quorum = quorum, a.n = n, a.rows = rows, a.d_msg_hash32 = d_msg_hash32, a.d_msg_flags = d_msg_flags;
    a.d_prepared_check = d_prepared_check, a.d_sig_ok = d_sig_ok, a.d_work = d_work, a.work_bytes = work_bytes;
    const int rc = launch_pbft_check(suite, a, as_stream(stream));
    if (rc == BCOSGPU_E_ARG)
        return set_err(rc, "work buffer too small, batch too large, or no key registered on this device");
    return rc ? hip_err(hipGetLastError(), "pbft check launch") : 0;
}

// The signature checks of a drained PBFT message queue (see bcos_gpu.h): every requested signature becomes a
// row (the proofs of all prepared proposals first, then the message and proposal signatures) with its node's
// key and weight, everything packed into pinned staging as one block (PbftStage, consensus_stage.h), one H2D,
// the four phases, one D2H.
int bcosgpu_pbft_check(int suite, const bcosgpu_PBFTMessageData* msgs, size_t n, const bcosgpu_PBFTGroup* groups,
                       size_t ngroups, const bcosgpu_ConsensusSet* consensus, int flags, uint8_t* msg_hash32,
                       uint32_t* msg_flags, uint8_t* prepared_check_or_null, uint8_t* sig_ok_or_null) {
    if (int rc = check_suite(suite)) return rc;
    if (flags) return set_err(BCOSGPU_E_ARG, "flags must be 0");
    if (n == 0) return 0;
    if (!msgs || !consensus || !msg_hash32 || !msg_flags || (ngroups && !groups))
        return set_err(BCOSGPU_E_ARG, "null pointer");
    const bcosgpu_ConsensusSet& cs = *consensus;
    if (int rc = check_consensus_set(cs)) return rc;
    PbftStage st{msgs, n, groups, ngroups, cs};
    if (const char* bad = st.validate()) return set_err(BCOSGPU_E_ARG, bad);
    WsCall c;
    if (c.rc) return c.rc;
    Workspace* w = c.w;
    const ConsensusKeys keys(suite, cs, st.rows);
    st.plan(keys.slots);
    const PbftStage::Plan& p = st.p;
    HIP_OK(w->h[0].ensure(p.total + 16));
    uint8_t* hs = w->h[0].as<uint8_t>();
    st.pack(hs);
    const uint64_t work = pbft_check_work_bytes(n, st.rows);
    HIP_OK(w->h[1].ensure(p.out_bytes + 16));
    HIP_OK(c.ensure({p.total + 16, work, p.out_bytes + 16}));
    HIP_OK(c.h2d(0, hs, p.total));
    uint8_t* ho = w->h[1].as<uint8_t>();
    PbftCheckArgs a = st.args(c.buf(0), c.buf(2), c.buf<void>(1), work);
    if (int rc = run_rows(c, keys, st.cr, a, launch_pbft_check, "pbft check launch", ho, c.buf(2), p.out_bytes)) return rc;
    if (int rc = c.finish()) return rc;
    st.scatter(hs, ho, msg_hash32, msg_flags, prepared_check_or_null, sig_ok_or_null);
    return 0;
}

// ------------------------------------------------------------------ Merkle proofs
uint64_t bcosgpu_merkle_proof_stride(uint64_t n, int width) {
    if (width < 2 || width > 64 || n == 0) return 0;
    return merkle_proof_stride(n, width);
}

int bcosgpu_merkle_proofs_dev(int width, const uint8_t* d_leaves32, size_t n, const uint8_t* d_tree,
                              const uint64_t* d_index, size_t m, uint8_t* d_proofs, uint32_t* d_proof_len, void* stream) {
    if (int rc = check_width(width)) return rc;
    if (n == 0) return set_err(BCOSGPU_E_EMPTY, "Empty input");
    if (m && (!d_leaves32 || !d_tree || !d_index || !d_proofs || !d_proof_len)) return set_err(BCOSGPU_E_ARG, "null pointer");
    int rc = launch_merkle_proofs(width, d_leaves32, n, d_tree, d_index, m, d_proofs, d_proof_len, as_stream(stream));
    return rc ? hip_err(hipGetLastError(), "merkle proofs launch") : 0;
}

int bcosgpu_merkle_proofs(int hasher, int width, const uint8_t* leaves32, size_t n, const uint64_t* index, size_t m,
                          uint8_t* proofs, uint32_t* proof_len) {
    if (int rc = check_hasher(hasher)) return rc;
    if (int rc = check_width(width)) return rc;
    if (n == 0) return set_err(BCOSGPU_E_EMPTY, "Empty input");
    if (m == 0) return 0;
    if (!leaves32 || !index || !proofs || !proof_len) return set_err(BCOSGPU_E_ARG, "null pointer");
    for (size_t q = 0; q < m; ++q)
        if (index[q] >= n) return set_err(BCOSGPU_E_ARG, "Out of range!");  // Merkle.h:124-127
    const uint64_t stride = merkle_proof_stride(n, width), tree = bcosgpu_merkle_size(n, width);
    WsCall c;
    if (c.rc) return c.rc;
    HIP_OK(c.ensure({n * 32, tree * 32 + 32, m * 8, m * stride * 32, m * 4}));
    HIP_OK(c.h2d(0, leaves32, n * 32));
    HIP_OK(c.h2d(2, index, m * 8));
    if (launch_merkle(hasher, width, c.buf(0), n, c.buf(1), nullptr, c.stream()) ||
        launch_merkle_proofs(width, c.buf(0), n, c.buf(1), c.buf<uint64_t>(2), m, c.buf(3), c.buf<uint32_t>(4), c.stream()))
        return hip_err(hipGetLastError(), "merkle proofs launch");
    HIP_OK(c.d2h(proofs, 3, m * stride * 32));
    HIP_OK(c.d2h(proof_len, 4, m * 4));
    return c.finish();
}

int bcosgpu_merkle_verify_proofs_dev(int hasher, const uint8_t* d_proofs, uint64_t stride, const uint32_t* d_proof_len,
                                     const uint8_t* d_hashes32, const uint8_t* d_roots32, int per_proof_root, size_t m,
                                     uint8_t* d_ok, void* stream) {
    if (int rc = check_hasher(hasher)) return rc;
    if (stride == 0 || stride > 0xFFFFFFFFull) return set_err(BCOSGPU_E_ARG, "bad proof stride");
    if (m && (!d_proofs || !d_proof_len || !d_hashes32 || !d_roots32 || !d_ok)) return set_err(BCOSGPU_E_ARG, "null pointer");
    int rc = launch_merkle_verify(hasher, d_proofs, stride, d_proof_len, d_hashes32, d_roots32, per_proof_root ? 1 : 0, m,
                                  d_ok, as_stream(stream));
    return rc ? hip_err(hipGetLastError(), "merkle verify launch") : 0;
}

int bcosgpu_merkle_verify_proofs(int hasher, const uint8_t* proofs, uint64_t stride, const uint32_t* proof_len,
                                 const uint8_t* hashes32, const uint8_t* roots32, int per_proof_root, size_t m, uint8_t* ok) {
    if (int rc = check_hasher(hasher)) return rc;
    if (stride == 0 || stride > 0xFFFFFFFFull) return set_err(BCOSGPU_E_ARG, "bad proof stride");
    if (m == 0) return 0;
    if (!proofs || !proof_len || !hashes32 || !roots32 || !ok) return set_err(BCOSGPU_E_ARG, "null pointer");
    WsCall c;
    if (c.rc) return c.rc;
    const size_t nroots = per_proof_root ? m : 1;
    HIP_OK(c.ensure({m * stride * 32, m * 4, m * 32, nroots * 32, m}));
    HIP_OK(c.h2d(0, proofs, m * stride * 32));
    HIP_OK(c.h2d(1, proof_len, m * 4));
    HIP_OK(c.h2d(2, hashes32, m * 32));
    HIP_OK(c.h2d(3, roots32, nroots * 32));
    if (launch_merkle_verify(hasher, c.buf(0), stride, c.buf<uint32_t>(1), c.buf(2), c.buf(3), per_proof_root ? 1 : 0, m,
                             c.buf(4), c.stream()))
        return hip_err(hipGetLastError(), "merkle verify launch");
    HIP_OK(c.d2h(ok, 4, m));
    return c.finish();
}

// ------------------------------------------------------------------ signatures
int bcosgpu_secp256k1_recover_batch_dev(const uint8_t* d_hash32, const uint8_t* d_sig65, size_t n,
                                        uint8_t* d_pub64, uint8_t* d_addr20, uint8_t* d_ok,
                                        void* stream) {
    if (n && (!d_hash32 || !d_sig65 || !d_ok)) return set_err(BCOSGPU_E_ARG, "null pointer");
    int rc = launch_secp256k1_recover(d_hash32, d_sig65, 65, n, d_pub64, d_addr20, d_ok, as_stream(stream));
    return rc ? set_err(rc, "secp256k1 recover launch failed") : 0;
}

int bcosgpu_secp256k1_recover_batch(const uint8_t* hash32, const uint8_t* sig65, size_t n,
                                    uint8_t* pub64, uint8_t* addr20, uint8_t* ok) {
    if (n == 0) return 0;
    if (!hash32 || !sig65 || !ok) return set_err(BCOSGPU_E_ARG, "null pointer");
    int dev = 0;
    if (int rc = calling_device(&dev)) return rc;
    SigJob job = sig_job(kSigJobRecoverK1, n, hash32, sig65, 65, nullptr, pub64, addr20, ok);
    return run_job(dev, job);
}

int bcosgpu_sm2_verify_batch_dev(const uint8_t* d_hash32, const uint8_t* d_sig128, size_t n,
                                 uint8_t* d_addr20, uint8_t* d_ok, void* stream) {
    if (n && (!d_hash32 || !d_sig128 || !d_ok)) return set_err(BCOSGPU_E_ARG, "null pointer");
    int rc = launch_sm2_verify(d_hash32, d_sig128, 128, n, d_addr20, d_ok, as_stream(stream));
    return rc ? set_err(rc, "sm2 verify launch failed") : 0;
}

int bcosgpu_sm2_verify_batch(const uint8_t* hash32, const uint8_t* sig128, size_t n,
                             uint8_t* addr20, uint8_t* ok) {
    if (n == 0) return 0;
    if (!hash32 || !sig128 || !ok) return set_err(BCOSGPU_E_ARG, "null pointer");
    int dev = 0;
    if (int rc = calling_device(&dev)) return rc;
    SigJob job = sig_job(kSigJobVerifySM2, n, hash32, sig128, 128, nullptr, nullptr, addr20, ok);
    return run_job(dev, job);
}

int bcosgpu_secp256k1_sign_batch_dev(const uint8_t* d_sk32, const uint8_t* d_hash32, size_t n,
                                     uint8_t* d_pub64, uint8_t* d_sig65, uint8_t* d_ok, void* stream) {
    if (n && (!d_sk32 || !d_hash32 || !d_sig65 || !d_ok)) return set_err(BCOSGPU_E_ARG, "null pointer");
    int rc = launch_secp256k1_sign(d_sk32, d_hash32, n, d_pub64, d_sig65, d_ok, as_stream(stream));
    return rc ? set_err(rc, "secp256k1 sign launch failed") : 0;
}

int bcosgpu_sm2_sign_batch_dev(const uint8_t* d_sk32, const uint8_t* d_hash32, size_t n,
                               uint8_t* d_sig128, uint8_t* d_ok, void* stream) {
    if (n && (!d_sk32 || !d_hash32 || !d_sig128 || !d_ok)) return set_err(BCOSGPU_E_ARG, "null pointer");
    int rc = launch_sm2_sign(d_sk32, d_hash32, n, d_sig128, d_ok, as_stream(stream));
    return rc ? set_err(rc, "sm2 sign launch failed") : 0;
}

// ------------------------------------------------------------------ verify with a known key, ecRecover
int bcosgpu_verify_batch_dev(int suite, const uint8_t* d_pub64, const uint8_t* d_hash32, const uint8_t* d_sig,
                             size_t sig_stride, size_t n, uint8_t* d_ok, void* stream) {
    if (int rc = check_suite(suite)) return rc;
    if (int rc = check_stride(sig_stride)) return rc;
    if (n && (!d_pub64 || !d_hash32 || !d_sig || !d_ok)) return set_err(BCOSGPU_E_ARG, "null pointer");
    int rc = launch_sig_verify(suite, d_pub64, d_hash32, d_sig, static_cast<uint32_t>(sig_stride), n, d_ok,
                               as_stream(stream));
    return rc ? set_err(rc, "verify launch failed") : 0;
}

int bcosgpu_verify_batch(int suite, const uint8_t* pub64, const uint8_t* hash32, const uint8_t* sig,
                         size_t sig_stride, size_t n, uint8_t* ok) {
    if (int rc = check_suite(suite)) return rc;
    if (int rc = check_stride(sig_stride)) return rc;
    if (n == 0) return 0;
    if (!pub64 || !hash32 || !sig || !ok) return set_err(BCOSGPU_E_ARG, "null pointer");
    int dev = 0;
    if (int rc = calling_device(&dev)) return rc;
    SigJob job = sig_job(suite == BCOSGPU_SUITE_SM2 ? kSigJobVerifySM2 : kSigJobVerifyK1, n, hash32, sig, sig_stride, pub64,
                         nullptr, nullptr, ok);
    return run_job(dev, job);
}

// ------------------------------------------------------------------ registered keys (ecc_keyed.hip)
int bcosgpu_register_keys(int device, int suite, const uint8_t* pub64, size_t n, int32_t* slots) {
    if (int rc = check_suite(suite)) return rc;
    if (n && (!pub64 || !slots)) return set_err(BCOSGPU_E_ARG, "null pointer");
    if (int rc = ready_device(device)) return rc;
    DeviceScope on(device);
    if (on.err != hipSuccess) return set_err(BCOSGPU_E_HIP, "hipSetDevice failed");
    if (int rc = keyed_register(suite, pub64, n, slots)) return set_err(rc, "key table build failed");
    int cached = 0;
    for (size_t i = 0; i < n; ++i) cached += slots[i] >= 0;
    return cached;
}

int bcosgpu_verify_keyed_batch_dev(int suite, const int32_t* d_slots, const uint8_t* d_hash32, const uint8_t* d_sig,
                                   size_t sig_stride, size_t n, uint8_t* d_ok, void* stream) {
    if (int rc = check_suite(suite)) return rc;
    if (int rc = check_stride(sig_stride)) return rc;
    if (n && (!d_slots || !d_hash32 || !d_sig || !d_ok)) return set_err(BCOSGPU_E_ARG, "null pointer");
    const int rc = launch_sig_verify_keyed(suite, d_slots, d_hash32, d_sig, static_cast<uint32_t>(sig_stride), n, d_ok,
                                           nullptr, as_stream(stream));
    return rc ? set_err(rc, rc == BCOSGPU_E_ARG ? "no key registered on this device" : "keyed verify launch failed") : 0;
}

int bcosgpu_key_cache_info(int device, int suite, int64_t* out5) {
    if (int rc = check_suite(suite)) return rc;
    if (!out5) return set_err(BCOSGPU_E_ARG, "null pointer");
    const int rc = keyed_cache_info(device, suite, out5);
    return rc ? set_err(rc, "bad device") : 0;
}

int bcosgpu_clear_keys(int device, int suite) {
    if (int rc = check_suite(suite)) return rc;
    const int rc = keyed_clear(device, suite);
    return rc ? set_err(rc, "clearing the key cache failed") : 0;
}

int bcosgpu_ecrecover_batch_dev(const uint8_t* d_in128, size_t n, uint8_t* d_out32, uint8_t* d_ok, void* stream) {
    if (n && (!d_in128 || !d_out32 || !d_ok)) return set_err(BCOSGPU_E_ARG, "null pointer");
    int rc = launch_ecrecover(d_in128, n, d_out32, d_ok, as_stream(stream));
    return rc ? set_err(rc, "ecrecover launch failed") : 0;
}

int bcosgpu_ecrecover_batch(const uint8_t* in128, size_t n, uint8_t* out32, uint8_t* ok) {
    if (n == 0) return 0;
    if (!in128 || !out32 || !ok) return set_err(BCOSGPU_E_ARG, "null pointer");
    WsCall c;
    if (c.rc) return c.rc;
    HIP_OK(c.ensure({n * 128, n * 32, n}));
    HIP_OK(c.h2d(0, in128, n * 128));
    if (int rc = launch_ecrecover(c.buf(0), n, c.buf(1), c.buf(2), c.stream())) return set_err(rc, "ecrecover launch failed");
    HIP_OK(c.d2h(out32, 1, n * 32));
    HIP_OK(c.d2h(ok, 2, n));
    return c.finish();
}

// ------------------------------------------------------------------ whole-tx admission
int bcosgpu_tx_verify_batch_dev(int suite, const uint8_t* d_pre, const uint64_t* d_pre_off,
                                const uint8_t* d_sig, const uint64_t* d_sig_off, size_t n,
                                uint8_t* d_txhash32, uint8_t* d_sender20, uint8_t* d_status,
                                void* stream) {
    if (int rc = check_suite(suite)) return rc;
    if (n && (!d_pre || !d_pre_off || !d_sig || !d_sig_off || !d_txhash32 || !d_sender20 || !d_status))
        return set_err(BCOSGPU_E_ARG, "null pointer");
    int rc = launch_tx_verify(suite, d_pre, d_pre_off, d_sig, d_sig_off, n, d_txhash32, d_sender20, d_status,
                              as_stream(stream));
    return rc ? set_err(rc, "tx verify launch failed") : 0;
}

// The batch site TransactionSync::importDownloadedTxs (TransactionSync.cpp:516-548) holds host memory:
// the chunked copy / compute pipeline of txpipe.hip on a pipeline of the calling thread's device (its own
// streams and buffers: concurrent callers overlap).
int bcosgpu_tx_verify_batch(int suite, const uint8_t* pre, const uint64_t* pre_off,
                            const uint8_t* sig, const uint64_t* sig_off, size_t n,
                            uint8_t* txhash32, uint8_t* sender20, uint8_t* status) {
    if (int rc = check_suite(suite)) return rc;
    if (n == 0) return 0;
    if (!pre || !pre_off || !sig || !sig_off || !txhash32 || !sender20 || !status)
        return set_err(BCOSGPU_E_ARG, "null pointer");
    int dev = 0;  // (the offsets are checked by the pipeline, chunk by chunk)
    if (int rc = calling_device(&dev)) return rc;
    TxPipe* p = tx_pipe_acquire(dev);
    if (!p) return hip_err(hipGetLastError(), "tx pipeline setup");
    std::string msg;
    const HostTxRange t = host_range(suite, pre, pre_off, sig, sig_off, 0, n, txhash32, sender20, status);
    const int rc = tx_pipeline(*p, t, nullptr, msg);
    tx_pipe_release(p);
    return rc ? set_err(rc, msg) : 0;
}

// ------------------------------------------------------------------ Tars-encoded transactions
uint64_t bcosgpu_tars_decode_work_size(size_t n) { return tars_decode_work_bytes(n); }

int bcosgpu_tars_tx_decode_dev(const uint8_t* d_enc, const uint64_t* d_enc_off, size_t n, uint8_t* d_pre,
                               uint64_t* d_pre_off, uint8_t* d_sig, uint64_t* d_sig_off, uint8_t* d_dec_status,
                               void* d_work, uint64_t work_bytes, void* stream) {
    if (n == 0) return 0;
    if (!d_enc || !d_enc_off || !d_pre || !d_pre_off || !d_sig || !d_sig_off || !d_work)
        return set_err(BCOSGPU_E_ARG, "null pointer");
    int rc = launch_tars_tx_decode(d_enc, d_enc_off, n, d_pre, d_pre_off, d_sig, d_sig_off, d_dec_status, d_work,
                                   work_bytes, as_stream(stream));
    if (rc == BCOSGPU_E_ARG) return set_err(rc, "work buffer too small or batch too large");
    return rc ? hip_err(hipGetLastError(), "tars decode launch") : 0;
}

int bcosgpu_tars_tx_verify_batch_dev(int suite, const uint8_t* d_enc, const uint64_t* d_enc_off, size_t n,
                                     int check_sig, int check_hash, uint8_t* d_pre, uint64_t* d_pre_off, uint8_t* d_sig,
                                     uint64_t* d_sig_off, void* d_work, uint64_t work_bytes, uint8_t* d_txhash32,
                                     uint8_t* d_sender20, uint8_t* d_status, void* stream) {
    if (int rc = check_suite(suite)) return rc;
    if (n == 0) return 0;
    if (!d_enc || !d_enc_off || !d_pre || !d_pre_off || !d_sig || !d_sig_off || !d_work || !d_txhash32 ||
        !d_sender20 || !d_status)
        return set_err(BCOSGPU_E_ARG, "null pointer");
    hipStream_t st = as_stream(stream);
    int rc = launch_tars_tx_decode(d_enc, d_enc_off, n, d_pre, d_pre_off, d_sig, d_sig_off, nullptr, d_work,
                                   work_bytes, st);
    if (rc == BCOSGPU_E_ARG) return set_err(rc, "work buffer too small or batch too large");
    if (!rc && check_sig) {
        rc = launch_tx_verify(suite, d_pre, d_pre_off, d_sig, d_sig_off, n, d_txhash32, d_sender20, d_status, st);
    } else if (!rc) {  // checkSig = false: decode + hash only (TransactionFactoryImpl.h:52-60)
        rc = launch_hash_batch(suite == BCOSGPU_SUITE_SM2 ? BCOSGPU_SM3 : BCOSGPU_KECCAK256, d_pre, d_pre_off, n,
                               d_txhash32, st);
        if (!rc && (hipMemsetAsync(d_sender20, 0, 20 * n, st) != hipSuccess ||
                    hipMemsetAsync(d_status, 0, n, st) != hipSuccess))
            rc = BCOSGPU_E_HIP;
    }
    if (!rc) rc = launch_tars_finish(d_enc, d_work, nullptr, d_txhash32, d_status, n, check_hash, st);
    return rc ? hip_err(hipGetLastError(), "tars tx verify launch") : 0;
}

int bcosgpu_tars_tx_verify_batch(int suite, const uint8_t* enc, const uint64_t* enc_off, size_t n, int check_sig,
                                 int check_hash, uint8_t* txhash32, uint8_t* sender20, uint8_t* status) {
    if (int rc = check_suite(suite)) return rc;
    if (n == 0) return 0;
    if (!enc || !enc_off || !txhash32 || !sender20 || !status) return set_err(BCOSGPU_E_ARG, "null pointer");
    for (size_t i = 0; i < n; ++i)
        if (enc_off[i + 1] < enc_off[i]) return set_err(BCOSGPU_E_ARG, "offsets must be non-decreasing");
    const uint64_t base = enc_off[0], bytes = enc_off[n] - base;
    std::vector<uint64_t> off(n + 1);  // (declared before the call: the drain runs while it is alive)
    for (size_t i = 0; i <= n; ++i) off[i] = enc_off[i] - base;
    WsCall c;
    if (c.rc) return c.rc;
    const uint64_t work = tars_decode_work_bytes(n);
    // encoded txs, their offsets | preimages, preimage + signature offsets, signatures | txhash, sender, status | work
    HIP_OK(c.ensure({bytes + 8, (n + 1) * 8, bytes + 12 * n + 8, 2 * (n + 1) * 8, bytes + 8, n * 53, work}));
    HIP_OK(c.h2d(0, enc + base, bytes));
    HIP_OK(c.h2d(1, off.data(), (n + 1) * 8));
    uint64_t* pre_off = c.buf<uint64_t>(3);
    uint8_t* out = c.buf(5);
    if (int rc = bcosgpu_tars_tx_verify_batch_dev(suite, c.buf(0), c.buf<uint64_t>(1), n, check_sig, check_hash, c.buf(2),
                                                  pre_off, c.buf(4), pre_off + (n + 1), c.buf<void>(6), work, out,
                                                  out + 32 * n, out + 52 * n, c.stream()))
        return rc;
    HIP_OK(hipMemcpyAsync(txhash32, out, n * 32, hipMemcpyDeviceToHost, c.stream()));
    HIP_OK(hipMemcpyAsync(sender20, out + 32 * n, n * 20, hipMemcpyDeviceToHost, c.stream()));
    HIP_OK(hipMemcpyAsync(status, out + 52 * n, n, hipMemcpyDeviceToHost, c.stream()));
    return c.finish();
}

// ------------------------------------------------------------------ single calls (coalesced)
int bcosgpu_secp256k1_recover(int device, const uint8_t* hash32, const uint8_t* sig, size_t sig_len, uint8_t* pub64) {
    if (!hash32 || !sig || !pub64) return set_err(BCOSGPU_E_ARG, "null pointer");
    if (int rc = ready_device(device)) return rc;
    if (sig_len != 65) {  // SECP256K1_SIGNATURE_LEN (Secp256k1Crypto.h:29): InvalidSignature
        std::memset(pub64, 0, 64);
        return 0;
    }
    uint8_t ok = 0;
    SigJob job = sig_job(kSigJobRecoverK1, 1, hash32, sig, 65, nullptr, pub64, nullptr, &ok);
    if (int rc = run_job(device, job)) return rc;
    return ok ? 1 : 0;
}

int bcosgpu_secp256k1_verify(int device, const uint8_t* pub64, const uint8_t* hash32, const uint8_t* sig,
                             size_t sig_len) {
    if (!pub64 || !hash32 || !sig) return set_err(BCOSGPU_E_ARG, "null pointer");
    if (int rc = ready_device(device)) return rc;
    if (sig_len < 64) return 0;
    uint8_t ok = 0;
    SigJob job = sig_job(kSigJobVerifyK1, 1, hash32, sig, 64, pub64, nullptr, nullptr, &ok);
    if (int rc = run_job(device, job)) return rc;
    return ok ? 1 : 0;
}

int bcosgpu_sm2_verify(int device, const uint8_t* pub64, const uint8_t* hash32, const uint8_t* sig64) {
    if (!pub64 || !hash32 || !sig64) return set_err(BCOSGPU_E_ARG, "null pointer");
    if (int rc = ready_device(device)) return rc;
    uint8_t ok = 0;
    SigJob job = sig_job(kSigJobVerifySM2, 1, hash32, sig64, 64, pub64, nullptr, nullptr, &ok);
    if (int rc = run_job(device, job)) return rc;
    return ok ? 1 : 0;
}

int bcosgpu_coalesce_stats(int device, uint64_t* out10, int reset) {
    if (!out10) return set_err(BCOSGPU_E_ARG, "null pointer");
    const int rc = coalesce_stats(device, out10, 10, reset);
    return rc ? set_err(rc, "bad device") : 0;
}

// ------------------------------------------------------------------ wedpr-ABI shims
// On the calling thread's current device.  0 = WEDPR_SUCCESS, -1 = WEDPR_ERROR (invalid input or
// signature), BCOSGPU_WEDPR_ENGINE_ERROR = the engine failed (no device, HIP error): the message is in
// bcosgpu_last_error().
static int shim_device() {
    int dev = 0;
    return current_device(&dev) ? -1 : dev;
}

int8_t bcosgpu_wedpr_secp256k1_recover_public_key(const bcosgpu_CInputBuffer* hash,
                                                   const bcosgpu_CInputBuffer* sig,
                                                   bcosgpu_COutputBuffer* pub) {
    if (!hash || !sig || !pub || hash->len != 32 || pub->len < 64) return -1;
    const int dev = shim_device();
    if (dev < 0) return BCOSGPU_WEDPR_ENGINE_ERROR;
    const int rc = bcosgpu_secp256k1_recover(dev, reinterpret_cast<const uint8_t*>(hash->data),
                                             reinterpret_cast<const uint8_t*>(sig->data), sig->len,
                                             reinterpret_cast<uint8_t*>(pub->data));
    return rc < 0 ? BCOSGPU_WEDPR_ENGINE_ERROR : rc == 1 ? 0 : -1;
}

int8_t bcosgpu_wedpr_sm2_verify(const bcosgpu_CInputBuffer* pub, const bcosgpu_CInputBuffer* hash,
                                 const bcosgpu_CInputBuffer* sig) {
    if (!pub || !hash || !sig || hash->len != 32 || sig->len != 64 || pub->len != 64) return -1;
    const int dev = shim_device();
    if (dev < 0) return BCOSGPU_WEDPR_ENGINE_ERROR;
    const int rc = bcosgpu_sm2_verify(dev, reinterpret_cast<const uint8_t*>(pub->data),
                                      reinterpret_cast<const uint8_t*>(hash->data),
                                      reinterpret_cast<const uint8_t*>(sig->data));
    return rc < 0 ? BCOSGPU_WEDPR_ENGINE_ERROR : rc == 1 ? 0 : -1;
}

int8_t bcosgpu_wedpr_secp256k1_verify(const bcosgpu_CInputBuffer* pub, const bcosgpu_CInputBuffer* hash,
                                      const bcosgpu_CInputBuffer* sig) {
    if (!pub || !hash || !sig || hash->len != 32 || pub->len != 64 || sig->len < 64) return -1;
    const int dev = shim_device();
    if (dev < 0) return BCOSGPU_WEDPR_ENGINE_ERROR;
    const int rc = bcosgpu_secp256k1_verify(dev, reinterpret_cast<const uint8_t*>(pub->data),
                                            reinterpret_cast<const uint8_t*>(hash->data),
                                            reinterpret_cast<const uint8_t*>(sig->data), sig->len);
    return rc < 0 ? BCOSGPU_WEDPR_ENGINE_ERROR : rc == 1 ? 0 : -1;
}

}  // extern "C"
