// cipher_kernels.hip -- the storage cipher: AES-256-CBC and SM4-CBC over a batch of storage values under one
// key (gfx950).
//
// Replaces, for the values of a block commit or a batched read with storage_security.enable=true:
//   RocksDBStorage::asyncPrepare    bcos-storage/bcos-storage/RocksDBStorage.cpp:348-353   encrypt, one by one
//   RocksDBStorage::setRows         :513-524                                               encrypt, parallel_for
//   RocksDBStorage::asyncGetRow     :106-108                                               decrypt
//   RocksDBStorage::asyncGetRows    :204-205                                               decrypt
//   DataEncryption::encrypt/decrypt bcos-security/bcos-security/DataEncryption.cpp:143-165
//   AESCrypto / SM4Crypto           bcos-crypto/bcos-crypto/encrypt/AESCrypto.cpp:29-51, SM4Crypto.cpp:28-49
// The key, IV, padding and failure rules, the stated deviation (a default IV from a key shorter than 16 bytes
// is zero-filled, where the reference reads past the caller's buffer) and the unpinned parity are in
// cipher_host.h's header comment.
//
// Encryption: CBC chains a value's blocks, so one lane owns one value.  The round keys and the IV are the same
// for every lane and arrive by value in the kernel arguments (SGPRs), the tables sit in LDS (cipher_device.h).
// Input is the packed layout, values back to back at any byte offset, off[n+1]; output offsets are 16 times the
// running sum of the values' block counts (two small kernels sum the counts per workgroup and scan the sums,
// the encrypt kernel finishes the scan and writes out_off), the output base is 16-byte aligned and every
// ciphertext block leaves as one 16-byte store.  A wave costs its longest value: a value longer than
// kCipherLongBytes is not run in place but listed (an atomicAdd on a count the launcher zeroes on the stream),
// and a second launch of the same kernel runs the list, so long values share waves.
//
// Decryption: P_j = D(C_j) ^ C_{j-1} needs no chain, so one lane owns one 16-byte block; it finds its item by
// a binary search of its byte offset in off[].  Offsets are multiples of 16 (this build's own ciphertext
// layout).  The lane that holds an item's last block sees the whole padding (p <= 16): it alone checks it and
// writes the item's out_len and status.  The plaintext lands at the item's input offset, padding included.
// The grid is fixed (the block count is on the device) and strides over the blocks.
#include <cstdlib>
#include "cipher_device.h"
#include "engine.h"

namespace bcosgpu {

namespace {

using cipher::kAes256;
using cipher::kSm4;

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d) {
    const uint32_t lo = static_cast<uint32_t>(__shfl_up(static_cast<int>(static_cast<uint32_t>(v)), d, 64));
    const uint32_t hi = static_cast<uint32_t>(__shfl_up(static_cast<int>(static_cast<uint32_t>(v >> 32)), d, 64));
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

// exclusive scan of v over the workgroup (every thread calls it); *total: the workgroup's sum
__device__ __forceinline__ uint64_t block_exclusive_scan(uint64_t v, uint64_t* total) {
    __shared__ uint64_t wave_sum[kCipherThreads / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = shfl_up64(inc, d);
        if (lane >= static_cast<uint32_t>(d)) inc += o;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    uint64_t base = 0, sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < kCipherThreads / 64; ++w) {
        if (w < wave) base += wave_sum[w];
        sum += wave_sum[w];
    }
    *total = sum;
    return base + inc - v;
}

__device__ __forceinline__ uint64_t value_blocks(const uint64_t* __restrict__ off, uint64_t i) {
    return ((off[i + 1] - off[i]) >> 4) + 1;
}

// sums[g] = the ciphertext blocks of workgroup g's 256 values
__global__ __launch_bounds__(kCipherThreads) void cbc_block_sums_kernel(const uint64_t* __restrict__ off, uint64_t n,
                                                                        uint64_t* __restrict__ sums) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kCipherThreads + threadIdx.x;
    uint64_t total;
    (void)block_exclusive_scan(i < n ? value_blocks(off, i) : 0, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums[0..rows) -> its exclusive scan in place (one workgroup, a contiguous chunk per thread)
__global__ __launch_bounds__(kCipherThreads) void cbc_scan_sums_kernel(uint64_t* __restrict__ sums, uint64_t rows) {
    const uint64_t chunk = (rows + kCipherThreads - 1) / kCipherThreads;
    const uint64_t lo = chunk * threadIdx.x < rows ? chunk * threadIdx.x : rows;
    const uint64_t hi = lo + chunk < rows ? lo + chunk : rows;
    uint64_t mine = 0, total;
    for (uint64_t r = lo; r < hi; ++r) mine += sums[r];
    uint64_t run = block_exclusive_scan(mine, &total);
    for (uint64_t r = lo; r < hi; ++r) {
        const uint64_t v = sums[r];
        sums[r] = run;
        run += v;
    }
}

// one value through CBC: out = its first ciphertext block
template <int CIPHER>
__device__ __forceinline__ void cbc_encrypt_value(const cipher::Schedule& ck, const CipherTable& tab,
                                                  const uint8_t* __restrict__ p, uint32_t len,
                                                  uint4* __restrict__ out) {
    const CipherBlockReader rd(p, len);
    const uint32_t blocks = (len >> 4) + 1u;
    uint32_t c[4] = {ck.iv[0], ck.iv[1], ck.iv[2], ck.iv[3]};
#pragma unroll 1
    for (uint32_t j = 0; j < blocks; ++j) {
        uint32_t w[4];
        rd.block(j, w);
        cipher_swap_words<CIPHER>(w);
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] ^= w[k];
        if (CIPHER == kSm4) sm4_crypt_dev(ck, tab, c);
        else aes256_encrypt_dev(ck, tab, c);
        uint32_t o[4] = {c[0], c[1], c[2], c[3]};
        cipher_swap_words<CIPHER>(o);
        out[j] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// LIST false: lane t runs value t, or appends it to long_list when it is longer than long_len; it also writes
// out_off[t] (and the last lane out_off[n]) from the scanned workgroup sums in `base`.
// LIST true: lane t runs value long_list[t], t < *long_count; a workgroup past the count leaves at once.
template <int CIPHER, bool LIST>
__global__ __launch_bounds__(kCipherThreads) void cbc_encrypt_kernel(const cipher::Schedule ck,
                                                                     const uint8_t* __restrict__ data,
                                                                     const uint64_t* __restrict__ off, uint64_t n,
                                                                     const uint64_t* __restrict__ base,
                                                                     uint32_t long_len, uint32_t* __restrict__ long_count,
                                                                     uint32_t* __restrict__ long_list,
                                                                     uint4* __restrict__ out,
                                                                     uint64_t* __restrict__ out_off) {
    __shared__ uint32_t lds_tab[kCipherTableWords];
    const uint64_t t = static_cast<uint64_t>(blockIdx.x) * kCipherThreads + threadIdx.x;
    uint64_t i = t, first_block = 0;
    bool run;
    if (LIST) {
        const uint64_t count = *long_count;
        if (static_cast<uint64_t>(blockIdx.x) * kCipherThreads >= count) return;  // (the whole workgroup)
        run = t < count;
        if (run) {
            i = long_list[t];
            first_block = out_off[i] >> 4;
        }
    } else {
        uint64_t total;
        run = t < n;
        const uint64_t mine = run ? value_blocks(off, t) : 0;
        first_block = base[blockIdx.x] + block_exclusive_scan(mine, &total);
        if (run) {
            out_off[t] = first_block << 4;
            if (t == n - 1) out_off[n] = (first_block + mine) << 4;
        }
    }
    cipher_fill_table(lds_tab, CIPHER == kSm4 ? kDevSm4T0 : kDevAesTe0);
    __syncthreads();
    if (!run) return;
    const uint64_t a = off[i];
    const uint32_t len = static_cast<uint32_t>(off[i + 1] - a);
    if (!LIST && len > long_len) {
        long_list[atomicAdd(long_count, 1u)] = static_cast<uint32_t>(i);
        return;
    }
    cbc_encrypt_value<CIPHER>(ck, CipherTable(lds_tab), data + a, len, out + first_block);
}

constexpr uint32_t kPadOk = cipher::kStatusOk, kPadBad = cipher::kStatusBadPadding, kBadLength = cipher::kStatusBadLength;

template <int CIPHER>
__global__ __launch_bounds__(kCipherThreads) void cbc_decrypt_kernel(const cipher::Schedule ck,
                                                                     const uint4* __restrict__ in,
                                                                     const uint64_t* __restrict__ off, uint64_t n,
                                                                     uint4* __restrict__ out,
                                                                     uint32_t* __restrict__ out_len,
                                                                     uint8_t* __restrict__ status) {
    __shared__ uint32_t lds_tab[kCipherTableWords];
    __shared__ uint8_t lds_isb[256];
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kCipherThreads;
    const uint64_t gt = static_cast<uint64_t>(blockIdx.x) * kCipherThreads + threadIdx.x;
    // an empty item has no block and so no lane of its own: bad length
    for (uint64_t i = gt; i < n; i += stride)
        if (off[i + 1] == off[i]) {
            status[i] = static_cast<uint8_t>(kBadLength);
            out_len[i] = 0;
        }
    const uint64_t first = off[0] >> 4, end = off[n] >> 4;
    if (first + static_cast<uint64_t>(blockIdx.x) * kCipherThreads >= end) return;  // (the whole workgroup)
    cipher_fill_table(lds_tab, CIPHER == kSm4 ? kDevSm4T0 : kDevAesTd0);
    if (CIPHER == kAes256) lds_isb[threadIdx.x] = kDevAesInvSbox.v[threadIdx.x];
    __syncthreads();
    const CipherTable tab(lds_tab);
#pragma unroll 1
    for (uint64_t t = first + gt; t < end; t += stride) {
        const uint64_t pos = t << 4;
        uint64_t lo = 0, hi = n;  // the last item with off[i] <= pos: the one item that is not empty there
        while (hi - lo > 1) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (off[mid] <= pos) lo = mid;
            else hi = mid;
        }
        const uint64_t a = off[lo], b = off[lo + 1];
        const uint4 cb = in[t];
        uint32_t c[4] = {cb.x, cb.y, cb.z, cb.w}, prev[4];
        if (pos <= a) {  // the item's first block (<: never with offsets that are multiples of 16)
            prev[0] = ck.iv[0], prev[1] = ck.iv[1], prev[2] = ck.iv[2], prev[3] = ck.iv[3];
        } else {
            const uint4 pb = in[t - 1];
            prev[0] = pb.x, prev[1] = pb.y, prev[2] = pb.z, prev[3] = pb.w;
            cipher_swap_words<CIPHER>(prev);
        }
        cipher_swap_words<CIPHER>(c);
        if (CIPHER == kSm4) sm4_crypt_dev(ck, tab, c);
        else aes256_decrypt_dev(ck, tab, lds_isb, c);
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] ^= prev[k];
        cipher_swap_words<CIPHER>(c);
        out[t] = make_uint4(c[0], c[1], c[2], c[3]);
        if (pos + 16 == b) {  // the item's last block: PKCS#7
            const uint32_t p = c[3] >> 24;
            bool ok = p >= 1u && p <= 16u;
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) {
                const uint32_t byte = (c[k >> 2] >> ((k & 3u) * 8u)) & 0xffu;
                if (k >= 16u - p && byte != p) ok = false;
            }
            status[lo] = static_cast<uint8_t>(ok ? kPadOk : kPadBad);
            out_len[lo] = ok ? static_cast<uint32_t>(b - a) - p : 0u;
        }
    }
}

uint64_t cipher_rows(uint64_t n) { return (n + kCipherThreads - 1) / kCipherThreads; }

// a value longer than this goes through the long list (up to 64 blocks stay in place)
constexpr uint32_t kCipherLongBytes = 1024;

// test only (tests/test_gpu_cipher.py runs the list at small sizes): BCOSGPU_CIPHER_LONG_BYTES, read per launch
uint32_t cipher_long_bytes() {
    const char* e = std::getenv("BCOSGPU_CIPHER_LONG_BYTES");
    if (!e || !*e) return kCipherLongBytes;
    char* end = nullptr;
    const unsigned long v = std::strtoul(e, &end, 10);
    return end && !*end && v <= 0xFFFFFFFFul ? static_cast<uint32_t>(v) : kCipherLongBytes;
}

}  // namespace

// d_work: the workgroups' block sums (uint64 each), the long list's count, the long list (a uint32 per value)
uint64_t cbc_work_bytes(uint64_t n) { return 8 * cipher_rows(n) + 32 + 4 * n + 32; }

int launch_cbc_encrypt(int cipher_id, const cipher::Schedule& ck, const uint8_t* d_in, const uint64_t* d_in_off,
                       uint64_t n, uint8_t* d_out, uint64_t* d_out_off, void* d_work, uint64_t work_bytes,
                       hipStream_t st) {
    if (n > 0xFFFFFFFFull || (n && work_bytes < cbc_work_bytes(n))) return BCOSGPU_E_ARG;
    if (n == 0) return 0;
    const uint64_t rows = cipher_rows(n);
    uint64_t* sums = static_cast<uint64_t*>(d_work);
    uint32_t* long_count = reinterpret_cast<uint32_t*>(sums + rows);
    uint32_t* long_list = long_count + 8;
    const uint32_t long_len = cipher_long_bytes();
    const dim3 g(static_cast<unsigned>(rows)), b(kCipherThreads);
    if (hipMemsetAsync(long_count, 0, 4, st) != hipSuccess) return BCOSGPU_E_HIP;
    hipLaunchKernelGGL(cbc_block_sums_kernel, g, b, 0, st, d_in_off, n, sums);
    hipLaunchKernelGGL(cbc_scan_sums_kernel, dim3(1), b, 0, st, sums, rows);
    uint4* out = reinterpret_cast<uint4*>(d_out);
#define CBC_ENCRYPT(C, LIST)                                                                                     \
    hipLaunchKernelGGL((cbc_encrypt_kernel<C, LIST>), g, b, 0, st, ck, d_in, d_in_off, n, sums, long_len, long_count, \
                       long_list, out, d_out_off)
    if (cipher_id == kSm4) {
        CBC_ENCRYPT(kSm4, false);
        CBC_ENCRYPT(kSm4, true);
    } else {
        CBC_ENCRYPT(kAes256, false);
        CBC_ENCRYPT(kAes256, true);
    }
#undef CBC_ENCRYPT
    return hipGetLastError() == hipSuccess ? 0 : BCOSGPU_E_HIP;
}

int launch_cbc_decrypt(int cipher_id, const cipher::Schedule& ck, const uint8_t* d_in, const uint64_t* d_in_off,
                       uint64_t n, uint8_t* d_out, uint32_t* d_out_len, uint8_t* d_status, hipStream_t st) {
    if (n > 0xFFFFFFFFull) return BCOSGPU_E_ARG;
    if (n == 0) return 0;
    const dim3 g(static_cast<unsigned>(8 * cu_count())), b(kCipherThreads);
    const uint4* in = reinterpret_cast<const uint4*>(d_in);
    uint4* out = reinterpret_cast<uint4*>(d_out);
    if (cipher_id == kSm4)
        hipLaunchKernelGGL(cbc_decrypt_kernel<kSm4>, g, b, 0, st, ck, in, d_in_off, n, out, d_out_len, d_status);
    else
        hipLaunchKernelGGL(cbc_decrypt_kernel<kAes256>, g, b, 0, st, ck, in, d_in_off, n, out, d_out_len, d_status);
    return hipGetLastError() == hipSuccess ? 0 : BCOSGPU_E_HIP;
}

}  // namespace bcosgpu
