// header_kernels.hip -- the block-header check for a run of headers: hash, parent link, quorum (gfx950).
//
// Replaces, for every downloaded block of a sync catch-up:
//   impl_calculate<Hasher>(bcostars::BlockHeader)   bcos-tars-protocol/bcos-tars-protocol/impl/TarsHashable.h:77-126
//   BlockValidator::asyncCheckBlock                  bcos-pbft/bcos-pbft/pbft/engine/BlockValidator.cpp:28-182
//     (caller: bcos-sync/bcos-sync/state/DownloadingQueue.cpp:407)
//   the ledger's parent check                        bcos-ledger/src/libledger/LedgerImpl.h:290-312
//
// Three phases on one stream (launch_headers_check):
//   header_hash_kernel<H>   one header per lane over the packed preimages of bcosgpu_pack_header_preimages
//                           (pack.cpp), with the one-lane hashers of hash_device.h.  The digest -- or the given
//                           hash of a header that came with a dataHash (TarsHashable.h:81-85) -- goes to hash32
//                           and to each of the header's signature rows in d_work, so that the known-key verify
//                           kernels read hash + 32 row unchanged.
//   the signatures          launch_sig_verify_keyed (slot ids of registered keys) or launch_sig_verify (keys in
//                           the rows), stride 64, into the row ok array.  Those kernels are used as they are.
//   header_verdict_kernel   one header per lane: folds the header's rows (all ok; the u64 sum of the row
//                           weights), merges the host's early verdict, writes check[] and link[].
//
// Row semantics are the reference's, even where they surprise (BlockValidator.cpp:149-180):
//   - a row whose index names no consensus node fails (getConsensusNodeByIndex, ConsensusConfig.cpp:150-158);
//     the host gives such a row a negative slot id, or a zero key and a zero signature;
//   - ONE failed row fails the block, even if the remaining weight would reach the quorum: code 19 (a signature
//     row failed) comes before code 20 (weight below the quorum);
//   - a sealer index that appears twice is counted twice: the reference sums per list entry and never
//     deduplicates, so neither does the fold.
// d_work holds the per-row hashes and, when the caller wants no row verdicts, the row ok array; every byte of it
// that is read is written by this call's kernels first, so its earlier contents never matter.
#include "hash_device.h"
#include "engine.h"

namespace bcosgpu {

namespace {

constexpr int kHeaderThreads = 64;  // one wave: a header of a 100-node sealer list is 7 KB, a wave costs its longest

template <int H>
__global__ __launch_bounds__(kHeaderThreads) void header_hash_kernel(
    const uint8_t* __restrict__ pre, const uint64_t* __restrict__ pre_off, const uint32_t* __restrict__ given,
    const uint8_t* __restrict__ given_mask, const uint64_t* __restrict__ sig_off, uint64_t n, uint64_t rows,
    uint32_t* __restrict__ hash, uint32_t* __restrict__ row_hash) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kHeaderThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t d[8];
    if (given && given_mask && given_mask[i]) {
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = given[8 * i + k];
    } else {
        const uint64_t a = pre_off[i], b = pre_off[i + 1];
        const uint32_t len = static_cast<uint32_t>(b - a);
        FlatReader rd(pre + a, len);
        uint32_t w[8];
        if (H == KECCAK256) keccak256_msg(rd, len, w);
        else sm3_msg(rd, len, w);
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = H == SM3 ? bswap32(w[k]) : w[k];  // memory order, as store_digest
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) hash[8 * i + k] = d[k];
    uint64_t r = sig_off[i], e = sig_off[i + 1];
    if (e > rows) e = rows;  // (a CSR that overruns `rows` writes nothing past the row arrays)
    for (; r < e; ++r) {
#pragma unroll
        for (int k = 0; k < 8; ++k) row_hash[8 * r + k] = d[k];
    }
}

__global__ __launch_bounds__(kHeaderThreads) void header_verdict_kernel(
    const uint8_t* __restrict__ pre_status, const int64_t* __restrict__ number,
    const int64_t* __restrict__ parent_number, const uint32_t* __restrict__ parent_hash,
    const uint8_t* __restrict__ parent_ok, const uint32_t* __restrict__ prev_hash, int64_t prev_number,
    const uint64_t* __restrict__ sig_off, const uint64_t* __restrict__ row_weight, const uint8_t* __restrict__ row_ok,
    uint64_t quorum, uint64_t n, uint64_t rows, const uint32_t* __restrict__ hash, uint8_t* __restrict__ check,
    uint8_t* __restrict__ link) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kHeaderThreads + threadIdx.x;
    if (i >= n) return;
    // BlockValidator.cpp:35-63 ran on the host (pre_status); :64-69 is the fold of the rows
    uint32_t code = pre_status[i];
    if (code == 0) {
        uint64_t r = sig_off[i], e = sig_off[i + 1];
        if (e > rows) e = rows;
        bool all = true;
        uint64_t weight = 0;  // size_t signatureWeight (:148): wraps as the reference's does
        for (; r < e; ++r) {
            all = all && row_ok[r] == 1;
            weight += row_weight[r];  // per list entry, duplicates included (:171)
        }
        code = !all ? BCOSGPU_HEADER_E_SIGNATURE : weight < quorum ? BCOSGPU_HEADER_E_QUORUM : BCOSGPU_HEADER_OK;
    }
    check[i] = static_cast<uint8_t>(code);
    // LedgerImpl.h:290-312
    uint32_t lk;
    const uint32_t* ph = i ? hash + 8 * (i - 1) : prev_hash;
    if (number[i] == 0 || !ph) {
        lk = BCOSGPU_LINK_UNCHECKED;  // :290, or nothing to compare the first header with
    } else if (!parent_ok[i] || parent_number[i] != (i ? number[i - 1] : prev_number)) {
        lk = BCOSGPU_LINK_BROKEN;  // :302-304
    } else {
        uint32_t diff = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) diff |= parent_hash[8 * i + k] ^ ph[k];
        lk = diff ? BCOSGPU_LINK_BROKEN : BCOSGPU_LINK_OK;  // :305-306
    }
    link[i] = static_cast<uint8_t>(lk);
}

uint64_t align8(uint64_t x) { return (x + 7) & ~uint64_t{7}; }

}  // namespace

// d_work: the per-row hashes (32 bytes a row), then the row ok array (used when the caller passes none)
uint64_t headers_check_work_bytes(uint64_t n, uint64_t rows) {
    (void)n;
    return 32 * rows + align8(rows) + 32;
}

int launch_headers_check(int suite, const HeadersCheckArgs& a, hipStream_t st) {
    const uint64_t n = a.n, rows = a.rows;
    if (n == 0) return 0;
    if (n > 0xFFFFFFFFull || rows > 0xFFFFFFFFull || a.work_bytes < headers_check_work_bytes(n, rows))
        return BCOSGPU_E_ARG;
    if (rows && (a.d_row_slot != nullptr) == (a.d_row_pub64 != nullptr)) return BCOSGPU_E_ARG;
    uint32_t* row_hash = static_cast<uint32_t*>(a.d_work);
    uint8_t* row_ok = a.d_sig_ok ? a.d_sig_ok : static_cast<uint8_t*>(a.d_work) + 32 * rows;
    const dim3 g(static_cast<unsigned>((n + kHeaderThreads - 1) / kHeaderThreads)), b(kHeaderThreads);
    const uint32_t* given = reinterpret_cast<const uint32_t*>(a.d_given32);
    uint32_t* hash = reinterpret_cast<uint32_t*>(a.d_hash32);
    if (suite == BCOSGPU_SUITE_SM2)
        hipLaunchKernelGGL(header_hash_kernel<SM3>, g, b, 0, st, a.d_pre, a.d_pre_off, given, a.d_given_mask, a.d_sig_off,
                           n, rows, hash, row_hash);
    else
        hipLaunchKernelGGL(header_hash_kernel<KECCAK256>, g, b, 0, st, a.d_pre, a.d_pre_off, given, a.d_given_mask,
                           a.d_sig_off, n, rows, hash, row_hash);
    if (hipGetLastError() != hipSuccess) return BCOSGPU_E_HIP;
    if (rows) {
        const uint8_t* rh = reinterpret_cast<const uint8_t*>(row_hash);
        const int rc = a.d_row_slot ? launch_sig_verify_keyed(suite, a.d_row_slot, rh, a.d_sig, 64, rows, row_ok, nullptr, st)
                                    : launch_sig_verify(suite, a.d_row_pub64, rh, a.d_sig, 64, rows, row_ok, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(header_verdict_kernel, g, b, 0, st, a.d_pre_status, a.d_number, a.d_parent_number,
                       reinterpret_cast<const uint32_t*>(a.d_parent_hash32), a.d_parent_ok,
                       reinterpret_cast<const uint32_t*>(a.d_prev_hash32), a.prev_number, a.d_sig_off, a.d_row_weight,
                       row_ok, a.quorum, n, rows, hash, a.d_check, a.d_link);
    return hipGetLastError() == hipSuccess ? 0 : BCOSGPU_E_HIP;
}

}  // namespace bcosgpu
