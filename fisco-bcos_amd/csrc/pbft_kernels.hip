// pbft_kernels.hip -- every signature of a drained PBFT message queue in one call (gfx950).
//
// Replaces, for the messages a PBFT worker popped from its queue (PBFTEngine::executeWorker,
// bcos-pbft/bcos-pbft/pbft/engine/PBFTEngine.cpp:555-601), the verifies its handlers run one at a time:
//   checkSignature                              PBFTEngine.cpp:732-750
//   checkProposalSignature                      PBFTEngine.cpp:752-771
//   PBFTCacheProcessor::checkPrecommitWeight    bcos-pbft/bcos-pbft/pbft/cache/PBFTCacheProcessor.cpp:795-821
//   isValidNewViewMsg (the view-change loop)    PBFTEngine.cpp:1238-1263
//
// Four phases on one stream (launch_pbft_check):
//   pbft_hash_kernel<H>     one message per lane: the digest of its signed data (hashFieldsData, tens of bytes;
//                           PBFTMessage.cpp:92-98) with the one-lane hashers of hash_device.h, or the given
//                           signatureDataHash, to msg_hash32 and to the message's signature row of row_hash32.
//                           The hashes of the proposal and proof rows are given: the caller uploaded them.
//   the signatures          launch_sig_verify_keyed (slot ids of registered keys) or launch_sig_verify (keys in
//                           the rows) over all rows, stride 64, into the row ok array.  Used as they are.
//   pbft_verdict_kernel     one message per lane: its signature rows into bits 2 and 4, each of its prepared
//                           proposals folded (all proofs ok; the wrapping u64 sum of their weights against the
//                           quorum) into prepared_check and bit 8, the host's bit 1 merged.
//   pbft_group_kernel       one NewView group per lane, only when there are groups: a failed view change is
//                           bit 16 of the parent, a weight below the quorum bit 32.
//
// Row semantics are the header check's (header_kernels.hip), as the reference's loops are the same
// (PBFTCacheProcessor.cpp:801-820 against BlockValidator.cpp:149-180): a row whose index names no consensus node
// fails (a negative slot id, or a zero key and a zero signature); ONE failed proof fails the proposal whatever
// the remaining weight; an index listed twice counts twice.
// The proof rows of the prepared proposals lie back to back in the proposals' order (prep_row_off is a CSR over
// them); a message's own two rows may be anywhere and are named by msg_row / prop_row.
// d_work holds the row ok array when the caller wants no row verdicts; every byte of it that is read is written
// by this call's kernels first, so its earlier contents never matter.
#include "hash_device.h"
#include "engine.h"

namespace bcosgpu {

namespace {

constexpr int kPbftThreads = 64;  // one wave: messages are short, a wave costs its longest

template <int H>
__global__ __launch_bounds__(kPbftThreads) void pbft_hash_kernel(
    const uint8_t* __restrict__ data, const uint64_t* __restrict__ data_off, const uint32_t* __restrict__ given,
    const uint8_t* __restrict__ given_mask, const int64_t* __restrict__ msg_row, uint64_t n, uint64_t rows,
    uint32_t* __restrict__ hash, uint32_t* __restrict__ row_hash) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kPbftThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t d[8];
    if (given && given_mask && given_mask[i]) {
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = given[8 * i + k];
    } else {
        const uint64_t a = data_off[i], b = data_off[i + 1];
        const uint32_t len = static_cast<uint32_t>(b - a);
        FlatReader rd(data + a, len);
        uint32_t w[8];
        if (H == KECCAK256) keccak256_msg(rd, len, w);
        else sm3_msg(rd, len, w);
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = H == SM3 ? bswap32(w[k]) : w[k];  // memory order, as store_digest
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) hash[8 * i + k] = d[k];
    const int64_t r = msg_row[i];
    if (r >= 0 && static_cast<uint64_t>(r) < rows) {
#pragma unroll
        for (int k = 0; k < 8; ++k) row_hash[8 * r + k] = d[k];
    }
}

// a requested signature whose row is outside [0, rows) fails: an absent proposal signature has row -1
__device__ __forceinline__ bool row_passed(int64_t r, uint64_t rows, const uint8_t* __restrict__ row_ok) {
    return r >= 0 && static_cast<uint64_t>(r) < rows && row_ok[r] == 1;
}

__global__ __launch_bounds__(kPbftThreads) void pbft_verdict_kernel(
    const uint8_t* __restrict__ pre_flags, const uint8_t* __restrict__ checks, const int64_t* __restrict__ msg_row,
    const int64_t* __restrict__ prop_row, const uint64_t* __restrict__ prep_off,
    const uint64_t* __restrict__ prep_row_off, uint64_t nprep, const uint64_t* __restrict__ row_weight,
    const uint8_t* __restrict__ row_ok, uint64_t quorum, uint64_t n, uint64_t rows, uint32_t* __restrict__ msg_flags,
    uint8_t* __restrict__ prepared_check) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kPbftThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t f = pre_flags[i] & BCOSGPU_PBFT_E_NODE;  // PBFTEngine.cpp:735-741, decided on the host
    const uint32_t want = checks[i];
    if ((want & BCOSGPU_PBFT_CHECK_MSG_SIG) && !row_passed(msg_row[i], rows, row_ok)) f |= BCOSGPU_PBFT_E_MSG_SIG;
    if ((want & BCOSGPU_PBFT_CHECK_PROPOSAL_SIG) && !row_passed(prop_row[i], rows, row_ok))
        f |= BCOSGPU_PBFT_E_PROPOSAL_SIG;
    uint64_t p = prep_off[i], pe = prep_off[i + 1];
    if (pe > nprep) pe = nprep;  // (a CSR that overruns nprep or rows reads and writes nothing past the arrays)
    for (; p < pe; ++p) {
        uint32_t code = BCOSGPU_PREPARED_UNCHECKED;
        if (want & BCOSGPU_PBFT_CHECK_PREPARED) {  // PBFTCacheProcessor.cpp:799-820
            uint64_t r = prep_row_off[p], e = prep_row_off[p + 1];
            if (e > rows) e = rows;
            bool all = true;
            uint64_t weight = 0;  // uint64_t weight (:799): wraps as the reference's does
            for (; r < e; ++r) {
                all = all && row_ok[r] == 1;
                weight += row_weight[r];  // per list entry, duplicates included (:817)
            }
            code = !all ? BCOSGPU_PREPARED_E_PROOF : weight < quorum ? BCOSGPU_PREPARED_E_QUORUM : BCOSGPU_PREPARED_OK;
            if (code != BCOSGPU_PREPARED_OK) f |= BCOSGPU_PBFT_E_PREPARED;  // PBFTEngine.cpp:1171-1177
        }
        prepared_check[p] = static_cast<uint8_t>(code);
    }
    msg_flags[i] = f;
}

// isValidNewViewMsg's loop (PBFTEngine.cpp:1239-1263).  A lane reads its view changes' own bits (1-8) and ORs
// 16 / 32 into its parent atomically: a message may be the parent of several groups, or a child and a parent.
__global__ __launch_bounds__(kPbftThreads) void pbft_group_kernel(const uint64_t* __restrict__ groups, uint64_t ngroups,
                                                                  const uint64_t* __restrict__ msg_weight,
                                                                  uint64_t quorum, uint64_t n, uint32_t* msg_flags) {
    const uint64_t g = static_cast<uint64_t>(blockIdx.x) * kPbftThreads + threadIdx.x;
    if (g >= ngroups) return;
    const uint64_t parent = groups[3 * g];
    uint64_t j = groups[3 * g + 1], count = groups[3 * g + 2];
    if (parent >= n) return;
    if (j > n) j = n;
    if (count > n - j) count = n - j;
    constexpr uint32_t own = BCOSGPU_PBFT_E_NODE | BCOSGPU_PBFT_E_MSG_SIG | BCOSGPU_PBFT_E_PROPOSAL_SIG |
                             BCOSGPU_PBFT_E_PREPARED;
    bool all = true;
    uint64_t weight = 0;  // uint64_t weight (:1239)
    for (const uint64_t e = j + count; j < e; ++j) {
        all = all && (__hip_atomic_load(msg_flags + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & own) == 0;  // :1243-1248
        weight += msg_weight[j];  // 0 for a node that is unknown (:1249-1254)
    }
    const uint32_t bits = (all ? 0u : BCOSGPU_PBFT_E_VIEWCHANGE) | (weight < quorum ? BCOSGPU_PBFT_E_GROUP_QUORUM : 0u);
    if (bits) atomicOr(msg_flags + parent, bits);
}

uint64_t align8(uint64_t x) { return (x + 7) & ~uint64_t{7}; }

}  // namespace

// d_work: the row ok array (used when the caller passes none)
uint64_t pbft_check_work_bytes(uint64_t n, uint64_t rows) {
    (void)n;
    return align8(rows) + 32;
}

int launch_pbft_check(int suite, const PbftCheckArgs& a, hipStream_t st) {
    const uint64_t n = a.n, rows = a.rows;
    if (n == 0) return 0;
    if (n > 0xFFFFFFFFull || rows > 0xFFFFFFFFull || a.nprep > 0xFFFFFFFFull || a.ngroups > 0xFFFFFFFFull ||
        a.work_bytes < pbft_check_work_bytes(n, rows))
        return BCOSGPU_E_ARG;
    if (rows && (a.d_row_slot != nullptr) == (a.d_row_pub64 != nullptr)) return BCOSGPU_E_ARG;
    uint32_t* row_hash = reinterpret_cast<uint32_t*>(a.d_row_hash32);
    uint8_t* row_ok = a.d_sig_ok ? a.d_sig_ok : static_cast<uint8_t*>(a.d_work);
    const dim3 g(static_cast<unsigned>((n + kPbftThreads - 1) / kPbftThreads)), b(kPbftThreads);
    const uint32_t* given = reinterpret_cast<const uint32_t*>(a.d_given32);
    uint32_t* hash = reinterpret_cast<uint32_t*>(a.d_msg_hash32);
    if (suite == BCOSGPU_SUITE_SM2)
        hipLaunchKernelGGL(pbft_hash_kernel<SM3>, g, b, 0, st, a.d_data, a.d_data_off, given, a.d_given_mask, a.d_msg_row,
                           n, rows, hash, row_hash);
    else
        hipLaunchKernelGGL(pbft_hash_kernel<KECCAK256>, g, b, 0, st, a.d_data, a.d_data_off, given, a.d_given_mask,
                           a.d_msg_row, n, rows, hash, row_hash);
    if (hipGetLastError() != hipSuccess) return BCOSGPU_E_HIP;
    if (rows) {
        const int rc = a.d_row_slot
                           ? launch_sig_verify_keyed(suite, a.d_row_slot, a.d_row_hash32, a.d_sig, 64, rows, row_ok, nullptr, st)
                           : launch_sig_verify(suite, a.d_row_pub64, a.d_row_hash32, a.d_sig, 64, rows, row_ok, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(pbft_verdict_kernel, g, b, 0, st, a.d_pre_flags, a.d_checks, a.d_msg_row, a.d_prop_row,
                       a.d_prep_off, a.d_prep_row_off, a.nprep, a.d_row_weight, row_ok, a.quorum, n, rows, a.d_msg_flags,
                       a.d_prepared_check);
    if (hipGetLastError() != hipSuccess) return BCOSGPU_E_HIP;
    if (a.ngroups) {
        const dim3 gg(static_cast<unsigned>((a.ngroups + kPbftThreads - 1) / kPbftThreads));
        hipLaunchKernelGGL(pbft_group_kernel, gg, b, 0, st, a.d_groups, a.ngroups, a.d_msg_weight, a.quorum, n,
                           a.d_msg_flags);
    }
    return hipGetLastError() == hipSuccess ? 0 : BCOSGPU_E_HIP;
}

}  // namespace bcosgpu
