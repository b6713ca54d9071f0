// txpool_admit.h -- the kernel bodies of transaction admission against the pool's three key sets (sorted_set.h,
// whose five rules hold here too): the independent verdict I(j), one lane per transaction, and the
// index-order rule in closed form over the transactions sorted by (nonce, index).  __host__ __device__ functions
// of (thread index, arguments), no intrinsics: csrc/txpool_kernels.hip wraps them, tests/cpp/txpool_sets_test.cpp
// runs them serially against a literal loop of the reference's order.
//
// What is restated (the literal order on Python sets, with the citations line by line: tests/txpool_restatement.py):
//   MemoryStorage::verifyAndSubmitTransaction   bcos-txpool/bcos-txpool/txpool/storage/MemoryStorage.cpp:223-273
//   TxValidator::verify                         bcos-txpool/bcos-txpool/txpool/validator/TxValidator.cpp:27-69
//   TxPoolNonceChecker::checkNonce              .../validator/TxPoolNonceChecker.cpp:34-49
//   LedgerNonceChecker::checkNonce / checkBlockLimit   .../validator/LedgerNonceChecker.cpp:36-61
//   MemoryStorage::enforceSubmitTransaction     MemoryStorage.cpp:147-221 (mode PROPOSAL)
//   TransactionImpl::nonce()                    nonce_parse.h
//
// Mode FULL, in kernel order: verdict_body -> sort the records by (skip, nonce, index) -> run_ok_body -> exclusive
// scan c of ok -> run_rule_body (losers' statuses, winners' flags) -> exclusive scan of the winners' flags ->
// sset::compact_body + sset::merge_body (the winners' nonces, already sorted and distinct, into `nonces`) ->
// finalize_body (senders, the records of the accepted hashes) -> sort -> the union of sorted_set.h into `hashes`.
// Mode PROPOSAL: verdict_body -> finalize_body -> sort -> union into `hashes`.
#pragma once
#include "nonce_parse.h"
#include "sorted_set.h"

namespace bcosgpu {
namespace admit {

using sset::Rec;
using sset::SetView;

enum : int { kModeFull = 0, kModeProposal = 1 };
enum : uint32_t {
    kOk = 0, kMalformed = 2, kNonceForHost = 4, kNonceCheckFail = 10000, kBlockLimitCheckFail = 10001,
    kAlreadyInTxPool = 10004, kInvalidChainId = 10006, kInvalidGroupId = 10007, kInvalidSignature = 10008
};
// the indices of tars::TxFields' off[] / len[] this header reads (txpool_kernels.hip asserts they are tars::F_*)
enum : int { kFieldChain = 0, kFieldGroup = 1, kFieldNonce = 2 };

// the pool's constants as a kernel argument
struct PoolParams {
    const uint8_t* chain;  // device copies of the pool's chain id and group id
    const uint8_t* group;
    uint32_t chain_len, group_len;
    int64_t number, range;  // 0 <= number, 0 <= range, number + range does not overflow (checked by the host)
};

SSET_HD bool bytes_equal(const uint8_t* a, uint32_t alen, const uint8_t* b, uint32_t blen) {
    if (alen != blen) return false;
    for (uint32_t i = 0; i < alen; ++i)  // alen: a decoded field's length, within the encoded bytes
        if (a[i] != b[i]) return false;
    return true;
}

// the verdicts the index-order rule leaves alone, and whose transactions stay out of the sort
SSET_HD bool out_of_group(uint32_t st) {
    return st == kMalformed || st == kAlreadyInTxPool || st == kInvalidGroupId || st == kInvalidChainId ||
           st == kNonceForHost;
}

// ---- the independent verdict of transaction j against the sets as they are before the call.
// vstatus is the existing decode + verify's status byte (0 ok, 1 InvalidSignature, 2 the decode throws), fields
// its TxFields (Fields: any struct with off[] / len[] / block_limit), txhash its hashes (n x 32; zeroed here for a
// transaction that did not decode).  Writes status[j], nonce_out[j] (zero when not decoded or not canonical) and
// the sort record of j; status, nonce_out, recs and txhash all hold out_cap entries.
template <class Fields>
SSET_HD void verdict_body(uint64_t j, uint32_t n, int mode, const uint8_t* enc, uint64_t enc_bytes,
                          const Fields* fields, const uint8_t* vstatus, uint8_t* txhash, SetView hashes,
                          SetView nonces, SetView ledger, PoolParams pp, uint32_t* status, uint8_t* nonce_out,
                          Rec* recs, uint32_t out_cap, uint32_t* err) {
    if (j >= n) return;
    if (j >= out_cap) {  // status, nonce_out and recs all hold out_cap entries
        sset::set_error(err, sset::kErrStore);
        return;
    }
    uint8_t key[sset::kKeyBytes];
    for (uint32_t i = 0; i < sset::kKeyBytes; ++i) key[i] = 0;
    uint32_t st = kOk;
    bool decoded = vstatus[j] != 2, canonical = false;
    if (decoded) {  // the decoder leaves every field inside the transaction's bytes; checked all the same
        for (int k = kFieldChain; k <= kFieldNonce; ++k)
            if (fields[j].off[k] > enc_bytes || fields[j].len[k] > enc_bytes - fields[j].off[k]) decoded = false;
        if (!decoded) sset::set_error(err, sset::kErrInput);
    }
    if (!decoded) {
        st = kMalformed;
        for (uint32_t i = 0; i < 32; ++i) txhash[j * 32 + i] = 0;  // no transaction, no hash
    } else {
        const Fields& f = fields[j];
        canonical = parse_canonical_nonce(enc + f.off[kFieldNonce], f.len[kFieldNonce], key);
        if (!canonical)
            for (uint32_t i = 0; i < sset::kKeyBytes; ++i) key[i] = 0;
        const uint32_t nl = sset::clamp_count(ledger.count, ledger.cap, err);
        if (mode == kModeFull) {
            const uint32_t nh = sset::clamp_count(hashes.count, hashes.cap, err);
            const uint32_t nn = sset::clamp_count(nonces.count, nonces.cap, err);
            const int64_t limit = f.block_limit;
            if (sset::contains_key(hashes.keys, nh, txhash + j * 32)) st = kAlreadyInTxPool;
            else if (!bytes_equal(enc + f.off[kFieldGroup], f.len[kFieldGroup], pp.group, pp.group_len))
                st = kInvalidGroupId;
            else if (!bytes_equal(enc + f.off[kFieldChain], f.len[kFieldChain], pp.chain, pp.chain_len))
                st = kInvalidChainId;
            else if (!canonical) st = kNonceForHost;
            else if (sset::contains_key(nonces.keys, nn, key)) st = kNonceCheckFail;
            else if (sset::contains_key(ledger.keys, nl, key)) st = kNonceCheckFail;
            else if (pp.number >= limit || pp.number + pp.range < limit) st = kBlockLimitCheckFail;
            else if (vstatus[j] != 0) st = kInvalidSignature;
        } else {
            if (!canonical) st = kNonceForHost;
            else if (sset::contains_key(ledger.keys, nl, key)) st = kNonceCheckFail;
            else if (vstatus[j] != 0) st = kInvalidSignature;
        }
    }
    status[j] = st;
    sset::key_copy(nonce_out + j * 32, key);
    sset::key_copy(recs[j].key, key);
    recs[j].idx = static_cast<uint32_t>(j);
    recs[j].skip = out_of_group(st) ? 1u : 0u;
}

// ---- ok[p] = the record at sorted position p takes part and its transaction's independent verdict is 0
SSET_HD void run_ok_body(uint64_t p, uint32_t n, const Rec* recs, const uint32_t* status, uint32_t* ok, uint32_t ok_cap,
                         uint32_t* err) {
    if (p >= n) return;
    if (p >= ok_cap) {
        sset::set_error(err, sset::kErrStore);
        return;
    }
    const uint32_t j = recs[p].idx;
    ok[p] = recs[p].skip == 0 && j < n && status[j] == kOk ? 1u : 0u;
}

// ---- the index-order rule at sorted position p.  c is the exclusive scan of ok.  The run of p's nonce starts at
// s = lower_bound(p's nonce); c[p] - c[s] counts the verdict-0 transactions of the run before p.  None: p keeps its
// verdict and is the run's winner W iff ok[p].  Some: W is the first of them (found by a lower bound over c, which
// does not decrease), W's index is below p's (the sort's second key), and p's status becomes 10004 when its hash
// is W's, else 10000.  A lane writes only its own transaction's status and its own position's flag, and reads
// statuses nowhere: ok and c are the previous kernels' outputs.
SSET_HD void run_rule_body(uint64_t p, uint32_t n, const Rec* recs, const uint32_t* ok, const uint32_t* c,
                           const uint8_t* txhash, uint32_t* status, uint32_t* win, uint32_t out_cap, uint32_t* err) {
    if (p >= n) return;
    if (p >= out_cap) {
        sset::set_error(err, sset::kErrStore);
        return;
    }
    if (recs[p].skip != 0) {
        win[p] = 0;
        return;
    }
    const uint32_t s = sset::lower_bound_recs(recs, n, recs[p].key);  // s <= p: p's own key is there
    const uint32_t before = c[p] - c[s];
    if (before == 0) {
        win[p] = ok[p];
        return;
    }
    win[p] = 0;
    // the first q in [s, p) with ok[q]: the first q whose c[q + 1] exceeds c[s]  (q + 1 <= p < n)
    uint32_t lo = s, hi = static_cast<uint32_t>(p);
    for (uint32_t k = 0; k < sset::kMaxSearchSteps && lo < hi; ++k) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (c[mid + 1] > c[s]) hi = mid;
        else lo = mid + 1;
    }
    const uint32_t j = recs[p].idx, w = recs[lo].idx;
    if (j >= out_cap || w >= n) {
        sset::set_error(err, sset::kErrStore);
        return;
    }
    status[j] = sset::key_cmp(txhash + static_cast<size_t>(j) * 32, txhash + static_cast<size_t>(w) * 32) == 0
                    ? kAlreadyInTxPool
                    : kNonceCheckFail;
}

// ---- after the final statuses: the sender of a transaction that is not accepted is zero; the record of j's
// hash takes part in the union with `hashes` iff j is accepted
SSET_HD void finalize_body(uint64_t j, uint32_t n, const uint32_t* status, const uint8_t* txhash, uint8_t* sender,
                           Rec* recs, uint32_t out_cap, uint32_t* err) {
    if (j >= n) return;
    if (j >= out_cap) {
        sset::set_error(err, sset::kErrStore);
        return;
    }
    const bool accepted = status[j] == kOk;
    if (!accepted)
        for (int i = 0; i < 20; ++i) sender[j * 20 + i] = 0;
    sset::key_copy(recs[j].key, txhash + j * 32);
    recs[j].idx = static_cast<uint32_t>(j);
    recs[j].skip = accepted ? 0u : 1u;
}

}  // namespace admit
}  // namespace bcosgpu
