// consensus_stage.h -- the host half of bcosgpu_headers_check and bcosgpu_pbft_check (api.hip), no HIP: what a
// bad view is, the signature rows against the consensus set, the layout of the one pinned staging block, its
// packing, the kernels' arguments over it, and the way from the download back to the caller's outputs.  Each
// check is a stage with the same five steps: validate (an error text or null; it also counts, since the counts
// walk the same views), plan (every offset, once), pack (a block of exactly p.total bytes), args (the same offsets
// on any base pointer) and scatter.  tests/cpp/consensus_stage_test.cpp pins all of it without a GPU.
#pragma once
#include <stdint.h>
#include <cstring>
#include <utility>
#include <vector>
#include "../../include/bcos_gpu.h"
#include "consensus_args.h"

namespace bcosgpu {

inline uint64_t stage_align(uint64_t bytes) { return (bytes + 7) & ~uint64_t{7}; }

// The bump allocator of a staging block: regions in the order taken, each 8-byte aligned.
struct StageAlloc {
    uint64_t total = 0;
    uint64_t take(uint64_t bytes) {
        const uint64_t o = total;
        total += stage_align(bytes);
        return o;
    }
};
template <class T>
T* stage_at(uint8_t* base, uint64_t off) { return reinterpret_cast<T*>(base + off); }

// The signature rows of a check against a consensus set (block headers, PBFT messages): a row is a node index
// and a signature, verified against that node's key and counted with that node's weight.  With a slot id of the
// device key cache for every consensus key (the registration is api.hip's) the rows carry slot ids, otherwise
// the keys.  A row whose index names no consensus node (ConsensusConfig.cpp:150-158), or whose signature is shorter
// than verify accepts (bcos_gpu.hpp:94-115), fails without a key: a negative id, or a zero key, and a zero
// signature and weight.
struct ConsensusRows {
    const bcosgpu_ConsensusSet* cs = nullptr;
    uint64_t rows = 0;
    bool keyed = false;          // the rows carry slot ids
    std::vector<int32_t> slots;  // of the consensus keys
    std::vector<int32_t> node;   // the consensus node of each row, -1 = the row fails without a key
    std::vector<uint8_t> pubs;   // the rows' keys, when the run has to be repeated
    uint8_t* sig = nullptr;      // staging of the rows: r || s [64 rows], weights [rows], slot ids or keys
    uint64_t* weight = nullptr;
    uint8_t* key = nullptr;

    // slot_ids: one per consensus key, negative = none (an empty set has none: its rows all fail, without keys)
    void begin(const bcosgpu_ConsensusSet& cs_, uint64_t rows_, std::vector<int32_t> slot_ids) {
        cs = &cs_, rows = rows_, slots = std::move(slot_ids), node.assign(rows, -1);
        keyed = rows != 0 && cs->n != 0 && slots.size() == cs->n;
        for (size_t k = 0; keyed && k < cs->n; ++k) keyed = slots[k] >= 0;
    }
    uint64_t key_bytes() const { return keyed ? 4 * rows : 64 * rows; }
    void stage(uint8_t* sig_, uint64_t* weight_, uint8_t* key_) {
        sig = sig_, weight = weight_, key = key_;
        std::memset(sig, 0, 64 * rows);
        if (!keyed) std::memset(key, 0, 64 * rows);
    }
    bool known(int64_t index) const { return index >= 0 && static_cast<uint64_t>(index) < cs->n; }
    void put(uint64_t r, int64_t index, const uint8_t* signature, size_t signature_len) {
        const bool ok = known(index) && signature_len >= 64;
        const int32_t k = ok ? static_cast<int32_t>(index) : -1;
        node[r] = k;
        weight[r] = ok ? cs->weights[k] : 0;
        if (ok) std::memcpy(sig + 64 * r, signature, 64);
        if (keyed) reinterpret_cast<int32_t*>(key)[r] = ok ? slots[k] : -1;
        else if (ok) std::memcpy(key + 64 * r, cs->node_ids64 + 64 * k, 64);
    }
    const uint8_t* row_pubs() {
        pubs.assign(64 * rows, 0);
        for (uint64_t q = 0; q < rows; ++q)
            if (node[q] >= 0) std::memcpy(pubs.data() + 64 * q, cs->node_ids64 + 64 * node[q], 64);
        return pubs.data();
    }
    template <class Args>
    void wire(Args& a, const uint8_t* key_region) const {  // exactly one of the two
        if (keyed) a.d_row_slot = reinterpret_cast<const int32_t*>(key_region);
        else a.d_row_pub64 = key_region;
    }
};

// A field of a view: a null pointer with a length, or (hashes) more than 32 bytes, is a bad view.
inline bool bad_field(const uint8_t* p, size_t len, size_t max_len = ~size_t{0}) { return (!p && len) || len > max_len; }

// ------------------------------------------------------------------ block headers
// The host-side part of asyncCheckBlock for one header (BlockValidator.cpp:35-63 with
// checkSealerListAndWeightList, :80-139): the early verdict, 0 = go on to the signature rows.
inline uint8_t header_pre_status(const bcosgpu_BlockHeaderData& h, const bcosgpu_ConsensusSet& cs) {
    if (h.block_number == 0) return BCOSGPU_HEADER_GENESIS;                         // :35-39
    if (h.block_number <= cs.committed_index) return BCOSGPU_HEADER_E_COMMITTED;    // :49-53
    if (h.tx_count == 0) return BCOSGPU_HEADER_NO_TXS;                              // :54-58
    if (h.sealer < 0 || static_cast<uint64_t>(h.sealer) >= cs.n) return BCOSGPU_HEADER_E_SEALER;  // :85-93
    if (h.nsealer_list != cs.n || h.nconsensus_weights != cs.n) return BCOSGPU_HEADER_E_SEALER_LIST;  // :98-108
    for (size_t k = 0; k < cs.n; ++k) {                                             // :110-137
        const bcosgpu_Bytes& id = h.sealer_list[k];
        if (id.len != 64 || std::memcmp(id.data, cs.node_ids64 + 64 * k, 64) != 0) return BCOSGPU_HEADER_E_SEALER_LIST;
        if (static_cast<uint64_t>(h.consensus_weights[k]) != cs.weights[k]) return BCOSGPU_HEADER_E_SEALER_LIST;
    }
    return 0;
}

// BlockValidator::asyncCheckBlock and the ledger's parent check for a run of headers (see bcos_gpu.h): the
// early verdicts and the rows' keys and weights on the host, everything in one block (64-bit arrays first, then
// the 32-byte hashes, signatures, keys, byte arrays, the preimages last).  The download is hash32 [32 n] |
// check [n] | link [n] | sig_ok [rows] from the next multiple of 8.
struct HeadersStage {
    const bcosgpu_BlockHeaderData* const headers;
    const size_t n;
    const bcosgpu_ConsensusSet& cs;
    const uint8_t* const prev_hash32;  // nullable
    const int64_t prev_number;
    const int flags;
    std::vector<uint8_t> pre_status{};  // after validate
    uint64_t rows = 0;                  // after validate: the signatures of the headers without an early verdict
    uint64_t pre_bytes = 0;
    ConsensusRows cr{};
    struct Plan {
        uint64_t pre_off, sig_off, number, pnum, weight, phash, given, prev, sig, key, mask, status, pok, pre, total;
        uint64_t out_check, out_link, out_ok, out_bytes;
    } p{};

    // bad views first (the packer checks the hashed fields again; it does not see the signatures)
    const char* validate() {
        for (size_t i = 0; i < n; ++i) {
            const bcosgpu_BlockHeaderData& h = headers[i];
            if ((!h.signatures && h.nsignatures) || (!h.sealer_list && h.nsealer_list) ||
                (!h.consensus_weights && h.nconsensus_weights) || (!h.parents && h.nparents) ||
                (h.data_hash_len && (!h.data_hash || h.data_hash_len > 32)))
                return "bad header view (null field with a length, or a dataHash over 32 bytes)";
            for (size_t k = 0; k < h.nsealer_list; ++k)
                if (!h.sealer_list[k].data && h.sealer_list[k].len) return "bad header view";
            for (size_t s = 0; s < h.nsignatures; ++s)
                if (!h.signatures[s].signature && h.signatures[s].signature_len)
                    return "bad header view (null signature with a length)";
        }
        pre_status.resize(n);
        rows = 0;
        for (size_t i = 0; i < n; ++i)
            if (!(pre_status[i] = header_pre_status(headers[i], cs))) rows += headers[i].nsignatures;
        return nullptr;
    }

    void plan(std::vector<int32_t> slot_ids) {
        cr.begin(cs, rows, std::move(slot_ids));
        pre_bytes = bcosgpu_header_preimage_size(headers, n, flags);
        StageAlloc s;
        p.pre_off = s.take(8 * (n + 1)), p.sig_off = s.take(8 * (n + 1)), p.number = s.take(8 * n);
        p.pnum = s.take(8 * n), p.weight = s.take(8 * rows), p.phash = s.take(32 * n), p.given = s.take(32 * n);
        p.prev = s.take(32), p.sig = s.take(64 * rows), p.key = s.take(cr.key_bytes());
        p.mask = s.take(n), p.status = s.take(n), p.pok = s.take(n), p.pre = s.take(pre_bytes);
        p.total = s.total;
        p.out_check = 32 * n, p.out_link = 33 * n, p.out_ok = stage_align(34 * n), p.out_bytes = p.out_ok + rows;
    }

    const char* pack(uint8_t* hs) {
        if (bcosgpu_pack_header_preimages(headers, n, flags, hs + p.pre, pre_bytes, stage_at<uint64_t>(hs, p.pre_off)))
            return "bad header view (null field with a length, a dataHash over 32 bytes, or a header of 4 GiB or more)";
        uint64_t* sig_off = stage_at<uint64_t>(hs, p.sig_off);
        int64_t* number = stage_at<int64_t>(hs, p.number);
        int64_t* pnum = stage_at<int64_t>(hs, p.pnum);
        cr.stage(hs + p.sig, stage_at<uint64_t>(hs, p.weight), hs + p.key);
        std::memset(hs + p.phash, 0, 32 * n);
        std::memset(hs + p.given, 0, 32 * n);
        if (prev_hash32) std::memcpy(hs + p.prev, prev_hash32, 32);
        uint64_t r = 0;
        for (size_t i = 0; i < n; ++i) {
            const bcosgpu_BlockHeaderData& h = headers[i];
            number[i] = h.block_number;
            const bool pok = h.nparents && h.parents[0].block_hash_len == 32;  // LedgerImpl.h:302-306 reads [0] only
            pnum[i] = h.nparents ? h.parents[0].block_number : 0;
            hs[p.pok + i] = pok;
            if (pok) std::memcpy(hs + p.phash + 32 * i, h.parents[0].block_hash, 32);
            const bool given = h.data_hash_len && !(flags & BCOSGPU_HEADER_RECOMPUTE);  // TarsHashable.h:81-85
            hs[p.mask + i] = given;
            if (given) std::memcpy(hs + p.given + 32 * i, h.data_hash, h.data_hash_len);
            hs[p.status + i] = pre_status[i];
            sig_off[i] = r;
            if (pre_status[i]) continue;
            for (size_t s = 0; s < h.nsignatures; ++s, ++r)
                cr.put(r, h.signatures[s].sealer_index, h.signatures[s].signature, h.signatures[s].signature_len);
        }
        sig_off[n] = r;
        return nullptr;
    }

    HeadersCheckArgs args(uint8_t* in, uint8_t* out, void* work, uint64_t work_bytes) const {
        HeadersCheckArgs a;
        a.d_pre = in + p.pre, a.d_pre_off = stage_at<const uint64_t>(in, p.pre_off);
        a.d_given32 = in + p.given, a.d_given_mask = in + p.mask, a.d_pre_status = in + p.status;
        a.d_number = stage_at<const int64_t>(in, p.number), a.d_parent_number = stage_at<const int64_t>(in, p.pnum);
        a.d_parent_hash32 = in + p.phash, a.d_parent_ok = in + p.pok;
        a.d_prev_hash32 = prev_hash32 ? in + p.prev : nullptr, a.prev_number = prev_number;
        a.d_sig_off = stage_at<const uint64_t>(in, p.sig_off), a.d_sig = in + p.sig;
        a.d_row_weight = stage_at<const uint64_t>(in, p.weight);
        cr.wire(a, in + p.key);
        a.quorum = cs.min_required_quorum, a.n = n, a.rows = rows;
        a.d_hash32 = out, a.d_check = out + p.out_check, a.d_link = out + p.out_link, a.d_sig_ok = out + p.out_ok;
        a.d_work = work, a.work_bytes = work_bytes;
        return a;
    }

    // ho: the download.  sig_ok has one entry per signature; 2 = the header's signatures were not checked
    void scatter(const uint8_t* ho, uint8_t* hash32, uint8_t* check, uint8_t* link, uint8_t* sig_ok_or_null) const {
        std::memcpy(hash32, ho, 32 * n);
        std::memcpy(check, ho + p.out_check, n);
        std::memcpy(link, ho + p.out_link, n);
        if (!sig_ok_or_null) return;
        uint64_t s = 0, q = 0;
        for (size_t i = 0; i < n; ++i) {
            const size_t m = headers[i].nsignatures;
            if (pre_status[i]) std::memset(sig_ok_or_null + s, 2, m);
            else if (m) std::memcpy(sig_ok_or_null + s, ho + p.out_ok + q, m), q += m;
            s += m;
        }
    }
};

// ------------------------------------------------------------------ PBFT messages
inline bool bad_pbft_view(const bcosgpu_PBFTMessageData& m) {
    if (bad_field(m.signed_data, m.signed_data_len, 0xFFFFFFFEull) || bad_field(m.signature_hash, m.signature_hash_len, 32) ||
        bad_field(m.signature, m.signature_len) || bad_field(m.proposal_hash, m.proposal_hash_len, 32) ||
        bad_field(m.proposal_signature, m.proposal_signature_len) || (!m.prepared && m.nprepared))
        return true;
    for (size_t p = 0; p < m.nprepared; ++p) {
        const bcosgpu_PrecommitProof& pp = m.prepared[p];
        if (bad_field(pp.hash, pp.hash_len, 32) || (!pp.proofs && pp.nproofs)) return true;
        for (size_t s = 0; s < pp.nproofs; ++s)
            if (bad_field(pp.proofs[s].signature, pp.proofs[s].signature_len)) return true;
    }
    return false;
}

// The signature checks of a drained PBFT message queue (see bcos_gpu.h): every requested signature becomes a
// row (the proofs of every checked prepared proposal first, in order: the CSR of the verdict kernel; then the
// message and proposal signatures) with its node's key and weight, everything in one block (64-bit arrays
// first, then the 32-byte hashes, signatures, keys, byte arrays, the signed data last).  The download is
// msg_hash32 [32 n] | msg_flags [n] (u32) | prepared_check [nprep] | sig_ok [rows] from the next multiple of 8.
struct PbftStage {
    const bcosgpu_PBFTMessageData* const msgs;
    const size_t n;
    const bcosgpu_PBFTGroup* const groups;
    const size_t ngroups;
    const bcosgpu_ConsensusSet& cs;
    uint64_t proof_rows = 0, sig_rows = 0, rows = 0, nprep = 0, data_bytes = 0;  // after validate
    ConsensusRows cr{};
    struct Plan {
        uint64_t data_off, mweight, mrow, prow, prep_off, prep_row, groups, weight, given, rhash, sig, key, mask, pre,
            checks, data, total;
        uint64_t out_flags, out_prep, out_ok, out_bytes;
    } p{};

    const char* validate() {
        proof_rows = sig_rows = nprep = data_bytes = 0;
        for (size_t i = 0; i < n; ++i) {
            const bcosgpu_PBFTMessageData& m = msgs[i];
            if (bad_pbft_view(m))
                return "bad PBFT message view (null field with a length, a hash over 32 bytes, or signed data of 4 GiB "
                       "or more)";
            sig_rows += (m.checks & BCOSGPU_PBFT_CHECK_MSG_SIG) != 0;
            sig_rows += (m.checks & BCOSGPU_PBFT_CHECK_PROPOSAL_SIG) && m.proposal_signature_len;  // absent: no row (:755-758)
            for (size_t k = 0; k < m.nprepared && (m.checks & BCOSGPU_PBFT_CHECK_PREPARED); ++k)
                proof_rows += m.prepared[k].nproofs;
            nprep += m.nprepared;
            if (!m.signature_hash_len) data_bytes += m.signed_data_len;
        }
        rows = proof_rows + sig_rows;
        for (size_t g = 0; g < ngroups; ++g)
            if (groups[g].parent >= n || groups[g].first > n || groups[g].count > n - groups[g].first)
                return "a group names messages outside [0, n)";
        return nullptr;
    }

    void plan(std::vector<int32_t> slot_ids) {
        cr.begin(cs, rows, std::move(slot_ids));
        StageAlloc s;
        p.data_off = s.take(8 * (n + 1)), p.mweight = s.take(8 * n), p.mrow = s.take(8 * n), p.prow = s.take(8 * n);
        p.prep_off = s.take(8 * (n + 1)), p.prep_row = s.take(8 * (nprep + 1)), p.groups = s.take(24 * ngroups);
        p.weight = s.take(8 * rows), p.given = s.take(32 * n), p.rhash = s.take(32 * rows), p.sig = s.take(64 * rows);
        p.key = s.take(cr.key_bytes()), p.mask = s.take(n), p.pre = s.take(n), p.checks = s.take(n);
        p.data = s.take(data_bytes);
        p.total = s.total;
        p.out_flags = 32 * n, p.out_prep = 36 * n, p.out_ok = stage_align(p.out_prep + nprep);
        p.out_bytes = p.out_ok + rows;
    }

    void pack(uint8_t* hs) {
        uint64_t* data_off = stage_at<uint64_t>(hs, p.data_off);
        uint64_t* mweight = stage_at<uint64_t>(hs, p.mweight);
        int64_t* mrow = stage_at<int64_t>(hs, p.mrow);
        int64_t* prow = stage_at<int64_t>(hs, p.prow);
        uint64_t* prep_off = stage_at<uint64_t>(hs, p.prep_off);
        uint64_t* prep_row = stage_at<uint64_t>(hs, p.prep_row);
        cr.stage(hs + p.sig, stage_at<uint64_t>(hs, p.weight), hs + p.key);
        std::memset(hs + p.given, 0, 32 * n);
        std::memset(hs + p.rhash, 0, 32 * rows);
        uint64_t q = 0, r = proof_rows, np = 0, d = 0;  // the next proof row, the next signature row
        for (size_t i = 0; i < n; ++i) {
            const bcosgpu_PBFTMessageData& m = msgs[i];
            const bool known = cr.known(m.generated_from);
            hs[p.pre + i] = known ? 0 : BCOSGPU_PBFT_E_NODE;  // PBFTEngine.cpp:735-741, :759-767
            hs[p.checks + i] = static_cast<uint8_t>(m.checks & 7u);
            mweight[i] = known ? cs.weights[m.generated_from] : 0;
            hs[p.mask + i] = m.signature_hash_len != 0;
            data_off[i] = d;
            if (m.signature_hash_len) std::memcpy(hs + p.given + 32 * i, m.signature_hash, m.signature_hash_len);
            else if (m.signed_data_len) std::memcpy(hs + p.data + d, m.signed_data, m.signed_data_len), d += m.signed_data_len;
            mrow[i] = prow[i] = -1;
            if (m.checks & BCOSGPU_PBFT_CHECK_MSG_SIG) {  // the hash kernel writes this row's hash
                cr.put(r, m.generated_from, m.signature, m.signature_len);
                mrow[i] = static_cast<int64_t>(r++);
            }
            if ((m.checks & BCOSGPU_PBFT_CHECK_PROPOSAL_SIG) && m.proposal_signature_len) {
                cr.put(r, m.generated_from, m.proposal_signature, m.proposal_signature_len);
                if (m.proposal_hash_len) std::memcpy(hs + p.rhash + 32 * r, m.proposal_hash, m.proposal_hash_len);
                prow[i] = static_cast<int64_t>(r++);
            }
            prep_off[i] = np;
            for (size_t k = 0; k < m.nprepared; ++k, ++np) {
                const bcosgpu_PrecommitProof& pp = m.prepared[k];
                prep_row[np] = q;
                for (size_t s = 0; s < pp.nproofs && (m.checks & BCOSGPU_PBFT_CHECK_PREPARED); ++s, ++q) {
                    cr.put(q, pp.proofs[s].sealer_index, pp.proofs[s].signature, pp.proofs[s].signature_len);
                    if (pp.hash_len) std::memcpy(hs + p.rhash + 32 * q, pp.hash, pp.hash_len);
                }
            }
        }
        data_off[n] = d, prep_off[n] = np, prep_row[nprep] = q;
        for (size_t g = 0; g < ngroups; ++g) {
            uint64_t* t = stage_at<uint64_t>(hs, p.groups) + 3 * g;
            t[0] = groups[g].parent, t[1] = groups[g].first, t[2] = groups[g].count;
        }
    }

    PbftCheckArgs args(uint8_t* in, uint8_t* out, void* work, uint64_t work_bytes) const {
        PbftCheckArgs a;
        a.d_data = in + p.data, a.d_data_off = stage_at<const uint64_t>(in, p.data_off);
        a.d_given32 = in + p.given, a.d_given_mask = in + p.mask, a.d_pre_flags = in + p.pre, a.d_checks = in + p.checks;
        a.d_msg_weight = stage_at<const uint64_t>(in, p.mweight);
        a.d_msg_row = stage_at<const int64_t>(in, p.mrow), a.d_prop_row = stage_at<const int64_t>(in, p.prow);
        a.d_prep_off = stage_at<const uint64_t>(in, p.prep_off);
        a.d_prep_row_off = stage_at<const uint64_t>(in, p.prep_row), a.nprep = nprep;
        a.d_row_hash32 = in + p.rhash, a.d_sig = in + p.sig, a.d_row_weight = stage_at<const uint64_t>(in, p.weight);
        cr.wire(a, in + p.key);
        a.d_groups = stage_at<const uint64_t>(in, p.groups), a.ngroups = ngroups;
        a.quorum = cs.min_required_quorum, a.n = n, a.rows = rows;
        a.d_msg_hash32 = out, a.d_msg_flags = stage_at<uint32_t>(out, p.out_flags);
        a.d_prepared_check = out + p.out_prep, a.d_sig_ok = out + p.out_ok;
        a.d_work = work, a.work_bytes = work_bytes;
        return a;
    }

    // hs: the packed block (its row maps are read back), ho: the download.  sig_ok has, per message, the message
    // signature, the proposal signature and the proofs: 2 = not requested, an absent proposal signature failed (0)
    void scatter(const uint8_t* hs, const uint8_t* ho, uint8_t* msg_hash32, uint32_t* msg_flags,
                 uint8_t* prepared_check_or_null, uint8_t* sig_ok_or_null) const {
        std::memcpy(msg_hash32, ho, 32 * n);
        std::memcpy(msg_flags, ho + p.out_flags, 4 * n);
        if (prepared_check_or_null && nprep) std::memcpy(prepared_check_or_null, ho + p.out_prep, nprep);
        if (!sig_ok_or_null) return;
        const int64_t* mrow = reinterpret_cast<const int64_t*>(hs + p.mrow);
        const int64_t* prow = reinterpret_cast<const int64_t*>(hs + p.prow);
        const uint64_t* prep_off = reinterpret_cast<const uint64_t*>(hs + p.prep_off);
        const uint64_t* prep_row = reinterpret_cast<const uint64_t*>(hs + p.prep_row);
        const uint8_t* ok = ho + p.out_ok;
        uint8_t* s = sig_ok_or_null;
        for (size_t i = 0; i < n; ++i) {
            const bcosgpu_PBFTMessageData& m = msgs[i];
            *s++ = mrow[i] >= 0 ? ok[mrow[i]] : 2;
            *s++ = prow[i] >= 0 ? ok[prow[i]] : (m.checks & BCOSGPU_PBFT_CHECK_PROPOSAL_SIG) ? 0 : 2;
            for (size_t k = 0; k < m.nprepared; ++k) {
                const size_t cnt = m.prepared[k].nproofs;
                if (m.checks & BCOSGPU_PBFT_CHECK_PREPARED) std::memcpy(s, ok + prep_row[prep_off[i] + k], cnt);
                else std::memset(s, 2, cnt);
                s += cnt;
            }
        }
    }
};

}  // namespace bcosgpu
