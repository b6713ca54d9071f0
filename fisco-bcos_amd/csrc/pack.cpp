// pack.cpp -- host-side zero-copy packer of tx-hash preimages into the SoA layout the kernels read
// (SURVEY.md §8(f)3).  Field order and encodings restate impl_calculate<Hasher>(bcostars::Transaction)
// (bcos-tars-protocol/bcos-tars-protocol/impl/TarsHashable.h:16-41): be32(version) || chainID ||
// groupID || be64(blockLimit) || nonce || to || input || abi.  Large batches are packed by a pool of
// std::threads over contiguous ranges (each range's output offset is known from a prefix sum), into
// caller memory (e.g. pinned host or HIP-registered buffers handed to bcosgpu_tx_verify_batch_dev's copy).
#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>
#include "../../include/bcos_gpu.h"

namespace {

size_t preimage_len(const bcosgpu_TransactionData& t) {
    return 4 + t.chain_id_len + t.group_id_len + 8 + t.nonce_len + t.to_len + t.input_len + t.abi_len;
}

uint8_t* put(uint8_t* o, const void* p, size_t n) {
    if (n) std::memcpy(o, p, n);
    return o + n;
}

void pack_one(const bcosgpu_TransactionData& t, uint8_t* o) {
    const uint32_t v = static_cast<uint32_t>(t.version);
    const uint8_t ver[4] = {uint8_t(v >> 24), uint8_t(v >> 16), uint8_t(v >> 8), uint8_t(v)};
    const uint64_t b = static_cast<uint64_t>(t.block_limit);
    uint8_t bl[8];
    for (int i = 0; i < 8; ++i) bl[i] = uint8_t(b >> (56 - 8 * i));
    o = put(o, ver, 4);
    o = put(o, t.chain_id, t.chain_id_len);
    o = put(o, t.group_id, t.group_id_len);
    o = put(o, bl, 8);
    o = put(o, t.nonce, t.nonce_len);
    o = put(o, t.to, t.to_len);
    o = put(o, t.input, t.input_len);
    put(o, t.abi, t.abi_len);
}

bool valid(const bcosgpu_TransactionData& t) {
    return (t.chain_id || !t.chain_id_len) && (t.group_id || !t.group_id_len) && (t.nonce || !t.nonce_len) &&
           (t.to || !t.to_len) && (t.input || !t.input_len) && (t.abi || !t.abi_len);
}

// ---- receipts: impl_calculate<Hasher>(bcostars::TransactionReceipt), TarsHashable.h:43-75.  A receipt
// with a dataHash is not hashed (:47-51), so its preimage is empty here.
size_t receipt_len(const bcosgpu_TransactionReceiptData& r) {
    if (r.data_hash_len) return 0;
    size_t s = 4 + r.gas_used_len + r.contract_address_len + 4 + r.output_len + 8;
    for (size_t l = 0; l < r.nlogs; ++l) {
        const bcosgpu_LogEntry& e = r.logs[l];
        s += e.address_len + e.data_len;
        for (size_t t = 0; t < e.ntopics; ++t) s += e.topics[t].len;
    }
    return s;
}

bool valid(const bcosgpu_TransactionReceiptData& r) {
    if (r.data_hash_len) return r.data_hash && r.data_hash_len <= 32;
    if ((!r.gas_used && r.gas_used_len) || (!r.contract_address && r.contract_address_len) ||
        (!r.output && r.output_len) || (!r.logs && r.nlogs))
        return false;
    for (size_t l = 0; l < r.nlogs; ++l) {
        const bcosgpu_LogEntry& e = r.logs[l];
        if ((!e.address && e.address_len) || (!e.data && e.data_len) || (!e.topics && e.ntopics)) return false;
        for (size_t t = 0; t < e.ntopics; ++t)
            if (!e.topics[t].data && e.topics[t].len) return false;
    }
    return true;
}

void be(uint8_t* o, uint64_t v, int bytes) {
    for (int i = 0; i < bytes; ++i) o[i] = uint8_t(v >> (8 * (bytes - 1 - i)));
}

// be32(version) || gasUsed || contractAddress || be32(status) || output ||
// for each log (address || topic_0 .. topic_k || data) || be64(blockNumber)      (TarsHashable.h:54-73)
void pack_receipt(const bcosgpu_TransactionReceiptData& r, uint8_t* o) {
    if (r.data_hash_len) return;
    uint8_t w[8];
    be(w, static_cast<uint32_t>(r.version), 4);
    o = put(o, w, 4);
    o = put(o, r.gas_used, r.gas_used_len);
    o = put(o, r.contract_address, r.contract_address_len);
    be(w, static_cast<uint32_t>(r.status), 4);
    o = put(o, w, 4);
    o = put(o, r.output, r.output_len);
    for (size_t l = 0; l < r.nlogs; ++l) {
        const bcosgpu_LogEntry& e = r.logs[l];
        o = put(o, e.address, e.address_len);
        for (size_t t = 0; t < e.ntopics; ++t) o = put(o, e.topics[t].data, e.topics[t].len);
        o = put(o, e.data, e.data_len);
    }
    be(w, static_cast<uint64_t>(r.block_number), 8);
    put(o, w, 8);
}

// ---- state entries: table || key || value, the slices StateStorage::hash (StateStorage.h:397-431) and
// Entry::hash (Entry.h:229-309) hash.  Only a MODIFIED entry's value is read (Entry.h:244-247, :281-285).
bool valid(const bcosgpu_StateEntry& e) {
    if (e.status < BCOSGPU_ENTRY_NORMAL || e.status > BCOSGPU_ENTRY_MODIFIED) return false;
    if ((!e.table && e.table_len) || (!e.key && e.key_len)) return false;
    return e.status != BCOSGPU_ENTRY_MODIFIED || e.value || !e.value_len;
}

size_t state_value_len(const bcosgpu_StateEntry& e) { return e.status == BCOSGPU_ENTRY_MODIFIED ? e.value_len : 0; }

// false when the entry's packed length reaches 2^32 (the kernels' readers take 32-bit lengths)
bool state_entry_len(const bcosgpu_StateEntry& e, uint64_t* len) {
    const uint64_t lim = 1ull << 32;
    const uint64_t t = e.table_len, k = e.key_len, v = state_value_len(e);
    if (t >= lim || k >= lim || v >= lim || t + k + v >= lim) return false;
    *len = t + k + v;
    return true;
}

// ---- block headers: impl_calculate<Hasher>(bcostars::BlockHeader), TarsHashable.h:77-126.  A header with a
// dataHash is not hashed (:81-85), so its preimage is empty here -- unless the caller asks to recompute.
bool header_given(const bcosgpu_BlockHeaderData& h, int flags) {
    return h.data_hash_len && !(flags & BCOSGPU_HEADER_RECOMPUTE);
}

size_t header_len(const bcosgpu_BlockHeaderData& h, int flags) {
    if (header_given(h, flags)) return 0;
    size_t s = 4 + h.txs_root_len + h.receipt_root_len + h.state_root_len + 8 + h.gas_used_len + 8 + 8 +
               h.extra_data_len + 8 * h.nconsensus_weights;
    for (size_t p = 0; h.parents && p < h.nparents; ++p) s += 8 + h.parents[p].block_hash_len;
    for (size_t k = 0; h.sealer_list && k < h.nsealer_list; ++k) s += h.sealer_list[k].len;
    return s;
}

// (the dataHash is checked whether or not it is used: a view that is wrong without the flag is wrong with it)
bool valid(const bcosgpu_BlockHeaderData& h) {
    if (h.data_hash_len && (!h.data_hash || h.data_hash_len > 32)) return false;
    if ((!h.parents && h.nparents) || (!h.txs_root && h.txs_root_len) || (!h.receipt_root && h.receipt_root_len) ||
        (!h.state_root && h.state_root_len) || (!h.gas_used && h.gas_used_len) || (!h.sealer_list && h.nsealer_list) ||
        (!h.extra_data && h.extra_data_len) || (!h.consensus_weights && h.nconsensus_weights))
        return false;
    for (size_t p = 0; p < h.nparents; ++p)
        if (!h.parents[p].block_hash && h.parents[p].block_hash_len) return false;
    for (size_t k = 0; k < h.nsealer_list; ++k)
        if (!h.sealer_list[k].data && h.sealer_list[k].len) return false;
    return true;
}

// be32(version) || per parent (be64(blockNumber) || blockHash) || txsRoot || receiptRoot || stateRoot ||
// be64(blockNumber) || gasUsed || be64(timestamp) || be64(sealer) || sealerList entries || extraData ||
// be64 of every weight                                                            (TarsHashable.h:90-125)
void pack_header(const bcosgpu_BlockHeaderData& h, int flags, uint8_t* o) {
    if (header_given(h, flags)) return;
    uint8_t w[8];
    be(w, static_cast<uint32_t>(h.version), 4);
    o = put(o, w, 4);
    for (size_t p = 0; p < h.nparents; ++p) {
        be(w, static_cast<uint64_t>(h.parents[p].block_number), 8);
        o = put(o, w, 8);
        o = put(o, h.parents[p].block_hash, h.parents[p].block_hash_len);
    }
    o = put(o, h.txs_root, h.txs_root_len);
    o = put(o, h.receipt_root, h.receipt_root_len);
    o = put(o, h.state_root, h.state_root_len);
    be(w, static_cast<uint64_t>(h.block_number), 8);
    o = put(o, w, 8);
    o = put(o, h.gas_used, h.gas_used_len);
    be(w, static_cast<uint64_t>(h.timestamp), 8);
    o = put(o, w, 8);
    be(w, static_cast<uint64_t>(h.sealer), 8);
    o = put(o, w, 8);
    for (size_t k = 0; k < h.nsealer_list; ++k) o = put(o, h.sealer_list[k].data, h.sealer_list[k].len);
    o = put(o, h.extra_data, h.extra_data_len);
    for (size_t k = 0; k < h.nconsensus_weights; ++k) {
        be(w, static_cast<uint64_t>(h.consensus_weights[k]), 8);
        o = put(o, w, 8);
    }
}

// items [0, n) packed by `pack(i, out + offsets[i])` on a pool of std::threads over contiguous ranges
template <class F>
void pack_parallel(size_t n, F&& pack) {
    const size_t hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t nt = std::min<size_t>(hw, std::max<size_t>(1, n / 4096));  // threads only for large batches
    if (nt == 1) {
        for (size_t i = 0; i < n; ++i) pack(i);
        return;
    }
    std::vector<std::thread> pool;
    const size_t per = (n + nt - 1) / nt;
    for (size_t k = 0; k < nt; ++k) {
        const size_t lo = std::min(n, k * per), hi = std::min(n, (k + 1) * per);
        if (lo < hi)
            pool.emplace_back([&pack, lo, hi] {
                for (size_t i = lo; i < hi; ++i) pack(i);
            });
    }
    for (auto& th : pool) th.join();
}

}  // namespace

extern "C" {

uint64_t bcosgpu_tx_preimage_size(const bcosgpu_TransactionData* txs, size_t n) {
    if (!txs) return 0;
    uint64_t s = 0;
    for (size_t i = 0; i < n; ++i) s += preimage_len(txs[i]);
    return s;
}

int bcosgpu_pack_tx_preimages(const bcosgpu_TransactionData* txs, size_t n, uint8_t* out, uint64_t cap,
                              uint64_t* offsets) {
    if (n == 0) {
        if (offsets) offsets[0] = 0;
        return BCOSGPU_OK;
    }
    if (!txs || !offsets) return BCOSGPU_E_ARG;
    offsets[0] = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!valid(txs[i])) return BCOSGPU_E_ARG;
        offsets[i + 1] = offsets[i] + preimage_len(txs[i]);
    }
    if (offsets[n] > cap || (offsets[n] && !out)) return BCOSGPU_E_ARG;
    pack_parallel(n, [&](size_t i) { pack_one(txs[i], out + offsets[i]); });
    return BCOSGPU_OK;
}

uint64_t bcosgpu_receipt_preimage_size(const bcosgpu_TransactionReceiptData* receipts, size_t n) {
    if (!receipts) return 0;
    uint64_t s = 0;
    for (size_t i = 0; i < n; ++i) s += receipt_len(receipts[i]);
    return s;
}

int bcosgpu_pack_receipt_preimages(const bcosgpu_TransactionReceiptData* receipts, size_t n, uint8_t* out,
                                   uint64_t cap, uint64_t* offsets) {
    if (n == 0) {
        if (offsets) offsets[0] = 0;
        return BCOSGPU_OK;
    }
    if (!receipts || !offsets) return BCOSGPU_E_ARG;
    offsets[0] = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!valid(receipts[i])) return BCOSGPU_E_ARG;
        offsets[i + 1] = offsets[i] + receipt_len(receipts[i]);
    }
    if (offsets[n] > cap || (offsets[n] && !out)) return BCOSGPU_E_ARG;
    pack_parallel(n, [&](size_t i) { pack_receipt(receipts[i], out + offsets[i]); });
    return BCOSGPU_OK;
}

uint64_t bcosgpu_state_entries_size(const bcosgpu_StateEntry* entries, size_t n) {
    if (!entries) return 0;
    uint64_t s = 0;
    for (size_t i = 0; i < n; ++i) s += entries[i].table_len + entries[i].key_len + state_value_len(entries[i]);
    return s;
}

int bcosgpu_pack_state_entries(const bcosgpu_StateEntry* entries, size_t n, uint8_t* out, uint64_t cap, uint64_t* off3,
                               uint8_t* kind) {
    if (n == 0) {
        if (off3) off3[0] = 0;
        return BCOSGPU_OK;
    }
    if (!entries || !off3 || !kind) return BCOSGPU_E_ARG;
    off3[0] = 0;
    for (size_t i = 0; i < n; ++i) {
        const bcosgpu_StateEntry& e = entries[i];
        uint64_t len;
        if (!valid(e) || !state_entry_len(e, &len)) return BCOSGPU_E_ARG;
        off3[3 * i + 1] = off3[3 * i] + e.table_len;
        off3[3 * i + 2] = off3[3 * i + 1] + e.key_len;
        off3[3 * i + 3] = off3[3 * i] + len;
    }
    if (off3[3 * n] > cap || (off3[3 * n] && !out)) return BCOSGPU_E_ARG;
    pack_parallel(n, [&](size_t i) {
        const bcosgpu_StateEntry& e = entries[i];
        uint8_t* o = put(out + off3[3 * i], e.table, e.table_len);
        o = put(o, e.key, e.key_len);
        put(o, e.value, state_value_len(e));
        kind[i] = static_cast<uint8_t>(static_cast<uint8_t>(e.status) | (e.flags << 4));
    });
    return BCOSGPU_OK;
}

uint64_t bcosgpu_header_preimage_size(const bcosgpu_BlockHeaderData* headers, size_t n, int flags) {
    if (!headers) return 0;
    uint64_t s = 0;
    for (size_t i = 0; i < n; ++i) s += header_len(headers[i], flags);
    return s;
}

int bcosgpu_pack_header_preimages(const bcosgpu_BlockHeaderData* headers, size_t n, int flags, uint8_t* out,
                                  uint64_t cap, uint64_t* offsets) {
    if (n == 0) {
        if (offsets) offsets[0] = 0;
        return BCOSGPU_OK;
    }
    if (!headers || !offsets) return BCOSGPU_E_ARG;
    offsets[0] = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!valid(headers[i])) return BCOSGPU_E_ARG;
        const uint64_t len = header_len(headers[i], flags);
        if (len >> 32) return BCOSGPU_E_ARG;  // the kernel's reader takes a 32-bit length
        offsets[i + 1] = offsets[i] + len;
    }
    if (offsets[n] > cap || (offsets[n] && !out)) return BCOSGPU_E_ARG;
    pack_parallel(n, [&](size_t i) { pack_header(headers[i], flags, out + offsets[i]); });
    return BCOSGPU_OK;
}

void bcosgpu_apply_receipt_data_hashes(const bcosgpu_TransactionReceiptData* receipts, size_t n, uint8_t* hashes32) {
    if (!receipts || !hashes32) return;
    for (size_t i = 0; i < n; ++i) {
        const bcosgpu_TransactionReceiptData& r = receipts[i];
        if (!r.data_hash_len || r.data_hash_len > 32 || !r.data_hash) continue;
        std::memset(hashes32 + 32 * i, 0, 32);
        std::memcpy(hashes32 + 32 * i, r.data_hash, r.data_hash_len);
    }
}

}  // extern "C"
