/*
 * bcos_gpu.hpp -- header-only C++ adapters over the C ABI (bcos_gpu.h) with the shapes of the
 * reference's interfaces, so that the reference's call sites can be rewired without other changes:
 *
 *   bcos::crypto::Hash::hash(bytesConstRef) -> h256            interfaces/crypto/Hash.h:44
 *       -> bcosgpu::GpuKeccak256 / GpuSM3 ::hash, plus batch hash_batch()
 *   bcos::crypto::SignatureCrypto::recover(HashType, bytesConstRef) -> PublicPtr (throws InvalidSignature)
 *                                                              interfaces/crypto/Signature.h:53-54
 *       -> bcosgpu::GpuSecp256k1Crypto / GpuSM2Crypto ::recover, plus recover_batch()
 *   SignatureCrypto::verify(PublicPtr, HashType, bytesConstRef) -> bool       Signature.h:45-48
 *   bcos::crypto::merkle::Merkle<Hasher, width>::generateMerkle(originHashes, out)  merkle/Merkle.h:170-208
 *       -> bcosgpu::GpuMerkle<width>::generateMerkle (same output vector layout)
 *
 * The reference's own types (bcos::bytes, h256, KeyImpl, ...) are not available here; these adapters
 * use std::vector<uint8_t> / std::array, and INTEGRATION.md shows the few lines that wrap them into a
 * bcos::crypto::SignatureCrypto subclass.  Errors from the engine throw std::runtime_error; crypto
 * failures throw bcosgpu::InvalidSignature exactly where the reference throws InvalidSignature.
 */
#ifndef BCOS_GPU_HPP
#define BCOS_GPU_HPP
#include <algorithm>
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

#include "bcos_gpu.h"

namespace bcosgpu {

using bytes = std::vector<uint8_t>;
using HashType = std::array<uint8_t, 32>;

struct InvalidSignature : std::runtime_error {
    using std::runtime_error::runtime_error;
};

inline void check(int rc) {
    if (rc != BCOSGPU_OK) throw std::runtime_error(std::string("bcosgpu: ") + bcosgpu_last_error());
}

// ---------------------------------------------------------------- Hash
template <int HASHER>
class GpuHash {
public:
    HashType hash(const uint8_t* data, size_t len) const {
        uint64_t off[2] = {0, len};
        HashType out{};
        check(bcosgpu_hash_batch(HASHER, len ? data : &zero_, off, 1, out.data()));
        return out;
    }
    HashType hash(const bytes& b) const { return hash(b.data(), b.size()); }
    /* batch: message i = data[offsets[i] .. offsets[i+1]) */
    std::vector<HashType> hash_batch(const bytes& data, const std::vector<uint64_t>& offsets) const {
        const size_t n = offsets.empty() ? 0 : offsets.size() - 1;
        std::vector<HashType> out(n);
        if (n) check(bcosgpu_hash_batch(HASHER, data.empty() ? &zero_ : data.data(), offsets.data(), n, out[0].data()));
        return out;
    }

private:
    static constexpr uint8_t zero_ = 0;
};
using GpuKeccak256 = GpuHash<BCOSGPU_KECCAK256>;
using GpuSM3 = GpuHash<BCOSGPU_SM3>;

inline std::array<uint8_t, 20> right160(const HashType& h) {
    std::array<uint8_t, 20> a{};
    for (int i = 0; i < 20; ++i) a[i] = h[12 + i];
    return a;
}

// ---------------------------------------------------------------- SignatureCrypto
class GpuSecp256k1Crypto {
public:
    static constexpr size_t SIGNATURE_LEN = 65; /* SECP256K1_SIGNATURE_LEN (Secp256k1Crypto.h:29) */
    /* Secp256k1Crypto::recover (Secp256k1Crypto.h:57-60): 64-byte public key or InvalidSignature */
    bytes recover(const HashType& hash, const uint8_t* sig, size_t sig_len) const {
        if (sig_len != SIGNATURE_LEN) throw InvalidSignature("invalid signature: secp256k1Recover failed");
        bytes pub(64);
        uint8_t ok = 0;
        check(bcosgpu_secp256k1_recover_batch(hash.data(), sig, 1, pub.data(), nullptr, &ok));
        if (!ok) throw InvalidSignature("invalid signature: secp256k1Recover failed");
        return pub;
    }
    /* batch recover: hashes n x 32, sigs n x 65 -> pubs n x 64, addrs n x 20 (keccak), ok[n] */
    void recover_batch(const uint8_t* hashes, const uint8_t* sigs, size_t n, uint8_t* pubs, uint8_t* addrs,
                       uint8_t* ok) const {
        check(bcosgpu_secp256k1_recover_batch(hashes, sigs, n, pubs, addrs, ok));
    }
    /* Secp256k1Crypto::verify -> secp256k1Verify (Secp256k1Crypto.cpp:51-63): r || s = sig[0:64] */
    bool verify(const uint8_t pub[64], const HashType& hash, const uint8_t* sig, size_t sig_len) const {
        if (sig_len < 64) return false;
        uint8_t ok = 0;
        check(bcosgpu_verify_batch(BCOSGPU_SUITE_SECP256K1, pub, hash.data(), sig, 64, 1, &ok));
        return ok != 0;
    }
    /* batch verify with known keys (sealer signatures): item i = pubs + 64 i, hashes + 32 i, sigs + stride i */
    void verify_batch(const uint8_t* pubs, const uint8_t* hashes, const uint8_t* sigs, size_t stride, size_t n,
                      uint8_t* ok) const {
        check(bcosgpu_verify_batch(BCOSGPU_SUITE_SECP256K1, pubs, hashes, sigs, stride, n, ok));
    }
};

class GpuSM2Crypto {
public:
    static constexpr size_t SIGNATURE_LEN = 64; /* SM2_SIGNATURE_LEN: r || s */
    /* SM2Crypto::verify (SM2Crypto.cpp:66-79): only sig[0:64] is used */
    bool verify(const uint8_t pub[64], const HashType& hash, const uint8_t* sig, size_t sig_len) const {
        if (sig_len < SIGNATURE_LEN) return false;
        uint8_t ok = 0;
        check(bcosgpu_verify_batch(BCOSGPU_SUITE_SM2, pub, hash.data(), sig, SIGNATURE_LEN, 1, &ok));
        return ok != 0;
    }
    void verify_batch(const uint8_t* pubs, const uint8_t* hashes, const uint8_t* sigs, size_t stride, size_t n,
                      uint8_t* ok) const {
        check(bcosgpu_verify_batch(BCOSGPU_SUITE_SM2, pubs, hashes, sigs, stride, n, ok));
    }
    /* SM2Crypto::recover (SM2Crypto.cpp:81-92): verify with the embedded key, return it */
    bytes recover(const HashType& hash, const uint8_t* sig, size_t sig_len) const {
        if (sig_len != 128) throw InvalidSignature("invalid signature: sm2 recover public key failed");
        uint8_t ok = 0;
        check(bcosgpu_sm2_verify_batch(hash.data(), sig, 1, nullptr, &ok));
        if (!ok) throw InvalidSignature("invalid signature: sm2 recover public key failed");
        return bytes(sig + 64, sig + 128);
    }
    void recover_batch(const uint8_t* hashes, const uint8_t* sigs128, size_t n, uint8_t* addrs, uint8_t* ok) const {
        check(bcosgpu_sm2_verify_batch(hashes, sigs128, n, addrs, ok));
    }
};

// ---------------------------------------------------------------- Merkle
template <int HASHER, size_t width = 2>
class GpuMerkle {
    static_assert(width >= 2, "Width too short, at least 2");

public:
    /* generateMerkle (Merkle.h:170-208): out = the reference's output vector (count records are
     * 32-byte entries with the big-endian count in bytes 0..3, as in Merkle<..>'s std::array case) */
    void generateMerkle(const std::vector<HashType>& originHashes, std::vector<HashType>& out) const {
        if (originHashes.empty()) throw std::invalid_argument("Empty input");
        out.resize(bcosgpu_merkle_size(originHashes.size(), static_cast<int>(width)));
        HashType root{};
        check(bcosgpu_merkle_root(HASHER, static_cast<int>(width), BCOSGPU_MERKLE_NEW, originHashes[0].data(),
                                  originHashes.size(), root.data(), out[0].data()));
    }
    /* generateMerkle into a vector of byte buffers -- BlockImpl's m_inner->transactionsMerkle
     * (vector<vector<char>>, BlockImpl.h:136) and merkleBench's vector<bytes> (merkleBench.cpp:53-56):
     * count records are 4-byte entries (Merkle.h:213-217 resizeTo(output, 4)), nodes 32 bytes.
     * Bytes = any resizable byte container (std::vector<char>, std::vector<uint8_t>, bcos::bytes). */
    template <class Bytes>
    void generateMerkle(const std::vector<HashType>& originHashes, std::vector<Bytes>& out) const {
        if (originHashes.empty()) throw std::invalid_argument("Empty input");
        const size_t n = originHashes.size();
        std::vector<uint8_t> flat(bcosgpu_merkle_bytes_size(n, static_cast<int>(width)));
        HashType root{};
        check(bcosgpu_merkle_root(HASHER, static_cast<int>(width), BCOSGPU_MERKLE_NEW_BYTES, originHashes[0].data(), n,
                                  root.data(), flat.data()));
        out.clear();
        auto put = [&out](const uint8_t* p, size_t len) {
            out.emplace_back(len);
            std::copy(p, p + len, reinterpret_cast<uint8_t*>(&out.back()[0]));
        };
        if (n == 1) {
            put(flat.data(), 32);
            return;
        }
        for (size_t at = 0; at < flat.size();) {
            const uint32_t cnt = (uint32_t(flat[at]) << 24) | (uint32_t(flat[at + 1]) << 16) |
                                 (uint32_t(flat[at + 2]) << 8) | uint32_t(flat[at + 3]);
            put(flat.data() + at, 4);
            at += 4;
            for (uint32_t k = 0; k < cnt; ++k, at += 32) put(flat.data() + at, 32);
        }
    }
    /* generateMerkleProof(originHashes, index, out) (Merkle.h:121-168): out is replaced (the reference
     * appends to a caller-cleared vector); index out of range throws std::invalid_argument */
    void generateMerkleProof(const std::vector<HashType>& originHashes, uint64_t index, std::vector<HashType>& out) const {
        if (originHashes.empty()) throw std::invalid_argument("Empty input");
        if (index >= originHashes.size()) throw std::invalid_argument("Out of range!");
        out.resize(bcosgpu_merkle_proof_stride(originHashes.size(), static_cast<int>(width)));
        uint32_t len = 0;
        check(bcosgpu_merkle_proofs(HASHER, static_cast<int>(width), originHashes[0].data(), originHashes.size(), &index,
                                    1, out[0].data(), &len));
        out.resize(len);
    }
    /* verifyMerkleProof(proof, hash, root) (Merkle.h:45-81); an empty proof throws std::invalid_argument */
    bool verifyMerkleProof(const std::vector<HashType>& proof, const HashType& hash, const HashType& root) const {
        if (proof.empty()) throw std::invalid_argument("Empty input proof!");
        const uint32_t len = static_cast<uint32_t>(proof.size());
        uint8_t ok = 0;
        check(bcosgpu_merkle_verify_proofs(HASHER, proof[0].data(), proof.size(), &len, hash.data(), root.data(), 0, 1, &ok));
        return ok == 1;
    }
    HashType root(const std::vector<HashType>& originHashes) const {
        if (originHashes.empty()) throw std::invalid_argument("Empty input");
        HashType r{};
        check(bcosgpu_merkle_root(HASHER, static_cast<int>(width), BCOSGPU_MERKLE_NEW, originHashes[0].data(),
                                  originHashes.size(), r.data(), nullptr));
        return r;
    }
};

/* BlockImpl::calculateTransactionRoot (BlockImpl.h:111-154): width-2 root, zero hash when empty */
template <int HASHER>
inline HashType calculateTransactionRoot(const std::vector<HashType>& txHashes) {
    if (txHashes.empty()) return HashType{};
    return GpuMerkle<HASHER, 2>().root(txHashes);
}

/* calculateTransactionRoot / calculateReceiptRoot of many blocks in one engine call; an empty block
 * gives the zero hash (BlockImpl.h:114-119, :159-163). */
template <int HASHER>
inline std::vector<HashType> calculateRoots(const std::vector<std::vector<HashType>>& blocks) {
    std::vector<uint64_t> off(blocks.size() + 1, 0);
    std::vector<HashType> leaves;
    for (size_t b = 0; b < blocks.size(); ++b) {
        leaves.insert(leaves.end(), blocks[b].begin(), blocks[b].end());
        off[b + 1] = leaves.size();
    }
    std::vector<HashType> roots(blocks.size());
    if (blocks.empty()) return roots;
    static const HashType zero{};
    check(bcosgpu_merkle_roots_batch(HASHER, 2, leaves.empty() ? zero.data() : leaves[0].data(), off.data(),
                                     blocks.size(), roots[0].data()));
    return roots;
}

/* BlockImpl::calculateReceiptRoot (BlockImpl.h:156-183) for many blocks in one engine call: every receipt
 * hashed on the GPU (impl_calculate<Hasher>(TransactionReceipt), TarsHashable.h:43-75, a set dataHash
 * used as is), then each block's width-2 root; a block without receipts gives the zero hash.
 * receiptHashes (nullable) receives every receipt's hash, blocks back to back. */
template <int HASHER>
inline std::vector<HashType> calculateReceiptRoots(const std::vector<std::vector<bcosgpu_TransactionReceiptData>>& blocks,
                                                   std::vector<HashType>* receiptHashes = nullptr) {
    std::vector<uint64_t> off(blocks.size() + 1, 0);
    std::vector<bcosgpu_TransactionReceiptData> all;
    for (size_t b = 0; b < blocks.size(); ++b) {
        all.insert(all.end(), blocks[b].begin(), blocks[b].end());
        off[b + 1] = all.size();
    }
    std::vector<HashType> roots(blocks.size());
    if (receiptHashes) receiptHashes->assign(all.size(), HashType{});
    if (blocks.empty()) return roots;
    check(bcosgpu_receipt_roots(HASHER, all.data(), off.data(), blocks.size(), roots[0].data(),
                                receiptHashes && !all.empty() ? (*receiptHashes)[0].data() : nullptr));
    return roots;
}

/* BlockImpl::calculateReceiptRoot for one block */
template <int HASHER>
inline HashType calculateReceiptRoot(const std::vector<bcosgpu_TransactionReceiptData>& receipts) {
    return calculateReceiptRoots<HASHER>({receipts})[0];
}

/* The state root of a block's dirty storage entries -- TransactionExecutor::getHash -> StateStorage::hash
 * (StateStorage.h:397-431) / KeyPageStorage::hash (KeyPageStorage.cpp:351-406): the XOR of every entry's
 * Entry::hash (Entry.h:229-309), with H(table) ^ H(key) for the entries flagged BCOSGPU_STATE_XOR_NAMES,
 * hashed and reduced on the GPU.  No entries, or only clean ones, give the zero hash. */
template <int HASHER>
inline HashType calculateStateRoot(const std::vector<bcosgpu_StateEntry>& entries, uint32_t blockVersion) {
    HashType root{};
    check(bcosgpu_state_root(HASHER, blockVersion, entries.data(), entries.size(), root.data()));
    return root;
}

/* DataEncryption::encrypt over the values of a storage write (bcos-security/bcos-security/DataEncryption.cpp:143-165:
 * AES-256-CBC or SM4-CBC under the data key, the default IV), for the batch sites of RocksDBStorage with
 * storage_security.enable=true:
 *   asyncPrepare   bcos-storage/bcos-storage/RocksDBStorage.cpp:348-353   the block commit's dirty entries
 *   setRows        :513-524
 * out[i] is the ciphertext of values[i].  With skipEmpty an empty value stays empty, as asyncPrepare's
 * `!value.empty()` leaves it (:348); setRows has no such test (:518-522) and passes skipEmpty = false, which
 * turns an empty value into one padding block.  CIPHER: BCOSGPU_CIPHER_AES256 / BCOSGPU_CIPHER_SM4. */
template <int CIPHER>
inline std::vector<std::string> encryptStorageValues(std::string_view dataKey, const std::vector<std::string_view>& values,
                                                     bool skipEmpty = true) {
    std::vector<bcosgpu_Bytes> views;
    std::vector<size_t> index;
    uint64_t cap = 0;
    for (size_t i = 0; i < values.size(); ++i) {
        if (skipEmpty && values[i].empty()) continue;
        views.push_back({reinterpret_cast<const uint8_t*>(values[i].data()), values[i].size()});
        index.push_back(i);
        cap += bcosgpu_cbc_padded_size(values[i].size());
    }
    std::vector<std::string> out(values.size());
    if (views.empty()) return out;
    bytes packed(cap);
    std::vector<uint64_t> off(views.size() + 1);
    check(bcosgpu_cbc_encrypt_batch(CIPHER, reinterpret_cast<const uint8_t*>(dataKey.data()), dataKey.size(), nullptr, 0,
                                    views.data(), views.size(), packed.data(), cap, off.data()));
    for (size_t k = 0; k < index.size(); ++k)
        out[index[k]].assign(reinterpret_cast<const char*>(packed.data() + off[k]), off[k + 1] - off[k]);
    return out;
}

/* DataEncryption::decrypt over the values of a read -- asyncGetRow (RocksDBStorage.cpp:106-108) and the batched
 * asyncGetRows (:204-205).  An empty value stays empty, as both sites leave it.  status[i] is BCOSGPU_CBC_OK, or
 * BCOSGPU_CBC_E_LENGTH / BCOSGPU_CBC_E_PADDING with an empty values[i] where the reference throws
 * DecryptException (bcos-crypto/bcos-crypto/encrypt/AESCrypto.cpp:69-72): the caller throws for the rows it needs. */
struct DecryptedStorageValues {
    std::vector<std::string> values;
    std::vector<uint8_t> status;
};
template <int CIPHER>
inline DecryptedStorageValues decryptStorageValues(std::string_view dataKey, const std::vector<std::string_view>& values) {
    std::vector<bcosgpu_Bytes> views;
    std::vector<size_t> index;
    uint64_t cap = 0;
    for (size_t i = 0; i < values.size(); ++i) {
        if (values[i].empty()) continue;
        views.push_back({reinterpret_cast<const uint8_t*>(values[i].data()), values[i].size()});
        index.push_back(i);
        cap += values[i].size();
    }
    DecryptedStorageValues r{std::vector<std::string>(values.size()), std::vector<uint8_t>(values.size(), BCOSGPU_CBC_OK)};
    if (views.empty()) return r;
    bytes packed(cap);
    std::vector<uint64_t> off(views.size() + 1);
    std::vector<uint8_t> st(views.size());
    check(bcosgpu_cbc_decrypt_batch(CIPHER, reinterpret_cast<const uint8_t*>(dataKey.data()), dataKey.size(), nullptr, 0,
                                    views.data(), views.size(), packed.data(), cap, off.data(), st.data()));
    for (size_t k = 0; k < index.size(); ++k) {
        r.values[index[k]].assign(reinterpret_cast<const char*>(packed.data() + off[k]), off[k + 1] - off[k]);
        r.status[index[k]] = st[k];
    }
    return r;
}

/* BlockHeader::hash -- impl_calculate<Hasher>(bcostars::BlockHeader) (TarsHashable.h:77-126) for a run of
 * headers: the packed preimages through one hash call; a header's non-empty dataHash is its hash (:81-85,
 * zero-filled to 32 bytes) unless flags has BCOSGPU_HEADER_RECOMPUTE. */
template <int HASHER>
inline std::vector<HashType> calculateBlockHeaderHash(const std::vector<bcosgpu_BlockHeaderData>& headers, int flags = 0) {
    const size_t n = headers.size();
    std::vector<HashType> out(n, HashType{});
    if (n == 0) return out;
    std::vector<uint64_t> off(n + 1, 0);
    bytes pre(bcosgpu_header_preimage_size(headers.data(), n, flags) + 1);
    if (bcosgpu_pack_header_preimages(headers.data(), n, flags, pre.data(), pre.size() - 1, off.data()) != BCOSGPU_OK)
        throw std::invalid_argument("bcosgpu: bad block header view");
    check(bcosgpu_hash_batch(HASHER, pre.data(), off.data(), n, out[0].data()));
    for (size_t i = 0; i < n; ++i) {
        const bcosgpu_BlockHeaderData& h = headers[i];
        if (!h.data_hash_len || (flags & BCOSGPU_HEADER_RECOMPUTE)) continue;
        out[i] = HashType{};
        std::copy(h.data_hash, h.data_hash + h.data_hash_len, out[i].begin());
    }
    return out;
}

/* What checkBlockHeaders returns: per header its hash, the verdict of BlockValidator::asyncCheckBlock
 * (BCOSGPU_HEADER_*; accepted iff < 16) and the parent link (BCOSGPU_LINK_*); per signature of every header,
 * headers back to back, 1 verified / 0 failed / 2 not checked. */
struct BlockHeaderCheck {
    std::vector<HashType> hashes;
    std::vector<uint8_t> check, link, sigOk;
    bool accepted(size_t i) const { return check[i] < 16; }
};

/* The check a syncing node runs on every downloaded block (BlockValidator::asyncCheckBlock,
 * BlockValidator.cpp:28-182, called from DownloadingQueue.cpp:407) plus the ledger's parent check
 * (LedgerImpl.h:290-312) for a run of consecutive headers in one engine call.  SUITE: BCOSGPU_SUITE_*; prevHash:
 * the hash of the header before the first one (null: the first link is reported as not checked). */
template <int SUITE>
inline BlockHeaderCheck checkBlockHeaders(const std::vector<bcosgpu_BlockHeaderData>& headers,
                                          const bcosgpu_ConsensusSet& consensus, const HashType* prevHash = nullptr,
                                          int64_t prevNumber = 0, int flags = 0) {
    const size_t n = headers.size();
    size_t nsig = 0;
    for (const bcosgpu_BlockHeaderData& h : headers) nsig += h.nsignatures;
    BlockHeaderCheck r;
    r.hashes.assign(n, HashType{});
    r.check.assign(n, 0);
    r.link.assign(n, 0);
    r.sigOk.assign(nsig, 0);
    if (n == 0) return r;
    check(bcosgpu_headers_check(SUITE, headers.data(), n, &consensus, prevHash ? prevHash->data() : nullptr, prevNumber,
                                flags, r.hashes[0].data(), r.check.data(), r.link.data(),
                                nsig ? r.sigOk.data() : nullptr));
    return r;
}

/* What checkPBFTMessages returns: per message its signatureDataHash and its verdict bits (BCOSGPU_PBFT_E_*;
 * accepted iff 0); per prepared proposal, messages back to back, BCOSGPU_PREPARED_*; per message 2 + (its
 * proofs) signature verdicts (message signature, proposal signature, proofs): 1 verified / 0 failed / 2 not
 * requested. */
struct PBFTMessageCheck {
    std::vector<HashType> hashes;
    std::vector<uint32_t> flags;
    std::vector<uint8_t> preparedCheck, sigOk;
    bool accepted(size_t i) const { return flags[i] == 0; }
};

/* Every signature of the messages a PBFT worker drained from its queue, in one engine call: checkSignature and
 * checkProposalSignature (PBFTEngine.cpp:732-771), checkPrecommitWeight (PBFTCacheProcessor.cpp:795-821) and the
 * view-change loop of isValidNewViewMsg (PBFTEngine.cpp:1238-1263; groups: a NewView and its view changes).
 * The handlers then read the verdicts; the views, the committed index and the second look at the cached precommit stay
 * theirs.  SUITE: BCOSGPU_SUITE_*. */
template <int SUITE>
inline PBFTMessageCheck checkPBFTMessages(const std::vector<bcosgpu_PBFTMessageData>& msgs,
                                          const bcosgpu_ConsensusSet& consensus,
                                          const std::vector<bcosgpu_PBFTGroup>& groups = {}) {
    const size_t n = msgs.size();
    size_t nprep = 0, nsig = 0;
    for (const bcosgpu_PBFTMessageData& m : msgs) {
        nprep += m.nprepared;
        nsig += 2;
        for (size_t p = 0; p < m.nprepared; ++p) nsig += m.prepared[p].nproofs;
    }
    PBFTMessageCheck r;
    r.hashes.assign(n, HashType{});
    r.flags.assign(n, 0);
    r.preparedCheck.assign(nprep, 0);
    r.sigOk.assign(nsig, 0);
    if (n == 0) return r;
    check(bcosgpu_pbft_check(SUITE, msgs.data(), n, groups.data(), groups.size(), &consensus, 0, r.hashes[0].data(),
                             r.flags.data(), nprep ? r.preparedCheck.data() : nullptr, r.sigOk.data()));
    return r;
}

/* EVM ecRecover precompile(bcos-executor/src/vm/Precompiled.cpp:443-482): {true, 32-byte output}
 * on success, {true, {}} on failure; `in` is read as 128 zero-padded bytes. */
inline std::pair<bool, bytes> ecRecover(const uint8_t* in, size_t len) {
    alignas(16) uint8_t buf[128] = {0};
    for (size_t i = 0; i < len && i < 128; ++i) buf[i] = in[i];
    uint8_t out[32], ok = 0;
    check(bcosgpu_ecrecover_batch(buf, 1, out, &ok));
    if (!ok) return {true, bytes()};
    return {true, bytes(out, out + 32)};
}

/* The transaction pool's admission state on the GPU (bcosgpu_txpool_*): the handle owned, the calls as members.
 * What replaces what: INTEGRATION.md, "Transaction admission with the pool's state".  A nonce is the 32-byte
 * big-endian form of TransactionImpl::nonce()'s u256. */
struct TxAdmission {
    std::vector<HashType> hashes;
    std::vector<std::array<uint8_t, 20>> senders;
    std::vector<HashType> nonces;
    std::vector<uint32_t> status;  // 0 accepted, 2, 4 or a TransactionStatus (bcos_gpu.h)
};
struct TxPoolInfo {
    uint64_t hashes, nonces, ledger, hashesCapacity, noncesCapacity, ledgerCapacity, blockNumber, blocks, errorWord;
};
class GpuTxPool {
public:
    GpuTxPool(int suite, std::string_view chainId, std::string_view groupId, int64_t blockLimitRange,
              int64_t blockNumber = 0, uint64_t initialCapacity = 0, int device = 0) {
        check(bcosgpu_txpool_create(device, suite, chainId.data(), chainId.size(), groupId.data(), groupId.size(),
                                    blockLimitRange, blockNumber, initialCapacity, &pool_));
    }
    ~GpuTxPool() { bcosgpu_txpool_destroy(pool_); }
    GpuTxPool(const GpuTxPool&) = delete;
    GpuTxPool& operator=(const GpuTxPool&) = delete;

    /* batchImportTxs (BCOSGPU_TXPOOL_FULL) / importDownloadedTxs with a proposal (BCOSGPU_TXPOOL_PROPOSAL) over
     * encoded transactions */
    TxAdmission admit(const std::vector<std::string_view>& encoded, int mode = BCOSGPU_TXPOOL_FULL) {
        const size_t n = encoded.size();
        TxAdmission r{std::vector<HashType>(n, HashType{}), std::vector<std::array<uint8_t, 20>>(n), std::vector<HashType>(n, HashType{}),
                      std::vector<uint32_t>(n, 0)};
        if (n == 0) return r;
        std::vector<uint64_t> off(n + 1, 0);
        bytes data;
        for (size_t i = 0; i < n; ++i) {
            data.insert(data.end(), encoded[i].begin(), encoded[i].end());
            off[i + 1] = data.size();
        }
        data.push_back(0);
        check(bcosgpu_txpool_admit(pool_, mode, data.data(), off.data(), n, r.hashes[0].data(), r.senders[0].data(),
                                   r.nonces[0].data(), r.status.data()));
        return r;
    }
    /* MemoryStorage::batchRemove + LedgerNonceChecker::batchInsert */
    void blockCommitted(int64_t number, const std::vector<HashType>& txHashes, const std::vector<HashType>& nonces) {
        check(bcosgpu_txpool_block_committed(pool_, number, flat(txHashes), txHashes.size(), flat(nonces), nonces.size()));
    }
    /* removeInvalidTxs */
    void remove(const std::vector<HashType>& txHashes, const std::vector<HashType>& nonces) {
        check(bcosgpu_txpool_remove(pool_, flat(txHashes), txHashes.size(), flat(nonces), nonces.size()));
    }
    /* LedgerNonceChecker::initNonceCache */
    void loadLedgerNonces(const std::vector<std::pair<int64_t, std::vector<HashType>>>& blocks) {
        std::vector<int64_t> numbers;
        std::vector<uint64_t> off{0};
        std::vector<HashType> all;
        for (const auto& b : blocks) {
            numbers.push_back(b.first);
            all.insert(all.end(), b.second.begin(), b.second.end());
            off.push_back(all.size());
        }
        check(bcosgpu_txpool_load_ledger_nonces(pool_, numbers.data(), off.data(), flat(all), blocks.size()));
    }
    TxPoolInfo info() const {
        uint64_t w[BCOSGPU_TXPOOL_INFO_WORDS] = {};
        check(bcosgpu_txpool_info(pool_, w));
        return TxPoolInfo{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8]};
    }
    /* the keys of BCOSGPU_TXPOOL_HASHES / _NONCES / _LEDGER in ascending order */
    std::vector<HashType> dump(int which) const {
        if (which < 0 || which > 2) throw std::invalid_argument("bcosgpu: bad set");
        uint64_t n = 0, w[BCOSGPU_TXPOOL_INFO_WORDS] = {};
        check(bcosgpu_txpool_info(pool_, w));
        std::vector<HashType> keys(std::max<uint64_t>(1, w[which]));
        check(bcosgpu_txpool_dump(pool_, which, keys[0].data(), keys.size(), &n));
        keys.resize(n);
        return keys;
    }

private:
    static const uint8_t* flat(const std::vector<HashType>& v) { return v.empty() ? nullptr : v[0].data(); }
    bcosgpu_txpool* pool_ = nullptr;
};

}  // namespace bcosgpu
#endif
