/*
 * bcos_gpu.h -- C ABI of the MI355X batch-verification engine for FISCO-BCOS's tx-admission and
 * block-check hot path (libbcosgpu.so).
 *
 * Drop-in boundary.  The reference reaches this path through
 *   - bcos::crypto::SignatureCrypto::recover / verify   bcos-crypto/bcos-crypto/interfaces/crypto/Signature.h:40-58
 *   - bcos::crypto::Hash::hash                          bcos-crypto/bcos-crypto/interfaces/crypto/Hash.h:44
 *   - bcos::crypto::merkle::Merkle<H,width>             bcos-crypto/bcos-crypto/merkle/Merkle.h:170-208
 * and, one level down, the wedpr / TASSL C ABI those classes bind (int8 return code, caller-owned
 * buffers): wedpr_secp256k1_recover_public_key (Secp256k1Crypto.cpp:79-93), wedpr_secp256k1_verify
 * (:51-63), fast_sm2_verify / wedpr_sm2_verify (fastsm2/fast_sm2.h:31-40, sm2/SM2Crypto.h:60-66).
 * This header exports (a) batch entry points -- what the batch sites TransactionSync::importDownloadedTxs
 * (bcos-txpool/bcos-txpool/sync/TransactionSync.cpp:516-548) and BlockImpl::calculateTransactionRoot
 * (bcos-tars-protocol/bcos-tars-protocol/protocol/BlockImpl.h:111-154) are rewired to -- and
 * (b) single-call shims with the exact wedpr signatures, so SignatureCrypto implementations can be
 * swapped without touching their callers.  include/bcos_gpu.hpp wraps (a) in the reference's C++
 * interface shapes; INTEGRATION.md shows the binding.
 *
 * Conventions: all functions return 0 on success and a negative BCOSGPU_E_* code on an API error
 * (never throw across the ABI); per-item crypto verdicts are written to caller-allocated ok[] /
 * status[] arrays (1 = valid / 0 = InvalidSignature for ok[]; 0 = ok, 1 = InvalidSignature for status[]).
 * Byte layouts are the reference's: 32-byte big-endian scalars and digests, 64-byte X||Y public keys
 * without the 0x04 prefix (Secp256k1KeyPair.h:29, SM2KeyPair.h:31), secp256k1 signatures r||s||v
 * (65 B, v = recovery id 0..3, SignatureDataWithV.h:43-61), SM2 signatures r||s||pub (128 B,
 * SignatureDataWithPub.h:55-64).  Functions are thread-safe.
 *
 * *_dev functions take DEVICE pointers and a hipStream_t (as void*; NULL = the legacy default
 * stream) and are stream-ordered: nothing is synchronised, nothing is allocated per call except the
 * engine's grow-only workspaces.  Device output pointers must be 4-byte aligned.  The other
 * functions take HOST pointers and return after the results are copied back.
 */
#ifndef BCOS_GPU_H
#define BCOS_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BCOSGPU_VERSION 1

/* error codes */
#define BCOSGPU_OK 0
#define BCOSGPU_E_ARG (-1)    /* invalid argument (size, width, null pointer) */
#define BCOSGPU_E_HIP (-2)    /* HIP runtime error (see bcosgpu_last_error) */
#define BCOSGPU_E_NODEV (-3)  /* no usable gfx950 device */
#define BCOSGPU_E_EMPTY (-4)  /* empty Merkle input: the reference throws std::invalid_argument (Merkle.h:172-175) */

/* hashers (Hash implementations: hash/Keccak256.h, hash/SM3.h) */
#define BCOSGPU_KECCAK256 0
#define BCOSGPU_SM3 1
/* signature suites (libinitializer/ProtocolInitializer.cpp:102-124) */
#define BCOSGPU_SUITE_SECP256K1 0 /* Keccak256 + Secp256k1Crypto */
#define BCOSGPU_SUITE_SM2 1       /* SM3 + (Fast)SM2Crypto */
/* Merkle variants */
#define BCOSGPU_MERKLE_NEW 0 /* Merkle<H,width>::generateMerkle (Merkle.h:170-208) */
#define BCOSGPU_MERKLE_OLD 1 /* calculateMerkleProofRoot, width 16 (ParallelMerkleProof.cpp:32-69) */
#define BCOSGPU_MERKLE_NEW_BYTES 2 /* NEW, with `levels` in the vector<bytes> layout (bcosgpu_merkle_bytes_size) */

int bcosgpu_version(void);
/* Number of visible HIP devices (0 when none). */
int bcosgpu_device_count(void);
/* Select the calling thread's device and build its constant tables (idempotent). */
int bcosgpu_init(int device);
/* Same, with flags: BCOSGPU_INIT_SMALL_TABLES skips the two 64 MiB 16-bit comb tables (the kernels
 * then use the 512 KiB 8-bit ones, as they also do when the 64 MiB allocation fails).  Flags only
 * matter at a device's first initialisation. */
#define BCOSGPU_INIT_SMALL_TABLES 1
int bcosgpu_init_ex(int device, int flags);
/* Kernel selection for the tx-verify batch (tuning / tests; the default is chosen by batch size and
 * read once from BCOSGPU_TXV_SPLIT / _OCC / _COOP and BCOSGPU_K1_F26 at the first init, never per launch):
 * split -1 by size (secp256k1 batches <= 2^15 run the small-batch kernels), 0 never, 1 always;
 * occupancy 0 by size (2 waves/SIMD for n >= 2^17), 1 or 2 forced; coop (secp256k1 small batches)
 * 3 the row kernels (one signature per workgroup on row-spread field elements, ecc_row.hip: recovery,
 * and known-key verify through bcosgpu_verify_batch*), 2 lane-trio (default; needs field 1; with split -1
 * the automatic choice among row, lane-trio, pair and one-lane kernels by rounds x latency),
 * 1 cooperative-pair, 0 split (SM2: 3 the SM2 row kernel sm2_verify_row_kernel, 2 lane-trio, 1 pair
 * kernel, 0 the one-lane kernel);
 * field (secp256k1 throughput kernels) 1 the 10 x 26-bit point arithmetic (default), 0 the 8 x 32-bit
 * one, -1 unchanged.  Every variant returns identical results. */
int bcosgpu_set_tx_kernel_policy(int split, int occupancy, int coop, int field);
/* Last error message of the calling thread. */
const char* bcosgpu_last_error(void);
/* Bytes of the reference's Merkle output vector, in 32-byte entries (Merkle.h:224-236 getMerkleSize). */
uint64_t bcosgpu_merkle_size(uint64_t n, int width);

/* ---------------------------------------------------------------- hashing (Hash::hash, batched) */
/* message i = data[offsets[i] .. offsets[i+1]), n+1 offsets; out32 = n x 32-byte digests */
int bcosgpu_hash_batch(int hasher, const uint8_t* data, const uint64_t* offsets, size_t n,
                       uint8_t* out32);
int bcosgpu_keccak256_batch(const uint8_t* data, const uint64_t* offsets, size_t n, uint8_t* out32);
int bcosgpu_sm3_batch(const uint8_t* data, const uint64_t* offsets, size_t n, uint8_t* out32);
int bcosgpu_hash_batch_dev(int hasher, const uint8_t* d_data, const uint64_t* d_offsets, size_t n,
                           uint8_t* d_out32, void* stream);

/* ---------------------------------------------------------------- Merkle (Merkle<H,width>) */
/* root32 receives the root; levels (nullable) receives bcosgpu_merkle_size(n,width) x 32 bytes laid
 * out as the reference's output vector: per level a count record (uint32 big-endian in bytes 0..3,
 * zero elsewhere) followed by the level's nodes; for n == 1 the single leaf.  variant OLD ignores
 * width (always 16) and levels; n == 0 returns H("") for OLD and BCOSGPU_E_EMPTY for NEW.
 * Variant NEW_BYTES: as NEW, with levels in the packed vector<bytes> layout (below). */
int bcosgpu_merkle_root(int hasher, int width, int variant, const uint8_t* leaves32, size_t n,
                        uint8_t* root32, uint8_t* levels);
/* d_tree must hold bcosgpu_merkle_size(n,width) x 32 bytes (>= 32 for n == 1). */
int bcosgpu_merkle_root_dev(int hasher, int width, const uint8_t* d_leaves32, size_t n,
                            uint8_t* d_tree, uint8_t* d_root32, void* stream);
/* The stored-tree layout of BlockImpl (m_inner->transactionsMerkle, a vector<vector<char>>,
 * BlockImpl.h:136) and merkleBench (vector<bytes>, merkleBench.cpp:53-56): generateMerkle into a
 * vector of byte buffers leaves each count record a 4-byte entry (setNumberToHash -> resizeTo(out, 4),
 * Merkle.h:213-217, concepts/bcos-concepts/Basic.h:50-61) and each node a 32-byte one.  Packed: the
 * entries back to back, count record (BE u32, 4 bytes) then that level's nodes (32 bytes each);
 * bcosgpu_merkle_bytes_size(n, width) bytes (32 for n == 1).  The 32-byte-entry layout above is the
 * one of fixed-size HashType vectors (Ledger proofs, LedgerTypeDef.h:27).
 * bcosgpu_merkle_tree_bytes_dev converts an output vector d_tree (of bcosgpu_merkle_root_dev for the
 * same n, width) into that layout at d_out (4-byte aligned, not overlapping d_tree);
 * bcosgpu_merkle_root(..., BCOSGPU_MERKLE_NEW_BYTES, ..., levels) returns it directly. */
uint64_t bcosgpu_merkle_bytes_size(uint64_t n, int width);
int bcosgpu_merkle_tree_bytes_dev(int width, const uint8_t* d_tree, size_t n, uint8_t* d_out, void* stream);

/* Multi-GPU tx root: compute `levels` levels of the reference tree over one shard of leaves.  The
 * shard's first global leaf index must be a multiple of width^levels; then its ceil(n / width^levels)
 * output nodes are exactly the reference's level-`levels` nodes for that range, and the root over the
 * concatenated frontiers of all shards (bcosgpu_merkle_root*) equals the single-device root.
 * d_work >= 64 * ceil(n / width) bytes; d_frontier receives ceil(n / width^levels) x 32 bytes. */
int bcosgpu_merkle_frontier_dev(int hasher, int width, const uint8_t* d_leaves32, size_t n, int levels,
                                uint8_t* d_work, uint8_t* d_frontier, void* stream);

/* Many blocks' roots in one call: BlockImpl::calculateTransactionRoot / calculateReceiptRoot
 * (bcos-tars-protocol/.../protocol/BlockImpl.h:111-183) for a batch of blocks, e.g. PBFT/sync replay.
 * Block b's leaves are entries [block_off[b], block_off[b+1]) of leaves32 (block_off: HOST array of
 * nblocks + 1 non-decreasing entry indices; leaves32 points at entry block_off[0]).  roots32[b] =
 * Merkle<H,width> root of block b; an empty block yields the zero hash (BlockImpl.h:114-119).
 * d_work >= bcosgpu_merkle_roots_work_size(block_off[nblocks] - block_off[0], nblocks, width) bytes. */
uint64_t bcosgpu_merkle_roots_work_size(uint64_t total_leaves, size_t nblocks, int width);
int bcosgpu_merkle_roots_batch(int hasher, int width, const uint8_t* leaves32, const uint64_t* block_off,
                               size_t nblocks, uint8_t* roots32);
int bcosgpu_merkle_roots_batch_dev(int hasher, int width, const uint8_t* d_leaves32, const uint64_t* block_off,
                                   size_t nblocks, uint8_t* d_work, uint8_t* d_roots32, void* stream);

/* Merkle proofs (Merkle<H,width>::generateMerkleProof / verifyMerkleProof, Merkle.h:45-168; callers
 * Ledger::getTransactionProof and the RPC proof queries).  A proof is a sequence of 32-byte entries:
 * per level below the root a count record (BE u32 in bytes 0..3) and the <= width nodes of the group
 * that contains the node (for a 1-leaf tree: the single leaf).  Proofs are written at a fixed stride
 * of bcosgpu_merkle_proof_stride(n, width) entries; proof_len[q] = entries used.
 * Index >= n is BCOSGPU_E_ARG ("Out of range!", Merkle.h:124-127).  Verification: ok[q] = 1 / 0, or
 * 2 for an empty proof (the reference throws std::invalid_argument{"Empty input proof!"}).  Roots: one
 * per proof (per_proof_root = 1) or one shared root (0). */
uint64_t bcosgpu_merkle_proof_stride(uint64_t n, int width);
int bcosgpu_merkle_proofs(int hasher, int width, const uint8_t* leaves32, size_t n, const uint64_t* index, size_t m,
                          uint8_t* proofs, uint32_t* proof_len);
/* d_tree = the output vector of bcosgpu_merkle_root_dev for the same leaves and width */
int bcosgpu_merkle_proofs_dev(int width, const uint8_t* d_leaves32, size_t n, const uint8_t* d_tree,
                              const uint64_t* d_index, size_t m, uint8_t* d_proofs, uint32_t* d_proof_len, void* stream);
int bcosgpu_merkle_verify_proofs(int hasher, const uint8_t* proofs, uint64_t stride, const uint32_t* proof_len,
                                 const uint8_t* hashes32, const uint8_t* roots32, int per_proof_root, size_t m,
                                 uint8_t* ok);
int bcosgpu_merkle_verify_proofs_dev(int hasher, const uint8_t* d_proofs, uint64_t stride, const uint32_t* d_proof_len,
                                     const uint8_t* d_hashes32, const uint8_t* d_roots32, int per_proof_root, size_t m,
                                     uint8_t* d_ok, void* stream);

/* ---------------------------------------------------------------- signatures (SignatureCrypto, batched) */
/* The host-pointer signature calls below (batched, single and the wedpr shims) are jobs of a
 * per-device queue: concurrent callers are coalesced into shared launches, each batch taking the
 * kernel the batch size calls for (the lane-trio / pair kernels for small batches, the one-lane kernel
 * at occupancy 1 or 2 for large ones; see bcosgpu_set_tx_kernel_policy).  Results are per call.
 * secp256k1 public-key recovery (Secp256k1Crypto::recover, Secp256k1Crypto.h:57-60).
 * pub64 / addr20 nullable; addr20 = right160(Keccak256(pub)) (calculateAddress, KeyPair.h:30-33). */
int bcosgpu_secp256k1_recover_batch(const uint8_t* hash32, const uint8_t* sig65, size_t n,
                                    uint8_t* pub64, uint8_t* addr20, uint8_t* ok);
int bcosgpu_secp256k1_recover_batch_dev(const uint8_t* d_hash32, const uint8_t* d_sig65, size_t n,
                                        uint8_t* d_pub64, uint8_t* d_addr20, uint8_t* d_ok,
                                        void* stream);
/* SM2 verify with the embedded public key (SM2Crypto::recover, SM2Crypto.cpp:81-92).
 * addr20 = right160(SM3(pub)), nullable. */
int bcosgpu_sm2_verify_batch(const uint8_t* hash32, const uint8_t* sig128, size_t n,
                             uint8_t* addr20, uint8_t* ok);
int bcosgpu_sm2_verify_batch_dev(const uint8_t* d_hash32, const uint8_t* d_sig128, size_t n,
                                 uint8_t* d_addr20, uint8_t* d_ok, void* stream);
/* Key derivation + deterministic signing (SignatureCrypto::createKeyPair / sign), used to build
 * synthetic signed batches on the device.  TEST / BENCHMARK USE ONLY: not constant-time (the comb
 * gather addresses depend on key and nonce bits) -- the reference signs on the host.  Nonce k = H(sk || hash) mod n (H = Keccak256 for
 * secp256k1, SM3 for SM2); sig65 = r||s||v (low-S, libsecp256k1 convention), sig128 = r||s||pub.
 * ok[i] = 0 when sk is out of range or the nonce is degenerate. */
int bcosgpu_secp256k1_sign_batch_dev(const uint8_t* d_sk32, const uint8_t* d_hash32, size_t n,
                                     uint8_t* d_pub64, uint8_t* d_sig65, uint8_t* d_ok, void* stream);
int bcosgpu_sm2_sign_batch_dev(const uint8_t* d_sk32, const uint8_t* d_hash32, size_t n,
                               uint8_t* d_sig128, uint8_t* d_ok, void* stream);

/* SignatureCrypto::verify(pub, hash, sig) with a KNOWN key (Signature.h:40-46), batched -- the sealer
 * signature checks BlockValidator::checkSignatureList (bcos-pbft/.../engine/BlockValidator.cpp:141-182)
 * and PBFTCacheProcessor::checkPrecommitWeight (.../cache/PBFTCacheProcessor.cpp:795-821).
 *   secp256k1: secp256k1Verify -> wedpr_secp256k1_verify (Secp256k1Crypto.cpp:51-63), libsecp256k1
 *              secp256k1_ecdsa_verify semantics (low-S required, pub on the curve);
 *   SM2:       SM2Crypto::verify (SM2Crypto.cpp:66-79) -> sm2_do_verify against the given key.
 * Item i: pub64 + 64 i, hash32 + 32 i, signature sig + sig_stride i (stride >= 64: 65 for r||s||v,
 * 128 for r||s||pub; only bytes 0..63 = r||s are read).  ok[i] = 1 iff the signature verifies. */
int bcosgpu_verify_batch(int suite, const uint8_t* pub64, const uint8_t* hash32, const uint8_t* sig,
                         size_t sig_stride, size_t n, uint8_t* ok);
int bcosgpu_verify_batch_dev(int suite, const uint8_t* d_pub64, const uint8_t* d_hash32, const uint8_t* d_sig,
                             size_t sig_stride, size_t n, uint8_t* d_ok, void* stream);

/* Registered keys: the sealer path.  BlockValidator::checkSignatureList and
 * PBFTCacheProcessor::checkPrecommitWeight verify against the consensus node list's keys -- a small
 * set known in advance (ConsensusNode list; PBFTConfig).  A registered key gets an 8-bit comb table of
 * its multiples in HBM (512 KiB, built once), so verifying against it needs table lookups and ~7 point
 * additions instead of a variable-base multiplication (~10x shorter per signature; same verdicts).
 *   bcosgpu_register_keys: tables for n keys (pub64 + 64 i) of `suite` on `device`; slots[i] = the key's
 *     slot id (opaque, >= 0), or -1 when the cache is full (BCOSGPU_KEY_CACHE keys per device and suite,
 *     default 256).  Returns the number of keys cached (< 0 on error).  Registering a cached key is a lookup.
 *   Host-pointer verify calls (bcosgpu_verify_batch, bcosgpu_secp256k1_verify, bcosgpu_sm2_verify, the
 *     device-set batches, SM2 recover) take the registered-key kernel when every key of the coalesced
 *     batch is cached.  A key NAMED (pub64 given: the sealer path) in BCOSGPU_KEY_PROMOTE (default 3;
 *     0 = never) verify calls is cached automatically -- counted once per call, at most 16 new tables per
 *     call, in at most half the capacity (the other half is kept for registrations); SM2 recover
 *     (admission, the sender's embedded key) only looks keys up.
 *   bcosgpu_verify_keyed_batch_dev: ok[i] = verify(key of slot id d_slots[i], d_hash32 + 32 i, d_sig +
 *     sig_stride i) on the calling thread's device, stream-ordered; an id that names no registered key
 *     fails (ok = 0) -- including every id handed out before a bcosgpu_clear_keys: ids carry the cache
 *     generation, so an old id never verifies against a key registered later in the same index.
 *   bcosgpu_key_cache_info: out5 = {keys cached, capacity, verified on the keyed path, verified
 *     elsewhere, tables built}.  bcosgpu_clear_keys: drains the device, then forgets every key (a
 *     consensus membership change); later registrations get new ids (a coalesced batch that looked its
 *     keys up before the clear runs again on the generic kernels). */
int bcosgpu_register_keys(int device, int suite, const uint8_t* pub64, size_t n, int32_t* slots);
int bcosgpu_verify_keyed_batch_dev(int suite, const int32_t* d_slots, const uint8_t* d_hash32, const uint8_t* d_sig,
                                   size_t sig_stride, size_t n, uint8_t* d_ok, void* stream);
int bcosgpu_key_cache_info(int device, int suite, int64_t* out5);
int bcosgpu_clear_keys(int device, int suite);

/* EVM ecRecover precompile (bcos-executor/src/vm/Precompiled.cpp:443-482), batched.  Input i =
 * in128 + 128 i = hash(32) || v(32) || r(32) || s(32); the recovery id is (uint8_t)(in[63] - 27).
 * On success out32 = 12 zero bytes || right160(Keccak256(pub)) and ok = 1; on failure the precompile
 * returns an empty output: ok = 0 (out32 zero).  d_in128 must be 16-byte aligned. */
int bcosgpu_ecrecover_batch(const uint8_t* in128, size_t n, uint8_t* out32, uint8_t* ok);
int bcosgpu_ecrecover_batch_dev(const uint8_t* d_in128, size_t n, uint8_t* d_out32, uint8_t* d_ok, void* stream);

/* ---------------------------------------------------------------- whole-tx admission (Transaction::verify, batched) */
/* Transaction::verify (bcos-framework/.../protocol/Transaction.h:68-82) for n transactions:
 * txhash = H(preimage) (TarsHashable.h:16-41), pub = recover(txhash, sig), sender = right160(H(pub)).
 * preimage i = pre[pre_off[i] .. pre_off[i+1]); signature i = sig[sig_off[i] .. sig_off[i+1]).
 * status[i] = 0 (ok) or 1 (TransactionStatus::InvalidSignature); sender20 zero when invalid. */
int bcosgpu_tx_verify_batch(int suite, const uint8_t* pre, const uint64_t* pre_off,
                            const uint8_t* sig, const uint64_t* sig_off, size_t n,
                            uint8_t* txhash32, uint8_t* sender20, uint8_t* status);
int bcosgpu_tx_verify_batch_dev(int suite, const uint8_t* d_pre, const uint64_t* d_pre_off,
                                const uint8_t* d_sig, const uint64_t* d_sig_off, size_t n,
                                uint8_t* d_txhash32, uint8_t* d_sender20, uint8_t* d_status,
                                void* stream);

/* ---------------------------------------------------------------- Tars-encoded transactions */
/* Batched TransactionFactoryImpl::createTransaction(txData, checkSig, checkHash)
 * (bcos-tars-protocol/bcos-tars-protocol/protocol/TransactionFactoryImpl.h:46-85), decode included:
 * decode n Tars-encoded bcostars::Transaction (TransactionImpl.cpp:38-41 -> TarsSerializable.h:28-35, the
 * tarscpp wire format), recompute the tx hash and, when check_sig, recover / verify the signature and
 * derive the sender (sender = 0 otherwise).  Callers: JsonRpcImpl_2_0.cpp:443-444 (sendTransaction,
 * checkSig false, checkHash true), TxPool.cpp:96 (pushed txs, checkSig false).
 * Encoded tx i = enc[enc_off[i] .. enc_off[i+1]).  status[i]: 0 ok, 1 InvalidSignature (verify throws),
 * 2 the decode throws, 3 check_hash != 0 and a non-empty dataHash differs from the recomputed hash. */
int bcosgpu_tars_tx_verify_batch(int suite, const uint8_t* enc, const uint64_t* enc_off, size_t n, int check_sig,
                                 int check_hash, uint8_t* txhash32, uint8_t* sender20, uint8_t* status);
/* Work buffer for the device entry points below: >= bcosgpu_tars_decode_work_size(n) bytes. */
uint64_t bcosgpu_tars_decode_work_size(size_t n);
/* Device decode only: writes the packed preimages / signatures in the layout bcosgpu_tx_verify_batch_dev
 * takes.  d_pre >= enc bytes + 12 n, d_sig >= enc bytes, d_pre_off / d_sig_off n + 1 entries,
 * d_dec_status n bytes (0 / 2; may be null). */
int bcosgpu_tars_tx_decode_dev(const uint8_t* d_enc, const uint64_t* d_enc_off, size_t n, uint8_t* d_pre,
                               uint64_t* d_pre_off, uint8_t* d_sig, uint64_t* d_sig_off, uint8_t* d_dec_status,
                               void* d_work, uint64_t work_bytes, void* stream);
/* Device decode + verify, stream-ordered (the buffers as for bcosgpu_tars_tx_decode_dev). */
int bcosgpu_tars_tx_verify_batch_dev(int suite, const uint8_t* d_enc, const uint64_t* d_enc_off, size_t n,
                                     int check_sig, int check_hash, uint8_t* d_pre, uint64_t* d_pre_off, uint8_t* d_sig,
                                     uint64_t* d_sig_off, void* d_work, uint64_t work_bytes, uint8_t* d_txhash32,
                                     uint8_t* d_sender20, uint8_t* d_status, void* stream);

/* ---------------------------------------------------------------- transaction admission with the pool's state */
/* The checks the batch sites make around Transaction::verify, against state that lives in HBM across calls:
 *   MemoryStorage::verifyAndSubmitTransaction  bcos-txpool/bcos-txpool/txpool/storage/MemoryStorage.cpp:223-273
 *       (under batchImportTxs), with TxValidator::verify  .../txpool/validator/TxValidator.cpp:27-69,
 *       TxPoolNonceChecker::checkNonce  .../validator/TxPoolNonceChecker.cpp:34-49 and
 *       LedgerNonceChecker::checkNonce / checkBlockLimit / batchInsert  .../validator/LedgerNonceChecker.cpp:36-99
 *   MemoryStorage::enforceSubmitTransaction    MemoryStorage.cpp:147-221 (importDownloadedTxs with a proposal)
 *   MemoryStorage::batchRemove                 MemoryStorage.cpp:435-498, and removeInvalidTxs
 * A pool owns three sets of 32-byte keys, each a strictly ascending array (ascending as a big-endian 256-bit
 * number) with a device-side count: the pool's tx hashes (m_txsTable's keys), the pool's nonces, the ledger's
 * nonces of the last block_limit_range blocks; plus the per-block nonce lists of
 * LedgerNonceChecker::m_blockNonceCache (host copies), chain id, group id, block_limit_range and the current block
 * number.  A nonce is TransactionImpl::nonce()'s u256 (TransactionImpl.cpp:62-68) as a 32-byte big-endian key;
 * only canonical strings are parsed (empty, or 1..78 digits without a leading 0 unless "0", below 2^256): any
 * other transaction gets status 4 and is left to the host's own code.
 * One mutex and one stream per pool: calls on one pool are serialised, every call returns after its work on the
 * pool's stream has finished, and an error return leaves nothing of the call running.  n == 0 is BCOSGPU_OK and
 * changes nothing.  A kernel that would store outside a buffer skips the store and sets the pool's error word;
 * the call then returns BCOSGPU_E_ENGINE, and so does every later call on that pool except info and destroy. */
#define BCOSGPU_E_ENGINE (-5) /* the pool's error word is set (see bcosgpu_txpool_info) */
typedef struct bcosgpu_txpool bcosgpu_txpool;
#define BCOSGPU_TXPOOL_FULL 0     /* batchImportTxs: every check, the batch judged in index order */
#define BCOSGPU_TXPOOL_PROPOSAL 1 /* enforceSubmitTransaction: decode, nonce against the ledger, signature */
#define BCOSGPU_TXPOOL_HASHES 0
#define BCOSGPU_TXPOOL_NONCES 1
#define BCOSGPU_TXPOOL_LEDGER 2
/* per-transaction status (uint32): 0 accepted, 2 the decode throws, 4 nonce string not canonical, and
 * TransactionStatus (bcos-protocol/TransactionStatus.h): 10000 NonceCheckFail, 10001 BlockLimitCheckFail,
 * 10004 AlreadyInTxPool, 10006 InvalidChainId, 10007 InvalidGroupId, 10008 InvalidSignature */
/* initial_capacity: keys per set before the first growth (0 = 4096); sets grow by at least doubling, between
 * calls.  0 <= block_number, block_limit_range <= 2^62. */
int bcosgpu_txpool_create(int device, int suite, const char* chain_id, size_t chain_len, const char* group_id,
                          size_t group_len, int64_t block_limit_range, int64_t block_number, uint64_t initial_capacity,
                          bcosgpu_txpool** out);
int bcosgpu_txpool_destroy(bcosgpu_txpool* pool);
/* Decode + verify n Tars-encoded transactions as the device call above does with check_sig on and check_hash
 * off, then judge them.  FULL: in the order hash in the pool (10004), group (10007), chain (10006), nonce not
 * canonical (4), nonce in the pool (10000), nonce in the ledger (10000), block limit (number >= limit or number +
 * range < limit: 10001), signature (10008), as if one after another: an accepted transaction's nonce and hash are in
 * the sets when the next one is judged.  PROPOSAL: 2, 4, 10000 (ledger only), 10008 or 0, no rule between the
 * transactions of the batch; the accepted hashes enter the pool's table.
 * Outputs per transaction: txhash32 (zero when the decode throws), sender20 (zero unless status 0), nonce32 (zero
 * unless canonical), status. */
int bcosgpu_txpool_admit(bcosgpu_txpool* pool, int mode, const uint8_t* enc, const uint64_t* enc_off, size_t n,
                         uint8_t* txhash32, uint8_t* sender20, uint8_t* nonce32, uint32_t* status);
/* The same over device buffers (enc_bytes: the readable bytes at d_enc, at least d_enc_off[n]; d_status 4-byte
 * aligned).  Runs on the pool's stream: the inputs must be complete before the call, the outputs are complete when
 * it returns. */
int bcosgpu_txpool_admit_dev(bcosgpu_txpool* pool, int mode, const uint8_t* d_enc, const uint64_t* d_enc_off, size_t n,
                             uint64_t enc_bytes, uint8_t* d_txhash32, uint8_t* d_sender20, uint8_t* d_nonce32,
                             uint32_t* d_status);
/* A block went to the ledger (batchRemove + LedgerNonceChecker::batchInsert; host pointers, duplicates allowed):
 * hashes -= txhashes; the pool's block number advances to `number`; ledger += nonces; nonces -= nonces; the list
 * is remembered under `number` unless that number already has one; block number - block_limit_range expires:
 * ledger -= its remembered list. */
int bcosgpu_txpool_block_committed(bcosgpu_txpool* pool, int64_t number, const uint8_t* txhashes32, size_t nhashes,
                                   const uint8_t* nonces32, size_t nnonces);
/* removeInvalidTxs: hashes -= txhashes, nonces -= nonces. */
int bcosgpu_txpool_remove(bcosgpu_txpool* pool, const uint8_t* txhashes32, size_t nhashes, const uint8_t* nonces32,
                          size_t nnonces);
/* LedgerNonceChecker::initNonceCache (:26-34): block b's nonces are nonces32[32 nonce_off[b] .. 32 nonce_off[b+1]);
 * every list is remembered (replacing an earlier one of that number), every nonce enters the ledger set. */
int bcosgpu_txpool_load_ledger_nonces(bcosgpu_txpool* pool, const int64_t* numbers, const uint64_t* nonce_off,
                                      const uint8_t* nonces32, size_t nblocks);
/* out: counts of hashes / nonces / ledger, their capacities, the block number, the remembered blocks, the error
 * word (0 = no kernel ever refused a store or a count). */
#define BCOSGPU_TXPOOL_INFO_WORDS 9
int bcosgpu_txpool_info(bcosgpu_txpool* pool, uint64_t out[BCOSGPU_TXPOOL_INFO_WORDS]);
/* A set's keys in ascending order (tests, diagnosis): *count receives the set's count; keys32 must hold it
 * (capacity in keys), else BCOSGPU_E_ARG. */
int bcosgpu_txpool_dump(bcosgpu_txpool* pool, int which, uint8_t* keys32, uint64_t capacity, uint64_t* count);

/* ---------------------------------------------------------------- host-side preimage packer */
/* A view of bcostars::TransactionData (bcos-tars-protocol/.../tars/Transaction.tars:2-11): pointers
 * into the caller's decoded transaction, nothing is copied until packing. */
typedef struct {
    int32_t version;
    const char* chain_id;  size_t chain_id_len;
    const char* group_id;  size_t group_id_len;
    int64_t block_limit;
    const char* nonce;     size_t nonce_len;
    const char* to;        size_t to_len;
    const uint8_t* input;  size_t input_len;
    const char* abi;       size_t abi_len;
} bcosgpu_TransactionData;
/* Total preimage bytes of n transactions. */
uint64_t bcosgpu_tx_preimage_size(const bcosgpu_TransactionData* txs, size_t n);
/* Packs the tx-hash preimages impl_calculate<Hasher>(Transaction) hashes (TarsHashable.h:16-41:
 * be32(version) || chainID || groupID || be64(blockLimit) || nonce || to || input || abi) back to
 * back into out (cap bytes) and writes offsets[n+1] -- the SoA layout bcosgpu_tx_verify_batch* take.
 * Host only (no device needed); multithreaded for large batches.  BCOSGPU_E_ARG if cap is too small. */
int bcosgpu_pack_tx_preimages(const bcosgpu_TransactionData* txs, size_t n, uint8_t* out, uint64_t cap,
                              uint64_t* offsets);

/* ---------------------------------------------------------------- receipts (calculateReceiptRoot) */
/* Views of bcostars::LogEntry / TransactionReceiptData / TransactionReceipt.dataHash
 * (bcos-tars-protocol/bcos-tars-protocol/tars/TransactionReceipt.tars:2-23): pointers into the caller's
 * decoded receipt.  topic is vector<vector<byte>>: ntopics byte strings. */
typedef struct { const uint8_t* data; size_t len; } bcosgpu_Bytes;
typedef struct {
    const char* address;   size_t address_len;
    const bcosgpu_Bytes* topics; size_t ntopics;
    const uint8_t* data;   size_t data_len;
} bcosgpu_LogEntry;
typedef struct {
    int32_t version;
    const char* gas_used;          size_t gas_used_len;
    const char* contract_address;  size_t contract_address_len;
    int32_t status;
    const uint8_t* output;         size_t output_len;
    const bcosgpu_LogEntry* logs;  size_t nlogs;
    int64_t block_number;
    /* TransactionReceipt.dataHash: when non-empty it IS the receipt hash (TarsHashable.h:47-51) and the
     * fields above are not read.  At most 32 bytes (the reference's assignTo into a 32-byte hash throws
     * NoEnoughSpace beyond that); a shorter one fills the leading bytes, the rest are zero here (the
     * reference leaves them uninitialised, BlockImpl.h:171). */
    const uint8_t* data_hash;      size_t data_hash_len;
} bcosgpu_TransactionReceiptData;
/* Total preimage bytes of n receipts (0 for a receipt with a dataHash). */
uint64_t bcosgpu_receipt_preimage_size(const bcosgpu_TransactionReceiptData* receipts, size_t n);
/* Packs the receipt-hash preimages impl_calculate<Hasher>(TransactionReceipt) hashes
 * (TarsHashable.h:54-73: be32(version) || gasUsed || contractAddress || be32(status) || output ||
 * per log (address || topic_0 .. topic_k || data) || be64(blockNumber)) back to back into out (cap bytes)
 * and writes offsets[n+1]; a receipt with a dataHash gets an empty preimage.  Host only, multithreaded
 * for large batches.  BCOSGPU_E_ARG if cap is too small, a field pointer is null with a non-zero length,
 * or a dataHash is longer than 32 bytes. */
int bcosgpu_pack_receipt_preimages(const bcosgpu_TransactionReceiptData* receipts, size_t n, uint8_t* out,
                                   uint64_t cap, uint64_t* offsets);
/* hashes32[i] = receipt i's dataHash for every receipt that has one (host only; the step after hashing
 * the packed preimages). */
void bcosgpu_apply_receipt_data_hashes(const bcosgpu_TransactionReceiptData* receipts, size_t n, uint8_t* hashes32);
/* BlockImpl::calculateReceiptRoot (bcos-tars-protocol/.../protocol/BlockImpl.h:156-183) for nblocks blocks
 * in one call: block b's receipts are receipts[block_off[b] .. block_off[b+1]) (HOST array, block_off[0] =
 * 0); every receipt hashed on the GPU with `hasher` (impl_calculate, dataHash short-circuit), then
 * roots32 + 32 b = Merkle<H, 2> root of block b's receipt hashes (zero hash for a block without
 * receipts, BlockImpl.h:159-163).  hashes32 (nullable) receives the block_off[nblocks] receipt hashes. */
int bcosgpu_receipt_roots(int hasher, const bcosgpu_TransactionReceiptData* receipts, const uint64_t* block_off,
                          size_t nblocks, uint8_t* roots32, uint8_t* hashes32);

/* ---------------------------------------------------------------- state root (StateStorage::hash / KeyPageStorage::hash) */
/* The third root of a block header (bcos-scheduler/src/BlockExecutive.cpp:1120-1126), from
 * TransactionExecutor::getHash -> storage->hash(hashImpl) (bcos-executor/src/executor/TransactionExecutor.cpp:1099):
 * the 256-bit XOR, over the block's dirty storage entries, of each entry's contribution
 *   StateStorage::hash (bcos-table/src/StateStorage.h:397-431):
 *       H(table) ^ H(key) ^ Entry::hash(table, key, H, blockVersion)
 *   KeyPageStorage::hash (bcos-table/src/KeyPageStorage.cpp:351-406), a system-table entry (:385-390): the same
 *   PageData::hash (bcos-table/src/KeyPageStorage.h:862-893), a page entry: Entry::hash alone at block version
 *       >= 3.1 (:873-876), H(table) ^ H(key) ^ Entry::hash at 3.0 (:877-881)
 *   Entry::hash (bcos-framework/bcos-framework/storage/Entry.h:229-309):
 *       blockVersion >= V3_1_VERSION 0x03010000 (:233): MODIFIED H(table || key || value) (:239-248),
 *                                                       DELETED H(table || key) (:258-260)
 *       3.0 (:279-307): MODIFIED H(value) (:281-285), DELETED HashType(0x1) = 31 zero bytes then 0x01
 *                                                       (:293-295, bcos-utilities/bcos-utilities/FixedBytes.h:171)
 *       a clean entry (NORMAL, EMPTY) is not dirty and contributes nothing (:269-274, :302-306, StateStorage.h:412)
 * XOR is exact and commutative: entries may be given in any order. */
/* Entry::Status (Entry.h) */
#define BCOSGPU_ENTRY_NORMAL 0
#define BCOSGPU_ENTRY_DELETED 1
#define BCOSGPU_ENTRY_EMPTY 2
#define BCOSGPU_ENTRY_MODIFIED 3
/* per-entry flag: the entry also contributes H(table) ^ H(key).  Set for every StateStorage entry
 * (StateStorage.h:414), every KeyPage system-table entry (KeyPageStorage.cpp:386-388) and every KeyPage page
 * entry when the block version is 3.0 (KeyPageStorage.h:879); not for a page entry from 3.1 on (:875). */
#define BCOSGPU_STATE_XOR_NAMES 1
/* A view of one storage entry: pointers into the caller's storage, nothing is copied until packing.  value is
 * read only when status is MODIFIED. */
typedef struct {
    const char* table;     size_t table_len;
    const char* key;       size_t key_len;
    const uint8_t* value;  size_t value_len;
    int8_t status;  /* BCOSGPU_ENTRY_* */
    uint8_t flags;  /* BCOSGPU_STATE_XOR_NAMES */
} bcosgpu_StateEntry;
/* Total packed bytes of n entries (table + key, plus the value of a MODIFIED entry). */
uint64_t bcosgpu_state_entries_size(const bcosgpu_StateEntry* entries, size_t n);
/* Packs table || key || value of every entry back to back into out (cap bytes): off3 has 3n+1 entries,
 * off3[3i], off3[3i+1], off3[3i+2] the starts of entry i's table, key and value and off3[3i+3] its value's end,
 * so H(table), H(key), H(value), H(table||key) and H(table||key||value) are all contiguous slices; kind[i] =
 * status | flags << 4.  A DELETED or clean entry packs no value bytes.  Host only, multithreaded for large
 * batches.  BCOSGPU_E_ARG if cap is too small, a pointer is null with a non-zero length, a status is outside
 * 0..3, or one entry's packed length reaches 2^32 (the kernels read 32-bit lengths). */
int bcosgpu_pack_state_entries(const bcosgpu_StateEntry* entries, size_t n, uint8_t* out, uint64_t cap,
                               uint64_t* off3, uint8_t* kind);
/* Bytes of d_work (4-byte aligned) for bcosgpu_state_root_dev over n entries. */
uint64_t bcosgpu_state_root_work_size(size_t n);
/* The state root of n packed entries (the layout above, in device memory; block_version as in the block header,
 * e.g. 0x03010000), stream-ordered: a fused hash-and-XOR kernel (no digest is written to memory) whose
 * workgroups leave 32-byte partials in d_work, the same over the entries of more than 1 KiB it set aside
 * (listed in d_work, so that long messages share waves), and a fold of the partials into d_root32.  d_work's
 * earlier contents do not matter.  n == 0 writes the zero hash.  n and every entry's packed length must be
 * below 2^32. */
int bcosgpu_state_root_dev(int hasher, uint32_t block_version, const uint8_t* d_data, const uint64_t* d_off3,
                           const uint8_t* d_kind, size_t n, void* d_work, uint64_t work_bytes, uint8_t* d_root32,
                           void* stream);
/* The same from host views: packed into pinned staging, one H2D copy, the kernels, a 32-byte copy back. */
int bcosgpu_state_root(int hasher, uint32_t block_version, const bcosgpu_StateEntry* entries, size_t n,
                       uint8_t* root32);

/* ---------------------------------------------------------------- storage cipher (DataEncryption over storage values) */
/* The third member of the reference's CryptoSuite, SymmetricEncryption (bcos-crypto/bcos-crypto/interfaces/crypto/
 * CryptoSuite.h:33-67), at its batch sites: with storage_security.enable=true RocksDBStorage runs every non-empty
 * value through DataEncryption::encrypt on the way to disk (asyncPrepare, bcos-storage/bcos-storage/
 * RocksDBStorage.cpp:348-353; setRows, :513-524) and through decrypt on the way back (asyncGetRow, :106-108;
 * asyncGetRows, :204-205).  DataEncryption (bcos-security/bcos-security/DataEncryption.cpp:143-165) calls
 * symmetricEncrypt / symmetricDecrypt(data, size, key, keySize), i.e. AESCrypto / SM4Crypto
 * (bcos-crypto/bcos-crypto/encrypt/AESCrypto.cpp:29-51, SM4Crypto.cpp:28-49) over wedpr's AES-256-CBC / SM4-CBC.
 *   key     the first min(key_len, K) bytes, zero-filled to K; K = 32 (AES-256), 16 (SM4)
 *           (bcos-utilities/bcos-utilities/FixedBytes.h:173-176, AESCrypto.cpp:34, SM4Crypto.cpp:33); a longer key is
 *           cut (bcos-crypto/test/unittests/EncryptionTest.cpp:73 passes 69 bytes)
 *   iv      iv != NULL: its first min(iv_len, 16) bytes, zero-filled to 16 (AESCrypto.cpp:37, SM4Crypto.cpp:36).
 *           iv == NULL: the default IV of the two-argument form DataEncryption uses (AESCrypto.h:41-51,
 *           SM4Crypto.h:41-50), the first 16 bytes of the raw key.  STATED DEVIATION: with a key shorter than 16
 *           bytes the reference reads past the end of the caller's buffer (the key "abcd" of EncryptionTest.cpp:38
 *           does); this build zero-fills instead.
 *   mode    CBC with PKCS#7 padding: len bytes become (len / 16 + 1) * 16, an empty value one block (the reference
 *           sizes its buffer len + 26 and shrinks it to what wedpr reports, AESCrypto.cpp:41-49).  The RocksDB sites
 *           skip empty values themselves (!value.empty()): that is the adapter's job (bcos_gpu.hpp), not this call's.
 *   decrypt fails per item, as a status byte, where the reference throws DecryptException (AESCrypto.cpp:69-72): a
 *           length that is zero or no multiple of 16, a last plaintext byte p outside 1..16, or last p bytes that are
 *           not all p.  It never fails the call.
 * Parity unpinned: mode and padding live in wedpr (Rust), which is not built here, and the reference's
 * only test is a round trip (EncryptionTest.cpp:35-92).  The ciphers are pinned by FIPS-197 C.3, SP 800-38A
 * F.2.5 / F.2.6 and GB/T 32907 A.1, CBC and the padding by OpenSSL's output (tests/golden/cipher.json). */
#define BCOSGPU_CIPHER_AES256 0
#define BCOSGPU_CIPHER_SM4 1
#define BCOSGPU_CBC_OK 0
#define BCOSGPU_CBC_E_LENGTH 1
#define BCOSGPU_CBC_E_PADDING 2
/* The ciphertext bytes of a value of len bytes: (len / 16 + 1) * 16. */
uint64_t bcosgpu_cbc_padded_size(uint64_t len);
/* Bytes of d_work (8-byte aligned) for bcosgpu_cbc_encrypt_batch_dev over n values. */
uint64_t bcosgpu_cbc_work_size(size_t n);
/* Encrypts n packed values (d_in, value i at d_in_off[i] .. d_in_off[i+1], any byte offsets) under one key,
 * stream-ordered.  key and iv are HOST pointers (iv == NULL: the default IV); the schedule is expanded on the host
 * and travels in the kernel arguments.  Writes d_out_off[n+1] (d_out_off[i] = 16 * the blocks of the values before
 * i, d_out_off[n] the total) and the ciphertexts at those offsets of d_out, which must be 16-byte aligned and hold
 * the sum of bcosgpu_cbc_padded_size over the values.  One lane runs one value; a value of more than 1 KiB is
 * listed in d_work and run by a second launch, so that long values share waves.  d_work's earlier contents do not
 * matter.  n and every value's length must be below 2^32.  n == 0 writes nothing. */
int bcosgpu_cbc_encrypt_batch_dev(int cipher, const uint8_t* key, size_t key_len, const uint8_t* iv, size_t iv_len,
                                  const uint8_t* d_in, const uint64_t* d_in_off, size_t n, uint8_t* d_out,
                                  uint64_t* d_out_off, void* d_work, uint64_t work_bytes, void* stream);
/* Decrypts n packed ciphertexts (d_in 16-byte aligned, every d_in_off a multiple of 16: the layout the call above
 * writes), stream-ordered, one lane per 16-byte block.  The plaintext of item i lands at d_out + d_in_off[i], padding
 * included; d_out_len[i] (uint32) is its length without the padding and d_status[i] (uint8) BCOSGPU_CBC_OK, or
 * d_out_len[i] = 0 with BCOSGPU_CBC_E_LENGTH (an empty item) or BCOSGPU_CBC_E_PADDING.  d_out must be 16-byte
 * aligned, as large as d_in and must not overlap it (a lane reads its neighbour's ciphertext block):
 * BCOSGPU_E_ARG when d_in == d_out. */
int bcosgpu_cbc_decrypt_batch_dev(int cipher, const uint8_t* key, size_t key_len, const uint8_t* iv, size_t iv_len,
                                  const uint8_t* d_in, const uint64_t* d_in_off, size_t n, uint8_t* d_out,
                                  uint32_t* d_out_len, uint8_t* d_status, void* stream);
/* The same from host views: the values are gathered into pinned staging, one H2D copy, the kernels, one copy back.
 * Encrypt: out (cap bytes) receives the ciphertexts back to back, out_off[n+1] their offsets (multiples of 16);
 * BCOSGPU_E_ARG if cap is below the sum of bcosgpu_cbc_padded_size over the values.
 * Decrypt: an item whose length is not a non-zero multiple of 16 gets BCOSGPU_CBC_E_LENGTH without reaching the
 * GPU; out receives the plaintexts back to back (nothing for a failed item), out_off[n+1] their offsets, status[n]
 * the BCOSGPU_CBC_* of each item; BCOSGPU_E_ARG if cap is below the sum of the well-formed items' lengths (always
 * enough: a plaintext is shorter than its ciphertext).
 * Both: BCOSGPU_E_ARG for an unknown cipher, a null pointer with a non-zero length, or n or a value of 2^32 or
 * more; n == 0 succeeds and writes nothing. */
int bcosgpu_cbc_encrypt_batch(int cipher, const uint8_t* key, size_t key_len, const uint8_t* iv, size_t iv_len,
                              const bcosgpu_Bytes* values, size_t n, uint8_t* out, uint64_t cap, uint64_t* out_off);
int bcosgpu_cbc_decrypt_batch(int cipher, const uint8_t* key, size_t key_len, const uint8_t* iv, size_t iv_len,
                              const bcosgpu_Bytes* values, size_t n, uint8_t* out, uint64_t cap, uint64_t* out_off,
                              uint8_t* status);

/* ---------------------------------------------------------------- block headers (hash, parent link, quorum) */
/* The check a syncing node runs on every downloaded block, for a run of consecutive headers in one call:
 *   the header hash    impl_calculate<Hasher>(bcostars::BlockHeader), bcos-tars-protocol/.../impl/TarsHashable.h:77-126
 *   the block check    BlockValidator::asyncCheckBlock, bcos-pbft/bcos-pbft/pbft/engine/BlockValidator.cpp:28-182
 *                      (caller: bcos-sync/bcos-sync/state/DownloadingQueue.cpp:407)
 *   the parent link    the ledger's header sync loop, bcos-ledger/src/libledger/LedgerImpl.h:290-312
 * Views of bcostars::ParentInfo / Signature / BlockHeader (bcos-tars-protocol/.../tars/Block.tars:6-35):
 * pointers into the caller's decoded header, nothing is copied until packing. */
typedef struct { int64_t block_number; const uint8_t* block_hash; size_t block_hash_len; } bcosgpu_ParentInfo;
typedef struct { int64_t sealer_index; const uint8_t* signature; size_t signature_len; } bcosgpu_HeaderSignature;
typedef struct {
    int32_t version;
    const bcosgpu_ParentInfo* parents;  size_t nparents;
    /* the three roots are hashed as whatever bytes the vectors hold, of any length (TarsHashable.h:98-100) */
    const uint8_t* txs_root;      size_t txs_root_len;
    const uint8_t* receipt_root;  size_t receipt_root_len;
    const uint8_t* state_root;    size_t state_root_len;
    int64_t block_number;
    const char* gas_used;         size_t gas_used_len;
    int64_t timestamp;
    int64_t sealer;
    const bcosgpu_Bytes* sealer_list;  size_t nsealer_list;
    const uint8_t* extra_data;    size_t extra_data_len;
    const int64_t* consensus_weights;  size_t nconsensus_weights;
    /* BlockHeader.dataHash: when non-empty it IS the header hash (TarsHashable.h:81-85) and the fields above
     * are not hashed -- unless BCOSGPU_HEADER_RECOMPUTE.  Lengths as for a receipt's dataHash: more than 32
     * bytes is BCOSGPU_E_ARG, a shorter one fills the leading bytes and the rest are zero. */
    const uint8_t* data_hash;     size_t data_hash_len;
    const bcosgpu_HeaderSignature* signatures;  size_t nsignatures;
    uint64_t tx_count; /* Block::transactionsSize(), for the short cut at BlockValidator.cpp:54-58 */
} bcosgpu_BlockHeaderData;
/* The consensus set the headers are checked against (PBFTConfig): n nodes, node i's 64-byte id (its public key,
 * X||Y) at node_ids64 + 64 i and its weight weights[i]; minRequiredQuorum(); committedProposal()->index(). */
typedef struct {
    const uint8_t* node_ids64;
    const uint64_t* weights;
    size_t n;
    uint64_t min_required_quorum;
    int64_t committed_index;
} bcosgpu_ConsensusSet;
/* flag: ignore every dataHash and hash the fields (a node that does not trust a peer's header) */
#define BCOSGPU_HEADER_RECOMPUTE 1
/* Total preimage bytes of n headers (0 for a header whose dataHash is used). */
uint64_t bcosgpu_header_preimage_size(const bcosgpu_BlockHeaderData* headers, size_t n, int flags);
/* Packs the header-hash preimages (TarsHashable.h:90-125: be32(version) || per parent (be64(blockNumber) ||
 * blockHash) || txsRoot || receiptRoot || stateRoot || be64(blockNumber) || gasUsed || be64(timestamp) ||
 * be64(sealer) || every sealerList entry || extraData || be64 of every consensus weight) back to back into out
 * (cap bytes) and writes offsets[n+1]; a header whose dataHash is used gets an empty preimage.  Host only,
 * multithreaded for large batches.  BCOSGPU_E_ARG if cap is too small, a pointer is null with a non-zero
 * length or count, or a dataHash is longer than 32 bytes. */
int bcosgpu_pack_header_preimages(const bcosgpu_BlockHeaderData* headers, size_t n, int flags, uint8_t* out,
                                  uint64_t cap, uint64_t* offsets);
/* Verdicts.  check[i] -- header i is accepted iff the code is < 16; precedence is the reference's order of
 * returns (BlockValidator.cpp:35-69):
 *    0 passed every check            1 genesis, nothing checked (:35-39)     2 no transactions, nothing checked (:54-58)
 *   16 number <= committed index (:49-53)                17 the sealer is not a consensus node (:85-93)
 *   18 sealer list or weight list differs from the consensus set (:98-137)
 *   19 a signature row failed (:149-170)                 20 weight below the quorum (:173-180)
 * Signature rows follow the reference even where that surprises: a row whose index names no consensus node
 * (negative included) fails (getConsensusNodeByIndex, ConsensusConfig.cpp:150-158); ONE failed row fails the
 * block even if the remaining weight reaches the quorum (19 before 20); an index that appears twice is counted
 * twice (the reference sums per list entry and never deduplicates).
 * link[i] -- 1 linked: parentInfo[0].blockNumber is the previous header's number and its hash the previous
 * header's hash (LedgerImpl.h:302-306); 0 not linked (also: parentInfo empty, or its hash not 32 bytes long);
 * 2 not checked: block number 0 (:290), or the first header with no previous hash given. */
#define BCOSGPU_HEADER_OK 0
#define BCOSGPU_HEADER_GENESIS 1
#define BCOSGPU_HEADER_NO_TXS 2
#define BCOSGPU_HEADER_E_COMMITTED 16
#define BCOSGPU_HEADER_E_SEALER 17
#define BCOSGPU_HEADER_E_SEALER_LIST 18
#define BCOSGPU_HEADER_E_SIGNATURE 19
#define BCOSGPU_HEADER_E_QUORUM 20
#define BCOSGPU_LINK_BROKEN 0
#define BCOSGPU_LINK_OK 1
#define BCOSGPU_LINK_UNCHECKED 2
/* Bytes of d_work (4-byte aligned) for bcosgpu_headers_check_dev over n headers with `rows` signature rows. */
uint64_t bcosgpu_headers_check_work_size(size_t n, size_t rows);
/* The device path, stream-ordered, three phases on the one stream: header_hash_kernel (one header per lane:
 * the digest of preimage i = d_pre[d_pre_off[i] .. d_pre_off[i+1]), or d_given32 + 32 i where d_given_mask[i]
 * is set, to d_hash32 and to each of the header's rows in d_work), the existing known-key verify kernels over
 * the rows (the registered-key kernel when d_row_slot is given, the generic one when d_row_pub64 is: exactly
 * one of the two), and header_verdict_kernel (one header per lane: folds its rows -- all ok, and the u64 sum of
 * their weights against `quorum` -- merges d_pre_status and writes d_check and d_link).  The hasher follows the
 * suite (Keccak-256 with secp256k1, SM3 with SM2).  All pointers are device pointers; hash arrays and d_work
 * are 4-byte aligned, 64-bit arrays 8-byte aligned:
 *   d_given32 [32 n], d_given_mask [n]   both nullable: the hash of a header that came with a dataHash
 *   d_pre_status [n]                     the host's early verdict (a code above; 0 = go on to the rows)
 *   d_number [n]                         the block numbers
 *   d_parent_number [n], d_parent_hash32 [32 n], d_parent_ok [n]   parentInfo[0]; parent_ok = 0 when parentInfo
 *                                        is empty or its hash is not 32 bytes long
 *   d_prev_hash32 (nullable), prev_number   the header before the first one
 *   d_sig_off [n + 1]                    CSR: header i's rows are [d_sig_off[i], d_sig_off[i+1]); d_sig_off[n] = rows
 *   d_sig [64 rows]                      r || s of each row;  d_row_weight [rows] (u64)
 *   d_row_slot [rows] (ids of bcosgpu_register_keys; a negative or stale id fails its row) or d_row_pub64 [64 rows]
 * Outputs d_hash32 [32 n], d_check [n], d_link [n], d_sig_ok [rows] (nullable).  d_work's earlier contents
 * do not matter.  n and every preimage length must be below 2^32. */
int bcosgpu_headers_check_dev(int suite, const uint8_t* d_pre, const uint64_t* d_pre_off, const uint8_t* d_given32,
                              const uint8_t* d_given_mask, const uint8_t* d_pre_status, const int64_t* d_number,
                              const int64_t* d_parent_number, const uint8_t* d_parent_hash32,
                              const uint8_t* d_parent_ok, const uint8_t* d_prev_hash32, int64_t prev_number,
                              const uint64_t* d_sig_off, const uint8_t* d_sig, const uint64_t* d_row_weight,
                              const int32_t* d_row_slot, const uint8_t* d_row_pub64, uint64_t quorum, size_t n,
                              size_t rows, uint8_t* d_hash32, uint8_t* d_check, uint8_t* d_link, uint8_t* d_sig_ok,
                              void* d_work, uint64_t work_bytes, void* stream);
/* The same from host views, on the calling thread's device: the host-side parts of asyncCheckBlock per header
 * (genesis, committed, tx_count == 0, sealer in range, sealer list and weight list equal to the consensus set),
 * each signature's index mapped to the consensus key and weight, the consensus keys registered (a cached key is
 * a lookup; when the cache cannot hold them all the rows carry the keys instead), everything packed into pinned
 * staging, one H2D copy, the three phases, one D2H copy.  A header with a non-zero early verdict contributes no
 * rows; it is still hashed and linked.  A signature shorter than 64 bytes, or one whose index names no
 * consensus node, fails its row without a key.  hash32 [32 n], check [n], link [n]; sig_ok (nullable) has one
 * entry per signature of every header, headers back to back: 1 verified, 0 failed, 2 not checked (the header
 * had an early verdict).  Every row is verified, also those after a failed one.  n == 0 is a no-op. */
int bcosgpu_headers_check(int suite, const bcosgpu_BlockHeaderData* headers, size_t n,
                          const bcosgpu_ConsensusSet* consensus, const uint8_t* prev_hash32_or_null,
                          int64_t prev_number, int flags, uint8_t* hash32, uint8_t* check, uint8_t* link,
                          uint8_t* sig_ok_or_null);

/* ---------------------------------------------------------------- PBFT messages (a drained queue in one call) */
/* Every signature of every message a PBFT worker popped from its queue, in one call, with the verdicts the
 * handlers then read instead of verifying one signature at a time (PBFTEngine::executeWorker,
 * bcos-pbft/bcos-pbft/pbft/engine/PBFTEngine.cpp:555-601):
 *   the message signature     checkSignature, PBFTEngine.cpp:732-750
 *   the proposal signature    checkProposalSignature, :752-771 (also called at :971 and :1417)
 *   a prepared proposal       PBFTCacheProcessor::checkPrecommitWeight, pbft/cache/PBFTCacheProcessor.cpp:795-821
 *                             (from isValidViewChangeMsg, PBFTEngine.cpp:1161-1178)
 *   a NewView                 isValidNewViewMsg, PBFTEngine.cpp:1238-1263: every view change valid, and their
 *                             nodes' weight against minRequiredQuorum()
 * What stays on the host is everything stateful: the views and the committed index (PBFTEngine.cpp:1120-1160,
 * :1232, PBFTCacheProcessor.cpp:763-770) and the second look at the cached precommit (:776-792).  That look
 * never rescues a failed proposal -- checkPrecommitMsg returns the first result either way -- it only decides
 * whether the local cache entry is erased; a handler that finds prepared_check != 0 for a proposal it has
 * cached still runs it, as before.
 * Views, nothing copied until packing: */
typedef struct {                      /* a prepared (precommitted) proposal and its proof, PBFT.proto PBFTRawProposal */
    const uint8_t* hash; size_t hash_len;                    /* PBFTProposal::hash(); <= 32 bytes, zero-filled */
    const bcosgpu_HeaderSignature* proofs; size_t nproofs;   /* nodeList[i], signatureList[i] */
} bcosgpu_PrecommitProof;
#define BCOSGPU_PBFT_CHECK_MSG_SIG 1u
#define BCOSGPU_PBFT_CHECK_PROPOSAL_SIG 2u
#define BCOSGPU_PBFT_CHECK_PREPARED 4u
typedef struct {
    int64_t generated_from;
    /* what the signature is over: hashFieldsData (PBFTMessage.cpp:92-98) or the codec payLoad
     * (PBFTCodec.cpp:94-103).  Hashed on the device by ONE lane: meant for hashFieldsData, tens of bytes.  The
     * sender of a payload-signed packet (ViewChange, NewView: up to hundreds of kilobytes) passes the hash the
     * codec already computed as signature_hash instead. */
    const uint8_t* signed_data; size_t signed_data_len;
    /* non-empty: it IS signatureDataHash and signed_data is not hashed (a view change inside a NewView carries
     * it, BaseMessage field 7); <= 32 bytes, zero-filled, as a header's dataHash */
    const uint8_t* signature_hash; size_t signature_hash_len;
    const uint8_t* signature; size_t signature_len;
    const uint8_t* proposal_hash; size_t proposal_hash_len;   /* consensusProposal()->hash(); <= 32 bytes */
    const uint8_t* proposal_signature; size_t proposal_signature_len;
    const bcosgpu_PrecommitProof* prepared; size_t nprepared;
    uint32_t checks;                  /* BCOSGPU_PBFT_CHECK_MSG_SIG | _PROPOSAL_SIG | _PREPARED */
} bcosgpu_PBFTMessageData;
typedef struct { size_t parent, first, count; } bcosgpu_PBFTGroup;  /* a NewView at `parent`, its view changes at [first, first+count) */
/* msg_flags[i] is a bit set; message i is accepted iff it is 0.  The reference only ever returns false, so the
 * bits have no precedence:
 *    1  generated_from names no consensus node, negative included (getConsensusNodeByIndex,
 *       ConsensusConfig.cpp:150-158).  Set whatever `checks` asks for; a requested signature of such a message
 *       has no key and fails too (2, 4).
 *    2  the message signature fails (PBFTEngine.cpp:743-748)
 *    4  the proposal signature is absent (length 0) or fails (:755-758, :769-770)
 *    8  a prepared proposal fails (:1171-1177): its prepared_check is 1 or 2
 *   16  a view change of the group fails, i.e. its own bits 1-8 are not all 0 (:1243-1248)
 *   32  the group's weight is below min_required_quorum (:1249-1262): the sum, per view change, of the weight
 *       of its generated_from node; a view change whose node is unknown adds nothing
 * prepared_check[] has one entry per prepared proposal, messages back to back:
 *    0 passed   1 a proof names no node or fails (PBFTCacheProcessor.cpp:805-816)   2 weight below the quorum
 *    (:820)     3 not checked (the message's checks lack BCOSGPU_PBFT_CHECK_PREPARED)
 * The rows follow the header check's rules, for the same reason: ONE failed proof fails the proposal whatever
 * the remaining weight (1 before 2); a node index listed twice counts twice; a signature shorter than 64
 * bytes fails its row without a key; every row is verified, also those after a failed one. */
#define BCOSGPU_PBFT_E_NODE 1u
#define BCOSGPU_PBFT_E_MSG_SIG 2u
#define BCOSGPU_PBFT_E_PROPOSAL_SIG 4u
#define BCOSGPU_PBFT_E_PREPARED 8u
#define BCOSGPU_PBFT_E_VIEWCHANGE 16u
#define BCOSGPU_PBFT_E_GROUP_QUORUM 32u
#define BCOSGPU_PREPARED_OK 0
#define BCOSGPU_PREPARED_E_PROOF 1
#define BCOSGPU_PREPARED_E_QUORUM 2
#define BCOSGPU_PREPARED_UNCHECKED 3
/* Bytes of d_work (4-byte aligned) for bcosgpu_pbft_check_dev over n messages with `rows` signature rows. */
uint64_t bcosgpu_pbft_check_work_size(size_t n, size_t rows);
/* The device path, stream-ordered, four phases on the one stream: pbft_hash_kernel (one message per lane: the
 * digest of d_data[d_data_off[i] .. d_data_off[i+1]), or d_given32 + 32 i where d_given_mask[i] is set, to
 * d_msg_hash32 and to the message's signature row of d_row_hash32), the existing known-key verify kernels over
 * all rows (the registered-key kernel when d_row_slot is given, the generic one when d_row_pub64 is: exactly
 * one of the two), pbft_verdict_kernel (one message per lane: its rows, its prepared proposals -- all proofs
 * ok, and the wrapping u64 sum of their weights against `quorum` -- into bits 1-8 and d_prepared_check) and,
 * when ngroups > 0, pbft_group_kernel (one group per lane: bits 16 and 32 into the parent).  The hasher
 * follows the suite.  All pointers are device pointers; hash arrays, d_msg_flags and d_work are 4-byte aligned,
 * 64-bit arrays 8-byte aligned:
 *   d_given32 [32 n], d_given_mask [n]   both nullable: the given signatureDataHash of a message
 *   d_pre_flags [n]                      the host's bits: BCOSGPU_PBFT_E_NODE where generated_from names no node
 *   d_msg_weight [n] (u64)               the weight of the generated_from node, 0 where unknown (the group sum)
 *   d_checks [n]                         BCOSGPU_PBFT_CHECK_* of each message
 *   d_msg_row, d_prop_row [n] (i64)      the row of the message / proposal signature; a requested check whose
 *                                        row is not in [0, rows) fails (an absent proposal signature: -1)
 *   d_prep_off [n + 1]                   CSR: message i's prepared proposals are [d_prep_off[i], d_prep_off[i+1])
 *   d_prep_row_off [nprep + 1]           CSR: prepared proposal p's proof rows are [d_prep_row_off[p],
 *                                        d_prep_row_off[p+1]), so the proof rows lie back to back in the order of
 *                                        the prepared proposals; nprep = d_prep_off[n]; a message without
 *                                        BCOSGPU_PBFT_CHECK_PREPARED gets 3 and its rows are not read
 *   d_row_hash32 [32 rows]               IN/OUT: the hashes of the proposal and proof rows, given; the message
 *                                        rows are written by the call
 *   d_sig [64 rows]                      r || s of each row;  d_row_weight [rows] (u64)
 *   d_row_slot [rows] (ids of bcosgpu_register_keys; a negative or stale id fails its row) or d_row_pub64 [64 rows]
 *   d_groups [3 ngroups] (u64)           parent, first, count of each group; nullable when ngroups == 0.  A
 *                                        parent >= n is skipped, a range is clipped to n
 * Outputs d_msg_hash32 [32 n], d_msg_flags [n] (u32), d_prepared_check [nprep], d_sig_ok [rows] (nullable).
 * d_work's earlier contents do not matter.  n, rows, nprep and every data length must be below 2^32. */
int bcosgpu_pbft_check_dev(int suite, const uint8_t* d_data, const uint64_t* d_data_off, const uint8_t* d_given32,
                           const uint8_t* d_given_mask, const uint8_t* d_pre_flags, const uint64_t* d_msg_weight,
                           const uint8_t* d_checks, const int64_t* d_msg_row, const int64_t* d_prop_row,
                           const uint64_t* d_prep_off, const uint64_t* d_prep_row_off, size_t nprep,
                           uint8_t* d_row_hash32, const uint8_t* d_sig, const uint64_t* d_row_weight,
                           const int32_t* d_row_slot, const uint8_t* d_row_pub64, const uint64_t* d_groups,
                           size_t ngroups, uint64_t quorum, size_t n, size_t rows, uint8_t* d_msg_hash32,
                           uint32_t* d_msg_flags, uint8_t* d_prepared_check, uint8_t* d_sig_ok, void* d_work,
                           uint64_t work_bytes, void* stream);
/* The same from host views, on the calling thread's device: generated_from and every proof index mapped to the
 * consensus key and weight, the consensus keys registered (a cached key is a lookup; when the cache cannot hold
 * them all the rows carry the keys instead), everything packed into pinned staging, one H2D copy, the phases,
 * one D2H copy.  Each requested signature is one row.  consensus->committed_index is not read.  `flags` is
 * reserved (0).  msg_hash32 [32 n], msg_flags [n]; prepared_check (nullable) one entry per prepared proposal;
 * sig_ok (nullable) has, per message, 2 + (its proofs) entries -- the message signature, the proposal
 * signature, the proofs of every prepared proposal in order: 1 verified, 0 failed, 2 not requested.
 * BCOSGPU_E_ARG for a null field with a length, a hash longer than 32 bytes, signed_data of 2^32 - 1 bytes or
 * more, or a group that names messages outside [0, n).  n == 0 is a no-op. */
int bcosgpu_pbft_check(int suite, const bcosgpu_PBFTMessageData* msgs, size_t n, const bcosgpu_PBFTGroup* groups,
                       size_t ngroups, const bcosgpu_ConsensusSet* consensus, int flags, uint8_t* msg_hash32,
                       uint32_t* msg_flags, uint8_t* prepared_check_or_null, uint8_t* sig_ok_or_null);

/* ---------------------------------------------------------------- single calls on an explicit device */
/* One signature per call, for the reference's per-transaction call sites: TxPool's submitter threads
 * (TxPool.h:48-49) -> TxValidator::verify (TxValidator.cpp:56) -> Transaction::verify (Transaction.h:68-82)
 * -> SignatureCrypto::recover.  Concurrent calls on one device are coalesced into shared launches (one
 * H2D copy, one kernel, one D2H copy per batch; up to 4 batches in flight per device).  `device` is
 * initialised on first use; the calling thread's current device is left unchanged.
 * Return 1 = valid, 0 = invalid signature (the reference throws InvalidSignature / returns false),
 * < 0 = engine error (BCOSGPU_E_*, message in bcosgpu_last_error()). */
/* Secp256k1Crypto::recover (Secp256k1Crypto.cpp:79-93): sig = r||s||v, sig_len must be 65;
 * pub64 = X||Y (zero when invalid). */
int bcosgpu_secp256k1_recover(int device, const uint8_t* hash32, const uint8_t* sig, size_t sig_len, uint8_t* pub64);
/* secp256k1Verify -> wedpr_secp256k1_verify (Secp256k1Crypto.cpp:51-63): libsecp256k1 verify (low-S);
 * only sig[0..64) = r||s is read; sig_len < 64 is invalid. */
int bcosgpu_secp256k1_verify(int device, const uint8_t* pub64, const uint8_t* hash32, const uint8_t* sig,
                             size_t sig_len);
/* SM2Crypto::verify (SM2Crypto.cpp:66-79) -> fast_sm2_verify: sig64 = r||s, with the given key. */
int bcosgpu_sm2_verify(int device, const uint8_t* pub64, const uint8_t* hash32, const uint8_t* sig64);
/* Where the coalesced calls' time goes on `device` (diagnostics; counters since start or the last reset):
 * out10 = {batches, calls, signatures, queue ns (sum over calls: enqueued -> taken into a batch), leader ns
 * (sum over batches: staging and key lookup before the launch), GPU ns (launch -> results synchronised),
 * scatter ns (results copied to the callers), wake ns (sum over targeted wake-ups: notify -> running),
 * wake-ups, lock ns (sum over calls: waiting for the queue mutex)}; reset != 0 zeroes them. */
int bcosgpu_coalesce_stats(int device, uint64_t* out10, int reset);

/* ---------------------------------------------------------------- device sets (one process, several GPUs) */
/* A FISCO node is ONE process with one CryptoSuite (libinitializer/ProtocolInitializer.cpp:102-124) whose
 * batch sites run in-process (TransactionSync.cpp:516-548, BlockImpl.h:111-154); these entry points let
 * that process use all the GPUs of its node (SURVEY 8(b) "one context per GPU", 8(e)).  `devices` lists
 * ndev device indices (1 <= ndev <= 64); a batch is split by index into ndev contiguous shards, shard k
 * running on devices[k] on its own stream with its own buffers -- an index may repeat (two shards on one
 * GPU, distinct streams).  Results are identical to the single-device calls for every n.  Host pointers;
 * the calling thread's current device is left unchanged.  Test status: every entry point is checked
 * against the oracle on repeated-device lists ({0, 0}, {0, 0, 0}), including the cross-device peer-copy
 * gather (forced by BCOSGPU_MULTI_PEER=1); lists of distinct physical GPUs have not run on hardware yet.
 * Initialise every device of the set (tables, streams); idempotent. */
int bcosgpu_init_devices(const int* devices, int ndev);
/* The signature batches above, sharded over the set (each shard a coalesced job on its device). */
int bcosgpu_secp256k1_recover_batch_multi(const int* devices, int ndev, const uint8_t* hash32, const uint8_t* sig65,
                                          size_t n, uint8_t* pub64, uint8_t* addr20, uint8_t* ok);
int bcosgpu_sm2_verify_batch_multi(const int* devices, int ndev, const uint8_t* hash32, const uint8_t* sig128,
                                   size_t n, uint8_t* addr20, uint8_t* ok);
int bcosgpu_verify_batch_multi(const int* devices, int ndev, int suite, const uint8_t* pub64, const uint8_t* hash32,
                               const uint8_t* sig, size_t sig_stride, size_t n, uint8_t* ok);
/* bcosgpu_tx_verify_batch over the set: TransactionSync::importDownloadedTxs' verify loop
 * (TransactionSync.cpp:516-548) for a whole download on every GPU of the node. */
int bcosgpu_tx_verify_batch_multi(const int* devices, int ndev, int suite, const uint8_t* pre, const uint64_t* pre_off,
                                  const uint8_t* sig, const uint64_t* sig_off, size_t n, uint8_t* txhash32,
                                  uint8_t* sender20, uint8_t* status);
/* Block check in one call: bcosgpu_tx_verify_batch_multi plus the block's tx root
 * (BlockImpl::calculateTransactionRoot, BlockImpl.h:111-154: Merkle<H, width> over the tx hashes, H =
 * Keccak256 / SM3 by suite; zero hash for an empty block).  Shard starts are multiples of width^L, each
 * GPU reduces its shard's hashes to the reference tree's level-L nodes, the frontiers (a few KB) are
 * gathered on devices[0] with peer copies over xGMI, and the top levels run there. */
int bcosgpu_block_verify_multi(const int* devices, int ndev, int suite, const uint8_t* pre, const uint64_t* pre_off,
                               const uint8_t* sig, const uint64_t* sig_off, size_t n, int width, uint8_t* txhash32,
                               uint8_t* sender20, uint8_t* status, uint8_t* root32);
/* Many blocks in one call (a sync catch-up / replay of downloaded blocks, configs[4]): block b's txs are
 * [block_off[b], block_off[b+1]) (block_off[0] = 0, nblocks + 1 entries), every tx verified as
 * bcosgpu_tx_verify_batch does and roots32 + 32 b = block b's tx root (zero hash for an empty block).
 * Whole blocks go to the devices in contiguous ranges balanced by tx count; no exchange. */
int bcosgpu_blocks_verify_multi(const int* devices, int ndev, int suite, const uint8_t* pre, const uint64_t* pre_off,
                                const uint8_t* sig, const uint64_t* sig_off, const uint64_t* block_off, size_t nblocks,
                                int width, uint8_t* txhash32, uint8_t* sender20, uint8_t* status, uint8_t* roots32);
/* Merkle<H, width>::generateMerkle's root (Merkle.h:170-208) over the set, by the same frontier scheme;
 * n == 0 is BCOSGPU_E_EMPTY, n == 1 returns the leaf. */
int bcosgpu_merkle_root_multi(const int* devices, int ndev, int hasher, int width, const uint8_t* leaves32, size_t n,
                              uint8_t* root32);

/* ---------------------------------------------------------------- wedpr-ABI single-call shims */
/* Same layout as wedpr-crypto's CInputBuffer / COutputBuffer; on the calling thread's current device.
 * Return 0 (WEDPR_SUCCESS), -1 (WEDPR_ERROR: invalid input or signature) or
 * BCOSGPU_WEDPR_ENGINE_ERROR when the engine itself failed (no gfx950 device, HIP error; message in
 * bcosgpu_last_error()) -- a reference caller that only tests "!= WEDPR_SUCCESS" reads that as an
 * invalid signature, so the SignatureCrypto adapters (bcos_gpu_crypto.hpp) check for it and throw
 * SignException instead.
 * A reference translation unit that already has wedpr's types (<wedpr-crypto/WedprCrypto.h>) includes
 * bcos_gpu_wedpr.h instead, which declares these two symbols over CInputBuffer / COutputBuffer so they
 * bind to SM2Crypto::m_verifier (SM2Crypto.h:64-65) and to wedpr's call sites unchanged. */
#define BCOSGPU_WEDPR_ENGINE_ERROR (-2)
typedef struct { const char* data; uintptr_t len; } bcosgpu_CInputBuffer;
typedef struct { char* data; uintptr_t len; } bcosgpu_COutputBuffer;
#ifndef BCOSGPU_WEDPR_TYPES
/* wedpr_secp256k1_recover_public_key (Secp256k1Crypto.cpp:79-93) */
int8_t bcosgpu_wedpr_secp256k1_recover_public_key(const bcosgpu_CInputBuffer* hash,
                                                   const bcosgpu_CInputBuffer* sig,
                                                   bcosgpu_COutputBuffer* pub);
/* fast_sm2_verify / wedpr_sm2_verify (fast_sm2.cpp:139-227): sig = r||s (64 B), pub = 64 B */
int8_t bcosgpu_wedpr_sm2_verify(const bcosgpu_CInputBuffer* pub, const bcosgpu_CInputBuffer* hash,
                                 const bcosgpu_CInputBuffer* sig);
/* wedpr_secp256k1_verify (Secp256k1Crypto.cpp:51-63): libsecp256k1 verify semantics (low-S) */
int8_t bcosgpu_wedpr_secp256k1_verify(const bcosgpu_CInputBuffer* pub, const bcosgpu_CInputBuffer* hash,
                                      const bcosgpu_CInputBuffer* sig);
#endif

#ifdef __cplusplus
}
#endif
#endif
