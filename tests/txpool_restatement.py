"""The reference's transaction admission restated in plain Python: three sets and a dict of block lists, one
transaction after another.  It is the yardstick for a GPU admission call; the closed form such
kernels would use is NOT used here -- each accepted transaction's keys enter the sets before the next one is
judged, literally (tests/test_txpool_closed_form.py checks the closed form against this).

Decode: oracle/tars.py.  Hash, recover / verify, sender: the CPU oracle.  A nonce is u256(string) as
TransactionImpl::nonce() returns it (bcos-tars-protocol/.../protocol/TransactionImpl.cpp:62-68); only canonical
strings are restated (empty, or 1..78 digits without a leading 0 unless "0", value < 2^256): every other string
gets the library's own status 4 and takes no further part.
"""
import numpy as np

from oracle import tars as otars

OK, MALFORMED, NONCE_FOR_HOST = 0, 2, 4
NONCE_CHECK_FAIL, BLOCK_LIMIT_CHECK_FAIL, ALREADY_IN_TXPOOL = 10000, 10001, 10004
INVALID_CHAIN_ID, INVALID_GROUP_ID, INVALID_SIGNATURE = 10006, 10007, 10008
FULL, PROPOSAL = 0, 1
ZERO32, ZERO20 = bytes(32), bytes(20)


def canonical_nonce(s: bytes):
    """The value of a canonical nonce string, or None."""
    if s == b"":
        return 0
    if len(s) > 78 or not all(0x30 <= c <= 0x39 for c in s) or (len(s) > 1 and s[0] == 0x30):
        return None
    v = int(s)
    return v if v < 2 ** 256 else None


class Tx:
    """One decoded transaction with what Transaction::verify yields (hash, sender, signature verdict)."""

    def __init__(self, fields, txhash, sender, sig_ok):
        self.f, self.hash, self.sender, self.sig_ok = fields, txhash, sender, sig_ok
        self.nonce = None if fields is None else canonical_nonce(fields["nonce"])


def decode_batch(suite, encoded):
    """TransactionFactoryImpl::createTransaction(txData, checkSig = true, checkHash = false)
    (TransactionFactoryImpl.h:46-85) per transaction, over the oracle."""
    if not encoded:
        return []
    hs, ss, st = otars.create_transactions(suite, encoded, check_sig=True, check_hash=False)
    out = []
    for e, h, s, code in zip(encoded, hs, ss, st):
        if code == 2:
            out.append(Tx(None, ZERO32, ZERO20, False))
        else:
            out.append(Tx(otars.decode_transaction(e), h, s, code == 0))
    return out


class Pool:
    def __init__(self, suite, chain_id, group_id, block_limit_range, block_number=0):
        self.suite, self.chain, self.group = suite, bytes(chain_id), bytes(group_id)
        self.range, self.number = block_limit_range, block_number
        self.hashes, self.nonces, self.ledger = set(), set(), set()  # m_txsTable keys, m_nonces of both checkers
        self.blocks = {}  # LedgerNonceChecker::m_blockNonceCache

    # -- TxPoolNonceChecker::checkNonce (TxPoolNonceChecker.cpp:34-49)
    @staticmethod
    def _check_nonce(nonces, nonce):
        return NONCE_CHECK_FAIL if nonce in nonces else OK

    # -- LedgerNonceChecker::checkBlockLimit (LedgerNonceChecker.cpp:48-61)
    def _check_block_limit(self, tx):
        limit = tx.f["block_limit"]
        if self.number >= limit or self.number + self.range < limit:
            return BLOCK_LIMIT_CHECK_FAIL
        return OK

    # -- TxValidator::verify (TxValidator.cpp:27-69) after the library's own nonce gate
    def _verify(self, tx):
        if tx.f["group_id"] != self.group:
            return INVALID_GROUP_ID
        if tx.f["chain_id"] != self.chain:
            return INVALID_CHAIN_ID
        if tx.nonce is None:
            return NONCE_FOR_HOST  # (the library's: the reference would call lexical_cast here)
        st = self._check_nonce(self.nonces, tx.nonce)  # m_txPoolNonceChecker->checkNonce(_tx, false)
        if st:
            return st
        st = self._check_nonce(self.ledger, tx.nonce)  # submittedToChain: LedgerNonceChecker::checkNonce :36-46
        if st:
            return st
        st = self._check_block_limit(tx)
        if st:
            return st
        if not tx.sig_ok:
            return INVALID_SIGNATURE
        self.nonces.add(tx.nonce)  # m_txPoolNonceChecker->insert(_tx->nonce())
        return OK

    # -- MemoryStorage::verifyAndSubmitTransaction (MemoryStorage.cpp:223-273; txpoolStorageCheck is the lookup)
    def _verify_and_submit(self, tx):
        if tx.f is None:
            return MALFORMED
        if tx.hash in self.hashes:
            return ALREADY_IN_TXPOOL
        st = self._verify(tx)
        if st == OK:
            self.hashes.add(tx.hash)  # insert
        return st

    # -- MemoryStorage::enforceSubmitTransaction (MemoryStorage.cpp:147-221) after the proposal's signature checks
    def _enforce_submit(self, tx):
        if tx.f is None:
            return MALFORMED
        if tx.nonce is None:
            return NONCE_FOR_HOST
        if self._check_nonce(self.ledger, tx.nonce):  # submittedToChain; only NonceCheckFail is acted on
            return NONCE_CHECK_FAIL
        if not tx.sig_ok:  # importDownloadedTxs verified the signatures before it got here
            return INVALID_SIGNATURE
        self.hashes.add(tx.hash)  # insertWithoutLock unless the table has it
        return OK

    def admit(self, encoded, mode=FULL):
        """batchImportTxs (FULL) / importDownloadedTxs with a verified proposal (PROPOSAL), in index order.
        Returns (txhash[n,32], sender[n,20], nonce[n,32], status[n]) as the library lays them out."""
        txs = decode_batch(self.suite, encoded)
        n = len(txs)
        txhash = np.zeros((n, 32), dtype=np.uint8)
        sender = np.zeros((n, 20), dtype=np.uint8)
        nonce = np.zeros((n, 32), dtype=np.uint8)
        status = np.zeros(n, dtype=np.uint32)
        for j, tx in enumerate(txs):
            st = self._verify_and_submit(tx) if mode == FULL else self._enforce_submit(tx)
            status[j] = st
            txhash[j] = np.frombuffer(tx.hash, dtype=np.uint8)
            if tx.nonce is not None:
                nonce[j] = np.frombuffer(tx.nonce.to_bytes(32, "big"), dtype=np.uint8)
            if st == OK:
                sender[j] = np.frombuffer(tx.sender, dtype=np.uint8)
        return txhash, sender, nonce, status

    # -- MemoryStorage::batchRemove (:435-498) + LedgerNonceChecker::batchInsert (:64-99)
    def block_committed(self, number, txhashes, nonces):
        for h in txhashes:
            self.hashes.discard(bytes(h))
        if self.number < number:
            self.number = number
        to_remove = number - self.range if number > self.range else -1
        for v in nonces:
            self.ledger.add(v)  # TxPoolNonceChecker::batchInsert on the ledger checker
        for v in nonces:
            self.nonces.discard(v)  # txPoolNonceChecker()->batchRemove
        if number not in self.blocks:
            self.blocks[number] = list(nonces)
        if to_remove == -1 or to_remove not in self.blocks:
            return
        for v in self.blocks.pop(to_remove):
            self.ledger.discard(v)

    # -- MemoryStorage::removeInvalidTxs
    def remove(self, txhashes, nonces):
        for h in txhashes:
            self.hashes.discard(bytes(h))
        for v in nonces:
            self.nonces.discard(v)

    # -- LedgerNonceChecker::initNonceCache (:26-34)
    def load_ledger_nonces(self, blocks):
        for number, nonces in blocks.items():
            self.blocks[number] = list(nonces)
            for v in nonces:
                self.ledger.add(v)
