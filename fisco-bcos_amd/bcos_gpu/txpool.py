"""Transaction admission with the pool's own state on the GPU (bcosgpu_txpool_*).

  MemoryStorage::verifyAndSubmitTransaction  bcos-txpool/bcos-txpool/txpool/storage/MemoryStorage.cpp:223-273
  TxValidator::verify                        bcos-txpool/bcos-txpool/txpool/validator/TxValidator.cpp:27-69
  TxPoolNonceChecker / LedgerNonceChecker    .../validator/TxPoolNonceChecker.cpp:34-49, LedgerNonceChecker.cpp:26-99
  MemoryStorage::enforceSubmitTransaction    MemoryStorage.cpp:147-221
  MemoryStorage::batchRemove                 MemoryStorage.cpp:435-498

`Pool` keeps the pool's tx hashes, its nonces and the ledger's nonces as sorted key sets in HBM and has the
method names of the plain-Python restatement the tests compare it with (tests/txpool_restatement.py).  A nonce is
an int below 2^256 here and a 32-byte big-endian key in the library.
"""
import ctypes

import numpy as np

from ._lib import check, lib
from .crypto import _ptr, pack_messages

FULL, PROPOSAL = 0, 1
HASHES, NONCES, LEDGER = 0, 1, 2
OK, MALFORMED, NONCE_FOR_HOST = 0, 2, 4
NONCE_CHECK_FAIL, BLOCK_LIMIT_CHECK_FAIL, ALREADY_IN_TXPOOL = 10000, 10001, 10004
INVALID_CHAIN_ID, INVALID_GROUP_ID, INVALID_SIGNATURE = 10006, 10007, 10008
_INFO = ("hashes", "nonces", "ledger", "hashes_capacity", "nonces_capacity", "ledger_capacity", "block_number",
         "blocks", "error_word")


def _keys(values):
    """uint8[n, 32] from 32-byte strings, uint8 rows or ints (nonces)."""
    if isinstance(values, np.ndarray):
        return np.ascontiguousarray(values, dtype=np.uint8).reshape(-1, 32)
    rows = [v.to_bytes(32, "big") if isinstance(v, int) else bytes(v) for v in values]
    assert all(len(r) == 32 for r in rows), "keys are 32 bytes"
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, 32).copy()


class Pool:
    def __init__(self, suite, chain_id, group_id, block_limit_range, block_number=0, initial_capacity=0, device=0):
        self.handle = None
        chain, group = bytes(chain_id), bytes(group_id)
        h = ctypes.c_void_p()
        check(lib().bcosgpu_txpool_create(device, getattr(suite, "suite", suite), chain, len(chain), group, len(group),
                                          block_limit_range, block_number, initial_capacity, ctypes.byref(h)))
        self.handle = h

    def close(self):
        if self.handle is not None:
            lib().bcosgpu_txpool_destroy(self.handle)
            self.handle = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def admit(self, encoded, mode=FULL):
        """batchImportTxs (FULL) / importDownloadedTxs with a verified proposal (PROPOSAL) over a list of encoded
        transactions (or (data, offsets[n+1])).  Returns (txhash uint8[n,32], sender uint8[n,20], nonce uint8[n,32],
        status uint32[n])."""
        data, off = encoded if isinstance(encoded, tuple) else pack_messages([bytes(e) for e in encoded])
        n = len(off) - 1
        txhash = np.zeros((n, 32), dtype=np.uint8)
        sender = np.zeros((n, 20), dtype=np.uint8)
        nonce = np.zeros((n, 32), dtype=np.uint8)
        status = np.zeros(n, dtype=np.uint32)
        d = data if len(data) else np.zeros(1, dtype=np.uint8)
        check(lib().bcosgpu_txpool_admit(self.handle, mode, _ptr(d), _ptr(off), n, _ptr(txhash), _ptr(sender),
                                         _ptr(nonce), _ptr(status)))
        return txhash, sender, nonce, status

    def block_committed(self, number, txhashes, nonces):
        h, v = _keys(txhashes), _keys(nonces)
        check(lib().bcosgpu_txpool_block_committed(self.handle, number, _ptr(h), len(h), _ptr(v), len(v)))

    def remove(self, txhashes, nonces):
        h, v = _keys(txhashes), _keys(nonces)
        check(lib().bcosgpu_txpool_remove(self.handle, _ptr(h), len(h), _ptr(v), len(v)))

    def load_ledger_nonces(self, blocks):
        """blocks: {number: [nonce, ...]} (LedgerNonceChecker::initNonceCache)."""
        numbers = np.array(list(blocks.keys()), dtype=np.int64)
        lists = [_keys(v) for v in blocks.values()]
        off = np.zeros(len(lists) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(v) for v in lists], dtype=np.uint64)
        keys = np.concatenate(lists) if lists else np.zeros((0, 32), dtype=np.uint8)
        check(lib().bcosgpu_txpool_load_ledger_nonces(self.handle, _ptr(numbers), _ptr(off), _ptr(keys), len(lists)))

    def info(self):
        out = np.zeros(len(_INFO), dtype=np.uint64)
        check(lib().bcosgpu_txpool_info(self.handle, _ptr(out)))
        return dict(zip(_INFO, (int(x) for x in out)))

    def dump(self, which):
        """The keys of set `which` (HASHES / NONCES / LEDGER) in ascending order, uint8[count, 32]."""
        n = ctypes.c_uint64(0)
        count = self.info()[_INFO[which]]
        keys = np.zeros((max(count, 1), 32), dtype=np.uint8)
        check(lib().bcosgpu_txpool_dump(self.handle, which, _ptr(keys), len(keys), ctypes.byref(n)))
        return keys[:n.value]
