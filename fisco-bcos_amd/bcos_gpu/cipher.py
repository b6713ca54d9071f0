"""Storage-cipher mirror: DataEncryption over a batch of storage values (AES-256-CBC / SM4-CBC, PKCS#7).

  RocksDBStorage::asyncPrepare    bcos-storage/bcos-storage/RocksDBStorage.cpp:348-353  (encrypt, the block commit)
  RocksDBStorage::setRows         :513-524                                              (encrypt)
  RocksDBStorage::asyncGetRow     :106-108                                              (decrypt)
  RocksDBStorage::asyncGetRows    :204-205                                              (decrypt)
  DataEncryption::encrypt/decrypt bcos-security/bcos-security/DataEncryption.cpp:143-165
  AESCrypto / SM4Crypto           bcos-crypto/bcos-crypto/encrypt/AESCrypto.cpp:29-51, SM4Crypto.cpp:28-49

The key, IV and padding rules and the one stated deviation (a default IV from a key shorter than 16 bytes is
zero-filled) are in include/bcos_gpu.h.
"""
import ctypes

import numpy as np

from ._lib import CBC_E_LENGTH, CBC_E_PADDING, CBC_OK, CIPHER_AES256, CIPHER_SM4, check, ensure_device, lib
from .crypto import _ptr

__all__ = ["CIPHER_AES256", "CIPHER_SM4", "CBC_OK", "CBC_E_LENGTH", "CBC_E_PADDING", "padded_size",
           "encrypt_values", "decrypt_values"]


class _BytesView(ctypes.Structure):
    """bcosgpu_Bytes (include/bcos_gpu.h)."""
    _fields_ = [("data", ctypes.c_char_p), ("len", ctypes.c_size_t)]


def _views(values):
    keep = [bytes(v) for v in values]
    views = (_BytesView * max(len(keep), 1))()
    for i, b in enumerate(keep):
        views[i].data, views[i].len = b, len(b)
    return views, keep


def padded_size(n):
    """The ciphertext bytes of an n-byte value: (n // 16 + 1) * 16."""
    return (n // 16 + 1) * 16


def _iv(iv):
    return (None, 0) if iv is None else (bytes(iv), len(iv))


def encrypt_values(cipher, key, values, iv=None):
    """bcosgpu_cbc_encrypt_batch: list[bytes] -> list[bytes] of ciphertexts under one key (iv None: the default
    IV, the first 16 bytes of the raw key).  Every value is encrypted, an empty one to one block; the RocksDB
    sites skip empty values before they call."""
    ensure_device()
    n = len(values)
    views, keep = _views(values)
    cap = sum(padded_size(len(b)) for b in keep)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    ivb, ivn = _iv(iv)
    check(lib().bcosgpu_cbc_encrypt_batch(cipher, bytes(key), len(key), ivb, ivn, views, n, _ptr(out), cap, _ptr(off)))
    del keep
    raw = out.tobytes()
    return [raw[int(off[i]):int(off[i + 1])] for i in range(n)]


def decrypt_values(cipher, key, values, iv=None):
    """bcosgpu_cbc_decrypt_batch: list[bytes] of ciphertexts -> (list[bytes] plaintexts, uint8 status[n]); a
    failed item (CBC_E_LENGTH, CBC_E_PADDING: where the reference throws DecryptException) gives b""."""
    ensure_device()
    n = len(values)
    views, keep = _views(values)
    cap = sum(len(b) for b in keep)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    status = np.zeros(max(n, 1), dtype=np.uint8)
    ivb, ivn = _iv(iv)
    check(lib().bcosgpu_cbc_decrypt_batch(cipher, bytes(key), len(key), ivb, ivn, views, n, _ptr(out), cap, _ptr(off),
                                          _ptr(status)))
    del keep
    raw = out.tobytes()
    return [raw[int(off[i]):int(off[i + 1])] for i in range(n)], status[:n]
