"""State-side mirror: the state root of a block's dirty storage entries.

  TransactionExecutor::getHash    bcos-executor/src/executor/TransactionExecutor.cpp:1099
  StateStorage::hash              bcos-table/src/StateStorage.h:397-431
      XOR over dirty entries of H(table) ^ H(key) ^ Entry::hash(table, key, H, blockVersion)
  KeyPageStorage::hash            bcos-table/src/KeyPageStorage.cpp:351-406 (system-table entries: the same)
  PageData::hash                  bcos-table/src/KeyPageStorage.h:862-893 (page entries: Entry::hash alone from
                                  block version 3.1 on, with H(table) ^ H(key) at 3.0)
  Entry::hash                     bcos-framework/bcos-framework/storage/Entry.h:229-309
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from ._lib import check, ensure_device, lib
from .crypto import _ptr

ENTRY_NORMAL, ENTRY_DELETED, ENTRY_EMPTY, ENTRY_MODIFIED = 0, 1, 2, 3  # Entry::Status
STATE_XOR_NAMES = 1
V3_1_VERSION = 0x03010000  # BlockVersion::V3_1_VERSION


@dataclass
class StateEntry:
    """One storage entry as the state root sees it; flags: STATE_XOR_NAMES for every StateStorage entry,
    every KeyPage system-table entry, and every KeyPage page entry at block version 3.0."""
    table: bytes = b""
    key: bytes = b""
    value: bytes = b""
    status: int = ENTRY_MODIFIED
    flags: int = STATE_XOR_NAMES


class _StateEntryView(ctypes.Structure):
    """bcosgpu_StateEntry (include/bcos_gpu.h): pointers into the caller's fields."""
    _fields_ = [("table", ctypes.c_char_p), ("table_len", ctypes.c_size_t),
                ("key", ctypes.c_char_p), ("key_len", ctypes.c_size_t),
                ("value", ctypes.c_char_p), ("value_len", ctypes.c_size_t),
                ("status", ctypes.c_int8), ("flags", ctypes.c_uint8)]


def _b(x):
    return x.encode() if isinstance(x, str) else bytes(x)


def state_entry_views(entries):
    """ctypes views of StateEntry objects; returns (views array, keep-alive list)."""
    n = len(entries)
    views = (_StateEntryView * max(n, 1))()
    keep = []
    for i, e in enumerate(entries):
        fields = (_b(e.table), _b(e.key), _b(e.value))
        keep.append(fields)
        v = views[i]
        for name, b in zip(("table", "key", "value"), fields):
            setattr(v, name, b)
            setattr(v, name + "_len", len(b))
        v.status, v.flags = e.status, e.flags
    return views, keep


def pack_state_entries(entries):
    """The native packer (bcosgpu_pack_state_entries, host C++): list[StateEntry] -> (uint8 data,
    uint64 off3[3n+1], uint8 kind[n]), the layout bcosgpu_state_root_dev / device.state_root take."""
    views, keep = state_entry_views(entries)
    n = len(entries)
    size = int(lib().bcosgpu_state_entries_size(views, n))
    out = np.zeros(max(size, 1), dtype=np.uint8)
    off3 = np.zeros(3 * n + 1, dtype=np.uint64)
    kind = np.zeros(max(n, 1), dtype=np.uint8)
    check(lib().bcosgpu_pack_state_entries(views, n, _ptr(out), size, _ptr(off3), _ptr(kind)))
    del keep
    return out[:size], off3, kind[:n]


def state_root(hasher, block_version, entries) -> bytes:
    """bcosgpu_state_root: StateStorage::hash / KeyPageStorage::hash of `entries` on the GPU (hasher:
    KECCAK256 or SM3; block_version as in the block header, e.g. V3_1_VERSION)."""
    ensure_device()
    views, keep = state_entry_views(entries)
    root = np.zeros(32, dtype=np.uint8)
    check(lib().bcosgpu_state_root(hasher, block_version, views, len(entries), _ptr(root)))
    del keep
    return root.tobytes()
