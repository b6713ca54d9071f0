"""The bcosgpu_txpool_* C ABI without a device: the header's prototypes against the ctypes signatures of
bcos_gpu/_lib.py, and the argument checks that are made before any HIP call."""
import ctypes
import re

import numpy as np

from bcos_gpu import _lib, txpool

NAMES = ["create", "destroy", "admit", "admit_dev", "block_committed", "remove", "load_ledger_nonces", "info", "dump"]


def _ctype(param):
    if "*" in param or "[" in param:
        return "pointer"
    for c_name, t in (("size_t", ctypes.c_size_t), ("uint64_t", ctypes.c_uint64), ("int64_t", ctypes.c_int64),
                      ("int", ctypes.c_int)):
        if re.search(r"\b%s\b" % c_name, param):
            return t
    raise AssertionError(param)


def test_header_prototypes_and_ctypes_signatures_agree():
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    for name in NAMES:
        sym = "bcosgpu_txpool_" + name
        m = re.search(r"^int %s\(([^;]*)\);" % sym, text, re.M | re.S)
        assert m, sym
        want = [_ctype(p) for p in m.group(1).split(",")]
        res, args = _lib._SIGS[sym]
        assert res is ctypes.c_int
        got = ["pointer" if a in (ctypes.c_void_p, ctypes.c_char_p) else a for a in args]
        assert got == want, sym
    assert sorted(s for s in _lib.header_symbols() if "_txpool_" in s) == sorted("bcosgpu_txpool_" + n for n in NAMES)
    for macro, value in (("BCOSGPU_E_ENGINE", _lib.E_ENGINE), ("BCOSGPU_TXPOOL_FULL", txpool.FULL),
                         ("BCOSGPU_TXPOOL_PROPOSAL", txpool.PROPOSAL), ("BCOSGPU_TXPOOL_HASHES", txpool.HASHES),
                         ("BCOSGPU_TXPOOL_NONCES", txpool.NONCES), ("BCOSGPU_TXPOOL_LEDGER", txpool.LEDGER),
                         ("BCOSGPU_TXPOOL_INFO_WORDS", len(txpool._INFO))):
        m = re.search(r"#define %s \(?(-?\d+)\)?" % macro, text)
        assert m and int(m.group(1)) == value, macro


def _message():
    return _lib.lib().bcosgpu_last_error().decode()


def test_create_rejects_bad_arguments_before_touching_a_device():
    L = _lib.lib()
    h = ctypes.c_void_p()
    ok = (0, 0, b"chain0", 6, b"group0", 6, 10, 0, 8)
    assert L.bcosgpu_txpool_create(*ok, None) == _lib.E_ARG
    for bad in ((0, 7) + ok[2:], ok[:6] + (-1, 0, 8), ok[:6] + (10, -1, 8), ok[:6] + (2 ** 62 + 1, 0, 8),
                ok[:8] + (2 ** 31,), (0, 0, None, 6) + ok[4:], (0, 0, b"x", 1, None, 3) + ok[6:],
                (0, 0, b"chain0", 2 ** 16) + ok[4:]):
        assert L.bcosgpu_txpool_create(*bad, ctypes.byref(h)) == _lib.E_ARG, bad
        assert h.value is None and _message()


def test_a_null_pool_is_an_argument_error_on_every_call():
    L = _lib.lib()
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data
    assert L.bcosgpu_txpool_admit(None, 0, p, p, 1, p, p, p, p) == _lib.E_ARG
    assert L.bcosgpu_txpool_admit_dev(None, 0, p, p, 1, 1, p, p, p, p) == _lib.E_ARG
    assert L.bcosgpu_txpool_block_committed(None, 1, p, 1, p, 1) == _lib.E_ARG
    assert L.bcosgpu_txpool_remove(None, p, 1, p, 1) == _lib.E_ARG
    assert L.bcosgpu_txpool_load_ledger_nonces(None, p, p, p, 1) == _lib.E_ARG
    assert L.bcosgpu_txpool_info(None, p) == _lib.E_ARG
    assert L.bcosgpu_txpool_dump(None, 0, p, 1, p) == _lib.E_ARG
    assert "null pool" in _message()
    assert L.bcosgpu_txpool_destroy(None) == 0
