"""tests/sm2_vectors.py on the CPU: its restatement verify(e, r, s, P) equals the oracle when e is the hash the
shipped kernels compute, every class of its pool holds what names it, and its comparison helper reports a
flipped verdict under the class it belongs to.  No GPU."""
import os
import re

import numpy as np
import pytest

import sm2_vectors as sv
from test_gpu_ecc import _mutate_sm2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fisco-bcos_amd", "csrc")


@pytest.fixture(scope="module")
def rows():
    return sv.pool()


def _of(rows, cls):
    return [x for x in rows if x[0] == cls]


def _e(x):
    return int.from_bytes(x[2], "big")


def _t(x):
    return (x[3] + x[4]) % sv.N


def test_restatement_equals_the_oracle_on_signed_and_mutated_rows(oracle):
    """320 oracle signatures (a zero and an all-ones digest among them), row i edited by _mutate_sm2 kind i mod 8:
    verify() with e = SM3(Z_A || digest) gives oracle.sm2_recover's verdict on every one, and both verdicts occur
    for the bit flips."""
    rng = np.random.default_rng(0x5D2)
    n = 320
    seen = {k: set() for k in range(8)}
    for i in range(n):
        h = bytes(32) if i == 0 else b"\xff" * 32 if i == 1 else rng.bytes(32)
        sk, k = bytearray(rng.bytes(32)), bytearray(rng.bytes(32))
        sk[0] &= 0x7F
        k[0] &= 0x7F
        sig = _mutate_sm2(rng, oracle.sm2_sign(bytes(sk), h, bytes(k)), i % 8)
        want = oracle.sm2_recover(h, sig) is not None
        r, s, X, Y = (int.from_bytes(sig[j:j + 32], "big") for j in (0, 32, 64, 96))
        e = int.from_bytes(oracle.sm3(oracle.sm2_za(sig[64:]) + h), "big")
        assert sv.verify(e, r, s, (X, Y)) == want, (i, i % 8)
        seen[i % 8].add(want)
    assert seen[0] == {True} and all(seen[k] == {False} for k in range(2, 8)) and False in seen[1]


def test_counts_and_verdicts(rows):
    assert 80 <= len(rows) <= 120 and sum(sv.COUNTS.values()) == len(rows)
    for cls in sv.CLASSES:
        got = _of(rows, cls)
        assert len(got) == sv.COUNTS[cls] > 0, cls
    assert len({(x[0], x[1]) for x in rows}) == len(rows)  # labels name rows
    for x in rows:  # the stored verdict is the restatement's
        assert sv.verify(_e(x), x[3], x[4], (x[5], x[6])) == x[7], x[:2]
    for cls in ("e_rep", "t_shape", "s_shape", "keys"):
        assert all(x[7] for x in _of(rows, cls)), cls
    assert not any(x[7] for x in _of(rows, "reject"))
    for cls in ("x1_ge_n", "final_add", "keyed_lanes"):
        v = [x[7] for x in _of(rows, cls)]
        assert any(v) and not all(v), cls


def test_window_widths_are_the_kernels():
    with open(os.path.join(CSRC, "ecc_pair.hip")) as f:
        assert int(re.search(r"kSm2TrioSplit = (\d+);", f.read()).group(1)) == sv.TRIO_SPLIT
    with open(os.path.join(CSRC, "ecc_row.hip")) as f:
        assert int(re.search(r"kSm2RowSplit = (\d+);", f.read()).group(1)) == sv.ROW_SPLIT_BIT
    with open(os.path.join(CSRC, "ecc_device.h")) as f:
        assert int(re.search(r"kWideBits = (\d+);", f.read()).group(1)) == sv.COMB_WIDE


def test_e_rep(rows):
    got = {x[1]: x for x in _of(rows, "e_rep")}
    for k in range(3):
        a, b = got["small%d" % k], got["small%d+n" % k]
        assert _e(a) < sv.N <= _e(b) == _e(a) + sv.N and a[3:7] == b[3:7] and a[7] and b[7]
    assert [_e(got[l]) for l in ("e=0", "e=n", "e=n-1", "e=2^256-1")] == [0, sv.N, sv.N - 1, 2**256 - 1]
    # e + x1 (both reduced) reaches n in one and stays below it in the other
    w, nw = got["wrap:e+x1=n+1"], got["nowrap:e+x1=n-1"]
    assert _e(w) % sv.N + sv.x_of(w) % sv.N == sv.N + 1 and w[3] == 1
    assert _e(nw) % sv.N + sv.x_of(nw) % sv.N == sv.N - 1 == nw[3]
    a, b = got["wrap-small"], got["wrap-small+n"]  # e + x1 wraps with e small: r below e, in both forms of e
    assert a[3] < _e(a) < sv.N <= _e(b) == _e(a) + sv.N and a[3:7] == b[3:7] and a[7] and b[7]
    assert _e(a) + sv.x_of(a) == sv.N + a[3]
    assert sum(1 for x in got.values() if _e(x) >= sv.N) >= 6


def test_x1_ge_n(rows):
    got = {x[1]: x for x in _of(rows, "x1_ge_n")}
    gap = sv.P - sv.N
    for label in ("first>=n", "first>=n,-y", "last<p"):  # met through c + n alone
        x = got[label]
        x1, c = sv.x_of(x), sv.c_of(x)
        assert sv.N <= x1 < sv.P and c == x1 - sv.N and c != x1 and c + sv.N < sv.P and x[7]
    xa = sv.x_of(got["first>=n"])
    assert all(sv.lift_x(v) is None for v in range(sv.N, xa)) and got["first>=n"][6] != got["first>=n,-y"][6]
    assert all(sv.lift_x(v) is None for v in range(sv.x_of(got["last<p"]) + 1, sv.P))
    x = got["nearest<n"]  # met through c; c + n does not fit in 256 bits
    assert sv.c_of(x) == sv.x_of(x) < sv.N and sv.c_of(x) + sv.N >= 2**256 and x[7]
    assert all(sv.lift_x(v) is None for v in range(sv.x_of(x) + 1, sv.N))
    x = got["small"]  # met through c; c + n < p holds and is another value
    assert sv.c_of(x) == sv.x_of(x) < gap and x[7]
    x = got["c>=p-n:skip"]  # c + n = x(Q) + p fits in 256 bits and is x(Q) mod p: only `c + n < p` rejects
    c = sv.c_of(x)
    assert c >= gap and c + sv.N < 2**256 and (c + sv.N) % sv.P == sv.x_of(x) and not x[7]
    for label in ("c+n=x+1", "c=x-n-1"):  # the branch is taken and must not match
        x = got[label]
        assert sv.c_of(x) + sv.N < sv.P and abs(sv.c_of(x) + sv.N - sv.x_of(x)) == 1 and not x[7]


def test_final_add(rows):
    for x in _of(rows, "final_add"):
        sG, tP = sv.mul(x[4]), sv.mul(_t(x), (x[5], x[6]))
        if x[1].startswith("trio"):  # (s G + T_lo P) + T_hi P
            lo = sv.mul(sv.trio_low_part(_t(x)), (x[5], x[6]))
            hi = sv.add(tP, sv.neg(lo))
            assert lo is not None and hi is not None and x[7] == (not x[1].endswith("e^1"))
            if "dbl-lo" in x[1]:
                assert sG == lo
            elif "dbl-hi" in x[1]:
                assert sv.add(sG, lo) == hi
            else:
                assert sG == sv.neg(lo) and sv.x_of(x) == hi[0]
            continue
        if x[1].startswith("dbl"):
            assert sG == tP and x[7] == (sv.c_of(x) == sv.x_of(x) % sv.N) == (not x[1].endswith("e^1"))
        else:  # infinity, with c the x both operands share
            assert sG == sv.neg(tP) and sv.x_of(x) is None and sv.c_of(x) == sG[0] % sv.N == tP[0] % sv.N and not x[7]


def test_t_shape(rows):
    d = {x[1][2:]: sv.booth_digits(_t(x)) for x in _of(rows, "t_shape")}
    sp = sv.TRIO_SPLIT
    assert d["1"][0] == 1 and not any(d["1"][1:]) and d["2"][0] == 2 and not any(d["2"][1:])
    assert d["2^255"][64] == 1 and d["n-1"][64] == 1 and d["n-1"][63] == 0
    assert d["5"][0] == 5 and d["n-5"][0] != d["n-1"][0]
    assert d["top-window-0"][63:] == [0, 0] and d["top-window-0"][62] != 0
    assert not any(d["lead-windows-0"][51:]) and d["lead-windows-0"][50] == 1
    assert set(d["all+-8"][:64]) == {8, -8} and d["all+-8"][64] == 0
    assert set(d["all-7/-8"][:64]) == {-7, -8} and d["all-7/-8"][64] == 1
    assert not any(d["low-part-0"][:sp]) and any(d["low-part-0"][sp:])
    assert not any(d["high-part-0"][sp:]) and d["high-part-0"][sp - 1] != 0
    assert d["16^split"][sp] == 1 and sum(map(abs, d["16^split"])) == 1
    assert d["16^split/2"][sp - 1] == -8 and d["16^split/2"][sp] == 1  # a carry across the split
    assert d["16^split-1"][0] == -1 and d["16^split-1"][sp] == 1 and not any(d["16^split-1"][1:sp])
    assert d["n-2^176"][sp] != d["n-1"][sp]
    assert all(v == 0 for v in d["alt-windows-0"][1:64:2]) and all(d["alt-windows-0"][0:64:2])
    rs = sv.ROW_SPLIT_BIT
    tv = {x[1][2:]: _t(x) for x in _of(rows, "t_shape")}
    assert tv["row-low-part-0"] % 2**rs == 0 and tv["row-low-part-0"] >> rs and tv["row-2^split-1"] == 2**rs - 1
    assert tv["high-part-0"] >> rs == 0 and tv["n-1"] >> rs and tv["n-1"] % 2**rs
    assert len(d) == sv.COUNTS["t_shape"]


def test_s_shape(rows):
    w16 = {x[1][2:]: sv.comb_windows(x[4], sv.COMB_WIDE) for x in _of(rows, "s_shape")}
    w8 = {x[1][2:]: sv.comb_windows(x[4], sv.COMB_SMALL) for x in _of(rows, "s_shape")}
    assert w16["1"] == [1] + [0] * 15 and w16["2^16"] == [0, 1] + [0] * 14 and w8["2^8"] == [0, 1] + [0] * 30
    assert w16["0xffff"] == [0xFFFF] + [0] * 15 and w16["top16"] == [0] * 15 + [0xFFFF]
    assert w8["top8"] == [0] * 31 + [0xFE] and w16["2^240"] == [0] * 15 + [1] and w8["2^248"] == [0] * 31 + [1]
    assert w16["alt16-lo"] == [0xFFFF, 0] * 8 and w16["alt16-hi"] == [0, 0xFFFF] * 8
    assert w8["alt8-lo"] == [0xFF, 0] * 16 and w8["alt8-hi"] == [0, 0xFF] * 16
    assert w8["ones8"] == [1] * 32 and w16["ones16"] == [1] * 16
    assert all(w16["n-1"]) and all(w8["n-1"])
    assert len(w16) == sv.COUNTS["s_shape"]


def test_keys(rows):
    got = {x[1]: (x[5], x[6]) for x in _of(rows, "keys")}
    assert got["P=G"] == sv.G and got["P=2G"] == sv.mul(2) and got["P=-2G"] == sv.neg(sv.mul(2))
    assert got["P=8G"] == sv.mul(8) and got["P=-G"] == sv.neg(sv.G)
    assert got["P=(0,y)"][0] == 0 == got["P=(0,-y)"][0] and got["P=(0,y)"][1] + got["P=(0,-y)"][1] == sv.P
    assert all(sv.on_curve(p) for p in got.values())


def test_keyed_lanes(rows):
    for x in _of(rows, "keyed_lanes"):
        L = sv.keyed_lane_points(x)
        assert _t(x) < 2**16 and all(p is None for p in L[4:])
        kind = x[1].split("/")[0]
        assert x[7] == (kind != "inf" and not x[1].endswith("e^1"))
        if kind == "dbl1":
            assert L[0] == L[1] is not None
        elif kind == "neg1":
            assert L[0] == sv.neg(L[1]) is not None and L[2] is not None and x[7]
        elif kind == "dbl2":
            assert sv.add(L[0], L[1]) == sv.add(L[2], L[3]) is not None and L[0] != L[1]
        else:
            total = None
            for p in L:
                total = sv.add(total, p)
            assert kind == "inf" and total is None and not x[7]


def test_reject(rows):
    by = {(x[0], x[1]): x for x in rows}
    kinds = {"e^2": 0, "r+s=n": 0, "off-curve": 0}
    for x in _of(rows, "reject"):
        kind, twin = x[1].split(":", 1)
        kinds[kind[:3] if kind.startswith("e^2") else kind] += 1
        a = next(v for k, v in by.items() if k[1] == twin and k[0] != "reject")
        assert a[7] and not x[7]
        if kind.startswith("e^2"):
            assert bin(_e(a) ^ _e(x)).count("1") == 1 and a[3:7] == x[3:7]
        elif kind == "r+s=n":
            assert x[3] + x[4] == sv.N and a[3] == x[3]
        else:
            assert not sv.on_curve((x[5], x[6])) and sv.on_curve((a[5], a[6]))
    assert all(v >= 3 for v in kinds.values()), kinds


def test_compare_reports_the_class_of_a_flipped_verdict(rows):
    want = [x[7] for x in rows]
    assert sv.compare(rows, want) == {}
    for cls in sv.CLASSES:
        i = next(i for i, x in enumerate(rows) if x[0] == cls)
        bad = list(want)
        bad[i] = not bad[i]
        assert sv.compare(rows, bad) == {cls: [rows[i][1]]}
    with pytest.raises(AssertionError):
        sv.compare(rows, want[:-1])


def test_packed_round_trips(rows):
    for x, (h, sig) in zip(rows, sv.packed(rows)):
        assert len(h) == 32 and len(sig) == 128 and h == x[2]
        assert [int.from_bytes(sig[j:j + 32], "big") for j in (0, 32, 64, 96)] == list(x[3:7])
