"""tests/k1_verify_vectors.py on the CPU: its restatement verify(h32, r, s, P) equals the oracle on every row of
its pool and on signed-and-edited rows, every class holds what names it, each named wrong restatement of the
kernels' decisions gets a row of its class wrong, and the comparison helper reports a flipped verdict under the
class it belongs to.  No GPU."""
import os
import re

import numpy as np
import pytest

import k1_verify_vectors as kv
import test_gpu_glv_split as glv
from test_gpu_trio_chain_start import split
from test_gpu_verify import _edit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fisco-bcos_amd", "csrc")


@pytest.fixture(scope="module")
def rows():
    return kv.pool()


def _of(rows, cls):
    return [x for x in rows if x[0] == cls]


def _b(v):
    return v.to_bytes(32, "big")


def test_restatement_equals_the_oracle_on_every_row(rows, oracle):
    left_out = 0
    for x in rows:
        want = oracle.secp256k1_verify(_b(x[5]) + _b(x[6]), x[2], _b(x[3]) + _b(x[4]))
        assert want == x[7] == kv.verify(x[2], x[3], x[4], (x[5], x[6])), x[:2]
    assert left_out == 0


def test_restatement_equals_the_oracle_on_signed_and_edited_rows(oracle):
    """300 oracle signatures (a zero and an all-ones hash among them), row i edited by test_gpu_verify's _edit kind
    i mod 10: verify() gives oracle.secp256k1_verify's verdict on every one."""
    rng = np.random.default_rng(0x6B31)
    n = 300
    h = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    h[0], h[10] = 0, 0xFF
    pub, sig = np.zeros((n, 64), dtype=np.uint8), np.zeros((n, 65), dtype=np.uint8)
    for i in range(n):
        sk, k = bytearray(rng.bytes(32)), bytearray(rng.bytes(32))
        sk[0] &= 0x7F
        k[0] &= 0x7F
        pub[i] = np.frombuffer(oracle.secp256k1_pubkey(bytes(sk)), dtype=np.uint8)
        sig[i] = np.frombuffer(oracle.secp256k1_sign(bytes(sk), h[i].tobytes(), bytes(k)), dtype=np.uint8)
    seen = {k: set() for k in range(10)}
    for i in range(n):
        _edit(rng, pub, h, sig, i, i % 10, kv.N, pub[(i + 1) % n].copy())
        want = oracle.secp256k1_verify(pub[i].tobytes(), h[i].tobytes(), sig[i, :64].tobytes())
        r, s, X, Y = (int.from_bytes(v.tobytes(), "big") for v in (sig[i, 0:32], sig[i, 32:64], pub[i, 0:32], pub[i, 32:64]))
        assert kv.verify(h[i].tobytes(), r, s, (X, Y)) == want, (i, i % 10)
        seen[i % 10].add(want)
    assert seen[0] == {True} and all(seen[k] == {False} for k in (1, 2, 3, 5, 6, 7, 8, 9)) and False in seen[4]


def test_counts_and_verdicts(rows):
    assert 90 <= len(rows) <= 120 and sum(kv.COUNTS.values()) == len(rows)
    for cls in kv.CLASSES:
        assert len(_of(rows, cls)) == kv.COUNTS[cls] > 0, cls
    assert len({(x[0], x[1]) for x in rows}) == len(rows)  # labels name rows
    for cls in ("e_rep", "u2_shape", "u1_shape"):
        assert all(x[7] for x in _of(rows, cls)), cls
    assert not any(x[7] for x in _of(rows, "reject"))
    for cls in ("x_ge_n", "s_edge", "final_add", "keys"):
        v = [x[7] for x in _of(rows, cls)]
        assert any(v) and not all(v), cls
    # every launch of 21 or more rows, from any row on, holds both verdicts
    for n in (kv.LAUNCH_MIN, 39, 40, 41, 65):
        for a in range(len(rows) - n + 1):
            assert len({x[7] for x in rows[a:a + n]}) == 2, (n, a)


def test_comb_layout_and_scalars_are_the_kernels():
    with open(os.path.join(CSRC, "ecc_device.h")) as f:
        assert int(re.search(r"kWideBits = (\d+);", f.read()).group(1)) == kv.COMB_WIDE
    with open(os.path.join(CSRC, "ecc_coop.hip")) as f:
        m = re.search(r"kTrioVerifyShare = ([^;]*);", f.read())
    pairs = tuple((int(a), int(b)) for a, b in re.findall(r"\{(\d+), (\d+)\}", m.group(1)))
    assert pairs == kv.VERIFY_SHARE[kv.COMB_WIDE] + kv.VERIFY_SHARE[kv.COMB_SMALL]
    for bits, share in kv.VERIFY_SHARE.items():  # the four shares tile the windows
        s = sorted(share)
        assert s[0][0] == 0 and s[-1][1] == 256 // bits and all(a[1] == b[0] for a, b in zip(s, s[1:]))
    assert kv.GLV_EDGES == glv.EDGES[1:] and kv.GLV_FOUND == glv.FOUND and kv.GLV_SMALL == glv.SMALL
    assert kv.LAMBDA == glv.LAMBDA and kv.mul(kv.LAMBDA)[1] == kv.G[1] and kv.on_curve(kv.G)


def test_x_ge_n(rows):
    got = {x[1]: x for x in _of(rows, "x_ge_n")}
    gap = kv.P - kv.N
    # the curve's x values at the edges of [n, p): n (r = 0), n + 2, p - 3
    assert kv.lift_x(kv.N) is not None and kv.lift_x(kv.N + 1) is None and kv.lift_x(kv.N + 2) is not None
    assert kv.lift_x(kv.P - 1) is None and kv.lift_x(kv.P - 2) is None and kv.lift_x(kv.P - 3) is not None
    for label in ("first>n", "first>n,-y", "last<p", "last<p,-y", "mid"):  # met through r + n alone
        x = got[label]
        assert kv.N <= kv.x_of(x) < kv.P and x[3] == kv.x_of(x) - kv.N and x[3] + kv.N < kv.P and x[7]
    assert kv.x_of(got["first>n"]) == kv.N + 2 and kv.x_of(got["last<p"]) == kv.P - 3
    assert kv.N + 2**100 < kv.x_of(got["mid"]) < kv.P - 2**100
    ys = lambda l: kv.add(*kv.summands(got[l]))[1] & 1
    assert ys("first>n") != ys("first>n,-y") and ys("last<p") != ys("last<p,-y")
    x = got["small"]  # met through r; r + n < p holds and is another value
    assert x[3] == kv.x_of(x) == 1 and x[3] + kv.N < kv.P and x[7]
    x = got["r=p-n"]  # met through r; r + n = p
    assert x[3] == kv.x_of(x) == gap and x[7]
    x = got["r+n=x+p:skip"]  # r + n fits in 256 bits and is x(Q) mod p: only `r + n < p` rejects
    assert gap <= x[3] < kv.N and x[3] + kv.N < 2**256 and (x[3] + kv.N) % kv.P == kv.x_of(x) and not x[7]
    x = got["r+n=x+1"]  # the branch is taken and must not match
    assert x[3] + kv.N < kv.P and x[3] + kv.N == kv.x_of(x) + 1 and not x[7]
    x = got["r=x>=n"]  # x(Q) itself as r
    assert x[3] == kv.x_of(x) >= kv.N and not x[7]
    assert all(0 < x[4] <= kv.HALF for x in got.values())  # nothing but the comparison decides


def test_s_edge(rows):
    got = {x[1]: x for x in _of(rows, "s_edge")}
    want = {"s=1": 1, "s=2": 2, "s=(n-1)/2": kv.HALF, "s=(n-1)/2-1": kv.HALF - 1, "s=(n+1)/2": kv.HALF + 1,
            "s=n-1": kv.N - 1, "s=n": kv.N, "s=n+1": kv.N + 1, "s=0": 0}
    assert {l: x[4] for l, x in got.items()} == want and 2 * kv.HALF + 1 == kv.N
    assert all(x[7] == (0 < x[4] <= kv.HALF) for x in got.values())
    for low, high in (("s=(n-1)/2", "s=(n+1)/2"), ("s=1", "s=n-1")):  # the twin (r, n - s) is the same equation
        a, b = got[low], got[high]
        assert a[4] + b[4] == kv.N and a[2:4] == b[2:4] and a[5:7] == b[5:7]
        assert kv.x_of(b) % kv.N == b[3]
    assert got["s=n+1"][2:4] == got["s=1"][2:4] and got["s=n+1"][5:7] == got["s=1"][5:7]  # s mod n would be accepted


def test_e_rep(rows):
    got = {x[1]: x for x in _of(rows, "e_rep")}
    top = 2 * kv.N - 2**256
    want = {"h=0": 0, "h=n": kv.N, "h=n-1": kv.N - 1, "h=n+1": kv.N + 1, "h=2n-2^256-1": top - 1, "h=2n-2^256": top,
            "h=2n-2^256+1": top + 1, "h=2^256-1": 2**256 - 1}
    assert all(kv.h_of(got[l]) == h for l, h in want.items())
    assert kv.u1_of(got["h=0"]) == 0 == kv.u1_of(got["h=n"]) and kv.summands(got["h=n"])[0] is None
    a, b = got["e"], got["e+n"]
    assert kv.h_of(a) < kv.N <= kv.h_of(b) == kv.h_of(a) + kv.N and a[3:7] == b[3:7]
    assert sum(1 for x in got.values() if kv.h_of(x) >= kv.N) == 4


def test_final_add(rows):
    got = {x[1]: x for x in _of(rows, "final_add")}
    keys = {"P=G": kv.G, "P=-G": kv.neg(kv.G), "P=2G": kv.mul(2), "P=lambdaG": kv.mul(kv.LAMBDA)}
    for label, x in got.items():
        A, B = kv.summands(x)
        assert A is not None and B is not None
        kind, key = label.split(":")
        if key == "keyed-last":  # the registered-key kernel's last lane sum: lanes 0..7 against lanes 8..15
            u1, u2 = kv.u1_of(x), kv.u2_of(x)
            low = kv.add(kv.mul(u1 % 2**128), B)
            assert u2 < 2**16 and low == kv.mul(u1 >> 128 << 128) and A != B and x[7]
            continue
        if key in keys:
            assert (x[5], x[6]) == keys[key]
        if kind == "dbl":
            assert A == B and x[7] == (key != "d,r+1")
        else:
            assert A == kv.neg(B) and kv.x_of(x) is None and x[3] == A[0] % kv.N and not x[7]
    assert kv.h_of(got["dbl:P=G"]) == got["dbl:P=G"][3]  # h = r
    assert kv.h_of(got["inf:P=G"]) == kv.N - got["inf:P=G"][3]  # h = n - r
    a, b = got["dbl:d"], got["dbl:d,r+1"]
    assert b[3] == a[3] + 1 and kv.summands(a)[0][0] == kv.summands(b)[0][0] and a[5:7] == b[5:7]


def test_u2_shape(rows):
    got = {x[1]: kv.u2_of(x) for x in _of(rows, "u2_shape")}
    assert [got["edge%d" % i] for i in range(13)] == glv.EDGES[1:]
    assert [got["found%d" % i] for i in range(4)] == glv.FOUND and [got["small%d" % i] for i in range(20)] == glv.SMALL
    for label, want in kv.GLV_HALVES.items():
        assert split(got[label]) == want, label  # halves this short are the cell's own
    for label in ("low++", "low-+"):
        k1, k2 = split(got[label])
        assert 0 < abs(k1) < 2**123 and 0 < abs(k2) < 2**123
    assert {(split(got[l])[0] == 0, split(got[l])[1] == 0) for l in ("k1=0", "k1=0,-", "k2=0", "k2=0,-")} == \
        {(True, False), (False, True)}
    assert split(got["k1=0,-"])[1] < 0 < split(got["k1=0"])[1] and split(got["k2=0,-"])[0] < 0 < split(got["k2=0"])[0]
    assert all(split(got["small%d" % i])[1 - (i % 4) // 2] == 0 for i in range(20))  # c: k2 = 0; c lambda: k1 = 0
    assert len(got) == kv.COUNTS["u2_shape"]


def test_u1_shape(rows):
    got = {x[1][3:]: kv.u1_of(x) for x in _of(rows, "u1_shape")}
    nz = lambda u, bits: [w for w, v in enumerate(kv.comb_shares(u, bits)) if v]  # the waves with a nonzero share
    for bits in (kv.COMB_WIDE, kv.COMB_SMALL):
        for w in range(4):
            assert nz(got["only%d" % w], bits) == [w], (bits, w)
            assert nz(got["zero%d" % w], bits) == [v for v in range(4) if v != w], (bits, w)
        assert nz(got["n-1"], bits) == [0, 1, 2, 3] and nz(got["1"], bits) == [0]
    assert nz(got["only0/16,3/8"], 16) == [0] and nz(got["only0/16,3/8"], 8) == [3]
    assert nz(got["only3/16,2/8"], 16) == [3] and nz(got["only3/16,2/8"], 8) == [2]
    assert got["1"] == 1 and got["n-1"] == kv.N - 1
    w = kv.comb_windows(got["max-windows"], 16)
    assert w.count(0xFFFF) == 15 and got["max-windows"] < kv.N
    # no scalar below n has 16: n's own windows 8..15 are 0xfffe, 0xffff x 7, so a 16th would reach n
    assert kv.comb_windows(kv.N, 16)[8:] == [0xFFFE] + [0xFFFF] * 7 and kv.comb_windows(got["max-windows"], 8).count(0xFF) == 31
    assert len(got) == kv.COUNTS["u1_shape"]


def test_keys(rows):
    got = {x[1]: x for x in _of(rows, "keys")}
    key = lambda l: (got[l][5], got[l][6])
    assert key("x=1")[0] == 1 and pow(key("x=1")[1], 2, kv.P) == 8 and key("x=1,-y") == kv.neg(key("x=1"))
    assert key("y=1")[1] == 1 and all(kv.on_curve(key(l)) and got[l][7] for l in ("x=1", "x=1,-y", "y=1"))
    for twin, label in (("x=1", "x=1+p"), ("y=1", "y=1+p")):  # valid once reduced, under the twin's signature
        a, b = got[twin], got[label]
        assert a[2:5] == b[2:5] and (b[5] % kv.P, b[6] % kv.P) == key(twin) and key(label) != key(twin)
        assert max(key(label)) == 1 + kv.P < 2**256 and not b[7]
    assert key("(0,0)") == (0, 0) and not got["(0,0)"][7]
    x, y = key("twist")
    assert x < kv.P and y < kv.P and (y * y + x**3 + 7) % kv.P == 0 and kv.lift_x(x) is None and not got["twist"][7]
    assert key("y^2^200") == (1, key("x=1")[1] ^ (1 << 200)) and got["y^2^200"][2:5] == got["x=1"][2:5]
    # rows follow their twins
    order = [x[1] for x in rows if x[0] == "keys"]
    assert order.index("x=1+p") == order.index("x=1") + 1 and order.index("y=1+p") == order.index("y=1") + 1


def test_reject(rows):
    by = {x[1]: x for x in rows if x[0] != "reject"}
    kinds = set()
    for x in _of(rows, "reject"):
        kind, twin = x[1].split(":", 1)
        a = by[twin]
        assert a[7] and not x[7]
        same = [a[i] == x[i] for i in (2, 3, 4)] + [a[5:7] == x[5:7]]
        assert same.count(False) == 1, x[1]  # one field differs from an accepted row
        kinds.add(kind.split("^")[0].split("-")[0].split("=")[0].split("+")[0])
    assert kinds == {"h", "r", "s", "key"}
    assert by["found0"][3] and not next(x for x in rows if x[1] == "r=0:found0")[3]
    assert next(x for x in rows if x[1] == "r=n:small0")[3] == kv.N


# ------------------------------------------------------------------ the rows catch what they are named after
def _restated(h32, r, s, pub, second=True, guard=True, s_max=kv.HALF, key_range=True, reduce_e=True, inf_ok=False,
              dbl_inf=False):
    """The kernels' decisions as they take them (the comparison on X == r Z^2, not on x mod n), each of which a
    flag gets wrong.  reduce_e=False: no step takes the hash into [0, n), so a hash of n or more is no scalar and
    the row is refused, as an r or s out of range is.  inf_ok: the infinity flag is not read and X = Z = 0 meets
    X == r Z^2.  dbl_inf: the final addition's equal operands give infinity."""
    X, Y = pub
    if key_range and not (X < kv.P and Y < kv.P):
        return False
    pub = (X % kv.P, Y % kv.P)
    if not kv.on_curve(pub) or not (0 < r < kv.N and 0 < s <= s_max):
        return False
    e = int.from_bytes(h32, "big")
    if reduce_e:
        e %= kv.N
    elif e >= kv.N:
        return False
    w = pow(s, -1, kv.N)
    A, B = kv.mul(e * w % kv.N), kv.mul(r * w % kv.N, pub)
    Q = None if dbl_inf and A == B else kv.add(A, B)
    if Q is None:
        return inf_ok
    if Q[0] == r:
        return True
    return second and (not guard or r + kv.N < kv.P) and (r + kv.N) % kv.P == Q[0]


MUTANTS = {"no second comparison": ("x_ge_n", dict(second=False)),
           "second comparison without the r + n < p guard": ("x_ge_n", dict(guard=False)),
           "s <= n/2 + 1": ("s_edge", dict(s_max=kv.HALF + 1)),
           "s < (n-1)/2": ("s_edge", dict(s_max=kv.HALF - 1)),
           "no key range check": ("keys", dict(key_range=False)),
           "e not reduced": ("e_rep", dict(reduce_e=False)),
           "Q = infinity accepted": ("final_add", dict(inf_ok=True)),
           "doubling returned as infinity": ("final_add", dict(dbl_inf=True))}


def test_restated_decisions_equal_the_reference(rows):
    for x in rows:
        assert _restated(x[2], x[3], x[4], (x[5], x[6])) == x[7], x[:2]


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_each_wrong_restatement_fails_a_row_of_its_class(rows, name):
    cls, flags = MUTANTS[name]
    wrong = kv.compare(rows, [_restated(x[2], x[3], x[4], (x[5], x[6]), **flags) for x in rows])
    assert wrong.get(cls), (name, wrong)
    print(name, wrong)


def test_compare_reports_the_class_of_a_flipped_verdict(rows):
    want = [x[7] for x in rows]
    assert kv.compare(rows, want) == {}
    for cls in kv.CLASSES:
        i = next(i for i, x in enumerate(rows) if x[0] == cls)
        bad = list(want)
        bad[i] = not bad[i]
        assert kv.compare(rows, bad) == {cls: [rows[i][1]]}
    with pytest.raises(AssertionError):
        kv.compare(rows, want[:-1])


def test_packed_round_trips(rows):
    for x, (h, sig, pub) in zip(rows, kv.packed(rows)):
        assert len(h) == 32 and len(sig) == 64 and len(pub) == 64 and h == x[2]
        assert [int.from_bytes(v[j:j + 32], "big") for v in (sig, pub) for j in (0, 32)] == list(x[3:7])
