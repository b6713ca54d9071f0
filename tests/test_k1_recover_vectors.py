"""tests/k1_recover_vectors.py on the CPU: its restatement recover(h32, r, s, v) equals the oracle on every row of
its pool, on the transaction rows and on signed-and-mutated rows, every class holds what names it, the share
tables are the source's, no intermediate addition of any body can meet equal or opposite operands, each named
wrong restatement of the kernels' decisions gets a row of its class wrong, and the comparison helper reports a
wrong verdict, key or address under the class it belongs to.  No GPU."""
import hashlib
import os
import re

import numpy as np
import pytest

import k1_recover_vectors as rv
import k1_verify_vectors as kv
import test_gpu_glv_split as glv
from test_gpu_ecc import _mutate
from test_gpu_trio_chain_start import A1, A2, MB1, split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fisco-bcos_amd", "csrc")
N, P = kv.N, kv.P


@pytest.fixture(scope="module")
def rows():
    return rv.pool()


@pytest.fixture(scope="module")
def tx_rows():
    return rv.tx_rows([hashlib.sha256(b"tx %d" % i).digest() for i in range(41)])


def _of(rows, cls):
    return [x for x in rows if x[0] == cls]


def _labelled(rows, cls):
    return {x[1]: x for x in rows if x[0] == cls}


def _pub(x):
    return None if x[4] is None else rv.pub_bytes(x[4])


def test_restatement_equals_the_oracle_on_every_row(rows, tx_rows, oracle):
    assert rv.CASES_LEFT_OUT == 0
    for x in rows + tx_rows:
        assert oracle.secp256k1_recover(x[2], x[3]) == _pub(x), x[:2]
        assert rv.recover(x[2], *rv.rsv_of(x)) == x[4], x[:2]


def test_restatement_equals_the_oracle_on_signed_and_mutated_rows(oracle):
    """300 oracle signatures (a zero and an all-ones hash among them), row i mutated by test_gpu_ecc's _mutate kind
    i mod 9: recover() gives oracle.secp256k1_recover's key or refusal on every one."""
    rng = np.random.default_rng(0x6B32)
    seen = {k: set() for k in range(9)}
    for i in range(300):
        h = bytes(32) if i == 0 else b"\xff" * 32 if i == 9 else rng.bytes(32)
        sk, k = bytearray(rng.bytes(32)), bytearray(rng.bytes(32))
        sk[0] &= 0x7F
        k[0] &= 0x7F
        sk[31] |= 1
        k[31] |= 1
        sig = _mutate(rng, oracle.secp256k1_sign(bytes(sk), h, bytes(k)), i % 9)
        want = oracle.secp256k1_recover(h, sig)
        got = rv.recover(h, int.from_bytes(sig[0:32], "big"), int.from_bytes(sig[32:64], "big"), sig[64])
        assert (None if got is None else rv.pub_bytes(got)) == want, (i, i % 9)
        if i % 9 == 0:
            assert want == oracle.secp256k1_pubkey(bytes(sk))
        seen[i % 9].add(want is not None)
    assert seen[0] == {True} and seen[4] == seen[5] == seen[6] == {False} and seen[2] == seen[7] == {True, False}


def test_counts_and_verdicts(rows, tx_rows):
    assert 150 <= len(rows) <= 200 and sum(rv.COUNTS.values()) == len(rows)
    for cls in rv.CLASSES:
        assert len(_of(rows, cls)) == rv.COUNTS[cls] > 0, cls
    for cls, n in rv.TX_COUNTS.items():
        assert len(_of(tx_rows, cls)) == n, cls
    for pool in (rows, tx_rows):
        assert len({(x[0], x[1]) for x in pool}) == len(pool)  # labels name rows
        for n in (rv.LAUNCH_MIN, 39, 40, 41, 65):  # every launch of 21 or more rows, from any row on
            for a in range(len(pool) - n + 1):
                assert len({x[4] is None for x in pool[a:a + n]}) == 2, (n, a)
    for cls in ("e_rep", "u2_shape", "u1_shape", "key_out"):
        assert all(x[4] is not None for x in _of(rows, cls)), cls
    assert not any(x[4] is not None for x in _of(rows, "reject") + _of(tx_rows, "reject"))
    for cls in ("x_r", "s_edge", "final_add"):
        v = [x[4] is None for x in _of(rows, cls)]
        assert any(v) and not all(v), cls
    # a transaction row over a hash keeps the signature of the pool's row
    pool_sig = {(x[0], x[1]): x[3] for x in rows}
    for x in tx_rows:
        if x[0] in ("x_r", "s_edge", "u2_shape"):
            assert x[3] == pool_sig[(x[0], x[1])]


def test_share_tables_and_scalars_are_the_kernels():
    with open(os.path.join(CSRC, "ecc_device.h")) as f:
        assert int(re.search(r"kWideBits = (\d+);", f.read()).group(1)) == kv.COMB_WIDE
    with open(os.path.join(CSRC, "ecc_coop.hip")) as f:
        src = f.read()
    a, b, c = (int(v) for v in re.search(r"kTrioSplitWin\[3\] = \{(\d+), (\d+), (\d+)\};", src).groups())
    assert re.search(r"return \{\{\{0, a\}, \{a, b\}, \{c, 16\}, \{b, c\}\}, "
                     r"\{\{0, 2 \* a\}, \{2 \* a, 2 \* b\}, \{2 \* c, 32\}, \{2 \* b, 2 \* c\}\}\};", src)
    assert rv.RECOVER_SHARE["trio"][16] == ((0, a), (a, b), (c, 16), (b, c))
    assert rv.RECOVER_SHARE["trio"][8] == ((0, 2 * a), (2 * a, 2 * b), (2 * c, 32), (2 * b, 2 * c))
    m = re.search(r"kPairShare\[4\]\[2\] = ([^;]*);", src)
    assert tuple((int(x), int(y)) for x, y in re.findall(r"\{(\d+), (\d+)\}", m.group(1))) == rv.RECOVER_SHARE["pair"][8]
    w0, w1 = (int(v) for v in re.search(r"kCombW0 = (\d+), kCombW1 = (\d+);", src).groups())
    assert ((0, w0), (w1, 32), (0, 0), (w0, w1)) == rv.RECOVER_SHARE["pair"][8]  # waves 0, 1, -, 3
    assert "comb_mul<CurveK1, 8>(PG, u1, tab);" in src
    with open(os.path.join(CSRC, "ecc_row.hip")) as f:
        assert "const int lo = wave * (W / 4), hi = lo + W / 4;" in f.read()
    for body, cuts in rv.SHARE_BITS.items():  # the bit ranges are the window ranges of both layouts, and tile
        for bits, share in rv.RECOVER_SHARE[body].items():
            assert sorted((x * bits, y * bits) for x, y in share if x != y) == list(cuts), (body, bits)
        assert cuts[0][0] == 0 and cuts[-1][1] == 256 and all(x[1] == y[0] for x, y in zip(cuts, cuts[1:]))
    assert kv.GLV_EDGES == glv.EDGES[1:] and kv.GLV_FOUND == glv.FOUND and kv.GLV_SMALL == glv.SMALL


def test_x_r(rows):
    got = _labelled(rows, "x_r")
    gap = P - N
    # the curve's x values the rows stand on, on integers
    assert kv.lift_x(N) is not None and kv.lift_x(1) is not None and kv.lift_x(P - 3) is not None
    assert kv.lift_x(0) is None and kv.lift_x(N - 1) is None and kv.lift_x(N - 2) is not None
    assert kv.lift_x(P - 1) is None and kv.lift_x(P - 2) is None and kv.lift_x(N + 1) is None
    want = {"r=0,v=2": (0, 2), "r=0,v=3": (0, 3), "r=1,v=0": (1, 0), "r=1,v=1": (1, 1), "r=1+p-n,v=2": (1 + gap, 2),
            "r=1+p-n,v=3": (1 + gap, 3), "r=1,v=2": (1, 2), "r=p-3-n,v=2": (gap - 3, 2), "r=p-3-n,v=3": (gap - 3, 3),
            "r=p-3,v=0": (P - 3, 0), "r=p-3-n,v=0": (gap - 3, 0), "r=p-n-1,v=2": (gap - 1, 2), "r=p-n,v=2": (gap, 2),
            "r=2,v=2": (2, 2), "r=2,v=3": (2, 3), "r=n+2,v=0": (N + 2, 0), "r=n-2,v=0": (N - 2, 0),
            "r=n-2,v=1": (N - 2, 1), "r=n-1,v=0": (N - 1, 0), "r=n,v=0": (N, 0)}
    for label, (r, v) in want.items():
        assert rv.rsv_of(got[label])[0::2] == (r, v), label
    assert all(0 < rv.rsv_of(x)[1] < N for x in got.values())  # s decides nothing here
    accepted = {l for l, x in got.items() if x[4] is not None}
    assert accepted == {"r=1,v=0", "r=1,v=1", "r=p-3-n,v=2", "r=p-3-n,v=3", "r=p-3-n,v=0", "r=2,v=2", "r=2,v=3",
                        "r=n-2,v=0", "r=n-2,v=1", "r=mid-n,v=2", "r=mid-n,v=3"}
    # only one comparison rejects: with it dropped the row names a curve point
    assert kv.lift_x((0 + N) % P) and kv.lift_x((1 + gap + N) % P) == kv.lift_x(1) and 1 + gap < N
    assert kv.lift_x(N % P) is not None and N + 2 < P and gap - 1 + N == P - 1
    # both parities of y give two keys, opposite only when u1 = 0
    for a, b in (("r=1,v=0", "r=1,v=1"), ("r=p-3-n,v=2", "r=p-3-n,v=3"), ("r=2,v=2", "r=2,v=3"), ("r=n-2,v=0", "r=n-2,v=1")):
        assert rv.point_of(got[a]) == kv.neg(rv.point_of(got[b])) and got[a][4] != got[b][4]
    x = rv.point_of(got["r=mid-n,v=2"])[0]
    assert N + 2**100 < x < P - 2**100
    # the seats of the trio kernel's pair inversion in a launch from row 0: the r = 0 rows beside accepted rows
    assert [x[1] for x in rows[:2]] == ["r=0,v=2", "r=0,v=3"]
    assert rows[20][0] == rows[21][0] == "x_r" and rows[20][4] is not None and rows[21][4] is not None


def test_s_edge(rows):
    got = _labelled(rows, "s_edge")
    half = (N - 1) // 2
    want = {"s=1": 1, "s=2": 2, "s=(n-1)/2": half, "s=(n+1)/2": half + 1, "s=n-1": N - 1, "s=n": N, "s=n+1": N + 1,
            "s=0": 0, "s=2^256-1": 2**256 - 1}
    assert {l: rv.rsv_of(x)[1] for l, x in got.items()} == want
    assert all((x[4] is not None) == (0 < rv.rsv_of(x)[1] < N) for x in got.values())
    for twin, label in (("s=1", "s=0"), ("s=1", "s=n+1"), ("s=n-1", "s=n"), ("s=2", "s=2^256-1")):
        assert got[twin][2] == got[label][2] and got[twin][3][:32] == got[label][3][:32] and got[twin][3][64] == got[label][3][64]
    assert sum(1 for x in got.values() if x[4] is not None and rv.rsv_of(x)[1] > half) == 2  # high s accepted


def test_e_rep(rows):
    got = _labelled(rows, "e_rep")
    top = 2 * N - 2**256
    want = {"h=0": 0, "h=n": N, "h=n-1": N - 1, "h=n+1": N + 1, "h=2n-2^256-1": top - 1, "h=2n-2^256": top,
            "h=2n-2^256+1": top + 1, "h=2^256-1": 2**256 - 1}
    assert all(rv.h_of(got[l]) == h for l, h in want.items())
    assert rv.u1_of(got["h=0"]) == 0 == rv.u1_of(got["h=n"]) and rv.summands(got["h=n"])[0] is None
    a, b = got["e"], got["e+n"]
    assert rv.h_of(a) < N <= rv.h_of(b) == rv.h_of(a) + N and a[3] == b[3] and a[4] == b[4]
    assert sum(1 for x in got.values() if rv.h_of(x) >= N) == 4


def test_final_add(rows, tx_rows):
    points = {"R=G": kv.G, "R=-G": kv.neg(kv.G), "R=lambdaG": kv.mul(kv.LAMBDA)}
    for pool in (rows, tx_rows):
        got = _labelled(pool, "final_add")
        assert len(got) == 10
        for label, x in got.items():
            A, B = rv.summands(x)
            assert A is not None and B is not None
            kind, where = label.split(":")
            if where.split(",")[0] in points:
                assert rv.point_of(x) == points[where.split(",")[0]]
            if kind == "inf":
                assert A == kv.neg(B) and x[4] is None
            elif where.endswith(",s+1"):
                twin = got[label[:-4]]
                assert A != B and A != kv.neg(B) and x[4] not in (None, twin[4]) and x[3][0:32] == twin[3][0:32]
                if pool is rows:  # (a transaction row stands over its own hash: s = -e / k + 1 for that e)
                    assert x[2] == twin[2] and rv.rsv_of(x)[1] == rv.rsv_of(twin)[1] + 1
                assert kv.mul(rv.u2_of(x) - pow(rv.rsv_of(x)[0], -1, N), rv.point_of(x)) == A  # (s - 1) / r R = u1 G
            else:
                assert A == B and x[4] == kv.add(A, A)
    # R = G: u1 = u2, e = -s
    x = _labelled(rows, "final_add")["dbl:R=G"]
    assert (rv.h_of(x) + rv.rsv_of(x)[1]) % N == 0


def test_u2_shape(rows):
    got = {x[1]: rv.u2_of(x) for x in _of(rows, "u2_shape")}
    assert [got["edge%d" % i] for i in range(13)] == glv.EDGES[1:]
    assert [got["found%d" % i] for i in range(4)] == glv.FOUND and [got["small%d" % i] for i in range(20)] == glv.SMALL
    for label, want in list(kv.GLV_HALVES.items()) + list(rv.ROW_QUARTERS.items()):
        assert split(got[label]) == want, label  # halves this short are the cell's own
    for label in ("low++", "low-+"):
        k1, k2 = split(got[label])
        assert 0 < abs(k1) < 2**123 and 0 < abs(k2) < 2**123
    assert all(split(got["small%d" % i])[1 - (i % 4) // 2] == 0 for i in range(20))  # c: k2 = 0; c lambda: k1 = 0
    # the row kernel's chains: lo(k1), lo(k2), hi(k1), hi(k2)
    quarters = lambda u: tuple(bool(v) for k in split(u) for v in (abs(k) & (2**64 - 1), abs(k) >> 64))
    assert {l: quarters(got[l]) for l in rv.ROW_QUARTERS} == {
        "q:lo1": (True, False, False, False), "q:hi1": (False, True, False, False), "q:lo2": (False, False, True, False),
        "q:hi2": (False, False, False, True), "q:lo1+lo2": (True, False, True, False), "q:hi1+hi2": (False, True, False, True)}
    assert len(got) == rv.COUNTS["u2_shape"]


def test_u1_shape(rows):
    got = {x[1][3:]: rv.u1_of(x) for x in _of(rows, "u1_shape")}
    for body, cuts in rv.SHARE_BITS.items():
        for bits, share in rv.RECOVER_SHARE[body].items():
            # the waves with a nonzero part, and wave j's windows all nonzero where the row fills them
            order = sorted((w for w in range(len(share)) if share[w][0] != share[w][1]), key=lambda w: share[w][0])
            nz = lambda u: [w for w, v in enumerate(rv.share_parts(u, body, bits)) if v]
            for j, w in enumerate(order):
                assert nz(got["%s:only%d" % (body, j)]) == [w], (body, bits, j)
                assert nz(got["%s:zero%d" % (body, j)]) == sorted(v for v in order if v != w), (body, bits, j)
                win = kv.comb_windows(got["%s:only%d" % (body, j)], bits)
                assert all(win[i] for i in range(*share[w])) and sum(1 for v in win if v) == share[w][1] - share[w][0]
            assert nz(got["n-1"]) == sorted(order) and nz(got["1"]) == order[:1] == nz(got["lowest"])
            assert nz(got["highest/8"]) == order[-1:] == nz(got["highest/16"])
    for bits in (16, 8):
        w = kv.comb_windows(got["lowest"], bits)
        assert w[0] and not any(w[1:])
        assert [i for i, v in enumerate(kv.comb_windows(got["highest/%d" % bits], bits)) if v] == [256 // bits - 1]
        assert rv.share_parts(got["lowest"], "whole", bits) == [got["lowest"]]
    assert kv.comb_windows(got["highest/16"], 8)[31] == 0  # the 16-bit comb's top window, not the 8-bit comb's
    assert got["1"] == 1 and got["n-1"] == N - 1
    assert kv.comb_windows(got["max-windows"], 16).count(0xFFFF) == 15 and got["max-windows"] < N
    assert len(got) == rv.COUNTS["u1_shape"] and all(0 < u < N for u in got.values())


def test_key_out(rows):
    got = _labelled(rows, "key_out")
    xc = got["y=1"][4][0]
    want = {"x=1": kv.lift_x(1, 0), "x=1,-y": kv.lift_x(1, 1), "x=2": kv.lift_x(2, 0), "x=3": kv.lift_x(3, 1), "G": kv.G,
            "-G": kv.neg(kv.G), "2G": kv.mul(2), "lambdaG": kv.mul(kv.LAMBDA), "x=p-3": kv.lift_x(P - 3, 0), "y=1": (xc, 1),
            "y=p-1": (xc, P - 1)}
    assert {l: x[4] for l, x in got.items()} == want and all(kv.on_curve(q) for q in want.values())
    assert sum(1 for q in want.values() if rv.pub_bytes(q)[:31] == bytes(31)) == 4  # leading zero bytes in x
    assert rv.pub_bytes(want["y=1"])[32:63] == bytes(31) and rv.pub_bytes(want["y=p-1"])[32:59] == b"\xff" * 27
    for x in got.values():  # ordinary final additions: the key is the point of the row, not the path to it
        A, B = rv.summands(x)
        assert A is not None and B is not None and A != B and A != kv.neg(B)


def test_reject(rows, tx_rows):
    by = {x[1]: x for x in rows if x[0] != "reject"}
    kinds = set()
    for x in _of(rows, "reject"):
        kind, twin = x[1].split(":", 1)
        a = by[twin]
        assert a[4] is not None and x[4] is None and a[2] == x[2]
        assert [a[3][0:32] == x[3][0:32], a[3][32:64] == x[3][32:64], a[3][64] == x[3][64]].count(False) == 1, x[1]
        kinds.add(kind.split("=")[0])
    assert kinds == {"v", "r", "s"}
    assert all(x[3][64] > 3 for x in _of(tx_rows, "reject"))


# ------------------------------------------------------------------ no intermediate addition meets P = +-Q
def _lattice(span=3):
    """The vectors (x, y) != 0 with x + y lambda = 0 mod n, from the split's basis (A1, -MB1), (A2, A1)."""
    out = []
    for i in range(-span, span + 1):
        for j in range(-span, span + 1):
            if (i, j) != (0, 0):
                x, y = i * A1 + j * A2, -i * MB1 + j * A1
                assert (x + y * kv.LAMBDA) % N == 0
                out.append((x, y))
    return out


K1_MAX = (A1 + A2 + 2) // 2  # the split's halves: |k1| < (a1 + a2 + 2) / 2, |k2| < (-b1 + b2) / 2 + 1, the bounds
K2_MAX = (MB1 + A1) // 2 + 1   # libsecp256k1 proves for secp256k1_scalar_split_lambda (its rounding included)


def test_no_lattice_vector_is_in_range(rows):
    """Two partials a R' + b phi(R') and a' R' + b' phi(R') of one recovery are equal or opposite iff
    (a -+ a', b -+ b') is a nonzero vector of the split's lattice.  Where the operands are the two whole chains
    (trio, pair, coop, split: k1 R' = +-k2 phi(R')) that vector is (|k1|, |k2|) up to signs; in the one-lane
    bodies' joint chain the accumulator (16 a, 16 b), Booth prefixes of the halves, meets a digit |d| <= 8 of
    either half, and a prefix is at most its half plus 8.  So the vector's entries are within 16 of the halves'
    bounds, and the lattice has no nonzero vector there: the nearest, +-(A1, -MB1) and +-(A2, A1), each have an
    entry beyond."""
    reach = lambda span: [v for v in _lattice(span) if abs(v[0]) <= K1_MAX + 16 and abs(v[1]) <= K2_MAX + 16]
    assert reach(3) == [] and reach(8) == []
    assert MB1 > K2_MAX + 16 and A2 > K1_MAX + 16 and A1 < K1_MAX  # which entry it is
    # the bounds, on the rows whose u2 is the point, the split's found worst cases among them
    for x in _of(rows, "u2_shape") + _of(rows, "key_out"):
        k1, k2 = split(rv.u2_of(x))
        assert abs(k1) < K1_MAX and abs(k2) < K2_MAX, x[:2]
    assert max(abs(split(u)[1]) for u in glv.FOUND) > K2_MAX - 2**116  # (they sit at the bound)


def test_row_kernel_halves_never_coincide():
    """recover_row_kernel: c0 + c1 and c2 + c3 are lo(k1) R' + lo(k2) phi(R') and its twin on 2^64 R', entries below
    2^64: no lattice vector.  (c0 + c1) + (c2 + c3): equal needs (s1 (lo1 - 2^64 hi1), s2 (lo2 - 2^64 hi2)) in the
    lattice (opposite needs u2 = 0); an entry -d names its half (lo < 2^64: hi = ceil(d / 2^64), lo = 2^64 hi - d),
    which is d + 2 lo >= d, and for every vector in range one of the two halves so named is beyond the split's
    bound."""
    seen = 0
    for x, y in _lattice():
        if not (abs(x) < 2**128 and abs(y) < 2**128):
            continue
        halves = []
        for d in (abs(x), abs(y)):
            hi = -(-d // 2**64)
            halves.append(2**64 * hi + (2**64 * hi - d))
            assert halves[-1] >= d and (halves[-1] & (2**64 - 1)) - 2**64 * (halves[-1] >> 64) == -d
        assert halves[0] >= K1_MAX or halves[1] >= K2_MAX, (x, y)
        seen += 1
    assert seen == 2  # +-(A1, -MB1)
    assert not [v for v in _lattice() if abs(v[0]) < 2**64 and abs(v[1]) < 2**64]


# ------------------------------------------------------------------ the rows catch what they are named after
def _inv(x):
    """x^-1 mod n as a kernel's inversion leaves it: 0 for 0."""
    return pow(x, N - 2, N)


def _restated(h32, r, s, v, guard=True, add_n=True, parity=True, r_min=1, reduce_e=True, inf_ok=False, dbl_inf=False,
              s_min=1, s_max=N - 1, u1_sign=-1, rinv=None):
    """The kernels' decisions as they take them, each of which a flag gets wrong.  guard=False: x = r + n mod p with
    no r < p - n.  add_n=False: x = r under v & 2.  parity=False: the square root as it comes.  r_min=0: r = 0
    passes.  reduce_e=False: u1 = (n - hash mod 2^256) / r, the negation of an unreduced word.  inf_ok: the
    infinity flag is not read (X = Y = 0 comes out).  dbl_inf: the final addition's equal operands give infinity.
    rinv: r^-1 as the pair inversion hands it over."""
    if v > 3 or not (r_min <= r < N and s_min <= s <= s_max):
        return None
    x = r
    if v & 2:
        if guard and r >= P - N:
            return None
        if add_n:
            x = (r + N) % P
    R = kv.lift_x(x, v & 1)
    if R is None:
        return None
    if not parity:
        y = pow((x**3 + 7) % P, (P + 1) // 4, P)
        R = (x, y)
    e = int.from_bytes(h32, "big")
    w = _inv(r) if rinv is None else rinv
    u1 = (u1_sign * (e - N if e >= N else e) * w) % N if reduce_e else ((N - e) % 2**256) * w % N
    A, B = kv.mul(u1), kv.mul(s % N * w % N, R)
    Q = None if dbl_inf and A == B and A is not None else kv.add(A, B)
    if Q is None:
        return (0, 0) if inf_ok else None
    return Q


MUTANTS = {"1 no r < p - n guard": ("x_r", dict(guard=False)),
           "2 x = r for v & 2": ("x_r", dict(add_n=False)),
           "3 parity ignored": ("x_r", dict(parity=False)),
           "5 e not reduced": ("e_rep", dict(reduce_e=False)),
           "6 infinity accepted": ("final_add", dict(inf_ok=True)),
           "7 a doubling returned as infinity": ("final_add", dict(dbl_inf=True)),
           "8 high s rejected": ("s_edge", dict(s_max=(N - 1) // 2)),
           "9 s = 0 accepted": ("s_edge", dict(s_min=0)),
           "9 s = 1 rejected": ("s_edge", dict(s_min=2)),
           "9 s = n accepted": ("s_edge", dict(s_max=N)),
           "9 s = n - 1 rejected": ("s_edge", dict(s_max=N - 2)),
           "10 the sign of u1 dropped": ("u1_shape", dict(u1_sign=1))}


def _wrong(rows, keys):
    bad = {}
    for x, q in zip(rows, keys):
        if q != x[4]:
            bad.setdefault(x[0], []).append(x[1])
    return bad


def test_restated_decisions_equal_the_reference(rows, tx_rows):
    for x in rows + tx_rows:
        assert _restated(x[2], *rv.rsv_of(x)) == x[4], x[:2]


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_each_wrong_restatement_fails_a_row_of_its_class(rows, name):
    cls, flags = MUTANTS[name]
    wrong = _wrong(rows, [_restated(x[2], *rv.rsv_of(x), **flags) for x in rows])
    assert wrong.get(cls), (name, wrong)
    print(name, wrong)


def _pair_launch(rows, r_min):
    """A launch of the trio kernel from row 0 with r^-1 as its pair inversion gives it (pair_inv.h): txs t and t + 20
    of each 40 share one inversion of r_a r_b; a member that fails the range checks enters as r = 1.  r_min = 0
    is the wrong restatement 4: r = 0 passes, and zeroes its partner's inverse."""
    keys = []
    for i, x in enumerate(rows):
        j = i + 20 if i % 40 < 20 else i - 20
        rs = []
        for y in (x, rows[j] if j < len(rows) else None):
            r, s, v = rv.rsv_of(y) if y is not None else (1, 0, 0)
            rs.append(r if v <= 3 and r_min <= r < N and 0 < s < N else 1)
        rinv = _inv(rs[0] * rs[1]) * rs[1] % N
        keys.append(_restated(x[2], *rv.rsv_of(x), r_min=r_min, rinv=rinv))
    return keys


def test_r_zero_accepted_fails_a_row_of_its_class(rows):
    """Wrong restatement 4.  Alone, an r = 0 that passes the range check inverts to 0, so u1 = u2 = 0 and the row is
    still refused as infinity: its own verdict cannot show it.  What shows it is the trio kernel's pair
    inversion, where it zeroes the r^-1 of the row 20 places on: rows 20 and 21 of the pool are accepted x_r rows."""
    assert _wrong(rows, [_restated(x[2], *rv.rsv_of(x), r_min=0) for x in rows]) == {}
    assert _wrong(rows, _pair_launch(rows, 1)) == {}
    wrong = _wrong(rows, _pair_launch(rows, 0))
    assert wrong == {"x_r": [rows[20][1], rows[21][1]]}, wrong


def test_compare_reports_the_class_of_a_wrong_answer(rows):
    addr = lambda pub: hashlib.sha256(pub).digest()[12:]
    ok = [x[4] is not None for x in rows]
    pubs = [bytes(64) if x[4] is None else rv.pub_bytes(x[4]) for x in rows]
    addrs = [bytes(20) if x[4] is None else addr(rv.pub_bytes(x[4])) for x in rows]
    assert rv.compare(rows, ok, pubs, addrs, addr) == {} and rv.compare(rows, ok, pubs) == {}
    for cls in rv.CLASSES:
        i = next(i for i, x in enumerate(rows) if x[0] == cls)
        flipped = list(ok)
        flipped[i] = not flipped[i]
        assert rv.compare(rows, flipped, pubs, addrs, addr) == {cls: [rows[i][1]]}
        other = list(pubs)
        other[i] = bytes([other[i][0] ^ 1]) + other[i][1:]
        assert rv.compare(rows, ok, other, addrs, addr) == {cls: [rows[i][1]]}
        other = list(addrs)
        other[i] = other[i][:19] + bytes([other[i][19] ^ 0x80])
        assert rv.compare(rows, ok, pubs, other, addr) == {cls: [rows[i][1]]}
    with pytest.raises(AssertionError):
        rv.compare(rows, ok[:-1], pubs)


def test_ecrecover_input_round_trips(rows, oracle):
    for x in rows:
        d = rv.ecrecover_input(x)
        assert len(d) == 128 and d[0:32] == x[2] and d[64:128] == x[3][0:64] and (d[63] - 27) & 0xFF == x[3][64]
        want = b"" if x[4] is None else bytes(12) + oracle.keccak256(rv.pub_bytes(x[4]))[12:]
        assert oracle.ecrecover(d) == want, x[:2]
