"""secp256k1 public-key recovery rows at the edges no signer produces, and their reference.

Seven device bodies recover a key (trio26_recover_body, coop26_body, recover_row_kernel, tx_verify_coop_kernel,
tx_verify_split_kernel, secp256k1_recover_lane26, secp256k1_recover_lane), each writing out the same decisions:
v <= 3, r and s in [1, n - 1], (v & 2) => r < p - n and x = r + n, y = sqrt(x^3 + 7) with the parity of v & 1,
e = hash reduced once, Q = (-e / r) G + (s / r) R, Q not infinity.  Over SigIO and EcrecIO the digest, r, s and v
are free inputs, so every row below is reached by integer arithmetic alone, on the shipped library, through two
exact constructions:

  at a point   any curve point R and any u1, u2: r = x(R) (or x(R) - n with v |= 2 where x(R) >= n), s = u2 r,
               e = -u1 r, hash = e (or e + n where that fits 32 bytes); with R = k G the key is (u1 + u2 k) G;
  at a key     any target Q and any u1, u2: R = u2^-1 (Q - u1 G), then r, s, e as above.

The reference is recover(h32, r, s, v) -> (x, y) | None: oracle_secp256k1_recover's steps (oracle/ec.c) over
the affine points and Python integers of tests/k1_verify_vectors.py; tests/test_k1_recover_vectors.py pins it to
the oracle on every row.  The signature of an x_r, s_edge or u2_shape row does not depend on e, so sig_specs()
gives those rows' (r, s, v) for tx_rows() to rebuild over the hashes of fixed transactions (TxIO: the digest is
the transaction's hash and only r, s, v are free), with the final_add rows that a fixed e allows.

pool() returns the rows (class, label, h32, sig65, expected key (x, y) or None), built once; COUNTS states the
rows per class.  No GPU, no compiler, no numpy.

The summing order of each body -- every addition of two partials, and whether its operands can be equal or
opposite while the total stays finite.  Notation: u1 = sum of g_j, the comb windows of one share; u2 = k1 + k2
lambda, the split's signed halves; R' the image of R on the chains' curve; T = u1 G; S = u2 R.

  trio26_recover_body (ecc_coop.hip)
    g0 + g1, (g0 + g1) + g3   trio_recover_helper, CurveK1x::add (helper 2 has no windows): multiples of G on
                              disjoint windows, a G + b G with 0 <= a, b and a + b <= u1 < n: equal only for
                              a = b = 0 (both infinite), never opposite.  Infinite operands: u1_shape trio:*.
    k1 R' + k2 phi(R')        trio_add, phase D: equal or opposite needs k1 -+ k2 lambda = 0 mod n, a nonzero
                              vector of the split's lattice with both entries in range of the halves: none
                              (test_no_lattice_vector_is_in_range).  One half zero: u2_shape small*, k1=0, k2=0.
    T + S                     trio_add / trio_add_z: the total.  final_add dbl:* and inf:*.
  coop26_body (ecc_coop.hip)
    g0 + g3 (coop26_store_partial), (g0 + g3) + g1, k1 R' + k2 phi(R'), S + T: as above on kPairShare;
    u1_shape pair:*, final_add.
  tx_verify_coop_kernel (ecc_coop.hip, TxIO only)
    (g0 + g3) + g1 on wave 1, k1 R' + k2 phi(R'), S + T: as coop26_body, on the same windows.
  tx_verify_split_kernel (ecc_coop.hip, TxIO only)
    u1 G is one comb_mul on wave 2 (window i's entry added to the sum of the windows below it: a G + b G with
    a < 2^(8 i) <= b, a + b < n: never equal or opposite); k1 R + k2 phi(R); S + T.
  recover_row_kernel (ecc_row.hip), four 64-bit chains c0 = lo(k1) R', c1 = lo(k2) phi(R'), c2 = hi(k1) 2^64 R',
  c3 = hi(k2) phi(2^64 R') and four comb quarters
    c0 + c1, c2 + c3          lattice vectors with entries below 2^64: none.  Infinite operands: u2_shape q:*.
    (c0 + c1) + (c2 + c3)     opposite needs u2 = 0; equal needs (lo1 - 2^64 hi1, lo2 - 2^64 hi2) in the lattice
                              up to the halves' signs, which no output of the split gives
                              (test_row_kernel_halves_never_coincide).
    g0 + g1, g2 + g3, their sum: disjoint windows, as above.  u1_shape row:*.
    S + T                     the total.
  secp256k1_recover_lane26 (recover26.h), secp256k1_recover_lane (ecc_device.h)
    one joint Booth chain over both halves (glv_mul_k1_26 / glv_mul_k1: the accumulator a R' + b phi(R') meets
    d R' or d phi(R'), |d| <= 8: equal or opposite is again a lattice vector in range), one comb from the lowest
    window up (comb_mul, as the split kernel's), then QG + QR: the total.

So in every body the G part and the R part are summed apart and meet in the last addition: the total's doubling
and infinity (final_add) are the only equal or opposite operands any input reaches, and what the bodies do not
share is which partials are infinite: the u1_shape and u2_shape rows."""
import functools
import random

from k1_verify_vectors import (COMB_SMALL, COMB_WIDE, G, GLV_EDGES, GLV_FOUND, GLV_HALVES, GLV_SMALL, LAMBDA, N, P, add,
                               comb_windows, lift_x, mul, neg, on_curve)

GAP = P - N

# The comb windows [a, b) of u1 G that each wave (helper) takes, per body, on the 16-bit comb (kWideBits) and the
# 8-bit one.  The CPU test has nothing to compare these with but the source:
#   trio   kTrioSplitWin = {5, 10, 16} -> kTrioRecoverShare, by helper 0, 1, 2, 3   ecc_coop.hip:1374-1382
#   pair   kPairShare, by wave (coop26_body)                                        ecc_coop.hip:1369
#          kCombW0 = 12, kCombW1 = 24: waves 0, 3, 1 (tx_verify_coop_kernel)        ecc_coop.hip:645-648
#   row    lo = wave * (W / 4), hi = lo + W / 4 (recover_row_kernel)                ecc_row.hip:299-301
#   whole  comb_mul<CurveK1, 8> on wave 2 (tx_verify_split_kernel)                  ecc_coop.hip:198
#          comb_mul_rt / comb_mul26_rt (the one-lane bodies)                        ecc_device.h:195, recover26.h:276
RECOVER_SHARE = {
    "trio": {COMB_WIDE: ((0, 5), (5, 10), (16, 16), (10, 16)), COMB_SMALL: ((0, 10), (10, 20), (32, 32), (20, 32))},
    "pair": {COMB_SMALL: ((0, 12), (24, 32), (0, 0), (12, 24))},
    "row": {COMB_WIDE: ((0, 4), (4, 8), (8, 12), (12, 16)), COMB_SMALL: ((0, 8), (8, 16), (16, 24), (24, 32))},
    "whole": {COMB_WIDE: ((0, 16),), COMB_SMALL: ((0, 32),)},
}
# the same shares as bit ranges of u1, lowest first (the wide and narrow layouts of a body cut at the same bits)
SHARE_BITS = {"trio": ((0, 80), (80, 160), (160, 256)), "pair": ((0, 96), (96, 192), (192, 256)),
              "row": ((0, 64), (64, 128), (128, 192), (192, 256))}

# the row kernel's four 64-bit chains: signed halves (k1, k2) with whole quarters zero
ROW_QUARTERS = {"q:lo1": (0xB504F333F9DE6485, 0), "q:hi1": (-(0x9E3779B97F4A7C << 64), 0),
                "q:lo2": (0, -0xC6A4A7935BD1E995), "q:hi2": (0, 0x2545F4914F6CDD << 64),
                "q:lo1+lo2": (0xD1B54A32D192ED03, 0x8CB92BA72F3D8DD7), "q:hi1+hi2": (0x6A09E667F3BCC9 << 64, -(0x3C6EF372FE94F8 << 64))}

CLASSES = ("x_r", "s_edge", "e_rep", "final_add", "u2_shape", "u1_shape", "key_out", "reject")
COUNTS = {"x_r": 22, "s_edge": 9, "e_rep": 10, "final_add": 10, "u2_shape": 49, "u1_shape": 26, "key_out": 11,
          "reject": 16}
TX_COUNTS = {"x_r": 22, "s_edge": 9, "final_add": 10, "u2_shape": 49, "reject": 8}
LAUNCH_MIN = 21  # every run of this many rows of the pool (and of tx_rows) holds both verdicts
CASES_LEFT_OUT = 0  # every search below is bounded and raises when it fails; no row is skipped at run time


def recover(h32, r, s, v):
    """oracle_secp256k1_recover's steps: v <= 3, r and s in [1, n - 1], (v & 2) => r < p - n and x = r + n, y from
    x^3 + 7 with the parity of v & 1, e = hash reduced once, Q = (-e / r) G + (s / r) R, Q not infinity."""
    if v > 3 or not (0 < r < N and 0 < s < N):
        return None
    x = r
    if v & 2:
        if r >= GAP:
            return None
        x = r + N
    R = lift_x(x, v & 1)
    if R is None:
        return None
    e = int.from_bytes(h32, "big")
    if e >= N:
        e -= N  # once is enough: 2^256 < 2 n
    w = pow(r, -1, N)
    return add(mul(-e * w % N), mul(s * w % N, R))


# ------------------------------------------------------------------ what the classes are named after
def h_of(row):
    return int.from_bytes(row[2], "big")


def rsv_of(row):
    sig = row[3]
    return int.from_bytes(sig[0:32], "big"), int.from_bytes(sig[32:64], "big"), sig[64]


def point_of(row):
    """R of a row whose r, v name a curve point (None otherwise; the range checks are not applied)."""
    r, _, v = rsv_of(row)
    return lift_x(r + N if v & 2 else r, v & 1)


def u1_of(row):
    r, _, _ = rsv_of(row)
    return -(h_of(row) % N) * pow(r, -1, N) % N


def u2_of(row):
    r, s, _ = rsv_of(row)
    return s * pow(r, -1, N) % N


def summands(row):
    """(u1 G, u2 R), the two points the final addition takes."""
    return mul(u1_of(row)), mul(u2_of(row), point_of(row))


def share_parts(u, body, bits):
    """The part of u each wave (helper) of `body` puts through the comb of `bits`-bit windows; their sum is u."""
    w = comb_windows(u, bits)
    out = [sum(w[i] << (bits * i) for i in range(a, b)) for a, b in RECOVER_SHARE[body][bits]]
    assert sum(out) == u
    return out


def pub_bytes(pt):
    return pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")


# ------------------------------------------------------------------ the rows
def _scalar(rnd):
    return rnd.randrange(2**200, N)


def _rv(R):
    """(r, v) that name the curve point R."""
    x, y = R
    return (x, y & 1) if x < N else (x - N, 2 | (y & 1))


def _sig(r, s, v):
    return r.to_bytes(32, "big") + s.to_bytes(32, "big") + bytes([v])


def _row(cls, label, h, r, s, v, intended=None):
    assert 0 <= h < 2**256 and 0 <= r < 2**256 and 0 <= s < 2**256 and 0 <= v < 256
    h32 = h.to_bytes(32, "big")
    got = recover(h32, r, s, v)
    assert got is None or on_curve(got)
    assert intended is None or (got is not None) == intended, (cls, label, got)
    return (cls, label, h32, _sig(r, s, v), got)


def _at_point(cls, label, R, u1, u2, intended=True):
    """The row whose recovery computes u1 G + u2 R."""
    r, v = _rv(R)
    x = _row(cls, label, -u1 * r % N, r, u2 * r % N, v, intended)
    assert x[4] == add(mul(u1), mul(u2, R))
    return x


def _at_key(cls, label, rnd, Q):
    """The accepted row whose recovered key is the given point: R = u2^-1 (Q - u1 G)."""
    u1, u2 = _scalar(rnd), _scalar(rnd)
    R = mul(pow(u2, -1, N), add(Q, neg(mul(u1))))
    x = _at_point(cls, label, R, u1, u2)
    assert x[4] == Q
    return x


def _first_x(start, step, tries=64):
    """The first curve x from `start` on in steps of `step`; a bounded search that raises."""
    for i in range(tries):
        if lift_x(start + i * step) is not None:
            return start + i * step
    raise AssertionError("no curve x within %d steps of %d" % (tries, start))


def _no_point_x(rnd, tries=64):
    for _ in range(tries):
        x = rnd.randrange(2**200, N)
        if lift_x(x) is None:
            return x
    raise AssertionError("no x without a curve point in %d draws" % tries)


def _fill(rnd, lo, hi):
    """A value on the bits [lo, hi) with every byte of them nonzero (and the top byte of 256 bits below 0xff, so
    the scalar stays below n)."""
    return sum(rnd.randrange(1, 0xFF) << b for b in range(lo, hi, 8))


@functools.lru_cache(maxsize=None)
def sig_specs():
    """(class, label, r, s, v, intended verdict or None) of the x_r, s_edge and u2_shape rows, none of which depends
    on e.  intended None: whatever the reference says (the row stands beside a twin that is the point)."""
    rnd = random.Random(0x6B32)
    out = []
    # -------- x_r: x(R) and the range guard where only one comparison decides.  The facts on integers:
    assert lift_x(N) is not None and lift_x(1) is not None and lift_x(P - 3) is not None and lift_x(N - 2) is not None
    assert lift_x(0) is None and lift_x(N - 1) is None and lift_x(P - 1) is None and lift_x(P - 2) is None
    assert lift_x(N + 1) is None and lift_x(N + 2) is not None
    xm = _first_x((N + P) // 2, 1)
    x_r = [("r=0,v=2", 0, 2, False),              # x = n is a curve x: only r != 0 rejects
           ("r=0,v=3", 0, 3, False),
           ("r=1,v=0", 1, 0, True), ("r=1,v=1", 1, 1, True),
           ("r=1+p-n,v=2", 1 + GAP, 2, False),    # r + n = 1 mod p, a curve x: only r < p - n rejects
           ("r=1+p-n,v=3", 1 + GAP, 3, False),
           ("r=1,v=2", 1, 2, None),
           ("r=p-3-n,v=2", GAP - 3, 2, True), ("r=p-3-n,v=3", GAP - 3, 3, True),  # x = p - 3, the largest curve x
           ("r=p-3,v=0", P - 3, 0, False),        # that x as r itself: only r < n rejects
           ("r=p-3-n,v=0", GAP - 3, 0, None),
           ("r=p-n-1,v=2", GAP - 1, 2, False),    # the last r the guard passes: x = p - 1 has no point
           ("r=p-n,v=2", GAP, 2, False),          # r + n = p
           ("r=2,v=2", 2, 2, True), ("r=2,v=3", 2, 3, True),  # x = n + 2, the first curve x above n
           ("r=n+2,v=0", N + 2, 0, False),        # that x as r itself
           ("r=n-2,v=0", N - 2, 0, True), ("r=n-2,v=1", N - 2, 1, True),  # the largest curve x below n
           ("r=n-1,v=0", N - 1, 0, False),        # in range, no point
           ("r=n,v=0", N, 0, False),              # a curve x: only r < n rejects
           ("r=mid-n,v=2", xm - N, 2, True), ("r=mid-n,v=3", xm - N, 3, True)]
    for label, r, v, intended in x_r:
        out.append(("x_r", label, r, _scalar(rnd), v, intended))
    # -------- s_edge: high s is accepted in recovery; each end of [1, n - 1] and its neighbour outside
    half = (N - 1) // 2
    edge = {}
    for label, s in (("s=1", 1), ("s=2", 2), ("s=(n-1)/2", half), ("s=(n+1)/2", half + 1), ("s=n-1", N - 1)):
        r, v = _rv(mul(_scalar(rnd)))
        edge[label] = ("s_edge", label, r, s, v, True)
    again = lambda a, label, s: ("s_edge", label, a[2], s, a[4], False)
    out += [edge["s=1"], again(edge["s=1"], "s=0", 0), again(edge["s=1"], "s=n+1", N + 1), edge["s=2"],
            edge["s=(n-1)/2"], edge["s=(n+1)/2"], edge["s=n-1"], again(edge["s=n-1"], "s=n", N),
            again(edge["s=2"], "s=2^256-1", 2**256 - 1)]
    # -------- u2_shape: the GLV halves of u2 = s / r, and the row kernel's quarters of them
    u2s = [("edge%d" % i, v) for i, v in enumerate(GLV_EDGES)] + [("found%d" % i, v) for i, v in enumerate(GLV_FOUND)]
    u2s += [("small%d" % i, v) for i, v in enumerate(GLV_SMALL)]
    u2s += [(label, (k1 + k2 * LAMBDA) % N) for label, (k1, k2) in list(GLV_HALVES.items()) + list(ROW_QUARTERS.items())]
    for label, u2 in u2s:
        r, v = _rv(mul(_scalar(rnd)))
        out.append(("u2_shape", label, r, u2 * r % N, v, True))
    return tuple(out)


def _final_add_plan(rnd):
    """(label, k, sign, plus) of the final_add rows over R = k G: e = sign s k, presented with s + plus.  sign -1:
    u1 G = u2 R, the total is a doubling (plus 1: its neighbour, an ordinary addition); sign 1: u1 G = -u2 R."""
    ks = (("k", _scalar(rnd)), ("R=G", 1), ("R=-G", N - 1), ("R=lambdaG", LAMBDA))
    out = []
    for label, k in ks:
        out += [("dbl:" + label, k, -1, 0), ("dbl:" + label + ",s+1", k, -1, 1)]
    return out + [("inf:" + label, k, 1, 0) for label, k in ks[:2]]


def _thread(rows, spare, run=9):
    """rows, with one of `spare` (rejected rows) put in wherever `run` accepted rows would stand in line; the rest
    of `spare` at the end."""
    out, spare, line = [], list(spare), 0
    for x in rows:
        if x[4] is not None and line == run and spare:
            out.append(spare.pop(0))
            line = 0
        out.append(x)
        line = line + 1 if x[4] is not None else 0
    return out + spare


def _check_runs(rows):
    for i in range(len(rows) - LAUNCH_MIN + 1):
        assert len({x[4] is None for x in rows[i:i + LAUNCH_MIN]}) == 2, i


@functools.lru_cache(maxsize=None)
def pool():
    rnd = random.Random(0x6B33)
    rows = []
    specs = sig_specs()
    by_cls = lambda cls: [x for x in specs if x[0] == cls]
    h_by = {}  # an s_edge row and its twins (the same r, v) stand over one hash

    def put(x):
        h = h_by.setdefault(x[1:3] if x[0] != "s_edge" else (x[2], x[4]), rnd.randrange(2**256))
        rows.append(_row(x[0], x[1], h, x[2], x[3], x[4], x[5]))

    # x_r comes first and whole, so that in a launch from row 0 the two r = 0 rows (places 0, 1) share a seat of the
    # trio kernel's pair inversion with the accepted rows at places 20, 21 (pair_inv.h: txs t and t + 20)
    for x in by_cls("x_r") + by_cls("s_edge"):
        put(x)

    # -------- e_rep: hashes at the ends of [0, n) and [n, 2^256), and one signature under e and under e + n
    top = 2 * N - 2**256  # the reduced value of the largest hash, plus one
    for label, h in (("h=0", 0), ("h=n", N), ("h=n-1", N - 1), ("h=n+1", N + 1), ("h=2n-2^256-1", top - 1),
                     ("h=2n-2^256", top), ("h=2n-2^256+1", top + 1), ("h=2^256-1", 2**256 - 1)):
        r, v = _rv(mul(_scalar(rnd)))
        rows.append(_row("e_rep", label, h, r, _scalar(rnd), v, True))
    r, v = _rv(mul(_scalar(rnd)))
    a = _row("e_rep", "e", rnd.randrange(2**100, 2**256 - N), r, _scalar(rnd), v, True)
    b = _row("e_rep", "e+n", h_of(a) + N, r, rsv_of(a)[1], v, True)
    assert a[4] == b[4]
    rows += [a, b]

    # -------- final_add: u1 G = u2 R (a doubling, beside its neighbour s + 1) and u1 G = -u2 R (infinity)
    for label, k, sign, plus in _final_add_plan(rnd):
        if not plus:
            s = _scalar(rnd)
        r, v = _rv(mul(k))
        rows.append(_row("final_add", label, sign * s * k % N, r, s + plus, v, sign < 0))

    for x in by_cls("u2_shape"):
        put(x)

    # -------- u1_shape: the comb shares of u1 = -e / r, per body
    u1s = []
    for body, cuts in SHARE_BITS.items():
        for j, (lo, hi) in enumerate(cuts):
            u1s.append(("%s:only%d" % (body, j), _fill(rnd, lo, hi)))
        for j in range(len(cuts)):
            u1s.append(("%s:zero%d" % (body, j), sum(_fill(rnd, lo, hi) for i, (lo, hi) in enumerate(cuts) if i != j)))
    u1s += [("lowest", 0xA5), ("highest/8", 0xC3 << 248), ("highest/16", 0x5A << 240), ("1", 1), ("n-1", N - 1),
            ("max-windows", 2**256 - 1 - (2 << 128))]
    for label, u1 in u1s:
        x = _at_point("u1_shape", "u1=" + label, mul(_scalar(rnd)), u1, _scalar(rnd))
        assert u1_of(x) == u1
        rows.append(x)

    # -------- key_out: the recovered key at chosen points (leading zero bytes, coordinates near p)
    xc = pow(-6 % P, (P + 2) // 9, P)  # p = 7 mod 9: the cube root of y^2 - 7 for y = 1
    assert pow(xc, 3, P) == -6 % P and on_curve((xc, 1))
    targets = [("x=1", lift_x(1, 0)), ("x=1,-y", lift_x(1, 1)), ("x=2", lift_x(2, 0)), ("x=3", lift_x(3, 1)), ("G", G),
               ("-G", neg(G)), ("2G", mul(2)), ("lambdaG", mul(LAMBDA)), ("x=p-3", lift_x(P - 3, 0)), ("y=1", (xc, 1)),
               ("y=p-1", (xc, P - 1))]
    for label, Q in targets:
        if Q is None:
            raise AssertionError("no curve point for key_out " + label)
        rows.append(_at_key("key_out", label, rnd, Q))

    # -------- reject: ordinary wrong rows, threaded through the long accepted stretches
    by = {(x[0], x[1]): x for x in rows}
    spare = []
    for (cls, label), v in ((("u2_shape", "edge0"), 4), (("u2_shape", "found0"), 5), (("u1_shape", "u1=1"), 27),
                            (("e_rep", "h=0"), 255), (("key_out", "G"), 128), (("final_add", "dbl:R=G"), 4)):
        a = by[(cls, label)]
        r, s, _ = rsv_of(a)
        spare.append(_row("reject", "v=%d:%s" % (v, label), h_of(a), r, s, v, False))
    for (cls, label), what, val in ((("u2_shape", "small0"), "r", 0), (("u2_shape", "small7"), "r", N),
                                    (("u2_shape", "k1=0"), "r", N + 5), (("u1_shape", "u1=n-1"), "r", 2**256 - 1),
                                    (("u2_shape", "q:lo1"), "s", 0), (("u1_shape", "u1=row:only0"), "s", N),
                                    (("key_out", "x=1"), "s", N + 1), (("u1_shape", "u1=pair:zero1"), "r", 5),
                                    (("u1_shape", "u1=trio:zero2"), "r", _no_point_x(rnd)),
                                    (("key_out", "y=1"), "r", _no_point_x(rnd))):
        a = by[(cls, label)]
        r, s, v = rsv_of(a)
        r, s = (val, s) if what == "r" else (r, val)
        spare.append(_row("reject", "%s=%s:%s" % (what, "no-point" if val > 5 and val < N else hex(val), label), h_of(a), r,
                          s, v, False))
    rows = _thread(rows, spare)

    got = {c: sum(1 for x in rows if x[0] == c) for c in CLASSES}
    assert got == COUNTS, got
    assert len({(x[0], x[1]) for x in rows}) == len(rows)
    assert [x[1] for x in rows[:2]] == ["r=0,v=2", "r=0,v=3"] and rows[20][4] is not None and rows[21][4] is not None
    assert rows[20][0] == rows[21][0] == "x_r"
    _check_runs(rows)
    return tuple(rows)


def tx_rows(hashes):
    """The x_r, s_edge and u2_shape signatures over the given transaction hashes (row j over hashes[j mod len]),
    with the final_add rows a fixed e allows (s = -e / k: the total doubles; s = e / k: infinity) and a v > 3 row
    before every sixth u2_shape row: the rows (class, label, h32, sig65, expected); row j belongs to transaction
    j mod len."""
    rnd = random.Random(0x6B34)
    specs = sig_specs()
    plan = [x for x in specs if x[0] != "u2_shape"] + [("final_add",) + x for x in _final_add_plan(rnd)]
    for i, x in enumerate(x for x in specs if x[0] == "u2_shape"):
        if i % 6 == 3:
            plan.append(("reject", "v=%d:%s" % (4 + i, x[1]), x[2], x[3], 4 + i, False))
        plan.append(x)
    rows = []
    for j, x in enumerate(plan):
        h = int.from_bytes(hashes[j % len(hashes)], "big")
        if x[0] == "final_add":
            _, label, k, sign, plus = x
            r, v = _rv(mul(k))
            s = (sign * (h % N) * pow(k, -1, N) + plus) % N
            rows.append(_row("final_add", label, h, r, s, v, sign < 0))
        else:
            rows.append(_row(x[0], x[1], h, x[2], x[3], x[4], x[5]))
    got = {c: sum(1 for x in rows if x[0] == c) for c in TX_COUNTS}
    assert got == TX_COUNTS and len(rows) == sum(TX_COUNTS.values()), got
    _check_runs(rows)
    return tuple(rows)


def ecrecover_input(row):
    """The 128 bytes of the ecRecover precompile for a row: hash || v + 27 as a 32-byte word || r || s."""
    return row[2] + bytes(31) + bytes([(row[3][64] + 27) & 0xFF]) + row[3][0:64]


def compare(rows, ok, pubs, addrs=None, address_of=None):
    """The rows' expected verdicts and keys against the given ones (ok[i] truthy or not, pubs[i] 64 bytes, addrs[i]
    20 bytes compared with address_of(expected key bytes); zeros for a rejected row):
    {class: [labels that differ]}, empty when equal."""
    assert len(rows) == len(ok) == len(pubs) and (addrs is None or len(addrs) == len(rows))
    bad = {}
    for i, x in enumerate(rows):
        want = x[4]
        good = bool(ok[i]) == (want is not None) and bytes(pubs[i]) == (bytes(64) if want is None else pub_bytes(want))
        if good and addrs is not None:
            good = bytes(addrs[i]) == (bytes(20) if want is None else address_of(pub_bytes(want)))
        if not good:
            bad.setdefault(x[0], []).append(x[1])
    return bad
