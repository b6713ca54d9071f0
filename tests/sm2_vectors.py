"""SM2 verification rows with a chosen e, for the kernels built with BCOSGPU_SM2_RAW_E (lib/libbcosgpu_rawe.so:
sm2_e / sm2_e_from_za return the 32 digest bytes as e, not reduced), and their reference.

Every SM2 verify kernel ends with t = r + s mod n, Q = s G + t P, e reduced once mod n, c = r - e mod n, accept
iff x(Q) is c, or c + n when c + n < p.  With e = SM3(Z_A || digest) no input chooses e; with e free a valid
signature follows from any s, t and P: Q by integers, r = t - s, e = r - x(Q) mod n.  So every edge below is
an ACCEPTED row, which a wrong kernel rejects.

The reference is verify(e, r, s, P): oracle_sm2_recover's steps (oracle/ec.c) with e given, over affine
points and Python integers; tests/test_sm2_vectors.py pins it to the oracle with e = SM3(Z_A || digest).

pool() returns the rows (class, label, e32, r, s, X, Y, expected), built once; COUNTS states the rows per class.
No GPU, no compiler, no numpy."""
import functools
import random

P = 0xFFFFFFFEFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF00000000FFFFFFFFFFFFFFFF
N = 0xFFFFFFFEFFFFFFFFFFFFFFFFFFFFFFFF7203DF6B21C6052B53BBF40939D54123
B = 0x28E9FA9E9D9F5E344D5A9E4BCF6509A7F39789F515AB8F92DDBCBD414D940E93
G = (0x32C4AE2C1F1981195F9904466A39C9948FE30BBFF2660BE1715A4589334C74C7,
     0xBC3736A2F4F6779C59BDCEE36B692153D0A9877CC62A474002DF32E52139F0A0)

# the kernels' window widths: t P on 65 radix-16 Booth windows (digit 64 is bit 255; ecc_device.h
# booth_digit256), the lane-trio kernel's chain split at window kSm2TrioSplit (ecc_pair.hip), the row kernel's
# t = t_lo + 2^kSm2RowSplit t_hi (ecc_row.hip), s G on a 16-bit
# comb (kWideBits, ecc_device.h) or the 8-bit one (BCOSGPU_INIT_SMALL_TABLES)
BOOTH_BITS = 4
TRIO_SPLIT = 44
ROW_SPLIT_BIT = 212
COMB_WIDE = 16
COMB_SMALL = 8

CLASSES = ("e_rep", "x1_ge_n", "final_add", "t_shape", "s_shape", "keys", "keyed_lanes", "reject")
COUNTS = {"e_rep": 14, "x1_ge_n": 8, "final_add": 11, "t_shape": 20, "s_shape": 16, "keys": 10, "keyed_lanes": 10,
          "reject": 10}


# ------------------------------------------------------------------ affine SM2 over Python integers
def on_curve(pt):
    x, y = pt
    return (y * y - (x * x * x - 3 * x + B)) % P == 0


def add(A, Q):
    """SM2 affine addition (None = infinity)."""
    if A is None:
        return Q
    if Q is None:
        return A
    (x1, y1), (x2, y2) = A, Q
    if x1 == x2 and (y1 + y2) % P == 0:
        return None
    if A == Q:
        lam = (3 * x1 * x1 - 3) * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def neg(A):
    return None if A is None else (A[0], (-A[1]) % P)


def mul(k, A=G):
    R = None
    for bit in bin(k % N)[2:] if k % N else "":
        R = add(R, R)
        if bit == "1":
            R = add(R, A)
    return R


def lift_x(x, odd=0):
    """The curve point with this x and y of the given parity, or None."""
    v = (x * x * x - 3 * x + B) % P
    y = pow(v, (P + 1) // 4, P)  # p = 3 mod 4
    if y * y % P != v:
        return None
    return (x, y if (y & 1) == odd else (P - y) % P)


def verify(e, r, s, pub):
    """oracle_sm2_recover's steps with e (0 <= e < 2^256) given: the key's coordinates below p and on the curve,
    r, s in [1, n - 1], t = r + s mod n nonzero, Q = s G + t P not infinity, (e mod n + x(Q) mod n) mod n = r."""
    X, Y = pub
    if not (0 <= X < P and 0 <= Y < P and on_curve(pub)):
        return False
    if not (0 < r < N and 0 < s < N):
        return False
    t = (r + s) % N
    if t == 0:
        return False
    Q = add(mul(s), mul(t, pub))
    if Q is None:
        return False
    return (e % N + Q[0] % N) % N == r


# ------------------------------------------------------------------ what the classes are named after
def booth_digits(t):
    """The 65 radix-16 Booth digits of t (index = window), as booth_digit256 takes them from the top."""
    d = []
    for w in range(64):
        nib = (t >> (4 * w)) & 15
        below = (t >> (4 * w - 1)) & 1 if w else 0
        d.append(nib + below - 16 * (nib >> 3))
    d.append((t >> 255) & 1)
    assert sum(x << (4 * w) for w, x in enumerate(d)) == t
    return d


def trio_low_part(t):
    """The Booth windows of t below the lane-trio kernel's split, as a signed number (its low chains' scalar)."""
    return sum(x << (BOOTH_BITS * w) for w, x in enumerate(booth_digits(t)[:TRIO_SPLIT]))


def comb_windows(s, bits):
    return [(s >> (bits * i)) & ((1 << bits) - 1) for i in range(256 // bits)]


def c_of(row):
    """c = r - (e mod n) mod n, the kernels' comparison value."""
    return (row[3] - int.from_bytes(row[2], "big") % N) % N


def x_of(row):
    """x(Q) of the row's s G + t P (None: infinity)."""
    Q = add(mul(row[4]), mul((row[3] + row[4]) % N, (row[5], row[6])))
    return None if Q is None else Q[0]


def keyed_lane_points(row):
    """The registered-key kernel's 16 partial sums 2^(16 L) (w_L G + c_L P), w / c the 16-bit windows of s / t."""
    s, t, pub = row[4], (row[3] + row[4]) % N, (row[5], row[6])
    ws, cs = comb_windows(s, 16), comb_windows(t, 16)
    return [mul(1 << (16 * L), add(mul(ws[L]), mul(cs[L], pub))) for L in range(16)]


# ------------------------------------------------------------------ the rows
def _row(cls, label, e, r, s, pub, intended):
    assert 0 <= e < 2**256 and 0 <= r < 2**256 and 0 <= s < 2**256
    got = verify(e, r, s, pub)
    assert got == intended, (cls, label, got)
    return (cls, label, e.to_bytes(32, "big"), r, s, pub[0], pub[1], got)


def _valid(cls, label, s, t, pub):
    """The accepted signature whose verification computes s G + t P: r = t - s, e = r - x(Q) mod n."""
    Q = add(mul(s), mul(t, pub))
    r = (t - s) % N
    assert Q is not None and r != 0 and 0 < s < N and 0 < t < N, (cls, label)
    return _row(cls, label, (r - Q[0]) % N, r, s, pub, True)


def _with_e(cls, label, e, d, u, intended=True):
    """The signature under P = d G whose e is the given one and whose Q is u G: r = e + x(u G) mod n,
    t (1 + d) = u + r, s = t - r."""
    x1 = mul(u)[0]
    r = (e + x1) % N
    t = (u + r) * pow(1 + d, -1, N) % N
    s = (t - r) % N
    assert r and s and t
    return _row(cls, label, e, r, s, mul(d), intended), x1


def _at_point(cls, label, Q, s, t, c=None, intended=True):
    """The signature whose s G + t P is the given point Q: a key of unknown discrete log P = t^-1 (Q - s G).
    c (default x(Q) mod n) is the comparison value the row's e leads to."""
    pub = mul(pow(t, -1, N), add(Q, neg(mul(s))))
    assert add(mul(s), mul(t, pub)) == Q
    r = (t - s) % N
    c = Q[0] % N if c is None else c
    return _row(cls, label, (r - c) % N, r, s, pub, intended)


def _first_x(start, step):
    x = start
    while lift_x(x) is None:
        x += step
    return x


def _scalar(rnd):
    return rnd.randrange(2**200, N)


@functools.lru_cache(maxsize=None)
def pool():
    rnd = random.Random(0x5D2)
    rows = []

    # -------- e_rep: the same signature with e and with e + n; e at the ends of both ranges; e + x1 wrapping n
    for k, e in enumerate((1, rnd.randrange(2**200, 2**223), 2**256 - N - 1)):
        d, u = _scalar(rnd), _scalar(rnd)
        a, _ = _with_e("e_rep", "small%d" % k, e, d, u)
        rows += [a, _row("e_rep", "small%d+n" % k, e + N, a[3], a[4], (a[5], a[6]), True)]
    for label, e in (("e=0", 0), ("e=n", N), ("e=n-1", N - 1), ("e=2^256-1", 2**256 - 1)):
        rows.append(_with_e("e_rep", label, e, _scalar(rnd), _scalar(rnd))[0])
    d, u = _scalar(rnd), _scalar(rnd)
    x1 = mul(u)[0] % N
    rows.append(_with_e("e_rep", "wrap:e+x1=n+1", N + 1 - x1, d, u)[0])  # r = 1
    rows.append(_with_e("e_rep", "nowrap:e+x1=n-1", N - 1 - x1, d, u)[0])  # r = n - 1
    # e >= n whose reduced value exceeds r (e + x1 wraps n, x1 just below n): r - e, e not reduced, is short of
    # c by n twice, so one correction of the difference does not make up for a missing reduction of e
    xq = _first_x(N - 1, -1)
    s, r = _scalar(rnd), rnd.randrange(2**200, 2**222)
    a = _at_point("e_rep", "wrap-small", lift_x(xq, 1), s, (s + r) % N)
    e = int.from_bytes(a[2], "big")
    assert r < e < 2**256 - N
    rows += [a, _row("e_rep", "wrap-small+n", e + N, a[3], a[4], (a[5], a[6]), True)]

    # -------- x1_ge_n: x(Q) in [n, p) is met through c + n alone; the branch's two conditions at their edges
    xa = _first_x(N, 1)          # the first curve x at or above n
    xb = _first_x(P - 1, -1)     # the last below p
    xc = _first_x(N - 1, -1)     # the nearest below n: c + n carries out of 256 bits
    xd = _first_x(1, 1)          # a small x: c + n < p holds and is not x(Q)
    for label, x, odd in (("first>=n", xa, 0), ("first>=n,-y", xa, 1), ("last<p", xb, 0), ("nearest<n", xc, 0),
                          ("small", xd, 1)):
        rows.append(_at_point("x1_ge_n", label, lift_x(x, odd), _scalar(rnd), _scalar(rnd)))
    # c >= p - n with c + n = x(Q) + p: equal to x(Q) mod p, so only the `c + n < p` test rejects it
    rows.append(_at_point("x1_ge_n", "c>=p-n:skip", lift_x(xd, 0), _scalar(rnd), _scalar(rnd), c=xd + P - N,
                          intended=False))
    # c + n < p holds and is one off x(Q), on either side of the first point at or above n
    rows.append(_at_point("x1_ge_n", "c+n=x+1", lift_x(xa, 0), _scalar(rnd), _scalar(rnd), c=xa - N + 1, intended=False))
    rows.append(_at_point("x1_ge_n", "c=x-n-1", lift_x(xa, 1), _scalar(rnd), _scalar(rnd), c=xa - N - 1, intended=False))

    # -------- final_add: s G = t P (a doubling) and s G = -t P (infinity, with c = x of both operands)
    for k in range(2):
        d, t = _scalar(rnd), _scalar(rnd)
        a = _valid("final_add", "dbl%d" % k, t * d % N, t, mul(d))
        # the same doubling with another e: a doubling computed as X = Z = 0 meets the projective x-check for every c
        rows += [a, _row("final_add", "dbl%d:e^1" % k, int.from_bytes(a[2], "big") ^ 1, a[3], a[4], (a[5], a[6]), False)]
        s = (-t * d) % N
        r = (t - s) % N
        rows.append(_row("final_add", "inf%d" % k, (r - mul(s)[0]) % N, r, s, mul(d), False))

    # the lane-trio kernel's default schedule sums (s G + T_lo P) + T_hi P, T_lo the Booth windows below the split
    # taken as a signed number: each of its two additions as a doubling, and the first as infinity (accepted)
    d, t = _scalar(rnd), _scalar(rnd)
    t_lo = trio_low_part(t)
    for label, s in (("trio-dbl-lo", t_lo * d % N), ("trio-dbl-hi", (t - 2 * t_lo) * d % N), ("trio-inf-lo", -t_lo * d % N)):
        a = _valid("final_add", label, s, t, mul(d))
        rows.append(a)
        if "dbl" in label:
            rows.append(_row("final_add", label + ":e^1", int.from_bytes(a[2], "big") ^ 1, a[3], a[4], (a[5], a[6]), False))

    # -------- t_shape: the chains over structured t (65 Booth windows; the trio kernel's split at window 44)
    lo = 4 * TRIO_SPLIT
    ts = [("1", 1), ("2", 2), ("n-1", N - 1), ("n-2", N - 2), ("5", 5), ("n-5", N - 5), ("2^255", 2**255),
          ("top-window-0", 2**251 - 12345), ("lead-windows-0", 2**200 + 777), ("all+-8", int("78" * 32, 16)),
          ("all-7/-8", int("8" * 64, 16)), ("low-part-0", rnd.randrange(2**70, 2**79) << lo),
          ("high-part-0", rnd.randrange(2**170, 2**(lo - 1))), ("16^split", 1 << lo),
          ("16^split/2", 1 << (lo - 1)), ("16^split-1", (1 << lo) - 1), ("n-2^176", N - (1 << lo)),
          ("alt-windows-0", int("07" * 32, 16)), ("row-low-part-0", rnd.randrange(2**30, 2**43) << ROW_SPLIT_BIT),
          ("row-2^split-1", (1 << ROW_SPLIT_BIT) - 1)]
    for label, t in ts:
        rows.append(_valid("t_shape", "t=" + label, _scalar(rnd), t, mul(_scalar(rnd))))

    # -------- s_shape: the comb over structured s (16 windows of 16 bits, 32 of 8)
    ss = [("1", 1), ("2", 2), ("n-1", N - 1), ("2^8", 2**8), ("2^16", 2**16), ("0xffff", 0xFFFF),
          ("top16", 0xFFFF << 240), ("top8", 0xFE << 248), ("2^240", 2**240), ("2^248", 2**248),
          ("alt16-lo", int("0000ffff" * 8, 16)), ("alt16-hi", int("ffff0000" * 8, 16)),
          ("alt8-lo", int("00ff" * 16, 16)), ("alt8-hi", int("ff00" * 16, 16)), ("ones8", int("01" * 32, 16)),
          ("ones16", int("0001" * 16, 16))]
    for label, s in ss:
        rows.append(_valid("s_shape", "s=" + label, s, _scalar(rnd), mul(_scalar(rnd))))

    # -------- keys: P among the comb's own entries, -G, and the two points with X = 0
    y0 = lift_x(0, 0)
    for label, pub in (("G", G), ("G'", G), ("2G", mul(2)), ("-2G", neg(mul(2))), ("8G", mul(8)), ("-G", neg(G)),
                       ("-G'", neg(G)), ("(0,y)", y0), ("(0,y)'", y0), ("(0,-y)", neg(y0))):
        s, t = (3, 5) if label in ("G'", "-G'") else (_scalar(rnd), _scalar(rnd))
        rows.append(_valid("keys", "P=" + label, s, t, pub))

    # -------- keyed_lanes: the registered-key kernel's partial sums coincide or cancel; t = c0 in window 0 only
    for c0 in (3, 0xFFFF):
        inv = pow(c0, -1, N)
        # lanes 0 and 1 equal: c0 d + w0 = 2^16 w1, s = w0 + 2^16 w1
        rows.append(_valid("keyed_lanes", "dbl1/%x" % c0, 5 + 2**16, c0, mul((2**16 - 5) * inv % N)))
        if c0 == 3:  # and with another e, rejected (as final_add's)
            a = rows[-1]
            rows.append(_row("keyed_lanes", "dbl1/3:e^1", int.from_bytes(a[2], "big") ^ 1, a[3], a[4], (a[5], a[6]), False))
        # lanes 0 and 1 opposite, lane 2 keeps the total: c0 d + w0 = -2^16 w1
        rows.append(_valid("keyed_lanes", "neg1/%x" % c0, 5 + 2**16 + 2**32, c0, mul((-2**16 - 5) * inv % N)))
        # lanes {0, 1} equal to lanes {2, 3}: c0 d + w0 = 2^32 w2
        rows.append(_valid("keyed_lanes", "dbl2/%x" % c0, 5 + 2**32, c0, mul((2**32 - 5) * inv % N)))
        if c0 == 3:
            a = rows[-1]
            rows.append(_row("keyed_lanes", "dbl2/3:e^1", int.from_bytes(a[2], "big") ^ 1, a[3], a[4], (a[5], a[6]), False))
        # the total is infinity: c0 d = -s
        s = 7 + 2**16 + 2**48
        d = (-s) * inv % N
        r = (c0 - s) % N
        rows.append(_row("keyed_lanes", "inf/%x" % c0, (r - mul(s)[0]) % N, r, s, mul(d), False))

    # -------- reject: rejected twins of accepted rows, so that every launch holds both verdicts
    by = {(x[0], x[1]): x for x in rows}
    for (cls, label), bit in ((("e_rep", "small0"), 0), (("e_rep", "small1+n"), 255), (("x1_ge_n", "first>=n"), 2),
                              (("t_shape", "t=all+-8"), 131)):
        a = by[(cls, label)]
        e = int.from_bytes(a[2], "big") ^ (1 << bit)
        rows.append(_row("reject", "e^2^%d:%s" % (bit, label), e, a[3], a[4], (a[5], a[6]), False))
    for cls, label in (("e_rep", "e=0"), ("keys", "P=G"), ("s_shape", "s=ones16")):
        a = by[(cls, label)]
        rows.append(_row("reject", "r+s=n:" + label, int.from_bytes(a[2], "big"), a[3], N - a[3], (a[5], a[6]), False))
    for cls, label in (("e_rep", "e=n"), ("keys", "P=(0,y)"), ("final_add", "dbl0")):
        a = by[(cls, label)]
        rows.append(_row("reject", "off-curve:" + label, int.from_bytes(a[2], "big"), a[3], a[4], (a[5], a[6] ^ 1), False))

    got = {c: sum(1 for x in rows if x[0] == c) for c in CLASSES}
    assert got == COUNTS, got
    assert 80 <= len(rows) <= 120
    return tuple(rows)


def packed(rows):
    """(digest32, r || s || X || Y) of each row, as the C ABI takes them."""
    return [(x[2], b"".join(v.to_bytes(32, "big") for v in x[3:7])) for x in rows]


def compare(rows, verdicts):
    """The rows' expected verdicts against the given ones: {class: [labels that differ]}, empty when equal."""
    assert len(rows) == len(verdicts)
    bad = {}
    for x, v in zip(rows, verdicts):
        if bool(v) != x[7]:
            bad.setdefault(x[0], []).append(x[1])
    return bad
