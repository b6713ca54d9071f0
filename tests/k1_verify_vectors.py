"""secp256k1 known-key verification rows at the edges no signer produces, and their reference.

Every secp256k1 verify kernel (secp256k1_verify_lane, secp256k1_verify_lane26, trio26_verify_body, the row kernel's
verify mode, the registered-key kernel) checks the key (x, y < p, on the curve), r in [1, n - 1], s in
[1, (n - 1) / 2], takes e = hash mod n, u1 = e / s, u2 = r / s, Q = u1 G + u2 P and accepts iff Q is not infinity
and x(Q) is r, or r + n when r + n < p.  verify() takes the hash as input, so e, r, s and the key are all free and
every edge below is reached by integer arithmetic alone, through three exact constructions:

  under a key   any P, u1, u2: R = u1 G + u2 P, r = x(R) mod n, s = r / u2, hash = u1 s.  (r, n - s) under the same
                hash is the row of (-u1, -u2), so s is made low by negating both, or, where the shape of u1 or u2
                is the point of the row, by taking another key;
  at a point    any R, r, u1, u2: s = r / u2, hash = u1 s, P = u2^-1 (R - u1 G), of unknown discrete log;
  with an s     any s, k, d: r = x(k G) mod n, e = s k - r d, P = d G.

The reference is verify(h32, r, s, P): oracle_secp256k1_verify's steps (oracle/ec.c) over affine points and Python
integers; tests/test_k1_verify_vectors.py pins it to the oracle on every row.

pool() returns the rows (class, label, h32, r, s, X, Y, expected), built once; COUNTS states the rows per class.
No GPU, no compiler, no numpy."""
import functools
import random

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
     0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
HALF = (N - 1) // 2  # the largest s libsecp256k1's verify accepts
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72

# the comb of u1 G: 16 windows of 16 bits (kWideBits, ecc_device.h) or 32 of 8 (BCOSGPU_INIT_SMALL_TABLES), and
# the windows [a, b) the lane-trio verify kernel gives each wave (kTrioVerifyShare, ecc_coop.hip), by wave
COMB_WIDE = 16
COMB_SMALL = 8
VERIFY_SHARE = {COMB_WIDE: ((0, 6), (15, 16), (10, 15), (6, 10)), COMB_SMALL: ((0, 11), (30, 32), (19, 30), (11, 19))}

# u2 = r / s as the scalars of tests/test_gpu_glv_split.py (its EDGES[1:], FOUND and SMALL; the CPU test compares)
GLV_EDGES = [1, 2, N - 1, N - 2, N // 2, N // 2 + 1, LAMBDA, N - LAMBDA, LAMBDA + 1, LAMBDA - 1, 2**128 - 1, 2**128,
             2**255]
GLV_FOUND = [0x2BA21979BC9B03DC7F8305635D5F9CBBDADB3C7BA53288ED9BE7A239C47B5D16,
             0x4F4670EEA6A05C074B4FDB244230C5F4DA0349093B3E53534EE80E8993FDBCF4,
             0xD27846A992B8A76DB9CF8B9C6C33FE4FC21F5B98E3B769D923AE6414AFCCE4F7,
             0x30B9ECDA70F6287D503159279B8A5F40360EB24A4FEA2448A0DCEEB849A78676]
GLV_SMALL = [x % N for c in (3, 4, 5, 6, 7) for x in (c, -c, c * LAMBDA, -c * LAMBDA)]
# chosen signed halves (k1, k2), u2 = k1 + k2 lambda: both below 2^123 (the chains start at infinity), one zero
GLV_HALVES = {"low++": (0x5A5A5A5A5A5A5A5A << 59, (0x3C3C3C3C3C3C3C3C << 58) + 1),
              "low-+": (-(0x7123456789ABCDEF << 59), (0x1FEDCBA987654321 << 60) + 1),
              "k1=0": (0, 0xC3D2E1F00112233445566778899AAB | 1),
              "k1=0,-": (0, -(0x9E3779B97F4A7C15F39CC0605CEDC8 | 1)),
              "k2=0": (0xB7E151628AED2A6ABF7158809CF4F3 | 1, 0),
              "k2=0,-": (-(0xA4093822299F31D0082EFA98EC4E6C | 1), 0)}

CLASSES = ("x_ge_n", "s_edge", "e_rep", "final_add", "u2_shape", "keys", "u1_shape", "reject")
COUNTS = {"x_ge_n": 10, "s_edge": 9, "e_rep": 10, "final_add": 9, "u2_shape": 43, "keys": 8, "u1_shape": 13,
          "reject": 10}
LAUNCH_MIN = 21  # every run of this many rows of the pool holds both verdicts


# ------------------------------------------------------------------ affine secp256k1 over Python integers
def on_curve(pt):
    x, y = pt
    return (y * y - (x * x * x + 7)) % P == 0


def add(A, Q):
    """secp256k1 affine addition (None = infinity)."""
    if A is None:
        return Q
    if Q is None:
        return A
    (x1, y1), (x2, y2) = A, Q
    if x1 == x2 and (y1 + y2) % P == 0:
        return None
    if A == Q:
        lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def neg(A):
    return None if A is None else (A[0], (-A[1]) % P)


def mul(k, A=G):
    """k A by double-and-add on Jacobian coordinates (one inversion at the end); the exceptional steps go through
    add()."""
    k %= N
    if k == 0 or A is None:
        return None
    ax, ay = A
    X, Y, Z = ax, ay, 1
    for bit in bin(k)[3:]:
        # doubling (a = 0); Y = 0 never happens on a curve of odd order
        S = 4 * X * Y * Y % P
        M = 3 * X * X % P
        X3 = (M * M - 2 * S) % P
        Y3 = (M * (S - X3) - 8 * pow(Y, 4, P)) % P
        X, Y, Z = X3, Y3, 2 * Y * Z % P
        if bit == "1":
            Z2 = Z * Z % P
            H = (ax * Z2 - X) % P
            Rr = (ay * Z2 * Z - Y) % P
            if H == 0:  # the running point is +-A: leave the fast path
                zi = pow(Z, -1, P)
                pt = add((X * zi * zi % P, Y * zi * zi * zi % P), A)
                if pt is None:
                    return mul_rest(k, A)
                X, Y, Z = pt[0], pt[1], 1
                continue
            H2 = H * H % P
            X3 = (Rr * Rr - H2 * H - 2 * X * H2) % P
            Y, Z = (Rr * (X * H2 - X3) - Y * H2 * H) % P, Z * H % P
            X = X3
    zi = pow(Z, -1, P)
    return X * zi * zi % P, Y * zi * zi * zi % P


def mul_rest(k, A):
    """k A by affine double-and-add (the path mul() takes where its running point met -A)."""
    R = None
    for bit in bin(k)[2:]:
        R = add(R, R)
        if bit == "1":
            R = add(R, A)
    return R


def lift_x(x, odd=0):
    """The curve point with this x and y of the given parity, or None."""
    v = (x * x * x + 7) % P
    y = pow(v, (P + 1) // 4, P)  # p = 3 mod 4
    if y * y % P != v:
        return None
    return (x, y if (y & 1) == odd else (P - y) % P)


def verify(h32, r, s, pub):
    """oracle_secp256k1_verify's steps: the key's coordinates below p and on the curve, r in [1, n - 1], s in
    [1, (n - 1) / 2], e = hash mod n, Q = (e / s) G + (r / s) P not infinity, x(Q) mod n = r."""
    X, Y = pub
    if not (0 <= X < P and 0 <= Y < P and on_curve(pub)):
        return False
    if not (0 < r < N and 0 < s <= HALF):
        return False
    e = int.from_bytes(h32, "big") % N
    w = pow(s, -1, N)
    Q = add(mul(e * w % N), mul(r * w % N, pub))
    if Q is None:
        return False
    return Q[0] % N == r


# ------------------------------------------------------------------ what the classes are named after
def h_of(row):
    return int.from_bytes(row[2], "big")


def u1_of(row):
    """u1 = (hash mod n) / s of a row whose s is invertible."""
    return h_of(row) % N * pow(row[4], -1, N) % N


def u2_of(row):
    return row[3] * pow(row[4], -1, N) % N


def summands(row):
    """(u1 G, u2 P), the two points the final addition takes; the key reduced mod p."""
    pub = (row[5] % P, row[6] % P)
    return mul(u1_of(row)), mul(u2_of(row), pub)


def x_of(row):
    """x(Q) of the row's u1 G + u2 P (None: infinity)."""
    Q = add(*summands(row))
    return None if Q is None else Q[0]


def comb_windows(u, bits):
    return [(u >> (bits * i)) & ((1 << bits) - 1) for i in range(256 // bits)]


def comb_shares(u, bits):
    """The part of u each wave of the lane-trio verify kernel puts through the comb (by wave); their sum is u."""
    w = comb_windows(u, bits)
    out = [sum(w[i] << (bits * i) for i in range(a, b)) for a, b in VERIFY_SHARE[bits]]
    assert sum(out) == u
    return out


# ------------------------------------------------------------------ the rows
def _row(cls, label, h, r, s, pub, intended):
    assert 0 <= h < 2**256 and 0 <= r < 2**256 and 0 <= s < 2**256 and 0 <= pub[0] < 2**256 and 0 <= pub[1] < 2**256
    h32 = h.to_bytes(32, "big")
    got = verify(h32, r, s, pub)
    assert got == intended, (cls, label, got)
    return (cls, label, h32, r, s, pub[0], pub[1], got)


def _again(cls, label, a, intended, h=None, r=None, s=None, pub=None):
    """Row a with some of its fields replaced."""
    return _row(cls, label, h_of(a) if h is None else h, a[3] if r is None else r, a[4] if s is None else s,
                (a[5], a[6]) if pub is None else pub, intended)


def _under(cls, label, pub, u1, u2, r=None, intended=True):
    """The row under the key `pub` whose verification computes u1 G + u2 P (or -u1, -u2 where that makes s low;
    None where the caller must keep the scalars and s is high): r = x(R) mod n unless given."""
    R = add(mul(u1), mul(u2, pub))
    if r is None:
        r = R[0] % N
    s = r * pow(u2, -1, N) % N
    assert r and s
    return _row(cls, label, u1 * s % N, r, min(s, N - s), pub, intended), s <= HALF


def _shaped(cls, label, rnd, u1=None, u2=None):
    """An accepted row with the given u1 or u2 kept as it is: keys d G are tried until s is low."""
    while True:
        a, b = _scalar(rnd) if u1 is None else u1, _scalar(rnd) if u2 is None else u2
        d = _scalar(rnd)
        if (a + b * d) % N == 0:
            continue
        x, kept = _under(cls, label, mul(d), a, b)
        if kept:
            assert (u1 is None or u1_of(x) == u1) and (u2 is None or u2_of(x) == u2)
            return x


def _at_point(cls, label, rnd, R, r=None, intended=True):
    """The row whose u1 G + u2 P is the given point R, presented with r (default x(R) mod n): a key of unknown
    discrete log P = u2^-1 (R - u1 G)."""
    u1, u2 = _scalar(rnd), _scalar(rnd)
    r = R[0] % N if r is None else r
    s = r % N * pow(u2, -1, N) % N
    if s > HALF:
        u2, s = N - u2, N - s
    pub = mul(pow(u2, -1, N), add(R, neg(mul(u1))))
    assert add(mul(u1), mul(u2, pub)) == R
    return _row(cls, label, u1 * s % N, r, s, pub, intended)


def _with_s(cls, label, rnd, s):
    """The accepted row with this s (low): r = x(k G) mod n, e = s k - r d under P = d G."""
    k, d = _scalar(rnd), _scalar(rnd)
    r = mul(k)[0] % N
    return _row(cls, label, (s * k - r * d) % N, r, s, mul(d), True)


def _with_h(cls, label, rnd, h):
    """The accepted row over this hash: e = h mod n, s = (e + r d) / k or its negative, whichever is low."""
    k, d = _scalar(rnd), _scalar(rnd)
    r = mul(k)[0] % N
    s = (h % N + r * d) * pow(k, -1, N) % N
    return _row(cls, label, h, r, min(s, N - s), mul(d), True)


def _first_x(start, step):
    x = start
    while lift_x(x) is None:
        x += step
    return x


def _scalar(rnd):
    return rnd.randrange(2**200, N)


def _thread(rows, spare, run=9):
    """rows, with one of `spare` (rejected rows) put in wherever `run` accepted rows would stand in line; the rest
    of `spare` at the end."""
    out, spare, line = [], list(spare), 0
    for x in rows:
        if x[7] and line == run and spare:
            out.append(spare.pop(0))
            line = 0
        out.append(x)
        line = line + 1 if x[7] else 0
    return out + spare


@functools.lru_cache(maxsize=None)
def pool():
    rnd = random.Random(0x6B31)
    rows = []
    gap = P - N

    # -------- x_ge_n: x(Q) in [n, p) is met through r + n alone; the branch's two conditions at their edges
    xa = _first_x(N + 1, 1)              # the first curve x above n (x = n is on the curve and gives r = 0)
    xb = _first_x(P - 1, -1)             # the last below p
    xm = _first_x((N + P) // 2, 1)       # mid-range
    for label, x, odd in (("first>n", xa, 0), ("first>n,-y", xa, 1), ("last<p", xb, 0), ("last<p,-y", xb, 1),
                          ("mid", xm, 0)):
        rows.append(_at_point("x_ge_n", label, rnd, lift_x(x, odd)))
    # r small, met by the first comparison; r + n < p holds and is another value
    xs = _first_x(1, 1)
    rows.append(_at_point("x_ge_n", "small", rnd, lift_x(xs, 1)))
    # r = p - n: r + n = p is not below p, the second comparison is skipped (and would compare with 0)
    assert lift_x(gap) is not None
    rows.append(_at_point("x_ge_n", "r=p-n", rnd, lift_x(gap, 0)))
    # r + n = x(Q) + p fits in 256 bits and is x(Q) mod p: only the `r + n < p` test rejects
    rows.append(_at_point("x_ge_n", "r+n=x+p:skip", rnd, lift_x(xs, 0), r=xs + gap, intended=False))
    # the branch is taken and must not match; and x(Q) itself as r, which is no scalar
    rows.append(_at_point("x_ge_n", "r+n=x+1", rnd, lift_x(xa, 0), r=xa - N + 1, intended=False))
    rows.append(_at_point("x_ge_n", "r=x>=n", rnd, lift_x(xa, 1), r=xa, intended=False))

    # -------- s_edge: the ends of [1, (n - 1) / 2], and each end's twin (r, n - s) just outside
    edge = {}
    for label, s in (("s=1", 1), ("s=2", 2), ("s=(n-1)/2", HALF), ("s=(n-1)/2-1", HALF - 1)):
        edge[label] = _with_s("s_edge", label, rnd, s)
    rows += [edge["s=(n-1)/2"], _again("s_edge", "s=(n+1)/2", edge["s=(n-1)/2"], False, s=HALF + 1),
             edge["s=1"], _again("s_edge", "s=n-1", edge["s=1"], False, s=N - 1),
             _again("s_edge", "s=n+1", edge["s=1"], False, s=N + 1),
             edge["s=2"], _again("s_edge", "s=n", edge["s=2"], False, s=N), _again("s_edge", "s=0", edge["s=2"], False, s=0),
             edge["s=(n-1)/2-1"]]

    # -------- e_rep: hashes at the ends of [0, n) and [n, 2^256), each signed for e = hash mod n; one signature
    # under e and under e + n
    top = 2 * N - 2**256  # the reduced value of the largest hash, plus one
    for label, h in (("h=0", 0), ("h=n", N), ("h=n-1", N - 1), ("h=n+1", N + 1), ("h=2n-2^256-1", top - 1),
                     ("h=2n-2^256", top), ("h=2n-2^256+1", top + 1), ("h=2^256-1", 2**256 - 1)):
        rows.append(_with_h("e_rep", label, rnd, h))
    a = _with_h("e_rep", "e", rnd, rnd.randrange(2**100, 2**256 - N))
    rows += [a, _again("e_rep", "e+n", a, True, h=h_of(a) + N)]

    # -------- final_add: u1 G = u2 P (a doubling) and u1 G = -u2 P (infinity)
    for label, d in (("d", _scalar(rnd)), ("P=G", 1), ("P=-G", N - 1), ("P=2G", 2), ("P=lambdaG", LAMBDA)):
        u2 = _scalar(rnd)
        a, _ = _under("final_add", "dbl:" + label, mul(d), u2 * d % N, u2)
        rows.append(a)
        if label == "d":
            # the same doubling presented with another r: a doubling computed as X = Z = 0 meets the projective
            # x-check for every r
            rows.append(_under("final_add", "dbl:d,r+1", mul(d), u2 * d % N, u2, r=a[3] + 1, intended=False)[0])
    for label, d in (("P=G", 1), ("d", _scalar(rnd))):
        u2 = _scalar(rnd)
        u1 = -u2 * d % N
        rows.append(_under("final_add", "inf:" + label, mul(d), u1, u2, r=mul(u1)[0] % N, intended=False)[0])
    # the registered-key kernel sums lane L = 2^(16 L) (w_L G + c_L P) over the 16-bit windows w of u1 and c of u2,
    # lanes 0..7 and 8..15 last: with u2 = c0 in window 0 alone and c0 d + (u1 mod 2^128) = u1 - u1 mod 2^128 that
    # last addition is a doubling, whose result goes to the x-check as it is.  R does not depend on c0, so s does
    lo, hi = rnd.randrange(2**120, 2**128), rnd.randrange(2**120, 2**127) << 128
    for c0 in range(1, 200):
        a, kept = _under("final_add", "dbl:keyed-last", mul((hi - lo) * pow(c0, -1, N) % N), hi + lo, c0)
        if kept:
            break
    rows.append(a)

    # -------- u2_shape: the GLV halves of u2 = r / s
    u2s = [("edge%d" % i, v) for i, v in enumerate(GLV_EDGES)] + [("found%d" % i, v) for i, v in enumerate(GLV_FOUND)]
    u2s += [("small%d" % i, v) for i, v in enumerate(GLV_SMALL)]
    u2s += [(label, (k1 + k2 * LAMBDA) % N) for label, (k1, k2) in GLV_HALVES.items()]
    for label, u2 in u2s:
        rows.append(_shaped("u2_shape", label, rnd, u2=u2))

    # -------- keys: coordinates at and above p beside their canonical twins; off the curve; small coordinates
    x1 = lift_x(1, 0)
    xc = pow(-6 % P, (P + 2) // 9, P)  # p = 7 mod 9: the cube root of y^2 - 7 for y = 1
    assert pow(xc, 3, P) == -6 % P and on_curve((xc, 1))
    a, _ = _under("keys", "x=1", x1, _scalar(rnd), _scalar(rnd))
    b, _ = _under("keys", "y=1", (xc, 1), _scalar(rnd), _scalar(rnd))
    xt = _first_x(2, 1) + 1
    while lift_x(xt) is not None:
        xt += 1
    yt = pow(-(xt**3 + 7) % P, (P + 1) // 4, P)  # on -y^2 = x^3 + 7, the quadratic twist
    assert (yt * yt + xt**3 + 7) % P == 0
    rows += [a, _again("keys", "x=1+p", a, False, pub=(1 + P, x1[1])),
             _under("keys", "x=1,-y", neg(x1), _scalar(rnd), _scalar(rnd))[0],
             b, _again("keys", "y=1+p", b, False, pub=(xc, 1 + P)),
             _again("keys", "(0,0)", a, False, pub=(0, 0)), _again("keys", "twist", b, False, pub=(xt, yt)),
             _again("keys", "y^2^200", a, False, pub=(1, x1[1] ^ (1 << 200)))]

    # -------- u1_shape: the comb shares of u1 = e / s (kTrioVerifyShare: bits [0, 96), [96, 160), [160, 240),
    # [240, 256) on the 16-bit comb, [0, 88), [88, 152), [152, 240), [240, 256) on the 8-bit one)
    bits = lambda lo, hi: rnd.randrange(1 << (hi - lo - 1), 1 << (hi - lo)) << lo
    full = bits(0, 88) | bits(96, 152) | bits(160, 240) | (0xFFFE << 240)
    u1s = [("only0", bits(0, 88)), ("only3", bits(96, 152)), ("only2", bits(160, 240)), ("only1", 0xFFFF << 240),
           ("only0/16,3/8", 0xA5 << 88), ("only3/16,2/8", 0xC3 << 152),  # the windows the two layouts place apart
           ("zero0", full >> 96 << 96), ("zero3", full & ~(((1 << 72) - 1) << 88)),
           ("zero2", full & ~(((1 << 88) - 1) << 152)), ("zero1", full & ((1 << 240) - 1)),
           ("1", 1), ("n-1", N - 1), ("max-windows", 2**256 - 1 - (2 << 128))]
    for label, u1 in u1s:
        rows.append(_shaped("u1_shape", "u1=" + label, rnd, u1=u1))

    # -------- reject: ordinary wrong rows, threaded through the long accepted stretches
    by = {(x[0], x[1]): x for x in rows}
    spare = []
    for (cls, label), what, bit in ((("e_rep", "h=0"), "h", 0), (("e_rep", "e"), "h", 255),
                                    (("u2_shape", "edge0"), "r", 7), (("u1_shape", "u1=1"), "s", 3)):
        a = by[(cls, label)]
        v = {"h": h_of(a), "r": a[3], "s": a[4]}[what] ^ (1 << bit)
        spare.append(_again("reject", "%s^2^%d:%s" % (what, bit, label), a, False, **{what: v}))
    spare.append(_again("reject", "r=0:found0", by[("u2_shape", "found0")], False, r=0))
    spare.append(_again("reject", "r=n:small0", by[("u2_shape", "small0")], False, r=N))
    spare.append(_again("reject", "r+n:small", by[("x_ge_n", "small")], False, r=by[("x_ge_n", "small")][3] + N))
    for label, other in (("edge4", "edge5"), ("u1=n-1", "u1=1")):
        cls = "u1_shape" if label.startswith("u1") else "u2_shape"
        o = by[(cls, other)]
        spare.append(_again("reject", "key-of-%s:%s" % (other, label), by[(cls, label)], False, pub=(o[5], o[6])))
    spare.append(_again("reject", "h+1:dbl:P=G", by[("final_add", "dbl:P=G")], False,
                        h=h_of(by[("final_add", "dbl:P=G")]) + 1))
    rows = _thread(rows, spare)

    got = {c: sum(1 for x in rows if x[0] == c) for c in CLASSES}
    assert got == COUNTS, got
    assert 90 <= len(rows) <= 120
    for i in range(len(rows) - LAUNCH_MIN + 1):
        assert len({x[7] for x in rows[i:i + LAUNCH_MIN]}) == 2, i
    return tuple(rows)


def packed(rows):
    """(hash32, r || s, X || Y) of each row, as the C ABI takes them."""
    return [(x[2], x[3].to_bytes(32, "big") + x[4].to_bytes(32, "big"), x[5].to_bytes(32, "big") + x[6].to_bytes(32, "big"))
            for x in rows]


def compare(rows, verdicts):
    """The rows' expected verdicts against the given ones: {class: [labels that differ]}, empty when equal."""
    assert len(rows) == len(verdicts)
    bad = {}
    for x, v in zip(rows, verdicts):
        if bool(v) != x[7]:
            bad.setdefault(x[0], []).append(x[1])
    return bad
