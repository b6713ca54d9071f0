"""Cases and checker for fisco-bcos_amd/tools/triovec.hip: the lane-trio point operations of ec26_trio.h
(secp256k1, lib/triovec) and ecp26_trio.h (SM2, lib/triovec_sm2) on a real wave (4 rows x 5 trios, the phantom
lane 15 of each row besides).  The reference is affine point arithmetic over Python integers (as
tests/test_fe26.py's _add), never another GPU path; a result is right when it is affine-equal to the integer
result, or both are infinity.  SM2 coordinates are in fp26's Montgomery form (x R mod p, R = 2^286).

Operands are on-curve points in a random Jacobian representation with (m - 1) p added limb by limb to each
coordinate up to the op's entry contract, so every limb sits just under its bound while the point stays on the
curve.  The exceptional additions (P = Q, P = -Q, P = infinity, and for trio_add Q = infinity and both) are
placed across the wave: on the device trio::any votes over all 64 lanes, so one exceptional trio takes the
nineteen ordinary ones through the exceptional branch.  Every mixed wave is a copy of one all-ordinary wave
with only the exceptional trios replaced, so each ordinary trio runs with the same operands in an ordinary
and in several mixed waves, and must give the same limbs every time."""
import random

R286 = 2**286
N_RANDOM = 300
ZERO = [0] * 10


class Curve:
    def __init__(self, p, a, b, mont):
        self.p, self.a, self.b, self.mont = p, a, b, mont
        self.pl = [(p >> (26 * i)) & 0x3FFFFFF for i in range(9)] + [p >> 234]
        self.rinv = pow(mont, -1, p)

    def add(self, p, q):
        P = self.p
        if p is None:
            return q
        if q is None:
            return p
        if p[0] == q[0] and (p[1] + q[1]) % P == 0:
            return None
        if p == q:
            lam = (3 * p[0] * p[0] + self.a) * pow(2 * p[1], -1, P) % P
        else:
            lam = (q[1] - p[1]) * pow(q[0] - p[0], -1, P) % P
        x = (lam * lam - p[0] - q[0]) % P
        return x, (lam * (p[0] - x) - p[1]) % P

    def neg(self, p):
        return None if p is None else (p[0], -p[1] % self.p)

    def mul(self, k, pt):
        if k < 0:
            return self.mul(-k, self.neg(pt))
        r = None
        for bit in bin(k)[2:] if k else "":
            r = self.add(r, r)
            if bit == "1":
                r = self.add(r, pt)
        return r

    def rand_point(self, rnd):
        P = self.p
        while True:
            x = rnd.randrange(P)
            rhs = (x**3 + self.a * x + self.b) % P
            y = pow(rhs, (P + 1) // 4, P)
            if y * y % P == rhs:
                return x, (y if rnd.randrange(2) else P - y)

    def limbs(self, x, m=1):
        """The field element x as stored (times R for SM2), canonical limbs plus (m - 1) p limb by limb."""
        x = x * self.mont % self.p
        c = [(x >> (26 * i)) & 0x3FFFFFF for i in range(9)] + [x >> 234]
        return [u + (m - 1) * v for u, v in zip(c, self.pl)]

    def value(self, l):
        """The field element that stored limbs stand for."""
        return sum(x << (26 * i) for i, x in enumerate(l)) * self.rinv % self.p

    def jac(self, rnd, pt, mags, lam=None):
        """(X, Y, Z limbs, inf) of pt in a random Jacobian representation at the given magnitudes."""
        if pt is None:
            return ZERO, ZERO, ZERO, 1
        lam = lam or rnd.randrange(1, self.p)
        m = [rnd.randint(1, k) if rnd.randrange(3) == 0 else k for k in mags]
        return (self.limbs(pt[0] * lam * lam, m[0]), self.limbs(pt[1] * lam**3, m[1]), self.limbs(lam, m[2]), 0)

    def aff(self, rnd, pt):
        return self.limbs(pt[0], rnd.randint(1, 2)), self.limbs(pt[1], rnd.randint(1, 2)), ZERO, 0


K1 = Curve(2**256 - 2**32 - 977, 0, 7, 1)
SM2 = Curve(2**256 - 2**224 - 2**96 + 2**64 - 1, -3,
            0x28E9FA9E9D9F5E344D5A9E4BCF6509A7F39789F515AB8F92DDBCBD414D940E93, R286)
P = K1.p
PL = K1.pl
GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
TABLE = [K1.mul(k, K1.mul(0x1234567, (GX, GY))) for k in range(1, 9)]  # 1 R .. 8 R

K1_OPS = ("dbl", "dbl_zz", "madd", "madd_zz", "add", "window", "chain_start", "scale", "add_z")
SM2_OPS = ("dbl_sm2", "dbl_sm2_d", "madd_sm2_d", "add_sm2_jd", "madd_sm2")
OPS = K1_OPS + SM2_OPS
# (X, Y, Z) magnitudes: entry contract, and what an ordinary result promises (the headers' own tables)
ENTRY = {"dbl": (10, 10, 16), "dbl_zz": (10, 10, 16), "madd": (10, 10, 16), "madd_zz": (10, 10, 16),
         "add": (16, 16, 16), "window": (16, 16, 16), "chain_start": (1, 1, 1), "scale": (16, 16, 16),
         "add_z": (16, 16, 16), "dbl_sm2": (5, 8, 8), "dbl_sm2_d": (12, 15, 15), "madd_sm2_d": (11, 11, 15),
         "add_sm2_jd": (15, 15, 15), "madd_sm2": (2, 2, 8)}
RESULT = {"dbl": (10, 10, 2), "dbl_zz": (10, 10, 2), "madd": (9, 6, 2), "madd_zz": (9, 6, 2), "add": (6, 4, 2),
          "window": (10, 10, 2), "chain_start": (10, 10, 2), "scale": (1, 1, 1), "add_z": (16, 16, 16),
          "dbl_sm2": (2, 2, 2), "dbl_sm2_d": (11, 11, 2), "madd_sm2_d": (11, 8, 2), "add_sm2_jd": (11, 8, 2),
          "madd_sm2": (2, 2, 2)}
# P = Q: the one-lane doubling's bound (CurveK1x::dbl; CurveSM2x::dbl weakly normalised by trio_madd_sm2)
DOUBLED = {"madd": (10, 10, 2), "add": (10, 10, 2), "madd_sm2": (2, 2, 2)}
KINDS = {"madd": ("eq", "neg", "pinf"), "add": ("eq", "neg", "pinf", "qinf", "both"), "madd_zz": ("pinf",),
         "window": ("pinf",), "scale": ("pinf",), "add_z": ("eq", "pinf", "qinf"), "madd_sm2_d": ("pinf",),
         "add_sm2_jd": ("pinf",), "madd_sm2": ("eq", "neg", "pinf")}


def curve_of(op):
    return SM2 if "sm2" in op else K1


def within(l, m):
    return all(x <= m << 26 for x in l[:9]) and l[9] <= m << 22


def limbs(x, m=1):
    return K1.limbs(x, m)


def value(l):
    return K1.value(l)


def jac(rnd, pt, mags):
    return K1.jac(rnd, pt, mags)


def one(rnd, op, kind="ord"):
    """One trio: dict(op, k, p, q, e, want, kind, mags, exact, extra).  exact: the (X, Y, Z) limbs an operand
    handed through must come back as; extra: what E must be (a value mod p, its magnitude, or exact limbs)."""
    C = curve_of(op)
    A, B = C.rand_point(rnd), C.rand_point(rnd)
    k = 0
    if kind in ("pinf", "both"):
        A = None
    if kind in ("qinf", "both"):
        B = None
    if kind == "eq":
        B = A
    if kind == "neg":
        B = C.neg(A)
    p = C.jac(rnd, A, ENTRY[op])
    q = (ZERO, ZERO, ZERO, 0)
    e = [ZERO, ZERO, ZERO]
    one_l = C.limbs(1)
    exact = extra = None
    mags = RESULT[op] if kind == "ord" else DOUBLED.get(op) if kind == "eq" else None
    z1 = C.value(p[2])
    if op in ("dbl", "dbl_zz", "dbl_sm2"):
        want = C.add(A, A)
    elif op in ("madd", "madd_sm2"):
        q, want = C.aff(rnd, B), C.add(A, B)
        if kind == "pinf":
            exact = (q[0], q[1], one_l)
    elif op == "madd_zz":
        e[0] = C.limbs(z1 * z1, rnd.randint(1, 4))
        q, want = C.aff(rnd, B), C.add(A, B)
        if kind == "pinf":
            exact = (q[0], q[1], one_l)
    elif op == "add":
        q, want = C.jac(rnd, B, ENTRY[op]), C.add(A, B)
        if kind == "pinf":
            exact = q[:3]
        if kind == "qinf":
            exact = p[:3]
    elif op == "window":
        k = rnd.randint(-8, 8)
        want = C.add(C.mul(16, A), C.mul(k, TABLE[0]))
        if kind == "pinf":
            mags = (1, 2, 1)  # the table point: x as stored, y or its neg<2>, Z = 1
    elif op == "chain_start":
        t = rnd.randint(0, 16)
        b = 1 if t == 16 else 0 if t == 0 else rnd.randrange(2)
        k = ((t - b) << 28) | (b << 27) | rnd.randrange(1 << 27)
        p, want = (ZERO, ZERO, ZERO, 0), C.mul(t, TABLE[0])
    elif op == "scale":
        # (X K, Y K l, Z K) is the point (X, Y, Z l) for K = l^2: build (X, Y, Z) so that Z l = mu
        l, mu = rnd.randrange(1, C.p), rnd.randrange(1, C.p)
        if A is not None:
            p = C.jac(rnd, A, ENTRY[op], lam=mu)
            p = (p[0], p[1], C.limbs(mu * pow(l, -1, C.p), rnd.choice((1, 16))), 0)
        e[0], e[1] = C.limbs(l * l, rnd.randint(1, 2)), C.limbs(l, rnd.randint(1, 2))
        want = A
        mags = (1, 1, 1)
    elif op == "add_z":
        q, want = C.jac(rnd, B, ENTRY[op]), None
        x1, y1, x2, z2 = C.value(p[0]), C.value(p[1]), C.value(q[0]), C.value(q[2])
        if kind == "pinf":
            extra = ("exact", q[2])
        elif kind == "qinf":
            extra = ("exact", p[2])
        elif kind == "eq":
            extra = ("value", 2 * y1 * z1 % C.p, 16)
        else:
            extra = ("value", 2 * z1 * z2 * (x2 * z1 * z1 - x1 * z2 * z2) % C.p, 16)
    elif op == "dbl_sm2_d":
        e[0] = C.limbs(z1 * z1)
        want = C.add(A, A)
    elif op == "madd_sm2_d":
        e[0] = C.limbs(z1 * z1)
        q, want = C.aff(rnd, B), C.add(A, B)
        if kind == "pinf":
            exact, extra = (q[0], q[1], one_l), ("exact", one_l)
    elif op == "add_sm2_jd":
        e[0] = C.limbs(z1 * z1)
        q = C.jac(rnd, B, (1, 1, 1))
        z2 = C.value(q[2])
        e[1], e[2] = C.limbs(z2 * z2), C.limbs(z2**3)
        want = C.add(A, B)
        if kind == "pinf":
            exact, extra = q[:3], ("exact", e[1])
    else:
        raise ValueError(op)
    if op in ("dbl_zz", "dbl_sm2_d", "madd_sm2_d", "add_sm2_jd") and extra is None:
        extra = ("zsquared", 4 if op == "dbl_zz" else 1)  # ZZ / D = Z3^2 of the result, at this magnitude
    return dict(op=op, k=k, p=p, q=q, e=e, want=want, kind=kind, mags=mags, exact=exact, extra=extra)


def trios(ops=K1_OPS):
    """The trios in wave order (20 to a wave, row-major), whole blocks of four waves."""
    rnd = random.Random(333 + len(ops))
    out = []

    def wave(op, special, base=None):
        """special: {(row, trio): kind}; everything else ordinary (fresh, or the base wave's own trios)."""
        w = []
        for r in range(4):
            for t in range(5):
                kind = special.get((r, t), "ord")
                w.append(base[5 * r + t] if base and kind == "ord" else one(rnd, op, kind))
        out.extend(w)
        return w

    for op in ops:
        for _ in range(N_RANDOM // 20 - 1):
            wave(op, {})
        base = wave(op, {})                          # none exceptional; the mixed waves below are copies of it
        kinds = KINDS.get(op, ())
        for kind in kinds:
            wave(op, {(0, 0): kind}, base)           # one exceptional trio among nineteen ordinary ones
            wave(op, {(3, 4): kind}, base)           # next to the phantom lane 63
            wave(op, {(0, 4): kind, (1, 2): kind, (2, 0): kind}, base)
        if kinds:
            wave(op, {(r, 4): kinds[r % len(kinds)] for r in range(3)}, base)  # a kind per row, row 3 ordinary
            wave(op, {(r, t): kinds[(5 * r + t) % len(kinds)] for r in range(4) for t in range(5)})  # all twenty
    if "window" in ops:
        # every digit of the window and every t of the chain start (the random draws above need not hit all)
        for d in range(-8, 9):
            for _ in range(4):
                c = one(rnd, "window")
                a16 = K1.add(c["want"], K1.mul(-c["k"], TABLE[0]))
                c["k"], c["want"] = d, K1.add(a16, K1.mul(d, TABLE[0]))
                out.append(c)
        for _ in range((-len(out)) % 20):
            out.append(one(rnd, "window"))
        for t in range(17):
            for b in ((1,) if t == 16 else (0,) if t == 0 else (0, 1)):
                c = one(rnd, "chain_start")
                c["k"], c["want"] = ((t - b) << 28) | (b << 27) | rnd.randrange(1 << 27), K1.mul(t, TABLE[0])
                out.append(c)
        for _ in range((-len(out)) % 20):
            out.append(one(rnd, "chain_start"))
    while len(out) % 80:
        wave(ops[0], {})
    return out


def _j(l):
    return ",".join("%x" % x for x in l)


def text(ts):
    head = "".join("table %s %s\n" % (_j(K1.limbs(x)), _j(K1.limbs(y))) for x, y in TABLE)
    return head + "".join("%s %d %s %s %s %d %s %s %s %d %s %s %s\n" % (
        (c["op"], c["k"]) + tuple(_j(x) for x in c["p"][:3]) + (c["p"][3],) + tuple(_j(x) for x in c["q"][:3])
        + (c["q"][3],) + tuple(_j(x) for x in c["e"])) for c in ts)


def check(c, line):
    C = curve_of(c["op"])
    f = line.split()
    assert len(f) == 5, (c["op"], line)
    X, Y, Z, E = ([int(x, 16) for x in f[i].split(",")] for i in (0, 1, 2, 4))
    inf = int(f[3])
    ctx = (c["op"], c["kind"], c["k"], line)
    ex = c["extra"]
    if c["op"] == "add_z":  # only Z3 is the answer
        if ex[0] == "exact":
            assert E == ex[1], ("Z3 handed through",) + ctx
        else:
            assert C.value(E) == ex[1] and within(E, ex[2]), ("Z3",) + ctx
        return
    assert inf in (0, 1) and inf == int(c["want"] is None), ("infinity flag",) + ctx
    if inf:
        return
    z = C.value(Z)
    assert z != 0, ctx
    zi = pow(z, -1, C.p)
    assert (C.value(X) * zi * zi % C.p, C.value(Y) * zi**3 % C.p) == c["want"], ("affine value",) + ctx
    if c["exact"] is not None:  # an operand handed through comes back limb for limb
        assert (X, Y, Z) == tuple(c["exact"]), ("operand handed through",) + ctx
    else:
        for l, m in zip((X, Y, Z), c["mags"]):
            assert within(l, m), ("magnitude", c["mags"]) + ctx
    if ex is not None:
        if ex[0] == "exact":
            assert E == ex[1], ("D handed through",) + ctx
        else:
            assert C.value(E) == z * z % C.p and within(E, ex[1]), ("ZZ / D = Z^2",) + ctx


def check_all(ts, lines):
    assert len(lines) == len(ts) and len(ts) % 80 == 0, (len(lines), len(ts))
    seen, answers = {}, {}
    for i, (c, line) in enumerate(zip(ts, lines)):
        check(c, line)
        key = (c["op"], c["kind"])
        seen[key] = seen.get(key, 0) + 1
        if c["kind"] != "ord" and i % 5 == 4:
            seen[(c["op"], c["kind"], "trio4")] = 1
        answers.setdefault(id(c), set()).add(line)
    for op in set(c["op"] for c in ts):
        for kind in KINDS.get(op, ()):
            assert (op, kind, "trio4") in seen, ("no %s in trio 4 of a row" % kind, op)
    # an ordinary trio gives the same limbs in an all-ordinary wave and in every mixed wave it sits in
    repeated = 0
    for c in ts:
        got = answers[id(c)]
        assert len(got) == 1, ("an ordinary trio's limbs change with the wave around it", c["op"], got)
    counts = {}
    for c in ts:
        counts[id(c)] = counts.get(id(c), 0) + 1
    repeated = sum(1 for n in counts.values() if n > 1)
    seen["repeated"] = repeated
    return seen
