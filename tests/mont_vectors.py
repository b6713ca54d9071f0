"""Cases and checker for the Montgomery fields and the inversions of fisco-bcos_amd/tools/fetest.hip: FieldP2
(redc_sm2p), FieldN1, FieldN2 (Mont<> with mod_add_asm / mod_sub_asm) and the safegcd inversions of modinv.h.
The reference is Python integer arithmetic mod m; every comparison is exact, and since these ops return
residues in [0, m) with nothing normalised after them, a right value that is not reduced fails too.

A Montgomery residue is x R mod m with R = 2^256.  Operands are < m, as the contracts say.

Zero: Mont<>::inv and FieldP2::inv are Fermat powers (0^(m-2) = 0), and the safegcd variants return 0 for 0
(modinv.h says so at modinv_safegcd).  No kernel relies on either: the oracle rejects r = 0, s = 0 and the point
at infinity before an inversion is reached, and the kernels make the same range checks first; the value is
pinned here so that a change of it is seen."""
import random

R = 2**256
MODULI = {
    "k1": 2**256 - 2**32 - 977,
    "p2": 2**256 - 2**224 - 2**96 + 2**64 - 1,
    "n1": 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141,
    "n2": 0xFFFFFFFEFFFFFFFFFFFFFFFFFFFFFFFF7203DF6B21C6052B53BBF40939D54123,
}
MONT_FIELDS = ("p2", "n1", "n2")
BINARY = ("mul", "add", "sub")
UNARY = ("sqr", "neg", "from_plain", "to_plain")
FERMAT = ("inv",)
GCD = ("gcd", "gcd_pipe", "gcd_var")          # plain residue in, plain inverse out
MINV = ("minv", "minv_pipe", "minv_var")      # Montgomery residue in, Montgomery inverse out
N_RANDOM = 1000


def redc_raw(a, b, m):
    """The Montgomery product before its final subtraction, as Mont<>::mul and redc_sm2p form it:
    t = (a b + q m) / R with q = -(a b) / m mod R, 0 <= t < 2 m."""
    T = a * b
    q = (-T * pow(m, -1, R)) % R
    return (T + q * m) >> 256


def edges(m):
    out = [0, 1, 2, m - 2, m - 1, (m + 1) // 2]
    for k in range(256):
        out += [x for x in (2**k, 2**k - 1) if x < m]
    seen, uniq = set(), []
    for x in out:
        if x not in seen:
            seen.add(x)
            uniq.append(x)
    return uniq


def cases():
    """[(field, op, a, b, family)], seeded."""
    rnd = random.Random(256)
    out = []
    for f in MONT_FIELDS:
        m = MODULI[f]
        edge = edges(m)
        core = [0, 1, 2, m - 2, m - 1, (m + 1) // 2, 2**255, 2**255 - 1, 2**128, 2**128 - 1, 2**64, 2**64 - 1,
                2**32, 2**32 - 1, 2**224, 2**224 - 1]
        for op in BINARY:
            for a in core:
                for b in core:
                    out.append((f, op, a, b, "edge"))
            for a in edge:
                for b in (1, m - 1, (m + 1) // 2):
                    out.append((f, op, a, b, "edge"))
        for op in UNARY + FERMAT + GCD + MINV:
            for a in edge:
                out.append((f, op, a, 0, "edge"))
        # add: a + b just below, at and above m, across 2^256 (every modulus here has 2 m - 2 > 2^256), and
        # a + b - m with a borrow chain through j words; sub: a - b around 0 and a borrow through j words
        sums = [m - 2, m - 1, m, m + 1, R - 2, R - 1, R, R + 1, 2 * m - 2]
        sums += [m + 2**(32 * j) - d for j in range(1, 8) for d in (0, 1)]
        for s in sums:
            for _ in range(8):
                a = rnd.randrange(max(0, s - m + 1), min(m, s + 1))
                out.append((f, "add", a, s - a, "tail"))
        diffs = [-1, 0, 1, -(m - 1), m - 1] + [s * (2**(32 * j) - d) for j in range(1, 8) for d in (0, 1) for s in (1, -1)]
        for d in diffs:
            for _ in range(8):
                b = rnd.randrange(max(0, -d), min(m, m - d))
                out.append((f, "sub", b + d, b, "tail"))
        # mul: (m - 1)^2, and products whose value before the final subtraction lies in [m, 2 m): found by a
        # bounded search over the restated reduction (about one random pair in four), and, with the bit above
        # 2^256 set as well, operands just under m ([m, 2^256) alone is too thin a slice to search for: 2^128
        # wide for n1)
        out.append((f, "mul", m - 1, m - 1, "redc_top"))
        found = 0
        for _ in range(4000):
            if found == 100:
                break
            a, b = rnd.randrange(m), rnd.randrange(m)
            if redc_raw(a, b, m) >= m:
                out.append((f, "mul", a, b, "redc_mid"))
                out.append((f, "sqr", a, 0, "redc_any"))
                found += 1
        for _ in range(100):
            a, b = m - 1 - rnd.randrange(2**16), m - 1 - rnd.randrange(2**16)
            out.append((f, "mul", a, b, "redc_top"))
            out.append((f, "sqr", a, 0, "redc_any"))
        for op in BINARY + UNARY + FERMAT + GCD + MINV:
            for _ in range(N_RANDOM):
                out.append((f, op, rnd.randrange(m), rnd.randrange(m) if op in BINARY else 0, "random"))
    # FieldK1's inversions (FieldInv<FieldK1>: normalize, then one of these) on the secp256k1 prime
    m = MODULI["k1"]
    for op in GCD:
        for a in edges(m):
            out.append(("k1", op, a, 0, "edge"))
        for _ in range(N_RANDOM):
            out.append(("k1", op, rnd.randrange(m), 0, "random"))
    return out


def text(cs):
    return "".join("%s:%s %x %x\n" % (f, op, a, b) for f, op, a, b, _ in cs)


def expected(f, op, a, b):
    m = MODULI[f]
    rinv = pow(R, -1, m)
    if op == "mul":
        return a * b * rinv % m
    if op == "sqr":
        return a * a * rinv % m
    if op == "add":
        return (a + b) % m
    if op == "sub":
        return (a - b) % m
    if op == "neg":
        return -a % m
    if op == "from_plain":
        return a * R % m
    if op == "to_plain":
        return a * rinv % m
    if op in GCD:
        return pow(a, -1, m) if a else 0
    if op in FERMAT or op in MINV:  # a = x R -> x^-1 R = R^2 / a
        return R * R * pow(a, -1, m) % m if a else 0
    raise ValueError(op)


def check(case, line):
    f, op, a, b, fam = case
    assert len(line) == 64, (case, line)
    got = int(line, 16)
    want = expected(f, op, a, b)
    assert got == want, (f, op, fam, hex(a), hex(b), hex(got), hex(want))


def check_all(cs, lines):
    assert len(lines) == len(cs), (len(lines), len(cs))
    seen = {}
    for case, line in zip(cs, lines):
        check(case, line)
        f, op, a, b, fam = case
        seen[fam] = seen.get(fam, 0) + 1
        m = MODULI[f]
        # the search did find what it was for: the subtraction taken without and with the bit above 2^256
        if fam == "redc_mid":
            assert m <= redc_raw(a, b, m) < 2 * m, case
        if fam == "redc_top":
            seen["top_hits"] = seen.get("top_hits", 0) + (redc_raw(a, b, m) >= R)
    assert seen.get("top_hits", 0) >= 3 * 50, seen
    return seen
