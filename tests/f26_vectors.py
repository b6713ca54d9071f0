"""Cases and checker for fisco-bcos_amd/tools/f26vec.hip: the 10 x 26-bit fields fe26 (secp256k1) and fp26
(SM2, Montgomery with R = 2^286) one operation at a time, on operands given as raw limbs so that
non-canonical, bound-hugging representations reach the code.  The reference is Python integer arithmetic
mod p and nothing else; every comparison is exact.  Shared by the GPU test (the device build, where mul and
sqr are the generated asm blocks of fe_asm.h), the CPU test of the tool's host leg, and the checker's own
test.

Magnitude (fe26.h / fp26.h): an element has magnitude m when limbs 0..8 are <= m 2^26 and limb 9 <= m 2^22.
Each op's accepted input magnitudes and promised output magnitude below restate the headers' contract
tables."""
import random

PK1 = 2**256 - 2**32 - 977
PP2 = 2**256 - 2**224 - 2**96 + 2**64 - 1
R286 = 2**286
M256 = 2**256

# the K of sub<K> / neg<K> and the C of mul_int<C> instantiated by ec26.h, ecp26.h, ec26_trio.h, ecp26_trio.h,
# recover26.h, verify_sm2_26.h, ecc_device.h and the kernels (grep 'f[ep]26_(sub|neg|mul_int)<'); f26vec.hip's
# dispatch has exactly these
SUB_K = {"k1": (2, 3, 4, 6, 7, 9, 10, 11), "p2": (2, 3, 4, 8, 9, 12, 13)}
NEG_K = {"k1": (2,), "p2": (2,)}
MUL_INT_C = {"k1": (2, 3, 4, 8, 16), "p2": (2, 3, 4, 8, 12)}
SQRT_OPS = ("sqrt_cand", "sqrt_split0", "sqrt_split1")  # the whole chain, and head<CUT> + tail<CUT> for both cuts
BOUND_MS = (1, 2, 3, 4, 8, 10)
N_RANDOM = 500


class Field:
    def __init__(self, name, p, mul_max, sub_extra):
        self.name, self.p, self.mul_max, self.sub_extra = name, p, mul_max, sub_extra
        self.plimbs = limbs_of(p)
        self.rinv = 1 if name == "k1" else pow(R286, -1, p)


def limbs_of(x):
    """Canonical limbs of 0 <= x < 2^256."""
    assert 0 <= x < M256
    return [(x >> (26 * i)) & 0x3FFFFFF for i in range(9)] + [x >> 234]


def value(limbs):
    return sum(x << (26 * i) for i, x in enumerate(limbs))


def magnitude(limbs):
    """The smallest magnitude that holds the limbs (at least 1)."""
    return max([1] + [-(-x >> 26) for x in limbs[:9]] + [-(-limbs[9] >> 22)])


def within(limbs, m):
    return all(x <= m << 26 for x in limbs[:9]) and limbs[9] <= m << 22


def canonical(limbs, p):
    return all(x < 1 << 26 for x in limbs[:9]) and limbs[9] < 1 << 22 and value(limbs) < p


K1 = Field("k1", PK1, 16, 0)
P2 = Field("p2", PP2, 15, 1)  # fp26's K p is written with every limb >= (K - 1) 2^26, one magnitude more
FIELDS = {"k1": K1, "p2": P2}


def op_list(f):
    ops = ["mul", "sqr", "add", "weak", "norm", "is_zero"]
    ops += ["sub%d" % k for k in SUB_K[f.name]] + ["neg%d" % k for k in NEG_K[f.name]]
    ops += ["mul_int%d" % c for c in MUL_INT_C[f.name]]
    ops += list(SQRT_OPS) if f.name == "k1" else ["to_mont", "from_mont", "inv"]
    return ops


def _split(op):
    for pre in ("mul_int", "sub", "neg"):
        if op.startswith(pre) and op[len(pre):].isdigit():
            return pre, int(op[len(pre):])
    return op, 0


def contract(f, op):
    """(binary, amax, bmax(ma)): the input magnitudes the header's table accepts."""
    base, k = _split(op)
    if base in ("mul",):
        return True, f.mul_max, lambda ma: f.mul_max
    if base in ("sqr", "to_mont", "from_mont") or op in SQRT_OPS:
        return False, f.mul_max, None
    if base == "add":
        return True, 62, lambda ma: 63 - ma
    if base in ("weak", "norm", "is_zero", "inv"):  # inv normalises its operand first (fp26_to_fe)
        return False, 63, None
    if base == "sub":
        return True, 63 - k - f.sub_extra, lambda ma: k - 1
    if base == "neg":
        return False, k - 1, None
    if base == "mul_int":
        return False, 63 // k, None
    raise ValueError(op)


def bound(m):
    return [m << 26] * 9 + [m << 22]


def single(i, m):
    r = [0] * 10
    r[i] = m << (22 if i == 9 else 26)
    return r


def lazy_kp(f, k, delta=0):
    """k p added limb by limb (magnitude k), plus delta in limb 0."""
    r = [k * x for x in f.plimbs]
    r[0] += delta
    return r


def rand_limbs(rnd, m):
    """Uniform limbs of magnitude m; one time in three every limb sits within 3 of its bound."""
    if rnd.randrange(3) == 0:
        return [x - rnd.randrange(4) for x in bound(m)]
    return [rnd.randrange((m << 26) + 1) for _ in range(9)] + [rnd.randrange((m << 22) + 1)]


ZERO = [0] * 10


def limb3_candidates(rnd):
    """Operands whose fe26 product leaves limb 3 at exactly 2^26, the case fe26_reduce's comment names: the
    first carry pass leaves limbs 1..3 all ones and a unit above 2^256, whose fold (64 into limb 1) ripples
    into limb 3 after its mask.  a = (x0, ones, ones, ones, ..., 2^22 in limb 9) times b = 1 does that when
    x0 is small; the family varies x0 and the free limbs, and the tests assert that the search hit."""
    out = []
    for _ in range(40):
        a = [rnd.randrange(1 << 12), 0x3FFFFFF, 0x3FFFFFF, 0x3FFFFFF] + [rnd.randrange(1 << 26) for _ in range(5)]
        a.append(1 << 22)
        out.append((a, limbs_of(1)))
        out.append((limbs_of(1), a))
    return out


def cases():
    """[(field, op, a limbs, b limbs, family)] in a fixed order (seeded)."""
    rnd = random.Random(2626)
    out = []
    for f in (K1, P2):
        canon = [limbs_of(x) for x in (f.p - 1, f.p, f.p + 1, M256 - 1, 0, 1)]
        sqrt_ops_seen = []
        for op in op_list(f):
            if op in SQRT_OPS[1:]:
                # the split chains take the very operands of sqrt_cand: head then tail is limb for limb the chain
                out += [(f.name, op, a, b, fam) for (_, o, a, b, fam) in sqrt_ops_seen]
                continue
            binary, amax, bmax = contract(f, op)
            mine = []

            def put(a, b, fam):
                assert within(a, amax) and (not binary or within(b, bmax(magnitude(a)))), (op, fam)
                mine.append((f.name, op, a, b if binary else ZERO, fam))

            top_a = 31 if op == "add" else amax  # add: both operands near the middle of a + b <= 63
            for m in sorted(set(x for x in BOUND_MS + (amax,) if x <= amax)):
                put(bound(m), bound(min(m, bmax(m))) if binary else ZERO, "bound")
            if binary:
                put(bound(top_a), bound(bmax(top_a)), "bound")
                put(bound(1), bound(bmax(1)), "bound")
            for i in range(10):
                put(single(i, top_a), bound(bmax(top_a)) if binary else ZERO, "single")
                if binary:
                    put(bound(top_a), single(i, bmax(top_a)), "single")
            if op == "mul":
                for i in range(10):
                    for j in range(10):
                        put(single(i, amax), single(j, amax), "single")
            for k in range(1, amax + 1):
                for d in (0, 1, -1):
                    put(lazy_kp(f, k, d), canon[0], "kp")
            for a in canon:
                for b in canon if binary else [ZERO]:
                    put(a, b, "canon")
            if f is K1 and op == "mul":
                for a, b in limb3_candidates(rnd):
                    put(a, b, "limb3")
            for _ in range(N_RANDOM):
                ma = rnd.randint(1, amax)
                a = rand_limbs(rnd, ma)
                put(a, rand_limbs(rnd, rnd.randint(1, bmax(magnitude(a)))) if binary else ZERO, "random")
            if op == "sqrt_cand":
                sqrt_ops_seen = mine
            out += mine
    return out


def text(cs):
    return "".join("%s %s %s %s\n" % (f, op, ",".join("%x" % x for x in a), ",".join("%x" % x for x in b))
                   for f, op, a, b, _ in cs)


def expected(f, op, a, b):
    """(value mod p, output magnitude or 0 for canonical) by integer arithmetic."""
    p, A, B = f.p, value(a), value(b)
    base, k = _split(op)
    ma, mb = magnitude(a), magnitude(b)
    if base == "mul":
        return A * B * f.rinv % p, 1
    if base == "sqr":
        return A * A * f.rinv % p, 1
    if base == "add":
        return (A + B) % p, ma + mb
    if base == "weak":
        return A % p, 2
    if base == "norm":
        return A % p, 0
    if base == "sub":
        return (A - B) % p, ma + k + f.sub_extra
    if base == "neg":
        return -A % p, k + f.sub_extra
    if base == "mul_int":
        return A * k % p, ma * k
    if base == "to_mont":
        return A * R286 % p, 1
    if base == "from_mont":
        return A * f.rinv % p, 0
    if base == "inv":  # a = x R  ->  x^-1 R = R^2 / a; a = 0 (mod p) gives 0, as the safegcd does for 0
        return (R286 * R286 * pow(A, -1, p) % p if A % p else 0), 1
    if op in SQRT_OPS:
        return pow(A, (p + 1) // 4, p), 1
    raise ValueError(op)


def check(case, line, host=False):
    """Asserts that one output line of f26vec answers one case.  host: the host leg, which cannot run the
    device-only `inv` and says "na" for it."""
    fname, op, a, b, fam = case
    f = FIELDS[fname]
    ctx = (fname, op, fam, a, b, line)
    if op == "inv" and host:
        assert line == "na", ctx
        return
    if op == "is_zero":
        assert line in ("0", "1"), ctx
        assert int(line) == int(value(a) % f.p == 0), ctx
        return
    r = [int(x, 16) for x in line.split(",")]
    assert len(r) == 10, ctx
    want, mout = expected(f, op, a, b)
    assert value(r) % f.p == want, ctx
    if mout == 0:
        assert canonical(r, f.p), ctx
    else:
        assert within(r, mout), ctx + (mout,)
    if op == "weak":
        # beyond magnitude 2, the headers' own statement: limbs 0..8 carried, at most 2^6 above limb 9's
        # 22 bits (the carry out of limb 8 of a magnitude-63 operand), so the value is < 2^256 + 2^240 < 2p
        assert all(x < 1 << 26 for x in r[:9]) and r[9] < (1 << 22) + 64, ctx
    if op in SQRT_OPS:
        # the caller's test: the candidate squares to the operand exactly when the operand is a residue
        A = value(a) % f.p
        residue = A == 0 or pow(A, (f.p - 1) // 2, f.p) == 1
        assert (value(r) ** 2 % f.p == A) == residue, ctx


def check_all(cs, lines, host=False):
    """Every line against its case, then what only the whole run shows.  Returns per-family counts."""
    assert len(lines) == len(cs), (len(lines), len(cs))
    seen, limb3_hits, roots = {}, 0, {}
    for case, line in zip(cs, lines):
        check(case, line, host)
        fname, op, a, _, fam = case
        seen[fam] = seen.get(fam, 0) + 1
        if fam == "limb3" and int(line.split(",")[3], 16) == 1 << 26:
            limb3_hits += 1
        if op in SQRT_OPS:
            roots.setdefault(tuple(a), {})[op] = line
    # the search found operands that leave limb 3 at exactly 2^26, and this build ran them
    assert limb3_hits > 0, "no product left limb 3 at 2^26"
    # head<CUT> then tail<CUT> is limb for limb the whole chain
    for a, got in roots.items():
        assert len(set(got.values())) == 1 and len(got) == 3, (a, got)
    seen["limb3_hits"] = limb3_hits
    return seen
