"""Cases and checker for fisco-bcos_amd/tools/rowvec.hip: the row-spread fields of fe_row.h (one limb per lane
of a 16-lane DPP row, lanes 10..15 zero) and the row helpers of ec_row.h.  The code is device-only, so the
GPU test is its only execution; the reference is Python integer arithmetic mod p, every comparison exact.

Both row fields hold PLAIN residues: frow::mul folds with 2^260 = 2^36 + R0 (mod p), and frow::mul_sm2 folds
the high columns through kSm2RowM[j] = 2^(26 (10 + j)) mod p, plain residues of the weights themselves, so
mul_sm2(a, b) = a b mod p with no Montgomery factor (unlike fp26).

Row magnitude m (fe_row.h): EVERY limb, limb 9 included, is <= m B with B = 2^26 + 2^16.
  mul, sqr (both fields): inputs m <= 16 -> lanes 10..15 zero and, secp256k1: limbs 0..8 < 2^26 + 2^14, limb 9
                          < 2^26 + 2^15.1; SM2: every limb <= B
  add: m_a + m_b;  mul_int<C>: C m;  sub<K> / sub_sm2<K>: b.m <= K - 1 -> m_a + K;  neg<K>: m <= K - 1 -> K
A wave runs one op on its four rows; the rows are independent, which the cases check by running every case
once between three all-zero rows and once between three rows with every limb at the op's bound, and the
random cases a third time four to a wave: the three answers must be the same limbs."""
import random

PK1 = 2**256 - 2**32 - 977
PP2 = 2**256 - 2**224 - 2**96 + 2**64 - 1
B = 2**26 + 2**16
LIMB9_K1 = 2**26 + 35120  # 2^15.1 = 35119.9...
SUB_K = (2, 3, 7, 9, 10, 11)  # ec_row.h's sub<K> (grep 'sub<'), for both fields through FK1 / FSM2
NEG_K = (2,)
MUL_INT_C = (2, 3, 4, 8)
N_RANDOM = 500
BOUND_MS = (1, 2, 4, 8, 16)
ZERO = [0] * 10

Q_K1 = [0x3FFC2F0, 0x3FFFBFF] + [0x3FFFFFF] * 8
Q_SM2 = [0x3FFFFF0, 0x3FFFFFF, 0x400FFFF, 0x3BFFFFF, 0x3FFFFFF, 0x3FFFFFF, 0x3FFFFFF, 0x3FFFFFF, 0x3EFFFFF, 0x3FFFFFF]


def value(limbs):
    return sum(x << (26 * i) for i, x in enumerate(limbs))


assert value(Q_K1) == 16 * PK1 and value(Q_SM2) == 16 * PP2

ROW_OPS = (["mul", "sqr", "mul_sm2", "sqr_sm2", "add"] + ["sub%d" % k for k in SUB_K] + ["sub_sm2%d" % k for k in SUB_K]
           + ["neg%d" % k for k in NEG_K] + ["neg_sm2%d" % k for k in NEG_K] + ["mul_int%d" % c for c in MUL_INT_C])
WAVE_OPS = ("to_fe26", "is_zero", "is_zero_sm2")  # of row 0's element, answered on every row
GATHER_OPS = ("gather4_0", "gather4_1", "gather4_2", "gather4_3", "gather01_0", "gather01_1", "gather0", "sel4")


def limbs_of(x):
    assert 0 <= x < 2**256
    return [(x >> (26 * i)) & 0x3FFFFFF for i in range(9)] + [x >> 234]


def magnitude(limbs):
    return max([1] + [-(-x // B) for x in limbs])


def within(limbs, m):
    return all(x <= m * B for x in limbs)


def bound(m):
    return [m * B] * 10


def single(i, m):
    r = [0] * 10
    r[i] = m * B
    return r


def _split(op):
    for pre in ("sub_sm2", "neg_sm2", "mul_int", "sub", "neg"):
        if op.startswith(pre) and op[len(pre):].isdigit():
            return pre, int(op[len(pre):])
    return op, 0


def modulus(op):
    return PP2 if "sm2" in op else PK1


def contract(op):
    """(binary, amax, bmax(ma))."""
    base, k = _split(op)
    if base in ("mul", "mul_sm2"):
        return True, 16, lambda ma: 16
    if base in ("sqr", "sqr_sm2") or op in WAVE_OPS:
        return False, 16, None
    if base == "add":
        return True, 62, lambda ma: 63 - ma
    if base in ("sub", "sub_sm2"):
        return True, 63 - k, lambda ma: k - 1
    if base in ("neg", "neg_sm2"):
        return False, k - 1, None
    if base == "mul_int":
        return False, 63 // k, None
    raise ValueError(op)


def rand_limbs(rnd, m):
    if rnd.randrange(3) == 0:
        return [m * B - rnd.randrange(4) for _ in range(10)]
    return [rnd.randrange(m * B + 1) for _ in range(10)]


def op_cases(op, rnd):
    """[(a, b, family)] for one op."""
    binary, amax, bmax = contract(op)
    p = modulus(op)
    out = []

    def put(a, b, fam):
        assert within(a, amax) and (not binary or within(b, bmax(magnitude(a)))), (op, fam)
        out.append((a, b if binary else ZERO, fam))

    top = 31 if op == "add" else amax
    for m in sorted(set(x for x in BOUND_MS + (amax,) if x <= amax)):
        put(bound(m), bound(min(m, bmax(m))) if binary else ZERO, "bound")
    if binary:
        put(bound(top), bound(bmax(top)), "bound")
    for i in range(10):
        put(single(i, top), bound(bmax(top)) if binary else ZERO, "single")
        if binary:
            put(bound(top), single(i, bmax(top)), "single")
    pl = limbs_of(p)
    for k in range(1, min(amax, 16) + 1):  # multiples of p in row form: k p limb by limb, and k p +- 1
        for d in (0, 1, -1):
            a = [k * x for x in pl]
            a[0] += d
            put(a, limbs_of(p - 1), "kp")
    for a in (p - 1, p, 2**256 - 1, 0, 1):
        put(limbs_of(a), limbs_of(p - 1), "canon")
    for _ in range(N_RANDOM):
        a = rand_limbs(rnd, rnd.randint(1, amax))
        put(a, rand_limbs(rnd, rnd.randint(1, bmax(magnitude(a)))) if binary else ZERO, "random")
    return out


def rows():
    """[(op, a, b, family)], four consecutive entries a wave with one op (what rowvec reads)."""
    rnd = random.Random(1616)
    out = []
    for op in ROW_OPS:
        binary, amax, bmax = contract(op)
        top = 31 if op == "add" else amax
        hot = (bound(top), bound(bmax(top)) if binary else ZERO, "neighbour")
        cold = (ZERO, ZERO, "neighbour")
        cs = op_cases(op, rnd)
        for i, c in enumerate(cs):
            for nb in (cold, hot):
                wave = [nb] * 4
                wave[i % 4] = c
                out += [(op,) + w for w in wave]
        rand = [c for c in cs if c[2] == "random"]
        assert len(rand) % 4 == 0
        out += [(op,) + c for c in rand]  # four different cases per wave
    for op in ("from_fe26", "from_words"):
        for _ in range(64):
            if op == "from_words":
                x = rnd.choice([0, 1, PK1 - 1, PK1, PP2, 2**256 - 1, rnd.randrange(2**256), rnd.randrange(2**256)])
                a = [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [0, 0]
            else:
                a = [rnd.randrange(2**32) for _ in range(10)]
            out.append((op, a, ZERO, "random"))
    for op in GATHER_OPS:
        for _ in range(64):
            out.append((op, [rnd.randrange(2**32) for _ in range(10)], [rnd.randrange(2**32) for _ in range(10)], "random"))
    for op in WAVE_OPS:
        p = modulus(op)
        pl, ql = limbs_of(p), (Q_SM2 if p == PP2 else Q_K1)
        cs = [bound(m) for m in BOUND_MS] + [single(i, 16) for i in range(10)]
        for k in range(1, 17):
            for d in (0, 1, -1):
                a = [k * x for x in pl]
                a[0] += d
                cs.append(a)
            cs.append([min(k, 15) * x for x in ql])  # k Q = 16 k p with digits near 2^26 (15 Q is the most under 16 B)
        cs += [limbs_of(x) for x in (p - 1, p, p + 1, 2**256 - 1, 0, 1)]
        cs += [rand_limbs(rnd, rnd.randint(1, 16)) for _ in range(N_RANDOM)]
        for a in cs:
            assert within(a, 16), op
            for nb in (ZERO, bound(16)):
                out.append((op, a, ZERO, "case"))
                out += [(op, nb, ZERO, "neighbour")] * 3
    assert len(out) % 4 == 0
    return out


def text(rs):
    return "".join("%s %s %s\n" % (op, ",".join("%x" % x for x in a), ",".join("%x" % x for x in b)) for op, a, b, _ in rs)


def check_row(op, a, b, line):
    """One row of a per-row op: sixteen lane values."""
    ctx = (op, a, b, line)
    r = [int(x, 16) for x in line.split(",")]
    assert len(r) == 16, ctx
    assert r[10:] == [0] * 6, ("lanes 10..15",) + ctx
    r = r[:10]
    base, k = _split(op)
    p = modulus(op)
    A, Bv, ma, mb = value(a), value(b), magnitude(a), magnitude(b)
    if base == "from_fe26":
        assert r == a, ctx
        return
    if base == "from_words":
        assert r == limbs_of(sum(w << (32 * i) for i, w in enumerate(a[:8]))), ctx
        return
    want, mout = {"mul": (A * Bv, 1), "mul_sm2": (A * Bv, 1), "sqr": (A * A, 1), "sqr_sm2": (A * A, 1),
                  "add": (A + Bv, ma + mb), "sub": (A - Bv, ma + k), "sub_sm2": (A - Bv, ma + k), "neg": (-A, k),
                  "neg_sm2": (-A, k), "mul_int": (A * k, ma * k)}[base]
    assert value(r) % p == want % p, ctx
    assert within(r, mout), ctx
    if base in ("mul", "sqr"):
        assert all(x < 2**26 + 2**14 for x in r[:9]) and r[9] < LIMB9_K1, ("product limb bound",) + ctx


def check_all(rs, lines):
    assert len(lines) == len(rs) and len(rs) % 4 == 0, (len(lines), len(rs))
    seen, answers, done = {}, {}, set()
    for w in range(0, len(rs), 4):
        wave, got = rs[w:w + 4], lines[w:w + 4]
        op = wave[0][0]
        for (o, a, b, fam), line in zip(wave, got):
            seen[fam] = seen.get(fam, 0) + 1
        if op in GATHER_OPS:
            ins = [a + [0] * 6 for _, a, _, _ in wave]
            for r, ((_, a, b, _), line) in enumerate(zip(wave, got)):
                out = [int(x, 16) for x in line.split(",")]
                if op == "sel4":
                    full_b = b + [0] * 6
                    want = [ins[r], full_b, [(x + y) & 0xFFFFFFFF for x, y in zip(ins[r], full_b)],
                            [x ^ y for x, y in zip(ins[r], full_b)]][r]
                else:
                    want = ins[int(op[-1])] if op != "gather0" else ins[0]
                assert out == want, (op, r, line)
        elif op in WAVE_OPS:
            a, p = wave[0][1], modulus(op)
            assert len(set(got)) == 1, (op, a, got)  # every row sees the same answer
            if op == "to_fe26":
                r = [int(x, 16) for x in got[0].split(",")]
                assert len(r) == 10 and value(r) % p == value(a) % p, (op, a, got[0])
                assert all(x <= 2 << 26 for x in r[:9]) and r[9] <= 2 << 22, (op, a, got[0])  # fe26 magnitude 2
            else:
                assert got[0] in ("0", "1") and int(got[0]) == int(value(a) % p == 0), (op, a, got[0])
            answers.setdefault((op, tuple(a)), set()).add(got[0])
        else:
            for (o, a, b, fam), line in zip(wave, got):
                key = (o, tuple(a), tuple(b), line)
                if key not in done:
                    check_row(o, a, b, line)
                    done.add(key)
                answers.setdefault((o, tuple(a), tuple(b)), set()).add(line)
    # a row's answer does not depend on what the other three rows hold
    for key, got in answers.items():
        assert len(got) == 1, ("depends on the neighbouring rows", key, got)
    return seen
