"""The checkers of the GPU vector tests can fail: each one (tests/f26_vectors.py for f26vec, tests/mont_vectors.py
for fetest's Montgomery fields and inversions) is fed answers synthesised here with Python integers, which it
must accept, and then corruptions of them, each of which it must reject: a result limb (or word) off by one, a
value off by the modulus where a reduced result is required, and a third that keeps the value right but breaks
what else the op promises (a limb over the contract's magnitude, a flipped is_zero, a residue in the wrong
domain).  No GPU and no compiler: this is about the Python side alone."""
import pytest

import f26_vectors as fv
import mont_vectors as mv


def _f26_answer(case):
    fname, op, a, b, fam = case
    f = fv.FIELDS[fname]
    if op == "is_zero":
        return "%d" % (fv.value(a) % f.p == 0)
    want, _ = fv.expected(f, op, a, b)
    r = fv.limbs_of(want)
    if fam == "limb3" and r[3] == 0 and r[4] > 0:  # the representation fe26_reduce leaves for these operands
        r[3], r[4] = 1 << 26, r[4] - 1
    return ",".join("%x" % x for x in r)


def _limbs(line):
    return [int(x, 16) for x in line.split(",")]


def _line(limbs):
    return ",".join("%x" % x for x in limbs)


@pytest.fixture(scope="module")
def f26():
    cs = fv.cases()
    return cs, [_f26_answer(c) for c in cs]


def test_f26_checker_accepts_right_answers(f26):
    cs, ans = f26
    seen = fv.check_all(cs, ans)
    assert seen["limb3_hits"] > 0 and seen["random"] > 0


def _one_per_op(cs, ans, want_family):
    picked = {}
    for c, l in zip(cs, ans):
        if c[4] == want_family and c[1] != "is_zero":
            picked.setdefault((c[0], c[1]), (c, l))
    return list(picked.values())


def test_f26_checker_rejects_a_limb_off_by_one(f26):
    cs, ans = f26
    reps = _one_per_op(cs, ans, "random")
    assert len(reps) == sum(len(fv.op_list(f)) for f in fv.FIELDS.values()) - 2  # every op but the two is_zero
    for c, l in reps:
        for i in (0, 3, 9):
            for d in (1, -1):
                r = _limbs(l)
                r[i] += d
                if r[i] >= 0:
                    with pytest.raises(AssertionError):
                        fv.check(c, _line(r))


def test_f26_checker_rejects_a_value_off_by_p(f26):
    cs, ans = f26
    n = 0
    for c, l in zip(cs, ans):
        f = fv.FIELDS[c[0]]
        if c[1] in ("norm", "from_mont") and fv.value(_limbs(l)) + f.p < fv.M256:
            with pytest.raises(AssertionError):
                fv.check(c, _line(fv.limbs_of(fv.value(_limbs(l)) + f.p)))
            n += 1
    assert n > 50  # both fields' norm and fp26's from_mont: the lazy multiples of p and the small canonical values


def test_f26_checker_rejects_a_limb_over_its_magnitude_and_a_flipped_flag(f26):
    cs, ans = f26
    n = z = 0
    for c, l in zip(cs, ans):
        if c[1] == "is_zero":
            with pytest.raises(AssertionError):
                fv.check(c, "%d" % (1 - int(l)))
            z += 1
        elif c[1] in ("mul", "sqr", "to_mont", "inv", "sqrt_cand", "weak") and c[4] == "random":
            r = _limbs(l)
            if r[1] >= 2 and r[0] > 0:  # same value, limb 0 now above 2 * 2^26: over magnitude 1 (and weak's 2)
                r[0] += 2 << 26
                r[1] -= 2
                with pytest.raises(AssertionError):
                    fv.check(c, _line(r))
                n += 1
    assert n > 1000 and z > 1000


def test_f26_checker_rejects_split_roots_that_differ_from_the_chain(f26):
    cs, ans = f26
    f = fv.K1
    bad = list(ans)
    for i, c in enumerate(cs):
        if c[1] == "sqrt_split1" and fv.value(_limbs(ans[i])) not in (0,):
            # the other root: right as a square root, but not what the chain returns limb for limb
            bad[i] = _line(fv.limbs_of(f.p - fv.value(_limbs(ans[i]))))
            break
    with pytest.raises(AssertionError):
        fv.check_all(cs, bad)


def _row_answers(rs):
    """Right answers for tests/row_vectors.py's rows, in canonical limbs (under every bound the ops promise)."""
    import row_vectors as rv
    out = []
    for w in range(0, len(rs), 4):
        wave = rs[w:w + 4]
        op = wave[0][0]
        for r, (_, a, b, _) in enumerate(wave):
            p = rv.modulus(op)
            base, k = rv._split(op)
            A, Bv = rv.value(a), rv.value(b)
            if op in rv.WAVE_OPS:
                A0 = rv.value(wave[0][1])
                out.append(_line(rv.limbs_of(A0 % p)) if op == "to_fe26" else "%d" % (A0 % p == 0))
                continue
            if op in rv.GATHER_OPS:
                ins = [x[1] + [0] * 6 for x in wave]
                fb = b + [0] * 6
                if op == "sel4":
                    v = [ins[r], fb, [(x + y) & 0xFFFFFFFF for x, y in zip(ins[r], fb)], [x ^ y for x, y in zip(ins[r], fb)]][r]
                else:
                    v = ins[0] if op == "gather0" else ins[int(op[-1])]
                out.append(_line(v))
                continue
            if base == "from_fe26":
                v = a
            elif base == "from_words":
                v = rv.limbs_of(sum(x << (32 * i) for i, x in enumerate(a[:8])))
            else:
                want = {"mul": A * Bv, "mul_sm2": A * Bv, "sqr": A * A, "sqr_sm2": A * A, "add": A + Bv, "sub": A - Bv,
                        "sub_sm2": A - Bv, "neg": -A, "neg_sm2": -A, "mul_int": A * k}[base]
                v = rv.limbs_of(want % p)
            out.append(_line(v + [0] * 6))
    return out


@pytest.fixture(scope="module")
def row():
    import row_vectors as rv
    rs = rv.rows()
    return rs, _row_answers(rs)


def test_row_checker_accepts_right_answers(row):
    import row_vectors as rv
    rs, ans = row
    seen = rv.check_all(rs, ans)
    assert seen["random"] > 0 and seen["neighbour"] > 0


def test_row_checker_rejects_corruptions(row):
    import row_vectors as rv
    rs, ans = row
    picked = {}
    for (op, a, b, fam), l in zip(rs, ans):
        if fam == "random" and op in rv.ROW_OPS + ["from_fe26", "from_words"]:
            picked.setdefault(op, (op, a, b, l))
    assert len(picked) == len(rv.ROW_OPS) + 2
    for op, a, b, l in picked.values():
        r = _limbs(l)
        for i, d in ((0, 1), (9, 1), (10, 1), (15, 7)):  # a limb off by one; a nonzero lane 10, a nonzero lane 15
            bad = list(r)
            bad[i] += d
            with pytest.raises(AssertionError):
                rv.check_row(op, a, b, _line(bad))
        if op == "from_words" and rv.value(r[:10]) + rv.PK1 < 2**256:  # exact limbs required: off by p is wrong
            with pytest.raises(AssertionError):
                rv.check_row(op, a, b, _line(rv.limbs_of(rv.value(r[:10]) + rv.PK1) + [0] * 6))
        if op in ("mul", "sqr", "mul_sm2", "sqr_sm2") and r[1] >= 1:  # value right, limb 0 over the product's bound
            bad = list(r)
            bad[0] += 1 << 26
            bad[1] -= 1
            if bad[0] > rv.B:
                with pytest.raises(AssertionError):
                    rv.check_row(op, a, b, _line(bad))
    # a canonical value off by p where the zero test decides, and an answer that changes with the neighbours
    i = next(i for i, x in enumerate(rs) if x[0] == "is_zero" and x[3] == "case")
    bad = list(ans)
    bad[i:i + 4] = ["%d" % (1 - int(ans[i]))] * 4
    with pytest.raises(AssertionError):
        rv.check_all(rs, bad)
    i = next(i for i, x in enumerate(rs) if x[0] == "mul" and x[3] == "random")
    bad = list(ans)
    r = _limbs(ans[i])
    r[0], r[1] = (r[0] + (1 << 26), r[1] - 1) if r[1] else (r[0], r[1])
    assert r[1] != _limbs(ans[i])[1]
    bad[i] = _line(r)  # right value, other limbs than the same case gives in its other placements
    with pytest.raises(AssertionError):
        rv.check_all(rs, bad)


def _trio_answer(c, rnd):
    """A right answer for one of tests/trio_vectors.py's trios: the integer result in a random Jacobian form
    (an operand handed through: its own limbs), with the ZZ / D / Z3 the op returns."""
    import trio_vectors as tv
    C = tv.curve_of(c["op"])
    j = lambda l: ",".join("%x" % x for x in l)
    z = j(tv.ZERO)
    ex = c["extra"]
    if c["op"] == "add_z":
        return "%s %s %s 0 %s" % (z, z, z, j(ex[1] if ex[0] == "exact" else C.limbs(ex[1])))
    if c["want"] is None:
        return "%s %s %s 1 %s" % (z, z, z, z)
    X, Y, Z = c["exact"] if c["exact"] is not None else C.jac(rnd, c["want"], (1, 1, 1))[:3]
    E = tv.ZERO if ex is None else ex[1] if ex[0] == "exact" else C.limbs(C.value(Z) ** 2)
    return "%s %s %s 0 %s" % (j(X), j(Y), j(Z), j(E))


@pytest.fixture(scope="module", params=["k1", "sm2"])
def trio(request):
    import random
    import trio_vectors as tv
    ts = tv.trios(tv.K1_OPS if request.param == "k1" else tv.SM2_OPS)
    rnd = random.Random(7)
    once = {}  # a trio that sits in several waves answers with the same limbs each time
    for c in ts:
        if id(c) not in once:
            once[id(c)] = _trio_answer(c, rnd)
    return ts, [once[id(c)] for c in ts]


def test_trio_checker_accepts_right_answers(trio):
    import trio_vectors as tv
    ts, ans = trio
    seen = tv.check_all(ts, ans)
    assert seen["repeated"] >= 19 and any(len(k) == 3 and k[1] == "eq" for k in seen)


def test_trio_checker_rejects_corruptions(trio):
    import trio_vectors as tv
    ts, ans = trio
    n = flags = extras = 0
    for c, l in zip(ts[::7], ans[::7]):
        C = tv.curve_of(c["op"])
        f = l.split()
        if c["extra"] is not None:  # a wrong ZZ / delta / Z3: one limb off, and (where a value) off by p over its bound
            v = _limbs(f[4])
            v[0] += 1
            with pytest.raises(AssertionError):
                tv.check(c, " ".join(f[:4] + [_line(v)]))
            if c["extra"][0] != "exact" and (c["op"] == "add_z" or c["want"] is not None):
                v = [a + 16 * b for a, b in zip(_limbs(f[4]), C.pl)]
                with pytest.raises(AssertionError):
                    tv.check(c, " ".join(f[:4] + [_line(v)]))
            extras += 1
        if c["op"] == "add_z":
            continue
        flipped = " ".join(f[:3] + [str(1 - int(f[3]))] + f[4:])  # a wrong infinity flag
        with pytest.raises(AssertionError):
            tv.check(c, flipped)
        flags += 1
        if c["want"] is None:
            continue
        for i in (0, 1, 2):  # a coordinate limb off by one
            v = _limbs(f[i])
            v[0] += 1
            with pytest.raises(AssertionError):
                tv.check(c, " ".join(f[:i] + [_line(v)] + f[i + 1:]))
        # the same point, Z over any result's magnitude (value + 16 p, limb by limb): too large for an ordinary
        # or doubled result, and not the limbs of an operand handed through
        v = [a + 16 * b for a, b in zip(_limbs(f[2]), C.pl)]
        with pytest.raises(AssertionError):
            tv.check(c, " ".join(f[:2] + [_line(v)] + f[3:]))
        n += 1
    assert n > 150 and flags > n and extras > 50
    # an ordinary trio whose limbs differ between the ordinary wave and a mixed one (same point, other form)
    counts = {}
    for i, c in enumerate(ts):
        counts.setdefault(id(c), []).append(i)
    i = next(ix[1] for ix in counts.values() if len(ix) > 1 and ts[ix[0]]["want"] is not None
             and ts[ix[0]]["op"] != "add_z" and ts[ix[0]]["exact"] is None)
    bad = list(ans)
    import random
    bad[i] = _trio_answer(ts[i], random.Random(99))
    assert bad[i] != ans[i]
    with pytest.raises(AssertionError):
        tv.check_all(ts, bad)


@pytest.fixture(scope="module")
def mont():
    cs = mv.cases()
    return cs, ["%064x" % mv.expected(f, op, a, b) for f, op, a, b, _ in cs]


def test_mont_checker_accepts_right_answers(mont):
    cs, ans = mont
    seen = mv.check_all(cs, ans)
    assert seen["redc_mid"] == 300 and seen["top_hits"] >= 150


def test_mont_checker_rejects_corruptions(mont):
    cs, ans = mont
    off_one = off_m = domain = 0
    seen_ops = set()
    for c, l in zip(cs, ans):
        f, op, a, b, fam = c
        m = mv.MODULI[f]
        got = int(l, 16)
        if (f, op) not in seen_ops:  # a word off by one, low and high, once per field and op
            seen_ops.add((f, op))
            for bad in (got ^ 1, got ^ (1 << 255)):
                with pytest.raises(AssertionError):
                    mv.check(c, "%064x" % bad)
            off_one += 1
        if got + m < mv.R and off_m < 500:  # right mod m but not reduced
            with pytest.raises(AssertionError):
                mv.check(c, "%064x" % (got + m))
            off_m += 1
        if op in mv.MINV + mv.FERMAT and fam == "random" and domain < 500:  # the plain inverse of the stored value
            with pytest.raises(AssertionError):
                mv.check(c, "%064x" % pow(a, -1, m))
            domain += 1
    assert off_one == 3 * 14 + 3 and off_m == 500 and domain == 500
