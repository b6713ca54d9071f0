"""The lane-trio recovery kernel (csrc/ecc_coop.hip, tx_verify_trio26_kernel) with the square root split
between phase A and phase D (trio26_recover_body): forced with bcosgpu_set_tx_kernel_policy(1, 1, 2, 1)
at 1, 39, 40, 41 and 81 signatures -- one partial workgroup, one short of a full one, a full one (40 txs: the
20 / 21 boundary of its two wave pairs lies inside), one more than a workgroup, one more than two -- against
the oracle as test_gpu_row._check does.  The inputs are signed by the oracle, so every case's accepted and
rejected counts follow from the CPU alone; each test asserts that it saw both.  A size below 18 runs a pool
of 18 items in launches of that size, so that a one-signature launch still meets every kind of input."""
import numpy as np
import pytest

from test_gpu_ecc import N_SECP, _mutate

pytestmark = pytest.mark.gpu

TRIO = (1, 1, 2, 1)
SIZES = [1, 39, 40, 41, 81]
P_SECP = 2**256 - 2**32 - 977


@pytest.fixture
def trio_policy(gpu):
    gpu.set_tx_kernel_policy(*TRIO)
    yield
    gpu.set_tx_kernel_policy()


def _pool(n):
    return max(n, 18)


def _signed(oracle, rng, m):
    """m digests and their oracle signatures r || s || v (a zero and an all-ones digest among them)."""
    h = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
    h[0] = 0
    if m > 1:
        h[1] = 0xFF
    sig = np.zeros((m, 65), dtype=np.uint8)
    for i in range(m):
        sk = rng.integers(0, 256, size=32, dtype=np.uint8)
        sk[0] &= 0x7F
        sk[31] |= 1
        k = rng.integers(0, 256, size=32, dtype=np.uint8)
        k[0] &= 0x7F
        k[31] |= 1
        sig[i] = np.frombuffer(oracle.secp256k1_sign(sk.tobytes(), h[i].tobytes(), k.tobytes()), dtype=np.uint8)
    return h, sig


def _b32(x):
    return np.frombuffer(int(x % N_SECP).to_bytes(32, "big"), dtype=np.uint8)


def mutation_inputs(oracle, n):
    """The nine mutation kinds of test_gpu_ecc._mutate, kind = index mod 9."""
    rng = np.random.default_rng(0x7210 + n)
    h, sig = _signed(oracle, rng, _pool(n))
    arr = np.array([np.frombuffer(_mutate(rng, sig[i].tobytes(), i % 9), dtype=np.uint8) for i in range(len(sig))])
    return h, arr


def parity_inputs(oracle, n):
    """Valid signatures of both parities of v, and v = 2 / 3 with a small r (x = r + n, on the curve for
    about half of them), alternating."""
    rng = np.random.default_rng(0x7220 + n)
    h, sig = _signed(oracle, rng, _pool(n))
    for i in range(1, len(sig), 2):
        sig[i, 0:32] = np.frombuffer(int(rng.integers(1, 2**63)).to_bytes(32, "big"), dtype=np.uint8)
        sig[i, 64] = 2 + (i // 2) % 2
    return h, sig


def no_root_inputs(oracle, n):
    """Every second signature's r replaced by an x < n with x^3 + 7 a non-residue (by rejection with the
    oracle: with r, s in range and v < 2 a recovery fails for no other reason)."""
    rng = np.random.default_rng(0x7230 + n)
    h, sig = _signed(oracle, rng, _pool(n))
    for i in range(0, len(sig), 2):
        while True:
            r = int.from_bytes(rng.bytes(32), "big") % N_SECP or 1
            if pow((pow(r, 3, P_SECP) + 7) % P_SECP, (P_SECP - 1) // 2, P_SECP) != 1:
                break
        sig[i, 0:32] = _b32(r)
        assert oracle.secp256k1_recover(h[i].tobytes(), sig[i].tobytes()) is None
    return h, sig


def crafted_inputs(oracle, n):
    """test_gpu_row.test_row_recover_crafted_scalars' cases: R = k G for a known nonce, then u1 = 0 (e = 0,
    e = n), u2 = c, u2 = -c (one GLV half zero), Q = O (e = s k: fails), u1 G = u2 R (e = -s k: the last
    addition doubles)."""
    rng = np.random.default_rng(0x7240 + n)
    hs, sigs = [], []
    t = 0
    while len(hs) < _pool(n):
        t += 1
        k = int.from_bytes(rng.bytes(32), "big") % N_SECP or 1
        R = oracle.secp256k1_pubkey(k.to_bytes(32, "big"))
        rx, ry = int.from_bytes(R[:32], "big"), int.from_bytes(R[32:], "big")
        if rx >= N_SECP:
            continue
        r, v = rx, ry & 1
        s = int.from_bytes(rng.bytes(32), "big") % N_SECP or 1
        c = 1 + t % 12
        cases = [(0, s), (N_SECP, s), (int.from_bytes(rng.bytes(32), "big"), r * c),
                 (int.from_bytes(rng.bytes(32), "big"), r * (N_SECP - c)), (s * k, s), (-s * k, s)]
        for e, ss in cases:
            ss %= N_SECP
            if ss == 0:
                continue
            hs.append(np.frombuffer(int(e % 2**256).to_bytes(32, "big"), dtype=np.uint8) if e == N_SECP else _b32(e))
            sigs.append(np.concatenate([_b32(r), _b32(ss), np.array([v], dtype=np.uint8)]))
    m = _pool(n)
    return np.array(hs)[:m], np.array(sigs)[:m]


INPUTS = {"mutations": mutation_inputs, "parity": parity_inputs, "no_root": no_root_inputs, "crafted": crafted_inputs}


def _check(gpu, oracle, h, sig):
    pub, addr, okg = gpu.Secp256k1Crypto().recover_batch(h, sig, want_address=True)
    want_pub, want_ok = oracle.secp256k1_recover_batch(h, sig, nthreads=8)
    assert np.array_equal(okg, want_ok)
    assert np.array_equal(pub[want_ok], want_pub[want_ok])
    assert not pub[~want_ok].any() and not addr[~want_ok].any()
    for i in np.nonzero(want_ok)[0]:
        assert addr[i].tobytes() == oracle.keccak256(want_pub[i].tobytes())[12:], i
    return want_ok


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", sorted(INPUTS))
def test_trio_recover(gpu, oracle, trio_policy, kind, n):
    h, sig = INPUTS[kind](oracle, n)
    oks = [_check(gpu, oracle, h[a:a + n], sig[a:a + n]) for a in range(0, len(sig) - n + 1, n)]
    ok = np.concatenate(oks)
    assert ok.sum() > 0 and (~ok).sum() > 0
    if kind == "parity":  # both parities among the accepted plain signatures, and an accepted x = r + n
        v = sig[:len(ok), 64][ok]
        assert (v == 0).any() and (v == 1).any() and (v >= 2).any()


def tx_inputs(oracle, gpu_mod, n=41):
    """n transactions signed by the oracle over their Keccak256 hash: every tenth with a signature one byte
    short, a flipped s bit, or an r with no curve point."""
    rng = np.random.default_rng(0x7250)
    pres = [gpu_mod.TransactionData(version=int(rng.integers(0, 3)), chain_id="chain" + str(i % 7),
                                    group_id="group" * int(rng.integers(0, 4)), block_limit=int(rng.integers(0, 2**40)),
                                    nonce=str(int(rng.integers(0, 2**62))), to="ab" * int(rng.integers(0, 21)),
                                    input=rng.bytes(int(rng.integers(0, 400))), abi="x" * int(rng.integers(0, 50))
                                    ).preimage() for i in range(n)]
    sigs = []
    for i, p in enumerate(pres):
        sk = bytes([1 + i % 100]) + rng.bytes(31)
        k = bytes([1]) + rng.bytes(31)
        s = bytearray(oracle.secp256k1_sign(sk, oracle.keccak256(p), k))
        if i % 10 == 3:
            s = s[:-1]
        elif i % 10 == 5:
            s[40] ^= 4
        elif i % 10 == 7:
            s[0:32] = (5).to_bytes(32, "big")  # 5^3 + 7 = 132 is a non-residue mod p
        sigs.append(bytes(s))
    pre, pre_off = gpu_mod.pack_messages(pres)
    sg, sg_off = gpu_mod.pack_messages(sigs)
    return pre, pre_off, sg, sg_off


def test_trio_tx_verify_41(gpu, oracle, trio_policy):
    pre, pre_off, sg, sg_off = tx_inputs(oracle, gpu)
    th, snd, st = gpu.verify_packed(gpu.secp256k1_suite(), pre, pre_off, sg, sg_off)
    wh, ws, wst = oracle.tx_verify_packed(0, pre, pre_off, sg, sg_off, nthreads=8)
    assert np.array_equal(th, wh) and np.array_equal(st, wst) and np.array_equal(snd, ws)
    assert (wst == 0).sum() > 0 and (wst != 0).sum() > 0


def key_inputs(oracle, n=41):
    """n known-key verifications: valid, wrong digest, another key, high-S, in turn."""
    rng = np.random.default_rng(0x7260)
    h, sig = _signed(oracle, rng, n)
    pub = np.array([np.frombuffer(oracle.secp256k1_recover(h[i].tobytes(), sig[i].tobytes()), dtype=np.uint8)
                    for i in range(n)])
    for i in range(n):
        if i % 4 == 1:
            h[i, 5] ^= 0x10
        elif i % 4 == 2:
            pub[i] = pub[(i + 1) % n]
        elif i % 4 == 3:
            s = int.from_bytes(sig[i, 32:64].tobytes(), "big")
            sig[i, 32:64] = np.frombuffer((N_SECP - s).to_bytes(32, "big"), dtype=np.uint8)
    want = np.array([oracle.secp256k1_verify(pub[i].tobytes(), h[i].tobytes(), sig[i, :64].tobytes())
                     for i in range(n)])
    return pub, h, sig, want


def test_trio_known_key_verify_41(gpu, oracle, trio_policy):
    """bcosgpu_verify_batch on the trio kernel's known-key mode, which has no square root and keeps its
    schedule."""
    pub, h, sig, want = key_inputs(oracle)
    got = gpu.Secp256k1Crypto().verify_batch(pub, h, sig)
    assert np.array_equal(got, want)
    assert want.sum() > 0 and (~want).sum() > 0
