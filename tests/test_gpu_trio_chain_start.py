"""The lane-trio kernel's chain start (trio_chain_start: the two top Booth digits of a GLV half as one
table load, one doubling and one addition) against the oracle, byte for byte, through the three entry
points that share the kernel body: Transaction::verify (TxIO: tx hash, sender, status), the recovery batch
(SigIO) and the known-key verification.  Batches of 1, 39, 40, 41 and 81 signatures: one lane, a workgroup
minus / exactly / plus one, two workgroups plus one.

Each batch mixes, in turn: random signatures; signatures whose u2 = s / r is built from chosen GLV halves
(u2 = k1 + k2 lambda, s = u2 r) -- both halves below 2^123 (top nibble 0 and bit 123 clear: t = 0, the chain
starts at infinity), k1 = 0, k2 = 0, and halves at the corner of the split's range; and invalid rows: r = 0,
an r that is the x of no curve point, v = 2.

The chain start's t = (top nibble) + (bit 123) reaches 16 only for a half of at least 15.5 * 2^124.  No
signature gives one: secp256k1's lambda split returns the coset's vector inside the lattice's fundamental
cell, |k1| <= (a1 + a2) / 2 + 1 < 0.64 * 2^128 and |k2| <= (-b1 + b2) / 2 + 1 < 0.55 * 2^128, so the top
nibble is at most 10.  The "corner" rows take the largest halves that exist (0.49 of either basis vector
each: top nibble 9 for k1, 8 for k2, asserted below with the split redone in Python); t from
11 to 16 is covered on the CPU (tests/test_trio_chain_start.py), for every t in 0..16."""
import numpy as np
import pytest

from test_gpu_ecc import N_SECP
from test_gpu_trio_split import P_SECP, TRIO, _b32, _signed

pytestmark = pytest.mark.gpu

SIZES = [1, 39, 40, 41, 81]
POOL = 81
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
# the lattice basis of the split: a + b lambda = 0 (mod n) for (A1, -MB1) and (A2, A1)
A1 = 0x3086D221A7D46BCDE86C90E49284EB15
MB1 = 0xE4437ED6010E88286F547FA90ABFE4C3
A2 = 0x114CA50F7A8E2F3F657C1108D9D44CFD8
KINDS = ["random", "low", "corner", "k1_zero", "k2_zero", "r_zero", "no_point", "v2", "corner2"]


@pytest.fixture
def trio_policy(gpu):
    gpu.set_tx_kernel_policy(*TRIO)
    yield
    gpu.set_tx_kernel_policy()


def split(k):
    """The lambda split of k (nearest lattice vector by rounding): signed halves with k = k1 + k2 lambda."""
    c1 = (2 * k * A1 + N_SECP) // (2 * N_SECP)    # round(k b2 / n), b2 = a1
    c2 = (2 * k * MB1 + N_SECP) // (2 * N_SECP)   # round(k (-b1) / n)
    k1 = k - c1 * A1 - c2 * A2
    k2 = c1 * MB1 - c2 * A1
    assert (k1 + k2 * LAMBDA - k) % N_SECP == 0
    return k1, k2


def test_lattice_constants():
    assert (A1 - MB1 * LAMBDA) % N_SECP == 0 and (A2 + A1 * LAMBDA) % N_SECP == 0
    assert A1 * A1 + MB1 * A2 == N_SECP  # the basis spans the whole lattice
    assert pow(LAMBDA, 3, N_SECP) == 1


def halves(rng, kind):
    """The chosen GLV halves (signed) of a crafted row, or None."""
    s1, s2 = (1 if rng.integers(0, 2) else -1), (1 if rng.integers(0, 2) else -1)
    if kind == "low":
        return s1 * int(rng.integers(1, 2**62)) * 2**61, s2 * (int(rng.integers(1, 2**62)) * 2**61 + 1)
    if kind == "k1_zero":
        return 0, s2 * (int.from_bytes(rng.bytes(15), "big") | 1)
    if kind == "k2_zero":
        return s1 * (int.from_bytes(rng.bytes(15), "big") | 1), 0
    if kind == "corner":   # 0.49 (v1 + v2): the largest k1
        x, y = s1 * 49, s1 * 49
    elif kind == "corner2":  # 0.49 (v2 - v1): the largest k2
        x, y = -s1 * 49, s1 * 49
    else:
        return None
    j = int.from_bytes(rng.bytes(12), "big")
    return (x * A1 + y * A2) // 100 + j, (-x * MB1 + y * A1) // 100 - j


def check_halves(kind, u2, want):
    k1, k2 = split(u2)
    if kind in ("low", "k1_zero", "k2_zero"):
        assert (k1, k2) == want, kind  # halves this short are the cell's own
    if kind == "low":
        assert 0 < abs(k1) < 2**123 and 0 < abs(k2) < 2**123
    if kind == "corner":
        assert (k1, k2) == want and abs(k1) >> 124 >= 9
    if kind == "corner2":
        assert (k1, k2) == want and abs(k2) >> 124 >= 8


def nonce_point(oracle, rng):
    while True:
        k = int.from_bytes(rng.bytes(32), "big") % N_SECP or 1
        R = oracle.secp256k1_pubkey(k.to_bytes(32, "big"))
        rx, ry = int.from_bytes(R[:32], "big"), int.from_bytes(R[32:], "big")
        if rx < N_SECP:
            return rx, ry & 1


def craft(oracle, rng, kind, sig):
    """Row `sig` (a valid r || s || v) turned into the row of its kind; recovery's chain scalar is s / r."""
    if kind == "random":
        return sig
    if kind == "r_zero":
        sig[0:32] = 0
    elif kind == "no_point":
        while True:
            r = int.from_bytes(rng.bytes(32), "big") % N_SECP or 1
            if pow((pow(r, 3, P_SECP) + 7) % P_SECP, (P_SECP - 1) // 2, P_SECP) != 1:
                break
        sig[0:32] = _b32(r)
    elif kind == "v2":
        sig[0:32] = np.frombuffer(int(rng.integers(1, 2**63)).to_bytes(32, "big"), dtype=np.uint8)
        sig[64] = 2
    else:
        want = halves(rng, kind)
        u2 = (want[0] + want[1] * LAMBDA) % N_SECP
        check_halves(kind, u2, want)
        r, v = nonce_point(oracle, rng)
        sig[0:32] = _b32(r)
        sig[32:64] = _b32(u2 * r)
        sig[64] = v
    return sig


_cache = {}


def recover_pool(oracle):
    """81 digests and signatures, kind = index mod 9, and the oracle's recovery of them (made once)."""
    if "rec" not in _cache:
        rng = np.random.default_rng(0x7310)
        h, sig = _signed(oracle, rng, POOL)
        for i in range(POOL):
            sig[i] = craft(oracle, rng, KINDS[i % len(KINDS)], sig[i].copy())
        want_pub, want_ok = oracle.secp256k1_recover_batch(h, sig, nthreads=8)
        for i in range(POOL):  # the crafted rows run their chains to an accepted key; the invalid ones fail
            kind = KINDS[i % len(KINDS)]
            assert want_ok[i] == (kind not in ("r_zero", "no_point")) or kind == "v2", (i, kind)
        _cache["rec"] = (h, sig, want_pub, want_ok)
    return _cache["rec"]


def _slices(n):
    """The launches of a size: the first n of the pool, and for one signature a launch per kind."""
    return [(a, a + n) for a in range(0, len(KINDS) if n == 1 else 1)]


@pytest.mark.parametrize("n", SIZES)
def test_chain_start_recover(gpu, oracle, trio_policy, n):
    h, sig, want_pub, want_ok = recover_pool(oracle)
    seen = np.zeros(0, dtype=bool)
    for a, b in _slices(n):
        pub, addr, okg = gpu.Secp256k1Crypto().recover_batch(h[a:b], sig[a:b], want_address=True)
        ok = want_ok[a:b]
        assert np.array_equal(okg, ok)
        assert np.array_equal(pub[ok], want_pub[a:b][ok])
        assert not pub[~ok].any() and not addr[~ok].any()
        for i in np.nonzero(ok)[0]:
            assert addr[i].tobytes() == oracle.keccak256(want_pub[a + i].tobytes())[12:], (a, i)
        seen = np.concatenate([seen, ok])
    assert seen.sum() > 0 and (~seen).sum() > 0


def tx_pool(oracle, gpu_mod):
    """81 transactions; the signature of row i is the recovery pool's kind over the tx's own hash."""
    if "tx" not in _cache:
        rng = np.random.default_rng(0x7320)
        pres = [gpu_mod.TransactionData(version=int(rng.integers(0, 3)), chain_id="chain" + str(i % 7),
                                        group_id="group" * int(rng.integers(0, 4)),
                                        block_limit=int(rng.integers(0, 2**40)), nonce=str(int(rng.integers(0, 2**62))),
                                        to="ab" * int(rng.integers(0, 21)), input=rng.bytes(int(rng.integers(0, 300))),
                                        abi="x" * int(rng.integers(0, 50))).preimage() for i in range(POOL)]
        sigs = []
        for i, p in enumerate(pres):
            sk = bytes([1 + i % 100]) + rng.bytes(31)
            k = bytes([1]) + rng.bytes(31)
            s = np.frombuffer(oracle.secp256k1_sign(sk, oracle.keccak256(p), k), dtype=np.uint8).copy()
            sigs.append(craft(oracle, rng, KINDS[i % len(KINDS)], s).tobytes())
        _cache["tx"] = (pres, sigs)
    return _cache["tx"]


@pytest.mark.parametrize("n", SIZES)
def test_chain_start_tx_verify(gpu, oracle, trio_policy, n):
    pres, sigs = tx_pool(oracle, gpu)
    good = bad = 0
    for a, b in _slices(n):
        pre, pre_off = gpu.pack_messages(pres[a:b])
        sg, sg_off = gpu.pack_messages(sigs[a:b])
        th, snd, st = gpu.verify_packed(gpu.secp256k1_suite(), pre, pre_off, sg, sg_off)
        wh, ws, wst = oracle.tx_verify_packed(0, pre, pre_off, sg, sg_off, nthreads=8)
        assert np.array_equal(th, wh) and np.array_equal(st, wst) and np.array_equal(snd, ws)
        good += int((wst == 0).sum())
        bad += int((wst != 0).sum())
    assert good > 0 and bad > 0


def key_pool(oracle):
    """81 known-key verifications, whose chain scalar is r / s on the key: valid signatures, and for the
    crafted kinds an s = r / u2 with the chosen halves (rejected, after the whole chain has run); r = 0, an
    r >= n and a high s as the invalid rows."""
    if "key" not in _cache:
        rng = np.random.default_rng(0x7330)
        h, sig = _signed(oracle, rng, POOL)
        pub = np.array([np.frombuffer(oracle.secp256k1_recover(h[i].tobytes(), sig[i].tobytes()), dtype=np.uint8)
                        for i in range(POOL)])
        for i in range(POOL):
            kind = KINDS[i % len(KINDS)]
            if kind == "r_zero":
                sig[i, 0:32] = 0
            elif kind == "no_point":
                sig[i, 0:32] = 0xFF  # r >= n
            elif kind == "v2":
                s = int.from_bytes(sig[i, 32:64].tobytes(), "big")
                sig[i, 32:64] = _b32(N_SECP - s)
            elif kind != "random":
                want = halves(rng, kind)
                u2 = (want[0] + want[1] * LAMBDA) % N_SECP
                check_halves(kind, u2, want)
                r = int.from_bytes(sig[i, 0:32].tobytes(), "big")
                sig[i, 32:64] = _b32(r * pow(u2, -1, N_SECP))
        want = np.array([oracle.secp256k1_verify(pub[i].tobytes(), h[i].tobytes(), sig[i, :64].tobytes())
                         for i in range(POOL)])
        _cache["key"] = (pub, h, sig, want)
    return _cache["key"]


@pytest.mark.parametrize("n", SIZES)
def test_chain_start_known_key(gpu, oracle, trio_policy, n):
    pub, h, sig, want = key_pool(oracle)
    seen = np.zeros(0, dtype=bool)
    for a, b in _slices(n):
        got = gpu.Secp256k1Crypto().verify_batch(pub[a:b], h[a:b], sig[a:b])
        assert np.array_equal(got, want[a:b])
        seen = np.concatenate([seen, want[a:b]])
    assert seen.sum() > 0 and (~seen).sum() > 0
