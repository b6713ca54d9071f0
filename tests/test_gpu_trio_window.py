"""The lane-trio kernel's lean window (trio_window, ec26_trio.h: sign-flipping doublings, the unscaled mixed
addition, the infinite accumulator behind a wave-uniform branch) against the oracle, byte for byte, through
the three entry points that share the kernel body: Transaction::verify (TxIO: tx hash, sender, status), the
recovery batch (SigIO) and the known-key verification.  Batches of 1, 39, 40, 41 and 81 signatures: one lane,
a workgroup minus / exactly / plus one, two workgroups plus one.

Rows (test_gpu_trio_chain_start.py's kinds): random signatures; crafted GLV halves -- "low" (both halves below
2^123: the accumulator is infinite for the first windows), k1 = 0 and k2 = 0 (a chain that stays infinite to
its end), the corner halves; the invalid rows r = 0, an r that is the x of no curve point, v = 2.  Two more
batches of one workgroup each make the kernel's `any(accumulator infinite)` branch go one way for whole
waves: 40 "low" rows (every trio of every wave starts infinite) and 40 "high" rows, crafted with both halves
between 2^123 and 2^125 (no trio does: about one random half in twenty is below 2^123; asserted below with the
split redone in Python)."""
import numpy as np
import pytest

from test_gpu_ecc import N_SECP
from test_gpu_trio_chain_start import KINDS, LAMBDA, check_halves, craft, halves, nonce_point, split
from test_gpu_trio_split import TRIO, _b32, _signed

pytestmark = pytest.mark.gpu

SIZES = [1, 39, 40, 41, 81]
POOL = 81
# the mixed pool (kind = index mod 9), a workgroup of "low" rows only, a workgroup with no infinite start
POOLS = {"mixed": [KINDS[i % len(KINDS)] for i in range(POOL)], "low": ["low"] * 40, "none": ["high"] * 40}


def halves_w(rng, kind):
    if kind != "high":
        return halves(rng, kind)
    s1, s2 = (1 if rng.integers(0, 2) else -1), (1 if rng.integers(0, 2) else -1)
    return s1 * (2**123 + int.from_bytes(rng.bytes(15), "big") * 8), s2 * (2**123 + int.from_bytes(rng.bytes(15), "big") * 8)


def craft_w(oracle, rng, kind, sig):
    if kind != "high":
        return craft(oracle, rng, kind, sig)
    want = halves_w(rng, kind)
    u2 = (want[0] + want[1] * LAMBDA) % N_SECP
    assert split(u2) == want
    r, v = nonce_point(oracle, rng)
    sig[0:32] = _b32(r)
    sig[32:64] = _b32(u2 * r)
    sig[64] = v
    return sig


@pytest.fixture
def trio_policy(gpu):
    gpu.set_tx_kernel_policy(*TRIO)
    yield
    gpu.set_tx_kernel_policy()


_cache = {}


def _starts_infinite(u2):
    """Whether either GLV chain of the scalar u2 starts at infinity (t = top nibble + bit 123 = 0)."""
    return any(abs(k) < 2**123 for k in split(u2))


def _check_none(sig):
    for s in sig:
        r, sv = int.from_bytes(s[0:32].tobytes(), "big"), int.from_bytes(s[32:64].tobytes(), "big")
        assert not _starts_infinite(sv * pow(r, -1, N_SECP) % N_SECP)


def recover_pool(oracle, name):
    key = ("rec", name)
    if key not in _cache:
        kinds = POOLS[name]
        rng = np.random.default_rng(0x7410 + len(name))
        h, sig = _signed(oracle, rng, len(kinds))
        for i, kind in enumerate(kinds):
            sig[i] = craft_w(oracle, rng, kind, sig[i].copy())
        if name == "none":
            _check_none(sig)
        want_pub, want_ok = oracle.secp256k1_recover_batch(h, sig, nthreads=8)
        for i, kind in enumerate(kinds):
            assert want_ok[i] == (kind not in ("r_zero", "no_point")) or kind == "v2", (i, kind)
        _cache[key] = (h, sig, want_pub, want_ok)
    return _cache[key]


def _slices(n):
    """The launches of a size: the first n of the pool, and for one signature a launch per kind."""
    return [(a, a + n) for a in range(0, len(KINDS) if n == 1 else 1)]


def _check_recover(gpu, oracle, pool, a, b):
    h, sig, want_pub, want_ok = pool
    pub, addr, okg = gpu.Secp256k1Crypto().recover_batch(h[a:b], sig[a:b], want_address=True)
    ok = want_ok[a:b]
    assert np.array_equal(okg, ok)
    assert np.array_equal(pub[ok], want_pub[a:b][ok])
    assert not pub[~ok].any() and not addr[~ok].any()
    for i in np.nonzero(ok)[0]:
        assert addr[i].tobytes() == oracle.keccak256(want_pub[a + i].tobytes())[12:], (a, i)
    return ok


@pytest.mark.parametrize("n", SIZES)
def test_window_recover(gpu, oracle, trio_policy, n):
    pool = recover_pool(oracle, "mixed")
    seen = np.concatenate([_check_recover(gpu, oracle, pool, a, b) for a, b in _slices(n)])
    assert seen.sum() > 0 and (~seen).sum() > 0


@pytest.mark.parametrize("name", ["low", "none"])
def test_window_recover_uniform_workgroup(gpu, oracle, trio_policy, name):
    assert _check_recover(gpu, oracle, recover_pool(oracle, name), 0, 40).all()


def tx_pool(oracle, gpu_mod, name):
    """Transactions whose signature is the pool's kind over the tx's own hash."""
    key = ("tx", name)
    if key not in _cache:
        kinds = POOLS[name]
        rng = np.random.default_rng(0x7420 + len(name))
        pres = [gpu_mod.TransactionData(version=int(rng.integers(0, 3)), chain_id="chain" + str(i % 7),
                                        group_id="group" * int(rng.integers(0, 4)),
                                        block_limit=int(rng.integers(0, 2**40)), nonce=str(int(rng.integers(0, 2**62))),
                                        to="ab" * int(rng.integers(0, 21)), input=rng.bytes(int(rng.integers(0, 300))),
                                        abi="x" * int(rng.integers(0, 50))).preimage() for i in range(len(kinds))]
        sigs = []
        for i, p in enumerate(pres):
            sk = bytes([1 + i % 100]) + rng.bytes(31)
            k = bytes([1]) + rng.bytes(31)
            s = np.frombuffer(oracle.secp256k1_sign(sk, oracle.keccak256(p), k), dtype=np.uint8).copy()
            sigs.append(craft_w(oracle, rng, kinds[i], s))
        if name == "none":
            _check_none(sigs)
        _cache[key] = (pres, [s.tobytes() for s in sigs])
    return _cache[key]


def _check_tx(gpu, oracle, pool, a, b):
    pres, sigs = pool
    pre, pre_off = gpu.pack_messages(pres[a:b])
    sg, sg_off = gpu.pack_messages(sigs[a:b])
    th, snd, st = gpu.verify_packed(gpu.secp256k1_suite(), pre, pre_off, sg, sg_off)
    wh, ws, wst = oracle.tx_verify_packed(0, pre, pre_off, sg, sg_off, nthreads=8)
    assert np.array_equal(th, wh) and np.array_equal(st, wst) and np.array_equal(snd, ws)
    return wst == 0


@pytest.mark.parametrize("n", SIZES)
def test_window_tx_verify(gpu, oracle, trio_policy, n):
    pool = tx_pool(oracle, gpu, "mixed")
    seen = np.concatenate([_check_tx(gpu, oracle, pool, a, b) for a, b in _slices(n)])
    assert seen.sum() > 0 and (~seen).sum() > 0


@pytest.mark.parametrize("name", ["low", "none"])
def test_window_tx_verify_uniform_workgroup(gpu, oracle, trio_policy, name):
    _check_tx(gpu, oracle, tx_pool(oracle, gpu, name), 0, 40)


def key_pool(oracle, name):
    """Known-key verifications, whose chain scalar is r / s on the key: valid signatures, and for the crafted
    kinds an s = r / u2 with the chosen halves (rejected, after the whole chain has run); r = 0, an r >= n and
    a high s as the invalid rows."""
    key = ("key", name)
    if key not in _cache:
        kinds = POOLS[name]
        rng = np.random.default_rng(0x7430 + len(name))
        h, sig = _signed(oracle, rng, len(kinds))
        pub = np.array([np.frombuffer(oracle.secp256k1_recover(h[i].tobytes(), sig[i].tobytes()), dtype=np.uint8)
                        for i in range(len(kinds))])
        for i, kind in enumerate(kinds):
            if kind == "r_zero":
                sig[i, 0:32] = 0
            elif kind == "no_point":
                sig[i, 0:32] = 0xFF  # r >= n
            elif kind == "v2":
                s = int.from_bytes(sig[i, 32:64].tobytes(), "big")
                sig[i, 32:64] = _b32(N_SECP - s)
            elif kind != "random":
                want = halves_w(rng, kind)
                u2 = (want[0] + want[1] * LAMBDA) % N_SECP
                if kind != "high":
                    check_halves(kind, u2, want)
                r = int.from_bytes(sig[i, 0:32].tobytes(), "big")
                sig[i, 32:64] = _b32(r * pow(u2, -1, N_SECP))
        if name == "none":
            for s in sig:
                r, sv = int.from_bytes(s[0:32].tobytes(), "big"), int.from_bytes(s[32:64].tobytes(), "big")
                assert not _starts_infinite(r * pow(sv, -1, N_SECP) % N_SECP)
        want = np.array([oracle.secp256k1_verify(pub[i].tobytes(), h[i].tobytes(), sig[i, :64].tobytes())
                         for i in range(len(kinds))])
        _cache[key] = (pub, h, sig, want)
    return _cache[key]


@pytest.mark.parametrize("n", SIZES)
def test_window_known_key(gpu, oracle, trio_policy, n):
    pub, h, sig, want = key_pool(oracle, "mixed")
    seen = np.zeros(0, dtype=bool)
    for a, b in _slices(n):
        got = gpu.Secp256k1Crypto().verify_batch(pub[a:b], h[a:b], sig[a:b])
        assert np.array_equal(got, want[a:b])
        seen = np.concatenate([seen, want[a:b]])
    assert seen.sum() > 0 and (~seen).sum() > 0


@pytest.mark.parametrize("name", ["low", "none"])
def test_window_known_key_uniform_workgroup(gpu, oracle, trio_policy, name):
    pub, h, sig, want = key_pool(oracle, name)
    got = gpu.Secp256k1Crypto().verify_batch(pub, h, sig)
    assert np.array_equal(got, want)
