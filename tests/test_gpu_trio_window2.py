"""The lane-trio kernels' window (trio_window, ec26_trio.h) after its role selects share their mask set-up
(trio::csel: the wave mask lives in VCC across the blocks of one role, one s_nop per ten limbs) against the
oracle, byte for byte, through Transaction::verify (TxIO), the recovery batch (SigIO) and the known-key
verification, at 1, 39, 40, 41 and 81 signatures.  The change is in the device's instruction stream only, so
this is where it is checked: a select that ran under another role's mask, or that read a limb too early, gives a
wrong point in the window where it happened.

The GLV halves are crafted as tests/test_gpu_glv_split.py crafts u2 (u2 = k1 + k2 lambda, s = u2 r for a
recovery, s = r / u2 for a known key; the split is redone in Python and must return the chosen halves):
  * every Booth digit -8 .. 8 of the radix-16 chain in the top window of the loop (window 30: the chain's start
    takes digits 32 and 31), in an interior window (15) and in the lowest one (0), in chain 0 with chain 1
    random and the reverse, under a random sign of the half (the table entry's sign is the digit's times the
    half's).  Window 0 has no bit below it, so its digit is -8 .. 7: 8 is left out there, and there only;
  * leading windows that are all zero: k1 < 16 with k2 = 0, and the reverse (30 windows of an infinite
    accumulator, then one digit);
  * a workgroup whose rows all start infinite and one whose rows never do (test_gpu_trio_window's pools)."""
import numpy as np
import pytest

import test_gpu_trio_window as w1
from test_gpu_ecc import N_SECP
from test_gpu_trio_chain_start import LAMBDA, nonce_point, split
from test_gpu_trio_helpers import check_recover, check_tx
from test_gpu_trio_split import TRIO, _b32, _signed

pytestmark = pytest.mark.gpu

SIZES = [1, 39, 40, 41, 81]
WINDOWS = (30, 15, 0)


def booth_digits(k):
    """The digits of windows 30 .. 0 of a half's magnitude, as booth_digit128 (ecc_device.h) gives them."""
    out = {}
    for w in range(30, -1, -1):
        nib = (k >> (4 * w)) & 15
        c = (k >> (4 * w - 1)) & 1 if w else 0
        out[w] = nib + c - 16 * (nib >> 3)
    return out


def half_with_digit(rng, w, d):
    """A magnitude below 2^124 whose Booth digit of window w is d."""
    c = 1 if d == 8 else 0
    nib = (d - c) % 16
    k = int.from_bytes(rng.bytes(16), "big") >> 5  # 123 random bits
    k &= ~(15 << (4 * w))
    k |= nib << (4 * w)
    if w:
        k = (k & ~(1 << (4 * w - 1))) | (c << (4 * w - 1))
    assert booth_digits(k)[w] == d
    return k


def crafted_halves():
    """(k1, k2, label) of every crafted row: signed halves that the lambda split returns as they are."""
    rng = np.random.default_rng(0x7710)
    rows = []
    for w in WINDOWS:
        for d in range(-8, 9):
            if w == 0 and d == 8:
                continue
            for chain in (0, 1):
                while True:
                    k = [int.from_bytes(rng.bytes(16), "big") >> 5 | 1, int.from_bytes(rng.bytes(16), "big") >> 5 | 1]
                    k[chain] = half_with_digit(rng, w, d)
                    k = [x * (1 if rng.integers(0, 2) else -1) for x in k]
                    if k[chain] and split((k[0] + k[1] * LAMBDA) % N_SECP) == (k[0], k[1]):
                        break
                rows.append((k[0], k[1], "w%d d%d c%d" % (w, d, chain)))
    for small in (1, 7, 8, 9, 15):
        for sgn in (1, -1):
            rows.append((sgn * small, 0, "k1 %d" % (sgn * small)))
            rows.append((0, sgn * small, "k2 %d" % (sgn * small)))
    for k1, k2, label in rows:
        assert split((k1 + k2 * LAMBDA) % N_SECP) == (k1, k2), label
    return rows


def test_every_digit_is_in_the_pool():
    seen = {(w, c): set() for w in WINDOWS for c in (0, 1)}
    for k1, k2, label in crafted_halves():
        if label.startswith("w"):
            w, d, c = (int(x[1:]) for x in label.split())
            assert booth_digits(abs((k1, k2)[c]))[w] == d
            seen[(w, c)].add(d)
    for (w, c), ds in seen.items():
        assert ds == set(range(-8, 8 if w == 0 else 9)), (w, c)


@pytest.fixture
def trio_policy(gpu):
    gpu.set_tx_kernel_policy(*TRIO)
    yield
    gpu.set_tx_kernel_policy()


_cache = {}


def _pool_rows():
    """The crafted rows with a random row after every fourth, cut to whole multiples of the largest size."""
    rows = []
    for i, r in enumerate(crafted_halves()):
        rows.append(r)
        if i % 4 == 3:
            rows.append(None)
    return rows


def _craft(oracle, rng, row, sig):
    if row is None:
        return sig
    u2 = (row[0] + row[1] * LAMBDA) % N_SECP
    r, v = nonce_point(oracle, rng)
    sig[0:32] = _b32(r)
    sig[32:64] = _b32(u2 * r)
    sig[64] = v
    return sig


def recover_pool(oracle):
    if "rec" not in _cache:
        rows = _pool_rows()
        rng = np.random.default_rng(0x7720)
        h, sig = _signed(oracle, rng, len(rows))
        for i, row in enumerate(rows):
            sig[i] = _craft(oracle, rng, row, sig[i].copy())
        want_pub, want_ok = oracle.secp256k1_recover_batch(h, sig, nthreads=8)
        assert want_ok.all()  # every chain runs to an accepted key
        _cache["rec"] = (h, sig, want_pub, want_ok)
    return _cache["rec"]


def tx_pool(oracle, gpu_mod):
    if "tx" not in _cache:
        rows = _pool_rows()
        rng = np.random.default_rng(0x7730)
        pres = [gpu_mod.TransactionData(version=int(rng.integers(0, 3)), chain_id="chain" + str(i % 7),
                                        group_id="group" * int(rng.integers(0, 4)),
                                        block_limit=int(rng.integers(0, 2**40)), nonce=str(int(rng.integers(0, 2**62))),
                                        to="ab" * int(rng.integers(0, 21)), input=rng.bytes(int(rng.integers(0, 300))),
                                        abi="x" * int(rng.integers(0, 50))).preimage() for i in range(len(rows))]
        sigs = []
        for i, p in enumerate(pres):
            sk = bytes([1 + i % 100]) + rng.bytes(31)
            k = bytes([1]) + rng.bytes(31)
            s = np.frombuffer(oracle.secp256k1_sign(sk, oracle.keccak256(p), k), dtype=np.uint8).copy()
            sigs.append(_craft(oracle, rng, rows[i], s).tobytes())
        _cache["tx"] = (pres, sigs, {})
    return _cache["tx"]


def key_pool(oracle):
    """Known-key verifications: the chain scalar is r / s on the key, so a crafted row takes s = r / u2 (rejected,
    after the whole chain has run); the random rows are valid."""
    if "key" not in _cache:
        rows = _pool_rows()
        rng = np.random.default_rng(0x7740)
        h, sig = _signed(oracle, rng, len(rows))
        pub = np.array([np.frombuffer(oracle.secp256k1_recover(h[i].tobytes(), sig[i].tobytes()), dtype=np.uint8)
                        for i in range(len(rows))])
        for i, row in enumerate(rows):
            if row is not None:
                u2 = (row[0] + row[1] * LAMBDA) % N_SECP
                r = int.from_bytes(sig[i, 0:32].tobytes(), "big")
                sig[i, 32:64] = _b32(r * pow(u2, -1, N_SECP))
        want = np.array([oracle.secp256k1_verify(pub[i].tobytes(), h[i].tobytes(), sig[i, :64].tobytes())
                         for i in range(len(rows))])
        _cache["key"] = (pub, h, sig, want)
    return _cache["key"]


def _launches(n, total):
    """Launches of n rows that together cover the whole pool (the last one ends with the pool)."""
    starts = list(range(0, total - n + 1, n))
    if starts[-1] + n < total:
        starts.append(total - n)
    return [(a, a + n) for a in starts]


@pytest.mark.parametrize("n", SIZES)
def test_window2_recover(gpu, oracle, trio_policy, n):
    pool = recover_pool(oracle)
    for a, b in _launches(n, len(pool[0])):
        assert check_recover(gpu, oracle, pool, a, b).all()


@pytest.mark.parametrize("n", SIZES)
def test_window2_tx_verify(gpu, oracle, trio_policy, n):
    pool = tx_pool(oracle, gpu)
    for a, b in _launches(n, len(pool[0])):
        assert check_tx(gpu, oracle, pool, a, b).all()


@pytest.mark.parametrize("n", SIZES)
def test_window2_known_key(gpu, oracle, trio_policy, n):
    pub, h, sig, want = key_pool(oracle)
    assert want.sum() > 0 and (~want).sum() > 0
    for a, b in _launches(n, len(pub)):
        got = gpu.Secp256k1Crypto().verify_batch(pub[a:b], h[a:b], sig[a:b])
        assert np.array_equal(got, want[a:b])


@pytest.mark.parametrize("name", ["low", "none"])
def test_window2_uniform_workgroup(gpu, oracle, trio_policy, name):
    """40 rows that all start infinite / of which none does, through the three entry points."""
    assert w1._check_recover(gpu, oracle, w1.recover_pool(oracle, name), 0, 40).all()
    w1._check_tx(gpu, oracle, w1.tx_pool(oracle, gpu, name), 0, 40)
    pub, h, sig, want = w1.key_pool(oracle, name)
    assert np.array_equal(gpu.Secp256k1Crypto().verify_batch(pub, h, sig), want)
