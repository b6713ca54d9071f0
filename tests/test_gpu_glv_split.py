"""The exact-integer GLV split (csrc/glv_split.h) inside every secp256k1 kernel a policy can force -- lane-trio,
row, pair, four-wave split, one-lane -- through the three entry points (Transaction::verify: TxIO, the recovery
batch: SigIO, the ecRecover precompile: EcrecIO), against the oracle byte for byte.

Each row is built as test_gpu_row's crafted scalars are: R = k G for a known nonce (so r, v follow), then
s = u2 r mod n, so that the kernel's u2 = s / r is the chosen scalar and its split is what the chains run on.  u2
comes from the host test's list (tests/cpp/glv_split_test.cpp): 0 (s = 0: rejected), 1, 2, n-1, n-2, (n-1)/2,
(n+1)/2, lambda, n-lambda, lambda+-1, 2^128-1, 2^128, 2^255; the four scalars its seeded search found (largest
|k1|, largest |k2|, the rounding fractions of c1 and c2 nearest 1/2); +-c and +-c lambda for small c (one half is
zero and its chain stays at infinity; the negatives make the other half negative).  Three more rows carry such an
s beside an r that is the x of no curve point, so rejected rows stand among the live ones.  The oracle decides
every row; none is left out.

Sizes 1 (a launch per row), 20, 21, 40, 41: one trio, the boundary between the trio kernel's two wave pairs, the
workgroup boundary."""
import numpy as np
import pytest

from test_gpu_ecc import N_SECP
from test_gpu_trio_helpers import _is_residue, _raw32, check_ecrec, check_recover, check_tx

pytestmark = pytest.mark.gpu

LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
POLICIES = {"trio": (1, 1, 2, 1), "row": (1, 1, 3, 1), "pair": (1, 1, 1, 1), "split": (1, 1, 0, 1), "onelane": (0, 1, 0, 1)}
SIZES = [1, 20, 21, 40, 41]
POOL = 41
LEFT_OUT = 0  # rows without an expectation from the oracle

EDGES = [0, 1, 2, N_SECP - 1, N_SECP - 2, N_SECP // 2, N_SECP // 2 + 1, LAMBDA, N_SECP - LAMBDA, LAMBDA + 1, LAMBDA - 1,
         2**128 - 1, 2**128, 2**255]
# (tests/test_glv_split.py compares these four with what the host program prints)
FOUND = [0x2BA21979BC9B03DC7F8305635D5F9CBBDADB3C7BA53288ED9BE7A239C47B5D16,  # |k1| = a29fa17e...: the largest found
         0x4F4670EEA6A05C074B4FDB244230C5F4DA0349093B3E53534EE80E8993FDBCF4,  # |k2| = 8a59da2b...
         0xD27846A992B8A76DB9CF8B9C6C33FE4FC21F5B98E3B769D923AE6414AFCCE4F7,  # c1's fraction within 8.4e-8 of 1/2
         0x30B9ECDA70F6287D503159279B8A5F40360EB24A4FEA2448A0DCEEB849A78676]  # c2's fraction within 1.83e-8 of 1/2
SMALL = [x % N_SECP for c in (3, 4, 5, 6, 7) for x in (c, -c, c * LAMBDA, -c * LAMBDA)]
NO_POINT_AT = (4, 17, 33)  # rows whose r is replaced by an x with no curve point (one inside every size >= 20)

_cache = {}


@pytest.fixture(params=sorted(POLICIES))
def policy(request, gpu):
    gpu.set_tx_kernel_policy(*POLICIES[request.param])
    yield request.param
    gpu.set_tx_kernel_policy()


def _scalars():
    u2 = EDGES + FOUND + SMALL
    for at in NO_POINT_AT:
        u2.insert(at, FOUND[at % 4])
    assert len(u2) == POOL
    return u2


def _rows(oracle, seed):
    """(r || s || v) of every row: s = u2 r mod n over a valid nonce point, or over an r with no curve point."""
    rng = np.random.default_rng(seed)
    sigs = []
    for i, u2 in enumerate(_scalars()):
        while True:
            k = int.from_bytes(rng.bytes(32), "big") % N_SECP or 1
            R = oracle.secp256k1_pubkey(k.to_bytes(32, "big"))
            r, v = int.from_bytes(R[:32], "big"), R[63] & 1
            if r < N_SECP:
                break
        if i in NO_POINT_AT:
            while _is_residue(r):
                r = int.from_bytes(rng.bytes(32), "big") % N_SECP or 1
        sigs.append(np.concatenate([_raw32(r), _raw32(u2 * r % N_SECP), np.array([v], dtype=np.uint8)]))
    return np.array(sigs)


def recover_pool(gpu, oracle):
    if "rec" not in _cache:
        sig = _rows(oracle, 0x61F0)
        h = np.random.default_rng(0x61F1).integers(0, 256, size=(POOL, 32), dtype=np.uint8)
        want_pub, want_ok = oracle.secp256k1_recover_batch(h, sig, nthreads=8)
        assert len(want_ok) == POOL - LEFT_OUT and LEFT_OUT == 0
        assert not want_ok[0] and not want_ok[list(NO_POINT_AT)].any() and want_ok.sum() == POOL - 1 - len(NO_POINT_AT)
        _cache["rec"] = (h, sig, want_pub, want_ok)
    return _cache["rec"]


def ecrec_pool(gpu, oracle):
    if "ecrec" not in _cache:
        h, sig, _, _ = recover_pool(gpu, oracle)
        inputs = [h[i].tobytes() + (27 + int(sig[i, 64])).to_bytes(32, "big") + sig[i, 0:64].tobytes() for i in range(POOL)]
        want = [oracle.ecrecover(x) for x in inputs]
        assert len(want) == POOL - LEFT_OUT
        _cache["ecrec"] = (inputs, want)
    return _cache["ecrec"]


def tx_pool(gpu, oracle):
    """Transactions that carry the rows as their signatures: the digest is the tx's hash, whatever it is, so a row
    over a valid nonce point recovers some sender."""
    if "tx" not in _cache:
        rng = np.random.default_rng(0x61F2)
        pres = [gpu.TransactionData(version=int(rng.integers(0, 3)), chain_id="chain" + str(i % 5),
                                    group_id="group" * int(rng.integers(0, 4)), block_limit=int(rng.integers(0, 2**40)),
                                    nonce=str(int(rng.integers(0, 2**62))), to="ef" * int(rng.integers(0, 21)),
                                    input=rng.bytes(int(rng.integers(0, 200))), abi="z" * int(rng.integers(0, 40))).preimage()
                for i in range(POOL)]
        sigs = [s.tobytes() for s in _rows(oracle, 0x61F3)]
        assert len(sigs) == POOL - LEFT_OUT
        _cache["tx"] = (pres, sigs, {})
    return _cache["tx"]


ENTRIES = {"sig": (recover_pool, check_recover), "ecrec": (ecrec_pool, check_ecrec), "tx": (tx_pool, check_tx)}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_crafted_scalars_through_every_kernel(gpu, oracle, policy, entry, n):
    pool_of, check = ENTRIES[entry]
    pool = pool_of(gpu, oracle)
    launches = [(a, a + 1) for a in range(POOL)] if n == 1 else [(0, n)]
    seen = np.concatenate([check(gpu, oracle, pool, a, b) for a, b in launches])
    assert len(seen) == (POOL if n == 1 else n)
    assert seen.sum() > 0 and (~seen).sum() > 0
