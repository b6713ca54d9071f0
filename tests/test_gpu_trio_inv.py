"""The lane-trio recovery kernel with Z^-1 on the lane trios (csrc/modinv30.h, modinv_safegcd_trio, called from
phase D of trio26_recover_body in csrc/ecc_coop.hip) against the oracle, byte for byte, through the three entry
points that share the body: Transaction::verify (TxIO), the recovery batch (SigIO) and the ecRecover precompile
(EcrecIO).  The trio kernel is forced as test_gpu_trio_helpers.trio_policy does.

Sizes 1, 19, 20, 21, 40, 41 and 81: one trio; both sides of the boundary between the two wave pairs (txs 0..19 /
20..39 of a workgroup, each pair's chain-0 wave inverting its own 20 values); both sides of the workgroup
boundary; a third workgroup with one tx.  A size n takes the first n rows of a pool of 81 whose row i is of kind
KINDS[i mod len(KINDS)]; n = 1 is a launch per kind.  The kinds are those of test_gpu_trio_helpers (r with no
curve point, r = 0, s = 0, s >= n, the v variants, digest 0, and Q at infinity, which is the inversion of Z = 0
beside live trios) and rows with r in {1, 2, n - 1, n - 2, (n + 1) / 2}: r is kept as it is, with v as signed, so
the row is a recovery from a valid nonce point where r is the x of a curve point and a rejected row otherwise --
the oracle decides, no row is left out, and the pool's size is asserted.  The two uniform workgroups of
test_gpu_trio_helpers run as well: one valid row 40 times (every trio's inversion ends in the same batch) and 40
rows with no curve point."""
import numpy as np
import pytest

from test_gpu_ecc import N_SECP
from test_gpu_trio_helpers import (FREE_DIGEST_KINDS, SIG_KINDS, UNIFORM, _raw32, check_ecrec, check_recover, check_tx,
                                   craft_free, craft_sig, run_uniform, slices, trio_policy)  # noqa: F401
from test_gpu_trio_split import _signed

pytestmark = pytest.mark.gpu

SIZES = [1, 19, 20, 21, 40, 41, 81]
POOL = 81
R_VALUES = {"r_1": 1, "r_2": 2, "r_n_minus_1": N_SECP - 1, "r_n_minus_2": N_SECP - 2, "r_half": (N_SECP + 1) // 2}
KINDS_SIG = SIG_KINDS + list(R_VALUES)
KINDS_FREE = FREE_DIGEST_KINDS + list(R_VALUES)
LEFT_OUT = 0  # rows without an expectation from the oracle

_cache = {}


def _kinds(free):
    ks = KINDS_FREE if free else KINDS_SIG
    return [ks[i % len(ks)] for i in range(POOL)]


def _with_r(kind, sig):
    sig[0:32] = _raw32(R_VALUES[kind])
    return sig


def recover_pool(oracle):
    if "rec" not in _cache:
        kinds = _kinds(True)
        rng = np.random.default_rng(0x7530)
        h, sig = _signed(oracle, rng, len(kinds))
        for i, kind in enumerate(kinds):
            if kind in R_VALUES:
                sig[i] = _with_r(kind, sig[i].copy())
            else:
                h[i], sig[i] = craft_free(oracle, rng, kind, h[i].copy(), sig[i].copy())
        want_pub, want_ok = oracle.secp256k1_recover_batch(h, sig, nthreads=8)
        assert len(want_ok) == len(sig) == POOL - LEFT_OUT and LEFT_OUT == 0
        _cache["rec"] = (h, sig, want_pub, want_ok)
    return _cache["rec"]


def ecrec_pool(oracle):
    if "ecrec" not in _cache:
        h, sig, _, _ = recover_pool(oracle)
        inputs = [h[i].tobytes() + (27 + int(sig[i, 64])).to_bytes(32, "big") + sig[i, 0:64].tobytes()
                  for i in range(len(sig))]
        want = [oracle.ecrecover(x) for x in inputs]
        assert len(want) == POOL - LEFT_OUT
        _cache["ecrec"] = (inputs, want)
    return _cache["ecrec"]


def tx_pool(oracle, gpu_mod):
    if "tx" not in _cache:
        kinds = _kinds(False)
        rng = np.random.default_rng(0x7540)
        pres = [gpu_mod.TransactionData(version=int(rng.integers(0, 3)), chain_id="chain" + str(i % 5),
                                        group_id="group" * int(rng.integers(0, 4)),
                                        block_limit=int(rng.integers(0, 2**40)), nonce=str(int(rng.integers(0, 2**62))),
                                        to="cd" * int(rng.integers(0, 21)), input=rng.bytes(int(rng.integers(0, 200))),
                                        abi="y" * int(rng.integers(0, 40))).preimage() for i in range(len(kinds))]
        sigs = []
        for i, kind in enumerate(kinds):
            sk = bytes([1 + i % 100]) + bytes(30) + b"\x03"
            k = bytes([2]) + bytes(30) + bytes([1 + i])
            s = np.frombuffer(oracle.secp256k1_sign(sk, oracle.keccak256(pres[i]), k), dtype=np.uint8).copy()
            sigs.append((_with_r(kind, s) if kind in R_VALUES else craft_sig(rng, kind, s)).tobytes())
        assert len(sigs) == POOL - LEFT_OUT
        _cache["tx"] = (pres, sigs, {})
    return _cache["tx"]


ENTRIES = {
    "sig": (lambda gpu, oracle: recover_pool(oracle), check_recover, len(KINDS_FREE)),
    "ecrec": (lambda gpu, oracle: ecrec_pool(oracle), check_ecrec, len(KINDS_FREE)),
    "tx": (lambda gpu, oracle: tx_pool(oracle, gpu), check_tx, len(KINDS_SIG)),
}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_trio_inversion_mixed(gpu, oracle, trio_policy, entry, n):  # noqa: F811
    pool_of, check, nkinds = ENTRIES[entry]
    pool = pool_of(gpu, oracle)
    seen = np.concatenate([check(gpu, oracle, pool, a, b) for a, b in slices(n, nkinds)])
    assert len(seen) == (nkinds if n == 1 else n)
    assert seen.sum() > 0 and (~seen).sum() > 0


@pytest.mark.parametrize("name", sorted(UNIFORM))
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_trio_inversion_uniform_workgroup(gpu, oracle, trio_policy, entry, name):  # noqa: F811
    run_uniform(gpu, oracle, entry, name)
