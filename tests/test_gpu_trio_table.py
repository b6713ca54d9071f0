"""The recovery kernel's table of R' built by three waves (csrc/ec26_trio.h, trio_table_shared: waves 1, 2 and 3 of
tx_verify_trio26_kernel share the multiples, the prefix / suffix products and the entries, and hand them over
through flags in LDS; K = Zc^2 w is stored with the table) against the oracle, byte for byte, through the three
entry points that share the body: Transaction::verify (TxIO), the recovery batch (SigIO) and the ecRecover
precompile (EcrecIO).  The trio kernel is forced with bcosgpu_set_tx_kernel_policy(1, 1, 2, 1).

Sizes 1, 20, 21, 40, 41 and 81: one tx, both sides of the boundary between the two wave pairs, both sides of the
workgroup boundary, and a third workgroup with one tx; the rows are test_gpu_trio_helpers' pool (random
signatures, an r with no curve point, r = 0, s = 0, s >= n, v = 4, v = 2 / 3 around p - n, digest 0, Q at
infinity), kind = index mod the number of kinds, and its two uniform workgroups: 40 rows with no curve point and
one valid row 40 times.

One more workgroup takes the table entry by entry: rows 5 (j - 1) .. 5 (j - 1) + 4, j = 1 .. 8, have u2 = s / r
built from GLV halves (u2 = k1 + k2 lambda, as test_gpu_trio_chain_start builds them) whose radix-16 Booth digits
are all +-j or 0 on both chains, so a row's chains read entry j - 1 of tab (chain 0) and of tabphx (chain 1) and
no other: a wrong entry, or a wrong beta x of one entry, cannot hide among right ones."""
import numpy as np
import pytest

from test_gpu_ecc import N_SECP
from test_gpu_trio_chain_start import LAMBDA, nonce_point, split
from test_gpu_trio_helpers import (ENTRIES, check_ecrec, check_recover, check_tx, run_mixed, run_uniform, trio_policy,  # noqa: F401
                                   UNIFORM)
from test_gpu_trio_split import _b32, _signed

pytestmark = pytest.mark.gpu

SIZES = [1, 20, 21, 40, 41, 81]
DIGITS = 30  # radix-16 digits 0 .. 29 of a half are +-j, the ones above are 0: the half is below 2^120


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_table_mixed(gpu, oracle, trio_policy, entry, n):
    run_mixed(gpu, oracle, entry, n)


@pytest.mark.parametrize("name", sorted(UNIFORM))
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_table_uniform_workgroup(gpu, oracle, trio_policy, entry, name):
    run_uniform(gpu, oracle, entry, name)


def booth_digits(k):
    """The radix-16 Booth digits 0 .. 32 of a 128-bit k: d_i = nibble_i + bit(4 i - 1) - 16 bit(4 i + 3)."""
    return [((k >> (4 * i)) & 15) + ((k >> (4 * i - 1)) & 1 if i else 0) - 16 * ((k >> (4 * i + 3)) & 1)
            for i in range(33)]


def half_of_digit(rng, j):
    """A positive half whose Booth digits 0 .. DIGITS - 1 are all +j or -j (the top one +j) and 0 above."""
    k, carry = 0, 0
    for i in range(DIGITS):
        plus = j - carry       # the nibble of digit +j: below 8, no carry out
        minus = 16 - j - carry  # the nibble of digit -j: 8 or above, carry out
        ok_plus, ok_minus = 0 <= plus < 8, 8 <= minus < 16
        take_plus = ok_plus and (i == DIGITS - 1 or not ok_minus or bool(rng.integers(0, 2)))
        assert take_plus or ok_minus, (j, i)
        k |= (plus if take_plus else minus) << (4 * i)
        carry = 0 if take_plus else 1
    assert carry == 0
    d = booth_digits(k)
    assert all(abs(x) == j for x in d[:DIGITS]) and not any(d[DIGITS:]) and sum(x * 16**i for i, x in enumerate(d)) == k
    return k


_cache = {}


def entry_rows(oracle, rng, h, sig):
    """Rows 0 .. 39 of (h, sig) with the signature of the per-entry workgroup: s = u2 r on a fresh nonce point."""
    for i in range(40):
        j = i // 5 + 1
        want = (1 if rng.integers(0, 2) else -1) * half_of_digit(rng, j), (1 if rng.integers(0, 2) else -1) * half_of_digit(rng, j)
        u2 = (want[0] + want[1] * LAMBDA) % N_SECP
        assert split(u2) == want, (i, j)  # halves this short are the split's own
        for half in want:  # both signs of the digit on either chain
            assert {j, -j} <= set(booth_digits(abs(half))), (i, j)
        r, v = nonce_point(oracle, rng)
        sig[i, 0:32] = _b32(r)
        sig[i, 32:64] = _b32(u2 * r)
        sig[i, 64] = v
    return h, sig


def entry_pool(oracle, gpu_mod, entry):
    if entry not in _cache:
        rng = np.random.default_rng(0x7620)
        if entry == "tx":
            pres = [gpu_mod.TransactionData(version=i % 3, chain_id="chain" + str(i % 7), group_id="group",
                                            block_limit=1000 + i, nonce=str(7 * i), to="ab" * 20,
                                            input=rng.bytes(int(rng.integers(0, 200))), abi="").preimage() for i in range(40)]
            _, sig = entry_rows(oracle, rng, None, np.zeros((40, 65), dtype=np.uint8))
            _cache[entry] = (pres, [s.tobytes() for s in sig], {})
        else:
            if "sig" not in _cache:
                h, sig = _signed(oracle, rng, 40)
                h, sig = entry_rows(oracle, rng, h, sig)
                want_pub, want_ok = oracle.secp256k1_recover_batch(h, sig, nthreads=8)
                assert want_ok.all()  # every row runs its chains to an accepted key
                _cache["sig"] = (h, sig, want_pub, want_ok)
            if entry == "ecrec":
                h, sig, _, _ = _cache["sig"]
                inputs = [h[i].tobytes() + (27 + int(sig[i, 64])).to_bytes(32, "big") + sig[i, 0:64].tobytes()
                          for i in range(40)]
                _cache[entry] = (inputs, [oracle.ecrecover(x) for x in inputs])
    return _cache[entry]


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_table_entry_by_entry(gpu, oracle, trio_policy, entry):
    check = {"sig": check_recover, "ecrec": check_ecrec, "tx": check_tx}[entry]
    ok = check(gpu, oracle, entry_pool(oracle, gpu, entry), 0, 40)
    assert ok.all()
