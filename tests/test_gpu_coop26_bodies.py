"""The workgroup edges of the two fe26 kernels of csrc/ecc_coop.hip that test_gpu_trio_split.py does not reach,
each kernel having a body of its own:

  sig_verify_trio26_kernel (trio26_verify_body), policy (1, 0, 2, 1): secp256k1 known-key verify at 1, 39, 40,
  41 and 81 signatures -- one partial workgroup, one short of a full one, a full one (40: the 20 / 21 boundary
  of its two wave pairs lies inside), one more than a workgroup, one more than two -- on the edit kinds of
  test_gpu_verify._edit, kind = index mod 10;

  tx_verify_coop26_kernel<SigIO> (coop26_body), policy (1, 1, 1, 1): recovery at 1, 63, 64, 65 and 129
  signatures (64 txs per workgroup) on test_gpu_trio_split's mutation, parity and no-root inputs.

Both against the oracle's verdicts.  The inputs are signed by the oracle, so every case's accepted and rejected
counts follow from the CPU alone; each test asserts that it saw both.  A size below the pool's runs the pool in
launches of that size, so that a one-signature launch still meets every kind of input."""
import numpy as np
import pytest

import test_gpu_trio_split as split
from test_gpu_ecc import N_SECP
from test_gpu_verify import _edit

pytestmark = pytest.mark.gpu

VERIFY_TRIO = (1, 0, 2, 1)
RECOVER_PAIR = (1, 1, 1, 1)
VERIFY_SIZES = [1, 39, 40, 41, 81]
PAIR_SIZES = [1, 63, 64, 65, 129]
PAIR_INPUTS = {k: split.INPUTS[k] for k in ("mutations", "parity", "no_root")}


@pytest.fixture
def policy(request, gpu):
    gpu.set_tx_kernel_policy(*request.param)
    yield
    gpu.set_tx_kernel_policy()


def verify_inputs(oracle, n):
    """max(n, 20) known-key verifications, item i edited by kind i mod 10, and the oracle's verdicts."""
    rng = np.random.default_rng(0x7310 + n)
    m = max(n, 20)
    h, sig = split._signed(oracle, rng, m)
    pub = np.array([np.frombuffer(oracle.secp256k1_recover(h[i].tobytes(), sig[i].tobytes()), dtype=np.uint8)
                    for i in range(m)])
    clean = pub.copy()
    for i in range(m):
        _edit(rng, pub, h, sig, i, i % 10, N_SECP, clean[(i + 1) % m].copy())
    want = np.array([oracle.secp256k1_verify(pub[i].tobytes(), h[i].tobytes(), sig[i, :64].tobytes())
                     for i in range(m)])
    return pub, h, sig, want


@pytest.mark.parametrize("policy", [VERIFY_TRIO], indirect=True, ids=["trio"])
@pytest.mark.parametrize("n", VERIFY_SIZES)
def test_trio_known_key_verify_edges(gpu, oracle, policy, n):
    pub, h, sig, want = verify_inputs(oracle, n)
    kinds = np.arange(len(want)) % 10
    assert want[kinds == 0].all() and not want[kinds == 1].any() and not want[kinds == 3].any()
    crypto = gpu.Secp256k1Crypto()
    m = len(want) - len(want) % n
    got = np.concatenate([crypto.verify_batch(pub[a:a + n], h[a:a + n], sig[a:a + n]) for a in range(0, m, n)])
    print("n", n, "items", m, "accepted", int(want[:m].sum()), "mismatches", int((got != want[:m]).sum()))
    assert np.array_equal(got, want[:m])
    assert want[:m].sum() > 0 and (~want[:m]).sum() > 0


@pytest.mark.parametrize("policy", [RECOVER_PAIR], indirect=True, ids=["pair"])
@pytest.mark.parametrize("n", PAIR_SIZES)
@pytest.mark.parametrize("kind", sorted(PAIR_INPUTS))
def test_pair_recover_edges(gpu, oracle, policy, kind, n):
    h, sig = PAIR_INPUTS[kind](oracle, n)
    oks = [split._check(gpu, oracle, h[a:a + n], sig[a:a + n]) for a in range(0, len(sig) - n + 1, n)]
    ok = np.concatenate(oks)
    assert ok.sum() > 0 and (~ok).sum() > 0
    if kind == "parity":  # both parities among the accepted plain signatures, and an accepted x = r + n
        v = sig[:len(ok), 64][ok]
        assert (v == 0).any() and (v == 1).any() and (v >= 2).any()
