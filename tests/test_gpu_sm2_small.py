"""The three SM2 small-batch kernels of csrc/ecc_pair.hip at their workgroup edges, each forced with
bcosgpu_set_tx_kernel_policy, against the oracle's verdicts:

  tx_verify_sm2_trio26_kernel, policy (1, 1, 2, 1), 40 txs per workgroup, chain waves 0 / 1 own txs 0..19 /
  20..39: SM2Crypto::recover over SigIO at 1, 19, 20, 21, 39, 40, 41 and 81 signatures (and at 41 without the
  low-window chains, BCOSGPU_SM2_SPLIT=0, and with every window on the Jacobian entries,
  BCOSGPU_SM2_JAC_ONLY=1; both read at each launch), known-key verify over KeyIO at 41, Transaction::verify
  over TxIO at 41;

  tx_verify_sm2_pair26_kernel, policy (1, 1, 1, 1), 64 txs per workgroup: recover over SigIO at 1, 63, 64, 65
  and 129, known-key verify over KeyIO at 65;

  tx_verify_sm2_pair_kernel (8 x 32-bit, TxIO only), policy (1, 1, 1, 0): Transaction::verify at 1, 64, 65.

  the trio, pair26 and row (policy (1, 1, 3, 1)) kernels on valid signatures under the keys d G, d in {1, 2, 3, 8,
  n - 2, n - 3}: the key is then among G's own multiples, so the table of P's multiples meets the comb's entries
  and, with 4-bit windows and P = G, the joint sums' first additions coincide about once in 16 signatures.

The inputs are signed by the oracle (a zero and an all-ones digest among them), so every case's accepted and
rejected counts follow from the CPU alone; each case asserts that it saw both and that every unedited item is
accepted.  A size below 16 runs a pool of 16 items in launches of that size, so that a one-signature launch
still meets every kind of input.  Each case seeds its pool by its own name: a key named in three calls of the
process is promoted to the registered-key cache (BCOSGPU_KEY_PROMOTE, default 3), and a batch whose keys are
all cached runs the registered-key kernel, not the kernel under test."""
import os
import zlib

import numpy as np
import pytest

from test_gpu_ecc import N_SM2, _mutate_sm2
from test_gpu_verify import _edit

pytestmark = pytest.mark.gpu

TRIO = (1, 1, 2, 1)
PAIR26 = (1, 1, 1, 1)
PAIR32 = (1, 1, 1, 0)
ROW = (1, 1, 3, 1)
TRIO_SIZES = [1, 19, 20, 21, 39, 40, 41, 81]
PAIR_SIZES = [1, 63, 64, 65, 129]


@pytest.fixture
def policy(request, gpu):
    gpu.set_tx_kernel_policy(*request.param)
    yield
    gpu.set_tx_kernel_policy()


def _rng(case):
    return np.random.default_rng(zlib.crc32(case.encode()))


def _scalar(rng):
    k = rng.integers(0, 256, size=32, dtype=np.uint8)
    k[0] &= 0x7F
    k[31] |= 1
    return k.tobytes()


def _signed(oracle, rng, m):
    """m digests and their oracle signatures r || s || pub, each under a key of its own."""
    h = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
    h[0] = 0
    if m > 1:
        h[1] = 0xFF
    sig = np.array([np.frombuffer(oracle.sm2_sign(_scalar(rng), h[i].tobytes(), _scalar(rng)), dtype=np.uint8)
                    for i in range(m)])
    return h, sig


def _slices(m, n):
    return [slice(a, a + n) for a in range(0, m - n + 1, n)]


def _recover_case(gpu, oracle, case, n):
    """SM2Crypto::recover with addresses: item i edited by _mutate_sm2 kind i mod 8."""
    rng = _rng(case)
    h, sig = _signed(oracle, rng, max(n, 16))
    sig = np.array([np.frombuffer(_mutate_sm2(rng, sig[i].tobytes(), i % 8), dtype=np.uint8) for i in range(len(sig))])
    want = oracle.sm2_verify_batch(h, sig, nthreads=8)
    crypto = gpu.SM2Crypto()
    used = np.zeros(len(want), dtype=bool)
    for sl in _slices(len(want), n):
        _, addr, got = crypto.recover_batch(h[sl], sig[sl], want_address=True)
        print(case, "items", sl.start, sl.stop, "accepted", int(want[sl].sum()), "mismatches",
              int((got != want[sl]).sum()))
        assert np.array_equal(got, want[sl])
        assert not addr[~want[sl]].any()
        for j in np.nonzero(want[sl])[0]:
            assert addr[j].tobytes() == oracle.sm3(sig[sl][j, 64:].tobytes())[12:], (case, sl.start + j)
        used[sl] = True
    kinds = np.arange(len(want)) % 8
    assert want[used].sum() > 0 and (~want[used]).sum() > 0
    assert want[used & (kinds == 0)].all()


def _verify_case(gpu, oracle, case, n):
    """SM2Crypto::verify with a known key: item i edited by test_gpu_verify._edit kind i mod 10."""
    rng = _rng(case)
    m = max(n, 20)
    h, sig = _signed(oracle, rng, m)
    pub = sig[:, 64:128].copy()
    clean = pub.copy()
    for i in range(m):
        _edit(rng, pub, h, sig, i, i % 10, N_SM2, clean[(i + 1) % m].copy())
    want = np.array([oracle.sm2_recover(h[i].tobytes(), sig[i, :64].tobytes() + pub[i].tobytes()) is not None
                     for i in range(m)])
    crypto = gpu.SM2Crypto()
    used = np.zeros(m, dtype=bool)
    for sl in _slices(m, n):
        got = crypto.verify_batch(pub[sl], h[sl], sig[sl])
        print(case, "items", sl.start, sl.stop, "accepted", int(want[sl].sum()), "mismatches",
              int((got != want[sl]).sum()))
        assert np.array_equal(got, want[sl])
        used[sl] = True
    kinds = np.arange(m) % 10
    assert want[used].sum() > 0 and (~want[used]).sum() > 0
    assert want[used & (kinds == 0)].all() and not want[kinds == 2].any() and not want[kinds == 3].any()


def _tx_case(gpu, oracle, case, n):
    """Transaction::verify over SM3 / SM2: every tenth signature one byte short, with a flipped s bit, or with
    its key's last byte flipped."""
    rng = _rng(case)
    m = max(n, 16)
    pres = [gpu.TransactionData(version=int(rng.integers(0, 3)), chain_id="chain" + str(i % 7),
                                group_id="group" * int(rng.integers(0, 4)), block_limit=int(rng.integers(0, 2**40)),
                                nonce=str(int(rng.integers(0, 2**62))), to="ab" * int(rng.integers(0, 21)),
                                input=rng.bytes(int(rng.integers(0, 400))), abi="x" * int(rng.integers(0, 50))
                                ).preimage() for i in range(m)]
    sigs = []
    for i, p in enumerate(pres):
        s = bytearray(oracle.sm2_sign(_scalar(rng), oracle.sm3(p), _scalar(rng)))
        if i % 10 == 3:
            s = s[:-1]
        elif i % 10 == 5:
            s[40] ^= 4
        elif i % 10 == 7:
            s[127] ^= 1
        sigs.append(bytes(s))
    cs = gpu.sm_suite()
    status = []
    for sl in _slices(m, n):
        pre, pre_off = gpu.pack_messages(pres[sl])
        sg, sg_off = gpu.pack_messages(sigs[sl])
        th, snd, st = gpu.verify_packed(cs, pre, pre_off, sg, sg_off)
        wh, ws, wst = oracle.tx_verify_packed(1, pre, pre_off, sg, sg_off, nthreads=8)
        print(case, "items", sl.start, sl.stop, "accepted", int((wst == 0).sum()), "mismatches",
              int((st != wst).sum()))
        assert np.array_equal(th, wh) and np.array_equal(st, wst) and np.array_equal(snd, ws)
        status.append(wst)
    wst = np.concatenate(status)
    edited = np.isin(np.arange(len(wst)) % 10, (3, 5, 7))
    assert (wst == 0).sum() > 0 and (wst != 0).sum() > 0
    assert (wst[~edited] == 0).all() and (wst[edited] != 0).all()


# ------------------------------------------------------------------ the lane-trio kernel
@pytest.mark.parametrize("policy", [TRIO], indirect=True, ids=["trio"])
@pytest.mark.parametrize("n", TRIO_SIZES)
def test_trio_sm2_recover_edges(gpu, oracle, policy, n):
    _recover_case(gpu, oracle, "trio-recover-%d" % n, n)


@pytest.mark.parametrize("policy", [TRIO], indirect=True, ids=["trio"])
@pytest.mark.parametrize("env", ["BCOSGPU_SM2_SPLIT=0", "BCOSGPU_SM2_JAC_ONLY=1"])
def test_trio_sm2_recover_41_schedules(gpu, oracle, policy, env):
    name, value = env.split("=")
    os.environ[name] = value
    try:
        _recover_case(gpu, oracle, "trio-recover-41-" + name, 41)
    finally:
        os.environ.pop(name, None)


@pytest.mark.parametrize("policy", [TRIO], indirect=True, ids=["trio"])
def test_trio_sm2_known_key_verify_41(gpu, oracle, policy):
    _verify_case(gpu, oracle, "trio-verify-41", 41)


@pytest.mark.parametrize("policy", [TRIO], indirect=True, ids=["trio"])
def test_trio_sm2_tx_verify_41(gpu, oracle, policy):
    _tx_case(gpu, oracle, "trio-tx-41", 41)


# ------------------------------------------------------------------ the fp26 pair kernel
@pytest.mark.parametrize("policy", [PAIR26], indirect=True, ids=["pair26"])
@pytest.mark.parametrize("n", PAIR_SIZES)
def test_pair26_sm2_recover_edges(gpu, oracle, policy, n):
    _recover_case(gpu, oracle, "pair26-recover-%d" % n, n)


@pytest.mark.parametrize("policy", [PAIR26], indirect=True, ids=["pair26"])
def test_pair26_sm2_known_key_verify_65(gpu, oracle, policy):
    _verify_case(gpu, oracle, "pair26-verify-65", 65)


# ------------------------------------------------------------------ the 8 x 32-bit pair kernel
@pytest.mark.parametrize("policy", [PAIR32], indirect=True, ids=["pair32"])
@pytest.mark.parametrize("n", [1, 64, 65])
def test_pair32_sm2_tx_verify_edges(gpu, oracle, policy, n):
    _tx_case(gpu, oracle, "pair32-tx-%d" % n, n)


# ------------------------------------------------------------------ keys among G's small multiples
_SMALL_KEYS = {}


def _small_key_signed(oracle):
    """32 oracle signatures under each of d = 1, 2, 3, 8, n - 2, n - 3, all valid; built once."""
    if not _SMALL_KEYS:
        rng = _rng("small-keys")
        ds = [1, 2, 3, 8, N_SM2 - 2, N_SM2 - 3]
        h = rng.integers(0, 256, size=(32 * len(ds), 32), dtype=np.uint8)
        sig = np.array([np.frombuffer(oracle.sm2_sign(ds[i // 32].to_bytes(32, "big"), h[i].tobytes(), _scalar(rng)),
                                      dtype=np.uint8) for i in range(len(h))])
        assert oracle.sm2_verify_batch(h, sig, nthreads=8).all()
        for k, d in enumerate(ds):
            assert (sig[32 * k:32 * k + 32, 64:] == np.frombuffer(oracle.sm2_pubkey(d.to_bytes(32, "big")),
                                                                  dtype=np.uint8)).all()
        _SMALL_KEYS["v"] = (h, sig, [oracle.sm3(x[64:].tobytes())[12:] for x in sig])
    return _SMALL_KEYS["v"]


@pytest.mark.parametrize("policy", [TRIO, PAIR26, ROW], indirect=True, ids=["trio", "pair26", "row"])
def test_sm2_recover_keys_among_small_multiples_of_g(gpu, oracle, policy):
    h, sig, addr = _small_key_signed(oracle)
    k0 = gpu.key_cache_info(1)["keyed"]
    _, got_addr, got = gpu.SM2Crypto().recover_batch(h, sig, want_address=True)
    assert gpu.key_cache_info(1)["keyed"] == k0  # not the registered-key kernel
    assert got.all(), np.nonzero(~got)[0].tolist()
    assert [a.tobytes() for a in got_addr] == addr
