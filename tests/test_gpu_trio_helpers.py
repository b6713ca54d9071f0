"""The lane-trio recovery kernel on eight waves (csrc/ecc_coop.hip, trio26_recover_body: waves 0..3 run the GLV
chains, waves 4..7 are helpers that take the digest, u1, the comb windows of u1 G and their sum, and the whole
square root, one lane per tx) against the oracle, byte for byte, through the three entry points that share the
body: Transaction::verify (TxIO: tx hash, sender, status), the recovery batch (SigIO: key, address, verdict)
and the ecRecover precompile (EcrecIO).  The trio kernel is forced with bcosgpu_set_tx_kernel_policy(1, 1, 2, 1).

Batch sizes 1, 19, 20, 21, 39, 40, 41 and 81: one tx, both sides of the boundary between the two wave pairs
(txs 0..19 / 20..39 of a workgroup), both sides of the workgroup boundary, and a third workgroup with one tx.
A size n takes the first n rows of a pool whose row i is of kind KINDS[i mod len(KINDS)], so helpers and chains
disagree lane by lane inside a workgroup (the helpers work on lane = tx, the chains on lane trios); n = 1 is a
launch per kind.  The kinds: random signatures; an r that is the x of no curve point; r = 0; s = 0; s >= n;
v = 4; v = 2 and v = 3 with r just below p - n (x = r + n < p, chosen on the curve) and just above it (rejected);
and, where the digest is free (SigIO, EcrecIO), digest 0 (u1 = 0: the G part is infinity) and z = s k (Q is
infinity: the recovery fails).  Two more workgroups are uniform: 40 rows that all have no curve point (every
verdict of the root helper is `no`), and one valid row 40 times (every trio runs the same digits).

The 16-bit comb is the default tables'; the 8-bit comb (32 windows, the helpers' other split) needs
bcosgpu_init_ex(dev, BCOSGPU_INIT_SMALL_TABLES) at the device's first initialisation, so one test runs every
case above again in a process of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_ecc import N_SECP
from test_gpu_trio_split import P_SECP, TRIO, _b32, _signed

pytestmark = pytest.mark.gpu

SIZES = [1, 19, 20, 21, 39, 40, 41, 81]
POOL = 81
SIG_KINDS = ["random", "no_point", "r_zero", "s_zero", "s_ge_n", "v4", "v2_below", "v3_below", "v2_above", "v3_above",
             "random"]
FREE_DIGEST_KINDS = SIG_KINDS + ["digest0", "q_inf"]
UNIFORM = {"invalid": ["no_point"] * 40, "same": ["same"] * 40}


@pytest.fixture
def trio_policy(gpu):
    gpu.set_tx_kernel_policy(*TRIO)
    yield
    gpu.set_tx_kernel_policy()


def _raw32(x):
    return np.frombuffer(int(x).to_bytes(32, "big"), dtype=np.uint8)


def _is_residue(x):
    return pow((pow(x, 3, P_SECP) + 7) % P_SECP, (P_SECP - 1) // 2, P_SECP) == 1


def craft_sig(rng, kind, sig):
    """Row `sig` (a valid r || s || v) turned into the row of its kind; only the signature changes."""
    if kind == "no_point":
        while True:
            r = int.from_bytes(rng.bytes(32), "big") % N_SECP or 1
            if not _is_residue(r):
                break
        sig[0:32] = _b32(r)
    elif kind == "r_zero":
        sig[0:32] = 0
    elif kind == "s_zero":
        sig[32:64] = 0
    elif kind == "s_ge_n":
        sig[32:64] = _raw32(N_SECP + int(rng.integers(0, 1000)))
    elif kind == "v4":
        sig[64] = 4
    elif kind in ("v2_below", "v3_below"):  # x = r + n = p - j, the first such x on the curve
        j = int(rng.integers(1, 1000))
        while not _is_residue(P_SECP - j):
            j += 1
        sig[0:32] = _raw32(P_SECP - N_SECP - j)
        sig[64] = 2 if kind == "v2_below" else 3
    elif kind in ("v2_above", "v3_above"):  # r + n >= p
        sig[0:32] = _raw32(P_SECP - N_SECP + int(rng.integers(0, 1000)))
        sig[64] = 2 if kind == "v2_above" else 3
    return sig


def craft_free(oracle, rng, kind, h, sig):
    """The kinds that choose the digest as well: (h, sig) of a row."""
    if kind not in ("digest0", "q_inf"):
        return h, craft_sig(rng, kind, sig)
    while True:
        k = int.from_bytes(rng.bytes(32), "big") % N_SECP or 1
        R = oracle.secp256k1_pubkey(k.to_bytes(32, "big"))
        rx, ry = int.from_bytes(R[:32], "big"), int.from_bytes(R[32:], "big")
        if rx < N_SECP:
            break
    s = int.from_bytes(rng.bytes(32), "big") % N_SECP or 1
    e = 0 if kind == "digest0" else s * k % N_SECP
    return _b32(e), np.concatenate([_b32(rx), _b32(s), np.array([ry & 1], dtype=np.uint8)])


_cache = {}


def _kinds(name, free):
    if name == "mixed":
        ks = FREE_DIGEST_KINDS if free else SIG_KINDS
        return [ks[i % len(ks)] for i in range(POOL)]
    return UNIFORM[name]


def recover_pool(oracle, name):
    """Digests, signatures and the oracle's recovery of them (made once per pool)."""
    key = ("rec", name)
    if key not in _cache:
        kinds = _kinds(name, True)
        rng = np.random.default_rng(0x7510 + len(name))
        h, sig = _signed(oracle, rng, len(kinds))
        for i, kind in enumerate(kinds):
            if kind == "same":
                h[i], sig[i] = h[2], sig[2]
            else:
                h[i], sig[i] = craft_free(oracle, rng, kind, h[i].copy(), sig[i].copy())
        want_pub, want_ok = oracle.secp256k1_recover_batch(h, sig, nthreads=8)
        for i, kind in enumerate(kinds):
            if kind in ("random", "same", "v2_below", "v3_below", "digest0"):
                assert want_ok[i], (i, kind)
            else:
                assert not want_ok[i], (i, kind)
        _cache[key] = (h, sig, want_pub, want_ok)
    return _cache[key]


def slices(n, nkinds):
    """The launches of a size: the first n rows of the pool, and for one row a launch per kind."""
    return [(a, a + n) for a in range(0, nkinds if n == 1 else 1)]


def check_recover(gpu, oracle, pool, a, b):
    h, sig, want_pub, want_ok = pool
    pub, addr, okg = gpu.Secp256k1Crypto().recover_batch(h[a:b], sig[a:b], want_address=True)
    ok = want_ok[a:b]
    assert np.array_equal(okg, ok)
    assert np.array_equal(pub[ok], want_pub[a:b][ok])
    assert not pub[~ok].any() and not addr[~ok].any()
    for i in np.nonzero(ok)[0]:
        assert addr[i].tobytes() == oracle.keccak256(want_pub[a + i].tobytes())[12:], (a, i)
    return ok


def ecrec_pool(oracle, name):
    """The recovery pool as ecRecover inputs (hash || v + 27 as a 32-byte word || r || s) and the oracle's
    outputs."""
    key = ("ecrec", name)
    if key not in _cache:
        h, sig, _, _ = recover_pool(oracle, name)
        inputs = [h[i].tobytes() + (27 + int(sig[i, 64])).to_bytes(32, "big") + sig[i, 0:64].tobytes()
                  for i in range(len(sig))]
        _cache[key] = (inputs, [oracle.ecrecover(x) for x in inputs])
    return _cache[key]


def check_ecrec(gpu, oracle, pool, a, b):
    from bcos_gpu.precompiled import ec_recover_batch
    inputs, want = pool
    out, okg = ec_recover_batch(inputs[a:b])
    for i in range(b - a):
        assert bool(okg[i]) == (want[a + i] != b""), (a, i)
        assert out[i].tobytes() == (want[a + i] if want[a + i] else bytes(32)), (a, i)
    return np.array([w != b"" for w in want[a:b]])


def tx_pool(oracle, gpu_mod, name):
    """Transactions whose signature is the pool's kind over the tx's own hash, and the oracle's verdicts."""
    key = ("tx", name)
    if key not in _cache:
        kinds = _kinds(name, False)
        rng = np.random.default_rng(0x7520 + len(name))
        pres = [gpu_mod.TransactionData(version=int(rng.integers(0, 3)), chain_id="chain" + str(i % 7),
                                        group_id="group" * int(rng.integers(0, 4)),
                                        block_limit=int(rng.integers(0, 2**40)), nonce=str(int(rng.integers(0, 2**62))),
                                        to="ab" * int(rng.integers(0, 21)), input=rng.bytes(int(rng.integers(0, 300))),
                                        abi="x" * int(rng.integers(0, 50))).preimage() for i in range(len(kinds))]
        sigs = []
        for i, kind in enumerate(kinds):
            if kind == "same":
                pres[i] = pres[0]
            sk = bytes([1 + (0 if kind == "same" else i) % 100]) + bytes(30) + b"\x01"
            k = bytes([1]) + bytes(30) + bytes([1 + (0 if kind == "same" else i)])
            s = np.frombuffer(oracle.secp256k1_sign(sk, oracle.keccak256(pres[i]), k), dtype=np.uint8).copy()
            sigs.append(craft_sig(rng, kind, s).tobytes())
        _cache[key] = (pres, sigs, {})
    return _cache[key]


def check_tx(gpu, oracle, pool, a, b):
    pres, sigs, want = pool
    pre, pre_off = gpu.pack_messages(pres[a:b])
    sg, sg_off = gpu.pack_messages(sigs[a:b])
    if (a, b) not in want:
        want[(a, b)] = oracle.tx_verify_packed(0, pre, pre_off, sg, sg_off, nthreads=8)
    wh, ws, wst = want[(a, b)]
    th, snd, st = gpu.verify_packed(gpu.secp256k1_suite(), pre, pre_off, sg, sg_off)
    assert np.array_equal(th, wh) and np.array_equal(st, wst) and np.array_equal(snd, ws)
    return wst == 0


ENTRIES = {
    "sig": (lambda gpu, oracle, name: recover_pool(oracle, name), check_recover, len(FREE_DIGEST_KINDS)),
    "ecrec": (lambda gpu, oracle, name: ecrec_pool(oracle, name), check_ecrec, len(FREE_DIGEST_KINDS)),
    "tx": (lambda gpu, oracle, name: tx_pool(oracle, gpu, name), check_tx, len(SIG_KINDS)),
}


def run_mixed(gpu, oracle, entry, n):
    pool_of, check, nkinds = ENTRIES[entry]
    pool = pool_of(gpu, oracle, "mixed")
    seen = np.concatenate([check(gpu, oracle, pool, a, b) for a, b in slices(n, nkinds)])
    assert seen.sum() > 0 and (~seen).sum() > 0


def run_uniform(gpu, oracle, entry, name):
    pool_of, check, _ = ENTRIES[entry]
    ok = check(gpu, oracle, pool_of(gpu, oracle, name), 0, 40)
    assert ok.all() if name == "same" else not ok.any()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_helpers_mixed(gpu, oracle, trio_policy, entry, n):
    run_mixed(gpu, oracle, entry, n)


@pytest.mark.parametrize("name", sorted(UNIFORM))
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_helpers_uniform_workgroup(gpu, oracle, trio_policy, entry, name):
    run_uniform(gpu, oracle, entry, name)


_SMALL_TABLES_SCRIPT = """
import sys
sys.path[:0] = [{tests!r}, {pkg!r}, {root!r}]
import bcos_gpu
from oracle import oracle
import test_gpu_trio_helpers as t
oracle.build()
bcos_gpu.check(bcos_gpu.lib().bcosgpu_init_ex(0, 1))  # BCOSGPU_INIT_SMALL_TABLES
bcos_gpu.set_tx_kernel_policy(*t.TRIO)
for entry in sorted(t.ENTRIES):
    for n in t.SIZES:
        t.run_mixed(bcos_gpu, oracle, entry, n)
    for name in sorted(t.UNIFORM):
        t.run_uniform(bcos_gpu, oracle, entry, name)
print("small-tables ok")
"""


def test_helpers_small_comb_tables(gpu):
    """Every case above on the 8-bit comb (32 comb windows over the helpers instead of 16).  Own process: the
    flag only matters at a device's first initialisation."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _SMALL_TABLES_SCRIPT.format(tests=os.path.join(root, "tests"), pkg=os.path.join(root, "fisco-bcos_amd"),
                                       root=root)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "small-tables ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
