"""The lane-trio recovery kernel's scalar phase on tx PAIRS (csrc/pair_inv.h in trio26_recover_body: seat t of
wave 0 holds txs t and t + 20 of a workgroup and inverts r_a r_b once) against the oracle, byte for byte, through
the three entry points that share the body: Transaction::verify (TxIO), the recovery batch (SigIO) and the
ecRecover precompile (EcrecIO).  The trio kernel is forced with bcosgpu_set_tx_kernel_policy(1, 1, 2, 1).

Sizes 1, 19, 20 (no tx has a partner; at 20 every seat is full), 21 (the first pair), 39, 40, 41 (a second workgroup
with a single tx) and 81, on test_gpu_trio_helpers' mixed pool.

Crafted batches of 40 and 41 rows: every case below sits at the columns t and t + 20 for t = 0, 4 and 19 (t = 4 is
the trio that the DPP row's phantom lane mirrors); the other columns are valid rows.  A row needs no signer: for
any r that is the x of a curve point, any s in [1, n) and any digest the recovery yields some key, and the oracle
says which.
  * a rejected member beside a valid one, in seat a, in seat b and in both: r = 0, r >= n, s = 0, v = 4, and (TxIO,
    whose signatures have a length) a 64-byte signature;
  * the same r in both seats;
  * r_b = 1 / r_a mod n (the inverted product is 1), r_a searched until both are the x of a curve point;
  * r = n - 1, or the nearest r below it that is the x of a curve point, in seat a, in seat b and in both.
The searches are bounded and must succeed; no case is left out (CASES_LEFT_OUT).

Each entry point runs in a child process under a time limit of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_ecc import N_SECP
from test_gpu_trio_helpers import ENTRIES, SIZES, _is_residue, _raw32, check_ecrec, check_recover, check_tx, run_mixed
from test_gpu_trio_split import TRIO

pytestmark = pytest.mark.gpu

SEATS = (0, 4, 19)
REJECTS = ["r_zero", "r_ge_n", "s_zero", "v4", "short"]
PLACES = ["a", "b", "both"]
CASES_LEFT_OUT = 0
SEARCH_LIMIT = 256


def _on_curve_r(rng):
    for _ in range(SEARCH_LIMIT):
        r = int.from_bytes(rng.bytes(32), "big") % N_SECP
        if r and _is_residue(r):
            return r
    raise AssertionError("no x of a curve point in %d draws" % SEARCH_LIMIT)


def inverse_pair(rng):
    """(r_a, r_b, draws) with r_a r_b = 1 mod n and both the x of a curve point."""
    for draws in range(1, SEARCH_LIMIT + 1):
        ra = _on_curve_r(rng)
        rb = pow(ra, -1, N_SECP)
        if _is_residue(rb):
            return ra, rb, draws
    raise AssertionError("no inverse pair on the curve in %d draws" % SEARCH_LIMIT)


def top_r():
    """(r, steps): the largest r < n that is the x of a curve point, searched down from n - 1."""
    for steps in range(SEARCH_LIMIT):
        if _is_residue(N_SECP - 1 - steps):
            return N_SECP - 1 - steps, steps
    raise AssertionError("no x of a curve point within %d of n - 1" % SEARCH_LIMIT)


def _valid_row(rng, r=None):
    r = _on_curve_r(rng) if r is None else r
    s = int.from_bytes(rng.bytes(32), "big") % (N_SECP - 1) + 1
    return np.concatenate([_raw32(r), _raw32(s), np.array([int(rng.integers(0, 2))], dtype=np.uint8)])


def _reject(rng, row, kind):
    row = row.copy()
    if kind == "r_zero":
        row[0:32] = 0
    elif kind == "r_ge_n":
        row[0:32] = _raw32(N_SECP + int(rng.integers(0, 3)))  # n, n + 1, n + 2
    elif kind == "s_zero":
        row[32:64] = 0
    elif kind == "v4":
        row[64] = 4
    elif kind == "short":
        row = row[:64]
    return row


def cases(with_short):
    """[(name, seat a's row, seat b's row, a is valid, b is valid)] -- the same for every entry point but `short`."""
    rng = np.random.default_rng(0x9A1F)
    out = []
    for kind in REJECTS:
        if kind == "short" and not with_short:
            continue
        for place in PLACES:
            a, b = _valid_row(rng), _valid_row(rng)
            if place in ("a", "both"):
                a = _reject(rng, a, kind)
            if place in ("b", "both"):
                b = _reject(rng, b, kind)
            out.append((kind + "_" + place, a, b, place == "b", place == "a"))
    r = _on_curve_r(rng)
    out.append(("equal_r", _valid_row(rng, r), _valid_row(rng, r), True, True))
    ra, rb, draws = inverse_pair(rng)
    assert ra * rb % N_SECP == 1 and 1 <= draws <= SEARCH_LIMIT
    out.append(("inverse_r", _valid_row(rng, ra), _valid_row(rng, rb), True, True))
    out.append(("inverse_r_swapped", _valid_row(rng, rb), _valid_row(rng, ra), True, True))
    rt, steps = top_r()
    assert 0 <= steps < SEARCH_LIMIT and _is_residue(rt)
    for place in PLACES:
        a = _valid_row(rng, rt if place in ("a", "both") else None)
        b = _valid_row(rng, rt if place in ("b", "both") else None)
        out.append(("top_r_" + place, a, b, True, True))
    want = (len(REJECTS) - (0 if with_short else 1)) * len(PLACES) + 3 + len(PLACES)
    assert len(out) == want - CASES_LEFT_OUT and CASES_LEFT_OUT == 0
    return out


def batch_rows(rng, a, b):
    """41 rows and which of them must verify: the case at columns t, t + 20 for t in SEATS, valid rows elsewhere."""
    rows = [_valid_row(rng) for _ in range(41)]
    for t in SEATS:
        rows[t], rows[t + 20] = a, b
    return rows


def run_crafted(gpu, oracle, entry):
    rng = np.random.default_rng(0x9A20 + len(entry))
    done = 0
    for name, a, b, a_ok, b_ok in cases(with_short=entry == "tx"):
        rows = batch_rows(rng, a, b)
        expect = np.ones(41, dtype=bool)
        for t in SEATS:
            expect[t], expect[t + 20] = a_ok, b_ok
        if entry == "tx":
            pres = [gpu.TransactionData(version=1, chain_id="chain" + str(i % 3), group_id="group", block_limit=1000 + i,
                                        nonce=str(int(rng.integers(0, 2**62))), to="cd" * 20,
                                        input=rng.bytes(int(rng.integers(0, 120))), abi="").preimage() for i in range(41)]
            pool = (pres, [r.tobytes() for r in rows], {})
            check = check_tx
        else:
            h = rng.integers(0, 256, size=(41, 32), dtype=np.uint8)
            sig = np.array(rows)
            if entry == "sig":
                want_pub, want_ok = oracle.secp256k1_recover_batch(h, sig, nthreads=8)
                assert np.array_equal(want_ok, expect), (name, np.nonzero(want_ok != expect)[0])
                pool = (h, sig, want_pub, want_ok)
                check = check_recover
            else:
                inputs = [h[i].tobytes() + (27 + int(sig[i, 64])).to_bytes(32, "big") + sig[i, 0:64].tobytes()
                          for i in range(41)]
                pool = (inputs, [oracle.ecrecover(x) for x in inputs])
                check = check_ecrec
        for n in (40, 41):
            seen = check(gpu, oracle, pool, 0, n)
            assert np.array_equal(np.asarray(seen, dtype=bool), expect[:n]), (entry, name, n)
        done += 1
    return done


def run_entry(gpu, oracle, entry):
    """Everything of one entry point (the child process calls it)."""
    gpu.set_tx_kernel_policy(*TRIO)
    for n in SIZES:
        run_mixed(gpu, oracle, entry, n)
    done = run_crafted(gpu, oracle, entry)
    gpu.set_tx_kernel_policy()
    return done


_CHILD = """
import sys
sys.path[:0] = [{tests!r}, {pkg!r}, {root!r}]
import bcos_gpu
from oracle import oracle
import test_gpu_trio_pairinv as t
oracle.build()
bcos_gpu.ensure_device(0)
print("pairinv ok", {entry!r}, t.run_entry(bcos_gpu, oracle, {entry!r}))
"""


def test_sizes_are_the_pairing_boundaries():
    assert SIZES == [1, 19, 20, 21, 39, 40, 41, 81]


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_tx_pairs_through_the_trio_kernel(gpu, entry):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _CHILD.format(tests=os.path.join(root, "tests"), pkg=os.path.join(root, "fisco-bcos_amd"), root=root, entry=entry)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "pairinv ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
    want = (len(REJECTS) - (0 if entry == "tx" else 1)) * len(PLACES) + 3 + len(PLACES)
    assert r.stdout.strip().endswith(str(want)), r.stdout[-300:]
