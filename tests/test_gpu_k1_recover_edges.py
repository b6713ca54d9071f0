"""The seven secp256k1 recovery bodies -- trio26_recover_body, coop26_body, recover_row_kernel,
tx_verify_coop_kernel, tx_verify_split_kernel, secp256k1_recover_lane26, secp256k1_recover_lane -- on the rows of
tests/k1_recover_vectors.py, through their three entry points: the recovery batch (SigIO), the ecRecover
precompile (EcrecIO) and Transaction::verify (TxIO).  Recovery takes the digest, r, s and v as they come, so the
shipped library meets every row as it is.  Every leg's verdicts, keys, addresses and senders are compared with the
rows' `expected` (the restatement's, pinned to the oracle on every row by tests/test_k1_recover_vectors.py),
never with another kernel's; the oracle gives Keccak256 only.

Each test starts one child process, which runs its launches and prints the results as JSON with its wall, setup
and launch seconds; the parent compares.  A child that exits nonzero fails its test; nothing is retried.

Over TxIO the digest is the transaction's hash, so only r, s and v are free: 41 fixed small transactions, the
x_r, s_edge and u2_shape signatures rebuilt over their hashes, and the final_add rows a fixed e allows.  That is
the only way into tx_verify_coop_kernel and tx_verify_split_kernel; the u1 shapes stay unpinned there.

The recovery batch's C ABI reads signatures at a stride of 65 bytes and has no other (launch_secp256k1_recover's
callers pass 65); the precompile's rows are 128 bytes apart, so 4-byte-aligned signatures run there."""
import json
import os
import struct
import subprocess
import sys
import time

import numpy as np
import pytest

import k1_recover_vectors as rv

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
PKG = os.path.join(ROOT, "fisco-bcos_amd")

# bcosgpu_set_tx_kernel_policy(split, occupancy, coop, field)
SIG_POLICIES = {"trio": (1, 1, 2, 1), "pair": (1, 1, 1, 1), "row": (1, 1, 3, 1), "lane26_occ1": (0, 1, 0, 1),
                "lane26_occ2": (0, 2, 0, 1), "lane32": (0, 1, 0, 0), "auto": (-1, 0, 2, 1)}
ECREC_POLICIES = ("trio", "row", "lane26_occ1", "auto")
TX_POLICIES = {"trio": (1, 1, 2, 1), "pair": (1, 1, 1, 1), "row": (1, 1, 3, 1), "coop32": (1, 1, 1, 0),
               "split": (1, 1, 0, 1), "lane26_occ1": (0, 1, 0, 1), "lane32": (0, 1, 0, 0)}
SIZES = (1, 39, 40, 41, 65, 0)  # kTrioTxs = 40; 0: the whole pool in one launch
TIMEOUT = 240  # a backstop, as the sibling tests'; the children report their own seconds
N_TX = 41

_CHILD = """
import sys
sys.path[:0] = [{pkg!r}, {root!r}, {tests!r}]
import test_gpu_k1_recover_edges
test_gpu_k1_recover_edges._child({mode!r})
"""


def preimages():
    """41 fixed small transactions: the bytes impl_calculate feeds the hasher (bcos_gpu.tx.TransactionData.preimage)."""
    return [struct.pack(">i", i % 3) + b"chain%d" % (i % 7) + b"group" * (i % 4) + struct.pack(">q", 1000 + 37 * i)
            + b"%d" % (10**15 + 977 * i) + b"ab" * (i % 21) + bytes((i + j) & 0xFF for j in range(7 * i % 90))
            for i in range(N_TX)]


# ------------------------------------------------------------------ the child
def _chunks(m, n):
    n = n or m
    return [(a, min(a + n, m)) for a in range(0, m, n)]


def _sig_legs(gpu, policies, sizes, tag=""):
    """Secp256k1Crypto.recover_batch(want_address=True) under each kernel policy, the pool in launches of each size."""
    rows = rv.pool()
    h = np.array([np.frombuffer(x[2], dtype=np.uint8) for x in rows])
    sig = np.array([np.frombuffer(x[3], dtype=np.uint8) for x in rows])
    crypto = gpu.Secp256k1Crypto()
    out = []
    for name in policies:
        gpu.set_tx_kernel_policy(*SIG_POLICIES[name])
        try:
            for n in sizes:
                pub, addr, ok = [], [], []
                for a, b in _chunks(len(rows), n):
                    p, ad, o = crypto.recover_batch(h[a:b], sig[a:b], want_address=True)
                    pub.append(p.tobytes())
                    addr.append(ad.tobytes())
                    ok += o.astype(int).tolist()
                out.append({"leg": "%ssig/%s/%d" % (tag, name, n or len(rows)), "ok": ok, "pub": b"".join(pub).hex(),
                            "addr": b"".join(addr).hex()})
        finally:
            gpu.set_tx_kernel_policy()
    return out


def _ecrec_legs(gpu):
    """precompiled.ec_recover_batch over the whole pool in one launch and in launches of 41."""
    from bcos_gpu import precompiled
    rows = rv.pool()
    data = np.array([np.frombuffer(rv.ecrecover_input(x), dtype=np.uint8) for x in rows])
    out = []
    for name in ECREC_POLICIES:
        gpu.set_tx_kernel_policy(*SIG_POLICIES[name])
        try:
            for n in (0, 41):
                res, ok = [], []
                for a, b in _chunks(len(rows), n):
                    r, o = precompiled.ec_recover_batch(data[a:b])
                    res.append(r.tobytes())
                    ok += o.astype(int).tolist()
                out.append({"leg": "ecrec/%s/%d" % (name, n or len(rows)), "ok": ok, "out": b"".join(res).hex()})
        finally:
            gpu.set_tx_kernel_policy()
    return out


def _tx_legs(gpu, job):
    """verify_packed over the transaction rows the parent built (preimage and signature per row), whole and in
    launches of 41, under each of the seven bodies' policies."""
    pres = [bytes.fromhex(p) for p in job["pre"]]
    sigs = [bytes.fromhex(s) for s in job["sig"]]
    suite = gpu.secp256k1_suite()
    out = []
    for name, policy in TX_POLICIES.items():
        gpu.set_tx_kernel_policy(*policy)
        try:
            for n in (0, 41):
                th, snd, st = [], [], []
                for a, b in _chunks(len(pres), n):
                    pre, pre_off = gpu.pack_messages(pres[a:b])
                    sg, sg_off = gpu.pack_messages(sigs[a:b])
                    t, s, status = gpu.verify_packed(suite, pre, pre_off, sg, sg_off)
                    th.append(t.tobytes())
                    snd.append(s.tobytes())
                    st += status.astype(int).tolist()
                out.append({"leg": "tx/%s/%d" % (name, n or len(pres)), "status": st, "txhash": b"".join(th).hex(),
                            "sender": b"".join(snd).hex()})
        finally:
            gpu.set_tx_kernel_policy()
    return out


def _child(mode):
    import bcos_gpu
    t0 = time.monotonic()
    job = json.loads(sys.stdin.read()) if mode == "tx" else None
    rv.pool()
    if mode == "small":
        bcos_gpu.check(bcos_gpu.lib().bcosgpu_init_ex(0, 1))  # BCOSGPU_INIT_SMALL_TABLES
    bcos_gpu.ensure_device(0)
    t1 = time.monotonic()
    if mode == "sig":
        legs = _sig_legs(bcos_gpu, SIG_POLICIES, SIZES)
    elif mode == "ecrec":
        legs = _ecrec_legs(bcos_gpu)
    elif mode == "tx":
        legs = _tx_legs(bcos_gpu, job)
    else:
        assert mode == "small"
        legs = _sig_legs(bcos_gpu, ("trio", "lane26_occ1"), (0,), "small:")
    print(json.dumps({"legs": legs, "setup_s": t1 - t0, "gpu_s": time.monotonic() - t1}))


# ------------------------------------------------------------------ the parent
def _run(mode, job=None):
    code = _CHILD.format(pkg=PKG, root=ROOT, tests=TESTS, mode=mode)
    env = dict(os.environ)
    env.pop("BCOSGPU_TXV_ROW", None)
    t0 = time.monotonic()
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=TIMEOUT, env=env,
                       input=None if job is None else json.dumps(job))
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print("k1 recover edges child %s: %.1f s wall, %.1f s setup, %.1f s launches, %d legs"
          % (mode, time.monotonic() - t0, out["setup_s"], out["gpu_s"], len(out["legs"])))
    return out["legs"]


def _cut(hexed, width):
    raw = bytes.fromhex(hexed)
    assert len(raw) % width == 0
    return [raw[i:i + width] for i in range(0, len(raw), width)]


def _report(failures):
    for leg, bad in failures.items():
        print("k1 recover edges leg %s: %s" % (leg, json.dumps(bad)))
    assert not failures, sorted(failures)


def _check_sig(legs, oracle):
    rows = rv.pool()
    address_of = lambda pub: oracle.keccak256(pub)[12:]
    failures = {}
    for leg in legs:
        bad = rv.compare(rows, leg["ok"], _cut(leg["pub"], 64), _cut(leg["addr"], 20), address_of)
        if bad:
            failures[leg["leg"]] = bad
    _report(failures)


def test_recovery_batch_every_kernel(oracle):
    """The lane-trio, pair, row, one-lane fe26 (at both occupancies), 8 x 32-bit and automatic choices through
    Secp256k1Crypto.recover_batch, the pool in launches of 1, 39, 40, 41, 65 and all of it: verdict, key, address,
    zeros for a rejected row."""
    legs = _run("sig")
    assert [x["leg"] for x in legs] == ["sig/%s/%d" % (k, n or len(rv.pool())) for k in SIG_POLICIES for n in SIZES]
    _check_sig(legs, oracle)


def test_recovery_batch_small_comb_tables(oracle):
    """BCOSGPU_INIT_SMALL_TABLES: u1 G on the 8-bit comb in the lane-trio and the one-lane fe26 kernels over the
    whole pool, so the u1_shape rows meet the narrow halves of the share tables."""
    legs = _run("small")
    assert [x["leg"] for x in legs] == ["small:sig/%s/%d" % (k, len(rv.pool())) for k in ("trio", "lane26_occ1")]
    _check_sig(legs, oracle)


def test_ecrecover_precompile(oracle):
    """bcosgpu_ecrecover_batch under the trio, row, one-lane fe26 and automatic policies, the whole pool and launches
    of 41, against oracle.ecrecover, which must agree with the rows' expected keys."""
    rows = rv.pool()
    want = []
    for x in rows:
        w = oracle.ecrecover(rv.ecrecover_input(x))
        assert w == (b"" if x[4] is None else bytes(12) + oracle.keccak256(rv.pub_bytes(x[4]))[12:]), x[:2]
        want.append(w)
    legs = _run("ecrec")
    assert [x["leg"] for x in legs] == ["ecrec/%s/%d" % (k, n or len(rows)) for k in ECREC_POLICIES for n in (0, 41)]
    failures = {}
    for leg in legs:
        bad = {}
        for x, w, ok, out in zip(rows, want, leg["ok"], _cut(leg["out"], 32)):
            if bool(ok) != bool(w) or out != (w or bytes(32)):
                bad.setdefault(x[0], []).append(x[1])
        assert len(leg["ok"]) == len(rows)
        if bad:
            failures[leg["leg"]] = bad
    _report(failures)


def test_transaction_verify_all_seven_bodies(oracle):
    """Transaction::verify over 41 fixed transactions: the x_r, s_edge and u2_shape signatures and the final_add rows
    of a fixed e under the policies of all seven bodies, the whole set and launches of 41: status, sender, tx hash."""
    pres = preimages()
    hashes = [oracle.keccak256(p) for p in pres]
    rows = rv.tx_rows(hashes)
    job = {"pre": [pres[j % N_TX].hex() for j in range(len(rows))], "sig": [x[3].hex() for x in rows]}
    legs = _run("tx", job)
    assert [x["leg"] for x in legs] == ["tx/%s/%d" % (k, n or len(rows)) for k in TX_POLICIES for n in (0, 41)]
    failures = {}
    for leg in legs:
        bad = {}
        assert len(leg["status"]) == len(rows)
        for x, st, th, snd in zip(rows, leg["status"], _cut(leg["txhash"], 32), _cut(leg["sender"], 20)):
            want = bytes(20) if x[4] is None else oracle.keccak256(rv.pub_bytes(x[4]))[12:]
            if st != (1 if x[4] is None else 0) or th != x[2] or snd != want:
                bad.setdefault(x[0], []).append(x[1])
        if bad:
            failures[leg["leg"]] = bad
    _report(failures)
