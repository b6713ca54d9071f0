"""The SM2 verify kernels' last steps -- e reduced once mod n, c = r - e mod n, Q = s G + t P, x(Q) against c or
c + n -- on the rows of tests/sm2_vectors.py, whose e is chosen (accepted signatures at every edge a hashed e
never reaches), against its restatement verify(e, r, s, P).

The kernels are those of lib/libbcosgpu_rawe.so: the shipped sources built with -DBCOSGPU_SM2_RAW_E, under which
sm2_e (ecc_device.h) and sm2_e_from_za (ecc_keyed.hip) return the 32 digest bytes as e and nothing else changes;
each kernel's own reduce_once, subtraction, chains, comb, final addition and comparison are the shipped text.
Each test starts one child process that points bcos_gpu._lib.LIB_PATH at that library before its first use, runs
its launches and prints the verdicts as JSON; the parent compares.  A child that dies fails its test.

Promotion to the registered-key cache is off in the children of the generic kernels (BCOSGPU_KEY_PROMOTE=0: a
batch whose keys are all cached would run the registered-key kernel instead, see tests/test_gpu_sm2_small.py),
and every leg reports key_cache_info's `keyed` count before and after.

Out of scope: tx_verify_sm2_pair_kernel (8 x 32-bit, policy (1, 1, 1, 0)) takes TxIO only, where the digest is
itself the hash of the transaction, so its e stays a hash of a hash even in this build."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import sm2_vectors as sv

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
PKG = os.path.join(ROOT, "fisco-bcos_amd")
RAWE = os.path.join(PKG, "lib", "libbcosgpu_rawe.so")

KERNELS = {"trio": (1, 1, 2, 1), "row": (1, 1, 3, 1), "pair26": (1, 1, 1, 1), "lane26": (0, 2, 0, 1),
           "lane32": (0, 2, 0, 0)}
SIZES = (1, 21, 41, 65, 0)  # 0: the whole pool in one launch

_CHILD = """
import sys
sys.path[:0] = [{pkg!r}, {root!r}, {tests!r}]
from bcos_gpu import _lib
_lib.LIB_PATH = {lib!r}
import test_gpu_sm2_raw_e
test_gpu_sm2_raw_e._child({mode!r})
"""


def _arrays():
    pk = sv.packed(sv.pool())
    h = np.array([np.frombuffer(a, dtype=np.uint8) for a, _ in pk])
    sig = np.array([np.frombuffer(b, dtype=np.uint8) for _, b in pk])
    return h, sig, np.ascontiguousarray(sig[:, 64:])


# ------------------------------------------------------------------ the child
def _legs(gpu, name, policy, sizes, h, sig, pub):
    """SM2Crypto::recover over SigIO (with addresses) and known-key verify over KeyIO, the pool in launches of each
    size (the last launch shorter)."""
    crypto = gpu.SM2Crypto()
    m = len(h)
    out = []
    gpu.set_tx_kernel_policy(*policy)
    try:
        for n in sizes:
            n = n or m
            k0 = gpu.key_cache_info(1)["keyed"]
            ok_r, ok_v, addr = [], [], []
            for a in range(0, m, n):
                _, ad, ok = crypto.recover_batch(h[a:a + n], sig[a:a + n], want_address=True)
                ok_r += ok.astype(int).tolist()
                addr += [x.tobytes().hex() for x in ad]
                ok_v += crypto.verify_batch(pub[a:a + n], h[a:a + n], sig[a:a + n]).astype(int).tolist()
            k1 = gpu.key_cache_info(1)["keyed"]
            out.append({"leg": "%s/recover/%d" % (name, n), "ok": ok_r, "addr": addr, "keyed": [k0, k1]})
            out.append({"leg": "%s/verify/%d" % (name, n), "ok": ok_v, "keyed": [k0, k1]})
    finally:
        gpu.set_tx_kernel_policy()
    return out


def _keyed_legs(gpu, h, sig, pub):
    """Every key of the pool registered (the off-curve ones, X = 0 and -G among them): the slot API, then the
    coalesced known-key verify and recover, which take the registered-key kernel."""
    import torch
    from bcos_gpu import device
    keys = sorted({p.tobytes() for p in pub})
    slots = gpu.register_keys(1, np.array([np.frombuffer(k, dtype=np.uint8) for k in keys]))
    assert (slots >= 0).all() and len(set(slots.tolist())) == len(keys)
    slot_of = dict(zip(keys, slots.tolist()))
    d_slots = torch.tensor([slot_of[p.tobytes()] for p in pub], dtype=torch.int32).cuda()
    d_h, d_s = torch.from_numpy(h).cuda(), torch.from_numpy(sig).cuda()
    ok = torch.zeros(len(h), dtype=torch.uint8, device="cuda")
    out = []
    device.verify_keyed(1, d_slots, d_h, d_s, ok)  # by slot: no lookup, so nothing for the cache to count
    torch.cuda.synchronize()
    k1 = gpu.key_cache_info(1)["keyed"]
    out.append({"leg": "keyed/slots", "ok": ok.cpu().numpy().astype(int).tolist(), "keyed": None})
    crypto = gpu.SM2Crypto()
    got = crypto.verify_batch(pub, h, sig)
    k2 = gpu.key_cache_info(1)["keyed"]
    out.append({"leg": "keyed/verify", "ok": got.astype(int).tolist(), "keyed": [k1, k2]})
    _, ad, got = crypto.recover_batch(h, sig, want_address=True)
    k3 = gpu.key_cache_info(1)["keyed"]
    out.append({"leg": "keyed/recover", "ok": got.astype(int).tolist(), "addr": [x.tobytes().hex() for x in ad],
                "keyed": [k2, k3]})
    return out


def _child(mode):
    import bcos_gpu
    t0 = time.monotonic()
    h, sig, pub = _arrays()
    if mode == "small":
        bcos_gpu.check(bcos_gpu.lib().bcosgpu_init_ex(0, 1))  # BCOSGPU_INIT_SMALL_TABLES
    bcos_gpu.ensure_device(0)
    t1 = time.monotonic()
    legs = []
    if mode == "generic":
        for name, pol in KERNELS.items():
            legs += _legs(bcos_gpu, name, pol, SIZES, h, sig, pub)
    elif mode == "schedules":
        for env in ("BCOSGPU_SM2_SPLIT=0", "BCOSGPU_SM2_JAC_ONLY=1"):  # both read at each launch
            k, v = env.split("=")
            os.environ[k] = v
            try:
                legs += _legs(bcos_gpu, "trio:" + env, KERNELS["trio"], (41,), h, sig, pub)
            finally:
                del os.environ[k]
    elif mode == "small":
        for name in ("trio", "lane26", "lane32"):
            legs += _legs(bcos_gpu, "small:" + name, KERNELS[name], (41, 0), h, sig, pub)
    else:
        assert mode == "keyed"
        legs = _keyed_legs(bcos_gpu, h, sig, pub)
    print(json.dumps({"lib": bcos_gpu.lib()._name, "legs": legs, "setup_s": t1 - t0,
                      "gpu_s": time.monotonic() - t1}))


# ------------------------------------------------------------------ the parent
def _run(mode, timeout, promote=False):
    code = _CHILD.format(pkg=PKG, root=ROOT, tests=TESTS, lib=RAWE, mode=mode)
    env = dict(os.environ)
    for k in ("BCOSGPU_SM2_SPLIT", "BCOSGPU_SM2_JAC_ONLY", "BCOSGPU_KEY_PROMOTE"):
        env.pop(k, None)
    if not promote:
        env["BCOSGPU_KEY_PROMOTE"] = "0"
    t0 = time.monotonic()
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print("raw-e child %s: %.1f s wall, %.1f s setup, %.1f s launches, %d legs"
          % (mode, time.monotonic() - t0, out["setup_s"], out["gpu_s"], len(out["legs"])))
    assert os.path.samefile(out["lib"], RAWE)
    return out["legs"]


def _check(legs, oracle, keyed):
    """Every leg's verdicts equal the restatement's, accepted rows carry SM3(pub)[12:] and rejected rows a zero
    address, and the cache's `keyed` count moved by the leg's rows (the keyed legs that look keys up) or not at all."""
    rows = sv.pool()
    want_addr = [oracle.sm3(b"".join(v.to_bytes(32, "big") for v in x[5:7]))[12:].hex() if x[7] else "00" * 20
                 for x in rows]
    failures = {}
    for leg in legs:
        bad = sv.compare(rows, leg["ok"])
        if "addr" in leg:
            wrong = [x[1] for x, a, w in zip(rows, leg["addr"], want_addr) if a != w]
            if wrong:
                bad["address"] = wrong
        if leg["keyed"] is not None:
            k0, k1 = leg["keyed"]
            if (k1 - k0 < len(rows)) if keyed else (k1 != k0):
                bad["keyed-count"] = [k0, k1]
        if bad:
            failures[leg["leg"]] = bad
    assert not failures, failures


def test_recover_and_known_key_verify_every_kernel(oracle):
    """The lane-trio, row, pair26 and the two one-lane kernels over SigIO and KeyIO, the pool in launches of 1, 21,
    41, 65 and all of it."""
    legs = _run("generic", 90)
    assert len(legs) == 2 * len(KERNELS) * len(SIZES)
    _check(legs, oracle, keyed=False)


def test_trio_schedules(oracle):
    """The lane-trio kernel at 41 without the low-window chains (BCOSGPU_SM2_SPLIT=0) and with every window on
    the Jacobian entries (BCOSGPU_SM2_JAC_ONLY=1)."""
    legs = _run("schedules", 60)
    assert len(legs) == 4
    _check(legs, oracle, keyed=False)


def test_registered_key_kernel(oracle):
    """register_keys, then verify_keyed, known-key verify and recover over the whole pool, keyed_lanes included: the
    registered-key kernel ran each (key_cache_info)."""
    legs = _run("keyed", 60, promote=True)
    assert [x["leg"] for x in legs] == ["keyed/slots", "keyed/verify", "keyed/recover"]
    _check(legs, oracle, keyed=True)


def test_small_comb_tables(oracle):
    """BCOSGPU_INIT_SMALL_TABLES: s G on the 8-bit comb in the lane-trio and the one-lane kernels."""
    legs = _run("small", 60)
    assert len(legs) == 12
    _check(legs, oracle, keyed=False)
