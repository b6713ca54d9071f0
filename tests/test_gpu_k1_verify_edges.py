"""The secp256k1 known-key verify bodies -- secp256k1_verify_lane (8 x 32-bit), secp256k1_verify_lane26,
trio26_verify_body, the row kernel's verify mode, the registered-key kernel -- on the rows of
tests/k1_verify_vectors.py: the second comparison X == (r + n) Z^2, the low-S bound, the key's range checks,
e = hash mod n with hash >= n and u1 = 0, the final addition as a doubling or as infinity, the GLV halves of u2 and
the comb shares of u1 at their edges.  verify() takes the hash as input, so the shipped library meets every row as
it is: no seam.  Every leg's verdicts are compared with the rows' `expected` (the restatement's, pinned to the
oracle on every row by tests/test_k1_verify_vectors.py), never with another kernel's.

Each test starts one child process, which runs its launches and prints the verdicts as JSON with its wall, setup
and launch seconds; the parent compares.  A child that exits nonzero fails its test; nothing is retried.

Promotion to the registered-key cache is off in the children of the generic kernels (BCOSGPU_KEY_PROMOTE=0: a
batch whose keys are all cached would run the registered-key kernel instead), and every leg reports
key_cache_info's `keyed` count before and after: unchanged there, risen by at least the rows where the coalesced
batch must take the registered-key kernel.

Out of scope: bcosgpu_headers_check and bcosgpu_pbft_check.  Their digest is the hash of a header or a message,
so e is not free; they reach the registered-key body, which the slot legs here cover."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import k1_verify_vectors as kv
from test_gpu_verify import SIG_VARIANTS

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
PKG = os.path.join(ROOT, "fisco-bcos_amd")

KERNELS = ("trio", "row", "onelane_occ1", "onelane_occ2", "fe32", "auto")
SIZES = (1, 39, 40, 41, 65, 0)  # kTrioTxs = 40; 0: the whole pool in one launch
SINGLE_CLASSES = ("x_ge_n", "s_edge", "keys")

_CHILD = """
import sys
sys.path[:0] = [{pkg!r}, {root!r}, {tests!r}]
import test_gpu_k1_verify_edges
test_gpu_k1_verify_edges._child({mode!r})
"""


def _arrays(stride=64):
    """hashes uint8[m,32], signatures uint8[m,stride] (a byte that is not read after r || s), keys uint8[m,64]."""
    pk = kv.packed(kv.pool())
    h = np.array([np.frombuffer(a, dtype=np.uint8) for a, _, _ in pk])
    sig = np.array([np.frombuffer(b + b"\xa5" * (stride - 64), dtype=np.uint8) for _, b, _ in pk])
    pub = np.array([np.frombuffer(c, dtype=np.uint8) for _, _, c in pk])
    return h, sig, pub


# ------------------------------------------------------------------ the child
def _legs(gpu, name, policy, sizes, stride):
    """Secp256k1Crypto.verify_batch under a kernel policy, the pool in launches of each size (the last shorter)."""
    h, sig, pub = _arrays(stride)
    crypto = gpu.Secp256k1Crypto()
    m = len(h)
    out = []
    gpu.set_tx_kernel_policy(*policy)
    try:
        for n in sizes:
            n = n or m
            k0 = gpu.key_cache_info(0)["keyed"]
            ok = []
            for a in range(0, m, n):
                ok += crypto.verify_batch(pub[a:a + n], h[a:a + n], sig[a:a + n]).astype(int).tolist()
            out.append({"leg": "%s/%d/%d" % (name, stride, n), "ok": ok, "keyed": [k0, gpu.key_cache_info(0)["keyed"]]})
    finally:
        gpu.set_tx_kernel_policy()
    return out


def _entry_legs(gpu):
    """bcosgpu_verify_batch_dev over the whole pool, and SignatureCrypto::verify one row a call (the coalescer)."""
    import torch
    from bcos_gpu import device
    h, sig, pub = _arrays(65)
    k0 = gpu.key_cache_info(0)["keyed"]
    ok = torch.zeros(len(h), dtype=torch.uint8, device="cuda")
    device.verify(0, torch.from_numpy(pub).cuda(), torch.from_numpy(h).cuda(), torch.from_numpy(sig).cuda(), ok)
    torch.cuda.synchronize()
    k1 = gpu.key_cache_info(0)["keyed"]
    out = [{"leg": "device/65", "ok": ok.cpu().numpy().astype(int).tolist(), "keyed": [k0, k1]}]
    crypto = gpu.Secp256k1Crypto()
    pick = [i for i, x in enumerate(kv.pool()) if x[0] in SINGLE_CLASSES]
    got = [int(crypto.verify(pub[i].tobytes(), h[i].tobytes(), sig[i].tobytes())) for i in pick]
    out.append({"leg": "single", "ok": got, "classes": SINGLE_CLASSES, "keyed": [k1, gpu.key_cache_info(0)["keyed"]]})
    return out


def _keyed_legs(gpu):
    """Every distinct key of the pool registered (the off-curve ones and those with a coordinate above p among
    them): the slot API, then the coalesced known-key verify, which takes the registered-key kernel."""
    import torch
    from bcos_gpu import device
    h, sig, pub = _arrays(64)
    keys = sorted({p.tobytes() for p in pub})
    slots = gpu.register_keys(0, np.array([np.frombuffer(k, dtype=np.uint8) for k in keys]))
    assert (slots >= 0).all() and len(set(slots.tolist())) == len(keys)
    slot_of = dict(zip(keys, slots.tolist()))
    d_slots = torch.tensor([slot_of[p.tobytes()] for p in pub], dtype=torch.int32).cuda()
    ok = torch.zeros(len(h), dtype=torch.uint8, device="cuda")
    device.verify_keyed(0, d_slots, torch.from_numpy(h).cuda(), torch.from_numpy(sig).cuda(), ok)  # by slot: no lookup
    torch.cuda.synchronize()
    k1 = gpu.key_cache_info(0)["keyed"]
    out = [{"leg": "keyed/slots", "ok": ok.cpu().numpy().astype(int).tolist(), "keyed": None}]
    got = gpu.Secp256k1Crypto().verify_batch(pub, h, sig)
    out.append({"leg": "keyed/verify", "ok": got.astype(int).tolist(), "keyed": [k1, gpu.key_cache_info(0)["keyed"]]})
    return out


def _child(mode):
    import bcos_gpu
    t0 = time.monotonic()
    kv.pool()
    if mode == "small":
        bcos_gpu.check(bcos_gpu.lib().bcosgpu_init_ex(0, 1))  # BCOSGPU_INIT_SMALL_TABLES
    bcos_gpu.ensure_device(0)
    t1 = time.monotonic()
    legs = []
    if mode.startswith("generic"):
        for name in KERNELS:
            legs += _legs(bcos_gpu, name, SIG_VARIANTS[name], SIZES, int(mode[7:]))
    elif mode == "small":
        for name in ("trio", "onelane_occ1"):
            legs += _legs(bcos_gpu, "small:" + name, SIG_VARIANTS[name], (41, 0), 64)
    elif mode == "entries":
        legs = _entry_legs(bcos_gpu)
    else:
        assert mode == "keyed"
        legs = _keyed_legs(bcos_gpu)
    print(json.dumps({"legs": legs, "setup_s": t1 - t0, "gpu_s": time.monotonic() - t1}))


# ------------------------------------------------------------------ the parent
def _run(mode, timeout, promote=False):
    code = _CHILD.format(pkg=PKG, root=ROOT, tests=TESTS, mode=mode)
    env = dict(os.environ)
    env.pop("BCOSGPU_KEY_PROMOTE", None)
    env.pop("BCOSGPU_TXV_ROW", None)
    if not promote:
        env["BCOSGPU_KEY_PROMOTE"] = "0"
    t0 = time.monotonic()
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print("k1 edges child %s: %.1f s wall, %.1f s setup, %.1f s launches, %d legs"
          % (mode, time.monotonic() - t0, out["setup_s"], out["gpu_s"], len(out["legs"])))
    return out["legs"]


def _check(legs, keyed):
    """Every leg's verdicts equal the rows' expected ones, and the cache's `keyed` count rose by at least the leg's
    rows (the keyed leg that looks keys up) or not at all."""
    pool = kv.pool()
    failures = {}
    for leg in legs:
        rows = [x for x in pool if x[0] in leg["classes"]] if "classes" in leg else pool
        bad = kv.compare(rows, leg["ok"])
        if leg["keyed"] is not None:
            k0, k1 = leg["keyed"]
            if (k1 - k0 < len(rows)) if keyed else (k1 != k0):
                bad["keyed-count"] = [k0, k1]
        if bad:
            failures[leg["leg"]] = bad
            print("k1 edges leg %s: %s" % (leg["leg"], json.dumps(bad)))
    assert not failures, sorted(failures)


@pytest.mark.parametrize("stride", [64, 65])
def test_every_generic_kernel(stride):
    """The lane-trio, row, one-lane fe26 (at both occupancies), 8 x 32-bit and automatic choices through
    Secp256k1Crypto.verify_batch, the pool in launches of 1, 39, 40, 41, 65 and all of it."""
    legs = _run("generic%d" % stride, 90)
    assert [x["leg"] for x in legs] == ["%s/%d/%d" % (k, stride, n or len(kv.pool())) for k in KERNELS for n in SIZES]
    _check(legs, keyed=False)


def test_device_entry_and_single_calls():
    """bcosgpu_verify_batch_dev (bcos_gpu.device.verify) over the whole pool, and crypto.verify(pub, h, sig) for
    every row of x_ge_n, s_edge and keys."""
    legs = _run("entries", 60)
    assert [x["leg"] for x in legs] == ["device/65", "single"]
    assert len(legs[1]["ok"]) == sum(kv.COUNTS[c] for c in SINGLE_CLASSES)
    _check(legs, keyed=False)


def test_registered_key_kernel():
    """register_keys over every distinct key, then verify_keyed by slot and the coalesced verify_batch over the
    whole pool: the registered-key kernel ran the latter (key_cache_info)."""
    legs = _run("keyed", 60, promote=True)
    assert [x["leg"] for x in legs] == ["keyed/slots", "keyed/verify"]
    _check(legs, keyed=True)


def test_small_comb_tables():
    """BCOSGPU_INIT_SMALL_TABLES: u1 G on the 8-bit comb in the lane-trio and the one-lane fe26 kernels, at 41 and
    the whole pool, so the narrow u1_shape rows meet the narrow shares."""
    legs = _run("small", 60)
    assert len(legs) == 4
    _check(legs, keyed=False)
