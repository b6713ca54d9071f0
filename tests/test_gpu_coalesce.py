"""The coalescer under a mixed workload, and its kernels overlapping without it.

test_mixed_calls: tests/cpp/coalesce_mix_test.cpp calls every host-pointer signature entry point of the C ABI from
many threads of one process -- single and batched recover (n = 2..300 and one of 2,500, past the zero-copy
staging), named-key verifies of both suites (few keys, so they are promoted to the registered-key kernel in the
middle of the run), embedded-key SM2 batches and known-key batches at strides 64 and 65 / 128 -- so jobs of all
three kinds and every shape share the queue (csrc/coalesce.hip, csrc/coalesce_queue.h), at the defaults and with
each BCOSGPU_COALESCE_* knob set.  A quarter of the items carry the edge mutations of test_gpu_ecc; the oracle
computes every expected value, the device only signs.  Every output has guard bytes on both sides, and a mismatch is
reported with tests/cpp/mismatch_record.h's records: other_item points to staging, scatter or the queue; untouched
or zeros with test_small_batches_overlap_on_streams and ZEROCOPY=0 clean points to the visibility of the zero-copy
output.  One child runs at a time; after a child that timed out, died of a signal or reported an engine (HIP) error
nothing more of this module starts.

test_small_batches_overlap_on_streams: the kernels alone -- four torch streams of different priorities each
launching 40 batches of 1, 3 and 20 signatures (the row kernels' range) back to back, one synchronisation at the
end -- with the automatic kernel choice and with the row kernels forced.
"""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from test_cpp_adapter import LIBDIR, ROOT
from test_gpu_ecc import _dev_sign, _mutate, _mutate_sm2

pytestmark = pytest.mark.gpu

M = 4096      # items per set of the data file
KEYS = 8      # distinct named keys of the verify sets
GUARD = 0xA5
ROW = (1, 0, 3, 1)
STREAM_SIZES = [(1, 3, 20)[b % 3] for b in range(40)]  # per stream: 40 batches in the row kernels' range
STREAM_ITEMS = 4 * sum(STREAM_SIZES)


class _Sets:
    pass


@pytest.fixture(scope="module")
def sets(gpu, oracle):
    """The four sets of the data file, every expected value from the oracle (computed once for the module)."""
    rng = np.random.default_rng(900)
    s = _Sets()

    def signed(suite, keys):
        sk = rng.integers(0, 256, size=(keys, 32), dtype=np.uint8)
        sk[:, 0] &= 0x7F
        sk = sk[np.arange(M) % keys]
        h = rng.integers(0, 256, size=(M, 32), dtype=np.uint8)
        pub, sig, _ = _dev_sign(gpu, suite, sk, h)
        # a quarter of the items carry the reference's edge cases (bad v, r = n, s = 0, flipped bits, ...); the kind
        # cycles with the count of mutated items (i % 4 == 1 alone would leave i % 8 at 1 and 5)
        kinds = 9 if suite == 0 else 8
        kind = [(i // 4) % kinds if i % 4 == 1 else 0 for i in range(M)]
        sig = np.array([np.frombuffer((_mutate if suite == 0 else _mutate_sm2)(rng, sig[i].tobytes(), kind[i]),
                                      dtype=np.uint8) for i in range(M)])
        # every kind occurs, in the whole set and in the part the stream test launches
        assert set(kind) == set(kind[:STREAM_ITEMS]) == set(range(kinds))
        if suite == 0:  # the device signed; the oracle derives the keys
            for i in range(0, M, max(1, M // 64)):
                assert pub[i].tobytes() == oracle.secp256k1_pubkey(sk[i].tobytes())
        return h, sig, np.ascontiguousarray(pub)

    s.rk_h, s.rk_sig, _ = signed(0, M)
    s.rk_pub, s.rk_ok = oracle.secp256k1_recover_batch(s.rk_h, s.rk_sig, nthreads=16)
    s.rk_pub[~s.rk_ok] = 0
    s.rk_addr = np.zeros((M, 20), dtype=np.uint8)
    for i in np.nonzero(s.rk_ok)[0]:
        s.rk_addr[i] = np.frombuffer(oracle.keccak256(s.rk_pub[i].tobytes())[12:], dtype=np.uint8)

    s.vk_h, s.vk_sig, s.vk_key = signed(0, KEYS)
    s.vk_ok = np.array([oracle.secp256k1_verify(s.vk_key[i].tobytes(), s.vk_h[i].tobytes(), s.vk_sig[i, :64].tobytes())
                        for i in range(M)])

    s.rs_h, s.rs_sig, _ = signed(1, M)
    s.rs_ok = oracle.sm2_verify_batch(s.rs_h, s.rs_sig, nthreads=16)
    s.rs_addr = np.zeros((M, 20), dtype=np.uint8)
    for i in np.nonzero(s.rs_ok)[0]:
        s.rs_addr[i] = np.frombuffer(oracle.sm3(s.rs_sig[i, 64:].tobytes())[12:], dtype=np.uint8)

    s.vs_h, s.vs_sig, _ = signed(1, KEYS)
    s.vs_ok = oracle.sm2_verify_batch(s.vs_h, s.vs_sig, nthreads=16)
    for ok in (s.rk_ok, s.vk_ok, s.rs_ok, s.vs_ok):
        assert M // 2 < ok.sum() < M
    return s


@pytest.fixture(scope="module")
def mix(sets, tmp_path_factory):
    d = tmp_path_factory.mktemp("coalesce_mix")
    exe = str(d / "coalesce_mix_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "coalesce_mix_test.cpp"), "-L" + LIBDIR, "-lbcosgpu",
                    "-Wl,-rpath," + LIBDIR, "-lpthread"], check=True)
    data = str(d / "mix.bin")
    s = sets
    with open(data, "wb") as f:
        f.write(b"BGMX" + struct.pack("<I", M))
        for a in (s.rk_h, s.rk_sig, s.rk_ok, s.rk_pub, s.rk_addr, s.vk_h, s.vk_sig, s.vk_key, s.vk_ok,
                  s.rs_h, s.rs_sig, s.rs_ok, s.rs_addr, s.vs_h, s.vs_sig, s.vs_ok):
            f.write(np.ascontiguousarray(a).astype(np.uint8).tobytes())
    return exe, data


CASES = [("defaults", {}, 64, 200)]
CASES += [(k + "=" + v, {"BCOSGPU_COALESCE_" + k: v}, 32, 100)
          for k, v in (("ZEROCOPY", "0"), ("LOCKFREE", "0"), ("SLOTS", "1"), ("PRIO", "0"), ("DEEP", "8"))]
CASES += [("WAIT=%d" % w, {"BCOSGPU_COALESCE_WAIT": str(w)}, 16, 100) for w in range(4)]
_died = []  # the case whose child timed out, aborted, died of a signal or met a HIP error: nothing starts after it


@pytest.mark.parametrize("name,env,threads,calls", CASES, ids=[c[0] for c in CASES])
def test_mixed_calls(mix, name, env, threads, calls):
    if _died:
        pytest.fail("not started: the child of case %s %s" % _died[0])
    exe, data = mix
    full = {k: v for k, v in os.environ.items() if not k.startswith("BCOSGPU_COALESCE_")}
    full.update(env)
    try:
        # (a run is a second or two, with the engine's start: tables, streams, staging)
        r = subprocess.run([exe, data, str(threads), str(calls)], capture_output=True, text=True, timeout=30, env=full)
    except subprocess.TimeoutExpired:
        _died.append((name, "timed out"))
        raise
    if r.returncode < 0 or r.returncode in (134, 139):
        _died.append((name, "ended with status %d" % r.returncode))
    lines = r.stdout.strip().splitlines()
    res = json.loads(lines[-1]) if lines and lines[-1].startswith("{") else {}
    if res.get("engine_errors") or (r.returncode != 0 and not res):
        # a HIP error inside the engine (an illegal memory access, say) is a GPU fault even when the child goes on
        _died.append((name, "reported engine errors: " + (lines[-1][:300] if lines else r.stderr[-300:])))
    if res.get("mismatches") or res.get("guard_violations"):
        for rec in res["records"]:
            print("mismatch:", rec)
        print("coalesce_stats:", res["coalesce_stats"], "key_cache:", res["key_cache"])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    print({k: v for k, v in res.items() if k != "records"})
    assert res["mismatches"] == 0 and res["engine_errors"] == 0 and res["guard_violations"] == 0
    assert res["calls"] == threads * calls == res["coalesce_stats"][1]  # every call was one job of the queue
    assert res["coalesce_stats"][2] == res["items"] and res["coalesce_stats"][0] <= res["calls"]
    assert all(n > 0 for n in res["ops"])
    if name == "defaults":
        # the named keys were promoted in the middle of the run: both kernel families verified
        for cached, _, keyed, elsewhere, _ in res["key_cache"]:
            assert cached > 0 and keyed > 0 and elsewhere > 0


def _priorities():
    import torch
    try:
        least, greatest = torch.cuda.Stream.priority_range()
    except AttributeError:
        least, greatest = 0, -1
    return list(range(least, greatest - 1, -1))


@pytest.mark.parametrize("policy", [None, ROW], ids=["auto", "row"])
def test_small_batches_overlap_on_streams(gpu, sets, policy):
    """Suspect (c) on its own: small launches of both suites overlapping on streams of different priorities, no
    coalescer.  Disjoint guard-filled outputs, one synchronisation, every item against the oracle."""
    if _died:
        pytest.fail("not started: the child of case %s %s" % _died[0])
    import torch
    from bcos_gpu import device
    s = sets
    prios = _priorities()
    streams = [torch.cuda.Stream(priority=prios[k % len(prios)]) for k in range(4)]
    sizes = STREAM_SIZES
    per_stream = sum(sizes)
    total = STREAM_ITEMS
    assert total <= M
    d = {k: torch.from_numpy(np.ascontiguousarray(getattr(s, k)[:total])).cuda() for k in ("rk_h", "rk_sig", "rs_h", "rs_sig")}
    pub = torch.full((total, 64), GUARD, dtype=torch.uint8, device="cuda")
    addr = torch.full((total, 20), GUARD, dtype=torch.uint8, device="cuda")
    ok = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    addr2 = torch.full((total, 20), GUARD, dtype=torch.uint8, device="cuda")
    ok2 = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu.set_tx_kernel_policy(*policy) if policy else gpu.set_tx_kernel_policy()
    try:
        at = [k * per_stream for k in range(4)]
        for n in sizes:  # round-robin on the host: each stream's launches are back to back, nothing waits
            for k, st in enumerate(streams):
                a, b = at[k], at[k] + n
                device.secp256k1_recover(d["rk_h"][a:b], d["rk_sig"][a:b], pub[a:b], addr[a:b], ok[a:b], stream=st)
                device.sm2_verify(d["rs_h"][a:b], d["rs_sig"][a:b], addr2[a:b], ok2[a:b], stream=st)
                at[k] = b
        torch.cuda.synchronize()
    finally:
        gpu.set_tx_kernel_policy()
    pub, addr, ok, addr2, ok2 = (x.cpu().numpy() for x in (pub, addr, ok, addr2, ok2))
    want = s.rk_ok[:total]
    assert np.array_equal(ok, want.astype(np.uint8)), np.nonzero(ok != want)[0][:16]
    assert np.array_equal(pub, s.rk_pub[:total]), np.nonzero((pub != s.rk_pub[:total]).any(axis=1))[0][:16]
    assert np.array_equal(addr, s.rk_addr[:total])  # (zero for an invalid signature, as the key)
    want2 = s.rs_ok[:total]
    assert np.array_equal(ok2, want2.astype(np.uint8)), np.nonzero(ok2 != want2)[0][:16]
    assert np.array_equal(addr2, s.rs_addr[:total])
    assert 0 < want.sum() < total and 0 < want2.sum() < total
