#!/usr/bin/env python3
"""Measures the block-header check on the GPU and writes profiles/header_check.json.

Two shapes, both suites, the consensus keys registered:
  catch_up   1,000 consecutive headers x 7 sealers (weight 1 each, quorum 5) x 5 signatures
  single     one such header
In one process, alternating, with the host clock around calls that end synchronised:
  A  what the library offered before bcosgpu_headers_check: the preimages packed outside the timed region, then
     bcosgpu_hash_batch, the expansion of the header hashes to one per signature row (numpy), bcosgpu_verify_batch
     and a numpy fold of the rows into verdicts -- the hash and verify calls taking host pointers;
  B  bcosgpu_headers_check over views of the same headers (it packs them itself).
Both are checked against each other (hashes, verdicts) before a time is kept.  Reported per leg: median, quartiles
and the spread (interquartile range) over the alternations.  Acceptance: B's median is not above A's by more than
A's own spread.

--trace SUITE runs only B's catch-up shape a few times, for a separate `rocprofv3 --kernel-trace --stats` run;
--kernel-stats SUITE=DIR merges that run's per-kernel times into the JSON (the hash phase's share of B's GPU time).
Needs a gfx950 GPU; there is no fallback."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

SUITES = (("secp256k1", 0), ("sm2", 1))
SEALERS, SIGNERS, QUORUM = 7, 5, 5


def scalar(rng):
    return b"\x00" + rng.bytes(30) + b"\x01"


def make_run(oracle, suite, n, seed):
    """n linked headers signed by 5 of the 7 sealers each: (headers, consensus set)."""
    from bcos_gpu.header import BlockHeader, ConsensusSet, HeaderSignature, pack_headers
    rng = np.random.default_rng(seed)
    sks = [scalar(rng) for _ in range(SEALERS)]
    pubs = [(oracle.secp256k1_pubkey if suite == 0 else oracle.sm2_pubkey)(sk) for sk in sks]
    cs = ConsensusSet(node_ids=pubs, weights=[1] * SEALERS, min_required_quorum=QUORUM, committed_index=0)
    sign = oracle.secp256k1_sign if suite == 0 else oracle.sm2_sign
    headers, prev = [], (9, rng.bytes(32))
    for i in range(n):
        h = BlockHeader(version=0x03020000, parents=[prev], txs_root=rng.bytes(32), receipt_root=rng.bytes(32),
                        state_root=rng.bytes(32), number=10 + i, gas_used=str(int(rng.integers(0, 10**9))).encode(),
                        timestamp=1700000000000 + i, sealer=i % SEALERS, sealer_list=list(pubs), extra_data=b"",
                        consensus_weights=[1] * SEALERS, tx_count=1000)
        data, _ = pack_headers([h])
        hh = oracle.hash_(suite, data.tobytes())  # hasher id == suite id (Keccak-256 / SM3)
        who = rng.permutation(SEALERS)[:SIGNERS]
        h.signatures = [HeaderSignature(int(k), sign(sks[int(k)], hh, scalar(rng))) for k in who]
        headers.append(h)
        prev = (h.number, hh)
    return headers, cs


class Legs:
    def __init__(self, suite, headers, cs):
        from bcos_gpu import _lib, header
        from bcos_gpu.crypto import _ptr
        self.L, self.check, self.ptr, self.suite = _lib.lib(), _lib.check, _ptr, suite
        n = self.n = len(headers)
        # A's inputs: packed preimages, the rows' keys and signatures, the rows' weights
        self.data, self.off = header.pack_headers(headers)
        self.row_pub = np.frombuffer(b"".join(cs.node_ids[s.index] for h in headers for s in h.signatures),
                                     dtype=np.uint8).copy()
        self.row_sig = np.frombuffer(b"".join(s.signature[:64] for h in headers for s in h.signatures),
                                     dtype=np.uint8).copy()
        self.row_w = np.array([cs.weights[s.index] for h in headers for s in h.signatures], dtype=np.uint64)
        self.a_hash = np.zeros((n, 32), dtype=np.uint8)
        self.a_ok = np.zeros(n * SIGNERS, dtype=np.uint8)
        self.quorum = cs.min_required_quorum
        # B's inputs: views of the same headers
        self.views, self.keep = header.header_views(headers)
        self.cv, self.ckeep = header.consensus_view(cs)
        self.b_hash = np.zeros((n, 32), dtype=np.uint8)
        self.b_check = np.zeros(n, dtype=np.uint8)
        self.b_link = np.zeros(n, dtype=np.uint8)
        self.b_ok = np.zeros(n * SIGNERS, dtype=np.uint8)
        import ctypes
        self.cvp = ctypes.byref(self.cv)

    def a(self):
        L, p = self.L, self.ptr
        self.check(L.bcosgpu_hash_batch(self.suite, p(self.data), p(self.off), self.n, p(self.a_hash)))
        rows = np.repeat(self.a_hash, SIGNERS, axis=0)  # the host expansion: one hash per signature row
        self.check(L.bcosgpu_verify_batch(self.suite, p(self.row_pub), p(rows), p(self.row_sig), 64, rows.shape[0],
                                          p(self.a_ok)))
        ok = self.a_ok.reshape(self.n, SIGNERS)
        weight = (self.row_w.reshape(self.n, SIGNERS)).sum(axis=1)
        self.a_check = np.where(~ok.all(axis=1), 19, np.where(weight < self.quorum, 20, 0)).astype(np.uint8)

    def b(self):
        self.check(self.L.bcosgpu_headers_check(self.suite, self.views, self.n, self.cvp, None, 0, 0,
                                                self.ptr(self.b_hash), self.ptr(self.b_check), self.ptr(self.b_link),
                                                self.ptr(self.b_ok)))


def quart(xs):
    xs = sorted(xs)
    q = statistics.quantiles(xs, n=4)
    return {"median_ms": float(statistics.median(xs)), "p25_ms": q[0], "p75_ms": q[2], "spread_ms": q[2] - q[0],
            "min_ms": xs[0], "max_ms": xs[-1], "samples": len(xs)}


def measure(legs, alternations, warmup):
    for _ in range(warmup):
        legs.a()
        legs.b()
    assert np.array_equal(legs.a_hash, legs.b_hash), "header hashes differ between A and B"
    assert np.array_equal(legs.a_check, legs.b_check) and not legs.b_check.any(), "verdicts differ between A and B"
    assert np.array_equal(legs.a_ok, legs.b_ok) and (legs.b_link[1:] == 1).all()
    ta, tb = [], []
    for _ in range(alternations):
        t0 = time.perf_counter()
        legs.a()
        t1 = time.perf_counter()
        legs.b()
        t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3)
        tb.append((t2 - t1) * 1e3)
    a, b = quart(ta), quart(tb)
    return {"A": a, "B": b, "b_over_a": b["median_ms"] / a["median_ms"],
            "accepted": bool(b["median_ms"] <= a["median_ms"] + a["spread_ms"])}


def kernel_stats(d):
    out = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row["Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").strip()
                out[name] = {"calls": int(row["Calls"]), "avg_ns": float(row["AverageNs"]),
                                                          "total_ns": float(row["TotalDurationNs"])}
    return out


def phase_of(name):
    return ("hash" if "header_hash_kernel" in name else "verdict" if "header_verdict_kernel" in name else
            "verify" if "sig_verify" in name else None)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--headers", type=int, default=1000)
    ap.add_argument("--alternations", type=int, default=60, help="timed A/B alternations per shape and suite (>= 50)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "header_check.json"))
    ap.add_argument("--trace", choices=[s for s, _ in SUITES], help="only run B's catch-up shape (for rocprofv3)")
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="SUITE=DIR",
                    help="merge a rocprofv3 --kernel-trace --stats output directory into --out")
    args = ap.parse_args()

    if args.kernel_stats:
        with open(args.out) as f:
            res = json.load(f)
        for item in args.kernel_stats:
            suite, d = item.split("=", 1)
            ks = {k: v for k, v in kernel_stats(d).items() if phase_of(k)}
            assert ks, "no kernel of the header check in " + d
            total = sum(v["total_ns"] for v in ks.values())
            phases = {}
            for k, v in ks.items():
                phases[phase_of(k)] = phases.get(phase_of(k), 0.0) + v["total_ns"]
            res["kernels_catch_up"][suite] = {"kernels": ks, "share": {p: t / total for p, t in phases.items()}}
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
        print("merged kernel stats into", args.out)
        return

    import torch
    import bcos_gpu
    from oracle import oracle
    oracle.build()
    bcos_gpu.ensure_device(0)
    if args.trace:
        suite = dict(SUITES)[args.trace]
        headers, cs = make_run(oracle, suite, args.headers, args.seed + suite)
        legs = Legs(suite, headers, cs)
        for _ in range(20):
            legs.b()
        assert not legs.b_check.any()
        print("traced 20 calls of B,", args.trace)
        return

    res = {"input": {"catch_up": "%d headers x %d sealers x %d signatures" % (args.headers, SEALERS, SIGNERS),
                     "single": "1 header x %d sealers x %d signatures" % (SEALERS, SIGNERS), "seed": args.seed},
           "method": {"clock": "time.perf_counter around calls that end synchronised; A and B alternate in one process",
                      "alternations": args.alternations, "warmup": args.warmup,
                      "spread": "interquartile range (p75 - p25) of the leg's samples",
                      "acceptance": "B median <= A median + A spread", "device": torch.cuda.get_device_name(0),
                      "A": "bcosgpu_hash_batch + numpy expansion to rows + bcosgpu_verify_batch + numpy fold "
                           "(preimages packed outside the timed region)",
                      "B": "bcosgpu_headers_check over header views (packs inside the call)"},
           "shapes": {}, "kernels_catch_up": {}}
    for sname, suite in SUITES:
        headers, cs = make_run(oracle, suite, args.headers, args.seed + suite)
        bcos_gpu.register_keys(suite, np.frombuffer(b"".join(cs.node_ids), dtype=np.uint8).reshape(-1, 64))
        for shape, hs in (("catch_up", headers), ("single", headers[:1])):
            r = measure(Legs(suite, hs, cs), args.alternations, args.warmup)
            res["shapes"].setdefault(shape, {})[sname] = r
            print(shape, sname, json.dumps(r), flush=True)
        info = bcos_gpu.key_cache_info(suite)
        res.setdefault("key_cache", {})[sname] = info
    res["accepted"] = all(r["accepted"] for shape in res["shapes"].values() for r in shape.values())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
