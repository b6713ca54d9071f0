#!/usr/bin/env python3
"""Measures the PBFT message check on the GPU and writes profiles/pbft_check.json.

Three shapes over a 100-node consensus set (weight 1 each, quorum 67), both suites, the keys registered:
  one_prepare   one PrePrepare: its signature and its proposal's (2 rows)
  block_round   99 PrePrepares plus 99 Commits (297 rows)
  new_view      a NewView of 67 view changes x 1 prepared proposal x 67 proofs (4,557 rows, one group)
In one process, alternating, with the host clock around calls that end synchronised:
  A   what the drop-in classes do today: one bcosgpu_secp256k1_verify / bcosgpu_sm2_verify per signature, one
      after another from one thread (the message hashes computed outside the timed region);
  A'  INTEGRATION 3c's row-by-row recipe: bcosgpu_hash_batch over the signed data, the hashes scattered into
      rows the caller expanded (keys and signatures outside the timed region), bcosgpu_verify_batch, the fold
      into verdicts in whole-array numpy operations (no per-row Python loop);
  B   bcosgpu_pbft_check over views of the same messages (it maps, packs and folds itself).
The three are checked against each other before a time is kept.  Reported per leg: median, quartiles and the
spread (interquartile range) over the alternations.  Acceptance: B's median is not above A''s by more than A''s
own spread, at every shape and both suites; B against A is reported, not gated.
Needs a gfx950 GPU; there is no fallback."""
import argparse
import ctypes
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
NODES, QUORUM = 100, 67
MSG, PROP, PREP = 1, 2, 4


def scalar(rng):
    return b"\x00" + rng.bytes(30) + b"\x01"


class World:
    """A seeded consensus set and its signer."""

    def __init__(self, oracle, suite, seed):
        from bcos_gpu.header import ConsensusSet
        self.oracle, self.suite, self.rng = oracle, suite, np.random.default_rng(seed)
        self.sks = [scalar(self.rng) for _ in range(NODES)]
        self.pubs = [(oracle.secp256k1_pubkey if suite == 0 else oracle.sm2_pubkey)(sk) for sk in self.sks]
        self.cs = ConsensusSet(node_ids=self.pubs, weights=[1] * NODES, min_required_quorum=QUORUM)

    def sign(self, k, hh):
        return (self.oracle.secp256k1_sign if self.suite == 0 else self.oracle.sm2_sign)(self.sks[k], hh, scalar(self.rng))

    def digest(self, data):
        return self.oracle.hash_(self.suite, data)  # hasher id == suite id (Keccak-256 / SM3)

    def message(self, frm, checks, given=False):
        """A message from node `frm` over 40 bytes of hashFieldsData (or, given: the codec's payload hash)."""
        from bcos_gpu.pbft import PBFTMessage
        m = PBFTMessage(generated_from=frm, checks=checks, signed_data=self.rng.bytes(40))
        hh = self.digest(m.signed_data)
        if given:
            m.signature_hash, m.signed_data = hh, b""
        m.signature = self.sign(frm, hh)
        if checks & PROP:
            m.proposal_hash = self.rng.bytes(32)
            m.proposal_signature = self.sign(frm, m.proposal_hash)
        return m

    def shapes(self):
        from bcos_gpu.header import HeaderSignature
        from bcos_gpu.pbft import PrecommitProof
        one = [self.message(0, MSG | PROP)]
        block = [self.message(k, MSG | PROP) for k in range(1, NODES)] + [self.message(k, MSG) for k in range(1, NODES)]
        # every view change carries the same prepared proposal with the same 67 proofs, as on a real chain
        ph = self.rng.bytes(32)
        proof = PrecommitProof(hash=ph, proofs=[HeaderSignature(k, self.sign(k, ph)) for k in range(QUORUM)])
        new_view = [self.message(99, MSG, given=True)]
        for k in range(QUORUM):
            vc = self.message(k, MSG | PREP, given=True)
            vc.prepared = [proof]
            new_view.append(vc)
        return (("one_prepare", one, []), ("block_round", block, []), ("new_view", new_view, [(0, 1, QUORUM)]))


class Legs:
    def __init__(self, world, msgs, groups):
        from bcos_gpu import _lib, pbft
        from bcos_gpu.crypto import _ptr, pack_messages
        from bcos_gpu.header import consensus_view
        self.L, self.check, self.ptr, self.suite = _lib.lib(), _lib.check, _ptr, world.suite
        cs, n = world.cs, len(msgs)
        self.n, self.groups, self.quorum = n, groups, cs.min_required_quorum
        # the rows the caller of A and A' expands: (message, key, signature, given hash or None = the message's)
        rows, self.msg_row, self.prop_row, self.prep_seg = [], [], [], []
        for i, m in enumerate(msgs):
            self.msg_row.append(len(rows))
            rows.append((cs.node_ids[m.generated_from], m.signature, None, i))
            if m.checks & PROP:
                self.prop_row.append((i, len(rows)))
                rows.append((cs.node_ids[m.generated_from], m.proposal_signature, m.proposal_hash, i))
            for pp in m.prepared:
                self.prep_seg.append((i, len(rows), len(pp.proofs)))
                rows += [(cs.node_ids[pr.index], pr.signature, pp.hash, i) for pr in pp.proofs]
        self.rows = len(rows)
        self.row_pub = np.frombuffer(b"".join(r[0] for r in rows), dtype=np.uint8).copy()
        self.row_sig = np.frombuffer(b"".join(r[1][:64] for r in rows), dtype=np.uint8).copy()
        self.row_hash = np.frombuffer(b"".join(r[2] or bytes(32) for r in rows), dtype=np.uint8).reshape(-1, 32).copy()
        self.msg_row = np.array(self.msg_row)
        self.row_weight = np.ones(self.rows, dtype=np.uint64)
        # the index arrays of A''s fold (part of the caller's expansion, outside the timed region): the proposal
        # rows and their messages; the proof rows gathered back to back with the start of each prepared proposal
        # in them (every proposal has proofs here, so reduceat sees no empty segment); the messages that have
        # prepared proposals with the start of each one's run of proposals
        self.prop_msg = np.array([i for i, _ in self.prop_row], dtype=np.int64)
        self.prop_rows = np.array([r for _, r in self.prop_row], dtype=np.int64)
        assert all(cnt > 0 for _, _, cnt in self.prep_seg)
        self.proof_idx = np.array([r + k for _, r, cnt in self.prep_seg for k in range(cnt)], dtype=np.int64)
        self.seg_off = np.cumsum([0] + [cnt for _, _, cnt in self.prep_seg[:-1]], dtype=np.int64) \
            if self.prep_seg else np.zeros(0, dtype=np.int64)
        owners = [i for i, _, _ in self.prep_seg]
        self.prep_msgs = np.array(sorted(set(owners)), dtype=np.int64)
        self.prep_msg_off = np.array([owners.index(i) for i in self.prep_msgs], dtype=np.int64)
        self.proof_weight = self.row_weight[self.proof_idx]
        self.msg_weight = np.array([cs.weights[m.generated_from] for m in msgs], dtype=np.uint64)
        self.hashed = np.array([i for i, m in enumerate(msgs) if not m.signature_hash], dtype=np.int64)
        self.data, self.off = pack_messages([msgs[i].signed_data for i in self.hashed])
        self.given = np.frombuffer(b"".join(m.signature_hash.ljust(32, b"\0") for m in msgs), dtype=np.uint8) \
            .reshape(-1, 32).copy()
        self.ap_hash = np.zeros((max(len(self.hashed), 1), 32), dtype=np.uint8)
        self.ap_ok = np.zeros(self.rows, dtype=np.uint8)
        # A: per row the pointers of a single call, the message hashes from outside the timed region
        full = self.row_hash.copy()
        full[self.msg_row] = np.frombuffer(b"".join(world.digest(m.signed_data) if not m.signature_hash else
                                                    m.signature_hash for m in msgs), dtype=np.uint8).reshape(-1, 32)
        self.a_hash = full
        base = (self.row_pub.ctypes.data, full.ctypes.data, self.row_sig.ctypes.data)
        self.a_args = [(base[0] + 64 * r, base[1] + 32 * r, base[2] + 64 * r) for r in range(self.rows)]
        self.a_ok = np.zeros(self.rows, dtype=np.uint8)
        # B: views of the same messages
        self.views, self.keep = pbft.message_views(msgs)
        self.cv, self.ckeep = consensus_view(cs)
        self.cvp = ctypes.byref(self.cv)
        self.gv = (pbft._PBFTGroupView * max(len(groups), 1))(*[pbft._PBFTGroupView(*g) for g in groups])
        self.b_hash = np.zeros((n, 32), dtype=np.uint8)
        self.b_flags = np.zeros(n, dtype=np.uint32)
        self.b_prep = np.zeros(max(len(self.prep_seg), 1), dtype=np.uint8)

    def a(self):
        L, ok = self.L, self.a_ok
        if self.suite == 0:
            for r, (pub, hh, sig) in enumerate(self.a_args):
                ok[r] = L.bcosgpu_secp256k1_verify(0, pub, hh, sig, 64)
        else:
            for r, (pub, hh, sig) in enumerate(self.a_args):
                ok[r] = L.bcosgpu_sm2_verify(0, pub, hh, sig)

    def a_prime(self):
        L, p = self.L, self.ptr
        hashes = self.given.copy()
        if len(self.hashed):
            self.check(L.bcosgpu_hash_batch(self.suite, p(self.data), p(self.off), len(self.hashed), p(self.ap_hash)))
            hashes[self.hashed] = self.ap_hash[:len(self.hashed)]
        rows = self.row_hash.copy()
        rows[self.msg_row] = hashes  # the host expansion: each message hash into its signature row
        self.check(L.bcosgpu_verify_batch(self.suite, p(self.row_pub), p(rows), p(self.row_sig), 64, self.rows,
                                          p(self.ap_ok)))
        self.ap_hashes = hashes
        self.ap_flags, self.ap_prep = self.fold()

    def fold(self):
        """A''s fold of ap_ok into (msg_flags, prepared_check), in whole-array operations as tools/headerbench.py's
        (one pass per group: there is at most one)."""
        ok = self.ap_ok == 1
        flags = np.where(ok[self.msg_row], 0, 2).astype(np.uint32)
        if len(self.prop_msg):  # a message has at most one proposal row: the indices are distinct
            flags[self.prop_msg] |= np.where(ok[self.prop_rows], 0, 4).astype(np.uint32)
        prep = np.zeros(0, dtype=np.uint8)
        if len(self.seg_off):
            all_ok = np.minimum.reduceat(self.ap_ok[self.proof_idx], self.seg_off) == 1
            weight = np.add.reduceat(self.proof_weight, self.seg_off)
            prep = np.where(~all_ok, 1, np.where(weight < self.quorum, 2, 0)).astype(np.uint8)
            flags[self.prep_msgs] |= np.where(np.maximum.reduceat(prep, self.prep_msg_off) != 0, 8, 0).astype(np.uint32)
        own = flags.copy()
        for parent, first, count in self.groups:
            if own[first:first + count].any():
                flags[parent] |= 16
            if int(self.msg_weight[first:first + count].sum()) < self.quorum:
                flags[parent] |= 32
        return flags, prep

    def b(self):
        self.check(self.L.bcosgpu_pbft_check(self.suite, self.views, self.n, self.gv, len(self.groups), self.cvp, 0,
                                             self.ptr(self.b_hash), self.ptr(self.b_flags), self.ptr(self.b_prep), None))


def quart(xs):
    xs = sorted(xs)
    q = statistics.quantiles(xs, n=4)
    return {"median_ms": float(statistics.median(xs)), "p25_ms": q[0], "p75_ms": q[2], "spread_ms": q[2] - q[0],
            "min_ms": xs[0], "max_ms": xs[-1], "samples": len(xs)}


def measure(legs, alternations, warmup):
    for _ in range(warmup):
        legs.a()
        legs.a_prime()
        legs.b()
    assert (legs.a_ok == 1).all(), "a single call rejected a valid signature"
    assert np.array_equal(legs.ap_hashes, legs.b_hash), "message hashes differ between A' and B"
    assert np.array_equal(legs.ap_flags, legs.b_flags) and not legs.b_flags.any(), "verdicts differ between A' and B"
    assert np.array_equal(legs.ap_prep, legs.b_prep[:len(legs.prep_seg)])
    assert np.array_equal(legs.a_hash[legs.msg_row], legs.b_hash)
    ta, tp, tb = [], [], []
    for _ in range(alternations):
        t0 = time.perf_counter()
        legs.a()
        t1 = time.perf_counter()
        legs.a_prime()
        t2 = time.perf_counter()
        legs.b()
        t3 = time.perf_counter()
        ta.append((t1 - t0) * 1e3)
        tp.append((t2 - t1) * 1e3)
        tb.append((t3 - t2) * 1e3)
    a, ap, b = quart(ta), quart(tp), quart(tb)
    return {"rows": legs.rows, "messages": legs.n, "A": a, "A_prime": ap, "B": b,
            "b_over_a_prime": b["median_ms"] / ap["median_ms"], "a_over_b": a["median_ms"] / b["median_ms"],
            "accepted": bool(b["median_ms"] <= ap["median_ms"] + ap["spread_ms"])}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--alternations", type=int, default=60, help="timed alternations per shape and suite (>= 50)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pbft_check.json"))
    args = ap.parse_args()

    import torch
    import bcos_gpu
    from oracle import oracle
    oracle.build()
    bcos_gpu.ensure_device(0)
    res = {"input": {"consensus_set": "%d nodes, weight 1 each, quorum %d" % (NODES, QUORUM), "seed": args.seed,
                     "one_prepare": "1 PrePrepare (message and proposal signature)",
                     "block_round": "99 PrePrepares + 99 Commits",
                     "new_view": "1 NewView + 67 view changes x 1 prepared proposal x 67 proofs, one group"},
           "method": {"clock": "time.perf_counter around calls that end synchronised; A, A' and B alternate in one "
                               "process",
                      "alternations": args.alternations, "warmup": args.warmup,
                      "spread": "interquartile range (p75 - p25) of the leg's samples",
                      "acceptance": "B median <= A' median + A' spread (B against A is reported, not gated)",
                      "device": torch.cuda.get_device_name(0),
                      "A": "one bcosgpu_secp256k1_verify / bcosgpu_sm2_verify per row from one thread (message "
                           "hashes computed outside the timed region)",
                      "A_prime": "bcosgpu_hash_batch + numpy scatter into the expanded rows + bcosgpu_verify_batch + "
                                 "numpy fold (the rows' keys and signatures expanded outside the timed region)",
                      "B": "bcosgpu_pbft_check over message views (maps, packs and folds inside the call)"},
           "shapes": {}}
    for sname, suite in SUITES:
        world = World(oracle, suite, args.seed + suite)
        bcos_gpu.register_keys(suite, np.frombuffer(b"".join(world.pubs), dtype=np.uint8).reshape(-1, 64))
        for shape, msgs, groups in world.shapes():
            r = measure(Legs(world, msgs, groups), args.alternations, args.warmup)
            res["shapes"].setdefault(shape, {})[sname] = r
            print(shape, sname, json.dumps(r), flush=True)
        res.setdefault("key_cache", {})[sname] = bcos_gpu.key_cache_info(suite)
    res["accepted"] = all(r["accepted"] for shape in res["shapes"].values() for r in shape.values())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
