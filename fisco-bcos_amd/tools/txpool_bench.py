#!/usr/bin/env python3
"""Measures transaction admission with the pool's state (bcosgpu_txpool_*) and writes
profiles/txpool_admit.json.  Not a leg of bench.py.

Workload: the 10,000-transaction secp256k1 batch of synth.tars_encodings (the C2 batch); a pool of 15,000 hashes
and nonces (txpool.limit's default), put there by admitting 15,000 other synthetic transactions; a ledger set of
1,000,000 random nonces in 1,000 remembered blocks (block_limit_range 1,000).

Reported, each the median of --reps runs (min and max beside it), by a host clock around calls that end in a
device synchronisation:
  tars_tx_verify        bcosgpu_tars_tx_verify_batch_dev alone on the batch, device-resident: the yardstick (that
                        entry point is what admission runs first, unchanged)
  admit_full_dev        bcosgpu_txpool_admit_dev, mode FULL, the same device buffers
  admit_proposal_dev    ... mode PROPOSAL
  host_create           bcosgpu_tars_tx_verify_batch from host memory: the yardstick of the two below
  admit_full_host       bcosgpu_txpool_admit from host memory, mode FULL
  admit_proposal_host   ... mode PROPOSAL
  block_committed       1,000 of the pool's transactions leave with their block; a remembered block of 1,000
                        nonces expires from the 1,000,000-key ledger set
The three calls of a group alternate within every round.  After every timed admission the batch's hashes and
nonces are removed again (untimed), so every run meets the same sets.  Before a time is kept: the admission's
statuses are 0 exactly where the stateless call's are, 10008 elsewhere, and the sets' counts are what they must be.
Needs a gfx950 GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
ROOT = os.path.dirname(PKG)
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def clock(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def summary(ts):
    return {"ms": float(statistics.median(ts)), "min_ms": min(ts), "max_ms": max(ts), "runs": len(ts)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=10000, help="transactions per admitted batch")
    ap.add_argument("--pool", type=int, default=15000, help="transactions in the pool beforehand")
    ap.add_argument("--blocks", type=int, default=1000, help="remembered blocks of the ledger set")
    ap.add_argument("--block-nonces", type=int, default=1000, help="nonces per remembered block")
    ap.add_argument("--commit", type=int, default=1000, help="transactions per committed block")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "txpool_admit.json"))
    args = ap.parse_args()

    import torch
    import bcos_gpu
    from bcos_gpu import device, synth, tars, txpool
    bcos_gpu.ensure_device(0)
    suite = device.SUITE_SECP256K1
    n = args.n

    def encodings(count, seed):
        b = synth.make_batch(suite, count, seed=seed)
        enc, off = synth.tars_encodings(b)
        torch.cuda.synchronize()
        return enc, off

    enc, off = encodings(n, 0xF15C0BC5)
    h_enc, h_off = enc.cpu().numpy(), off.cpu().numpy().astype(np.uint64)
    # the synthetic block limit is 500: block number 400 with a range of 1,000 lets it pass
    pool = txpool.Pool(suite, b"chain0", b"group0", args.blocks, 400)
    rng = np.random.default_rng(7)
    ledger = {1 + b: rng.integers(0, 256, size=(args.block_nonces, 32), dtype=np.uint8) for b in range(args.blocks)}
    t_load = clock(lambda: pool.load_ledger_nonces(ledger))
    p_enc, p_off = encodings(args.pool, 0xF15C0BC5 + 10 * n)  # (other nonces: the counter starts elsewhere)
    p_out = pool.admit((p_enc.cpu().numpy(), p_off.cpu().numpy().astype(np.uint64)))
    base = pool.info()
    assert base["error_word"] == 0 and base["ledger"] == args.blocks * args.block_nonces
    assert base["hashes"] == base["nonces"] == int((p_out[3] == 0).sum()) > 0.99 * args.pool

    # ---- device-resident
    work = torch.empty(device.tars_decode_work_size(n), dtype=torch.uint8, device="cuda")
    pre = torch.empty(enc.numel() + 12 * n + 8, dtype=torch.uint8, device="cuda")
    sig = torch.empty(enc.numel() + 8, dtype=torch.uint8, device="cuda")
    pre_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    sig_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    txhash = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    sender = torch.empty((n, 20), dtype=torch.uint8, device="cuda")
    nonce = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    vst = torch.empty(n, dtype=torch.uint8, device="cuda")
    st = torch.empty(n, dtype=torch.int32, device="cuda")

    def verify():
        device.tars_tx_verify(suite, enc, off, pre, pre_off, sig, sig_off, work, txhash, sender, vst)
        torch.cuda.synchronize()

    def undo():
        """(untimed) the batch's keys out again"""
        pool.remove(txhash.cpu().numpy(), nonce.cpu().numpy())
        now = pool.info()
        assert (now["hashes"], now["nonces"], now["error_word"]) == (base["hashes"], base["nonces"], 0)

    verify()
    accepted = (vst.cpu().numpy() == 0)

    def check_status(status, mode):
        status = np.asarray(status).astype(np.int64)
        assert ((status == 0) == accepted).all() and (status[~accepted] == 10008).all(), "statuses differ"
        now = pool.info()
        assert now["hashes"] == base["hashes"] + int(accepted.sum())
        assert now["nonces"] == base["nonces"] + (int(accepted.sum()) if mode == txpool.FULL else 0)

    times = {k: [] for k in ("tars_tx_verify", "admit_full_dev", "admit_proposal_dev", "host_create", "admit_full_host",
                             "admit_proposal_host")}
    for rnd in range(args.warmup + args.reps):
        keep = rnd >= args.warmup
        t = {"tars_tx_verify": clock(verify)}
        for name, mode in (("admit_full_dev", txpool.FULL), ("admit_proposal_dev", txpool.PROPOSAL)):
            t[name] = clock(lambda: device.txpool_admit(pool, enc, off, txhash, sender, nonce, st, mode))
            check_status(st.cpu().numpy(), mode)
            undo()
        if keep:
            for k, v in t.items():
                times[k].append(v)
    # ---- from host memory
    cs = bcos_gpu.secp256k1_suite()
    for rnd in range(args.warmup + args.reps):
        keep = rnd >= args.warmup
        t = {"host_create": clock(lambda: tars.create_transactions(cs, (h_enc, h_off)))}
        for name, mode in (("admit_full_host", txpool.FULL), ("admit_proposal_host", txpool.PROPOSAL)):
            out = []
            t[name] = clock(lambda: out.append(pool.admit((h_enc, h_off), mode)))
            check_status(out[0][3], mode)
            pool.remove(out[0][0], out[0][2])
        if keep:
            for k, v in t.items():
                times[k].append(v)
    # ---- block_committed with expiry: the pool's own transactions leave, block number - range expires
    hashes, nonces = p_out[0][p_out[3] == 0], p_out[2][p_out[3] == 0]
    commits = []
    for k in range(min(args.reps, len(hashes) // args.commit)):
        lo = k * args.commit
        number = args.blocks + 1 + k  # expires block 1 + k
        commits.append(clock(lambda: pool.block_committed(number, hashes[lo:lo + args.commit], nonces[lo:lo + args.commit])))
        now = pool.info()
        assert now["error_word"] == 0 and now["hashes"] == base["hashes"] - (k + 1) * args.commit
        assert now["ledger"] == base["ledger"] and now["blocks"] == args.blocks
    res = {"input": {"batch": n, "suite": "secp256k1", "pool_hashes": base["hashes"], "pool_nonces": base["nonces"],
                     "ledger_nonces": base["ledger"], "remembered_blocks": args.blocks, "commit": args.commit,
                     "accepted_in_batch": int(accepted.sum())},
           "method": "host clock around calls that end in a device synchronisation; %d runs after %d warm-up rounds, "
                     "the calls of a group alternating within every round; the batch's keys removed again (untimed) "
                     "after every admission" % (args.reps, args.warmup),
           "gpu": torch.cuda.get_device_name(0),
           "load_ledger_nonces_ms": t_load,
           "cases": {k: summary(v) for k, v in times.items()}}
    res["cases"]["block_committed"] = summary(commits)
    med = {k: v["ms"] for k, v in res["cases"].items()}
    res["added_over_stateless_ms"] = {"full_dev": med["admit_full_dev"] - med["tars_tx_verify"],
                                      "proposal_dev": med["admit_proposal_dev"] - med["tars_tx_verify"],
                                      "full_host": med["admit_full_host"] - med["host_create"],
                                      "proposal_host": med["admit_proposal_host"] - med["host_create"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res["cases"]))
    print(json.dumps(res["added_over_stateless_ms"]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
