#!/usr/bin/env python3
"""Measures the state-root path on the GPU and writes profiles/state_root.json.

Input: 100,000 seeded storage entries -- table names of 10-60 bytes from 200 distinct names, keys of 20-64
bytes, values 90 % 32 bytes / 9 % 100-1,000 bytes / 1 % 8-24 KiB, 5 % of the entries DELETED -- at block
version 3.1, for both hashers, with XOR_NAMES on every entry and on none.  For each of the four it reports

  (a) the fused path (bcosgpu_state_root_dev, device-resident input), event-timed per launch, median; also
      with one lane per entry (a child process with BCOSGPU_STATE_MAP=entry), without the long list (=flat),
      and with the same entries sorted by value length (what a full bucketing by compression-block count
      would buy on top);
  (b) the composition available without it: bcosgpu_hash_batch_dev over the same messages, a copy of every
      digest to the host and a numpy XOR -- the hashing alone, and end to end;
  (c) the host call bcosgpu_state_root end to end, with the packer, the copy of the packed bytes and the
      kernel timed on their own;
  (d) the oracle's CPU hashing of the same messages on the stated number of threads.

Every root is checked against (b)'s before a time is kept.  Needs a gfx950 GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

V3_1 = 0x03010000
HASHERS = (("keccak256", 0), ("sm3", 1))
RATE = {0: 136, 1: 64}  # bytes per compression block


def make_entries(n, seed, flags):
    from bcos_gpu.state import ENTRY_DELETED, ENTRY_MODIFIED, StateEntry
    rng = np.random.default_rng(seed)
    names = []
    for j, ln in enumerate(rng.integers(10, 61, size=200)):
        names.append((b"/t%03d/" % j + rng.bytes(30).hex().encode())[:int(ln)])
    ti = rng.integers(0, len(names), size=n)
    klen = rng.integers(20, 65, size=n)
    u = rng.random(n)
    vlen = np.where(u < 0.9, 32, np.where(u < 0.99, rng.integers(100, 1001, size=n), rng.integers(8192, 24577, size=n)))
    deleted = rng.random(n) < 0.05
    blob = rng.bytes(int(klen.sum() + vlen.sum()))
    out, at = [], 0
    for i in range(n):
        k, v = int(klen[i]), int(vlen[i])
        out.append(StateEntry(names[int(ti[i])], blob[at:at + k], blob[at + k:at + k + v],
                              ENTRY_DELETED if deleted[i] else ENTRY_MODIFIED, flags))
        at += k + v
    return out


def messages(entries):
    """What the composition hashes at 3.1: per entry table||key||value (table||key when DELETED), and with
    XOR_NAMES the table and the key (Entry.h:233-278, StateStorage.h:414-415)."""
    from bcos_gpu.state import ENTRY_MODIFIED, STATE_XOR_NAMES
    msgs, kinds = [], []
    for e in entries:
        msgs.append(e.table + e.key + (e.value if e.status == ENTRY_MODIFIED else b""))
        kinds.append(0)
        if e.flags & STATE_XOR_NAMES:
            msgs += [e.table, e.key]
            kinds += [1, 2]
    return msgs, np.array(kinds)


def blocks(hasher, lens):
    lens = np.asarray(lens, dtype=np.int64)
    return lens // 136 + 1 if hasher == 0 else (lens + 8) // 64 + 1


def med(xs):
    return float(statistics.median(xs))


def event_ms(fn, reps, warm):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return out


def host_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


class Fused:
    """The packed entries resident on the device and one launch of bcosgpu_state_root_dev over them."""

    def __init__(self, entries):
        import torch
        from bcos_gpu import device, state
        self.data, self.off3, self.kind = state.pack_state_entries(entries)
        n = len(entries)
        self.d_data = torch.from_numpy(np.concatenate([self.data, np.zeros(8, np.uint8)])).cuda()
        self.d_off = torch.from_numpy(self.off3.astype(np.int64)).cuda()
        self.d_kind = torch.from_numpy(self.kind.copy()).cuda()
        self.work = torch.empty(device.state_root_work_size(n), dtype=torch.uint8, device="cuda")
        self.root = torch.zeros(32, dtype=torch.uint8, device="cuda")

    def launch(self, hasher):
        from bcos_gpu import device
        device.state_root(hasher, V3_1, self.d_data, self.d_off, self.d_kind, self.work, self.root)

    def timed(self, hasher, reps, warm):
        ts = event_ms(lambda: self.launch(hasher), reps, warm)
        return ts, self.root.cpu().numpy().tobytes()


def fused_only(args):
    """The child of the other mapping: (a) for the four inputs, as one JSON line."""
    import bcos_gpu
    bcos_gpu.ensure_device(0)
    out = {}
    for flags in (1, 0):
        f = Fused(make_entries(args.n, args.seed, flags))
        for name, hasher in HASHERS:
            ts, root = f.timed(hasher, args.reps, args.warmup)
            out["%s/names_%s" % (name, "all" if flags else "none")] = {"ms": med(ts), "root": root.hex()}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--reps", type=int, default=60, help="timed launches of the fused kernel (>= 50)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=15, help="timed repeats of the host-clocked legs")
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1), help="oracle CPU threads")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_root.json"))
    ap.add_argument("--fused-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.fused_only:
        return fused_only(args)

    # the other mappings first, each in a process of its own (the mapping is read once per process)
    other = {}
    for mapping in ("entry", "flat"):
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--fused-only", "--n", str(args.n), "--seed",
                                str(args.seed), "--reps", str(args.reps), "--warmup", str(args.warmup)],
                               env=dict(os.environ, BCOSGPU_STATE_MAP=mapping), capture_output=True, text=True,
                               check=True)
        other[mapping] = json.loads(child.stdout.strip().splitlines()[-1])

    import torch
    import bcos_gpu
    from bcos_gpu import _lib, device, state
    from bcos_gpu.crypto import pack_messages
    from oracle import oracle
    assert os.environ.get("BCOSGPU_STATE_MAP") not in ("entry", "flat")
    oracle.build()
    bcos_gpu.ensure_device(0)
    L = _lib.lib()
    res = {"input": {"entries": args.n, "seed": args.seed, "block_version": "0x%08x" % V3_1,
                     "tables": "10-60 B, 200 distinct", "keys": "20-64 B",
                     "values": "90% 32 B, 9% 100-1000 B, 1% 8-24 KiB", "deleted": "5%"},
           "method": {"a": "torch.cuda.Event around each launch (fused kernel + fold), median of %d after %d warm-up"
                           % (args.reps, args.warmup),
                      "b,c,d": "host clock around work that ends in a synchronise, median of %d" % args.host_reps,
                      "device": torch.cuda.get_device_name(0), "oracle_threads": args.threads},
           "cases": {}}
    for flags in (1, 0):
        entries = make_entries(args.n, args.seed, flags)
        fused = Fused(entries)
        order = np.argsort([len(e.value) for e in entries], kind="stable")
        bucketed = Fused([entries[int(i)] for i in order])
        msgs, kinds = messages(entries)
        b_data, b_off = pack_messages(msgs)
        lens = np.diff(b_off.astype(np.int64))
        d_bdata = torch.from_numpy(np.concatenate([b_data, np.zeros(8, np.uint8)])).cuda()
        d_boff = torch.from_numpy(b_off.astype(np.int64)).cuda()
        d_dig = torch.empty((len(msgs), 32), dtype=torch.uint8, device="cuda")
        h_dig = torch.empty((len(msgs), 32), dtype=torch.uint8).pin_memory()
        views, keep = state.state_entry_views(entries)
        size = int(L.bcosgpu_state_entries_size(views, args.n))
        p_out = np.zeros(size + 8, dtype=np.uint8)
        p_off = np.zeros(3 * args.n + 1, dtype=np.uint64)
        p_kind = np.zeros(args.n, dtype=np.uint8)
        staged = 8 * (3 * args.n + 1) + size + args.n  # what the host call copies to the device
        h_stage = torch.empty(staged, dtype=torch.uint8).pin_memory()
        d_stage = torch.empty(staged, dtype=torch.uint8, device="cuda")
        root_out = np.zeros(32, dtype=np.uint8)
        for name, hasher in HASHERS:
            c = {}
            # (b) the composition: hash every message, copy every digest, XOR on the host
            hash_ts = event_ms(lambda: device.hash_batch(hasher, d_bdata, d_boff, d_dig), args.host_reps, 3)
            state_b = {}

            def composed():
                device.hash_batch(hasher, d_bdata, d_boff, d_dig)
                h_dig.copy_(d_dig, non_blocking=True)
                torch.cuda.synchronize()
                x = np.bitwise_xor.reduce(h_dig.numpy().view(np.uint64).reshape(-1, 4), axis=0)
                state_b["root"] = x.tobytes()

            total_ts = host_ms(composed, args.host_reps, 3)
            d2h_ts = event_ms(lambda: h_dig.copy_(d_dig, non_blocking=True), args.host_reps, 2)
            xor_ts = host_ms(lambda: np.bitwise_xor.reduce(h_dig.numpy().view(np.uint64).reshape(-1, 4), axis=0),
                             args.host_reps, 2)
            want = state_b["root"]
            c["b_composed"] = {"messages": len(msgs), "message_bytes": int(lens.sum()), "digest_bytes": 32 * len(msgs),
                               "hash_ms": med(hash_ts), "d2h_ms": med(d2h_ts), "xor_ms": med(xor_ts),
                               "end_to_end_ms": med(total_ts)}
            # (a) the fused kernel, three ways
            ts, root = fused.timed(hasher, args.reps, args.warmup)
            assert root == want, "fused root differs from the composition's"
            tsb, rootb = bucketed.timed(hasher, args.reps, args.warmup)
            assert rootb == want, "root changed under a permutation"
            case = "%s/names_%s" % (name, "all" if flags else "none")
            pe, flat = other["entry"][case], other["flat"][case]
            assert bytes.fromhex(pe["root"]) == want, "one-lane-per-entry root differs"
            assert bytes.fromhex(flat["root"]) == want, "root without the long list differs"
            c["a_fused"] = {"ms": med(ts), "min_ms": min(ts), "max_ms": max(ts), "launches": len(ts),
                            "lane_per_entry_ms": pe["ms"], "no_long_list_ms": flat["ms"],
                            "sorted_by_value_length_ms": med(tsb)}
            # (c) the host call, and its parts on their own
            call_ts = host_ms(lambda: _lib.check(L.bcosgpu_state_root(hasher, V3_1, views, args.n,
                                                                      root_out.ctypes.data)), args.host_reps, 3)
            assert root_out.tobytes() == want, "host-call root differs"
            pack_ts = host_ms(lambda: _lib.check(L.bcosgpu_pack_state_entries(
                views, args.n, p_out.ctypes.data, size, p_off.ctypes.data, p_kind.ctypes.data)), args.host_reps, 2)
            h2d_ts = event_ms(lambda: d_stage.copy_(h_stage, non_blocking=True), args.host_reps, 2)
            c["c_host_call"] = {"end_to_end_ms": med(call_ts), "pack_ms": med(pack_ts), "h2d_ms": med(h2d_ts),
                                "h2d_bytes": staged, "kernel_ms": med(ts),
                                "other_ms": med(call_ts) - med(pack_ts) - med(h2d_ts) - med(ts)}
            # (d) the oracle on the CPU
            cpu_ts = host_ms(lambda: oracle.hash_packed(hasher, b_data, b_off, nthreads=args.threads), 3, 1)
            c["d_oracle_cpu"] = {"threads": args.threads, "hash_ms": med(cpu_ts)}
            # the work by kind, in compression blocks (from the lengths): what a table-name de-duplication could save
            blk = blocks(hasher, lens)
            c["blocks"] = {"entry": int(blk[kinds == 0].sum()), "table": int(blk[kinds == 1].sum()),
                           "key": int(blk[kinds == 2].sum()),
                           "entry_max": int(blk[kinds == 0].max()), "rate_bytes": RATE[hasher]}
            a = med(ts)
            c["ratios"] = {"b_hash_over_a": med(hash_ts) / a, "b_end_to_end_over_a": med(total_ts) / a,
                           "b_end_to_end_over_c_end_to_end": med(total_ts) / med(call_ts),
                           "d_over_a": med(cpu_ts) / a, "d_over_c_end_to_end": med(cpu_ts) / med(call_ts),
                           "lane_per_entry_over_a": pe["ms"] / a, "no_long_list_over_a": flat["ms"] / a,
                           "a_over_sorted": a / med(tsb),
                           "c_pack_share": med(pack_ts) / med(call_ts), "c_h2d_share": med(h2d_ts) / med(call_ts),
                           "c_kernel_share": a / med(call_ts)}
            res["cases"][case] = c
            print(name, "names_all" if flags else "names_none", json.dumps(c["ratios"]), flush=True)
        del keep
    for name, _ in HASHERS:  # what the names cost inside the fused kernel
        on, off = res["cases"][name + "/names_all"], res["cases"][name + "/names_none"]
        res["cases"][name + "/names_all"]["ratios"]["a_names_all_over_names_none"] = on["a_fused"]["ms"] / off["a_fused"]["ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
