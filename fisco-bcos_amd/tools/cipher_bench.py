#!/usr/bin/env python3
"""Measures the storage cipher on the GPU and writes profiles/storage_cipher.json; with --ab, the A/B of the two
LDS table layouts, written to profiles/cipher_tables_ab.json.

Workloads, 100,000 seeded values each:
  state_mix     the state-root tests' value lengths: 60 % 32 bytes, 5 % empty, the rest 1-299 bytes
  keypage_mix   85 % 32-byte slots, 10 % 100-1,000 bytes, 5 % 10,240-byte KeyPage pages

For each workload, cipher (AES-256-CBC, SM4-CBC) and direction it reports
  device        bcosgpu_cbc_{en,de}crypt_batch_dev over device-resident input, a device event pair around each
                call (every launch of the call), median / min / max
  host_views    bcosgpu_cbc_{en,de}crypt_batch from host views end to end (gather, copy, kernels, copy back),
                host clock, median
  cpu           csrc/cipher_host.h's own CBC over the same values on 1 and 16 threads (lib/cipher_host_check
                bench, best of five)
Before a time is kept: the host call's ciphertext equals the device call's, and decrypting it gives every value back
with status 0.

--ab: the shipped library and lib/libbcosgpu_cipher_ab.so (`make cipher_ab`: the other table layout) alternate in
child processes, --rounds runs each; every run's medians are recorded with their spread.  The replicated layout
ships only if every run of it is below every run of the plain one, per case, in every case.
Needs a gfx950 GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
ROOT = os.path.dirname(PKG)
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

CIPHERS = (("aes256", 0), ("sm4", 1))
KEY = bytes((13 * i + 7) & 0xFF for i in range(32))


def workload(name, n, seed):
    """(blob bytes, int64 off[n+1])."""
    rng = np.random.default_rng(seed)
    u = rng.random(n)
    if name == "state_mix":
        lens = np.where(u < 0.6, 32, np.where(u < 0.65, 0, rng.integers(1, 300, size=n)))
    else:
        lens = np.where(u < 0.85, 32, np.where(u < 0.95, rng.integers(100, 1001, size=n), 10240))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rng.bytes(int(off[-1])), off


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


class Resident:
    """A workload on the device with the buffers of both directions."""

    def __init__(self, blob, off):
        import torch
        from bcos_gpu import device
        self.n = len(off) - 1
        self.off = off
        self.total = int((((off[1:] - off[:-1]) // 16 + 1) * 16).sum())
        self.d_in = torch.from_numpy(np.frombuffer(blob + bytes(16), dtype=np.uint8).copy()).cuda()
        self.d_off = torch.from_numpy(off).cuda()
        self.d_ct = torch.empty(self.total + 16, dtype=torch.uint8, device="cuda")
        self.d_ct_off = torch.empty(self.n + 1, dtype=torch.int64, device="cuda")
        self.work = torch.empty(device.cbc_work_size(self.n), dtype=torch.uint8, device="cuda")
        self.d_pt = torch.empty(self.total + 16, dtype=torch.uint8, device="cuda")
        self.d_len = torch.empty(self.n, dtype=torch.int32, device="cuda")
        self.d_st = torch.empty(self.n, dtype=torch.uint8, device="cuda")

    def encrypt(self, cipher):
        from bcos_gpu import device
        device.cbc_encrypt(cipher, KEY, self.d_in, self.d_off, self.d_ct, self.d_ct_off, self.work)

    def decrypt(self, cipher):
        from bcos_gpu import device
        device.cbc_decrypt(cipher, KEY, self.d_ct, self.d_ct_off, self.d_pt, self.d_len, self.d_st)

    def check_round_trip(self, blob):
        """After encrypt + decrypt: every status 0, every length right, the plaintext bytes equal the input."""
        import torch
        torch.cuda.synchronize()
        lens = self.off[1:] - self.off[:-1]
        assert not self.d_st.cpu().numpy().any(), "a status is not 0"
        assert np.array_equal(self.d_len.cpu().numpy().astype(np.int64), lens), "a plaintext length differs"
        ct_off = self.d_ct_off.cpu().numpy()
        assert int(ct_off[-1]) == self.total
        pt = self.d_pt.cpu().numpy()
        idx = np.repeat(ct_off[:-1] - self.off[:-1], lens) + np.arange(int(self.off[-1]))
        assert pt[idx].tobytes() == blob, "round trip differs from the input"


def device_times(args, names):
    """{workload/cipher/direction: [ms, ...]} for the loaded library."""
    import bcos_gpu
    bcos_gpu.ensure_device(0)
    out = {}
    for wname in names:
        blob, off = workload(wname, args.n, args.seed)
        r = Resident(blob, off)
        for cname, cipher in CIPHERS:
            enc = event_ms(lambda: r.encrypt(cipher), args.reps, args.warmup)
            dec = event_ms(lambda: r.decrypt(cipher), args.reps, args.warmup)
            r.check_round_trip(blob)
            out["%s/%s/encrypt" % (wname, cname)] = enc
            out["%s/%s/decrypt" % (wname, cname)] = dec
        del r
    return out


def summary(ts):
    return {"ms": med(ts), "min_ms": min(ts), "max_ms": max(ts), "launches": len(ts)}


def child(args):
    from bcos_gpu import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    print(json.dumps({k: summary(v) for k, v in device_times(args, args.workloads).items()}))


def ab(args):
    libs = {"shipped": os.path.join(PKG, "lib", "libbcosgpu.so"), "other": os.path.join(PKG, "lib", "libbcosgpu_cipher_ab.so")}
    for p in libs.values():
        assert os.path.exists(p), p + " not built (make -C fisco-bcos_amd all cipher_ab)"
    runs = {"shipped": [], "other": []}
    for rnd in range(args.rounds):
        for which in ("shipped", "other"):
            c = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--lib", libs[which], "--n",
                                str(args.n), "--seed", str(args.seed), "--reps", str(args.reps), "--warmup",
                                str(args.warmup)], capture_output=True, text=True, timeout=600)
            if c.returncode != 0:
                sys.exit("child failed (%s, round %d):\n%s" % (which, rnd, c.stdout + c.stderr))
            runs[which].append(json.loads(c.stdout.strip().splitlines()[-1]))
            print(which, rnd, {k: round(v["ms"], 4) for k, v in runs[which][-1].items()}, flush=True)
    layout = {"shipped": args.shipped_layout, "other": "replicated" if args.shipped_layout == "plain" else "plain"}
    cases = {}
    for case in runs["shipped"][0]:
        per = {layout[w]: [r[case]["ms"] for r in runs[w]] for w in runs}
        cases[case] = {k: {"runs_ms": v, "min_ms": min(v), "max_ms": max(v), "median_ms": med(v)} for k, v in per.items()}
        cases[case]["replicated_below_plain_in_every_run"] = max(per["replicated"]) < min(per["plain"])
    every = all(c["replicated_below_plain_in_every_run"] for c in cases.values())
    import torch
    res = {"method": "alternating child processes on one box, %d runs per build; a run's figure is the median of %d "
                     "event-timed calls after %d warm-up, device-resident input" % (args.rounds, args.reps, args.warmup),
           "input": {"values": args.n, "seed": args.seed}, "device": torch.cuda.get_device_name(0),
           "shipped_layout_of_this_run": args.shipped_layout, "cases": cases,
           "rule": "ship the replicated layout only if every run of it is below every run of the plain one, in every case",
           "replicated_wins_every_case": every, "ship": "replicated" if every else "plain"}
    write(args.ab_out, res)


def write(path, res):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


def cpu_line(cipher_name, direction, threads, path):
    exe = os.path.join(PKG, "lib", "cipher_host_check")
    r = subprocess.run([exe, "bench", cipher_name, direction, str(threads), path], capture_output=True, text=True,
                       check=True)
    return float(r.stdout.strip()) * 1e3


def dump(path, blob, off):
    with open(path, "wb") as f:
        f.write(np.array([len(off) - 1], dtype=np.uint64).tobytes())
        f.write(off.astype(np.uint64).tobytes())
        f.write(blob)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--reps", type=int, default=50, help="event-timed calls per case")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=11)
    ap.add_argument("--workloads", nargs="+", default=["state_mix", "keypage_mix"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "storage_cipher.json"))
    ap.add_argument("--ab", action="store_true", help="the table-layout A/B instead of the measurement")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shipped-layout", choices=("plain", "replicated"), default="plain",
                    help="the layout lib/libbcosgpu.so was built with (cipher_device.h's default)")
    ap.add_argument("--ab-out", default=os.path.join(ROOT, "profiles", "cipher_tables_ab.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.ab:
        return ab(args)

    import torch
    import bcos_gpu
    from bcos_gpu import _lib, cipher as C
    bcos_gpu.ensure_device(0)
    L = _lib.lib()
    res = {"input": {"values": args.n, "seed": args.seed,
                     "state_mix": "60% 32 B, 5% empty, the rest 1-299 B",
                     "keypage_mix": "85% 32 B, 10% 100-1000 B, 5% 10240 B"},
           "method": {"device": "torch.cuda.Event pair around each call (all its launches), median of %d after %d warm-up"
                                % (args.reps, args.warmup),
                      "host_views": "host clock around the call (it ends in a synchronise), median of %d" % args.host_reps,
                      "cpu": "cipher_host.h's CBC over the same values, std::thread, best of five, on this box's CPUs",
                      "gpu": torch.cuda.get_device_name(0)},
           "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for wname in args.workloads:
            blob, off = workload(wname, args.n, args.seed)
            lens = off[1:] - off[:-1]
            values = [blob[int(off[i]):int(off[i + 1])] for i in range(args.n)]
            views, keep = C._views(values)
            r = Resident(blob, off)
            plain_path = os.path.join(tmp, "plain.bin")
            dump(plain_path, blob, off)
            out = np.zeros(r.total, dtype=np.uint8)
            out_off = np.zeros(args.n + 1, dtype=np.uint64)
            back = np.zeros(r.total, dtype=np.uint8)
            back_off = np.zeros(args.n + 1, dtype=np.uint64)
            status = np.zeros(args.n, dtype=np.uint8)
            for cname, cipher in CIPHERS:
                enc = event_ms(lambda: r.encrypt(cipher), args.reps, args.warmup)
                dec = event_ms(lambda: r.decrypt(cipher), args.reps, args.warmup)
                r.check_round_trip(blob)
                ct = r.d_ct.cpu().numpy()[:r.total]
                ct_off = r.d_ct_off.cpu().numpy()
                h_enc = host_ms(lambda: _lib.check(L.bcosgpu_cbc_encrypt_batch(
                    cipher, KEY, 32, None, 0, views, args.n, out.ctypes.data, r.total, out_off.ctypes.data)),
                    args.host_reps, 2)
                assert np.array_equal(out, ct) and np.array_equal(out_off.astype(np.int64), ct_off), "host != device"
                ct_bytes = ct.tobytes()
                cts = [ct_bytes[int(ct_off[i]):int(ct_off[i + 1])] for i in range(args.n)]
                cviews, ckeep = C._views(cts)
                h_dec = host_ms(lambda: _lib.check(L.bcosgpu_cbc_decrypt_batch(
                    cipher, KEY, 32, None, 0, cviews, args.n, back.ctypes.data, r.total, back_off.ctypes.data,
                    status.ctypes.data)), args.host_reps, 2)
                assert not status.any() and back[:len(blob)].tobytes() == blob, "host decrypt differs"
                assert np.array_equal(back_off.astype(np.int64), off)
                ct_path = os.path.join(tmp, "ct.bin")
                dump(ct_path, ct_bytes, ct_off)
                cpu = {"encrypt": {t: cpu_line(cname, "enc", t, plain_path) for t in (1, 16)},
                       "decrypt": {t: cpu_line(cname, "dec", t, ct_path) for t in (1, 16)}}
                for direction, dev, host, nbytes in (("encrypt", enc, h_enc, int(off[-1])), ("decrypt", dec, h_dec, r.total)):
                    c = {"device": summary(dev), "host_views_ms": med(host),
                         "cpu_1_thread_ms": cpu[direction][1], "cpu_16_threads_ms": cpu[direction][16],
                         "input_bytes": nbytes, "blocks": r.total // 16,
                         "device_gb_per_s": nbytes / med(dev) / 1e6,
                         "ratios": {"cpu_1_over_device": cpu[direction][1] / med(dev),
                                    "cpu_16_over_device": cpu[direction][16] / med(dev),
                                    "cpu_16_over_host_views": cpu[direction][16] / med(host)}}
                    res["cases"]["%s/%s/%s" % (wname, cname, direction)] = c
                    print(wname, cname, direction, json.dumps({k: v for k, v in c.items() if k != "ratios"}), flush=True)
                del ckeep
            res["input"][wname + "_bytes"] = int(off[-1])
            res["input"][wname + "_longest"] = int(lens.max())
            del keep, r
    write(args.out, res)


if __name__ == "__main__":
    main()
