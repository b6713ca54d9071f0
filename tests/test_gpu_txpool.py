"""Transaction admission with the pool's state on the GPU (bcos_gpu.txpool.Pool over bcosgpu_txpool_*; csrc/
txpool_kernels.hip) against the literal restatement of the reference's order on Python sets
(tests/txpool_restatement.py::Pool).  Every expected value -- statuses, hashes, senders, nonces and the contents
of the three sets -- comes from that restatement, never from the library; the device only signs the inputs.

The pool of every test: chain0 / group0, block_limit_range 10, block number 100, so block limits 101..110 pass.
"""
import copy
import random

import numpy as np
import pytest

import txpool_restatement as R
from bcos_gpu.tars import encode_transaction
from bcos_gpu.tx import Transaction, TransactionData

pytestmark = pytest.mark.gpu

CHAIN, GROUP, RANGE, NUMBER = b"chain0", b"group0", 10, 100
SUITES = [pytest.param(0, id="secp256k1"), pytest.param(1, id="sm2")]
MODES = [pytest.param(R.FULL, id="full"), pytest.param(R.PROPOSAL, id="proposal")]


def spec(nonce, to="a", group="group0", chain="chain0", limit=105, bad_sig=False, malformed=False):
    return dict(nonce=str(nonce), to=to, group=group, chain=chain, limit=limit, bad_sig=bad_sig, malformed=malformed)


def build(gpu, oracle, suite, specs, seed):
    """The encoded transactions of `specs`, signed on the device (one key per transaction); a bad signature is
    v = 4 (secp256k1) or a flipped bit (SM2), a malformed one loses its last byte."""
    from test_gpu_ecc import _dev_sign
    datas = [TransactionData(version=0, chain_id=s["chain"], group_id=s["group"], block_limit=s["limit"],
                             nonce=s["nonce"], to=s["to"], input=b"\x01\x02", abi="") for s in specs]
    H = oracle.sm3 if suite else oracle.keccak256
    hashes = np.array([np.frombuffer(H(d.preimage()), dtype=np.uint8) for d in datas])
    sk = np.random.default_rng(seed).integers(0, 256, size=(len(specs), 32), dtype=np.uint8)
    sk[:, 0] &= 0x7F
    sk[:, 31] |= 1
    _, sig, ok = _dev_sign(gpu, suite, sk, hashes)
    assert ok.all()
    out = []
    for d, s, g in zip(datas, specs, sig):
        g = g.copy()
        if s["bad_sig"]:
            if suite == 0:
                g[64] = 4
            else:
                g[5] ^= 1
        e = encode_transaction(Transaction(d, signature=g.tobytes()))
        out.append(e[:-1] if s["malformed"] else e)
    return out


class Pair:
    """The library's pool and the restatement's, driven together."""

    def __init__(self, suite, capacity=0, mirror=None):
        from bcos_gpu import txpool
        self.gpu = txpool.Pool(suite, CHAIN, GROUP, RANGE, NUMBER, initial_capacity=capacity)
        self.ref = mirror if mirror is not None else R.Pool(suite, CHAIN, GROUP, RANGE, NUMBER)

    def admit(self, encoded, mode=R.FULL):
        got = self.gpu.admit(encoded, mode)
        want = self.ref.admit(encoded, mode)
        for g, w, name in zip(got, want, ("txhash", "sender", "nonce", "status")):
            assert g.dtype == w.dtype and np.array_equal(g, w), (name, np.nonzero((g != w).reshape(len(w), -1).any(1)))
        self.same()
        return want[3]

    def block_committed(self, number, hashes, nonces):
        self.gpu.block_committed(number, hashes, nonces)
        self.ref.block_committed(number, hashes, nonces)
        self.same()

    def remove(self, hashes, nonces):
        self.gpu.remove(hashes, nonces)
        self.ref.remove(hashes, nonces)
        self.same()

    def load_ledger_nonces(self, blocks):
        self.gpu.load_ledger_nonces(blocks)
        self.ref.load_ledger_nonces(blocks)
        self.same()

    def same(self):
        """The three dumps equal the Python sets in ascending order; counts, block number, remembered blocks; and
        the error word is 0."""
        from bcos_gpu import txpool
        info = self.gpu.info()
        assert info["error_word"] == 0
        assert (info["block_number"], info["blocks"]) == (self.ref.number, len(self.ref.blocks))
        for which, name, keys in ((txpool.HASHES, "hashes", sorted(self.ref.hashes)),
                                  (txpool.NONCES, "nonces", [v.to_bytes(32, "big") for v in sorted(self.ref.nonces)]),
                                  (txpool.LEDGER, "ledger", [v.to_bytes(32, "big") for v in sorted(self.ref.ledger)])):
            assert info[name] == len(keys) <= info[name + "_capacity"], name
            assert self.gpu.dump(which).tobytes() == b"".join(keys), name


# ---------------------------------------------------------------- the shared corpus (built and judged once per suite)
BIG = 4096


@pytest.fixture(scope="module", params=[0, 1], ids=["secp256k1", "sm2"])
def corpus(request, gpu, oracle):
    """Per suite: 4,096 valid transactions with the restatement's pool after admitting them (plus 4,096 ledger
    nonces), and a pool of 700 mixed transactions the batches are drawn from."""
    suite = request.param
    big = build(gpu, oracle, suite, [spec(10 ** 6 + i) for i in range(BIG)], seed=11 + suite)
    ref = R.Pool(suite, CHAIN, GROUP, RANGE, NUMBER)
    ledger = {90 + b: [2 * 10 ** 6 + 512 * b + i for i in range(512)] for b in range(8)}
    ref.load_ledger_nonces(ledger)
    big_out = ref.admit(big, R.FULL)
    assert (big_out[3] == 0).all()
    rng = random.Random(5 + suite)
    specs = []
    for i in range(700):
        r = rng.random()
        nonce = rng.choice([rng.randrange(40), 10 ** 6 + rng.randrange(BIG), 2 * 10 ** 6 + rng.randrange(BIG),
                            10 ** 6, 2 * 10 ** 6, "07", "", 2 ** 256 - 1, 5 * 10 ** 6 + i])
        specs.append(spec(nonce, to=rng.choice("ab"),
                          group="other" if 0.05 < r < 0.08 else "group0", chain="other" if 0.08 < r < 0.11 else "chain0",
                          limit=rng.choice([100, 101, 105, 110, 111] if rng.random() < 0.2 else [105]),
                          bad_sig=rng.random() < 0.12, malformed=r < 0.03))
    mixed = build(gpu, oracle, suite, specs, seed=23 + suite)
    mixed += [big[0], big[1], big[BIG - 1]]  # whole transactions the big pool already holds
    return dict(suite=suite, big=big, big_ref=ref, big_out=big_out, ledger=ledger, mixed=mixed)


def pair_with(corpus, size):
    """A pair whose sets hold 0, 1 or 4,096 keys each."""
    suite = corpus["suite"]
    if size == 0:
        return Pair(suite)
    if size == 1:
        p = Pair(suite)
        p.load_ledger_nonces({95: [2 * 10 ** 6]})
        st = p.admit(corpus["big"][:1])
        assert list(st) == [0]
        return p
    p = Pair(suite, mirror=copy.deepcopy(corpus["big_ref"]))
    p.gpu.load_ledger_nonces(corpus["ledger"])
    got = p.gpu.admit(corpus["big"])
    assert all(np.array_equal(g, w) for g, w in zip(got, corpus["big_out"]))
    p.same()
    return p


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", [0, 1, BIG])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257])
def test_boundaries(corpus, n, size, mode):
    """A batch of n transactions against empty sets, sets of one key and sets of 4,096 keys, then a second one
    against what the first left."""
    p = pair_with(corpus, size)
    rng = random.Random(1000 * size + 10 * n + mode)
    for _ in range(2):
        p.admit([rng.choice(corpus["mixed"]) for _ in range(n)], mode)


def test_the_mix_is_a_mix(corpus):
    """(of the batches above: the restatement gives the corpus every status but 10004 from an empty pool, and
    10004 too once it is admitted twice)"""
    ref = R.Pool(corpus["suite"], CHAIN, GROUP, RANGE, NUMBER)
    ref.load_ledger_nonces(corpus["ledger"])
    seen = set(int(s) for s in ref.admit(corpus["mixed"])[3]) | set(int(s) for s in ref.admit(corpus["mixed"])[3])
    assert seen == {0, 2, 4, 10000, 10001, 10004, 10006, 10007, 10008}


@pytest.mark.parametrize("suite", SUITES)
def test_every_status_once(gpu, oracle, suite):
    """One 64-transaction FULL batch with each of 2, 4, 10000 (pool), 10000 (ledger), 10001 (both sides), 10004,
    10006, 10007, 10008 and 0, and the precedence pairs of DESIGN.md 6e."""
    pre = build(gpu, oracle, suite, [spec(500), spec(501, group="other")], seed=31)
    s = [
        spec(1, malformed=True),                              # 0: 2
        spec("07"),                                           # 1: 4
        spec(500, to="b"),                                    # 2: 10000, the pool's nonce under another hash
        spec(600),                                            # 3: 10000, the ledger's nonce
        spec(2, limit=100), spec(3, limit=111),               # 4, 5: 10001 on both sides of the window
        spec(4, limit=101), spec(5, limit=110),               # 6, 7: 0 at both edges
        spec(6, chain="other"), spec(7, group="other"),       # 8, 9: 10006, 10007
        spec(8, bad_sig=True),                                # 10: 10008
        # precedence: group before chain, chain before the nonce's form, the form before the signature, the
        # pool's nonce before the block limit, the block limit before the signature
        spec(9, group="other", chain="other"), spec("+1", chain="other"), spec("00", bad_sig=True),
        spec(500, to="c", limit=111), spec(10, limit=100, bad_sig=True),
        # inside the batch: a bad signature ahead of a good one (W is not the first of its run), then the same
        # nonce under another hash (10000)
        spec(20, to="x", bad_sig=True), spec(20, to="y"), spec(20, to="z"),
        spec(21), spec(22, limit=111), spec(22),              # 10001 does not claim nonce 22
    ]
    s += [spec(100 + i) for i in range(64 - len(s) - 3)]
    batch = build(gpu, oracle, suite, s, seed=37)
    batch += [pre[0], pre[1], batch[19]]  # a known hash; a wrong group together with a known hash; 21 again
    assert len(batch) == 64
    p = Pair(suite)
    p.load_ledger_nonces({99: [600]})
    assert list(p.admit(pre[:1])) == [0]
    assert list(p.admit(pre[1:], R.PROPOSAL)) == [0]  # (no group check there: the hash is now known)
    st = list(p.admit(batch))
    assert st[:22] == [2, 4, 10000, 10000, 10001, 10001, 0, 0, 10006, 10007, 10008, 10007, 10006, 4, 10000, 10001,
                       10008, 0, 10000, 0, 10001, 0]
    assert st[61:] == [10004, 10004, 10004] and all(x == 0 for x in st[22:61])


@pytest.mark.parametrize("suite", SUITES)
def test_dense_repeats(gpu, oracle, suite):
    """256 transactions over 5 nonce values, whole transactions repeated, bad signatures ahead of good ones."""
    base = build(gpu, oracle, suite, [spec(n, to=t, bad_sig=b) for n in range(5) for t, b in
                                      (("a", True), ("b", False), ("c", False))], seed=41)
    rng = random.Random(43)
    batch = base[0:1] + base[3:4] + [rng.choice(base) for _ in range(254)]  # two runs open with a bad signature
    p = Pair(suite)
    st = p.admit(batch)
    assert (st == 0).sum() == 5 and set(int(x) for x in st) == {0, 10000, 10004, 10008}
    st = p.admit(batch)  # and again: everything is known now
    assert set(int(x) for x in st) <= {10000, 10004}


@pytest.mark.parametrize("suite", SUITES)
def test_growth(gpu, oracle, suite):
    """Initial capacity 8; every set crosses two growth steps, the dumps equal after every step."""
    txs = build(gpu, oracle, suite, [spec(i) for i in range(40)], seed=47)
    p = Pair(suite, capacity=8)
    caps = []
    for k, (lo, hi) in enumerate(((0, 5), (5, 9), (9, 20), (20, 40))):
        p.admit(txs[lo:hi], R.FULL if lo != 5 else R.PROPOSAL)
        p.block_committed(101 + k, [], [3000 + i for i in range(lo, hi)])
        caps.append(p.gpu.info())
    for name in ("hashes", "nonces", "ledger"):
        steps = sorted(set(c[name + "_capacity"] for c in caps + [p.gpu.info()]))
        assert steps[0] == 8 and len(steps) >= 3, (name, steps)
        assert all(b >= 2 * a for a, b in zip(steps, steps[1:]))


@pytest.mark.parametrize("suite", SUITES)
def test_life_cycle(gpu, oracle, suite):
    """40 random operations mirrored on the restatement, the statuses and the three dumps compared after each."""
    rng = random.Random(53 + suite)
    specs = [spec(rng.randrange(60), to=rng.choice("ab"), bad_sig=rng.random() < 0.1,
                  limit=rng.choice([105, 108, 112, 120])) for _ in range(300)]
    txs = build(gpu, oracle, suite, specs, seed=59)
    p = Pair(suite, capacity=8)
    number = NUMBER
    ops = ["admit"] * 14 + ["proposal"] * 5 + ["commit"] * 12 + ["remove"] * 5 + ["load"] * 2 + ["same130", "absent"]
    rng.shuffle(ops)
    assert len(ops) == 40
    expiries = 0
    for op in ops:
        expiries += op in ("commit", "same130", "absent") and number + 1 - RANGE in p.ref.blocks
        if op in ("admit", "proposal"):
            p.admit([rng.choice(txs) for _ in range(rng.randrange(1, 30))], R.FULL if op == "admit" else R.PROPOSAL)
        elif op == "commit":  # a block of some of the pool's transactions; expiry crosses `range` as number grows
            number += 1
            hashes = rng.sample(sorted(p.ref.hashes), min(len(p.ref.hashes), rng.randrange(0, 8)))
            nonces = rng.sample(sorted(p.ref.nonces), min(len(p.ref.nonces), rng.randrange(0, 8)))
            p.block_committed(number, hashes + hashes[:2], nonces + nonces[:1] + [rng.randrange(60)])
        elif op == "remove":
            hashes = rng.sample(sorted(p.ref.hashes), min(len(p.ref.hashes), 3)) + [bytes([7]) * 32]
            p.remove(hashes, [rng.randrange(60) for _ in range(4)])
        elif op == "load":
            p.load_ledger_nonces({number - 1: [rng.randrange(60) for _ in range(5)], number - 2: [], number: [61, 61]})
        elif op == "same130":  # one value 130 times
            number += 1
            p.block_committed(number, [], [17] * 130)
        else:  # hashes the pool does not hold
            number += 1
            p.block_committed(number, [bytes([i]) * 32 for i in range(1, 40)], [])
    assert expiries >= 3  # blocks did expire


@pytest.mark.parametrize("suite", SUITES)
def test_empty_calls_change_nothing(gpu, oracle, suite):
    p = Pair(suite, capacity=8)
    p.load_ledger_nonces({99: [1, 2, 3]})
    p.admit(build(gpu, oracle, suite, [spec(5), spec(6)], seed=61))
    before = p.gpu.info()
    for mode in (R.FULL, R.PROPOSAL):
        out = p.admit([], mode)
        assert len(out) == 0
    p.remove([], [])
    p.load_ledger_nonces({})
    assert p.gpu.info() == before
    p.block_committed(NUMBER, [], [])  # (remembers an empty list for block 100, as the reference does)
    assert p.gpu.info() == dict(before, blocks=2)


def _sets_bytes(ref):
    import struct
    out = b""
    for keys in (sorted(ref.hashes), [v.to_bytes(32, "big") for v in sorted(ref.nonces)],
                 [v.to_bytes(32, "big") for v in sorted(ref.ledger)]):
        out += struct.pack("<I", len(keys)) + b"".join(keys)
    return out


def _keys_bytes(keys):
    import struct
    return struct.pack("<I", len(keys)) + b"".join(k if isinstance(k, bytes) else k.to_bytes(32, "big") for k in keys)


@pytest.mark.parametrize("suite", SUITES)
def test_cpp_wrapper_on_gpu(tmp_path, gpu, oracle, suite):
    """bcosgpu::GpuTxPool of include/bcos_gpu.hpp through the C ABI (tests/cpp/txpool_test.cpp): admit, blockCommitted,
    remove, loadLedgerNonces, info and dump against a fixture the restatement computed."""
    import os
    import struct
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "fisco-bcos_amd", "lib")
    exe = str(tmp_path / "txpool_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                    os.path.join(root, "tests", "cpp", "txpool_test.cpp"), "-L" + libdir, "-lbcosgpu",
                    "-Wl,-rpath," + libdir], check=True)
    specs = [spec(i % 9, to="ab"[i % 2], bad_sig=i % 7 == 3, malformed=i == 5, group="other" if i == 11 else "group0")
             for i in range(30)]
    enc = build(gpu, oracle, suite, specs, seed=67)
    enc += [enc[0], enc[2]]
    ref = R.Pool(suite, CHAIN, GROUP, RANGE, NUMBER)
    txhash, sender, nonce, status = ref.admit(enc)
    fx = struct.pack("<II", suite, len(enc)) + b"".join(struct.pack("<I", len(e)) + e for e in enc)
    for i in range(len(enc)):
        fx += txhash[i].tobytes() + sender[i].tobytes() + nonce[i].tobytes() + struct.pack("<I", int(status[i]))
    fx += _sets_bytes(ref)
    hashes = sorted(ref.hashes)
    h1, n1 = hashes[:3] + hashes[:1] + [bytes(32)], [0, 1, 1, 77]
    ref.block_committed(103, h1, n1)
    fx += struct.pack("<q", 103) + _keys_bytes(h1) + _keys_bytes(n1) + _sets_bytes(ref)
    h2, n2 = hashes[2:5], [2, 3, 99]
    ref.remove(h2, n2)
    fx += _keys_bytes(h2) + _keys_bytes(n2) + _sets_bytes(ref)
    path = str(tmp_path / "txpool.bin")
    with open(path, "wb") as f:
        f.write(fx)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "txpool_test: ok" in r.stdout


@pytest.mark.parametrize("mode", MODES)
def test_device_resident_admission(corpus, mode):
    """bcosgpu_txpool_admit_dev over torch tensors (bcos_gpu.device.txpool_admit): the same outputs and sets as the
    restatement, on a pool that already holds 4,096 keys per set."""
    import torch
    from bcos_gpu import device
    from bcos_gpu.crypto import pack_messages
    p = pair_with(corpus, BIG)
    rng = random.Random(71 + mode)
    batch = [rng.choice(corpus["mixed"]) for _ in range(300)]
    data, off = pack_messages(batch)
    n = len(batch)
    enc = torch.from_numpy(data.copy()).cuda()
    enc_off = torch.from_numpy(off.astype(np.int64)).cuda()
    txhash = torch.full((n, 32), 0xCC, dtype=torch.uint8, device="cuda")
    sender = torch.full((n, 20), 0xCC, dtype=torch.uint8, device="cuda")
    nonce = torch.full((n, 32), 0xCC, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    device.txpool_admit(p.gpu, enc, enc_off, txhash, sender, nonce, status, mode)
    want = p.ref.admit(batch, mode)
    got = (txhash.cpu().numpy(), sender.cpu().numpy(), nonce.cpu().numpy(), status.cpu().numpy().astype(np.uint32))
    for g, w, name in zip(got, want, ("txhash", "sender", "nonce", "status")):
        assert np.array_equal(g, w), name
    p.same()
