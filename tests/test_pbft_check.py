"""The PBFT message check (every signature of a drained message queue in one call) through every layer: the
device path (bcosgpu_pbft_check_dev: pbft_hash_kernel, the known-key verify kernels, pbft_verdict_kernel,
pbft_group_kernel), the host call (bcosgpu_pbft_check), the Python mirror (bcos_gpu/pbft.py) and the C++ adapter
(tests/cpp/pbft_check_test.cpp over include/bcos_gpu.hpp), against a Python restatement of the reference's rules
over oracle.hash_ (KAT-pinned Keccak-256 / SM3), oracle.secp256k1_verify and oracle.sm2_recover on r || s || pub
(a verify against a known key):

  checkSignature                            bcos-pbft/bcos-pbft/pbft/engine/PBFTEngine.cpp:732-750
  checkProposalSignature                    bcos-pbft/bcos-pbft/pbft/engine/PBFTEngine.cpp:752-771
  getHashFieldsDataHash                     bcos-pbft/bcos-pbft/pbft/protocol/PB/PBFTMessage.cpp:92-98
  getConsensusNodeByIndex                   bcos-pbft/bcos-pbft/core/ConsensusConfig.cpp:150-158
  PBFTCacheProcessor::checkPrecommitWeight  bcos-pbft/bcos-pbft/pbft/cache/PBFTCacheProcessor.cpp:795-821
  isValidViewChangeMsg (prepared proposals) bcos-pbft/bcos-pbft/pbft/engine/PBFTEngine.cpp:1161-1191
  isValidNewViewMsg                         bcos-pbft/bcos-pbft/pbft/engine/PBFTEngine.cpp:1230-1271

Parity unpinned, as for the headers: the reference has no fixed PBFT message vectors, so the expected values
are the restatement's; the tests also state the verdict they expect for every case they build."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fisco-bcos_amd", "lib")

KECCAK256, SM3 = 0, 1
K1, SM2 = 0, 1  # suites; the hasher follows the suite (ProtocolInitializer.cpp:102-116)
SUITES = [pytest.param(K1, id="secp256k1"), pytest.param(SM2, id="sm2")]
MSG, PROP, PREP = 1, 2, 4  # checks
E_NODE, E_MSG, E_PROP, E_PREP, E_VC, E_GQ = 1, 2, 4, 8, 16, 32  # msg_flags bits
P_OK, P_PROOF, P_QUORUM, P_UNCHECKED = 0, 1, 2, 3  # prepared_check codes
K1_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
WEIGHTS, QUORUM = (1, 1, 1, 3), 4


# ---------------------------------------------------------------- the restatement
def hasher_of(suite):
    return SM3 if suite == SM2 else KECCAK256


def verify(oracle, suite, pub, hh, sig):
    """SignatureCrypto::verify with a known key; only r || s is read, fewer than 64 bytes fail."""
    if len(sig) < 64:
        return False
    if suite == K1:
        return oracle.secp256k1_verify(pub, hh, sig[:64])
    return oracle.sm2_recover(hh, sig[:64] + pub) == pub


def node_of(cs, index):
    """getConsensusNodeByIndex (ConsensusConfig.cpp:150-158): None for an index that names no node."""
    return index if 0 <= index < len(cs.node_ids) else None


def message_hash(oracle, suite, m):
    """signatureDataHash: the given one (zero-filled to 32 bytes), or the digest of what was signed
    (PBFTMessage.cpp:92-98)."""
    if m.signature_hash:
        return m.signature_hash.ljust(32, b"\0")
    return oracle.hash_(hasher_of(suite), m.signed_data)


def check_precommit_weight(oracle, suite, pp, cs):
    """PBFTCacheProcessor.cpp:795-821 -> (code, per-proof verdicts).  Every proof is judged on its own (the
    engine reports them all; the reference stops at the first failure, :806-816)."""
    rows, weight = [], 0
    hh = pp.hash.ljust(32, b"\0")
    for pr in pp.proofs:
        node = node_of(cs, pr.index)  # :805-809
        ok = node is not None and verify(oracle, suite, cs.node_ids[node], hh, pr.signature)  # :811-816
        rows.append(int(ok))
        if node is not None:
            weight = (weight + cs.weights[node]) & (2**64 - 1)  # per list entry: a duplicate counts twice (:817)
    if not all(rows):
        return P_PROOF, rows
    return (P_QUORUM if weight < cs.min_required_quorum else P_OK), rows  # :820


def check_message(oracle, suite, m, cs):
    """One message's own bits (1-8) -> (hash, flags, prepared codes, sig_ok entries: the message signature, the
    proposal signature, the proofs)."""
    hh = message_hash(oracle, suite, m)
    node = node_of(cs, m.generated_from)
    flags = 0 if node is not None else E_NODE  # PBFTEngine.cpp:735-741, :759-767
    sig_ok = [2, 2]
    if m.checks & MSG:  # :742-748
        sig_ok[0] = int(node is not None and verify(oracle, suite, cs.node_ids[node], hh, m.signature))
        flags |= 0 if sig_ok[0] else E_MSG
    if m.checks & PROP:  # :755-758 (absent), :769-770
        sig_ok[1] = int(len(m.proposal_signature) > 0 and node is not None and
                        verify(oracle, suite, cs.node_ids[node], m.proposal_hash.ljust(32, b"\0"), m.proposal_signature))
        flags |= 0 if sig_ok[1] else E_PROP
    prepared = []
    for pp in m.prepared:  # PBFTEngine.cpp:1162-1178
        if m.checks & PREP:
            code, rows = check_precommit_weight(oracle, suite, pp, cs)
            flags |= E_PREP if code else 0
        else:
            code, rows = P_UNCHECKED, [2] * len(pp.proofs)
        prepared.append(code)
        sig_ok += rows
    return hh, flags, prepared, sig_ok


def restate(oracle, suite, msgs, cs, groups=()):
    hashes, flags, prepared, sig_ok = [], [], [], []
    for m in msgs:
        hh, f, p, s = check_message(oracle, suite, m, cs)
        hashes.append(hh)
        flags.append(f)
        prepared += p
        sig_ok += s
    own = list(flags)
    for parent, first, count in groups:  # isValidNewViewMsg's loop, PBFTEngine.cpp:1239-1263
        weight = 0
        for j in range(first, first + count):
            if own[j] & 15:  # :1243-1248
                flags[parent] |= E_VC
            node = node_of(cs, msgs[j].generated_from)
            if node is not None:  # :1249-1254
                weight = (weight + cs.weights[node]) & (2**64 - 1)
        if weight < cs.min_required_quorum:  # :1257-1262
            flags[parent] |= E_GQ
    return (np.frombuffer(b"".join(hashes), dtype=np.uint8).reshape(-1, 32), np.array(flags, dtype=np.uint32),
            np.array(prepared, dtype=np.uint8), np.array(sig_ok, dtype=np.uint8))


# ---------------------------------------------------------------- inputs
_cache = {}


def scalar(rng):
    return b"\x00" + rng.bytes(30) + b"\x01"  # in [1, n - 2] on both curves


def keys(oracle, suite, count=5):
    """Seeded key pairs: the consensus set is the first four, the fifth is an outsider."""
    key = ("keys", suite, count)
    if key not in _cache:
        rng = np.random.default_rng(200 + suite)
        sks = [scalar(rng) for _ in range(count)]
        pub = oracle.secp256k1_pubkey if suite == K1 else oracle.sm2_pubkey
        _cache[key] = (sks, [pub(sk) for sk in sks])
    return _cache[key]


def consensus(oracle, suite, weights=WEIGHTS, quorum=QUORUM):
    from bcos_gpu.header import ConsensusSet
    return ConsensusSet(node_ids=list(keys(oracle, suite)[1][:len(weights)]), weights=list(weights),
                        min_required_quorum=quorum)


def sign(oracle, suite, sk, hh, rng, mode="ok"):
    """r || s || v (65 bytes) or r || s || pub (128 bytes), as the suites' sign() return them."""
    sig = (oracle.secp256k1_sign if suite == K1 else oracle.sm2_sign)(sk, hh, scalar(rng))
    assert sig is not None
    if mode == "high_s":  # libsecp256k1's verify rejects s > n / 2 (Secp256k1Crypto.cpp:51-63)
        s = K1_N - int.from_bytes(sig[32:64], "big")
        sig = sig[:32] + s.to_bytes(32, "big") + sig[64:]
    elif mode == "short":
        sig = sig[:63]
    elif mode == "flip":
        sig = sig[:40] + bytes([sig[40] ^ 1]) + sig[41:]
    return sig


GOOD = [(0, 0, "ok"), (1, 1, "ok"), (3, 3, "ok")]  # proofs (listed index, signing key, mode): weight 5


def make(oracle, suite, specs, seed):
    """Messages from specs.  A spec: frm (generated_from), key (the signing key, default frm), mode, checks, data
    (the signed data, default 40 random bytes), given (None: the data is hashed on the device; an int: the
    digest is passed as signature_hash, cut to that many bytes and signed as zero-filled), tamper (run on the
    finished message), proposal (None: no proposal; else (signing key, mode), mode "absent": a proposal without
    a signature), prepared: a list of proof lists or of (proof list, hash length)."""
    from bcos_gpu.header import HeaderSignature
    from bcos_gpu.pbft import PBFTMessage, PrecommitProof
    rng = np.random.default_rng(seed)
    sks = keys(oracle, suite)[0]
    out = []
    for spec in specs:
        frm = spec.get("frm", 0)
        m = PBFTMessage(generated_from=frm, checks=spec.get("checks", MSG),
                        signed_data=spec["data"] if "data" in spec else rng.bytes(40))
        if spec.get("given") is not None:
            m.signature_hash = oracle.hash_(hasher_of(suite), m.signed_data)[:spec["given"]]
        hh = message_hash(oracle, suite, m)
        k = spec.get("key", frm if 0 <= frm < len(sks) else 0)
        m.signature = sign(oracle, suite, sks[k], hh, rng, spec.get("mode", "ok"))
        if spec.get("proposal") is not None:
            pk, pmode = spec["proposal"]
            m.proposal_hash = rng.bytes(32)
            m.proposal_signature = b"" if pmode == "absent" else sign(oracle, suite, sks[pk], m.proposal_hash, rng, pmode)
        for entry in spec.get("prepared", []):
            rows, hlen = entry if isinstance(entry, tuple) else (entry, 32)
            ph = rng.bytes(hlen)
            m.prepared.append(PrecommitProof(hash=ph, proofs=[
                HeaderSignature(idx, sign(oracle, suite, sks[key], ph.ljust(32, b"\0"), rng, mode))
                for idx, key, mode in rows]))
        if "tamper" in spec:
            spec["tamper"](m)
        out.append(m)
    return out


def prepare(frm=0, **over):  # PrePrepare: checkSignature and checkProposalSignature
    return dict(dict(frm=frm, checks=MSG | PROP, proposal=(frm, "ok")), **over)


def commit(frm=0, **over):  # Prepare / Commit / CheckPoint: checkSignature only
    return dict(dict(frm=frm, checks=MSG), **over)


def view_change(frm=0, prepared=(GOOD,), **over):  # the payload-signed packet: its hash comes with it
    return dict(dict(frm=frm, checks=MSG | PREP, given=32, prepared=list(prepared)), **over)


def flip_data(m):
    m.signed_data = m.signed_data[:-1] + bytes([m.signed_data[-1] ^ 1])


# (spec, the message's expected msg_flags, its expected prepared_check): every bit alone, then combinations
def flag_cases(suite):
    cases = [
        (commit(0), 0, []),
        (prepare(3), 0, []),
        (view_change(1), 0, [P_OK]),
        (dict(frm=4, checks=0), E_NODE, []),  # bit 1 alone: the node is unknown, nothing else was asked
        (dict(frm=-1, checks=0), E_NODE, []),
        (commit(1, key=2), E_MSG, []),  # the wrong key
        (commit(1, tamper=flip_data), E_MSG, []),  # tampered signed_data
        (commit(1, mode="flip"), E_MSG, []),
        (commit(1, mode="short"), E_MSG, []),  # a 63-byte signature
        (prepare(2, proposal=(2, "absent")), E_PROP, []),  # a proposal without a signature (:755-758)
        (prepare(2, proposal=(1, "ok")), E_PROP, []),  # the proposal signed by another node
        (prepare(2, proposal=(2, "short")), E_PROP, []),
        (view_change(0, [[(2, 2, "flip"), (0, 0, "ok"), (1, 1, "ok"), (3, 3, "ok")]]), E_PREP, [P_PROOF]),  # weight 5 left
        (view_change(0, [[(0, 0, "ok"), (1, 1, "ok"), (2, 2, "ok")]]), E_PREP, [P_QUORUM]),  # one short of the quorum
        (view_change(0, [[(0, 0, "ok"), (3, 3, "ok")]]), 0, [P_OK]),  # the quorum met exactly
        (view_change(0, [[(0, 0, "ok"), (1, 1, "ok"), (0, 0, "ok"), (1, 1, "ok")]]), 0, [P_OK]),  # only by counting twice
        (view_change(0, [[(0, 0, "ok"), (3, 3, "ok"), (4, 4, "ok")]]), E_PREP, [P_PROOF]),  # an index equal to n
        (view_change(0, [[(-1, 0, "ok"), (0, 0, "ok"), (3, 3, "ok")]]), E_PREP, [P_PROOF]),  # a negative index
        (view_change(0, [[(0, 0, "ok"), (3, 3, "short"), (1, 1, "ok")]]), E_PREP, [P_PROOF]),  # a 63-byte proof
        (view_change(0, [[(0, 0, "ok"), (3, 3, "ok"), (2, 1, "ok")]]), E_PREP, [P_PROOF]),  # node 1's proof under 2
        (view_change(0, [GOOD, [(3, 3, "ok")], GOOD]), E_PREP, [P_OK, P_QUORUM, P_OK]),  # the middle one of three
        (view_change(0, [GOOD], checks=MSG), 0, [P_UNCHECKED]),  # prepared proposals not asked for
        (view_change(0, [[(2, 2, "flip")]], checks=MSG), 0, [P_UNCHECKED]),
        (commit(4), E_NODE | E_MSG, []),  # an unknown node's signature has no key
        (prepare(5, proposal=(0, "ok")), E_NODE | E_MSG | E_PROP, []),
        (prepare(-1, proposal=(0, "absent")), E_NODE | E_MSG | E_PROP, []),
        (prepare(1, key=0, proposal=(0, "ok")), E_MSG | E_PROP, []),
        (dict(frm=2, checks=MSG | PROP | PREP, mode="flip", proposal=(2, "flip"), prepared=[[(0, 0, "ok")]]),
         E_MSG | E_PROP | E_PREP, [P_QUORUM]),
        (dict(frm=2, checks=PROP, mode="flip", proposal=(2, "ok")), 0, []),  # the bad message signature not asked for
        (dict(frm=2, checks=PREP, mode="flip", prepared=[GOOD]), 0, [P_OK]),
    ]
    if suite == K1:
        cases.append((commit(1, mode="high_s"), E_MSG, []))
    return cases


def flag_run(oracle, suite):
    key = ("flags", suite)
    if key not in _cache:
        cs = consensus(oracle, suite)
        cases = flag_cases(suite)
        msgs = make(oracle, suite, [c[0] for c in cases], seed=31 + suite)
        _cache[key] = (msgs, cs, cases, restate(oracle, suite, msgs, cs))
    return _cache[key]


def mixed_run(oracle, suite):
    """65 seeded messages of 0, 1, 2, 4 and 7 rows (a message's rows straddle the keyed kernel's workgroups of 4
    rows), mostly passing: (msgs, cs, expected)."""
    key = ("mixed", suite)
    if key not in _cache:
        cs = consensus(oracle, suite)
        pool = [lambda j: commit(j % 4), lambda j: prepare(j % 4), lambda j: dict(frm=j % 4, checks=0),
                lambda j: view_change(j % 4), lambda j: view_change(j % 4, [GOOD, GOOD]),
                lambda j: commit(j % 4, given=None, data=bytes(j))]
        bad = {6: commit(1, mode="flip"), 13: prepare(2, proposal=(2, "absent")), 22: commit(4),
               27: view_change(1, [[(0, 0, "ok"), (1, 1, "flip"), (3, 3, "ok")]]), 40: view_change(3, [[(3, 3, "ok")]])}
        specs = [bad.get(j, pool[j % len(pool)](j)) for j in range(65)]
        msgs = make(oracle, suite, specs, seed=41 + suite)
        want = restate(oracle, suite, msgs, cs)
        assert int((want[1] == 0).sum()) == 60 and set(want[3].tolist()) == {0, 1, 2}
        _cache[key] = (msgs, cs, want)
    return _cache[key]


def new_view_run(oracle, suite):
    """Two NewViews and their view changes in one call, plus a prepare that belongs to no group:
    (msgs, groups, cs)."""
    key = ("newview", suite)
    if key not in _cache:
        cs = consensus(oracle, suite)
        specs = [view_change(3, [], given=32), view_change(0), view_change(1), view_change(3),  # 0: weight 5, all pass
                 view_change(2, [], given=32), view_change(0), view_change(1, mode="flip"), view_change(3),  # 4: a bad child
                 prepare(0)]
        _cache[key] = (make(oracle, suite, specs, seed=51 + suite), [(0, 1, 3), (4, 5, 3)], cs)
    return _cache[key]


def empty_set_run(oracle, suite):
    """A NewView, a prepare and a view change against a consensus set of no nodes: (msgs, cs)."""
    key = ("nobody", suite)
    if key not in _cache:
        msgs = make(oracle, suite, [commit(0), prepare(1), view_change(2, [[(0, 0, "ok")]])], seed=81 + suite)
        _cache[key] = (msgs, consensus(oracle, suite, weights=(), quorum=1))
    return _cache[key]


def assert_same(got, want, what=""):
    for name, g, w in zip(("msg_hash32", "msg_flags", "prepared_check", "sig_ok"), got, want):
        assert np.array_equal(np.asarray(g), w), (what, name, np.asarray(g).tolist(), w.tolist())


# ---------------------------------------------------------------- CPU
def test_restatement_accepts_honest_messages(oracle):
    """Before any GPU use: the restatement verifies what sign() made, for every message kind and a NewView."""
    for suite in (K1, SM2):
        sks, pubs = keys(oracle, suite)
        rng = np.random.default_rng(1)
        hh = rng.bytes(32)
        for k in range(5):
            assert verify(oracle, suite, pubs[k], hh, sign(oracle, suite, sks[k], hh, rng))
        msgs, groups, cs = new_view_run(oracle, suite)
        honest = msgs[:4] + msgs[8:]
        hashes, flags, prepared, sig_ok = restate(oracle, suite, honest, cs, groups[:1])
        assert flags.tolist() == [0] * 5 and prepared.tolist() == [P_OK] * 3
        assert sorted(set(sig_ok.tolist())) == [1, 2] and int((sig_ok == 1).sum()) == 4 + 9 + 2
        assert hashes[4].tobytes() == oracle.hash_(hasher_of(suite), honest[4].signed_data)
        assert hashes[1].tobytes() == honest[1].signature_hash
        mixed_run(oracle, suite)


def test_restatement_rejects_each_tampered_part(oracle):
    """Every case of the flag table gets the bits and the prepared-proposal codes the table states."""
    for suite in (K1, SM2):
        msgs, cs, cases, want = flag_run(oracle, suite)
        assert want[1].tolist() == [c[1] for c in cases]
        assert want[2].tolist() == [code for c in cases for code in c[2]]
        assert {c[1] for c in cases} >= {0, E_NODE, E_MSG, E_PROP, E_PREP}
        # a failed row leaves the other rows' verdicts alone: the first bad-proof case keeps its three good proofs
        at = [i for i, c in enumerate(cases) if c[2] == [P_PROOF]][0]
        start = sum(2 + sum(len(p.proofs) for p in m.prepared) for m in msgs[:at])
        assert want[3][start:start + 6].tolist() == [1, 2, 0, 1, 1, 1]
        # the groups: every view change passes and the weight is 5; one bad child; one short of the quorum
        msgs, groups, cs = new_view_run(oracle, suite)
        assert restate(oracle, suite, msgs, cs, groups)[1].tolist() == [0, 0, 0, 0, E_VC, 0, E_MSG, 0, 0]
        assert restate(oracle, suite, msgs, cs, [(0, 1, 2), (4, 7, 1)])[1][[0, 4]].tolist() == [E_GQ, E_GQ]
        assert restate(oracle, suite, msgs, cs, [(0, 5, 2)])[1][0] == E_VC | E_GQ


def test_new_symbols_exported():
    """The three entry points are declared in the header, exported by the library and typed in _lib._SIGS."""
    from bcos_gpu import _lib, device, pbft
    names = ["bcosgpu_pbft_check", "bcosgpu_pbft_check_dev", "bcosgpu_pbft_check_work_size"]
    syms = _lib.header_symbols()
    for name in names:
        assert name in syms and name in _lib._SIGS and hasattr(_lib.lib(), name), name
    assert len(_lib._SIGS["bcosgpu_pbft_check"][1]) == 11 and len(_lib._SIGS["bcosgpu_pbft_check_dev"][1]) == 30
    assert device.pbft_check_work_size(65, 300) >= 300
    import ctypes
    assert ctypes.sizeof(pbft._PBFTMessageView) == 14 * 8 and ctypes.sizeof(pbft._PrecommitProofView) == 32
    assert (pbft.E_NODE, pbft.E_MSG_SIG, pbft.E_PROPOSAL_SIG, pbft.E_PREPARED, pbft.E_VIEWCHANGE,
            pbft.E_GROUP_QUORUM) == (1, 2, 4, 8, 16, 32)


# ---------------------------------------------------------------- the same through C++
def write_fixture(path, oracle, suite, msgs, groups, cs):
    def bs(b):
        return struct.pack("<I", len(b)) + bytes(b)
    w = [b"PBFT", struct.pack("<iI", suite, len(cs.node_ids)), b"".join(cs.node_ids),
         struct.pack("<%dQ" % len(cs.weights), *cs.weights), struct.pack("<Q", cs.min_required_quorum),
         struct.pack("<I", len(msgs))]
    for m in msgs:
        w += [struct.pack("<qI", m.generated_from, m.checks), bs(m.signed_data), bs(m.signature_hash), bs(m.signature),
              bs(m.proposal_hash), bs(m.proposal_signature), struct.pack("<I", len(m.prepared))]
        for pp in m.prepared:
            w += [bs(pp.hash), struct.pack("<I", len(pp.proofs))]
            for pr in pp.proofs:
                w += [struct.pack("<q", pr.index), bs(pr.signature)]
    w.append(struct.pack("<I", len(groups)))
    w += [struct.pack("<3Q", *g) for g in groups]
    hashes, flags, prepared, sig_ok = restate(oracle, suite, msgs, cs, groups)
    w += [hashes.tobytes(), flags.astype("<u4").tobytes(), bs(prepared.tobytes()), bs(sig_ok.tobytes())]
    with open(path, "wb") as f:
        f.write(b"".join(w))


def _run_cpp(tmp_path, oracle):
    exe = str(tmp_path / "pbft_check_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "pbft_check_test.cpp"), "-L" + LIBDIR, "-lbcosgpu",
                    "-Wl,-rpath," + LIBDIR], check=True)
    fixtures = []
    for suite in (K1, SM2):
        msgs, cs, _, _ = flag_run(oracle, suite)
        nv, groups, _ = new_view_run(oracle, suite)
        fx = str(tmp_path / ("pbft%d.bin" % suite))
        write_fixture(fx, oracle, suite, nv + msgs, groups, cs)
        fixtures.append(fx)
    return subprocess.run([exe] + fixtures, capture_output=True, text=True, timeout=300)


def test_pbft_arguments_cpp(tmp_path, oracle):
    """The host call's argument checks through C++ views (no GPU needed)."""
    r = _run_cpp(tmp_path, oracle)
    assert r.returncode in (0, 77), r.stdout + r.stderr
    assert "arguments ok" in r.stdout or "pbft_check_test: ok" in r.stdout


# ---------------------------------------------------------------- GPU
def host_check(suite, msgs, cs, groups=()):
    from bcos_gpu import pbft
    return pbft.check_messages(suite, msgs, cs, groups)


def device_check(suite, msgs, cs, groups=(), slots=None, work=None, want_sig_ok=True):
    """bcosgpu_pbft_check_dev over torch tensors: the proof rows of all prepared proposals first, then each
    message's signature and proposal-signature rows; slots (ids of the consensus keys) selects the
    registered-key rows, None the key rows.  Returns what host_check returns."""
    import torch
    from bcos_gpu import device
    n, nodes = len(msgs), len(cs.node_ids)
    rhash, sig, weight, slot, pub = [], [], [], [], []

    def put(index, signature, hh):
        node = index if 0 <= index < nodes and len(signature) >= 64 else None
        rhash.append(bytes(hh).ljust(32, b"\0"))
        sig.append(signature[:64] if node is not None else bytes(64))
        weight.append(cs.weights[node] if node is not None else 0)
        slot.append(int(slots[node]) if node is not None and slots is not None else -1)
        pub.append(cs.node_ids[node] if node is not None else bytes(64))
        return len(sig) - 1

    msg_row, prop_row, prep_off, prep_row_off, data, data_off = [], [], [0], [], [], [0]
    for m in msgs:  # the proof rows first, back to back: prep_row_off is a CSR over them
        for pp in m.prepared:
            prep_row_off.append(len(sig))
            for pr in (pp.proofs if m.checks & PREP else []):
                put(pr.index, pr.signature, pp.hash)
        prep_off.append(len(prep_row_off))
    prep_row_off.append(len(sig))
    for m in msgs:
        data.append(b"" if m.signature_hash else m.signed_data)
        data_off.append(data_off[-1] + len(data[-1]))
        msg_row.append(put(m.generated_from, m.signature, b"") if m.checks & MSG else -1)
        prop_row.append(put(m.generated_from, m.proposal_signature, m.proposal_hash)
                        if m.checks & PROP and m.proposal_signature else -1)
    rows, nprep = len(sig), len(prep_row_off) - 1

    def u8(b, shape):
        return torch.from_numpy(np.frombuffer(bytes(b) + bytes(8), dtype=np.uint8).copy()).cuda()[:int(np.prod(shape))] \
            .reshape(shape)

    def i64(v):
        return torch.from_numpy(np.array(list(v) + [0], dtype=np.int64)).cuda()[:len(v)]

    known = [0 <= m.generated_from < nodes for m in msgs]
    msg_hash = torch.full((n, 32), 0xAA, dtype=torch.uint8, device="cuda")
    msg_flags = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    prepared = torch.full((nprep + 1,), 0xAA, dtype=torch.uint8, device="cuda")[:nprep]
    sig_ok = torch.full((rows + 1,), 0xAA, dtype=torch.uint8, device="cuda")[:rows] if want_sig_ok else None
    if work is None:
        work = torch.full((device.pbft_check_work_size(n, rows),), 0xFF, dtype=torch.uint8, device="cuda")
    device.pbft_check(
        suite, u8(b"".join(data), (data_off[-1],)), i64(data_off), u8(bytes(0 if k else E_NODE for k in known), (n,)),
        i64([cs.weights[m.generated_from] if k else 0 for m, k in zip(msgs, known)]),
        u8(bytes(m.checks for m in msgs), (n,)), i64(msg_row), i64(prop_row), i64(prep_off), i64(prep_row_off),
        u8(b"".join(rhash), (rows, 32)), u8(b"".join(sig), (rows, 64)), i64(weight), cs.min_required_quorum, msg_hash,
        msg_flags, prepared, work, given=u8(b"".join(m.signature_hash.ljust(32, b"\0") for m in msgs), (n, 32)),
        given_mask=u8(bytes(int(bool(m.signature_hash)) for m in msgs), (n,)),
        row_slot=torch.from_numpy(np.array(slot + [0], dtype=np.int32)).cuda()[:rows] if slots is not None else None,
        row_pub=u8(b"".join(pub), (rows, 64)) if slots is None else None,
        groups=i64([x for g in groups for x in g]) if groups else None, sig_ok=sig_ok)
    torch.cuda.synchronize()
    row_ok = sig_ok.cpu().numpy() if want_sig_ok else np.zeros(rows, dtype=np.uint8)
    out, p = [], 0
    for m, mr, pr in zip(msgs, msg_row, prop_row):
        out.append(row_ok[mr] if mr >= 0 else 2)
        out.append(row_ok[pr] if pr >= 0 else 0 if m.checks & PROP else 2)
        for pp in m.prepared:
            out += row_ok[prep_row_off[p]:prep_row_off[p + 1]].tolist() if m.checks & PREP else [2] * len(pp.proofs)
            p += 1
    return (msg_hash.cpu().numpy(), msg_flags.cpu().numpy().astype(np.uint32), prepared.cpu().numpy(),
            np.array(out, dtype=np.uint8))


def all_paths(gpu, oracle, suite, msgs, cs, groups=(), what=""):
    """The host call, the device path with slot ids and the device path with key rows against the restatement."""
    want = restate(oracle, suite, msgs, cs, groups)
    assert_same(host_check(suite, msgs, cs, groups), want, what + " host")
    slots = gpu.register_keys(suite, np.frombuffer(b"".join(cs.node_ids), dtype=np.uint8).reshape(-1, 64))
    assert (slots >= 0).all()
    assert_same(device_check(suite, msgs, cs, groups, slots=slots), want, what + " dev slots")
    assert_same(device_check(suite, msgs, cs, groups), want, what + " dev keys")
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 64, 65])
@pytest.mark.parametrize("suite", SUITES)
def test_message_geometry(oracle, gpu, suite, n):
    """Runs of 1, 2, 64 and 65 messages (the wave edge of the one-message-per-lane kernels) of 0, 1, 2, 4 and 7
    rows each."""
    msgs, cs, want = mixed_run(oracle, suite)
    nprep = sum(len(m.prepared) for m in msgs[:n])
    nsig = sum(2 + sum(len(p.proofs) for p in m.prepared) for m in msgs[:n])
    got = all_paths(gpu, oracle, suite, msgs[:n], cs, what="n=%d" % n)
    assert_same(got, (want[0][:n], want[1][:n], want[2][:nprep], want[3][:nsig]))


@pytest.mark.gpu
@pytest.mark.parametrize("suite", SUITES)
def test_empty_parts(oracle, gpu, suite):
    """A message with no checks and no rows, a prepared proposal with no proofs (below the quorum unless the
    quorum is 0), a group of no view changes (likewise), and a call with no rows at all."""
    cs, cs0 = consensus(oracle, suite), consensus(oracle, suite, quorum=0)
    msgs = make(oracle, suite, [dict(frm=2, checks=0), view_change(1, [[]]), commit(3), view_change(0, [[], GOOD, []])],
                seed=61)
    groups = [(2, 0, 0), (0, 4, 0)]
    want = all_paths(gpu, oracle, suite, msgs, cs, groups, what="empty")
    assert want[1].tolist() == [E_GQ, E_PREP, E_GQ, E_PREP] and want[2].tolist() == [P_QUORUM, P_QUORUM, P_OK, P_QUORUM]
    want = all_paths(gpu, oracle, suite, msgs, cs0, groups, what="empty, quorum 0")
    assert want[1].tolist() == [0] * 4 and want[2].tolist() == [P_OK] * 4
    none = make(oracle, suite, [dict(frm=2, checks=0), dict(frm=7, checks=0), view_change(1, [GOOD], checks=0)], seed=62)
    want = all_paths(gpu, oracle, suite, none, cs, [(0, 1, 2)], what="no rows")
    assert want[1].tolist() == [E_VC | E_GQ, E_NODE, 0] and want[2].tolist() == [P_UNCHECKED]
    assert want[3].tolist() == [2] * 9


@pytest.mark.gpu
@pytest.mark.parametrize("suite", SUITES)
def test_every_flag(oracle, gpu, suite):
    """Every bit of msg_flags one at a time, then combinations (the table in flag_cases)."""
    msgs, cs, cases, want = flag_run(oracle, suite)
    got = all_paths(gpu, oracle, suite, msgs, cs, what="flags")
    assert got[1].tolist() == [c[1] for c in cases]
    assert got[2].tolist() == [code for c in cases for code in c[2]]


@pytest.mark.gpu
@pytest.mark.parametrize("suite", SUITES)
def test_hash(oracle, gpu, suite):
    """The device hash against the given one: signed data of 0, 135, 136 and 137 bytes (the Keccak rate's edge),
    55, 56 and 64 (SM3's block edges) and 40 in one wave; the same messages with their digest given; a given
    hash of 5 bytes (zero-filled); a given hash that is not the digest of the data (it wins)."""
    cs = consensus(oracle, suite)
    rng = np.random.default_rng(71)
    lengths = [0, 135, 136, 137, 55, 56, 64, 40]
    datas = [rng.bytes(m) for m in lengths]
    specs = [commit(j % 4, data=d) for j, d in enumerate(datas)]
    specs += [commit(j % 4, data=d, given=32) for j, d in enumerate(datas)]
    specs.append(commit(1, data=datas[3], given=5))
    msgs = make(oracle, suite, specs, seed=72)
    other = make(oracle, suite, [commit(2, data=datas[1])], seed=73)[0]  # signed over the digest of datas[1] ...
    other.signature_hash, other.signed_data = message_hash(oracle, suite, other), datas[2]  # ... given beside other data
    msgs.append(other)
    want = all_paths(gpu, oracle, suite, msgs, cs, what="hash")
    assert want[1].tolist() == [0] * len(msgs)
    assert np.array_equal(want[0][:8], want[0][8:16])  # computed == given
    for j, d in enumerate(datas):
        assert want[0][j].tobytes() == oracle.hash_(hasher_of(suite), d)
    assert want[0][16].tobytes() == oracle.hash_(hasher_of(suite), datas[3])[:5] + bytes(27)
    assert want[0][17].tobytes() == want[0][1].tobytes()
    # the same signatures over data that was changed afterwards fail where the data is hashed, and only there
    for m in msgs[:16]:
        if m.signed_data:
            flip_data(m)
    want = all_paths(gpu, oracle, suite, msgs, cs, what="hash, tampered")
    assert want[1].tolist() == [0] + [E_MSG] * 7 + [0] * 10


@pytest.mark.gpu
@pytest.mark.parametrize("suite", SUITES)
def test_groups(oracle, gpu, suite):
    """A NewView whose view changes all pass, one with a failing child, weight one short of the quorum, two
    groups in one call, two groups on one parent."""
    msgs, groups, cs = new_view_run(oracle, suite)
    want = all_paths(gpu, oracle, suite, msgs, cs, groups, what="two groups")
    assert want[1].tolist() == [0, 0, 0, 0, E_VC, 0, E_MSG, 0, 0] and want[2].tolist() == [P_OK] * 6
    want = all_paths(gpu, oracle, suite, msgs, cs, [(0, 1, 2)], what="one short")  # nodes 0 and 1: weight 2
    assert want[1].tolist() == [E_GQ, 0, 0, 0, 0, 0, E_MSG, 0, 0]
    want = all_paths(gpu, oracle, suite, msgs, cs, [(0, 3, 1)], what="exactly")  # node 3 alone: weight 3 ... below 4
    assert want[1][0] == E_GQ
    want = all_paths(gpu, oracle, suite, msgs, cs, [(0, 2, 2)], what="met")  # nodes 1 and 3: weight 4
    assert want[1][0] == 0
    want = all_paths(gpu, oracle, suite, msgs, cs, [(8, 1, 3), (8, 6, 1), (0, 8, 1)], what="shared parent")
    assert want[1].tolist() == [E_GQ, 0, 0, 0, 0, 0, E_MSG, 0, E_VC | E_GQ]


@pytest.mark.gpu
@pytest.mark.parametrize("suite", SUITES)
def test_workspace_hygiene(oracle, gpu, suite):
    """Two different runs on one d_work that starts as 0xFF, with and without a caller's sig_ok array (without
    one the row verdicts live in d_work): each gives its own result."""
    import torch
    from bcos_gpu import device
    msgs, cs, want = mixed_run(oracle, suite)
    other, groups, cs2 = new_view_run(oracle, suite)
    want2 = restate(oracle, suite, other, cs2, groups)
    work = torch.full((device.pbft_check_work_size(65, 400),), 0xFF, dtype=torch.uint8, device="cuda")
    slots = gpu.register_keys(suite, np.frombuffer(b"".join(cs.node_ids), dtype=np.uint8).reshape(-1, 64))
    for sl in (slots, None):
        for want_ok in (True, False):
            got = device_check(suite, msgs, cs, slots=sl, work=work, want_sig_ok=want_ok)
            assert_same(got[:3], want[:3], "mixed")
            got = device_check(suite, other, cs2, groups, slots=sl, work=work, want_sig_ok=want_ok)
            assert_same(got[:3], want2[:3], "new view")


@pytest.mark.gpu
@pytest.mark.parametrize("suite", SUITES)
def test_stale_slot_ids_fail(oracle, gpu, suite):
    """Slot ids from before a bcosgpu_clear_keys name no key: every row fails; fresh ids and the host call (which
    registers again) pass."""
    msgs, groups, cs = new_view_run(oracle, suite)
    want = restate(oracle, suite, msgs, cs, groups)
    pubs = np.frombuffer(b"".join(cs.node_ids), dtype=np.uint8).reshape(-1, 64)
    old = gpu.register_keys(suite, pubs)
    gpu.clear_keys(suite)
    fresh_first = gpu.register_keys(suite, pubs[:1])  # the cache is in use again, under a new generation
    assert fresh_first[0] >= 0 and fresh_first[0] != old[0]
    got = device_check(suite, msgs, cs, groups, slots=old)
    vc = E_MSG | E_PREP
    assert got[1].tolist() == [E_MSG | E_VC, vc, vc, vc, E_MSG | E_VC, vc, vc, vc, E_MSG | E_PROP]
    assert got[2].tolist() == [P_PROOF] * 6 and not (got[3] == 1).any()
    assert np.array_equal(got[0], want[0])
    assert_same(device_check(suite, msgs, cs, groups, slots=gpu.register_keys(suite, pubs)), want)
    assert_same(host_check(suite, msgs, cs, groups), want)


@pytest.mark.gpu
@pytest.mark.parametrize("suite", SUITES)
def test_host_call_key_path_small_cache(oracle, gpu, suite):
    """In a fresh process with BCOSGPU_KEY_CACHE=2 the four consensus keys do not fit, so the host call takes
    the key rows: the same verdicts."""
    msgs, cs, want = mixed_run(oracle, suite)
    env = dict(os.environ, BCOSGPU_KEY_CACHE="2")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", str(suite)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["capacity"] == 2 and out["keys"] <= 2
    # the registration did not cover every key, so no call counted as keyed: the rows carried the keys
    assert out["keyed"] == 0 and out["generic"] > 0
    assert bytes.fromhex(out["hash32"]) == want[0].tobytes()
    assert out["flags"] == want[1].tolist() and out["prepared"] == want[2].tolist() and out["sig_ok"] == want[3].tolist()
    # before any key was registered in that process: an empty consensus set gives verdicts, not an error
    few, nobody = empty_set_run(oracle, suite)
    want = restate(oracle, suite, few, nobody, [(0, 1, 2)])
    assert out["empty_flags"] == want[1].tolist() == [E_NODE | E_MSG | E_VC | E_GQ, E_NODE | E_MSG | E_PROP,
                                                       E_NODE | E_MSG | E_PREP]
    assert out["empty_prepared"] == want[2].tolist() == [P_PROOF] and out["empty_sig_ok"] == want[3].tolist()


@pytest.mark.gpu
def test_pbft_check_cpp_on_gpu(tmp_path, oracle, gpu):
    r = _run_cpp(tmp_path, oracle)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pbft_check_test: ok" in r.stdout


def _child(suite):
    """The host call in this (fresh) process over the mixed run; one JSON line."""
    sys.path.insert(0, os.path.join(ROOT, "fisco-bcos_amd"))
    sys.path.insert(0, ROOT)
    import bcos_gpu
    from oracle import oracle
    oracle.build()
    few, nobody = empty_set_run(oracle, suite)
    empty = host_check(suite, few, nobody, [(0, 1, 2)])  # first: no key is registered in this process yet
    msgs, cs, _ = mixed_run(oracle, suite)
    hashes, flags, prepared, sig_ok = host_check(suite, msgs, cs)
    info = bcos_gpu.key_cache_info(suite)
    print(json.dumps({"hash32": hashes.tobytes().hex(), "flags": flags.tolist(), "prepared": prepared.tolist(),
                      "sig_ok": sig_ok.tolist(), "capacity": info["capacity"], "keys": info["keys"],
                      "keyed": info["keyed"], "generic": info["generic"], "empty_flags": empty[1].tolist(),
                      "empty_prepared": empty[2].tolist(), "empty_sig_ok": empty[3].tolist()}))


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "child":
    _child(int(sys.argv[2]))
