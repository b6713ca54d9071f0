"""The state root (StateStorage::hash / KeyPageStorage::hash) through every layer: the host packer
(bcosgpu_pack_state_entries), the fused hash-and-XOR kernel (bcosgpu_state_root_dev), the host call
(bcosgpu_state_root) and the C++ adapter (tests/cpp/state_root_test.cpp over include/bcos_gpu.hpp
calculateStateRoot), against a Python restatement of the reference's rules over oracle.hash_ (KAT-pinned
Keccak-256 / SM3):

  Entry::hash                 bcos-framework/bcos-framework/storage/Entry.h:229-309
  StateStorage::hash          bcos-table/src/StateStorage.h:397-431
  PageData::hash              bcos-table/src/KeyPageStorage.h:862-893
  KeyPageStorage::hash        bcos-table/src/KeyPageStorage.cpp:351-406

Parity unpinned beyond Entry.cpp's case: the hashes pinned in the reference's TestKeyPageStorage.cpp come from a
fake hasher under __APPLE__; its one real check is the property test
bcos-table/test/unittests/libtable/Entry.cpp:168-219, restated in test_reference_entry_case."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fisco-bcos_amd", "lib")

NORMAL, DELETED, EMPTY, MODIFIED = 0, 1, 2, 3  # Entry::Status
XOR_NAMES = 1
V3_0, V3_1 = 0, 0x03010000  # Entry.cpp:179 passes 0 for the 3.0 rules; BlockVersion::V3_1_VERSION
KECCAK256, SM3 = 0, 1
HASHERS = [pytest.param(KECCAK256, id="keccak256"), pytest.param(SM3, id="sm3")]
ZERO = bytes(32)
ONE = bytes(31) + b"\x01"  # HashType(0x1), FixedBytes.h:171


# ---------------------------------------------------------------- the restatement
def _xor(a, b):
    return (int.from_bytes(a, "big") ^ int.from_bytes(b, "big")).to_bytes(32, "big")


def entry_hash(oracle, hasher, e, version):
    """Entry::hash (Entry.h:229-309)."""
    if version >= V3_1:  # :233-278: table, key and, for a MODIFIED entry, the value through one hasher
        if e.status == MODIFIED:
            return oracle.hash_(hasher, e.table + e.key + e.value)
        if e.status == DELETED:
            return oracle.hash_(hasher, e.table + e.key)
        return ZERO
    if e.status == MODIFIED:  # 3.0, :281-285
        return oracle.hash_(hasher, e.value)
    if e.status == DELETED:  # :293-295
        return ONE
    return ZERO


def contribution(oracle, hasher, e, version):
    """One entry's term of the XOR: StateStorage.h:412-416 and KeyPageStorage.cpp:385-390 (XOR_NAMES set),
    KeyPageStorage.h:870-881 (set at 3.0, not set from 3.1 on); only dirty entries count."""
    if e.status not in (MODIFIED, DELETED):
        return ZERO
    h = entry_hash(oracle, hasher, e, version)
    if e.flags & XOR_NAMES:
        h = _xor(h, _xor(oracle.hash_(hasher, e.table), oracle.hash_(hasher, e.key)))
    return h


def restate_root(oracle, hasher, entries, version):
    r = 0
    for e in entries:
        r ^= int.from_bytes(contribution(oracle, hasher, e, version), "big")
    return r.to_bytes(32, "big")


def restate_pack(entries):
    """table || key || value back to back (the value of a MODIFIED entry only), off3[3n+1], kind[n]."""
    data, off3, kind = [], [0], []
    for e in entries:
        for part in (e.table, e.key, e.value if e.status == MODIFIED else b""):
            data.append(part)
            off3.append(off3[-1] + len(part))
        kind.append(e.status | (e.flags << 4))
    return b"".join(data), np.array(off3, dtype=np.uint64), np.array(kind, dtype=np.uint8)


# ---------------------------------------------------------------- inputs
def make_entries(seed, n):
    """Seeded entries with mixed statuses and flags; the first seven are the edge views: an empty table, an
    empty key, an empty value, a DELETED entry that still carries a value, two clean entries, and an entry
    with nothing in it."""
    from bcos_gpu.state import StateEntry
    rng = np.random.default_rng(seed)
    tables = [b""] + [b"/apps/" + rng.bytes(int(m)).hex().encode() for m in rng.integers(1, 28, size=6)]
    out = []
    for i in range(n):
        u = rng.random()
        vlen = 32 if u < 0.6 else 0 if u < 0.65 else int(rng.integers(1, 300))
        s = rng.random()
        out.append(StateEntry(table=tables[int(rng.integers(0, len(tables)))],
                              key=rng.bytes(int(rng.integers(0, 41))), value=rng.bytes(vlen),
                              status=MODIFIED if s < 0.6 else DELETED if s < 0.8 else NORMAL if s < 0.9 else EMPTY,
                              flags=int(rng.integers(0, 2))))
    edge = [StateEntry(b"", b"k0", b"v" * 32, MODIFIED, 1), StateEntry(b"t1", b"", b"v" * 5, MODIFIED, 1),
            StateEntry(b"t2", b"k2", b"", MODIFIED, 0), StateEntry(b"t3", b"k3", b"stale value", DELETED, 1),
            StateEntry(b"t4", b"k4", b"clean", NORMAL, 1), StateEntry(b"t5", b"k5", b"clean", EMPTY, 0),
            StateEntry(b"", b"", b"", MODIFIED, 1)]
    out[:len(edge)] = edge[:n]
    return out


_cache = {}


def contributions(oracle, hasher, version):
    """The terms of the 4099 shared entries, computed once per hasher and version: int array of Python ints."""
    key = (hasher, version)
    if key not in _cache:
        _cache[key] = [int.from_bytes(contribution(oracle, hasher, e, version), "big") for e in shared_entries()]
    return _cache[key]


def shared_entries():
    if "entries" not in _cache:
        _cache["entries"] = make_entries(41, 4099)
    return _cache["entries"]


def prefix_root(oracle, hasher, version, n):
    r = 0
    for c in contributions(oracle, hasher, version)[:n]:
        r ^= c
    return r.to_bytes(32, "big")


def device_root(hasher, version, entries, work=None):
    """bcosgpu_state_root_dev over torch tensors, from the native packer's layout."""
    import torch
    from bcos_gpu import device, state
    data, off3, kind = state.pack_state_entries(entries)
    n = len(entries)
    d_data = torch.from_numpy(np.concatenate([data, np.zeros(1, np.uint8)])).cuda()
    d_off = torch.from_numpy(off3.astype(np.int64)).cuda()
    d_kind = torch.from_numpy(np.concatenate([kind, np.zeros(1, np.uint8)])).cuda()[:n]
    if work is None:
        work = torch.zeros(device.state_root_work_size(n), dtype=torch.uint8, device="cuda")
    root = torch.full((32,), 0xAA, dtype=torch.uint8, device="cuda")
    device.state_root(hasher, version, d_data, d_off, d_kind, work, root)
    torch.cuda.synchronize()
    return root.cpu().numpy().tobytes()


# ---------------------------------------------------------------- CPU: the packer
def test_packer_matches_restatement():
    from bcos_gpu import lib, state
    entries = make_entries(7, 300)
    data, off3, kind = state.pack_state_entries(entries)
    want_data, want_off3, want_kind = restate_pack(entries)
    assert data.tobytes() == want_data
    assert np.array_equal(off3, want_off3)
    assert np.array_equal(kind, want_kind)
    views, keep = state.state_entry_views(entries)
    assert int(lib().bcosgpu_state_entries_size(views, len(entries))) == len(want_data) == int(off3[-1])
    # the DELETED entry's stale value and the clean entries' values are not packed
    for i in (3, 4, 5):
        assert off3[3 * i + 3] == off3[3 * i + 2]
    del keep


def test_packer_large_batch_threaded():
    """Past the packer's threading threshold the result is the same as the restatement's."""
    from bcos_gpu import state
    entries = make_entries(9, 300) * 40
    data, off3, kind = state.pack_state_entries(entries)
    want_data, want_off3, want_kind = restate_pack(entries)
    assert data.tobytes() == want_data and np.array_equal(off3, want_off3) and np.array_equal(kind, want_kind)


def test_packer_rejects_bad_views():
    from bcos_gpu import _lib, lib, state
    entries = make_entries(7, 20)
    n = len(entries)
    views, keep = state.state_entry_views(entries)
    size = int(lib().bcosgpu_state_entries_size(views, n))
    out = np.zeros(size + 8, dtype=np.uint8)
    off3 = np.zeros(3 * n + 1, dtype=np.uint64)
    kind = np.zeros(n, dtype=np.uint8)

    def pack(cap):
        return lib().bcosgpu_pack_state_entries(views, n, out.ctypes.data, cap, off3.ctypes.data, kind.ctypes.data)

    assert pack(size) == _lib.OK
    assert pack(size - 1) == _lib.E_ARG  # short cap
    saved = views[8].status
    for bad in (4, -1):  # a status outside 0..3
        views[8].status = bad
        assert pack(size) == _lib.E_ARG
    views[8].status = saved
    assert pack(size) == _lib.OK
    for name in ("table", "key", "value"):  # a null pointer with a length
        v = state._StateEntryView()
        v.status, v.flags = MODIFIED, 1
        setattr(v, name + "_len", 3)
        one = (state._StateEntryView * 1)(v)
        assert lib().bcosgpu_pack_state_entries(one, 1, out.ctypes.data, size, off3.ctypes.data,
                                                kind.ctypes.data) == _lib.E_ARG
    # ... but a DELETED entry's value is never read: a null value with a length is fine there
    v = state._StateEntryView()
    v.status, v.value_len = DELETED, 3
    one = (state._StateEntryView * 1)(v)
    assert lib().bcosgpu_pack_state_entries(one, 1, out.ctypes.data, size, off3.ctypes.data,
                                            kind.ctypes.data) == _lib.OK
    assert off3[3] == 0
    # an entry of 2^32 bytes or more is refused before anything is read
    buf = ctypes.create_string_buffer(8)
    v = state._StateEntryView()
    v.status, v.value_len = MODIFIED, 1 << 32
    v.value = ctypes.cast(buf, ctypes.c_char_p)
    one = (state._StateEntryView * 1)(v)
    assert lib().bcosgpu_pack_state_entries(one, 1, out.ctypes.data, 1 << 40, off3.ctypes.data,
                                            kind.ctypes.data) == _lib.E_ARG
    del keep


# ---------------------------------------------------------------- the same through C++
def write_fixture(path, entries, oracle):
    def bs(b):
        return struct.pack("<I", len(b)) + bytes(b)
    data, off3, kind = restate_pack(entries)
    w = [b"STRT", struct.pack("<I", len(entries))]
    for e in entries:
        w += [bs(e.table), bs(e.key), bs(e.value), struct.pack("<bB", e.status, e.flags)]
    w += [bs(data), off3.astype("<u8").tobytes(), kind.tobytes()]
    for hasher in (KECCAK256, SM3):
        for version in (V3_0, V3_1):
            w.append(restate_root(oracle, hasher, entries, version))
    with open(path, "wb") as f:
        f.write(b"".join(w))


def _run_cpp(tmp_path, oracle):
    exe = str(tmp_path / "state_root_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "state_root_test.cpp"), "-L" + LIBDIR, "-lbcosgpu",
                    "-Wl,-rpath," + LIBDIR], check=True)
    fx = str(tmp_path / "state.bin")
    write_fixture(fx, make_entries(13, 300), oracle)
    return subprocess.run([exe, fx], capture_output=True, text=True, timeout=300)


def test_state_packer_cpp_matches_restatement(tmp_path, oracle):
    """The C packer through C++ views: data, off3 and kind byte-equal to the restatement (no GPU needed)."""
    r = _run_cpp(tmp_path, oracle)
    assert r.returncode in (0, 77), r.stdout + r.stderr
    assert "packer ok" in r.stdout or "state_root_test: ok" in r.stdout


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("hasher", HASHERS)
def test_reference_entry_case(oracle, gpu, hasher):
    """Entry.cpp:168-219: table "table!", key "key!", value "Hello world!" as one entry, per status, block
    version and flag."""
    from bcos_gpu import state
    t, k, v = b"table!", b"key!", b"Hello world!"

    def H(m):
        return oracle.hash_(hasher, m)

    names = _xor(H(t), H(k))
    for status in (MODIFIED, DELETED, NORMAL):
        for version in (V3_0, V3_1):
            for flags in (XOR_NAMES, 0):
                e = state.StateEntry(t, k, v, status, flags)
                got = state.state_root(hasher, version, [e])
                if status == NORMAL:  # Entry.cpp:216-218; not dirty, so no names either
                    want = ZERO
                else:
                    if version == V3_0:  # Entry.cpp:179-181
                        want = H(v) if status == MODIFIED else ONE
                    else:  # Entry.cpp:183-214
                        want = H(t + k + v) if status == MODIFIED else H(t + k)
                    if flags:
                        want = _xor(want, names)
                assert got == want, (status, version, flags)
                assert got == restate_root(oracle, hasher, [e], version)
                assert device_root(hasher, version, [e]) == want
    assert state.state_root(hasher, V3_0, [state.StateEntry(t, k, v, DELETED, 0)]) == ONE


@pytest.mark.gpu
@pytest.mark.parametrize("version", [pytest.param(V3_0, id="v3.0"), pytest.param(V3_1, id="v3.1")])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1025, 4099])
@pytest.mark.parametrize("hasher", HASHERS)
def test_reduction_boundaries(oracle, gpu, hasher, n, version):
    from bcos_gpu import state
    entries = shared_entries()[:n]
    want = prefix_root(oracle, hasher, version, n)
    assert state.state_root(hasher, version, entries) == want
    assert device_root(hasher, version, entries) == want
    if n == 4099:
        perm = np.random.default_rng(5).permutation(n)
        shuffled = [entries[int(i)] for i in perm]
        assert state.state_root(hasher, version, shuffled) == want
        assert device_root(hasher, version, shuffled) == want
        # every term twice cancels: a lane or workgroup counted twice or dropped would leave its term
        assert state.state_root(hasher, version, entries + entries) == ZERO
        assert device_root(hasher, version, entries + shuffled) == ZERO


LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 135, 136, 137, 271, 272, 273]


@pytest.mark.gpu
@pytest.mark.parametrize("hasher", HASHERS)
def test_padding_boundaries(oracle, gpu, hasher):
    """One MODIFIED entry without XOR_NAMES: at 3.1 table+key+value has each length around the SM3 (55/56,
    64 B blocks) and Keccak (135/136 B rate) padding edges, at 3.0 the value alone has; the table length is
    odd, so the key and value slices start unaligned."""
    from bcos_gpu import state
    rng = np.random.default_rng(17)
    lead = state.StateEntry(b"abc", b"", b"", NORMAL, 1)  # clean: shifts the next entry's start to 3 mod 4
    for total in LENGTHS:
        t = 7 if total >= 7 else total if total % 2 else max(total - 1, 0)
        k = min(total - t, 5)
        e = state.StateEntry(rng.bytes(t), rng.bytes(k), rng.bytes(total - t - k), MODIFIED, 0)
        want = oracle.hash_(hasher, e.table + e.key + e.value)
        assert state.state_root(hasher, V3_1, [e]) == want, total
        assert device_root(hasher, V3_1, [e]) == want, total
        assert device_root(hasher, V3_1, [lead, e]) == want, total
    for vlen in LENGTHS:
        e = state.StateEntry(rng.bytes(7), rng.bytes(4), rng.bytes(vlen), MODIFIED, 0)
        want = oracle.hash_(hasher, e.value)
        assert state.state_root(hasher, V3_0, [e]) == want, vlen
        assert device_root(hasher, V3_0, [e]) == want, vlen
        assert device_root(hasher, V3_0, [lead, e]) == want, vlen
    # 3.0 tells a MODIFIED entry with an empty value from a DELETED one: H("") against 00...01
    empty = state.state_root(hasher, V3_0, [state.StateEntry(b"t", b"k", b"", MODIFIED, 0)])
    gone = state.state_root(hasher, V3_0, [state.StateEntry(b"t", b"k", b"", DELETED, 0)])
    assert empty == oracle.hash_(hasher, b"") and gone == ONE and empty != gone


@pytest.mark.gpu
@pytest.mark.parametrize("hasher", HASHERS)
def test_mixed_lengths_in_one_wave(oracle, gpu, hasher):
    """70 entries of mixed flags and statuses, one with a 20,000-byte value."""
    from bcos_gpu import state
    entries = make_entries(29, 70)
    entries[37] = state.StateEntry(b"/apps/code", b"code", np.random.default_rng(3).bytes(20000), MODIFIED, 1)
    for version in (V3_0, V3_1):
        want = restate_root(oracle, hasher, entries, version)
        assert state.state_root(hasher, version, entries) == want
        assert device_root(hasher, version, entries) == want


@pytest.mark.gpu
@pytest.mark.parametrize("hasher", HASHERS)
def test_long_entry_threshold(oracle, gpu, hasher):
    """An entry hash over more than 1024 bytes leaves the fused kernel for the long list: the lengths on
    both sides of that threshold, at 3.1 (table + key + value, and table + key of a DELETED entry) and at 3.0
    (the value alone), one at a time and together with short entries; then 300 long entries, more than one
    workgroup of the list's kernel."""
    from bcos_gpu import state
    rng = np.random.default_rng(19)
    short = make_entries(43, 130)
    edge = []
    for total in (1023, 1024, 1025, 1026):
        edge.append(state.StateEntry(rng.bytes(7), rng.bytes(16), rng.bytes(total - 23), MODIFIED, 1))  # 3.1 total
        edge.append(state.StateEntry(rng.bytes(7), rng.bytes(16), rng.bytes(total), MODIFIED, 0))  # 3.0 value
        edge.append(state.StateEntry(rng.bytes(total - 500), rng.bytes(500), b"stale", DELETED, 1))  # 3.1 names
    for version in (V3_0, V3_1):
        for e in edge:
            want = contribution(oracle, hasher, e, version)
            assert state.state_root(hasher, version, [e]) == want
            assert device_root(hasher, version, [e]) == want
        mixed = short[:65] + edge + short[65:]
        want = restate_root(oracle, hasher, mixed, version)
        assert state.state_root(hasher, version, mixed) == want
        assert device_root(hasher, version, mixed) == want
    many = [state.StateEntry(b"/apps/t", rng.bytes(8), rng.bytes(int(m)), MODIFIED, i & 1)
            for i, m in enumerate(rng.integers(1100, 1400, size=300))]
    want = restate_root(oracle, hasher, many, V3_1)
    assert state.state_root(hasher, V3_1, many) == want
    assert device_root(hasher, V3_1, many + many) == ZERO


@pytest.mark.gpu
@pytest.mark.parametrize("hasher", HASHERS)
def test_workspace_hygiene_long_list(oracle, gpu, hasher):
    """The long list and its count live in d_work too: a call with many long entries, then one with few and
    one with none, on the same 0xFF-filled d_work, each give their own root."""
    import torch
    from bcos_gpu import device, state
    rng = np.random.default_rng(23)

    def longs(k):
        return [state.StateEntry(b"/apps/code", rng.bytes(8), rng.bytes(1500), MODIFIED, 1) for _ in range(k)]

    first = make_entries(47, 200) + longs(70)
    second = longs(3) + make_entries(53, 40)
    third = make_entries(59, 300)
    work = torch.full((device.state_root_work_size(300),), 0xFF, dtype=torch.uint8, device="cuda")
    for entries in (first, second, third, first):
        assert device_root(hasher, V3_1, entries, work) == restate_root(oracle, hasher, entries, V3_1)


@pytest.mark.gpu
@pytest.mark.parametrize("hasher", HASHERS)
def test_workspace_hygiene(oracle, gpu, hasher):
    """Two device calls on one d_work that starts as 0xFF: each gives its own root, so neither the fill nor
    the first call's partials are folded into the second."""
    import torch
    from bcos_gpu import device
    first, second = shared_entries()[:1025], make_entries(31, 65)
    work = torch.full((device.state_root_work_size(1025),), 0xFF, dtype=torch.uint8, device="cuda")
    assert device_root(hasher, V3_1, first, work) == prefix_root(oracle, hasher, V3_1, 1025)
    assert device_root(hasher, V3_1, second, work) == restate_root(oracle, hasher, second, V3_1)
    assert device_root(hasher, V3_1, [], work) == ZERO


@pytest.mark.gpu
def test_state_root_cpp_on_gpu(tmp_path, oracle, gpu):
    r = _run_cpp(tmp_path, oracle)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "state_root_test: ok" in r.stdout
