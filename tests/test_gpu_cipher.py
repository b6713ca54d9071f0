"""The storage cipher on the GPU (csrc/cipher_kernels.hip): AES-256-CBC and SM4-CBC, both directions, through the
device calls (bcosgpu_cbc_encrypt_batch_dev / _decrypt_batch_dev over torch tensors), the host calls
(bcos_gpu.cipher) and the C++ adapter (tests/cpp/cipher_test.cpp over include/bcos_gpu.hpp), against the
pure-Python restatement tests/cipher_restatement.py, which tests/test_cipher.py pins to OpenSSL's output and the
standards' vectors.

Parity unpinned beyond the reference's round trip (bcos-crypto/test/unittests/EncryptionTest.cpp:35-92, restated in
test_reference_encryption_case): mode and padding live in wedpr, which is not built here."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cipher_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fisco-bcos_amd", "lib")
CIPHERS = [pytest.param(R.AES256, id="aes256"), pytest.param(R.SM4, id="sm4")]
KEY = bytes((11 * i + 5) & 0xFF for i in range(32))
h = bytes.fromhex


# ---------------------------------------------------------------- the device calls over torch tensors
def dev_encrypt(cipher, key, values, iv=None, lead=1, work=None):
    """Packs `values` back to back from byte `lead` of the data tensor (odd: every start unaligned) and runs
    bcosgpu_cbc_encrypt_batch_dev; checks out_off and returns the ciphertexts."""
    import torch
    from bcos_gpu import device
    n = len(values)
    off = np.zeros(n + 1, dtype=np.int64)
    off[0] = lead
    for i, v in enumerate(values):
        off[i + 1] = off[i] + len(v)
    data = np.frombuffer(b"\xEE" * lead + b"".join(values) + b"\xEE", dtype=np.uint8)
    total = sum((len(v) // 16 + 1) * 16 for v in values)
    d_data = torch.from_numpy(data.copy()).cuda()
    d_off = torch.from_numpy(off).cuda()
    d_out = torch.full((total + 16,), 0xCC, dtype=torch.uint8, device="cuda")
    d_out_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    if work is None:
        work = torch.zeros(device.cbc_work_size(n), dtype=torch.uint8, device="cuda")
    device.cbc_encrypt(cipher, key, d_data, d_off, d_out, d_out_off, work, iv=iv)
    torch.cuda.synchronize()
    out, out_off = d_out.cpu().numpy().tobytes(), d_out_off.cpu().numpy()
    want_off = np.concatenate([[0], np.cumsum([(len(v) // 16 + 1) * 16 for v in values])]) if n else np.array([-1])
    assert np.array_equal(out_off, want_off)
    assert out[total:] == b"\xCC" * 16  # nothing past the last block
    return [out[int(out_off[i]):int(out_off[i + 1])] for i in range(n)]


def dev_decrypt(cipher, key, items, iv=None):
    """bcosgpu_cbc_decrypt_batch_dev over items packed back to back (lengths multiples of 16, zero allowed):
    (plaintexts, status, raw blocks per item)."""
    import torch
    from bcos_gpu import device
    n = len(items)
    assert all(len(c) % 16 == 0 for c in items)
    off = np.concatenate([[0], np.cumsum([len(c) for c in items])]).astype(np.int64)
    total = int(off[-1])
    d_in = torch.from_numpy(np.frombuffer(b"".join(items) + bytes(16), dtype=np.uint8).copy()).cuda()
    d_off = torch.from_numpy(off).cuda()
    d_out = torch.full((total + 16,), 0xCC, dtype=torch.uint8, device="cuda")
    d_len = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_st = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda")
    device.cbc_decrypt(cipher, key, d_in, d_off, d_out, d_len, d_st, iv=iv)
    torch.cuda.synchronize()
    out, lens, st = d_out.cpu().numpy().tobytes(), d_len.cpu().numpy(), d_st.cpu().numpy()
    assert out[total:] == b"\xCC" * 16
    raw = [out[int(off[i]):int(off[i + 1])] for i in range(n)]
    return [raw[i][:int(lens[i])] for i in range(n)], st, raw


def check_both_ways(cipher, key, values, iv=None, lead=1, work=None):
    """Device and host encryption equal the restatement's; device and host decryption give the values back."""
    from bcos_gpu import cipher as C
    c = R.Cipher(cipher, key, iv)
    want = [c.encrypt(v) for v in values]
    assert dev_encrypt(cipher, key, values, iv=iv, lead=lead, work=work) == want
    assert C.encrypt_values(cipher, key, values, iv=iv) == want
    plains, st, _ = dev_decrypt(cipher, key, want, iv=iv)
    assert plains == list(values) and not st.any()
    plains, st = C.decrypt_values(cipher, key, want, iv=iv)
    assert plains == list(values) and not st.any()
    return want


def state_mix(seed, n):
    """The value lengths of the state-root tests' entries: 60 % 32 bytes, 5 % empty, the rest 1-299 bytes."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        u = rng.random()
        out.append(rng.bytes(32 if u < 0.6 else 0 if u < 0.65 else int(rng.integers(1, 300))))
    return out


# ---------------------------------------------------------------- the cases
@pytest.mark.gpu
def test_standard_vectors(gpu):
    """FIPS-197 C.3 and GB/T 32907 A.1 (one block under a zero IV), SP 800-38A F.2.5 / F.2.6 (four blocks; the
    fifth is the padding block, checked against the restatement), through the device and the host calls."""
    from bcos_gpu import cipher as C
    zero = bytes(16)
    cases = [(R.AES256, bytes(range(32)), zero, h("00112233445566778899aabbccddeeff"),
              h("8ea2b7ca516745bfeafc49904b496089")),
             (R.SM4, h("0123456789abcdeffedcba9876543210"), zero, h("0123456789abcdeffedcba9876543210"),
              h("681edf34d206965e86b3e94f536e4246")),
             (R.AES256, h("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4"),
              h("000102030405060708090a0b0c0d0e0f"),
              h("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e51"
                "30c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710"),
              h("f58c4c04d6e5f1ba779eabfb5f7bfbd69cfc4e967edb808d679f777bc6702c7d"
                "39f23369a9d9bacfa530e26304231461b2eb05e2c39be9fcda6c19078c6a9d1b"))]
    for cipher, key, iv, plain, published in cases:
        want = R.encrypt(cipher, key, plain, iv)
        for got in (dev_encrypt(cipher, key, [plain], iv=iv)[0], dev_encrypt(cipher, key, [plain], iv=iv, lead=0)[0],
                    C.encrypt_values(cipher, key, [plain], iv=iv)[0]):
            assert got[:len(plain)] == published
            assert got == want and len(got) == len(plain) + 16
        plains, st, raw = dev_decrypt(cipher, key, [want], iv=iv)
        assert plains == [plain] and list(st) == [0] and raw[0][:len(plain)] == plain
        assert C.decrypt_values(cipher, key, [want], iv=iv)[0] == [plain]
        # F.2.6 proper: the published blocks alone decrypt to the plaintext blocks (the padding check then fails)
        _, st, raw = dev_decrypt(cipher, key, [published], iv=iv)
        assert raw == [plain] and list(st) == [R.Cipher(cipher, key, iv).decrypt_raw(published)[0]]


@pytest.mark.gpu
@pytest.mark.parametrize("cipher", CIPHERS)
def test_reference_encryption_case(gpu, cipher):
    """EncryptionTest.cpp:35-92: a round trip under the key "abcd" and the default IV; a damaged first ciphertext
    byte no longer gives the plaintext; the 47-byte explicit IV with the 69-byte key; a wrong IV."""
    from bcos_gpu import cipher as C
    plain = b"testAESAndSM4 plain text, longer than a block"
    key = b"abcd"
    ct = check_both_ways(cipher, key, [plain])[0]
    bad = bytes([ct[0] + 1 & 0xFF]) + ct[1:]
    want = R.decrypt(cipher, key, bad)
    plains, st, _ = dev_decrypt(cipher, key, [bad])
    assert (int(st[0]), plains[0]) == want and plains[0] != plain
    plains, st = C.decrypt_values(cipher, key, [bad])
    assert (int(st[0]), plains[0]) == want
    long_key = bytes((7 * i + 3) & 0xFF for i in range(69))
    iv = bytes((200 - i) & 0xFF for i in range(47))
    ct = check_both_ways(cipher, long_key, [plain], iv=iv)[0]
    assert ct == R.encrypt(cipher, long_key[:R.key_bytes(cipher)], plain, iv=iv[:16])
    wrong_iv = bytes([iv[0] ^ 1]) + iv[1:]
    want = R.decrypt(cipher, long_key, ct, iv=wrong_iv)
    plains, st, _ = dev_decrypt(cipher, long_key, [ct], iv=wrong_iv)
    assert (int(st[0]), plains[0]) == want and plains[0] != plain
    plains, st = C.decrypt_values(cipher, long_key, [ct], iv=wrong_iv)
    assert (int(st[0]), plains[0]) == want


@pytest.mark.gpu
@pytest.mark.parametrize("cipher", CIPHERS)
def test_padding_boundaries(gpu, cipher):
    """Lengths around the block edges, each started at an odd byte offset (and at every offset mod 4), one at a
    time and all in one batch."""
    rng = np.random.default_rng(3)
    values = [rng.bytes(m) for m in (0, 1, 15, 16, 17, 31, 32, 33, 47, 48)]
    for v in values:
        check_both_ways(cipher, KEY, [v], lead=1)
        check_both_ways(cipher, KEY, [v], lead=3)
    for lead in (0, 1, 2, 3, 5):
        check_both_ways(cipher, KEY, values, lead=lead)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("cipher", CIPHERS)
def test_wave_and_workgroup_edges(gpu, cipher, n):
    """Mixed lengths in one wave, batch sizes around the wave (64) and the workgroup (256)."""
    values = state_mix(100 + n, n)
    if n >= 63:
        values[n // 2] = np.random.default_rng(n).bytes(700)  # one long value among short ones, still in place
    check_both_ways(cipher, KEY, values)


@pytest.mark.gpu
@pytest.mark.parametrize("cipher", CIPHERS)
def test_long_value_threshold(gpu, cipher, monkeypatch):
    """A value longer than the threshold leaves the first launch for the long list.  At the shipped threshold
    (1024): one below, at and one above, and a 10,240-byte page, among short values.  Then with the launcher's
    override at 48 bytes, so that most of a batch takes the list, twice on one dirty workspace."""
    import torch
    from bcos_gpu import device
    rng = np.random.default_rng(7)
    short = state_mix(9, 140)
    edge = [rng.bytes(m) for m in (1023, 1024, 1025, 10240)]
    check_both_ways(cipher, KEY, short[:70] + edge + short[70:])
    for v in edge[:3]:
        check_both_ways(cipher, KEY, [v])
    monkeypatch.setenv("BCOSGPU_CIPHER_LONG_BYTES", "48")
    edge = [rng.bytes(m) for m in (47, 48, 49, 64, 10240)]
    first = short[:70] + edge + short[70:]
    second = [rng.bytes(49)] + state_mix(11, 300)
    third = [rng.bytes(int(m)) for m in rng.integers(0, 48, size=90)]  # none listed
    work = torch.full((device.cbc_work_size(301),), 0xFF, dtype=torch.uint8, device="cuda")
    for values in (first, second, third, first):
        check_both_ways(cipher, KEY, values, work=work)


@pytest.mark.gpu
@pytest.mark.parametrize("cipher", CIPHERS)
def test_decrypt_failures(gpu, cipher):
    """A failed item between two good ones: length 17 (the host call), padding byte 0, padding byte 17, a run of
    padding bytes with one wrong; and an empty item (bad length on both paths).  The good items keep their
    plaintext, length and status; the bad item's status is the restatement's."""
    from bcos_gpu import cipher as C
    rng = np.random.default_rng(13)
    c = R.Cipher(cipher, KEY)
    good = [rng.bytes(40), rng.bytes(16)]
    gct = [c.encrypt(v) for v in good]

    def forge(last_block):
        """The ciphertext whose plaintext is 16 random bytes then last_block, with no padding of ours."""
        body = rng.bytes(16) + last_block
        chain, out = c.iv, []
        for j in (0, 16):
            chain = c.enc(bytes(x ^ y for x, y in zip(body[j:j + 16], chain)))
            out.append(chain)
        return b"".join(out)

    bad = {"pad 0": forge(rng.bytes(15) + b"\x00"), "pad 17": forge(rng.bytes(15) + b"\x11"),
           "run broken": forge(rng.bytes(11) + b"\x05\x04\x05\x05\x05"), "whole block": forge(b"\x10" * 16),
           "pad 1": forge(rng.bytes(15) + b"\x01")}
    for name, item in bad.items():
        want_st, want_plain = c.decrypt(item)
        assert want_st == (R.OK if name in ("whole block", "pad 1") else R.BAD_PADDING), name
        plains, st, _ = dev_decrypt(cipher, KEY, [gct[0], item, gct[1]])
        assert plains == [good[0], want_plain, good[1]] and list(st) == [0, want_st, 0], name
        plains, st = C.decrypt_values(cipher, KEY, [gct[0], item, gct[1]])
        assert plains == [good[0], want_plain, good[1]] and list(st) == [0, want_st, 0], name
    for item in (gct[0] + b"\0", b"", gct[0][:15], b"x"):  # 49, 0, 15 and 1 bytes
        plains, st = C.decrypt_values(cipher, KEY, [gct[0], item, gct[1]])
        assert plains == [good[0], b"", good[1]] and list(st) == [0, R.BAD_LENGTH, 0]
    assert R.decrypt(cipher, KEY, gct[0] + b"\0") == (R.BAD_LENGTH, b"")
    plains, st, _ = dev_decrypt(cipher, KEY, [b"", gct[0], b"", b"", gct[1], b""])  # empty items own no lane
    assert plains == [b"", good[0], b"", b"", good[1], b""] and list(st) == [1, 0, 1, 1, 0, 1]
    plains, st, _ = dev_decrypt(cipher, KEY, [b"", b""])
    assert plains == [b"", b""] and list(st) == [1, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("cipher", CIPHERS)
def test_wrong_key(gpu, cipher):
    """A seeded batch decrypted under another key: every status, and the bytes of the items whose padding
    happens to hold, equal the restatement's under that same wrong key."""
    from bcos_gpu import cipher as C
    values = state_mix(17, 700)
    right = R.Cipher(cipher, KEY)
    cts = [right.encrypt(v) for v in values]
    wrong_key = bytes([KEY[0] ^ 1]) + KEY[1:]
    wrong = R.Cipher(cipher, wrong_key)
    want = [wrong.decrypt_raw(ct) for ct in cts]
    plains, st, raw = dev_decrypt(cipher, wrong_key, cts)
    assert list(st) == [w[0] for w in want]
    assert plains == [w[1] for w in want] and raw == [w[2] for w in want]
    assert 0 < sum(w[0] == R.BAD_PADDING for w in want)
    plains, st = C.decrypt_values(cipher, wrong_key, cts)
    assert list(st) == [w[0] for w in want] and plains == [w[1] for w in want]


@pytest.mark.gpu
@pytest.mark.parametrize("cipher", CIPHERS)
def test_round_trip_state_mix(gpu, cipher):
    """4,099 values of the state-root mix: GPU ciphertext == the restatement's, GPU decryption == the input,
    through the device calls and the host calls."""
    check_both_ways(cipher, KEY, state_mix(41, 4099))


@pytest.mark.gpu
def test_decrypt_refuses_equal_buffers(gpu):
    import torch
    from bcos_gpu import BcosGpuError, _lib, device
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 32], dtype=torch.int64, device="cuda")
    with pytest.raises(BcosGpuError) as e:
        device.cbc_decrypt(R.AES256, KEY, d, off, d, torch.zeros(1, dtype=torch.int32, device="cuda"),
                           torch.zeros(1, dtype=torch.uint8, device="cuda"))
    assert e.value.code == _lib.E_ARG


# ---------------------------------------------------------------- the same through C++
def write_fixture(path, values):
    def bs(b):
        return struct.pack("<I", len(b)) + bytes(b)
    key = b"storage data key, longer than thirty-two bytes"
    w = [b"CIPH", bs(key), struct.pack("<I", len(values))]
    for v in values:
        w.append(bs(v))
    for cipher in (R.AES256, R.SM4):
        c = R.Cipher(cipher, key)
        for v in values:
            w.append(bs(c.encrypt(v)))
    with open(path, "wb") as f:
        f.write(b"".join(w))


@pytest.mark.gpu
def test_storage_values_cpp_on_gpu(tmp_path, gpu):
    """encryptStorageValues / decryptStorageValues of include/bcos_gpu.hpp over std::string_views."""
    exe = str(tmp_path / "cipher_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "cipher_test.cpp"), "-L" + LIBDIR, "-lbcosgpu",
                    "-Wl,-rpath," + LIBDIR], check=True)
    fx = str(tmp_path / "cipher.bin")
    write_fixture(fx, state_mix(23, 300) + [np.random.default_rng(1).bytes(5000)])
    r = subprocess.run([exe, fx], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cipher_test: ok" in r.stdout
