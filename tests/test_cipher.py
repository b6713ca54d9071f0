"""The storage cipher's host side (no GPU): the Python restatement (tests/cipher_restatement.py) against OpenSSL's
output (tests/golden/cipher.json) and the standards' vectors, the header csrc/cipher_host.h against the
restatement (through tools/cipher_host_check.cpp), and the C ABI's argument checks, which need no device.

  FIPS-197 C.3                AES-256, one block
  SP 800-38A F.2.5 / F.2.6    CBC-AES256 encrypt / decrypt, four blocks
  GB/T 32907-2016 A.1         SM4, one block
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cipher_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fisco-bcos_amd")
CIPHERS = [pytest.param(R.AES256, id="aes256"), pytest.param(R.SM4, id="sm4")]
NAMES = {R.AES256: "aes256", R.SM4: "sm4"}
h = bytes.fromhex

F25_KEY = h("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4")
F25_IV = h("000102030405060708090a0b0c0d0e0f")
F25_PLAIN = h("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e51"
              "30c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710")
F25_CIPHER = h("f58c4c04d6e5f1ba779eabfb5f7bfbd69cfc4e967edb808d679f777bc6702c7d"
               "39f23369a9d9bacfa530e26304231461b2eb05e2c39be9fcda6c19078c6a9d1b")
# the keys of the schedule comparison: short, exactly 16, exactly 32, and the 69 bytes of EncryptionTest.cpp:73
SCHEDULE_KEYS = [b"abcd", bytes(range(1, 17)), bytes(range(100, 132)), bytes((7 * i + 3) & 0xFF for i in range(69))]


@pytest.fixture(scope="module")
def golden():
    from conftest import load_golden
    return load_golden("cipher.json")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/cipher_host_check.cpp built with the plain host compiler."""
    exe = str(tmp_path_factory.mktemp("cipher") / "cipher_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                    os.path.join(PKG, "tools", "cipher_host_check.cpp"), "-lpthread"], check=True)
    return exe


def test_restatement_reproduces_golden(golden):
    assert len(golden["cases"]) >= 30
    for c in golden["cases"]:
        key, iv, plain, want = (h(c[k]) for k in ("key", "iv", "plain", "cipher_text"))
        assert len(want) == (len(plain) // 16 + 1) * 16
        assert R.encrypt(c["cipher"], key, plain, iv) == want, c["name"]
        assert R.decrypt(c["cipher"], key, want, iv) == (R.OK, plain), c["name"]
        if "published" in c:
            assert want[:len(plain)].hex() == c["published"]


def test_restatement_standard_vectors():
    key = bytes(range(32))  # FIPS-197 C.3
    w = R.aes256_block_keys(key)
    block = h("00112233445566778899aabbccddeeff")
    assert R.aes256_encrypt_block(w, block) == h("8ea2b7ca516745bfeafc49904b496089")
    assert R.aes256_decrypt_block(w, h("8ea2b7ca516745bfeafc49904b496089")) == block
    ct = R.encrypt(R.AES256, F25_KEY, F25_PLAIN, F25_IV)  # SP 800-38A F.2.5: all four blocks, then the padding
    assert ct[:64] == F25_CIPHER and len(ct) == 80
    c = R.Cipher(R.AES256, F25_KEY, F25_IV)  # F.2.6: the four blocks back, with no padding of ours in the way
    st, _, raw = c.decrypt_raw(F25_CIPHER)
    assert raw == F25_PLAIN and st == R.BAD_PADDING  # (its last byte is 0x10 but the run is not)
    assert R.decrypt(R.AES256, F25_KEY, ct, F25_IV) == (R.OK, F25_PLAIN)
    k = h("0123456789abcdeffedcba9876543210")  # GB/T 32907 A.1
    rk = R.sm4_round_keys(k)
    assert R.sm4_crypt_block(rk, k) == h("681edf34d206965e86b3e94f536e4246")
    assert R.sm4_crypt_block(rk[::-1], h("681edf34d206965e86b3e94f536e4246")) == k


def test_restatement_rules():
    """Key cut / zero-filled, explicit IV cut / zero-filled, default IV = the raw key's first 16 bytes."""
    for cipher in (R.AES256, R.SM4):
        K = R.key_bytes(cipher)
        long_key = SCHEDULE_KEYS[3]
        assert R.encrypt(cipher, long_key, b"x" * 20) == R.encrypt(cipher, long_key[:K], b"x" * 20, iv=long_key[:16])
        assert R.encrypt(cipher, b"abcd", b"") == R.encrypt(cipher, b"abcd".ljust(K, b"\0"), b"", iv=b"abcd")
        assert len(R.encrypt(cipher, b"abcd", b"")) == 16 and len(R.encrypt(cipher, b"abcd", bytes(32))) == 48
        iv47 = bytes(range(47))
        assert R.encrypt(cipher, long_key, b"y" * 5, iv=iv47) == R.encrypt(cipher, long_key, b"y" * 5, iv=iv47[:16])
        assert R.decrypt(cipher, b"abcd", b"") == (R.BAD_LENGTH, b"")
        assert R.decrypt(cipher, b"abcd", bytes(17)) == (R.BAD_LENGTH, b"")


def test_host_checker_runs_standard_vectors(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cipher_host_check: ok" in r.stdout


@pytest.mark.parametrize("cipher", CIPHERS)
def test_header_schedules_match_restatement(checker, cipher):
    """The header's encrypt and decrypt schedules and its default IV, word for word, for a short key, keys of
    exactly 16 and 32 bytes and the 69-byte key."""
    for key in SCHEDULE_KEYS:
        k = R.normalise_key(cipher, key)
        if cipher == R.SM4:
            enc = R.sm4_round_keys(k)
            dec = enc[::-1]
            iv = [int.from_bytes(R.normalise_iv(key)[4 * i:4 * i + 4], "big") for i in range(4)]
        else:
            enc, dec = R.aes256_encrypt_schedule_words(k), R.aes256_decrypt_schedule_words(k)
            iv = [int.from_bytes(R.normalise_iv(key)[4 * i:4 * i + 4], "little") for i in range(4)]
        for direction, want in (("enc", enc), ("dec", dec)):
            r = subprocess.run([checker, "schedule", NAMES[cipher], direction, key.hex()], capture_output=True,
                               text=True, check=True)
            words, ivw = r.stdout.split()
            assert words == "".join("%08x" % w for w in want), (len(key), direction)
            assert ivw == "".join("%08x" % w for w in iv), len(key)


@pytest.mark.parametrize("cipher", CIPHERS)
def test_header_cbc_matches_restatement(checker, cipher, golden):
    """The header's CBC over whole values: the golden cases, and the decrypt statuses of damaged input."""
    for c in golden["cases"]:
        if c["cipher"] != cipher:
            continue
        r = subprocess.run([checker, "cbc", NAMES[cipher], "enc", c["key"], c["iv"], c["plain"]],
                           capture_output=True, text=True, check=True)
        assert r.stdout.split() == ["0", c["cipher_text"]], c["name"]
        r = subprocess.run([checker, "cbc", NAMES[cipher], "dec", c["key"], c["iv"], c["cipher_text"]],
                           capture_output=True, text=True, check=True)
        assert r.stdout.split() == (["0", c["plain"]] if c["plain"] else ["0"]), c["name"]
    rng = np.random.default_rng(5)
    key = b"abcd"
    ct = R.encrypt(cipher, key, rng.bytes(40))
    for bad in (ct[:-1], ct + b"\0", bytes([ct[0] ^ 1]) + ct[1:], ct[:32] + bytes([ct[32] ^ 0x80]) + ct[33:],
                rng.bytes(48)):
        st, plain = R.decrypt(cipher, key, bad)
        r = subprocess.run([checker, "cbc", NAMES[cipher], "dec", key.hex(), "-", bad.hex()], capture_output=True,
                           text=True, check=True)
        assert r.stdout.split() == ([str(st), plain.hex()] if plain else [str(st)])


def test_abi_argument_checks_need_no_device():
    """BCOSGPU_E_ARG for an unknown cipher, a null pointer with a non-zero length and a cap that is too small,
    all before any device is touched; n == 0 succeeds and writes nothing."""
    from bcos_gpu import _lib, cipher
    L = _lib.lib()
    assert L.bcosgpu_cbc_padded_size(0) == 16 and L.bcosgpu_cbc_padded_size(15) == 16
    assert L.bcosgpu_cbc_padded_size(16) == 32 and L.bcosgpu_cbc_padded_size(32) == 48
    assert L.bcosgpu_cbc_work_size(1000) >= 8 * 4 + 4 * 1000 and L.bcosgpu_cbc_work_size(1000) % 8 == 0
    key = bytes(32)
    views, keep = cipher._views([b"hello", b"", b"x" * 40])
    out = np.full(256, 0xAA, dtype=np.uint8)
    off = np.full(4, 0xAAAAAAAA, dtype=np.uint64)
    status = np.full(3, 0xAA, dtype=np.uint8)
    po, pf, ps = out.ctypes.data, off.ctypes.data, status.ctypes.data
    enc, dec = L.bcosgpu_cbc_encrypt_batch, L.bcosgpu_cbc_decrypt_batch
    for bad_cipher in (2, -1):
        assert enc(bad_cipher, key, 32, None, 0, views, 3, po, 256, pf) == _lib.E_ARG
        assert dec(bad_cipher, key, 32, None, 0, views, 3, po, 256, pf, ps) == _lib.E_ARG
        assert L.bcosgpu_cbc_encrypt_batch_dev(bad_cipher, key, 32, None, 0, 16, 16, 1, 16, 16, 16, 1 << 20,
                                               None) == _lib.E_ARG
        assert L.bcosgpu_cbc_decrypt_batch_dev(bad_cipher, key, 32, None, 0, 16, 16, 1, 32, 16, 16, None) == _lib.E_ARG
    assert enc(0, None, 4, None, 0, views, 3, po, 256, pf) == _lib.E_ARG  # a null key with a length
    assert enc(0, key, 32, None, 7, views, 3, po, 256, pf) == _lib.E_ARG  # a null iv with a length
    assert enc(0, key, 32, None, 0, None, 3, po, 256, pf) == _lib.E_ARG  # null views
    assert enc(1, key, 32, None, 0, views, 3, po, 16 + 16 + 48 - 1, pf) == _lib.E_ARG  # cap one byte short
    assert enc(1, key, 32, None, 0, views, 3, None, 256, pf) == _lib.E_ARG
    assert dec(1, key, 32, None, 0, views, 3, po, 256, None, ps) == _lib.E_ARG
    null = (cipher._BytesView * 1)()
    null[0].len = 3  # a null value with a length
    assert enc(0, key, 32, None, 0, null, 1, po, 256, pf) == _lib.E_ARG
    assert dec(0, key, 32, None, 0, null, 1, po, 256, pf, ps) == _lib.E_ARG
    big = (cipher._BytesView * 1)()
    buf = ctypes.create_string_buffer(8)
    big[0].data, big[0].len = ctypes.cast(buf, ctypes.c_char_p), 1 << 32  # 2^32 bytes: refused before it is read
    assert enc(0, key, 32, None, 0, big, 1, po, 1 << 40, pf) == _lib.E_ARG
    cts, keep2 = cipher._views([bytes(32), bytes(16)])
    assert dec(0, key, 32, None, 0, cts, 2, po, 47, pf, ps) == _lib.E_ARG  # cap below the well-formed items' bytes
    # the device calls: a null pointer, equal input and output, a misaligned output, a short work buffer
    encd, decd = L.bcosgpu_cbc_encrypt_batch_dev, L.bcosgpu_cbc_decrypt_batch_dev
    assert encd(0, key, 32, None, 0, None, 16, 1, 16, 16, 16, 1 << 20, None) == _lib.E_ARG
    assert encd(0, key, 32, None, 0, 16, 16, 1, 24, 16, 16, 1 << 20, None) == _lib.E_ARG
    assert encd(0, key, 32, None, 0, 16, 16, 1, 16, 16, 16, L.bcosgpu_cbc_work_size(1) - 1, None) == _lib.E_ARG
    assert decd(0, key, 32, None, 0, 4096, 16, 1, 4096, 16, 16, None) == _lib.E_ARG
    assert decd(0, key, 32, None, 0, 4096, 16, 1, 8200, 16, 16, None) == _lib.E_ARG
    assert decd(0, key, 32, None, 0, 4096, 16, 1, 8192, None, 16, None) == _lib.E_ARG
    # n == 0: success, nothing written, no device needed
    assert enc(0, key, 32, None, 0, None, 0, None, 0, None) == _lib.OK
    assert dec(1, key, 32, None, 0, None, 0, None, 0, None, None) == _lib.OK
    assert encd(0, key, 32, None, 0, None, None, 0, None, None, None, 0, None) == _lib.OK
    assert decd(1, key, 32, None, 0, None, None, 0, None, None, None, None) == _lib.OK
    assert (out == 0xAA).all() and (off == 0xAAAAAAAA).all() and (status == 0xAA).all()
    # ... and a decrypt batch with no well-formed item is answered on the host
    odd, keep3 = cipher._views([b"", bytes(17)])
    assert dec(0, key, 32, None, 0, odd, 2, None, 0, pf, ps) == _lib.OK
    assert list(status[:2]) == [_lib.CBC_E_LENGTH] * 2 and list(off[:3]) == [0, 0, 0]
    del keep, keep2, keep3
