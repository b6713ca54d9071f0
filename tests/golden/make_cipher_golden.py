#!/usr/bin/env python3
"""Generates tests/golden/cipher.json.  Run in the build container only.

AES-256-CBC and SM4-CBC ciphertexts computed by OpenSSL 1.1.1 (EVP_aes_256_cbc / EVP_sm4_cbc through ctypes),
with PKCS#7 padding, over keys and IVs that already have their full length: the standards' vectors (FIPS-197
C.3, SP 800-38A F.2.5, GB/T 32907 A.1) and seeded cases.  OpenSSL reproduces the published ciphertexts of
those vectors; that is asserted here before anything is written.  The file is data only.
"""
import ctypes
import ctypes.util
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
AES256, SM4 = 0, 1


def _libcrypto():
    for name in ("/opt/conda/lib/libcrypto.so.1.1", "libcrypto.so.1.1", ctypes.util.find_library("crypto")):
        try:
            L = ctypes.CDLL(name)
        except (OSError, TypeError):
            continue
        if hasattr(L, "EVP_sm4_cbc"):
            return L
    raise SystemExit("no libcrypto with EVP_sm4_cbc found")


L = _libcrypto()
for fn in ("EVP_CIPHER_CTX_new", "EVP_aes_256_cbc", "EVP_sm4_cbc"):
    getattr(L, fn).restype = ctypes.c_void_p
L.EVP_EncryptInit_ex.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_char_p, ctypes.c_char_p]
L.EVP_EncryptUpdate.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p,
                                ctypes.c_int]
L.EVP_EncryptFinal_ex.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
L.EVP_CIPHER_CTX_free.argtypes = [ctypes.c_void_p]


def evp_encrypt(cipher, key, iv, data):
    assert len(key) == (16 if cipher == SM4 else 32) and len(iv) == 16
    ctx = L.EVP_CIPHER_CTX_new()
    evp = L.EVP_sm4_cbc() if cipher == SM4 else L.EVP_aes_256_cbc()
    assert L.EVP_EncryptInit_ex(ctx, evp, None, key, iv) == 1
    out = ctypes.create_string_buffer(len(data) + 32)
    n, m = ctypes.c_int(0), ctypes.c_int(0)
    assert L.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), data, len(data)) == 1
    tail = ctypes.create_string_buffer(32)
    assert L.EVP_EncryptFinal_ex(ctx, tail, ctypes.byref(m)) == 1
    L.EVP_CIPHER_CTX_free(ctx)
    return out.raw[:n.value] + tail.raw[:m.value]


def main():
    h = bytes.fromhex
    std = [
        ("FIPS-197 C.3 (one block, zero IV)", AES256,
         h("000102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f"), bytes(16),
         h("00112233445566778899aabbccddeeff"), "8ea2b7ca516745bfeafc49904b496089"),
        ("SP 800-38A F.2.5", AES256, h("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4"),
         h("000102030405060708090a0b0c0d0e0f"),
         h("6bc1bee22e409f96e93d7e117393172aae2d8a571e03ac9c9eb76fac45af8e51"
           "30c81c46a35ce411e5fbc1191a0a52eff69f2445df4f9b17ad2b417be66c3710"),
         "f58c4c04d6e5f1ba779eabfb5f7bfbd69cfc4e967edb808d679f777bc6702c7d"
         "39f23369a9d9bacfa530e26304231461b2eb05e2c39be9fcda6c19078c6a9d1b"),
        ("GB/T 32907 A.1 (one block, zero IV)", SM4, h("0123456789abcdeffedcba9876543210"), bytes(16),
         h("0123456789abcdeffedcba9876543210"), "681edf34d206965e86b3e94f536e4246"),
    ]
    cases = []
    for name, cipher, key, iv, pt, want in std:
        ct = evp_encrypt(cipher, key, iv, pt)
        assert ct[:len(pt)].hex() == want, name  # the published ciphertext, then the padding block
        assert len(ct) == len(pt) + 16
        cases.append({"name": name, "cipher": cipher, "key": key.hex(), "iv": iv.hex(), "plain": pt.hex(),
                      "published": want, "cipher_text": ct.hex()})
    assert len(evp_encrypt(AES256, bytes(32), bytes(16), bytes(32))) == 48
    assert len(evp_encrypt(SM4, bytes(16), bytes(16), b"")) == 16
    rng = random.Random(20240517)
    lengths = [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 100, 255, 256, 300, 1000]
    for cipher in (AES256, SM4):
        for n in lengths:
            key = bytes(rng.getrandbits(8) for _ in range(16 if cipher == SM4 else 32))
            iv = bytes(rng.getrandbits(8) for _ in range(16))
            pt = bytes(rng.getrandbits(8) for _ in range(n))
            ct = evp_encrypt(cipher, key, iv, pt)
            assert len(ct) == (n // 16 + 1) * 16
            cases.append({"name": "seeded %d" % n, "cipher": cipher, "key": key.hex(), "iv": iv.hex(),
                          "plain": pt.hex(), "cipher_text": ct.hex()})
    with open(os.path.join(HERE, "cipher.json"), "w") as f:
        json.dump({"source": "OpenSSL 1.1.1 EVP_aes_256_cbc / EVP_sm4_cbc, PKCS#7", "cases": cases}, f, indent=1)
    print("cipher.json: %d cases" % len(cases))


if __name__ == "__main__":
    main()
