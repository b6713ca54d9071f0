"""A pure-Python AES-256-CBC and SM4-CBC with the storage cipher's key, IV and padding rules: the restatement
the cipher tests compare the header (csrc/cipher_host.h) and the kernels (csrc/cipher_kernels.hip) against.

Written from FIPS-197 (SubBytes / ShiftRows / MixColumns on a byte state; the only tables are the S-box and the
GF(2^8) multiples MixColumns needs) and GB/T 32907-2016, so it shares no structure with the word-table code it
checks.  The rules (see cipher_host.h):

  key      first min(len, K) bytes, zero-filled to K; K = 32 (AES-256), 16 (SM4)
  iv       explicit: first min(len, 16) bytes, zero-filled; default (iv=None): first 16 bytes of the RAW key,
           zero-filled where the key is shorter (the build's stated deviation from the reference's over-read)
  mode     CBC, PKCS#7: len bytes -> (len // 16 + 1) * 16
  decrypt  status 1 for a length that is zero or no multiple of 16, 2 for bad padding, else 0
"""
AES256, SM4 = 0, 1
OK, BAD_LENGTH, BAD_PADDING = 0, 1, 2


# ---------------------------------------------------------------- AES (FIPS-197)
def _xtime(a):
    a <<= 1
    return (a ^ 0x11B) & 0xFF if a & 0x100 else a


def _gmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a = _xtime(a)
        b >>= 1
    return r


def _aes_sbox():
    inv = [0] * 256
    for a in range(1, 256):
        for b in range(1, 256):
            if _gmul(a, b) == 1:
                inv[a] = b
                break
    box = []
    for a in range(256):
        x = inv[a]
        s = x
        for k in range(1, 5):
            s ^= ((x << k) | (x >> (8 - k))) & 0xFF
        box.append(s ^ 0x63)
    return box


AES_SBOX = _aes_sbox()
AES_INV_SBOX = [AES_SBOX.index(a) for a in range(256)]


def aes256_round_keys(key32):
    """FIPS-197 5.2: 60 words as 4-byte lists."""
    w = [list(key32[4 * i:4 * i + 4]) for i in range(8)]
    rcon = 1
    for i in range(8, 60):
        t = list(w[i - 1])
        if i % 8 == 0:
            t = [AES_SBOX[b] for b in t[1:] + t[:1]]
            t[0] ^= rcon
            rcon = _xtime(rcon)
        elif i % 8 == 4:
            t = [AES_SBOX[b] for b in t]
        w.append([a ^ b for a, b in zip(w[i - 8], t)])
    return w


def aes256_block_keys(key32):
    """The 15 round keys as 16-byte lists in state order (byte i = row i % 4 of column i // 4)."""
    w = aes256_round_keys(key32)
    return [[b for col in w[4 * r:4 * r + 4] for b in col] for r in range(15)]


# ShiftRows as a gather: row r moves left by r, so out[4c + r] = in[4 * ((c + r) % 4) + r]; the inverse moves right
_SHIFT = [4 * ((c + r) % 4) + r for c in range(4) for r in range(4)]
_UNSHIFT = [4 * ((c - r) % 4) + r for c in range(4) for r in range(4)]
_MUL = {c: [_gmul(x, c) for x in range(256)] for c in (1, 2, 3, 9, 11, 13, 14)}  # x -> c * x in GF(2^8)


# row r of the (Inv)MixColumns matrix is its first row m rotated right by r
_ROWS = {m: [[_MUL[m[(j - r) % 4]] for j in range(4)] for r in range(4)] for m in ((2, 3, 1, 1), (14, 11, 13, 9))}


def _mix_columns(s, m):
    rows = _ROWS[m]
    out = []
    for c in range(4):
        c0, c1, c2, c3 = s[4 * c:4 * c + 4]
        for t0, t1, t2, t3 in rows:
            out.append(t0[c0] ^ t1[c1] ^ t2[c2] ^ t3[c3])
    return out


def _xor(a, b):
    return [x ^ y for x, y in zip(a, b)]


def aes256_encrypt_block(keys, block):
    """FIPS-197 5.1 (keys: aes256_block_keys)."""
    s = _xor(block, keys[0])
    for r in range(1, 14):
        s = _xor(_mix_columns([AES_SBOX[s[i]] for i in _SHIFT], (2, 3, 1, 1)), keys[r])
    return bytes(_xor([AES_SBOX[s[i]] for i in _SHIFT], keys[14]))


def aes256_decrypt_block(keys, block):
    """FIPS-197 5.3: the straightforward inverse cipher (not the equivalent one the header uses)."""
    s = _xor(block, keys[14])
    for r in range(13, 0, -1):
        s = _mix_columns(_xor([AES_INV_SBOX[s[i]] for i in _UNSHIFT], keys[r]), (14, 11, 13, 9))
    return bytes(_xor([AES_INV_SBOX[s[i]] for i in _UNSHIFT], keys[0]))


def aes256_decrypt_schedule_words(key32):
    """The equivalent inverse cipher's schedule (FIPS-197 5.3.5) as 60 little-endian-column words: what the
    header's aes256_decrypt_schedule gives."""
    w = aes256_round_keys(key32)
    out = []
    for r in range(15):
        for c in range(4):
            col = w[4 * (14 - r) + c]
            if 0 < r < 14:
                col = _mix_columns(col + [0] * 12, (14, 11, 13, 9))[:4]
            out.append(int.from_bytes(bytes(col), "little"))
    return out


def aes256_encrypt_schedule_words(key32):
    return [int.from_bytes(bytes(c), "little") for c in aes256_round_keys(key32)]


# ---------------------------------------------------------------- SM4 (GB/T 32907-2016)
SM4_SBOX = bytes.fromhex(
    "d690e9fecce13db716b614c228fb2c052b679a762abe04c3aa441326498606999c4250f491ef987a33540b43edcfac62"
    "e4b31ca9c908e89580df94fa758f3fa64707a7fcf37317ba83593c19e6854fa8686b81b27164da8bf8eb0f4b70569d35"
    "1e240e5e6358d1a225227c3b01217887d40046579fd327524c3602e7a0c4c89eeabf8ad240c738b5a3f7f2cef96115a1"
    "e0ae5da49b341a55ad933230f58cb1e31df6e22e8266ca60c02923ab0d534e6fd5db3745defd8e2f03ff6a726d6c5b51"
    "8d1baf92bbddbc7f11d95c411f105ad80ac13188a5cd7bbd2d74d012b8e5b4b08969974a0c96777e65b9f109c56ec684"
    "18f07dec3adc4d2079ee5f3ed7cb3948")
SM4_FK = (0xA3B1BAC6, 0x56AA3350, 0x677D9197, 0xB27022DC)
SM4_CK = [sum((((4 * i + j) * 7) & 0xFF) << (24 - 8 * j) for j in range(4)) for i in range(32)]


def _rol(x, r):
    return ((x << r) | (x >> (32 - r))) & 0xFFFFFFFF


def _tau(x):
    return int.from_bytes(bytes(SM4_SBOX[b] for b in x.to_bytes(4, "big")), "big")


def sm4_round_keys(key16):
    k = [int.from_bytes(key16[4 * i:4 * i + 4], "big") ^ SM4_FK[i] for i in range(4)]
    rk = []
    for i in range(32):
        b = _tau(k[1] ^ k[2] ^ k[3] ^ SM4_CK[i])
        rk.append(k[0] ^ b ^ _rol(b, 13) ^ _rol(b, 23))
        k = k[1:] + [rk[-1]]
    return rk


def sm4_crypt_block(rk, block):
    x = [int.from_bytes(block[4 * i:4 * i + 4], "big") for i in range(4)]
    for i in range(32):
        b = _tau(x[1] ^ x[2] ^ x[3] ^ rk[i])
        x = x[1:] + [x[0] ^ b ^ _rol(b, 2) ^ _rol(b, 10) ^ _rol(b, 18) ^ _rol(b, 24)]
    return b"".join(v.to_bytes(4, "big") for v in reversed(x))


# ---------------------------------------------------------------- the storage cipher's rules
def key_bytes(cipher):
    return 16 if cipher == SM4 else 32


def normalise_key(cipher, key):
    k = key_bytes(cipher)
    return bytes(key[:k]).ljust(k, b"\0")


def normalise_iv(key, iv=None):
    return bytes((key if iv is None else iv)[:16]).ljust(16, b"\0")


def _block_fns(cipher, key):
    k = normalise_key(cipher, key)
    if cipher == SM4:
        rk = sm4_round_keys(k)
        back = rk[::-1]
        return (lambda b: sm4_crypt_block(rk, b)), (lambda b: sm4_crypt_block(back, b))
    keys = aes256_block_keys(k)
    return (lambda b: aes256_encrypt_block(keys, b)), (lambda b: aes256_decrypt_block(keys, b))


def _xor16(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


class Cipher:
    """One cipher under one key and IV (iv=None: the default IV); the key schedule is computed once."""

    def __init__(self, cipher, key, iv=None):
        self.enc, self.dec = _block_fns(cipher, key)
        self.iv = normalise_iv(key, iv)

    def encrypt(self, data):
        pad = 16 - len(data) % 16
        data = bytes(data) + bytes([pad]) * pad
        out, chain = [], self.iv
        for j in range(0, len(data), 16):
            chain = self.enc(_xor16(data[j:j + 16], chain))
            out.append(chain)
        return b"".join(out)

    def decrypt_raw(self, data):
        """(status, plaintext, the blocks as decrypted with the padding still on)."""
        if len(data) == 0 or len(data) % 16:
            return BAD_LENGTH, b"", b""
        out, chain = [], self.iv
        for j in range(0, len(data), 16):
            out.append(_xor16(self.dec(data[j:j + 16]), chain))
            chain = data[j:j + 16]
        raw = b"".join(out)
        p = raw[-1]
        if p < 1 or p > 16 or raw[-p:] != bytes([p]) * p:
            return BAD_PADDING, b"", raw
        return OK, raw[:-p], raw

    def decrypt(self, data):
        st, plain, _ = self.decrypt_raw(data)
        return st, plain


def encrypt(cipher, key, data, iv=None):
    return Cipher(cipher, key, iv).encrypt(data)


def decrypt(cipher, key, data, iv=None):
    return Cipher(cipher, key, iv).decrypt(data)
