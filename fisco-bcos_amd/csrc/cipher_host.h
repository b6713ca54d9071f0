// cipher_host.h -- the host side of the storage cipher (AES-256-CBC and SM4-CBC over storage values): key and
// IV normalisation, the key schedules, a single-block encrypt / decrypt per cipher, CBC with PKCS#7 over one
// value, and the generators of the lookup tables the kernels copy into LDS (cipher_kernels.hip).
// Host-only C++17, no device code and no HIP (tools/cipher_host_check.cpp builds it with a plain compiler).
//
// What it restates (the reference's third CryptoSuite member, SymmetricEncryption):
//   DataEncryption::encrypt / decrypt     bcos-security/bcos-security/DataEncryption.cpp:143-165
//     symmetricEncrypt(data, size, key, keySize) -- the two-argument form
//   AESCrypto / SM4Crypto                 bcos-crypto/bcos-crypto/encrypt/AESCrypto.cpp:29-51, SM4Crypto.cpp:28-49
//   Key        the first min(key_len, K) bytes of the caller's key, zero-filled to K; K = 32 (AES), 16 (SM4)
//              (FixedBytes(byte const*, size_t), bcos-utilities/bcos-utilities/FixedBytes.h:173-176;
//              AESCrypto.cpp:34, SM4Crypto.cpp:33).  A longer key is cut (EncryptionTest.cpp:73 passes 69 bytes).
//   IV         explicit: the first min(iv_len, 16) bytes, zero-filled to 16 (AESCrypto.cpp:37, SM4Crypto.cpp:36).
//              default (the two-argument form, AESCrypto.h:41-51, SM4Crypto.h:41-50): the key pointer with
//              length 16, i.e. the first 16 bytes of the RAW key.
//              STATED DEVIATION: with a key shorter than 16 bytes the reference reads past the end of the
//              caller's buffer (the key "abcd" of EncryptionTest.cpp:38 does); this build zero-fills instead.
//   Mode       CBC with PKCS#7 padding: len bytes become (len / 16 + 1) * 16, an empty value one block.  The
//              reference sizes its buffer len + 26 and shrinks it to what wedpr reports (AESCrypto.cpp:41-49).
//   Decrypt    fails (DecryptException, AESCrypto.cpp:69-72) for a length that is zero or no multiple of 16,
//              and for a last plaintext byte p outside 1..16 or last p bytes that are not all p.
//   Parity unpinned: mode and padding live in wedpr (Rust), which is not built here; the reference's only test
//   is a round trip (EncryptionTest.cpp:35-92).  The ciphers are pinned by FIPS-197 C.3, SP 800-38A F.2.5 /
//   F.2.6 and GB/T 32907 A.1.
//
// Word conventions (the kernels share them): an AES column is a little-endian word (row 0 in the low byte),
// so a block is four plain dword loads; an SM4 word is big-endian, as the standard writes it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace bcosgpu {
namespace cipher {

constexpr int kAes256 = 0, kSm4 = 1;  // BCOSGPU_CIPHER_AES256 / BCOSGPU_CIPHER_SM4
constexpr int kAesRounds = 14, kAesWords = 60, kSm4Words = 32;
constexpr int kStatusOk = 0, kStatusBadLength = 1, kStatusBadPadding = 2;

struct ByteTable {
    uint8_t v[256];
};
struct WordTable {
    uint32_t v[256];
};

constexpr uint32_t rotl32(uint32_t x, int r) { return r ? (x << r) | (x >> (32 - r)) : x; }
constexpr uint32_t rotr32(uint32_t x, int r) { return r ? (x >> r) | (x << (32 - r)) : x; }

// ------------------------------------------------------------------ AES tables (FIPS-197 4.2, 5.1.1)
constexpr uint8_t gf_mul(uint8_t a, uint8_t b) {  // in GF(2^8) mod x^8 + x^4 + x^3 + x + 1
    uint8_t r = 0;
    for (int i = 0; i < 8; ++i) {
        if (b & 1) r ^= a;
        a = static_cast<uint8_t>((a << 1) ^ ((a & 0x80) ? 0x1b : 0));
        b >>= 1;
    }
    return r;
}

constexpr ByteTable aes_sbox() {  // the inverse in GF(2^8), then the affine map with 0x63
    ByteTable t{};
    uint8_t exp[256] = {}, log[256] = {};
    uint8_t x = 1;
    for (int i = 0; i < 255; ++i) {  // powers of the generator 3
        exp[i] = x;
        log[x] = static_cast<uint8_t>(i);
        x = static_cast<uint8_t>(x ^ gf_mul(x, 2));
    }
    for (int a = 0; a < 256; ++a) {
        const uint8_t inv = a ? exp[(255 - log[a]) % 255] : 0;
        uint8_t s = inv;
        for (int k = 1; k <= 4; ++k) s ^= static_cast<uint8_t>((inv << k) | (inv >> (8 - k)));
        t.v[a] = static_cast<uint8_t>(s ^ 0x63);
    }
    return t;
}

constexpr ByteTable invert(const ByteTable& s) {
    ByteTable t{};
    for (int a = 0; a < 256; ++a) t.v[s.v[a]] = static_cast<uint8_t>(a);
    return t;
}
constexpr ByteTable aes_inv_sbox() { return invert(aes_sbox()); }

constexpr bool is_permutation(const ByteTable& s) {
    bool seen[256] = {};
    for (int a = 0; a < 256; ++a) {
        if (seen[s.v[a]]) return false;
        seen[s.v[a]] = true;
    }
    return true;
}

// Te0[x]: the MixColumns column of S[x] in row 0, (2s, s, s, 3s) from the low byte up.  The tables of rows
// 1..3 are Te0 rotated left by 8, 16, 24; byte 1 of Te0[x] is the plain S[x] the last round needs.
constexpr WordTable aes_te0() {
    const ByteTable s = aes_sbox();
    WordTable t{};
    for (int a = 0; a < 256; ++a) {
        const uint32_t v = s.v[a];
        t.v[a] = gf_mul(s.v[a], 2) | (v << 8) | (v << 16) | (static_cast<uint32_t>(gf_mul(s.v[a], 3)) << 24);
    }
    return t;
}
// Td0[x]: the InvMixColumns column of InvS[x] in row 0, (14i, 9i, 13i, 11i) from the low byte up.
constexpr WordTable aes_td0() {
    const ByteTable s = aes_inv_sbox();
    WordTable t{};
    for (int a = 0; a < 256; ++a) {
        const uint8_t i = s.v[a];
        t.v[a] = gf_mul(i, 14) | (static_cast<uint32_t>(gf_mul(i, 9)) << 8) |
                 (static_cast<uint32_t>(gf_mul(i, 13)) << 16) | (static_cast<uint32_t>(gf_mul(i, 11)) << 24);
    }
    return t;
}

// ------------------------------------------------------------------ SM4 tables (GB/T 32907-2016 6.2)
constexpr ByteTable sm4_sbox() {  // typed from the standard's table; checked to be a permutation below
    return ByteTable{{
        0xd6, 0x90, 0xe9, 0xfe, 0xcc, 0xe1, 0x3d, 0xb7, 0x16, 0xb6, 0x14, 0xc2, 0x28, 0xfb, 0x2c, 0x05,
        0x2b, 0x67, 0x9a, 0x76, 0x2a, 0xbe, 0x04, 0xc3, 0xaa, 0x44, 0x13, 0x26, 0x49, 0x86, 0x06, 0x99,
        0x9c, 0x42, 0x50, 0xf4, 0x91, 0xef, 0x98, 0x7a, 0x33, 0x54, 0x0b, 0x43, 0xed, 0xcf, 0xac, 0x62,
        0xe4, 0xb3, 0x1c, 0xa9, 0xc9, 0x08, 0xe8, 0x95, 0x80, 0xdf, 0x94, 0xfa, 0x75, 0x8f, 0x3f, 0xa6,
        0x47, 0x07, 0xa7, 0xfc, 0xf3, 0x73, 0x17, 0xba, 0x83, 0x59, 0x3c, 0x19, 0xe6, 0x85, 0x4f, 0xa8,
        0x68, 0x6b, 0x81, 0xb2, 0x71, 0x64, 0xda, 0x8b, 0xf8, 0xeb, 0x0f, 0x4b, 0x70, 0x56, 0x9d, 0x35,
        0x1e, 0x24, 0x0e, 0x5e, 0x63, 0x58, 0xd1, 0xa2, 0x25, 0x22, 0x7c, 0x3b, 0x01, 0x21, 0x78, 0x87,
        0xd4, 0x00, 0x46, 0x57, 0x9f, 0xd3, 0x27, 0x52, 0x4c, 0x36, 0x02, 0xe7, 0xa0, 0xc4, 0xc8, 0x9e,
        0xea, 0xbf, 0x8a, 0xd2, 0x40, 0xc7, 0x38, 0xb5, 0xa3, 0xf7, 0xf2, 0xce, 0xf9, 0x61, 0x15, 0xa1,
        0xe0, 0xae, 0x5d, 0xa4, 0x9b, 0x34, 0x1a, 0x55, 0xad, 0x93, 0x32, 0x30, 0xf5, 0x8c, 0xb1, 0xe3,
        0x1d, 0xf6, 0xe2, 0x2e, 0x82, 0x66, 0xca, 0x60, 0xc0, 0x29, 0x23, 0xab, 0x0d, 0x53, 0x4e, 0x6f,
        0xd5, 0xdb, 0x37, 0x45, 0xde, 0xfd, 0x8e, 0x2f, 0x03, 0xff, 0x6a, 0x72, 0x6d, 0x6c, 0x5b, 0x51,
        0x8d, 0x1b, 0xaf, 0x92, 0xbb, 0xdd, 0xbc, 0x7f, 0x11, 0xd9, 0x5c, 0x41, 0x1f, 0x10, 0x5a, 0xd8,
        0x0a, 0xc1, 0x31, 0x88, 0xa5, 0xcd, 0x7b, 0xbd, 0x2d, 0x74, 0xd0, 0x12, 0xb8, 0xe5, 0xb4, 0xb0,
        0x89, 0x69, 0x97, 0x4a, 0x0c, 0x96, 0x77, 0x7e, 0x65, 0xb9, 0xf1, 0x09, 0xc5, 0x6e, 0xc6, 0x84,
        0x18, 0xf0, 0x7d, 0xec, 0x3a, 0xdc, 0x4d, 0x20, 0x79, 0xee, 0x5f, 0x3e, 0xd7, 0xcb, 0x39, 0x48}};
}

constexpr uint32_t sm4_L(uint32_t b) { return b ^ rotl32(b, 2) ^ rotl32(b, 10) ^ rotl32(b, 18) ^ rotl32(b, 24); }
constexpr uint32_t sm4_Lkey(uint32_t b) { return b ^ rotl32(b, 13) ^ rotl32(b, 23); }

// T0[x] = L(S[x] << 24): the round transform of the top byte.  L commutes with rotation, so the byte k
// places lower takes T0 rotated right by 8k.
constexpr WordTable sm4_t0() {
    const ByteTable s = sm4_sbox();
    WordTable t{};
    for (int a = 0; a < 256; ++a) t.v[a] = sm4_L(static_cast<uint32_t>(s.v[a]) << 24);
    return t;
}

inline constexpr ByteTable kAesSbox = aes_sbox();
inline constexpr ByteTable kAesInvSbox = aes_inv_sbox();
inline constexpr WordTable kAesTe0 = aes_te0();
inline constexpr WordTable kAesTd0 = aes_td0();
inline constexpr ByteTable kSm4Sbox = sm4_sbox();
inline constexpr WordTable kSm4T0 = sm4_t0();
static_assert(kAesSbox.v[0x00] == 0x63 && kAesSbox.v[0x53] == 0xed, "FIPS-197 figure 7");
static_assert(is_permutation(kAesSbox) && is_permutation(kSm4Sbox), "an S-box is a permutation");

// ------------------------------------------------------------------ key and IV
inline int key_bytes(int cipher) { return cipher == kSm4 ? 16 : 32; }

// the first min(key_len, K) bytes, zero-filled to K (out32: K bytes are written, the rest zeroed)
inline void normalise_key(int cipher, const uint8_t* key, size_t key_len, uint8_t out32[32]) {
    const size_t k = static_cast<size_t>(key_bytes(cipher)), m = key_len < k ? key_len : k;
    memset(out32, 0, 32);
    if (m) memcpy(out32, key, m);
}

// iv != null: its first min(iv_len, 16) bytes, zero-filled; iv == null: the default IV, the first 16 bytes of
// the raw key, zero-filled where the key is shorter (the stated deviation above)
inline void normalise_iv(const uint8_t* key, size_t key_len, const uint8_t* iv, size_t iv_len, uint8_t out16[16]) {
    const uint8_t* src = iv ? iv : key;
    const size_t len = iv ? iv_len : key_len, m = len < 16 ? len : 16;
    memset(out16, 0, 16);
    if (m) memcpy(out16, src, m);
}

inline uint32_t load_le32(const uint8_t* p) {
    return p[0] | (static_cast<uint32_t>(p[1]) << 8) | (static_cast<uint32_t>(p[2]) << 16) |
           (static_cast<uint32_t>(p[3]) << 24);
}
inline uint32_t load_be32(const uint8_t* p) {
    return p[3] | (static_cast<uint32_t>(p[2]) << 8) | (static_cast<uint32_t>(p[1]) << 16) |
           (static_cast<uint32_t>(p[0]) << 24);
}
inline void store_le32(uint8_t* p, uint32_t w) {
    p[0] = static_cast<uint8_t>(w), p[1] = static_cast<uint8_t>(w >> 8), p[2] = static_cast<uint8_t>(w >> 16),
    p[3] = static_cast<uint8_t>(w >> 24);
}
inline void store_be32(uint8_t* p, uint32_t w) {
    p[3] = static_cast<uint8_t>(w), p[2] = static_cast<uint8_t>(w >> 8), p[1] = static_cast<uint8_t>(w >> 16),
    p[0] = static_cast<uint8_t>(w >> 24);
}

// ------------------------------------------------------------------ AES-256 (FIPS-197 5.2, 5.3.5)
inline uint32_t aes_sub_word(uint32_t w) {
    return kAesSbox.v[w & 0xff] | (static_cast<uint32_t>(kAesSbox.v[(w >> 8) & 0xff]) << 8) |
           (static_cast<uint32_t>(kAesSbox.v[(w >> 16) & 0xff]) << 16) |
           (static_cast<uint32_t>(kAesSbox.v[w >> 24]) << 24);
}

// the 60 words of the encryption schedule, columns as little-endian words
inline void aes256_expand_key(const uint8_t key32[32], uint32_t rk[kAesWords]) {
    for (int i = 0; i < 8; ++i) rk[i] = load_le32(key32 + 4 * i);
    uint8_t rcon = 1;
    for (int i = 8; i < kAesWords; ++i) {
        uint32_t t = rk[i - 1];
        if (i % 8 == 0) {
            t = aes_sub_word(rotr32(t, 8)) ^ rcon;  // RotWord moves byte 1 to byte 0: a right rotation here
            rcon = gf_mul(rcon, 2);
        } else if (i % 8 == 4) {
            t = aes_sub_word(t);
        }
        rk[i] = rk[i - 8] ^ t;
    }
}

inline uint32_t aes_inv_mix_column(uint32_t w) {
    return kAesTd0.v[kAesSbox.v[w & 0xff]] ^ rotl32(kAesTd0.v[kAesSbox.v[(w >> 8) & 0xff]], 8) ^
           rotl32(kAesTd0.v[kAesSbox.v[(w >> 16) & 0xff]], 16) ^ rotl32(kAesTd0.v[kAesSbox.v[w >> 24]], 24);
}

// the schedule of the equivalent inverse cipher: the round keys in reverse order, InvMixColumns applied to
// all but the first and the last
inline void aes256_decrypt_schedule(const uint32_t rk[kAesWords], uint32_t dk[kAesWords]) {
    for (int r = 0; r <= kAesRounds; ++r)
        for (int c = 0; c < 4; ++c) {
            const uint32_t w = rk[4 * (kAesRounds - r) + c];
            dk[4 * r + c] = r == 0 || r == kAesRounds ? w : aes_inv_mix_column(w);
        }
}

inline void aes256_encrypt_words(const uint32_t rk[kAesWords], uint32_t s[4]) {
    const uint32_t* te = kAesTe0.v;
    uint32_t a = s[0] ^ rk[0], b = s[1] ^ rk[1], c = s[2] ^ rk[2], d = s[3] ^ rk[3];
    for (int r = 1; r < kAesRounds; ++r) {
        const uint32_t* k = rk + 4 * r;
        const uint32_t a2 = te[a & 0xff] ^ rotl32(te[(b >> 8) & 0xff], 8) ^ rotl32(te[(c >> 16) & 0xff], 16) ^
                            rotl32(te[d >> 24], 24) ^ k[0];
        const uint32_t b2 = te[b & 0xff] ^ rotl32(te[(c >> 8) & 0xff], 8) ^ rotl32(te[(d >> 16) & 0xff], 16) ^
                            rotl32(te[a >> 24], 24) ^ k[1];
        const uint32_t c2 = te[c & 0xff] ^ rotl32(te[(d >> 8) & 0xff], 8) ^ rotl32(te[(a >> 16) & 0xff], 16) ^
                            rotl32(te[b >> 24], 24) ^ k[2];
        const uint32_t d2 = te[d & 0xff] ^ rotl32(te[(a >> 8) & 0xff], 8) ^ rotl32(te[(b >> 16) & 0xff], 16) ^
                            rotl32(te[c >> 24], 24) ^ k[3];
        a = a2, b = b2, c = c2, d = d2;
    }
    const uint32_t* k = rk + 4 * kAesRounds;
    const uint8_t* sb = kAesSbox.v;
    s[0] = (sb[a & 0xff] | (uint32_t(sb[(b >> 8) & 0xff]) << 8) | (uint32_t(sb[(c >> 16) & 0xff]) << 16) |
            (uint32_t(sb[d >> 24]) << 24)) ^ k[0];
    s[1] = (sb[b & 0xff] | (uint32_t(sb[(c >> 8) & 0xff]) << 8) | (uint32_t(sb[(d >> 16) & 0xff]) << 16) |
            (uint32_t(sb[a >> 24]) << 24)) ^ k[1];
    s[2] = (sb[c & 0xff] | (uint32_t(sb[(d >> 8) & 0xff]) << 8) | (uint32_t(sb[(a >> 16) & 0xff]) << 16) |
            (uint32_t(sb[b >> 24]) << 24)) ^ k[2];
    s[3] = (sb[d & 0xff] | (uint32_t(sb[(a >> 8) & 0xff]) << 8) | (uint32_t(sb[(b >> 16) & 0xff]) << 16) |
            (uint32_t(sb[c >> 24]) << 24)) ^ k[3];
}

inline void aes256_decrypt_words(const uint32_t dk[kAesWords], uint32_t s[4]) {
    const uint32_t* td = kAesTd0.v;
    uint32_t a = s[0] ^ dk[0], b = s[1] ^ dk[1], c = s[2] ^ dk[2], d = s[3] ^ dk[3];
    for (int r = 1; r < kAesRounds; ++r) {
        const uint32_t* k = dk + 4 * r;
        const uint32_t a2 = td[a & 0xff] ^ rotl32(td[(d >> 8) & 0xff], 8) ^ rotl32(td[(c >> 16) & 0xff], 16) ^
                            rotl32(td[b >> 24], 24) ^ k[0];
        const uint32_t b2 = td[b & 0xff] ^ rotl32(td[(a >> 8) & 0xff], 8) ^ rotl32(td[(d >> 16) & 0xff], 16) ^
                            rotl32(td[c >> 24], 24) ^ k[1];
        const uint32_t c2 = td[c & 0xff] ^ rotl32(td[(b >> 8) & 0xff], 8) ^ rotl32(td[(a >> 16) & 0xff], 16) ^
                            rotl32(td[d >> 24], 24) ^ k[2];
        const uint32_t d2 = td[d & 0xff] ^ rotl32(td[(c >> 8) & 0xff], 8) ^ rotl32(td[(b >> 16) & 0xff], 16) ^
                            rotl32(td[a >> 24], 24) ^ k[3];
        a = a2, b = b2, c = c2, d = d2;
    }
    const uint32_t* k = dk + 4 * kAesRounds;
    const uint8_t* sb = kAesInvSbox.v;
    s[0] = (sb[a & 0xff] | (uint32_t(sb[(d >> 8) & 0xff]) << 8) | (uint32_t(sb[(c >> 16) & 0xff]) << 16) |
            (uint32_t(sb[b >> 24]) << 24)) ^ k[0];
    s[1] = (sb[b & 0xff] | (uint32_t(sb[(a >> 8) & 0xff]) << 8) | (uint32_t(sb[(d >> 16) & 0xff]) << 16) |
            (uint32_t(sb[c >> 24]) << 24)) ^ k[1];
    s[2] = (sb[c & 0xff] | (uint32_t(sb[(b >> 8) & 0xff]) << 8) | (uint32_t(sb[(a >> 16) & 0xff]) << 16) |
            (uint32_t(sb[d >> 24]) << 24)) ^ k[2];
    s[3] = (sb[d & 0xff] | (uint32_t(sb[(c >> 8) & 0xff]) << 8) | (uint32_t(sb[(b >> 16) & 0xff]) << 16) |
            (uint32_t(sb[a >> 24]) << 24)) ^ k[3];
}

// ------------------------------------------------------------------ SM4 (GB/T 32907-2016 6, 7)
// the 32 round keys; decryption runs the same rounds with them reversed
inline void sm4_expand_key(const uint8_t key16[16], uint32_t rk[kSm4Words]) {
    constexpr uint32_t fk[4] = {0xa3b1bac6u, 0x56aa3350u, 0x677d9197u, 0xb27022dcu};
    uint32_t k[4];
    for (int i = 0; i < 4; ++i) k[i] = load_be32(key16 + 4 * i) ^ fk[i];
    for (int i = 0; i < kSm4Words; ++i) {
        uint32_t ck = 0;  // byte j of CK_i is (4i + j) * 7 mod 256
        for (int j = 0; j < 4; ++j) ck = (ck << 8) | (((4 * i + j) * 7) & 0xff);
        const uint32_t x = k[1] ^ k[2] ^ k[3] ^ ck;
        const uint32_t t = (static_cast<uint32_t>(kSm4Sbox.v[x >> 24]) << 24) |
                           (static_cast<uint32_t>(kSm4Sbox.v[(x >> 16) & 0xff]) << 16) |
                           (static_cast<uint32_t>(kSm4Sbox.v[(x >> 8) & 0xff]) << 8) | kSm4Sbox.v[x & 0xff];
        rk[i] = k[0] ^ sm4_Lkey(t);
        k[0] = k[1], k[1] = k[2], k[2] = k[3], k[3] = rk[i];
    }
}
inline void sm4_decrypt_schedule(const uint32_t rk[kSm4Words], uint32_t dk[kSm4Words]) {
    for (int i = 0; i < kSm4Words; ++i) dk[i] = rk[kSm4Words - 1 - i];
}

// the 32 rounds and the reverse transform over big-endian words (decryption: the reversed schedule)
inline void sm4_crypt_words(const uint32_t rk[kSm4Words], uint32_t x[4]) {
    const uint32_t* t0 = kSm4T0.v;
    uint32_t a = x[0], b = x[1], c = x[2], d = x[3];
    for (int i = 0; i < kSm4Words; ++i) {
        const uint32_t v = b ^ c ^ d ^ rk[i];
        const uint32_t n = a ^ t0[v >> 24] ^ rotr32(t0[(v >> 16) & 0xff], 8) ^ rotr32(t0[(v >> 8) & 0xff], 16) ^
                           rotr32(t0[v & 0xff], 24);
        a = b, b = c, c = d, d = n;
    }
    x[0] = d, x[1] = c, x[2] = b, x[3] = a;
}

// ------------------------------------------------------------------ one cipher, one direction, one key
// The schedule a batch runs with and its IV as the words the block functions take (both what the kernels
// receive by value in their arguments).
struct Schedule {
    uint32_t rk[kAesWords];  // AES: 60 words; SM4: the first 32
    uint32_t iv[4];
};

inline void load_block(int cipher, const uint8_t* p, uint32_t w[4]) {
    for (int i = 0; i < 4; ++i) w[i] = cipher == kSm4 ? load_be32(p + 4 * i) : load_le32(p + 4 * i);
}
inline void store_block(int cipher, uint8_t* p, const uint32_t w[4]) {
    for (int i = 0; i < 4; ++i) cipher == kSm4 ? store_be32(p + 4 * i, w[i]) : store_le32(p + 4 * i, w[i]);
}

inline Schedule make_schedule(int cipher, bool decrypt, const uint8_t* key, size_t key_len, const uint8_t* iv,
                              size_t iv_len) {
    Schedule s{};
    uint8_t k[32], v[16];
    uint32_t enc[kAesWords] = {};
    normalise_key(cipher, key, key_len, k);
    normalise_iv(key, key_len, iv, iv_len, v);
    if (cipher == kSm4) {
        sm4_expand_key(k, enc);
        if (decrypt) sm4_decrypt_schedule(enc, s.rk);
        else memcpy(s.rk, enc, sizeof(uint32_t) * kSm4Words);
    } else {
        aes256_expand_key(k, enc);
        if (decrypt) aes256_decrypt_schedule(enc, s.rk);
        else memcpy(s.rk, enc, sizeof(enc));
    }
    load_block(cipher, v, s.iv);
    return s;
}

inline void encrypt_words(int cipher, const Schedule& s, uint32_t w[4]) {
    cipher == kSm4 ? sm4_crypt_words(s.rk, w) : aes256_encrypt_words(s.rk, w);
}
inline void decrypt_words(int cipher, const Schedule& s, uint32_t w[4]) {  // s: a decrypt schedule
    cipher == kSm4 ? sm4_crypt_words(s.rk, w) : aes256_decrypt_words(s.rk, w);
}
inline void encrypt_block(int cipher, const Schedule& s, const uint8_t in[16], uint8_t out[16]) {
    uint32_t w[4];
    load_block(cipher, in, w);
    encrypt_words(cipher, s, w);
    store_block(cipher, out, w);
}
inline void decrypt_block(int cipher, const Schedule& s, const uint8_t in[16], uint8_t out[16]) {
    uint32_t w[4];
    load_block(cipher, in, w);
    decrypt_words(cipher, s, w);
    store_block(cipher, out, w);
}

inline uint64_t cbc_padded_size(uint64_t len) { return (len / 16 + 1) * 16; }

// CBC with PKCS#7 over one value: out takes cbc_padded_size(len) bytes (s: an encrypt schedule)
inline void cbc_encrypt(int cipher, const Schedule& s, const uint8_t* in, uint64_t len, uint8_t* out) {
    uint32_t chain[4] = {s.iv[0], s.iv[1], s.iv[2], s.iv[3]};
    const uint64_t blocks = len / 16 + 1;
    for (uint64_t j = 0; j < blocks; ++j) {
        uint8_t b[16];
        const uint64_t have = j + 1 < blocks ? 16 : len - 16 * j;
        if (have) memcpy(b, in + 16 * j, have);
        memset(b + have, static_cast<int>(16 - have), 16 - have);
        uint32_t w[4];
        load_block(cipher, b, w);
        for (int i = 0; i < 4; ++i) chain[i] ^= w[i];
        encrypt_words(cipher, s, chain);
        store_block(cipher, out + 16 * j, chain);
    }
}

// The inverse (s: a decrypt schedule): out takes len bytes, the padding included; *out_len is the plaintext's
// length, 0 with a status other than kStatusOk.  in and out must not overlap.
inline int cbc_decrypt(int cipher, const Schedule& s, const uint8_t* in, uint64_t len, uint8_t* out,
                       uint64_t* out_len) {
    *out_len = 0;
    if (len == 0 || len % 16) return kStatusBadLength;
    uint32_t prev[4] = {s.iv[0], s.iv[1], s.iv[2], s.iv[3]};
    for (uint64_t j = 0; j < len / 16; ++j) {
        uint32_t c[4], w[4];
        load_block(cipher, in + 16 * j, c);
        for (int i = 0; i < 4; ++i) w[i] = c[i];
        decrypt_words(cipher, s, w);
        for (int i = 0; i < 4; ++i) w[i] ^= prev[i], prev[i] = c[i];
        store_block(cipher, out + 16 * j, w);
    }
    const uint8_t p = out[len - 1];
    if (p < 1 || p > 16) return kStatusBadPadding;
    for (uint64_t k = len - p; k < len; ++k)
        if (out[k] != p) return kStatusBadPadding;
    *out_len = len - p;
    return kStatusOk;
}

}  // namespace cipher
}  // namespace bcosgpu
