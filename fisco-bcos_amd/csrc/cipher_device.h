// cipher_device.h -- device helpers of the storage cipher kernels (cipher_kernels.hip): the lookup tables in
// LDS, the AES-256 and SM4 block functions over them, and the reader of 16-byte blocks at unaligned offsets.
// The rules, the word conventions and the table generators are cipher_host.h's.
//
// Tables: one 256-entry 32-bit table per direction; the other three byte positions take it rotated
// (v_alignbit_b32): Te0 / Td0 for AES (the last encryption round reads the plain S-box from byte 1 of Te0, the
// last decryption round a 256-byte inverse S-box), T0 = L(S[x] << 24) for SM4 in both directions (L commutes
// with rotation).  The workgroup copies them from constant memory into LDS when the kernel starts, in one of
// two layouts:
//   plain        tab[x], 1 KiB: a lookup's bank is (x % 32), so a wave's 64 data-dependent indices collide at
//                random
//   replicated   tab[x * 32 + (lane & 31)], 32 KiB: a ds_read_b32 banks by (a / 4) % 32 within each 32-lane
//                half, so lane l always reads bank l % 32 and no lookup conflicts
// BCOSGPU_CIPHER_TABLES_REPLICATED selects the layout at compile time; the shipped default and the A/B that
// chose it: DESIGN.md 6b, profiles/cipher_tables_ab.json.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cipher_host.h"

#ifndef BCOSGPU_CIPHER_TABLES_REPLICATED
#define BCOSGPU_CIPHER_TABLES_REPLICATED 0
#endif

namespace bcosgpu {

constexpr bool kCipherTablesReplicated = BCOSGPU_CIPHER_TABLES_REPLICATED != 0;
constexpr int kCipherThreads = 256;
constexpr int kCipherTableWords = kCipherTablesReplicated ? 256 * 32 : 256;

__device__ __constant__ static const cipher::WordTable kDevAesTe0 = cipher::aes_te0();
__device__ __constant__ static const cipher::WordTable kDevAesTd0 = cipher::aes_td0();
__device__ __constant__ static const cipher::WordTable kDevSm4T0 = cipher::sm4_t0();
__device__ __constant__ static const cipher::ByteTable kDevAesInvSbox = cipher::aes_inv_sbox();
__device__ __constant__ static const uint32_t kCipherZeroDwords[2] = {0u, 0u};

// the workgroup's copy of a word table (every thread calls it; the caller synchronises)
__device__ __forceinline__ void cipher_fill_table(uint32_t* __restrict__ lds, const cipher::WordTable& src) {
    if (kCipherTablesReplicated) {
        for (int k = threadIdx.x; k < kCipherTableWords; k += kCipherThreads) lds[k] = src.v[k >> 5];
    } else {
        for (int k = threadIdx.x; k < 256; k += kCipherThreads) lds[k] = src.v[k];
    }
}

// A thread's view of a word table in LDS.
struct CipherTable {
    const uint32_t* t;  // replicated: the table's base plus the lane's bank
    __device__ __forceinline__ explicit CipherTable(const uint32_t* lds)
        : t(kCipherTablesReplicated ? lds + (threadIdx.x & 31u) : lds) {}
    __device__ __forceinline__ uint32_t operator[](uint32_t x) const {
        return kCipherTablesReplicated ? t[x << 5] : t[x];
    }
};

__device__ __forceinline__ uint32_t cipher_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
__device__ __forceinline__ uint32_t cipher_bswap(uint32_t x) { return __builtin_bswap32(x); }

// ------------------------------------------------------------------ AES-256 (columns as little-endian words)
__device__ __forceinline__ void aes256_encrypt_dev(const cipher::Schedule& ck, const CipherTable& te, uint32_t s[4]) {
    uint32_t a = s[0] ^ ck.rk[0], b = s[1] ^ ck.rk[1], c = s[2] ^ ck.rk[2], d = s[3] ^ ck.rk[3];
#pragma unroll
    for (int r = 1; r < cipher::kAesRounds; ++r) {
        const uint32_t a2 = te[a & 0xff] ^ cipher_rotl(te[(b >> 8) & 0xff], 8) ^ cipher_rotl(te[(c >> 16) & 0xff], 16) ^
                            cipher_rotl(te[d >> 24], 24) ^ ck.rk[4 * r];
        const uint32_t b2 = te[b & 0xff] ^ cipher_rotl(te[(c >> 8) & 0xff], 8) ^ cipher_rotl(te[(d >> 16) & 0xff], 16) ^
                            cipher_rotl(te[a >> 24], 24) ^ ck.rk[4 * r + 1];
        const uint32_t c2 = te[c & 0xff] ^ cipher_rotl(te[(d >> 8) & 0xff], 8) ^ cipher_rotl(te[(a >> 16) & 0xff], 16) ^
                            cipher_rotl(te[b >> 24], 24) ^ ck.rk[4 * r + 2];
        const uint32_t d2 = te[d & 0xff] ^ cipher_rotl(te[(a >> 8) & 0xff], 8) ^ cipher_rotl(te[(b >> 16) & 0xff], 16) ^
                            cipher_rotl(te[c >> 24], 24) ^ ck.rk[4 * r + 3];
        a = a2, b = b2, c = c2, d = d2;
    }
    // the last round has no MixColumns: S[x] is byte 1 of Te0[x]
#define AES_SB(x, sh) (((te[(x)] >> 8) & 0xffu) << (sh))
    s[0] = (AES_SB(a & 0xff, 0) | AES_SB((b >> 8) & 0xff, 8) | AES_SB((c >> 16) & 0xff, 16) | AES_SB(d >> 24, 24)) ^ ck.rk[56];
    s[1] = (AES_SB(b & 0xff, 0) | AES_SB((c >> 8) & 0xff, 8) | AES_SB((d >> 16) & 0xff, 16) | AES_SB(a >> 24, 24)) ^ ck.rk[57];
    s[2] = (AES_SB(c & 0xff, 0) | AES_SB((d >> 8) & 0xff, 8) | AES_SB((a >> 16) & 0xff, 16) | AES_SB(b >> 24, 24)) ^ ck.rk[58];
    s[3] = (AES_SB(d & 0xff, 0) | AES_SB((a >> 8) & 0xff, 8) | AES_SB((b >> 16) & 0xff, 16) | AES_SB(c >> 24, 24)) ^ ck.rk[59];
#undef AES_SB
}

// the equivalent inverse cipher (ck: cipher_host.h's decrypt schedule); isb: the inverse S-box in LDS
__device__ __forceinline__ void aes256_decrypt_dev(const cipher::Schedule& ck, const CipherTable& td,
                                                   const uint8_t* __restrict__ isb, uint32_t s[4]) {
    uint32_t a = s[0] ^ ck.rk[0], b = s[1] ^ ck.rk[1], c = s[2] ^ ck.rk[2], d = s[3] ^ ck.rk[3];
#pragma unroll
    for (int r = 1; r < cipher::kAesRounds; ++r) {
        const uint32_t a2 = td[a & 0xff] ^ cipher_rotl(td[(d >> 8) & 0xff], 8) ^ cipher_rotl(td[(c >> 16) & 0xff], 16) ^
                            cipher_rotl(td[b >> 24], 24) ^ ck.rk[4 * r];
        const uint32_t b2 = td[b & 0xff] ^ cipher_rotl(td[(a >> 8) & 0xff], 8) ^ cipher_rotl(td[(d >> 16) & 0xff], 16) ^
                            cipher_rotl(td[c >> 24], 24) ^ ck.rk[4 * r + 1];
        const uint32_t c2 = td[c & 0xff] ^ cipher_rotl(td[(b >> 8) & 0xff], 8) ^ cipher_rotl(td[(a >> 16) & 0xff], 16) ^
                            cipher_rotl(td[d >> 24], 24) ^ ck.rk[4 * r + 2];
        const uint32_t d2 = td[d & 0xff] ^ cipher_rotl(td[(c >> 8) & 0xff], 8) ^ cipher_rotl(td[(b >> 16) & 0xff], 16) ^
                            cipher_rotl(td[a >> 24], 24) ^ ck.rk[4 * r + 3];
        a = a2, b = b2, c = c2, d = d2;
    }
#define AES_ISB(x, sh) (static_cast<uint32_t>(isb[(x)]) << (sh))
    s[0] = (AES_ISB(a & 0xff, 0) | AES_ISB((d >> 8) & 0xff, 8) | AES_ISB((c >> 16) & 0xff, 16) | AES_ISB(b >> 24, 24)) ^ ck.rk[56];
    s[1] = (AES_ISB(b & 0xff, 0) | AES_ISB((a >> 8) & 0xff, 8) | AES_ISB((d >> 16) & 0xff, 16) | AES_ISB(c >> 24, 24)) ^ ck.rk[57];
    s[2] = (AES_ISB(c & 0xff, 0) | AES_ISB((b >> 8) & 0xff, 8) | AES_ISB((a >> 16) & 0xff, 16) | AES_ISB(d >> 24, 24)) ^ ck.rk[58];
    s[3] = (AES_ISB(d & 0xff, 0) | AES_ISB((c >> 8) & 0xff, 8) | AES_ISB((b >> 16) & 0xff, 16) | AES_ISB(a >> 24, 24)) ^ ck.rk[59];
#undef AES_ISB
}

// ------------------------------------------------------------------ SM4 (big-endian words)
__device__ __forceinline__ uint32_t sm4_round_dev(const CipherTable& t0, uint32_t v) {
    return t0[v >> 24] ^ cipher_rotl(t0[(v >> 16) & 0xff], 24) ^ cipher_rotl(t0[(v >> 8) & 0xff], 16) ^
           cipher_rotl(t0[v & 0xff], 8);
}
// the 32 rounds and the reverse transform (decryption: the reversed schedule)
__device__ __forceinline__ void sm4_crypt_dev(const cipher::Schedule& ck, const CipherTable& t0, uint32_t x[4]) {
    uint32_t a = x[0], b = x[1], c = x[2], d = x[3];
#pragma unroll
    for (int i = 0; i < cipher::kSm4Words; i += 4) {
        a ^= sm4_round_dev(t0, b ^ c ^ d ^ ck.rk[i]);
        b ^= sm4_round_dev(t0, c ^ d ^ a ^ ck.rk[i + 1]);
        c ^= sm4_round_dev(t0, d ^ a ^ b ^ ck.rk[i + 2]);
        d ^= sm4_round_dev(t0, a ^ b ^ c ^ ck.rk[i + 3]);
    }
    x[0] = d, x[1] = c, x[2] = b, x[3] = a;
}

// memory order <-> the cipher's words: SM4's are big-endian
template <int CIPHER>
__device__ __forceinline__ void cipher_swap_words(uint32_t w[4]) {
    if (CIPHER == cipher::kSm4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = cipher_bswap(w[k]);
    }
}

// ------------------------------------------------------------------ 16-byte blocks of a value at any offset
// Block j of a value as four little-endian dwords, read through aligned dword loads (five per block, shifted
// by v_alignbyte_b32).  Never reads a dword that does not overlap the value: indices are clamped to the last
// such dword and the surplus selected away; an empty value reads a zero constant.  The last block is PKCS#7's:
// the bytes past the value's end hold 16 - len % 16.
struct CipherBlockReader {
    const uint32_t* q;
    uint32_t sh, len, nq, last;
    __device__ CipherBlockReader(const uint8_t* p, uint32_t n) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        sh = static_cast<uint32_t>(a & 3u);
        nq = n ? (n + sh + 3u) >> 2 : 0u;
        q = nq ? reinterpret_cast<const uint32_t*>(a - sh) : kCipherZeroDwords;
        last = nq ? nq - 1u : 0u;
        len = n;
    }
    __device__ __forceinline__ void block(uint32_t j, uint32_t w[4]) const {
        uint32_t d[5];
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) {
            const uint32_t i = 4u * j + k, v = q[i < last ? i : last];
            d[k] = i < nq ? v : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) w[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
        const uint32_t have = len - 16u * j;  // bytes of the value in this block and after
        if (have < 16u) {
            const uint32_t pad = (16u - have) * 0x01010101u;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t keep = have >= 4u * k + 4u ? 0xffffffffu
                                      : have <= 4u * k    ? 0u
                                                          : (1u << ((have - 4u * k) * 8u)) - 1u;
                w[k] = (w[k] & keep) | (pad & ~keep);
            }
        }
    }
};

}  // namespace bcosgpu
