// glv_split.h -- the core of the secp256k1 GLV scalar split (libsecp256k1's secp256k1_scalar_split_lambda)
// on plain 32-bit limb arrays.  Host/device in the manner of modinv30.h (F26_HD): no HIP header and no fe.h,
// so a host test can run it (tests/cpp/glv_split_test.cpp).  glv_split of ecc_device.h wraps it.
//
// The lattice basis (a1, b1), (a2, b2) has a1 + b1 lambda = a2 + b2 lambda = 0 (mod n).  With
//   c1 = round(k g1 / 2^384), c2 = round(k g2 / 2^384)     (g1 = round(2^384 b2 / n), g2 = round(2^384 (-b1) / n))
// the halves of k = k1 + k2 lambda (mod n) are the exact integers
//   k2 = c1 (-b1) - c2 b2,    k1 = k - c1 a1 - c2 a2,
// both of magnitude < 2^128 for every k < n.  So their low 160 bits in two's complement hold them whole: no
// product wider than that and no reduction mod n is needed (the earlier form took k2 mod n by a Montgomery
// product, k1 = k - k2 lambda by another, and compared both with (n - 1) / 2).  For every k in [0, n) the
// magnitudes and signs are those of that form, bit for bit (the host test restates it as the yardstick).
#pragma once
#include "fe26.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define GLV_TABLE __device__ __constant__ static const uint32_t
#else
#define GLV_TABLE static const uint32_t
#endif

namespace bcosgpu {

GLV_TABLE kGlvG1[8] = {0x45dbb031u, 0xe893209au, 0x71e8ca7fu, 0x3daa8a14u,
                       0x9284eb15u, 0xe86c90e4u, 0xa7d46bcdu, 0x3086d221u};
GLV_TABLE kGlvG2[8] = {0x8ac47f71u, 0x1571b4aeu, 0x9df506c6u, 0x221208acu,
                       0x0abfe4c4u, 0x6f547fa9u, 0x010e8828u, 0xe4437ed6u};
// -b1 (128 bits)
GLV_TABLE kGlvMB1[4] = {0x0abfe4c3u, 0x6f547fa9u, 0x010e8828u, 0xe4437ed6u};
// a1 = b2 (126 bits)
GLV_TABLE kGlvA1[4] = {0x9284eb15u, 0xe86c90e4u, 0xa7d46bcdu, 0x3086d221u};
// a2 (129 bits: limb 4 is its top bit)
GLV_TABLE kGlvA2[5] = {0x9d44cfd8u, 0x57c1108du, 0xa8e2f3f6u, 0x14ca50f7u, 0x00000001u};

// c = round(k g / 2^384): the full 8 x 8-limb product, bit 383 added to its top four limbs (the carry out of
// 2^128 cannot occur for k < n and is dropped, as it always was)
F26_HD void glv_round_mul(uint32_t c[4], const uint32_t k[8], const uint32_t* g) {
    uint32_t t[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) t[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint32_t carry = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint64_t p = static_cast<uint64_t>(k[i]) * g[j] + t[i + j] + carry;
            t[i + j] = static_cast<uint32_t>(p);
            carry = static_cast<uint32_t>(p >> 32);
        }
        t[i + 8] = carry;
    }
    uint64_t s = static_cast<uint64_t>(t[11] >> 31);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s += t[12 + i];
        c[i] = static_cast<uint32_t>(s);
        s >>= 32;
    }
}

// r = c m mod 2^160 for a four-limb c and an NB-limb m: the columns 0 .. 4 only, column 4's products low
// words only
template <int NB>
F26_HD void glv_mul_lo160(uint32_t r[5], const uint32_t c[4], const uint32_t* m) {
#pragma unroll
    for (int i = 0; i < 5; ++i) r[i] = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t carry = 0;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            if (i + j < 4) {
                const uint64_t p = static_cast<uint64_t>(c[i]) * m[j] + r[i + j] + carry;
                r[i + j] = static_cast<uint32_t>(p);
                carry = static_cast<uint32_t>(p >> 32);
            } else if (i + j == 4) {
                r[4] += c[i] * m[j] + carry;
                carry = 0;
            }
        }
        if (i + NB <= 4) r[i + NB] = carry;  // a column no earlier row has reached
    }
}

// r = a - b mod 2^160
F26_HD void glv_sub160(uint32_t r[5], const uint32_t a[5], const uint32_t b[5]) {
    uint32_t bw = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const uint64_t d = static_cast<uint64_t>(a[i]) - b[i] - bw;
        r[i] = static_cast<uint32_t>(d);
        bw = static_cast<uint32_t>(d >> 32) & 1u;
    }
}

// sign (bit 159) and magnitude (< 2^128) of a 160-bit two's complement value
F26_HD void glv_sign_mag(uint32_t mag[4], uint32_t& neg, const uint32_t x[5]) {
    neg = x[4] >> 31;
    const uint32_t m = 0u - neg;
    uint64_t s = neg;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s += x[i] ^ m;
        mag[i] = static_cast<uint32_t>(s);
        s >>= 32;
    }
}

// k = (neg1 ? -k1 : k1) + (neg2 ? -k2 : k2) lambda (mod n), k1, k2 < 2^128, for k < n (for n <= k < 2^256 the
// identity still holds mod n and the bound by a hair less; no caller passes such a k)
F26_HD void glv_split_core(uint32_t k1[4], uint32_t& neg1, uint32_t k2[4], uint32_t& neg2, const uint32_t k[8]) {
    uint32_t c1[4], c2[4];
    glv_round_mul(c1, k, kGlvG1);
    glv_round_mul(c2, k, kGlvG2);
    uint32_t p[5], q[5], x[5];
    glv_mul_lo160<4>(p, c1, kGlvMB1);
    glv_mul_lo160<4>(q, c2, kGlvA1);  // b2 = a1
    glv_sub160(x, p, q);
    glv_sign_mag(k2, neg2, x);
    glv_mul_lo160<4>(p, c1, kGlvA1);
    glv_mul_lo160<5>(q, c2, kGlvA2);
    glv_sub160(x, k, p);
    glv_sub160(x, x, q);
    glv_sign_mag(k1, neg1, x);
}

}  // namespace bcosgpu
