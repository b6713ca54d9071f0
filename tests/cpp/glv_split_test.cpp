// Host test of csrc/glv_split.h (glv_split_core: the exact-integer GLV split of the secp256k1 kernels).
//
// The yardstick is a literal restatement of the form the kernels ran before it, in 64-bit limbs with plain
// arithmetic mod n and no code of the header: c1, c2 by the full 512-bit rounding products, k2 = c1 (-b1) +
// c2 (n - b2) mod n, k1 = k - k2 lambda mod n, each negated when above (n - 1) / 2.  All four outputs are
// compared with it; independently of it, k1 + k2 lambda = k (mod n) with the signs applied (the core hands
// out four limbs per half, so a half of 2^128 or more would break this identity).
//
// Cases: the edge scalars, t and t lambda mod n for t = 1 .. 64 (one half is zero), 1,000,000 seeded random
// k < n, and a seeded search of 1,000,000 more for the largest |k1|, |k2| and for the rounding fractions of c1,
// c2 nearest 1/2, whose maxima are printed (tests/test_gpu_glv_split.py runs the found scalars through the
// kernels).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../fisco-bcos_amd/csrc/glv_split.h"

typedef unsigned __int128 u128;

namespace {

struct U256 {
    uint64_t v[4];
};

const U256 N = {{0xBFD25E8CD0364141ull, 0xBAAEDCE6AF48A03Bull, 0xFFFFFFFFFFFFFFFEull, 0xFFFFFFFFFFFFFFFFull}};
const uint64_t NC[3] = {0x402DA1732FC9BEBFull, 0x4551231950B75FC4ull, 1ull};  // 2^256 - n
const U256 HALF = {{0xDFE92F46681B20A0ull, 0x5D576E7357A4501Dull, 0xFFFFFFFFFFFFFFFFull, 0x7FFFFFFFFFFFFFFFull}};
const U256 LAMBDA = {{0xDF02967C1B23BD72ull, 0x122E22EA20816678ull, 0xA5261C028812645Aull, 0x5363AD4CC05C30E0ull}};
const U256 G1 = {{0xE893209A45DBB031ull, 0x3DAA8A1471E8CA7Full, 0xE86C90E49284EB15ull, 0x3086D221A7D46BCDull}};
const U256 G2 = {{0x1571B4AE8AC47F71ull, 0x221208AC9DF506C6ull, 0x6F547FA90ABFE4C4ull, 0xE4437ED6010E8828ull}};
const U256 MB1 = {{0x6F547FA90ABFE4C3ull, 0xE4437ED6010E8828ull, 0, 0}};
const U256 B2 = {{0xE86C90E49284EB15ull, 0x3086D221A7D46BCDull, 0, 0}};

// r[0 .. na + nb) = a * b
void mul_nm(uint64_t* r, const uint64_t* a, int na, const uint64_t* b, int nb) {
    for (int i = 0; i < na + nb; ++i) r[i] = 0;
    for (int i = 0; i < na; ++i) {
        uint64_t carry = 0;
        for (int j = 0; j < nb; ++j) {
            const u128 p = static_cast<u128>(a[i]) * b[j] + r[i + j] + carry;
            r[i + j] = static_cast<uint64_t>(p);
            carry = static_cast<uint64_t>(p >> 64);
        }
        r[i + nb] = carry;
    }
}
int cmp256(const U256& a, const U256& b) {
    for (int i = 3; i >= 0; --i)
        if (a.v[i] != b.v[i]) return a.v[i] < b.v[i] ? -1 : 1;
    return 0;
}
uint64_t add256(U256& r, const U256& a, const U256& b) {
    u128 c = 0;
    for (int i = 0; i < 4; ++i) {
        c += static_cast<u128>(a.v[i]) + b.v[i];
        r.v[i] = static_cast<uint64_t>(c);
        c >>= 64;
    }
    return static_cast<uint64_t>(c);
}
uint64_t sub256(U256& r, const U256& a, const U256& b) {
    uint64_t bw = 0;
    for (int i = 0; i < 4; ++i) {
        const u128 d = static_cast<u128>(a.v[i]) - b.v[i] - bw;
        r.v[i] = static_cast<uint64_t>(d);
        bw = static_cast<uint64_t>(d >> 64) & 1u;
    }
    return bw;
}
// t (512 bits) mod n: 2^256 = NC (mod n), folded until the upper half is empty
U256 mod_n(const uint64_t t[8]) {
    uint64_t cur[8];
    memcpy(cur, t, sizeof cur);
    for (;;) {
        bool hi = false;
        for (int i = 4; i < 8; ++i) hi = hi || cur[i] != 0;
        if (!hi) break;
        uint64_t f[8];
        mul_nm(f, cur + 4, 4, NC, 3);  // 7 limbs
        f[7] = 0;
        u128 c = 0;
        for (int i = 0; i < 8; ++i) {
            c += static_cast<u128>(f[i]) + (i < 4 ? cur[i] : 0);
            cur[i] = static_cast<uint64_t>(c);
            c >>= 64;
        }
    }
    U256 r = {{cur[0], cur[1], cur[2], cur[3]}};
    while (cmp256(r, N) >= 0) sub256(r, r, N);
    return r;
}
U256 mulmod(const U256& a, const U256& b) {
    uint64_t t[8];
    mul_nm(t, a.v, 4, b.v, 4);
    return mod_n(t);
}
U256 addmod(const U256& a, const U256& b) {
    U256 r;
    const uint64_t c = add256(r, a, b);
    if (c || cmp256(r, N) >= 0) sub256(r, r, N);
    return r;
}
U256 submod(const U256& a, const U256& b) {
    U256 r;
    if (sub256(r, a, b)) add256(r, r, N);
    return r;
}
U256 negmod(const U256& a) {
    const U256 z = {{0, 0, 0, 0}};
    return submod(z, a);
}

struct Split {
    U256 k1, k2;
    bool neg1, neg2;
    uint64_t frac1, frac2;  // the top 64 bits of the rounding products' fractions
};

// c = round(k g / 2^384), as the kernels always took it: limbs 6, 7 of the product plus bit 383, mod 2^128
U256 round_mul(const U256& k, const U256& g, uint64_t& frac) {
    uint64_t t[8];
    mul_nm(t, k.v, 4, g.v, 4);
    frac = t[5];
    u128 c = static_cast<u128>(t[6]) + (t[5] >> 63);
    U256 r = {{0, 0, 0, 0}};
    r.v[0] = static_cast<uint64_t>(c);
    c >>= 64;
    c += t[7];
    r.v[1] = static_cast<uint64_t>(c);
    return r;
}

Split yardstick(const U256& k) {
    Split s;
    const U256 c1 = round_mul(k, G1, s.frac1), c2 = round_mul(k, G2, s.frac2);
    const U256 x = mulmod(c1, MB1);
    const U256 y = mulmod(c2, negmod(B2));
    s.k2 = addmod(x, y);
    s.k1 = submod(k, mulmod(s.k2, LAMBDA));
    s.neg1 = cmp256(HALF, s.k1) < 0;
    if (s.neg1) s.k1 = negmod(s.k1);
    s.neg2 = cmp256(HALF, s.k2) < 0;
    if (s.neg2) s.k2 = negmod(s.k2);
    return s;
}

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint64_t rng() {  // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
U256 random_scalar() {
    for (;;) {
        const U256 k = {{rng(), rng(), rng(), rng()}};
        if (cmp256(k, N) < 0) return k;
    }
}

void print256(const char* tag, const U256& a) {
    printf("%s %016llx%016llx%016llx%016llx\n", tag, (unsigned long long)a.v[3], (unsigned long long)a.v[2],
           (unsigned long long)a.v[1], (unsigned long long)a.v[0]);
}

long checked = 0;

// the code under test on k, against the yardstick and against k1 + k2 lambda = k
Split check(const U256& k) {
    uint32_t kw[8], k1w[4], k2w[4], n1 = 7, n2 = 7;
    for (int i = 0; i < 4; ++i) {
        kw[2 * i] = static_cast<uint32_t>(k.v[i]);
        kw[2 * i + 1] = static_cast<uint32_t>(k.v[i] >> 32);
    }
    bcosgpu::glv_split_core(k1w, n1, k2w, n2, kw);
    const U256 k1 = {{k1w[0] | static_cast<uint64_t>(k1w[1]) << 32, k1w[2] | static_cast<uint64_t>(k1w[3]) << 32, 0, 0}};
    const U256 k2 = {{k2w[0] | static_cast<uint64_t>(k2w[1]) << 32, k2w[2] | static_cast<uint64_t>(k2w[3]) << 32, 0, 0}};
    const Split want = yardstick(k);
    bool ok = n1 <= 1 && n2 <= 1 && cmp256(k1, want.k1) == 0 && cmp256(k2, want.k2) == 0 &&
              (n1 != 0) == want.neg1 && (n2 != 0) == want.neg2;
    // independent of the yardstick: the identity, and the bound (the halves have four limbs each)
    const U256 s1 = n1 ? negmod(k1) : k1, s2 = n2 ? negmod(k2) : k2;
    const U256 back = addmod(s1, mulmod(s2, LAMBDA));
    ok = ok && cmp256(back, k) == 0 && want.k1.v[2] == 0 && want.k1.v[3] == 0 && want.k2.v[2] == 0 && want.k2.v[3] == 0;
    if (!ok) {
        print256("FAIL k      ", k);
        print256("  k1 got    ", k1);
        print256("  k1 want   ", want.k1);
        print256("  k2 got    ", k2);
        print256("  k2 want   ", want.k2);
        print256("  k1+k2 lam ", back);
        printf("  neg got %u %u want %d %d\n", n1, n2, want.neg1, want.neg2);
        exit(1);
    }
    ++checked;
    return want;
}

U256 small(uint64_t x) {
    const U256 r = {{x, 0, 0, 0}};
    return r;
}

}  // namespace

int main() {
    const U256 one = small(1), two = small(2);
    const U256 p128 = {{0, 0, 1, 0}}, p128m1 = {{~0ull, ~0ull, 0, 0}}, p255 = {{0, 0, 0, 1ull << 63}};
    const U256 edges[] = {small(0), one, two, submod(N, one), submod(N, two), HALF, addmod(HALF, one), LAMBDA,
                          negmod(LAMBDA), addmod(LAMBDA, one), submod(LAMBDA, one), p128m1, p128, p255};
    for (const U256& k : edges) check(k);
    for (uint64_t t = 1; t <= 64; ++t) {
        const Split a = check(small(t));  // k2 = 0
        const Split b = check(mulmod(small(t), LAMBDA));  // k1 = 0
        const Split c = check(negmod(small(t)));
        const Split d = check(negmod(mulmod(small(t), LAMBDA)));
        const U256 z = small(0), tt = small(t);
        if (cmp256(a.k2, z) || cmp256(a.k1, tt) || cmp256(b.k1, z) || cmp256(b.k2, tt) || cmp256(c.k2, z) ||
            cmp256(c.k1, tt) || !c.neg1 || cmp256(d.k1, z) || cmp256(d.k2, tt) || !d.neg2) {
            printf("FAIL: t = %llu does not split into (t, 0) / (0, t)\n", (unsigned long long)t);
            return 1;
        }
    }
    for (int i = 0; i < 1000000; ++i) check(random_scalar());
    // the search: largest halves, rounding fractions nearest 1/2 (distance of the fraction's top 64 bits from 2^63)
    rng_state = 0x243f6a8885a308d3ull;
    U256 best_k1 = small(0), best_k2 = small(0), arg_k1 = small(0), arg_k2 = small(0), arg_f1 = small(0), arg_f2 = small(0);
    uint64_t best_f1 = ~0ull, best_f2 = ~0ull;
    for (int i = 0; i < 1000000; ++i) {
        const U256 k = random_scalar();
        const Split s = check(k);
        if (cmp256(s.k1, best_k1) > 0) best_k1 = s.k1, arg_k1 = k;
        if (cmp256(s.k2, best_k2) > 0) best_k2 = s.k2, arg_k2 = k;
        const uint64_t d1 = s.frac1 >> 63 ? s.frac1 - (1ull << 63) : (1ull << 63) - 1 - s.frac1;
        const uint64_t d2 = s.frac2 >> 63 ? s.frac2 - (1ull << 63) : (1ull << 63) - 1 - s.frac2;
        if (d1 < best_f1) best_f1 = d1, arg_f1 = k;
        if (d2 < best_f2) best_f2 = d2, arg_f2 = k;
    }
    printf("glv split ok: %ld scalars\n", checked);
    print256("max |k1|        ", best_k1);
    print256("  at k          ", arg_k1);
    print256("max |k2|        ", best_k2);
    print256("  at k          ", arg_k2);
    printf("c1 fraction nearest 1/2: |frac - 1/2| < %.3g\n", (static_cast<double>(best_f1) + 1) / 18446744073709551616.0);
    print256("  at k          ", arg_f1);
    printf("c2 fraction nearest 1/2: |frac - 1/2| < %.3g\n", (static_cast<double>(best_f2) + 1) / 18446744073709551616.0);
    print256("  at k          ", arg_f2);
    return 0;
}
