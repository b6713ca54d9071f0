// ecc_keyed.hip -- signature verification against REGISTERED public keys: the sealer path.
//
// SignatureCrypto::verify(pub, hash, sig) is called with a small, fixed set of keys on the block-check
// path: BlockValidator::checkSignatureList verifies one signature per sealer of the block against the
// consensus node list's keys (bcos-pbft/.../BlockValidator.cpp:141-182), PBFTCacheProcessor::
// checkPrecommitWeight likewise (PBFTCacheProcessor.cpp:795-821), both through Secp256k1Crypto.cpp:51-63 /
// SM2Crypto.cpp:66-79.  With the key known in advance, its variable-base multiplication needs no
// doublings at verify time: the engine keeps an 8-bit comb table per key (32 windows x 256 affine
// multiples b 2^(8i) P, 512 KiB of HBM, built once by key_table_kernel), so u2 P (secp256k1) / t P (SM2)
// is 32 table lookups, like u1 G / s G over G's 16-bit comb (16 lookups).
//
// The verify kernel spends 16 lanes (one DPP row) on each signature, 4 signatures per wave:
//   - every lane of the 16 runs the scalar work (range checks, s^-1 mod n and u1, u2 for secp256k1;
//     t = r + s and e = SM3(Z_A || h) with Z_A cached per key for SM2) -- in lockstep, so it costs the
//     same as on one lane;
//   - lane L sums its three table points (windows 2L, 2L+1 of the key's comb, window L of G's 16-bit
//     comb; the 8-bit G comb adds windows 2L, 2L+1 of it instead) with complete mixed additions;
//   - four levels of complete Jacobian additions reduce the 16 partial sums inside the row (partners
//     fetched with ds_bpermute), then the projective x-check (no inversion) gives the verdict.
// Critical path: secp256k1 ~ s^-1 + 3 madds + 4 adds, SM2 ~ 2 SM3 compressions + 3 madds + 4 adds --
// against 256 doublings per signature on the generic path.  Same decisions and verdicts as
// secp256k1_verify_lane26 / sm2_verify_rs26 (libsecp256k1 ecdsa_verify with low-S; sm2_do_verify), for
// every input: the additions are the complete ones (P = Q, P = -Q, infinity), since a key's owner can
// pick u1, u2 so that two partial sums coincide.
//
// What differs between the suites (field, curve, address hash, Z_A) is named once, in KeyedSuite<SUITE>;
// the table kernel, a lane's table additions with the row reduction, and the x-check are written once over
// it.  Host side: the device half of a per-(device, suite) cache of key tables -- the arena, the build
// stream and the table launches; which key gets which table, and when, is key_cache.h's KeyCacheBook.
#include <algorithm>
#include <atomic>
#include "ecc_device.h"
#include "key_cache.h"

namespace bcosgpu {

// per key slot: a 64-word header, then the comb table [32 windows][256 entries][x[8] y[8]]
//   header: [0..7] x, [8..15] y (canonical, plain), [16..23] Z_A (SM2: SM3 state words), [24..28] the
//   address right160(H(pub)) as the kernels store it (Keccak256 secp256k1 / SM3 SM2), [32] 1 = valid key
//   (coordinates < p, on the curve)
static constexpr size_t kKeyHdrWords = 64;
static constexpr size_t kKeySlotWords = kKeyHdrWords + kTabWords;
static constexpr int kKeyEntriesPerKey = kCombWindows * kCombEntries;  // 8192 table lanes per key

// SM2 Z_A = SM3(ENTL || ID || a || b || xG || yG || xA || yA): the key-independent 128-byte prefix is the
// constant midstate kZaMid, then two blocks (as sm2_e's first half)
__device__ __forceinline__ void sm2_za(uint32_t V[8], const fe& px, const fe& py) {
    uint32_t W[16], X[8], Y[8];  // the coordinates' big-endian words
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        V[i] = kZaMid[i];
        X[i] = px.v[7 - i];
        Y[i] = py.v[7 - i];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) W[j] = kZaW32[j];
    W[4] = kZaC36 | (X[0] >> 16);
#pragma unroll
    for (int j = 1; j < 8; ++j) W[4 + j] = (X[j - 1] << 16) | (X[j] >> 16);
    W[12] = (X[7] << 16) | (Y[0] >> 16);
#pragma unroll
    for (int j = 1; j < 4; ++j) W[12 + j] = (Y[j - 1] << 16) | (Y[j] >> 16);
    sm3_compress(V, W);
#pragma unroll
    for (int j = 0; j < 4; ++j) W[j] = (Y[j + 3] << 16) | (Y[j + 4] >> 16);
    W[4] = (Y[7] << 16) | 0x8000u;
#pragma unroll
    for (int j = 5; j < 15; ++j) W[j] = 0;
    W[15] = 210u * 8u;
    sm3_compress(V, W);
}

// e = SM3(Z_A || hash) (sm2_e's second half)
__device__ __forceinline__ void sm2_e_from_za(fe& e, const uint32_t* za, const fe& hash_be) {
#ifdef BCOSGPU_SM2_RAW_E
    // test seam, as in sm2_e (ecc_device.h): the digest itself, not reduced
    fe_copy(e, hash_be);
    return;
#endif
    uint32_t V[8], W[16];
    sm3_init(V);
#pragma unroll
    for (int j = 0; j < 8; ++j) W[j] = za[j];
#pragma unroll
    for (int j = 0; j < 8; ++j) W[8 + j] = hash_be.v[7 - j];
    sm3_compress(V, W);
#pragma unroll
    for (int j = 0; j < 16; ++j) W[j] = 0;
    W[0] = 0x80000000u;
    W[15] = 512u;
    sm3_compress(V, W);
#pragma unroll
    for (int i = 0; i < 8; ++i) e.v[i] = V[7 - i];
}

// ------------------------------------------------------------------ what a suite is made of
// F the field a point's coordinates live in (fe26: plain residues; fp26: the R' = 2^286 Montgomery form),
// Aff / Jac / C the points and curve operations over it.  Table entries are canonical words of the stored
// F value: plain for secp256k1, R'-form for SM2 (the layout of the fp26 G tables, tables_sm2_26): load_entry
// reads one (or a window's base, which has the same form), to_words writes one; from_plain takes a plain
// residue < 2^256 into F.
template <int SUITE>
struct KeyedSuite;
template <>
struct KeyedSuite<BCOSGPU_SUITE_SECP256K1> {
    using F = fe26;
    using Aff = Aff26;
    using Jac = Jac26;
    using C = CurveK1x;
    __device__ static __forceinline__ bool lt_p(const fe& a) { return fe_lt_k(a, FieldK1::P); }
    __device__ static __forceinline__ const uint32_t* order() { return ParamN1::M; }
    __device__ static __forceinline__ void from_plain(F& r, const fe& a) { fe26_from_fe(r, a); }  // a < 2^256
    __device__ static __forceinline__ void to_words(fe& r, const F& a) { fe26_to_fe(r, a); }
    __device__ static __forceinline__ void load_entry(Aff& T, const uint32_t* tab) { load_aff26(T, tab); }
    __device__ static __forceinline__ void sqr(F& r, const F& a) { fe26_sqr(r, a); }
    __device__ static __forceinline__ void mul(F& r, const F& a, const F& b) { fe26_mul(r, a, b); }
    __device__ static __forceinline__ bool is_zero(const F& a) { return fe26_is_zero(a); }
    // rhs - X of the x-check.  acc.X <= 10: an addition may pass a mixed sum through (9) or double (10)
    __device__ static __forceinline__ void sub_x(F& d, const F& rhs, const F& X) { fe26_sub<11>(d, rhs, X); }
    __device__ static __forceinline__ bool on_curve(const Aff& P) {  // y^2 = x^3 + 7
        fe26 l, rr, t, seven;
        fe26_sqr(l, P.y);
        fe26_sqr(t, P.x);
        fe26_mul(rr, t, P.x);
        fe26_set_small(seven, 7u);
        fe26_add(rr, rr, seven);
        fe26_sub<3>(l, l, rr);
        return fe26_is_zero(l);
    }
    __device__ static __forceinline__ void set_g(Aff& P) {
        fe26_const(P.x, kK1Gx);
        fe26_const(P.y, kK1Gy);
    }
    __device__ static __forceinline__ void inv(F& r, const F& z) {
        fe w, wi;
        fe26_to_fe(w, z);
        modinv_safegcd(wi, w, kMod30K1P);
        fe26_from_fe(r, wi);
    }
    // the header's Z_A (none) and address words
    __device__ static __forceinline__ void header(uint32_t za[8], uint32_t a[5], const fe& px, const fe& py) {
#pragma unroll
        for (int q = 0; q < 8; ++q) za[q] = 0;
        keccak_address(a, px, py);
    }
};
template <>
struct KeyedSuite<BCOSGPU_SUITE_SM2> {
    using F = fp26;
    using Aff = AffP26;
    using Jac = JacP26;
    using C = CurveSM2x;
    __device__ static __forceinline__ bool lt_p(const fe& a) { return fe_lt_k(a, ParamP2::M); }
    __device__ static __forceinline__ const uint32_t* order() { return ParamN2::M; }
    __device__ static __forceinline__ void from_plain(F& r, const fe& a) { fp26_from_plain(r, a); }
    __device__ static __forceinline__ void to_words(fe& r, const F& a) { fp26_to_fe(r, a); }
    __device__ static __forceinline__ void load_entry(Aff& T, const uint32_t* tab) { load_affp26(T, tab); }
    __device__ static __forceinline__ void sqr(F& r, const F& a) { fp26_sqr(r, a); }
    __device__ static __forceinline__ void mul(F& r, const F& a, const F& b) { fp26_mul(r, a, b); }
    __device__ static __forceinline__ bool is_zero(const F& a) { return fp26_is_zero(a); }
    // acc.X <= 12 (CurveSM2x::add)
    __device__ static __forceinline__ void sub_x(F& d, const F& rhs, const F& X) { fp26_sub<13>(d, rhs, X); }
    __device__ static __forceinline__ bool on_curve(const Aff& P) { return sm2_on_curve26(P); }
    __device__ static __forceinline__ void set_g(Aff& P) {
        fe gx, gy;
        fe_set(gx, kSM2Gx);  // Montgomery (R = 2^256) form: back to plain first
        fe_set(gy, kSM2Gy);
        FieldP2::to_plain(gx, gx);
        FieldP2::to_plain(gy, gy);
        fp26_from_plain(P.x, gx);
        fp26_from_plain(P.y, gy);
    }
    __device__ static __forceinline__ void inv(F& r, const F& z) { fp26_inv(r, z); }
    __device__ static __forceinline__ void header(uint32_t za[8], uint32_t a[5], const fe& px, const fe& py) {
        sm2_za(za, px, py);
        sm3_address(a, px, py);
    }
};

// ------------------------------------------------------------------ table build
// Two launches.  BASES: lane (key k, window i) computes the window's base 2^(8i) P (8i doublings, one
// inversion to affine) into `base`; then lane (key k, window i, entry b) computes b 2^(8i) P by an 8-bit
// double-and-add of that base and one inversion.  The chain of 8i doublings runs once per window instead
// of once per entry (the build's work ~5x smaller, its latency one short launch longer), so a promotion
// build beside live batches takes less of the GPU from them.  Entry 0 holds 1 2^(8i) P (a valid point the
// kernels never select).  An invalid key (coordinates >= p or off the curve) gets G's multiples and
// valid = 0, which makes every verify against it fail, as the reference's does.
template <int SUITE, bool BASES>
__global__ __launch_bounds__(256) void key_table_kernel(uint32_t* __restrict__ arena, const int32_t* __restrict__ slots,
                                                        const uint8_t* __restrict__ pubs, uint32_t nkeys,
                                                        uint32_t* __restrict__ base) {
    using S = KeyedSuite<SUITE>;
    using C = typename S::C;
    const uint64_t idx = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    constexpr uint64_t per = BASES ? kCombWindows : kKeyEntriesPerKey;
    if (idx >= static_cast<uint64_t>(nkeys) * per) return;
    const uint32_t k = static_cast<uint32_t>(idx / per);
    const uint32_t ent = BASES ? static_cast<uint32_t>(idx % per) * kCombEntries + 1u : static_cast<uint32_t>(idx % per);
    const int win = static_cast<int>(ent / kCombEntries);
    uint32_t b = ent % kCombEntries;
    if (b == 0) b = 1;
    uint32_t* slot = arena + static_cast<size_t>(slots[k]) * kKeySlotWords;
    uint32_t* bp = base + (static_cast<size_t>(k) * kCombWindows + win) * 16;  // the window's base (affine)
    uint32_t* out = BASES ? bp : slot + kKeyHdrWords + static_cast<size_t>(ent) * 16;
    fe px, py;
    load_be256(px, pubs + 64ull * k);
    load_be256(py, pubs + 64ull * k + 32);
    bool valid = S::lt_p(px) && S::lt_p(py);
    typename S::Aff P;
    S::from_plain(P.x, px);
    S::from_plain(P.y, py);
    valid = valid && S::on_curve(P);
    if (!BASES) {  // the window's base, G's multiple for an invalid key
        S::load_entry(P, bp);
    } else if (!valid) {
        S::set_g(P);
    }
    typename S::Jac acc, T;
    C::set_inf(acc);
#pragma unroll 1
    for (int bit = 7; bit >= 0; --bit) {
        C::dbl(acc, acc);
        C::madd(T, acc, P);
        C::cmov(acc, T, ((b >> bit) & 1u) != 0u);
    }
    if (BASES) {
#pragma unroll 1
        for (int d = 0; d < 8 * win; ++d) C::dbl(acc, acc);
    }
    typename S::F zi, zi2, zi3, ax, ay;
    S::inv(zi, acc.Z);
    S::sqr(zi2, zi);
    S::mul(zi3, zi2, zi);
    S::mul(ax, acc.X, zi2);
    S::mul(ay, acc.Y, zi3);
    fe x, y;
    S::to_words(x, ax);
    S::to_words(y, ay);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        out[q] = x.v[q];
        out[8 + q] = y.v[q];
    }
    if (!BASES && ent == 0) {
        uint32_t za[8], a[5];
        S::header(za, a, px, py);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            slot[q] = px.v[q];
            slot[8 + q] = py.v[q];
            slot[16 + q] = za[q];
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) slot[24 + q] = a[q];
        slot[32] = valid ? 1u : 0u;
    }
}

// ------------------------------------------------------------------ verify
// the 16-lane row's partial sums -> lane 0 (lanes of a row are 16-aligned: __shfl_down with width 16)
template <class J, int LIMBS>
__device__ __forceinline__ void shfl_down_point(J& o, const J& a, int off) {
#pragma unroll
    for (int q = 0; q < LIMBS; ++q) {
        o.X.v[q] = __shfl_down(a.X.v[q], off, 16);
        o.Y.v[q] = __shfl_down(a.Y.v[q], off, 16);
        o.Z.v[q] = __shfl_down(a.Z.v[q], off, 16);
    }
    o.inf = __shfl_down(static_cast<int>(a.inf), off, 16) != 0;
}

// word q of k for a lane-varying q, by selects (a dynamic index would put k in scratch memory)
__device__ __forceinline__ uint32_t word_of(const fe& k, int q) {
    uint32_t w = k.v[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) w = q == j ? k.v[j] : w;
    return w;
}
__device__ __forceinline__ uint32_t byte_of(const fe& k, int j) { return (word_of(k, j >> 2) >> ((j & 3) * 8)) & 0xffu; }
__device__ __forceinline__ uint32_t half_of(const fe& k, int j) { return (word_of(k, j >> 1) >> ((j & 1) * 16)) & 0xffffu; }

// acc += the comb entry at tab when its digit d != 0 (complete mixed addition)
template <class S>
__device__ __forceinline__ void keyed_add_entry(typename S::Jac& acc, const uint32_t* tab, uint32_t d) {
    typename S::Aff T;
    S::load_entry(T, tab);
    typename S::Jac R;
    S::C::madd(R, acc, T);
    S::C::cmov(acc, R, d != 0u);
}

// acc = kk P + kg G in lane 0 of the row: lane L adds windows 2L, 2L+1 of the key's comb ktab and its share of
// G's comb (window L of the 16-bit one, windows 2L, 2L+1 of the 8-bit one), then four levels of complete
// additions reduce the row
template <class S>
__device__ __forceinline__ void keyed_row_sum(typename S::Jac& acc, int L, const uint32_t* ktab, const fe& kk,
                                              const uint32_t* gtab, const fe& kg, int gbits) {
    using J = typename S::Jac;
    S::C::set_inf(acc);
    const uint32_t b0 = byte_of(kk, 2 * L), b1 = byte_of(kk, 2 * L + 1);
    keyed_add_entry<S>(acc, ktab + (static_cast<size_t>(2 * L) * kCombEntries + b0) * 16, b0);
    keyed_add_entry<S>(acc, ktab + (static_cast<size_t>(2 * L + 1) * kCombEntries + b1) * 16, b1);
    if (gbits == kWideBits) {
        const uint32_t g = half_of(kg, L);
        keyed_add_entry<S>(acc, gtab + (static_cast<size_t>(L) * kWideEntries + g) * 16, g);
    } else {
        const uint32_t g0 = byte_of(kg, 2 * L), g1 = byte_of(kg, 2 * L + 1);
        keyed_add_entry<S>(acc, gtab + (static_cast<size_t>(2 * L) * kCombEntries + g0) * 16, g0);
        keyed_add_entry<S>(acc, gtab + (static_cast<size_t>(2 * L + 1) * kCombEntries + g1) * 16, g1);
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
        J o;
        shfl_down_point<J, 10>(o, acc, off);
        S::C::add(acc, acc, o);
    }
}

// x1 = X / Z^2 congruent to c (mod n), without the inversion: X = c Z^2 or (c + n) Z^2 (when c + n < p)
template <class S>
__device__ __forceinline__ bool keyed_x_matches(const typename S::Jac& acc, const fe& c) {
    typename S::F z2, cm, rhs, d;
    S::sqr(z2, acc.Z);
    S::from_plain(cm, c);
    S::mul(rhs, cm, z2);
    S::sub_x(d, rhs, acc.X);
    bool match = S::is_zero(d);
    fe c2;
    const uint32_t carry = fe_add_k(c2, c, S::order());
    if (carry == 0u && S::lt_p(c2)) {
        S::from_plain(cm, c2);
        S::mul(rhs, cm, z2);
        S::sub_x(d, rhs, acc.X);
        match = match || S::is_zero(d);
    }
    return match;
}

// ok[i] = SignatureCrypto::verify(key of slot[i], hash[i], sig[i]); addr (SM2 tx admission: the verified
// key's SM3 address) may be null.  One 64-thread workgroup = 4 signatures.
template <int SUITE>
__global__ __launch_bounds__(64) void sig_verify_keyed_kernel(const uint32_t* __restrict__ arena, uint32_t cap,
                                                              uint32_t gen15, const int32_t* __restrict__ slots,
                                                              const uint8_t* __restrict__ hash,
                                                              const uint8_t* __restrict__ sig, uint32_t stride,
                                                              uint64_t n, const uint32_t* __restrict__ gtab, int gbits,
                                                              uint8_t* __restrict__ okout, uint8_t* __restrict__ addr) {
    using S = KeyedSuite<SUITE>;
    const uint32_t lane = threadIdx.x;
    const int L = static_cast<int>(lane & 15u);
    const uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * 4u + (lane >> 4);
    const bool live = i0 < n;
    const uint64_t i = live ? i0 : n - 1;  // a spare row re-runs the last signature (nothing stored)
    // a slot id is (generation << 16) | index (key_cache.h slot_id): an id handed out before a
    // bcosgpu_clear_keys names an old generation and fails here, even once its index holds another key's table
    const int32_t sl = slots[i];
    const uint32_t idx = static_cast<uint32_t>(sl) & 0xFFFFu;
    const bool slot_ok = sl >= 0 && (static_cast<uint32_t>(sl) >> 16) == gen15 && idx < cap;
    const uint32_t* key = arena + static_cast<size_t>(slot_ok ? idx : 0) * kKeySlotWords;
    const uint32_t* ktab = key + kKeyHdrWords;
    fe h;
    load_be256(h, hash + 32 * i);
    ByteReader rs(sig + static_cast<uint64_t>(stride) * i, 64);
    uint32_t w[8];
    fe r, s;
#pragma unroll
    for (int q = 0; q < 8; ++q) w[q] = rs.word(q);
    fe_from_be_words(r, w);
#pragma unroll
    for (int q = 0; q < 8; ++q) w[q] = rs.word(8 + q);
    fe_from_be_words(s, w);
    bool ok = slot_ok && key[32] == 1u;
    typename S::Jac acc;
    fe c;  // the x-check's residue mod n: r (secp256k1), r - e (SM2)
    if constexpr (SUITE == BCOSGPU_SUITE_SECP256K1) {
        ok = ok && !fe_is_zero_raw(r) && !fe_is_zero_raw(s) && fe_lt_k(r, ParamN1::M) && fe_lt_k(s, kN1HalfPlus);
        fe e;
        fe_copy(e, h);
        reduce_once(e, ParamN1::M);
        fe ss = s;
        if (!ok) {
            fe_zero(ss);
            ss.v[0] = 1;
        }
        fe sm, sinv, u1, u2;
        FieldN1::from_plain(sm, ss);
        FieldInv<FieldN1>::inv_pipe(sinv, sm);
        FieldN1::mul(u1, e, sinv);
        FieldN1::mul(u2, r, sinv);
        keyed_row_sum<S>(acc, L, ktab, u2, gtab, u1, gbits);
        c = r;
    } else {
        ok = ok && !fe_is_zero_raw(r) && !fe_is_zero_raw(s) && fe_lt_k(r, ParamN2::M) && fe_lt_k(s, ParamN2::M);
        fe t;
        FieldN2::add(t, r, s);
        ok = ok && !fe_is_zero_raw(t);
        fe e;
        sm2_e_from_za(e, key + 16, h);
        reduce_once(e, ParamN2::M);
        keyed_row_sum<S>(acc, L, ktab, t, gtab, s, gbits);
        FieldN2::sub(c, r, e);
    }
    ok = ok && !acc.inf && keyed_x_matches<S>(acc, c);
    if (live && L == 0) {
        okout[i] = ok ? 1 : 0;
        if (addr) {
            uint32_t* a = reinterpret_cast<uint32_t*>(addr + 20 * i);
#pragma unroll
            for (int q = 0; q < 5; ++q) a[q] = ok ? key[24 + q] : 0u;
        }
    }
}

// the table kernel of a suite (the two have one signature): for the launches and the code-object warm-up
template <bool BASES>
auto table_kernel_of(int suite) {
    return suite == BCOSGPU_SUITE_SM2 ? &key_table_kernel<BCOSGPU_SUITE_SM2, BASES>
                                      : &key_table_kernel<BCOSGPU_SUITE_SECP256K1, BASES>;
}

// ------------------------------------------------------------------ host: the device half of the key cache
namespace {

struct KeyCache {
    std::mutex mu;
    std::mutex init_mu;              // prepare_promotion
    std::atomic<bool> ready{false};  // ... has run
    KeyCacheBook book;               // under mu: every decision (key_cache.h)
    uint32_t* arena = nullptr;       // book.cap key slots
    bool alloc_failed = false;
    // the one promotion build in flight (book.building): on its own lowest-priority stream, published by the
    // first cache call after its event completes (poll_build)
    hipStream_t build_stream = nullptr;
    hipEvent_t build_done = nullptr;
    std::vector<uint8_t> build_host;  // the build's upload source, alive until the build completes
    // the builds' key / slot upload buffer, grow-only: a build under mu costs its upload, the table kernel
    // and one stream sync, not a hipMalloc + hipFree (a hipFree can wait for the whole device)
    uint8_t* scratch = nullptr;
    size_t scratch_cap = 0;
    KeyCache(int cap, int promote_after) : book(cap, promote_after) {}
};

int capacity_env() {
    const char* e = getenv("BCOSGPU_KEY_CACHE");  // keys per (device, suite); 512 KiB each
    const long v = e ? atol(e) : 256;
    return static_cast<int>(v < 0 ? 0 : v > 65536 ? 65536 : v);
}
int promote_after_env() {
    // calls that must see a key before it is cached (0 = never).  3: a sealer's key is cached by its
    // third block, while admission traffic over many distinct keys (each seen once or twice) does not
    // fill the cache with one-off keys
    const char* e = getenv("BCOSGPU_KEY_PROMOTE");
    return e ? atoi(e) : 3;
}

// The cache of (device, suite), device < 0 = the current one; null for a device out of range.
KeyCache* cache_of(int device, int suite) {
    static std::mutex mu;
    static KeyCache* all[64][2] = {};  // never freed: no teardown races with the HIP runtime at exit
    static const int cap = capacity_env(), after = promote_after_env();  // read once
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return nullptr;
    if (device < 0 || device >= 64) return nullptr;
    std::lock_guard<std::mutex> g(mu);
    KeyCache*& c = all[device][suite == BCOSGPU_SUITE_SM2 ? 1 : 0];
    if (!c) c = new KeyCache(cap, after);
    return c;
}

// The key arena of `cap` tables, or null.
uint32_t* alloc_arena(int cap) {
    uint32_t* arena = nullptr;
    if (cap > 0 && hipMalloc(&arena, static_cast<size_t>(cap) * kKeySlotWords * 4) == hipSuccess) return arena;
    (void)hipGetLastError();
    return nullptr;
}
// Under c.mu: the arena, allocated on first use.
void ensure_arena(KeyCache& c) {
    if (c.arena || c.alloc_failed) return;
    c.arena = alloc_arena(c.book.cap);
    c.alloc_failed = !c.arena;
}

// Under c.mu on the current device: build the tables of b.keys at arena indices b.idx on st -- with
// `async`, record c.build_done after it and return (c.build_host keeps the upload's source), else
// synchronise st.  One build uses c.scratch at a time: an async one is in flight only while
// c.book.building, and a synchronous one (registration) first waits for it.
int build_tables(KeyCache& c, int suite, const KeyBuild& b, hipStream_t st, bool async) {
    const size_t kb = 64 * b.keys.size(), sb = 4 * b.idx.size();
    const size_t bo = (kb + sb + 255) & ~size_t{255}, bb = 64ull * kCombWindows * b.keys.size();  // window bases
    std::vector<uint8_t>& host = c.build_host;
    host.resize(kb + sb);
    for (size_t q = 0; q < b.keys.size(); ++q) std::memcpy(host.data() + 64 * q, b.keys[q].data(), 64);
    std::memcpy(host.data() + kb, b.idx.data(), sb);
    hipError_t e = hipSuccess;
    if (c.scratch_cap < bo + bb) {
        if (c.scratch) (void)hipFree(c.scratch);
        c.scratch = nullptr;
        c.scratch_cap = 0;
        const size_t want = std::max<size_t>(bo + bb, 256 + (64 * kCombWindows + 68) * 16);
        e = hipMalloc(reinterpret_cast<void**>(&c.scratch), want);
        if (e == hipSuccess) c.scratch_cap = want;
        else c.scratch = nullptr;
    }
    uint8_t* d = c.scratch;
    if (e == hipSuccess) e = hipMemcpyAsync(d, host.data(), kb + sb, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        const uint64_t nk = b.keys.size(), lanes1 = nk * kCombWindows, lanes2 = nk * kKeyEntriesPerKey;
        const dim3 g1(static_cast<unsigned>((lanes1 + 255) / 256)), g2(static_cast<unsigned>((lanes2 + 255) / 256));
        const int32_t* ds = reinterpret_cast<const int32_t*>(d + kb);
        uint32_t* db = reinterpret_cast<uint32_t*>(d + bo);
        hipLaunchKernelGGL(table_kernel_of<true>(suite), g1, dim3(256), 0, st, c.arena, ds, d,
                           static_cast<uint32_t>(nk), db);
        hipLaunchKernelGGL(table_kernel_of<false>(suite), g2, dim3(256), 0, st, c.arena, ds, d,
                           static_cast<uint32_t>(nk), db);
        e = hipGetLastError();
        const hipError_t e2 = async ? hipEventRecord(c.build_done, st) : hipStreamSynchronize(st);
        if (e == hipSuccess) e = e2;
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return BCOSGPU_E_HIP;
    }
    return 0;
}

// Outside c.mu, once per cache: what the first promotion needs -- the arena, the build stream and event,
// and the code object holding the table kernel (HIP loads it on first use, ~10 ms) -- so that no lookup
// waits behind these one-time costs.  Failures leave promotion off (build_stream null).
void prepare_promotion(KeyCache& c, int suite) {
    std::unique_lock<std::mutex> i(c.init_mu, std::try_to_lock);  // another caller preparing: skip, this
    if (!i.owns_lock() || c.ready.load(std::memory_order_acquire)) return;  // call does not promote
    bool need_arena;
    {
        std::lock_guard<std::mutex> g(c.mu);
        need_arena = !c.arena && !c.alloc_failed;
    }
    uint32_t* arena = need_arena ? alloc_arena(c.book.cap) : nullptr;
    hipStream_t s = nullptr;
    hipEvent_t ev = nullptr;
    hipFuncAttributes fa;
    int least = 0, greatest = 0;
    const bool ok = hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess &&
                    hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least) == hipSuccess &&
                    hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess &&
                    hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(table_kernel_of<true>(suite))) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    {
        std::lock_guard<std::mutex> g(c.mu);
        if (need_arena && !c.arena && arena) {
            c.arena = arena;
            arena = nullptr;
        } else if (need_arena && !c.arena) {
            c.alloc_failed = true;
        }
        if (ok) {
            c.build_stream = s;
            c.build_done = ev;
        }
    }
    if (arena) (void)hipFree(arena);  // a registration allocated the arena meanwhile
    c.ready.store(true, std::memory_order_release);
}

// Under c.mu: publish the promotion build in flight once it has completed (`wait`: block until then);
// a failed one publishes nothing.
void poll_build(KeyCache& c, bool wait) {
    if (!c.book.building) return;
    const hipError_t q = wait ? hipEventSynchronize(c.build_done) : hipEventQuery(c.build_done);
    if (q == hipErrorNotReady) return;
    c.book.build_finished(q == hipSuccess);
    if (q != hipSuccess) (void)hipGetLastError();
}

}  // namespace

// bcosgpu_register_keys on the current device: slot ids of the n keys at pubs + 64 i, every key without a
// table built now, synchronously, so the ids name built tables (-1: the cache is full).  Returns 0 or < 0.
int keyed_register(int suite, const uint8_t* pubs, size_t n, int32_t* out) {
    KeyCache* c = cache_of(-1, suite);
    if (!c) return BCOSGPU_E_NODEV;
    if (n == 0) return 0;
    std::lock_guard<std::mutex> g(c->mu);
    poll_build(*c, true);  // a registration reuses the scratch buffer: the build in flight finishes first
    ensure_arena(*c);
    const KeyBuild b = c->book.plan_registration(pubs, 64, n, out, c->arena != nullptr);
    if (!b.keys.empty())
        if (int rc = build_tables(*c, suite, b, nullptr, false)) return rc;
    c->book.registration_done(b, pubs, 64, n, out);
    return 0;
}

// The coalesced verify calls on the current device: slot ids of the n keys at pubs + pub_stride i, *all =
// every key has a table, *gen the cache generation the ids belong to.  Never waits: a call that names its
// keys (`named`) may start one asynchronous build on the cache's own lowest-priority stream, and takes the
// generic kernels until that is published (a build is ~0.9 ms, latency-bound, whatever its key count:
// profiles/r06_tail_ab.json).  Returns 0 or < 0.
int keyed_lookup(int suite, const uint8_t* pubs, size_t pub_stride, size_t n, int32_t* out, bool named, bool* all,
                 uint64_t* gen) {
    KeyCache* c = cache_of(-1, suite);
    if (!c) return BCOSGPU_E_NODEV;
    *all = n == 0;
    if (n == 0) return 0;
    named = named && c->book.promote_after > 0;
    if (named && !c->ready.load(std::memory_order_acquire)) prepare_promotion(*c, suite);
    std::lock_guard<std::mutex> g(c->mu);
    poll_build(*c, false);
    *gen = c->book.gen;
    KeyBuild b;
    *all = c->book.lookup(pubs, pub_stride, n, out, named && c->build_stream && c->arena, b);
    if (!b.keys.empty() && build_tables(*c, suite, b, c->build_stream, true) == 0) c->book.build_started(b);
    return 0;
}

int launch_sig_verify_keyed(int suite, const int32_t* d_slots, const uint8_t* d_hash, const uint8_t* d_sig,
                            uint32_t stride, uint64_t n, uint8_t* d_ok, uint8_t* d_addr, hipStream_t st) {
    if (n == 0) return 0;
    KeyCache* c = cache_of(-1, suite);
    if (!c) return BCOSGPU_E_NODEV;
    const uint32_t* arena;
    uint32_t cap, gen15;
    {
        std::lock_guard<std::mutex> g(c->mu);
        arena = c->arena;
        cap = static_cast<uint32_t>(c->book.next);  // a batch holds published ids only; pending ones are below next
        gen15 = gen_tag(c->book.gen);
    }
    if (!arena) return BCOSGPU_E_ARG;  // no key registered on this device
    const bool sm2 = suite == BCOSGPU_SUITE_SM2;
    const uint32_t *gtab = nullptr, *other = nullptr;  // G's comb in the suite's field
    int bits;
    if (int rc = sm2 ? tables_sm2_26(&gtab, &bits) : tables(&gtab, &other, &bits)) return rc;
    hipLaunchKernelGGL(sm2 ? &sig_verify_keyed_kernel<BCOSGPU_SUITE_SM2> : &sig_verify_keyed_kernel<BCOSGPU_SUITE_SECP256K1>,
                       dim3(static_cast<unsigned>((n + 3) / 4)), dim3(64), 0, st, arena, cap, gen15, d_slots, d_hash, d_sig,
                       stride, n, gtab, bits, d_ok, d_addr);
    return hipGetLastError() == hipSuccess ? 0 : BCOSGPU_E_HIP;
}

uint64_t keyed_generation(int suite) {
    KeyCache* c = cache_of(-1, suite);
    if (!c) return ~0ull;
    std::lock_guard<std::mutex> g(c->mu);
    return c->book.gen;
}

int keyed_cache_info(int device, int suite, int64_t out[5]) {
    KeyCache* c = device < 0 ? nullptr : cache_of(device, suite);
    if (!c) return BCOSGPU_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    poll_build(*c, false);
    c->book.info(out);
    return 0;
}

// Drop every cached key of (device, suite) after the device has drained (no launch reads a table then, and
// a build in flight has completed: it is dropped unpublished).
int keyed_clear(int device, int suite) {
    KeyCache* c = device < 0 ? nullptr : cache_of(device, suite);
    if (!c) return BCOSGPU_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    DeviceScope on(device);
    if (on.err != hipSuccess || hipDeviceSynchronize() != hipSuccess) return BCOSGPU_E_HIP;
    c->book.clear();
    return 0;
}

}  // namespace bcosgpu
