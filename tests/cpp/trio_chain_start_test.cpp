// trio_chain_start_test.cpp -- host build (FE26_CHECK) of the lane-trio kernel's chain start
// (trio_chain_start, ec26_trio.h): the two top Booth digits of a 128-bit GLV half taken together,
// t = 16 d32 + d31 = 2a + b, as a R from the table, one doubling and one addition of b R.
//  (a) the digits: for every scalar below, t 2^124 plus the radix-16 Booth digits 30..0 of the scalar
//      shifted left by four bits (what booth_digit128 goes on with) is the scalar again;
//  (b) the start as a point, against the start it replaces -- the top digit added onto infinity
//      (trio_madd<false>), then a whole window (three trio_dbl, trio_dbl_zz, trio_madd_zz) -- and against
//      t additions of the signed R on one lane (CurveK1x::madd).  The 16 lanes of one DPP row run as
//      lockstep threads (as tests/cpp/trio_test.cpp), so every field operation asserts its magnitude
//      contract on every lane, and the start's stated output magnitudes are checked as well.  Cases: every
//      t in 0..16, reached both ways (bit 123 clear and set), with random low bits, for both chains (phi
//      off and on) and both signs; and k = 0, k = 1, k = 2^128 - 1;
//  (c) whole chains (start + 31 windows) for k = 0, 1, 2^128 - 1, a t = 16 scalar and a random one, against
//      a one-lane double-and-add.
// Prints "chain start ok <cases>" and exits 0, or the first mismatch and exits 1.
#define FE26_CHECK 1
#include "../../fisco-bcos_amd/csrc/ec26_trio.h"

#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

using namespace bcosgpu;

namespace {
constexpr int kLanes = 16;
std::mutex mu;
std::condition_variable cv;
int arrived = 0;
unsigned long generation = 0;
uint32_t slot[kLanes];
thread_local int my_lane = 0;

void barrier() {
    std::unique_lock<std::mutex> lk(mu);
    const unsigned long g = generation;
    if (++arrived == kLanes) {
        arrived = 0;
        ++generation;
        cv.notify_all();
    } else {
        cv.wait(lk, [&] { return generation != g; });
    }
}
}  // namespace

namespace bcosgpu {
uint32_t trio_emu_dpp(uint32_t x, int ctrl) {
    slot[my_lane] = x;
    barrier();
    int src = my_lane;
    switch (ctrl) {
        case 0x111: src = my_lane - 1; break;  // row_shr:1
        case 0x112: src = my_lane - 2; break;  // row_shr:2
        case 0x101: src = my_lane + 1; break;  // row_shl:1
        case 0x102: src = my_lane + 2; break;  // row_shl:2
        default: abort();
    }
    const uint32_t r = (src >= 0 && src < kLanes) ? slot[src] : 0u;
    barrier();
    return r;
}
bool trio_emu_any(bool b) {
    slot[my_lane] = b ? 1u : 0u;
    barrier();
    bool r = false;
    for (int i = 0; i < kLanes; ++i) r = r || slot[i] != 0u;
    barrier();
    return r;
}
}  // namespace bcosgpu

namespace {
typedef unsigned __int128 u128;

uint64_t rng_state = 0x2545f4914f6cdd1dull;
uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return static_cast<uint32_t>(rng_state >> 11);
}
u128 rnd128() {
    u128 r = 0;
    for (int i = 0; i < 6; ++i) r = (r << 24) ^ rnd();
    return r;
}
void rand_fe(fe26& a) {
    for (int i = 0; i < 10; ++i) a.v[i] = (static_cast<uint64_t>(rnd()) << 20 ^ rnd()) & ((i == 9 ? 1u << 22 : 1u << 26) - 1u);
    a.m = 1;
}
bool same(const fe26& a, const fe26& b) {
    fe26 x = a, y = b;
    fe26_normalize(x);
    fe26_normalize(y);
    return memcmp(x.v, y.v, sizeof x.v) == 0;
}
bool same_point(const Jac26& a, const Jac26& b) {
    if (a.inf || b.inf) return a.inf == b.inf;
    fe26 za2, zb2, za3, zb3, l, r;
    fe26_sqr(za2, a.Z);
    fe26_sqr(zb2, b.Z);
    fe26_mul(l, a.X, zb2);
    fe26_mul(r, b.X, za2);
    if (!same(l, r)) return false;
    fe26_mul(za3, za2, a.Z);
    fe26_mul(zb3, zb2, b.Z);
    fe26_mul(l, a.Y, zb3);
    fe26_mul(r, b.Y, za3);
    return same(l, r);
}
// an affine point of E: y^2 = x^3 + 7
void rand_point(Aff26& P) {
    for (;;) {
        fe26 t, rhs, seven;
        rand_fe(P.x);
        fe26_sqr(t, P.x);
        fe26_mul(rhs, t, P.x);
        fe26_set_small(seven, 7u);
        fe26_add(rhs, rhs, seven);
        fe26_sqrt_cand(P.y, rhs);
        fe26_sqr(t, P.y);
        if (same(t, rhs)) {
            fe26_normalize(P.y);
            return;
        }
    }
}
// a^(p - 2), p = 2^256 - 2^32 - 977
void inv(fe26& r, const fe26& a) {
    static const uint32_t e[8] = {0xfffffc2du, 0xfffffffeu, 0xffffffffu, 0xffffffffu,
                                  0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    fe26 x;
    fe26_one(x);
    for (int i = 255; i >= 0; --i) {
        fe26_sqr(x, x);
        if ((e[i >> 5] >> (i & 31)) & 1u) fe26_mul(x, x, a);
    }
    r = x;
}
void to_aff(Aff26& A, const Jac26& J) {
    fe26 zi, zi2, zi3;
    inv(zi, J.Z);
    fe26_sqr(zi2, zi);
    fe26_mul(zi3, zi2, zi);
    fe26_mul(A.x, J.X, zi2);
    fe26_mul(A.y, J.Y, zi3);
    fe26_normalize(A.x);
    fe26_normalize(A.y);
}

// the kernel's table of a tx: (j + 1) R, j = 0..7, affine and canonical (m 1), and beta x beside it
struct Table {
    Aff26 e[8];
    fe26 phx[8];
};
fe26 beta;
void make_table(Table& Tb, const Aff26& R) {
    Jac26 acc;
    CurveK1x::from_aff(acc, R);
    Tb.e[0] = R;
    for (int j = 1; j < 8; ++j) {
        CurveK1x::madd(acc, acc, R);  // (doubles when acc = R)
        to_aff(Tb.e[j], acc);
    }
    for (int j = 0; j < 8; ++j) {
        fe26_mul(Tb.phx[j], Tb.e[j].x, beta);
        fe26_normalize(Tb.phx[j]);
    }
}
// the lookup of ecc_coop.hip's trio_entry, on the host table
void entry(Aff26& S, const Table& Tb, int d, bool neg, bool phi) {
    const uint32_t m = static_cast<uint32_t>((d < 0 ? -d : d) - 1) & 7u;
    S.x = phi ? Tb.phx[m] : Tb.e[m].x;
    S.y = Tb.e[m].y;
    F26_SETM(S.x, 1);
    F26_SETM(S.y, 1);
    fe26 ny;
    fe26_neg<2>(ny, S.y);
    fe26_cmov(S.y, ny, (d < 0) != neg);
}

// the radix-16 Booth digit of the top of k, and k <- k << 4 (ecc_device.h's booth_digit128)
int booth_digit(u128& k) {
    const uint32_t top = static_cast<uint32_t>(k >> 96);
    const uint32_t W = top >> 28, c = (top >> 27) & 1u;
    k <<= 4;
    return static_cast<int>(W + c) - static_cast<int>((W >> 3) << 4);
}

struct Case {
    u128 k;
    bool neg, phi;
    int tab;  // which table
};
std::vector<Table> tables;
std::vector<Case> cases;
std::vector<int> bad;
constexpr int cases_per_round = 5;

void add_digit_zz(TrioPt& acc, const Table& Tb, int d, bool neg, bool phi, const fe26& zz, const TrioLane& T) {
    Aff26 S;
    entry(S, Tb, d, neg, phi);
    TrioPt R;
    trio_madd_zz(R, acc, zz, S, T);
    trio_cmov(acc, R, d != 0);
}
void window(TrioPt& acc, const Table& Tb, u128& k, bool neg, bool phi, const TrioLane& T) {
    fe26 zz;
    for (int q = 0; q < 3; ++q) trio_dbl(acc, T);
    trio_dbl_zz(acc, zz, T);
    add_digit_zz(acc, Tb, booth_digit(k), neg, phi, zz, T);
}
// one lane: acc <- 16 acc + d (signed R)
void ref_window(Jac26& acc, const Table& Tb, int d, bool neg, bool phi) {
    for (int q = 0; q < 4; ++q) CurveK1x::dbl(acc, acc);
    Aff26 S;
    entry(S, Tb, d < 0 ? -1 : 1, neg, phi);
    fe26_normalize(S.y);
    for (int j = 0; j < (d < 0 ? -d : d); ++j) CurveK1x::madd(acc, acc, S);
}

void lane_main(int lane, int round, bool whole) {
    my_lane = lane;
    const TrioLane T(lane);
    const int t5 = (lane % 16) / 3;
    const int c = round * cases_per_round + (t5 < 5 ? t5 : 4);
    const Case& C = cases[c];
    const Table& Tb = tables[C.tab];
    const uint32_t top = static_cast<uint32_t>(C.k >> 96);
    // the new start
    TrioPt acc;
    trio_chain_start(acc, top, [&](Aff26& S, int d) { entry(S, Tb, d, C.neg, C.phi); }, T);
    const uint32_t t = (top >> 28) + ((top >> 27) & 1u);
    // the stated output magnitudes, those of a window's end (S1 is (X | Y | Y); X and Z live on lane 2)
    if (acc.S1.m > 10 || (T.r2 && (acc.Xs.m > 10 || acc.Zs.m > 2))) bad[c] = 5;
    // the start it replaces: digit 32 onto infinity, then a whole window with digit 31
    TrioPt old;
    u128 ko = C.k;
    {
        const int d32 = static_cast<int>(top >> 31);
        Aff26 S;
        entry(S, Tb, d32, C.neg, C.phi);
        TrioPt R;
        trio_set_inf(old);
        trio_madd<false>(R, old, S, T);
        trio_cmov(old, R, d32 != 0);
        window(old, Tb, ko, C.neg, C.phi, T);
    }
    // one lane: t times the signed R
    Jac26 ref;
    CurveK1x::set_inf(ref);
    {
        Aff26 S;
        entry(S, Tb, 1, C.neg, C.phi);
        fe26_normalize(S.y);
        for (uint32_t j = 0; j < t; ++j) CurveK1x::madd(ref, ref, S);
    }
    Jac26 jn, jo;
    trio_to_jac(jn, acc, T);
    trio_to_jac(jo, old, T);
    const bool real = T.r2 && t5 < 5;
    if (real) {
        if ((t == 0) != acc.inf) bad[c] = 1;
        else if (!same_point(jn, jo)) bad[c] = 2;
        else if (!same_point(jn, ref)) bad[c] = 3;
    }
    if (!whole) return;
    // (c) the rest of the chain: 31 windows, booth_digit128's state after the start being k << 4
    u128 kn = C.k << 4, kr = C.k << 4;
    for (int w = 30; w >= 0; --w) {
        window(acc, Tb, kn, C.neg, C.phi, T);
        ref_window(ref, Tb, booth_digit(kr), C.neg, C.phi);
    }
    // and a plain double-and-add of k on one lane
    Jac26 dn;
    CurveK1x::set_inf(dn);
    {
        Aff26 S;
        entry(S, Tb, 1, C.neg, C.phi);
        fe26_normalize(S.y);
        for (int i = 127; i >= 0; --i) {
            CurveK1x::dbl(dn, dn);
            if ((C.k >> i) & 1u) CurveK1x::madd(dn, dn, S);
        }
    }
    trio_to_jac(jn, acc, T);
    if (real) {
        if (!same_point(ref, dn)) bad[c] = 6;
        else if (!same_point(jn, dn)) bad[c] = 4;
    }
}

// (a): t 2^124 + sum d_i 16^i (i = 30..0, the digits of k << 4) = k, modulo 2^128 and with the signed sum
// of the 31 low digits in (-2^124, 2^124], which makes it an identity of integers (t 2^124 <= 2^128)
bool check_digits(u128 k) {
    const uint32_t top = static_cast<uint32_t>(k >> 96);
    const u128 t = (top >> 28) + ((top >> 27) & 1u);
    u128 s = k << 4, low = 0;
    bool lowneg = false;
    __int128 sl = 0;
    for (int i = 30; i >= 0; --i) {
        const int d = booth_digit(s);
        if (d < -8 || d > 8) return false;
        sl = sl * 16 + d;
    }
    lowneg = sl < 0;
    low = lowneg ? static_cast<u128>(-sl) : static_cast<u128>(sl);
    const u128 one124 = static_cast<u128>(1) << 124;
    if (low > one124) return false;
    const u128 hi = t << 124;  // t = 16 wraps to 0: then the low part must be negative or the scalar 0
    const u128 sum = lowneg ? hi - low : hi + low;
    if (t == 16 && !lowneg) return false;
    return sum == k;
}
}  // namespace

int main() {
    {
        static const uint32_t bw[8] = {0x719501eeu, 0xc1396c28u, 0x12f58995u, 0x9cf04975u,
                                       0xac3434e9u, 0x6e64479eu, 0x657c0710u, 0x7ae96a2bu};
        fe26_from_words(beta, bw);
        fe26 b3;
        fe26_sqr(b3, beta);
        fe26_mul(b3, b3, beta);
        fe26 one;
        fe26_one(one);
        if (!same(b3, one)) { printf("beta^3 != 1\n"); return 1; }
    }
    for (int j = 0; j < 4; ++j) {
        Aff26 R;
        rand_point(R);
        Table Tb;
        make_table(Tb, R);
        tables.push_back(Tb);
    }
    const u128 all = ~static_cast<u128>(0);
    int n = 0;
    // every t both ways: (nibble W, bit 123 = c), t = W + c
    for (int W = 0; W < 16; ++W)
        for (int c = 0; c < 2; ++c)
            for (int f = 0; f < 4; ++f) {
                const u128 lowbits = rnd128() & ((static_cast<u128>(1) << 123) - 1);
                const u128 k = (static_cast<u128>(W) << 124) | (static_cast<u128>(c) << 123) | lowbits;
                cases.push_back(Case{k, (f & 1) != 0, (f & 2) != 0, n++ % 4});
            }
    // k = j 2^123 exactly (no low bits)
    for (int j = 1; j < 32; j += 5)
        cases.push_back(Case{static_cast<u128>(j) << 123, (j & 1) != 0, (j & 2) != 0, n++ % 4});
    for (int f = 0; f < 4; ++f) {
        cases.push_back(Case{0, (f & 1) != 0, (f & 2) != 0, n++ % 4});
        cases.push_back(Case{1, (f & 1) != 0, (f & 2) != 0, n++ % 4});
        cases.push_back(Case{all, (f & 1) != 0, (f & 2) != 0, n++ % 4});
    }
    while (cases.size() % cases_per_round) cases.push_back(Case{rnd128(), false, true, n++ % 4});
    const size_t start_cases = cases.size();
    // (c): one round of whole chains
    cases.push_back(Case{0, false, false, 0});
    cases.push_back(Case{1, true, true, 1});
    cases.push_back(Case{all, false, true, 2});
    cases.push_back(Case{(static_cast<u128>(0xf8) << 120) | (rnd128() >> 8), true, false, 3});  // t = 16
    cases.push_back(Case{rnd128(), false, true, 0});
    bool seen[17] = {};
    for (const Case& C : cases) {
        if (!check_digits(C.k)) {
            printf("digits do not sum to k: top word %08x\n", static_cast<uint32_t>(C.k >> 96));
            return 1;
        }
        const uint32_t top = static_cast<uint32_t>(C.k >> 96);
        seen[(top >> 28) + ((top >> 27) & 1u)] = true;
    }
    for (int t = 0; t <= 16; ++t)
        if (!seen[t]) { printf("t = %d not covered\n", t); return 1; }
    bad.assign(cases.size(), 0);
    const int rounds = static_cast<int>(cases.size()) / cases_per_round;
    for (int r = 0; r < rounds; ++r) {
        const bool whole = static_cast<size_t>(r) * cases_per_round >= start_cases;
        std::vector<std::thread> th;
        for (int l = 0; l < kLanes; ++l) th.emplace_back(lane_main, l, r, whole);
        for (auto& x : th) x.join();
    }
    int nbad = 0;
    for (size_t i = 0; i < bad.size(); ++i)
        if (bad[i]) {
            if (!nbad)
                printf("chain start mismatch in case %zu (kind %d: 1 infinity flag, 2 against the old start, 3 against "
                       "t additions, 4 whole chain, 5 magnitude, 6 reference), top word %08x neg %d phi %d\n",
                       i, bad[i], static_cast<uint32_t>(cases[i].k >> 96), cases[i].neg, cases[i].phi);
            ++nbad;
        }
    if (nbad) {
        printf("chain start mismatches %d of %zu\n", nbad, cases.size());
        return 1;
    }
    printf("chain start ok %zu starts (t = 0..16, both chains, both signs) + %zu whole chains\n", start_cases,
           cases.size() - start_cases);
    return 0;
}
