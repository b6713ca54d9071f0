// trio_window_test.cpp -- host build (FE26_CHECK) of the lane-trio kernel's lean window (trio_window,
// ec26_trio.h: trio_dbln<0> .. trio_dbln<3>, trio_maddq_zz on a TrioAcc).  The 16 lanes of one DPP row run
// as lockstep threads (as tests/cpp/trio_test.cpp), so every field operation asserts its magnitude contract
// and every limb bound on every lane, and the window's stated output magnitudes are checked as well.
//  (a) windows, chained 32 deep so that a window's output is the next one's input, each compared by
//      projective equality with the window it replaces (three trio_dbl, trio_dbl_zz, trio_madd_zz, trio_cmov)
//      and with four CurveK1x::dbl and a CurveK1x::madd on one lane.  Inputs: random Jacobian points, and the
//      same points with multiples of p added to the limbs up to the entry contract's bounds (X, Y, Z at
//      magnitude 16 for the lean window; (10, 10, 16), the old window's contract, for the old one).  Digits:
//      every value in -8..8, both chains (phi off and on), both signs.  The accumulator starts infinite on
//      none, some and all of the row's trios, with runs of zero digits of different lengths before the first
//      addition, so the wave-uniform infinity branch is taken and not taken;
//  (b) trio_chain_start followed by two lean windows, for every t in 0..16 (an odd number of doublings
//      before the first window), against one lane;
//  (c) whole 128-bit chains (start + 31 lean windows) against a one-lane double-and-add: k = 0, 1,
//      2^128 - 1, a scalar with a run of zero digits, a random scalar.
// Prints "trio window ok ..." and exits 0, or the first mismatch and exits 1.
#define FE26_CHECK 1
#include "../../fisco-bcos_amd/csrc/ec26_trio.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

using namespace bcosgpu;

namespace {
constexpr int kLanes = 16;
// a sense-reversing barrier that yields while it waits (a window is some 800 of them: a condition
// variable's sleep and wake-up per barrier made the test take half a minute)
std::atomic<int> arrived{0};
std::atomic<unsigned long> generation{0};
uint32_t slot[kLanes];
thread_local int my_lane = 0;

void barrier() {
    const unsigned long g = generation.load(std::memory_order_acquire);
    if (arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == kLanes) {
        arrived.store(0, std::memory_order_relaxed);
        generation.store(g + 1, std::memory_order_release);
    } else {
        while (generation.load(std::memory_order_acquire) == g) std::this_thread::yield();
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

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
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
    fe26 za2, zb2, za3, zb3, l, r, zero;
    fe26_zero(zero);
    if (same(a.Z, zero) || same(b.Z, zero)) return false;
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

// the window that the lean one replaced (trio_dbl x 3, trio_dbl_zz, trio_madd_zz: removed from ecc_coop.hip)
void old_window(TrioPt& acc, const Table& Tb, int d, bool neg, bool phi, const TrioLane& T) {
    fe26 zz;
    for (int q = 0; q < 3; ++q) trio_dbl(acc, T);
    trio_dbl_zz(acc, zz, T);
    Aff26 S;
    entry(S, Tb, d, neg, phi);
    TrioPt R;
    trio_madd_zz(R, acc, zz, S, T);
    trio_cmov(acc, R, d != 0);
}
void lean_window(TrioAcc& acc, const Table& Tb, int d, bool neg, bool phi, const TrioLane& T) {
    trio_window(acc, d, [&](Aff26& S, int dd) { entry(S, Tb, dd, neg, phi); }, T);
}
// one lane: acc <- 16 acc + d (signed table point)
void ref_window(Jac26& acc, const Table& Tb, int d, bool neg, bool phi) {
    for (int q = 0; q < 4; ++q) CurveK1x::dbl(acc, acc);
    if (d == 0) return;
    Aff26 S;
    entry(S, Tb, d, neg, phi);
    fe26_normalize(S.y);
    CurveK1x::madd(acc, acc, S);
}
void jac_of(Jac26& J, const TrioAcc& A, const TrioLane& T) {
    TrioPt P;
    trio_acc_to(P, A, T);
    trio_to_jac(J, P, T);
}
// the window's stated end: (9, 3, 1) or (5, 3, 1), X on lane 0, Y on lanes 1 and 2, Z on lane 2
bool window_end_ok(const TrioAcc& A, const TrioLane& T) {
    if (T.r0 && A.S1.m > 9) return false;
    if (!T.r0 && A.S1.m > 3) return false;
    return !T.r2 || A.Zs.m <= 1;
}
// a += j p limb by limb: the same value at magnitude (a.m + j)
void add_p(fe26& a, int j) {
    for (int i = 0; i < 10; ++i) a.v[i] += static_cast<uint32_t>(j) * f26::plimb(i);
    a.m += j;
}

constexpr int cases_per_round = 5;
constexpr int kDepth = 32;
struct WCase {    // (a)
    int tab;
    bool neg, phi, inf;
    int hug;      // 0: canonical limbs, 1: X, Y at 10 and Z at 16 (both windows), 2: the lean window at (16, 16, 16)
    int zeros;    // leading zero digits
    int dbase;    // the digit sequence's offset
    Jac26 start;  // canonical coordinates
};
struct KCase {  // (b), (c)
    u128 k;
    bool neg, phi;
    int tab;
};
std::vector<Table> tables;
std::vector<WCase> wcases;
std::vector<KCase> scases, ccases;
std::vector<int> wbad, sbad, cbad;
bool digit_seen[17];

int wdigit(const WCase& C, int w) {
    if (w < C.zeros) return 0;
    return (w * 5 + C.dbase) % 17 - 8;
}

void window_main(int lane, int round) {
    my_lane = lane;
    const TrioLane T(lane);
    const int t5 = (lane % 16) / 3;
    const int c = round * cases_per_round + (t5 < 5 ? t5 : 4);
    const WCase& C = wcases[c];
    const Table& Tb = tables[C.tab];
    const bool real = T.r2 && t5 < 5;
    Jac26 ref = C.start;
    ref.inf = C.inf;
    Jac26 jo = C.start, jl = C.start;
    if (C.hug) {
        add_p(jo.X, 9);
        add_p(jo.Y, 9);
        add_p(jo.Z, 15);
        add_p(jl.X, C.hug == 2 ? 15 : 9);
        add_p(jl.Y, C.hug == 2 ? 15 : 9);
        add_p(jl.Z, 15);
    }
    TrioPt old, P;
    trio::sel(old.S1, T.r0, jo.X, jo.Y);
    old.Xs = jo.X;
    old.Zs = jo.Z;
    old.inf = C.inf;
    trio::sel(P.S1, T.r0, jl.X, jl.Y);
    P.Xs = jl.X;
    P.Zs = jl.Z;
    P.inf = C.inf;
    if (C.inf) {
        trio_set_inf(old);
        trio_set_inf(P);
    }
    TrioAcc acc;
    trio_acc_from(acc, P);
    for (int w = 0; w < kDepth; ++w) {
        const int d = wdigit(C, w);
        lean_window(acc, Tb, d, C.neg, C.phi, T);
        old_window(old, Tb, d, C.neg, C.phi, T);
        ref_window(ref, Tb, d, C.neg, C.phi);
        Jac26 a, b;
        jac_of(a, acc, T);
        trio_to_jac(b, old, T);
        if (!window_end_ok(acc, T) && !wbad[c]) wbad[c] = 100 + w;
        if (real && !wbad[c]) {
            if (!same_point(a, ref)) wbad[c] = 1000 + w;
            else if (!same_point(a, b)) wbad[c] = 2000 + w;
        }
    }
}

// (b) and (c): the chain start, then `windows` lean windows, against one lane
void chain_main(int lane, int round, int windows, const std::vector<KCase>* cases, std::vector<int>* bad) {
    my_lane = lane;
    const TrioLane T(lane);
    const int t5 = (lane % 16) / 3;
    const int c = round * cases_per_round + (t5 < 5 ? t5 : 4);
    const KCase& C = (*cases)[c];
    const Table& Tb = tables[C.tab];
    const uint32_t top = static_cast<uint32_t>(C.k >> 96);
    TrioPt st;
    trio_chain_start(st, top, [&](Aff26& S, int d) { entry(S, Tb, d, C.neg, C.phi); }, T);
    TrioAcc acc;
    trio_acc_from(acc, st);
    u128 kn = C.k << 4;
    for (int w = 0; w < windows; ++w) lean_window(acc, Tb, booth_digit(kn), C.neg, C.phi, T);
    // one lane: double-and-add over the bits that the start and the windows have consumed
    Jac26 dn;
    CurveK1x::set_inf(dn);
    {
        // the scalar consumed so far: t 16^windows plus the digits, a Booth prefix of k and so never negative;
        // summed modulo 2^128 (t = 16 wraps; the whole chain's sum is k < 2^128 itself)
        const uint32_t t = (top >> 28) + ((top >> 27) & 1u);
        u128 a = t;
        u128 kr = C.k << 4;
        for (int w = 0; w < windows; ++w) a = a * 16 + static_cast<u128>(static_cast<__int128>(booth_digit(kr)));
        if (windows == 31 && a != C.k) (*bad)[c] = 9;  // the digits sum to k
        Aff26 S;
        entry(S, Tb, 1, C.neg, C.phi);
        fe26_normalize(S.y);
        for (int i = 127; i >= 0; --i) {
            CurveK1x::dbl(dn, dn);
            if ((a >> i) & 1u) CurveK1x::madd(dn, dn, S);
        }
    }
    Jac26 jn;
    jac_of(jn, acc, T);
    const bool real = T.r2 && t5 < 5;
    if (real && !(*bad)[c] && !same_point(jn, dn)) (*bad)[c] = 1;
}

void run_rows(int rounds, const std::function<void(int, int)>& f) {
    for (int r = 0; r < rounds; ++r) {
        std::vector<std::thread> th;
        for (int l = 0; l < kLanes; ++l) th.emplace_back(f, l, r);
        for (auto& x : th) x.join();
    }
}
}  // namespace

int main() {
    {
        static const uint32_t bw[8] = {0x719501eeu, 0xc1396c28u, 0x12f58995u, 0x9cf04975u,
                                       0xac3434e9u, 0x6e64479eu, 0x657c0710u, 0x7ae96a2bu};
        fe26_from_words(beta, bw);
    }
    for (int j = 0; j < 4; ++j) {
        Aff26 R;
        rand_point(R);
        Table Tb;
        make_table(Tb, R);
        tables.push_back(Tb);
    }
    // (a) three rounds: no trio infinite / some / all
    for (int r = 0; r < 3; ++r)
        for (int j = 0; j < cases_per_round; ++j) {
            WCase C;
            C.tab = (r + j) % 4;
            C.neg = (j & 1) != 0;
            C.phi = ((j >> 1) ^ r) & 1;
            C.inf = r == 2 || (r == 1 && (j == 0 || j == 3));
            C.hug = C.inf ? 0 : (j + r) % 3;
            C.zeros = C.inf ? (j == 0 ? 0 : 2 * j - 1) : (j == 2 ? 3 : 0);
            C.dbase = 3 * j + 7 * r;
            // a multiple of the table's point the digits cannot meet: (2^40 + odd) R in a random representative
            CurveK1x::from_aff(C.start, tables[C.tab].e[0]);
            for (int i = 0; i < 40; ++i) CurveK1x::dbl(C.start, C.start);
            CurveK1x::madd(C.start, C.start, tables[C.tab].e[2 * (j % 4)]);
            if (C.phi) {  // phi(R)'s chain runs on phi's multiples
                fe26_mul(C.start.X, C.start.X, beta);
            }
            fe26 l, l2, l3;
            rand_fe(l);
            fe26_sqr(l2, l);
            fe26_mul(l3, l2, l);
            fe26_mul(C.start.X, C.start.X, l2);
            fe26_mul(C.start.Y, C.start.Y, l3);
            fe26_mul(C.start.Z, C.start.Z, l);
            fe26_normalize(C.start.X);
            fe26_normalize(C.start.Y);
            fe26_normalize(C.start.Z);
            wcases.push_back(C);
            for (int w = 0; w < kDepth; ++w) digit_seen[wdigit(C, w) + 8] = true;
        }
    for (int d = 0; d < 17; ++d)
        if (!digit_seen[d]) { printf("digit %d not covered\n", d - 8); return 1; }
    // (b) every t in 0..16, both ways where there are two
    const u128 all = ~static_cast<u128>(0);
    int n = 0;
    bool seen[17] = {};
    for (int t = 0; t <= 16; ++t) {
        const int W = t == 16 ? 15 : t, cbit = t == 16 ? 1 : 0;
        const u128 lowbits = rnd128() & ((static_cast<u128>(1) << 123) - 1);
        scases.push_back(KCase{(static_cast<u128>(W) << 124) | (static_cast<u128>(cbit) << 123) | lowbits, (n & 1) != 0,
                               (n & 2) != 0, n % 4});
        ++n;
    }
    for (int t = 1; t <= 3; ++t) {  // t = W + 1 with bit 123 set
        const u128 lowbits = rnd128() & ((static_cast<u128>(1) << 123) - 1);
        scases.push_back(KCase{(static_cast<u128>(4 * t - 1) << 124) | (static_cast<u128>(1) << 123) | lowbits, (n & 2) != 0,
                               (n & 1) != 0, n % 4});
        ++n;
    }
    for (const KCase& C : scases) {
        const uint32_t top = static_cast<uint32_t>(C.k >> 96);
        seen[(top >> 28) + ((top >> 27) & 1u)] = true;
    }
    for (int t = 0; t <= 16; ++t)
        if (!seen[t]) { printf("t = %d not covered\n", t); return 1; }
    // (c) whole chains
    ccases.push_back(KCase{0, false, false, 0});
    ccases.push_back(KCase{1, true, true, 1});
    ccases.push_back(KCase{all, false, true, 2});
    // runs of zero digits: in the middle (bits 40..99 clear), and at the top and the tail
    ccases.push_back(KCase{rnd128() & ~((static_cast<u128>(1) << 100) - (static_cast<u128>(1) << 40)), true, false, 3});
    ccases.push_back(KCase{rnd128(), false, true, 0});
    wbad.assign(wcases.size(), 0);
    sbad.assign(scases.size(), 0);
    cbad.assign(ccases.size(), 0);
    run_rows(static_cast<int>(wcases.size()) / cases_per_round, [](int l, int r) { window_main(l, r); });
    run_rows(static_cast<int>(scases.size()) / cases_per_round, [](int l, int r) { chain_main(l, r, 2, &scases, &sbad); });
    run_rows(static_cast<int>(ccases.size()) / cases_per_round, [](int l, int r) { chain_main(l, r, 31, &ccases, &cbad); });
    int nbad = 0;
    for (size_t i = 0; i < wbad.size(); ++i)
        if (wbad[i]) {
            printf("window mismatch: case %zu, code %d (1xx magnitude, 1xxx against one lane, 2xxx against the old window; "
                   "xx = window), neg %d phi %d inf %d hug %d\n", i, wbad[i], wcases[i].neg, wcases[i].phi, wcases[i].inf,
                   wcases[i].hug);
            ++nbad;
        }
    for (size_t i = 0; i < sbad.size(); ++i)
        if (sbad[i]) {
            printf("chain start + windows mismatch: case %zu, top word %08x\n", i, static_cast<uint32_t>(scases[i].k >> 96));
            ++nbad;
        }
    for (size_t i = 0; i < cbad.size(); ++i)
        if (cbad[i]) {
            printf("whole chain mismatch: case %zu, code %d, top word %08x\n", i, cbad[i],
                   static_cast<uint32_t>(ccases[i].k >> 96));
            ++nbad;
        }
    if (nbad) return 1;
    printf("trio window ok %zu x %d windows, %zu starts (t = 0..16), %zu whole chains\n", wcases.size(), kDepth,
           scases.size(), ccases.size());
    return 0;
}
