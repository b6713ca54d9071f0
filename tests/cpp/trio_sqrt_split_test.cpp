// trio_sqrt_split_test.cpp -- host build (FE26_CHECK) of the two pieces of the lane-trio kernel's split
// square root (ecc_coop.hip, trio26_recover_body):
//  (a) fe26_sqrt_head<CUT> then fe26_sqrt_tail<CUT> against fe26_sqrt_cand, limb for limb, for both cuts:
//      random elements, 0, 1, quadratic non-residues, magnitude-2 inputs (random and bound-hugging limbs);
//  (b) the split last addition: chain 0's Z3 (trio_scale_xz, trio_add_z) together with the
//      partner's X3, Y3 (trio_scale_xz, trio_scale_y, trio_add) against CurveK1x::add of T and (X, Y, Z Zc y), as affine
//      points.  The 16 lanes of one DPP row run as lockstep threads (as tests/cpp/trio_test.cpp), so every
//      field operation asserts its magnitude contract on every lane.  Cases: curve points (S on E_w for
//      a random Zc and w = y^2, T on E), random triples at every accepted magnitude, S_E = T, S_E = -T,
//      S = infinity, T = infinity, both.
// Prints "sqrt split ok <cases>" and exits 0, or the first mismatch and exits 1.
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
uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return static_cast<uint32_t>(rng_state >> 11);
}
void rand_fe(fe26& a, int m, int mode) {  // mode 0 random limbs, 1 every limb at its bound
    for (int i = 0; i < 10; ++i) {
        const uint64_t bound = static_cast<uint64_t>(m) << (i == 9 ? 22 : 26);
        a.v[i] = static_cast<uint32_t>(mode ? bound : ((static_cast<uint64_t>(rnd()) << 20 ^ rnd()) % (bound + 1)));
    }
    a.m = m;
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
bool is_residue(const fe26& a) {
    fe26 y, t;
    fe26_sqrt_cand(y, a);
    fe26_sqr(t, y);
    return same(t, a);
}

// (a)
int sqrt_cases = 0, sqrt_residues = 0, sqrt_nonresidues = 0;
template <int CUT>
bool check_split(const fe26& a) {
    fe26 want, got, st[fe26_sqrt_live<CUT>()];
    fe26_sqrt_cand(want, a);
    fe26_sqrt_head<CUT>(st, a);
    fe26_sqrt_tail<CUT>(got, st);
    return memcmp(want.v, got.v, sizeof want.v) == 0 && want.m == got.m;
}
bool check_sqrt(const fe26& a, const char* what) {
    ++sqrt_cases;
    if (is_residue(a)) ++sqrt_residues;
    else ++sqrt_nonresidues;
    if (!check_split<0>(a) || !check_split<1>(a)) {
        printf("head o tail differs from fe26_sqrt_cand: %s (case %d)\n", what, sqrt_cases);
        return false;
    }
    return true;
}

// (b)
struct CaseB {
    Jac26 S, T;   // S on E_w (co-Z scaled by Zc), T on E
    fe26 zc, y;   // w = y^2
};
std::vector<CaseB> cases;
std::vector<int> bad;
constexpr int cases_per_round = 5;

void to_trio(TrioPt& P, const Jac26& J, const TrioLane& T) {
    trio::sel(P.S1, T.r0, J.X, J.Y);
    P.Xs = J.X;
    P.Zs = J.Z;
    P.inf = J.inf;
}

void lane_main(int lane, int round) {
    my_lane = lane;
    const TrioLane T(lane);
    const int t = (lane % 16) / 3;
    const int c = round * cases_per_round + (t < 5 ? t : 4);
    const CaseB& C = cases[c];
    TrioPt S, G;
    to_trio(S, C.S, T);
    to_trio(G, C.T, T);
    fe26 w, K, l;
    fe26_sqr(w, C.y);
    fe26_sqr(K, C.zc);
    fe26_mul(K, K, w);    // K = Zc^2 w
    fe26_mul(l, C.zc, C.y);
    // chain 0: no y anywhere
    TrioPt SE0;
    fe26 Z3;
    trio_scale_xz(SE0, S, K, T);
    trio_add_z(Z3, G, SE0, T);
    // its partner: the complete addition
    TrioPt SE, O;
    trio_scale_xz(SE, S, K, T);
    trio_scale_y(SE, l, T);
    trio_add(O, G, SE, T);
    // the reference: T + (X, Y, Z Zc y) on one lane
    Jac26 Sref = C.S, R;
    fe26_mul(Sref.Z, C.S.Z, l);
    CurveK1x::add(R, C.T, Sref);
    if (T.r2 && t < 5) {
        Jac26 mine;
        mine.X = O.Xs;
        mine.Y = O.S1;
        mine.Z = Z3;
        mine.inf = O.inf;
        if (!same_point(mine, R)) bad[c] = 1;
        if (!R.inf && !same(Z3, O.Zs)) bad[c] = 2;  // the same representative on both sides
    }
}

// an affine point of E: y^2 = x^3 + 7
void rand_point(fe26& x, fe26& y) {
    for (;;) {
        fe26 t, rhs, seven;
        rand_fe(x, 1, 0);
        fe26_sqr(t, x);
        fe26_mul(rhs, t, x);
        fe26_set_small(seven, 7u);
        fe26_add(rhs, rhs, seven);
        fe26_sqrt_cand(y, rhs);
        fe26_sqr(t, y);
        if (same(t, rhs)) return;
    }
}
// (x, y) with Z = z: (x z^2, y z^3, z)
void jac_of(Jac26& J, const fe26& x, const fe26& y, const fe26& z) {
    fe26 z2, z3;
    fe26_sqr(z2, z);
    fe26_mul(z3, z2, z);
    fe26_mul(J.X, x, z2);
    fe26_mul(J.Y, y, z3);
    J.Z = z;
    J.inf = false;
}
}  // namespace

int main() {
    // ---- (a)
    {
        fe26 a;
        fe26_zero(a);
        if (!check_sqrt(a, "0")) return 1;
        fe26_one(a);
        if (!check_sqrt(a, "1")) return 1;
        for (int k = 0; k < 60; ++k) {
            rand_fe(a, 1, 0);
            if (!check_sqrt(a, "random, m 1")) return 1;
        }
        for (int k = 0; k < 30; ++k) {
            rand_fe(a, 2, 0);
            if (!check_sqrt(a, "random, m 2")) return 1;
        }
        rand_fe(a, 2, 1);
        if (!check_sqrt(a, "bound-hugging limbs, m 2")) return 1;
        rand_fe(a, 1, 1);
        if (!check_sqrt(a, "bound-hugging limbs, m 1")) return 1;
        // squares and non-residues by construction: s^2, and 3 s^2 (3 is a non-residue mod p)
        for (int k = 0; k < 10; ++k) {
            fe26 s, q, n;
            rand_fe(s, 1, 0);
            fe26_sqr(q, s);
            fe26_mul_int<3>(n, q);
            if (!check_sqrt(q, "square")) return 1;
            if (!is_residue(q)) { printf("s^2 is not a residue\n"); return 1; }
            if (!check_sqrt(n, "non-residue, m 3 input")) return 1;
            if (is_residue(n)) { printf("3 s^2 is a residue\n"); return 1; }
        }
        if (sqrt_residues < 10 || sqrt_nonresidues < 10) {
            printf("too few residues (%d) or non-residues (%d)\n", sqrt_residues, sqrt_nonresidues);
            return 1;
        }
    }
    // ---- (b)
    for (int k = 0; k < 300; ++k) {
        CaseB C;
        const int special = k % 10;
        rand_fe(C.zc, 1, 0);
        rand_fe(C.y, 1, 0);
        if (special == 7 || special == 9) {  // random triples at the magnitudes the entries accept
            const int mode = k % 7 == 6 ? 1 : 0;
            rand_fe(C.S.X, 1 + static_cast<int>(rnd() % 16), mode);
            rand_fe(C.S.Y, 1 + static_cast<int>(rnd() % 16), mode);
            rand_fe(C.S.Z, 1 + static_cast<int>(rnd() % 16), mode);
            rand_fe(C.T.X, 1 + static_cast<int>(rnd() % 16), mode);
            rand_fe(C.T.Y, 1 + static_cast<int>(rnd() % 16), mode);
            rand_fe(C.T.Z, 1 + static_cast<int>(rnd() % 16), mode);
            C.S.inf = C.T.inf = false;
        } else {
            fe26 xt, yt, xs, ys, zt, zs, l, ztot;
            rand_point(xt, yt);
            rand_point(xs, ys);
            if (special == 1 || special == 2) {  // S_E = +-T
                xs = xt;
                ys = yt;
                if (special == 2) {
                    fe26_neg<2>(ys, yt);
                    fe26_normalize(ys);
                }
            }
            rand_fe(zt, 1, 0);
            rand_fe(zs, 1, 0);
            jac_of(C.T, xt, yt, zt);
            // S = (xs Zt^2, ys Zt^3, zs) with Zt = zs Zc y: (X, Y, Z Zc y) is (xs, ys) on E
            fe26_mul(l, C.zc, C.y);
            fe26_mul(ztot, zs, l);
            jac_of(C.S, xs, ys, ztot);
            C.S.Z = zs;
            if (special == 3 || special == 5) CurveK1x::set_inf(C.S);
            if (special == 4 || special == 5) CurveK1x::set_inf(C.T);
        }
        cases.push_back(C);
    }
    bad.assign(cases.size(), 0);
    for (int r = 0; r < static_cast<int>(cases.size()) / cases_per_round; ++r) {
        std::vector<std::thread> th;
        for (int l = 0; l < kLanes; ++l) th.emplace_back(lane_main, l, r);
        for (auto& x : th) x.join();
    }
    int nbad = 0;
    for (size_t i = 0; i < bad.size(); ++i)
        if (bad[i]) {
            if (!nbad) printf("split addition mismatch in case %zu (kind %d, special %zu)\n", i, bad[i], i % 10);
            ++nbad;
        }
    if (nbad) {
        printf("split addition mismatches %d of %zu\n", nbad, cases.size());
        return 1;
    }
    printf("sqrt split ok %d roots (%d residues, %d non-residues) x 2 cuts + %zu split additions\n", sqrt_cases,
           sqrt_residues, sqrt_nonresidues, cases.size());
    return 0;
}
