// pair_inv_test.cpp -- host build of csrc/pair_inv.h: r^-1 and u2 = s / r (mod n) of a PAIR of signatures from one
// inversion, against one inversion per signature.
//
// The header's sequence (pair_enter, pair_scalars, pair_rinv) runs here as the kernel runs it: the three lanes
// of a trio in lockstep, one word of V holding the three lanes' words, the row shifts as index shifts (what
// comes from outside the trio -- the next trio's lanes -- is junk that changes from pair to pair).  Ops::mul is
// a plain CIOS Montgomery product mod n, Ops::inv the one-lane safegcd loop of csrc/modinv30.h
// (tests/cpp/modinv_trio_test.cpp shows that the trio form equals it).
//
// The yardstick is the path the kernel took before: per signature rm = M(r, R^2), rinv = M(safegcd(rm), R^3),
// u2 = M(s, rinv), after the same substitution of r = 1, s = 0 for a rejected member.  u2 and rinv of both
// members are compared with it word for word; independently of both, M(rinv, r) = 1 and u2 r = s (mod n).
//
// Cases: 1,000,000 seeded random pairs; r_a = r_b; r = 1 and r = n - 1 in either seat and both n - 1 (product
// 1); r_b = r_a^-1 (product 1); either or both members rejected, with r = 0, n, n + 1, 2^256 - 1 before the
// substitution, and with s = 0 -- the partner's u2 and rinv must stay exact.
// Prints "pair inv ok <counts>" and exits 0, or the first mismatch and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../fisco-bcos_amd/csrc/modinv30.h"
#include "../../fisco-bcos_amd/csrc/pair_inv.h"

using namespace bcosgpu;

namespace bcosgpu {
// modinv30.h's trio form is not used here; its host emulation hooks must exist to link
uint32_t trio_emu_dpp(uint32_t, int) { abort(); }
bool trio_emu_any(bool) { abort(); }
}  // namespace bcosgpu

namespace {

struct U256 {
    uint32_t v[8];
};
bool operator==(const U256& a, const U256& b) { return memcmp(a.v, b.v, sizeof a.v) == 0; }

const U256 N = {{0xd0364141u, 0xbfd25e8cu, 0xaf48a03bu, 0xbaaedce6u, 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu}};
const uint32_t NINV = 0x5588b13fu;  // -n^-1 mod 2^32
const U256 R2 = {{0x67d7d140u, 0x896cf214u, 0x0e7cf878u, 0x741496c2u, 0x5bcd07c6u, 0xe697f5e4u, 0x81c69bc5u, 0x9d671cd5u}};
const U256 R3 = {{0xe9ff41edu, 0x7bc0cfe0u, 0x44d4322cu, 0x00176484u, 0xf1d0b2dau, 0xb1b31347u, 0x18ef116du, 0x555d800cu}};
const U256 RONE = {{0x2fc9bebfu, 0x402da173u, 0x50b75fc4u, 0x45512319u, 0x00000001u, 0, 0, 0}};  // R mod n
const ModInfo30 MI = {{271991105, 1061780019, 881460155, 733428139, 1073741498, 1073741823, 1073741823, 1073741823, 65535},
                      712462017u};

U256 small(uint32_t x) {
    U256 r{};
    r.v[0] = x;
    return r;
}
bool lt(const U256& a, const U256& b) {
    for (int i = 7; i >= 0; --i)
        if (a.v[i] != b.v[i]) return a.v[i] < b.v[i];
    return false;
}
bool is_zero(const U256& a) { return a == small(0); }
U256 sub(const U256& a, const U256& b) {
    U256 r;
    uint64_t bw = 0;
    for (int i = 0; i < 8; ++i) {
        const uint64_t d = static_cast<uint64_t>(a.v[i]) - b.v[i] - bw;
        r.v[i] = static_cast<uint32_t>(d);
        bw = (d >> 32) & 1u;
    }
    return r;
}
U256 add(const U256& a, const U256& b) {  // mod 2^256
    U256 r;
    uint64_t c = 0;
    for (int i = 0; i < 8; ++i) {
        c += static_cast<uint64_t>(a.v[i]) + b.v[i];
        r.v[i] = static_cast<uint32_t>(c);
        c >>= 32;
    }
    return r;
}

// a b / 2^256 mod n (CIOS; any 256-bit a, b: the result is below 2n before the one subtraction)
U256 montmul(const U256& a, const U256& b) {
    uint32_t t[10] = {0};
    for (int i = 0; i < 8; ++i) {
        uint64_t c = 0;
        for (int j = 0; j < 8; ++j) {
            c += static_cast<uint64_t>(a.v[j]) * b.v[i] + t[j];
            t[j] = static_cast<uint32_t>(c);
            c >>= 32;
        }
        c += t[8];
        t[8] = static_cast<uint32_t>(c);
        t[9] = static_cast<uint32_t>(c >> 32);
        const uint32_t m = t[0] * NINV;
        c = static_cast<uint64_t>(m) * N.v[0] + t[0];
        c >>= 32;
        for (int j = 1; j < 8; ++j) {
            c += static_cast<uint64_t>(m) * N.v[j] + t[j];
            t[j - 1] = static_cast<uint32_t>(c);
            c >>= 32;
        }
        c += t[8];
        t[7] = static_cast<uint32_t>(c);
        t[8] = t[9] + static_cast<uint32_t>(c >> 32);
    }
    U256 r;
    memcpy(r.v, t, sizeof r.v);
    if (t[8] != 0u || !lt(r, N)) r = sub(r, N);
    return r;
}

// x^-1 mod n for x in [0, n) by the one-lane safegcd loop (modinv_safegcd of modinv.h, restated on the header)
U256 safegcd_inv(const U256& x) {
    S30 d{}, e{}, f, g;
    for (int i = 0; i < 9; ++i) {
        const int bit = 30 * i, w = bit >> 5, sh = bit & 31;
        uint64_t lo = x.v[w];
        if (w + 1 < 8) lo |= static_cast<uint64_t>(x.v[w + 1]) << 32;
        g.v[i] = static_cast<int32_t>((lo >> sh) & 0x3fffffffu);
        f.v[i] = MI.m[i];
    }
    e.v[0] = 1;
    int32_t zeta = -1;
    for (int it = 0; it < 20; ++it) {
        int32_t t[4];
        zeta = divsteps_30(zeta, static_cast<uint32_t>(f.v[0]), static_cast<uint32_t>(g.v[0]), t);
        update_de_30(d, e, t, MI);
        update_fg_30(f, g, t);
        int32_t gz = 0;
        for (int i = 0; i < 9; ++i) gz |= g.v[i];
        if (gz == 0) break;
    }
    normalize_30(d, f.v[8], MI);
    U256 r{};
    for (int i = 0; i < 9; ++i) {
        const int bit = 30 * i, w = bit >> 5, sh = bit & 31;
        const uint64_t y = static_cast<uint64_t>(static_cast<uint32_t>(d.v[i])) << sh;
        r.v[w] |= static_cast<uint32_t>(y);
        if (w + 1 < 8) r.v[w + 1] |= static_cast<uint32_t>(y >> 32);
    }
    return r;
}

uint64_t rng_state = 0x243f6a8885a308d3ull;
uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return static_cast<uint32_t>(rng_state >> 16);
}
U256 rand_any() {
    U256 x;
    for (int i = 0; i < 8; ++i) x.v[i] = rnd();
    return x;
}
U256 rand_scalar() {  // in [1, n)
    for (;;) {
        const U256 x = rand_any();
        if (lt(x, N) && !is_zero(x)) return x;
    }
}

// ---------------------------------------------------------------- the three lanes of a trio in lockstep
struct W3 {
    uint32_t l[3];
    W3& operator=(uint32_t x) {
        l[0] = l[1] = l[2] = x;
        return *this;
    }
};
struct V3 {
    W3 v[8];
};
U256 lane_of(const V3& a, int k) {
    U256 r;
    for (int i = 0; i < 8; ++i) r.v[i] = a.v[i].l[k];
    return r;
}
void set_lane(V3& a, int k, const U256& x) {
    for (int i = 0; i < 8; ++i) a.v[i].l[k] = x.v[i];
}
struct HostOps {
    U256 outside[3];  // what a fetch from beyond the trio brings
    // o = a of the lane `by` places to the right (negative: left)
    void shift(V3& o, const V3& a, int by) const {
        V3 t;
        for (int k = 0; k < 3; ++k) {
            const int src = k + by;
            set_lane(t, k, src >= 0 && src < 3 ? lane_of(a, src) : outside[k]);
        }
        o = t;
    }
    void right1(V3& o, const V3& a) const { shift(o, a, 1); }
    void left1(V3& o, const V3& a) const { shift(o, a, -1); }
    void left2(V3& o, const V3& a) const { shift(o, a, -2); }
    void sel(V3& o, int roles, const V3& a, const V3& b) const {
        V3 t;
        for (int k = 0; k < 3; ++k) set_lane(t, k, (roles >> k) & 1 ? lane_of(a, k) : lane_of(b, k));
        o = t;
    }
    void mul(V3& o, const V3& a, const V3& b) const {
        V3 t;
        for (int k = 0; k < 3; ++k) set_lane(t, k, montmul(lane_of(a, k), lane_of(b, k)));
        o = t;
    }
    void inv(V3& o, const V3& x) const {
        const U256 t = safegcd_inv(lane_of(x, 0));
        for (int k = 0; k < 3; ++k) set_lane(o, k, t);
    }
    void stamp(int) const {}
};

struct Member {
    U256 r, s;
};
// what parse_sig65 / EcrecIO::rsv accept of r and s
bool accepted(const Member& m) { return !is_zero(m.r) && !is_zero(m.s) && lt(m.r, N) && lt(m.s, N); }

size_t checked = 0;
void fail(const char* what, const char* name, int seat, const Member& a, const Member& b) {
    printf("%s: %s differs on seat %d (pair %zu)\n r_a %08x..%08x s_a %08x..%08x\n r_b %08x..%08x s_b %08x..%08x\n", name, what,
           seat, checked, a.r.v[7], a.r.v[0], a.s.v[7], a.s.v[0], b.r.v[7], b.r.v[0], b.s.v[7], b.s.v[0]);
    exit(1);
}

// ok_a / ok_b: the verdict that reaches the kernel (the parser's; a short signature or a bad v rejects a member
// whose r, s are in range)
void check_pair(const char* name, const Member& a, const Member& b, bool ok_a, bool ok_b) {
    const Member in[2] = {a, b};
    const bool ok[2] = {ok_a && accepted(a), ok_b && accepted(b)};
    // the yardstick: one inversion per member
    U256 want_u2[2], want_rinv[2];
    for (int m = 0; m < 2; ++m) {
        U256 r = in[m].r, s = in[m].s;
        if (!ok[m]) {
            r = small(1);
            s = small(0);
        }
        const U256 rm = montmul(r, R2);
        want_rinv[m] = montmul(safegcd_inv(rm), R3);
        want_u2[m] = montmul(s, want_rinv[m]);
        if (!(montmul(want_rinv[m], r) == small(1)) || !(montmul(montmul(want_u2[m], R2), r) == s) ||
            !lt(want_u2[m], N) || !lt(want_rinv[m], N))
            fail("the yardstick's own identity r^-1 r = 1, u2 r = s", name, m, a, b);
        if (!ok[m] && (!(want_rinv[m] == RONE) || !is_zero(want_u2[m])))
            fail("the yardstick of a rejected member (rinv = R, u2 = 0)", name, m, a, b);
    }
    // the pair on a trio
    V3 r, s, u2, inv, rinv;
    for (int k = 0; k < 3; ++k) {
        U256 rk = k < 2 ? in[k].r : rand_any(), sk = k < 2 ? in[k].s : rand_any();
        pair_enter(rk, sk, k < 2 && ok[k]);  // role 2 holds no member
        set_lane(r, k, rk);
        set_lane(s, k, sk);
    }
    HostOps ops;
    for (int k = 0; k < 3; ++k) ops.outside[k] = rand_any();
    pair_scalars(u2, inv, r, s, ops);
    pair_rinv(rinv, inv, r, ops);
    for (int m = 0; m < 2; ++m) {
        if (!(lane_of(u2, m) == want_u2[m])) fail("u2", name, m, a, b);
        if (!(lane_of(rinv, m) == want_rinv[m])) fail("r^-1", name, m, a, b);
    }
    ++checked;
}

}  // namespace

int main() {
    const U256 nm1 = sub(N, small(1));
    // ------------------------------------------------------------ crafted pairs
    size_t crafted = 0;
    {
        const Member p = {rand_scalar(), rand_scalar()}, q = {rand_scalar(), rand_scalar()};
        check_pair("equal r", p, Member{p.r, q.s}, true, true);
        check_pair("equal r and s", p, p, true, true);
        const U256 edges[2] = {small(1), nm1};
        for (const U256& e : edges) {
            check_pair("edge r in seat a", Member{e, p.s}, q, true, true);
            check_pair("edge r in seat b", p, Member{e, q.s}, true, true);
            check_pair("edge r in both seats", Member{e, p.s}, Member{e, q.s}, true, true);
        }
        check_pair("r = 1 beside r = n - 1", Member{small(1), p.s}, Member{nm1, q.s}, true, true);
        for (int k = 0; k < 64; ++k) {  // r_b = r_a^-1: the product is 1
            const U256 ra = k == 0 ? small(2) : rand_scalar();
            const U256 rb = safegcd_inv(ra);
            check_pair("r_b = 1 / r_a", Member{ra, rand_scalar()}, Member{rb, rand_scalar()}, true, true);
            check_pair("r_a = 1 / r_b", Member{rb, rand_scalar()}, Member{ra, rand_scalar()}, true, true);
        }
        // rejected members: by their r, by s = 0, by the parser alone (r, s in range)
        U256 ones;
        for (int i = 0; i < 8; ++i) ones.v[i] = 0xffffffffu;
        const U256 bad_r[4] = {small(0), N, add(N, small(1)), ones};
        for (int k = 0; k < 16; ++k) {
            const Member v1 = {rand_scalar(), rand_scalar()}, v2 = {rand_scalar(), rand_scalar()};
            for (const U256& br : bad_r) {
                const Member bad = {br, rand_scalar()}, bad0 = {br, small(0)};
                check_pair("bad r in seat a", bad, v1, true, true);
                check_pair("bad r in seat b", v1, bad, true, true);
                check_pair("bad r, s = 0 in seat a", bad0, v1, true, true);
                check_pair("bad r, s = 0 in seat b", v1, bad0, true, true);
                for (const U256& br2 : bad_r) check_pair("bad r in both seats", bad, Member{br2, rand_scalar()}, true, true);
            }
            const Member s0 = {rand_scalar(), small(0)}, sn = {rand_scalar(), N};
            check_pair("s = 0 in seat a", s0, v1, true, true);
            check_pair("s = 0 in seat b", v1, s0, true, true);
            check_pair("s = 0 in both seats", s0, Member{rand_scalar(), small(0)}, true, true);
            check_pair("s = n in seat a", sn, v1, true, true);
            check_pair("s = n in seat b", v1, sn, true, true);
            check_pair("parser rejects seat a", v1, v2, false, true);
            check_pair("parser rejects seat b", v1, v2, true, false);
            check_pair("parser rejects both", v1, v2, false, false);
            check_pair("a rejected member with the partner's r", Member{v1.r, v2.s}, v1, false, true);
        }
        crafted = checked;
    }
    // ------------------------------------------------------------ random pairs
    for (int k = 0; k < 1000000; ++k) {
        const Member a = {rand_scalar(), rand_scalar()}, b = {rand_scalar(), rand_scalar()};
        check_pair("random", a, b, true, true);
    }
    printf("pair inv ok %zu crafted + %zu random pairs\n", crafted, checked - crafted);
    return 0;
}
