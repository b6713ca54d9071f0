// modinv_trio_test.cpp -- host build of csrc/modinv30.h: the safegcd inversion on lane trios against the one-lane
// routines of the same header.  The 16 lanes of one DPP row (five trios and the phantom, lane 15) run as threads
// in lockstep, every DPP fetch and every wave vote a barrier, as in trio_test.cpp; out-of-row fetches read 0.
// For both secp256k1 moduli, p and n:
//   (a) divsteps_30_trio (the systolic form and the lag-free one): the matrix words on roles 1 and 2 and the
//       returned zeta on every lane equal divsteps_30's, on random words, on g0 in {0, 1, 2^32 - 1, 2^31, f0, -f0}
//       with zeta in {-1, 0, -31, 17}, and on every batch of whole inversions' trajectories;
//   (b) modinv_safegcd_trio equals the one-lane loop and x x^-1 = 1 (mod m) by a plain 512-bit product, on the
//       edge values, 2,000 random residues, rows of one value five times and rows mixing 0 with live values; the
//       number of batches a row runs is the largest any of its five values needs, no more (an exit vote that
//       counts lanes holding no g never ends early) and no fewer;
//   (c) every row runs twice with different words on the phantom lane, the second time with the result asked for
//       on another role: neither changes a real trio's result or the batch count.
// Prints "modinv trio ok <counts>" and exits 0, or the first mismatch and exits 1.
#include "../../fisco-bcos_amd/csrc/modinv30.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

using namespace bcosgpu;

namespace {
constexpr int kLanes = 16;
// a sense-reversing barrier that yields while it waits (a row's inversion is about 700 fetches)
std::atomic<int> arrived{0};
std::atomic<unsigned> generation{0};
uint32_t slot[2][kLanes];
thread_local int my_lane = 0;
thread_local unsigned my_phase = 0;

void barrier() {
    const unsigned g = generation.load(std::memory_order_acquire);
    if (arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == kLanes) {
        arrived.store(0, std::memory_order_relaxed);
        generation.store(g + 1, std::memory_order_release);
    } else {
        while (generation.load(std::memory_order_acquire) == g) std::this_thread::yield();
    }
}
}  // namespace

namespace bcosgpu {
// (two slot rows in turn: a lane's next write cannot overtake another lane's read of this one)
uint32_t trio_emu_dpp(uint32_t x, int ctrl) {
    const unsigned ph = my_phase++ & 1u;
    slot[ph][my_lane] = x;
    barrier();
    int src = my_lane;
    switch (ctrl) {
        case 0x111: src = my_lane - 1; break;  // row_shr:1
        case 0x112: src = my_lane - 2; break;  // row_shr:2
        case 0x101: src = my_lane + 1; break;  // row_shl:1
        case 0x102: src = my_lane + 2; break;  // row_shl:2
        default: abort();
    }
    return (src >= 0 && src < kLanes) ? slot[ph][src] : 0u;
}
bool trio_emu_any(bool b) {
    const unsigned ph = my_phase++ & 1u;
    slot[ph][my_lane] = b ? 1u : 0u;
    barrier();
    bool r = false;
    for (int i = 0; i < kLanes; ++i) r = r || slot[ph][i] != 0u;
    return r;
}
}  // namespace bcosgpu

namespace {
uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return static_cast<uint32_t>(rng_state >> 16);
}

struct U256 {
    uint32_t w[8];
};
bool operator==(const U256& a, const U256& b) { return memcmp(a.w, b.w, sizeof a.w) == 0; }
int cmp(const U256& a, const U256& b) {
    for (int i = 7; i >= 0; --i)
        if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
    return 0;
}
U256 sub(const U256& a, const U256& b) {
    U256 r;
    uint64_t bw = 0;
    for (int i = 0; i < 8; ++i) {
        const uint64_t d = static_cast<uint64_t>(a.w[i]) - b.w[i] - bw;
        r.w[i] = static_cast<uint32_t>(d);
        bw = (d >> 32) & 1u;
    }
    return r;
}
U256 small(uint32_t v) {
    U256 r{};
    r.w[0] = v;
    return r;
}
// a b mod m: the 512-bit schoolbook product, then bit-by-bit long division
U256 mulmod(const U256& a, const U256& b, const U256& m) {
    uint32_t p[16] = {0};
    for (int i = 0; i < 8; ++i) {
        uint64_t c = 0;
        for (int j = 0; j < 8; ++j) {
            c += static_cast<uint64_t>(a.w[i]) * b.w[j] + p[i + j];
            p[i + j] = static_cast<uint32_t>(c);
            c >>= 32;
        }
        p[i + 8] = static_cast<uint32_t>(c);
    }
    U256 r{};
    for (int bit = 511; bit >= 0; --bit) {
        const uint32_t top = r.w[7] >> 31;
        for (int i = 7; i > 0; --i) r.w[i] = (r.w[i] << 1) | (r.w[i - 1] >> 31);
        r.w[0] = (r.w[0] << 1) | ((p[bit >> 5] >> (bit & 31)) & 1u);
        if (top || cmp(r, m) >= 0) r = sub(r, m);
    }
    return r;
}
void to_s30(S30& r, const U256& a) {
    for (int i = 0; i < 9; ++i) {
        const int bit = 30 * i, w = bit >> 5, sh = bit & 31;
        uint64_t x = a.w[w];
        if (w + 1 < 8) x |= static_cast<uint64_t>(a.w[w + 1]) << 32;
        r.v[i] = static_cast<int32_t>((x >> sh) & 0x3fffffffu);
    }
}
U256 from_s30(const S30& a) {  // limbs in [0, 2^30), value < 2^256
    U256 r{};
    for (int i = 0; i < 9; ++i) {
        const int bit = 30 * i, w = bit >> 5, sh = bit & 31;
        const uint64_t x = static_cast<uint64_t>(static_cast<uint32_t>(a.v[i])) << sh;
        r.w[w] |= static_cast<uint32_t>(x);
        if (w + 1 < 8) r.w[w + 1] |= static_cast<uint32_t>(x >> 32);
    }
    return r;
}

struct Modulus {
    const char* name;
    U256 m;
    ModInfo30 mi;
};
Modulus make_modulus(const char* name, const U256& m, const int32_t want[9], uint32_t want_inv) {
    Modulus M;
    M.name = name;
    M.m = m;
    S30 s;
    to_s30(s, m);
    uint32_t inv = 1;
    for (int k = 0; k < 6; ++k) inv *= 2u - m.w[0] * inv;  // Newton: m^-1 mod 2^32
    M.mi.inv30 = inv & 0x3fffffffu;
    for (int i = 0; i < 9; ++i) M.mi.m[i] = s.v[i];
    // the words modinv.h keeps in constant memory
    if (memcmp(M.mi.m, want, sizeof M.mi.m) != 0 || M.mi.inv30 != want_inv) {
        printf("%s: ModInfo30 differs from the words of modinv.h\n", name);
        exit(1);
    }
    return M;
}

// the one-lane loop (modinv_safegcd of modinv.h, on S30); *batches = the batches it runs before g == 0
S30 ref_inv(const S30& x, const ModInfo30& mi, int* batches, std::vector<int32_t>* trajectory = nullptr) {
    S30 d{}, e{}, f, g = x;
    for (int i = 0; i < 9; ++i) f.v[i] = mi.m[i];
    e.v[0] = 1;
    int32_t zeta = -1;
    int it = 0;
    for (; it < 20;) {
        int32_t t[4];
        if (trajectory) {
            trajectory->push_back(zeta);
            trajectory->push_back(f.v[0]);
            trajectory->push_back(g.v[0]);
        }
        zeta = divsteps_30(zeta, static_cast<uint32_t>(f.v[0]), static_cast<uint32_t>(g.v[0]), t);
        update_de_30(d, e, t, mi);
        update_fg_30(f, g, t);
        ++it;
        int32_t gz = 0;
        for (int i = 0; i < 9; ++i) gz |= g.v[i];
        if (gz == 0) break;
    }
    *batches = it;
    normalize_30(d, f.v[8], mi);
    return d;
}

// ---------------------------------------------------------------- (a) one batch of divsteps
struct StepCase {
    int32_t zeta;
    uint32_t f, g;
};
std::vector<StepCase> scases;  // five per row
std::vector<uint32_t> sphantom;  // per row: the phantom's f, g
struct StepOut {
    int32_t t[4];
    int32_t zeta[3];
};
std::vector<StepOut> sout;

template <bool SYSTOLIC>
void step_lane(int lane, int rows) {
    my_lane = lane;
    my_phase = 0;
    const TrioLane T(lane);
    const int trio_idx = lane / 3, role = lane % 3;
    for (int r = 0; r < rows; ++r) {
        uint32_t A, B;
        int32_t zeta;
        if (lane == 15) {  // the phantom: a role-0 lane with words of its own
            A = sphantom[2 * r] | 1u;
            B = sphantom[2 * r + 1];
            zeta = static_cast<int32_t>(sphantom[2 * r] % 67u) - 33;
        } else {
            const StepCase& c = scases[5 * r + trio_idx];
            zeta = c.zeta;
            A = role == 0 ? c.f : 0xdeadbeefu * (lane + 1);  // what roles 1 and 2 bring is not read
            B = role == 0 ? c.g : 0x9e3779b9u * (lane + 7);
        }
        const int32_t z = divsteps_30_trio<SYSTOLIC>(zeta, A, B, T);
        if (lane == 15) continue;
        StepOut& o = sout[5 * r + trio_idx];
        o.zeta[role] = z;
        if (role == 1) {
            o.t[0] = static_cast<int32_t>(A);
            o.t[2] = static_cast<int32_t>(B);
        } else if (role == 2) {
            o.t[1] = static_cast<int32_t>(A);
            o.t[3] = static_cast<int32_t>(B);
        }
    }
}
template <bool SYSTOLIC>
size_t check_steps(const char* form) {
    const int rows = static_cast<int>(scases.size() / 5);
    sout.assign(scases.size(), StepOut{});
    std::vector<std::thread> th;
    for (int l = 0; l < kLanes; ++l) th.emplace_back(step_lane<SYSTOLIC>, l, rows);
    for (auto& x : th) x.join();
    for (size_t k = 0; k < scases.size(); ++k) {
        const StepCase& c = scases[k];
        int32_t t[4];
        const int32_t z = divsteps_30(c.zeta, c.f, c.g, t);
        const StepOut& o = sout[k];
        if (memcmp(t, o.t, sizeof t) != 0 || o.zeta[0] != z || o.zeta[1] != z || o.zeta[2] != z) {
            printf("divsteps_30_trio (%s) differs in case %zu: zeta %d f %08x g %08x\n one lane %d %d %d %d -> %d\n"
                   " trio     %d %d %d %d -> %d %d %d\n",
                   form, k, c.zeta, c.f, c.g, t[0], t[1], t[2], t[3], z, o.t[0], o.t[1], o.t[2], o.t[3], o.zeta[0],
                   o.zeta[1], o.zeta[2]);
            exit(1);
        }
    }
    return scases.size();
}

// ---------------------------------------------------------------- (b), (c) whole inversions
struct Row {
    U256 x[5];
    S30 phantom[2];  // the phantom lane's input of the first and of the second run
};
std::vector<Row> rows;
struct RowOut {
    S30 d[2][5];
    int batches[2][kLanes];
};
std::vector<RowOut> rout;
const Modulus* cur = nullptr;

void inv_lane(int lane) {
    my_lane = lane;
    my_phase = 0;
    const TrioLane T(lane);
    const int trio_idx = lane / 3, role = lane % 3;
    for (size_t r = 0; r < rows.size(); ++r) {
        for (int run = 0; run < 2; ++run) {
            S30 x, out;
            if (lane == 15) {
                x = rows[r].phantom[run];
            } else if (role == 0) {
                to_s30(x, rows[r].x[trio_idx]);
            } else {  // not read
                for (int i = 0; i < 9; ++i) x.v[i] = 0x12345 * (lane + i + run);
            }
            // the first run hands the result to role 2 (what the recovery kernel asks for), the second to role 0
            const int n = run == 0 ? modinv_safegcd_trio<2>(out, x, cur->mi, T, lane)
                                   : modinv_safegcd_trio<0>(out, x, cur->mi, T, lane);
            rout[r].batches[run][lane] = n;
            if (lane != 15 && role == (run == 0 ? 2 : 0)) rout[r].d[run][trio_idx] = out;
        }
    }
}
size_t check_rows(const Modulus& M) {
    cur = &M;
    rout.assign(rows.size(), RowOut{});
    std::vector<std::thread> th;
    for (int l = 0; l < kLanes; ++l) th.emplace_back(inv_lane, l);
    for (auto& x : th) x.join();
    for (size_t r = 0; r < rows.size(); ++r) {
        int want_batches = 0;
        for (int t = 0; t < 5; ++t) {
            const U256& x = rows[r].x[t];
            S30 xs;
            to_s30(xs, x);
            int nb;
            const S30 want = ref_inv(xs, M.mi, &nb);
            if (nb > want_batches) want_batches = nb;
            const U256 wi = from_s30(want);
            const U256 prod = mulmod(x, wi, M.m);
            const bool zero = x == small(0);
            if (cmp(wi, M.m) >= 0 || !(prod == small(zero ? 0u : 1u))) {
                printf("%s row %zu trio %d: the one-lane inverse fails x x^-1 = 1\n", M.name, r, t);
                exit(1);
            }
            for (int run = 0; run < 2; ++run)
                if (memcmp(&rout[r].d[run][t], &want, sizeof want) != 0) {
                    printf("%s row %zu trio %d run %d: modinv_safegcd_trio differs from the one-lane loop (x = %08x..%08x)\n",
                           M.name, r, t, run, x.w[7], x.w[0]);
                    exit(1);
                }
        }
        for (int run = 0; run < 2; ++run)
            for (int l = 0; l < kLanes; ++l)
                if (rout[r].batches[run][l] != want_batches) {
                    printf("%s row %zu run %d lane %d: %d batches, the row's slowest value needs %d\n", M.name, r, run, l,
                           rout[r].batches[run][l], want_batches);
                    exit(1);
                }
    }
    return rows.size();
}
U256 rand_residue(const U256& m) {
    for (;;) {
        U256 x;
        for (int i = 0; i < 8; ++i) x.w[i] = rnd();
        if (cmp(x, m) < 0) return x;
    }
}
void fill_phantoms(Row& R, const U256& m) {
    // a live value the first time (a phantom that voted would hold the row back or be cut short), other words
    // and a finished g the second
    to_s30(R.phantom[0], rand_residue(m));
    for (int i = 0; i < 9; ++i) R.phantom[1].v[i] = 0;
    if (rnd() & 1u) to_s30(R.phantom[1], rand_residue(m));
}
}  // namespace

int main() {
    const U256 p = {{0xfffffc2fu, 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}};
    const U256 n = {{0xd0364141u, 0xbfd25e8cu, 0xaf48a03bu, 0xbaaedce6u, 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu}};
    const int32_t p30[9] = {1073740847, 1073741819, 1073741823, 1073741823, 1073741823, 1073741823, 1073741823, 1073741823, 65535};
    const int32_t n30[9] = {271991105, 1061780019, 881460155, 733428139, 1073741498, 1073741823, 1073741823, 1073741823, 65535};
    const Modulus mods[2] = {make_modulus("p", p, p30, 769313487u), make_modulus("n", n, n30, 712462017u)};
    size_t nsteps = 0, nrows = 0;
    for (const Modulus& M : mods) {
        // ------------------------------------------------------------ (a)
        scases.clear();
        const int32_t zetas[4] = {-1, 0, -31, 17};
        for (int k = 0; k < 8; ++k) {
            const uint32_t f = k == 0 ? static_cast<uint32_t>(M.mi.m[0]) : k == 1 ? 1u : k == 2 ? 0xffffffffu : (rnd() | 1u);
            const uint32_t gs[6] = {0u, 1u, 0xffffffffu, 0x80000000u, f, 0u - f};
            for (uint32_t g : gs)
                for (int32_t z : zetas) scases.push_back({z, f, g});
        }
        for (int k = 0; k < 1500; ++k)
            scases.push_back({static_cast<int32_t>(rnd() % 1201u) - 600, rnd() | 1u, rnd()});
        for (int k = 0; k < 40; ++k) {  // every batch of whole inversions
            S30 xs;
            to_s30(xs, k == 0 ? small(1) : k == 1 ? sub(M.m, small(1)) : rand_residue(M.m));
            std::vector<int32_t> tr;
            int nb;
            ref_inv(xs, M.mi, &nb, &tr);
            for (size_t j = 0; j + 2 < tr.size(); j += 3)
                scases.push_back({tr[j], static_cast<uint32_t>(tr[j + 1]), static_cast<uint32_t>(tr[j + 2])});
        }
        while (scases.size() % 5) scases.push_back({-1, 1u, 0u});
        sphantom.clear();
        for (size_t k = 0; k < 2 * scases.size() / 5; ++k) sphantom.push_back(rnd());
        nsteps += check_steps<true>("systolic");
        nsteps += check_steps<false>("lag-free");

        // ------------------------------------------------------------ (b), (c)
        rows.clear();
        U256 half = M.m;  // (m + 1) / 2 = (m >> 1) + 1, m odd
        for (int i = 0; i < 8; ++i) half.w[i] = (M.m.w[i] >> 1) | (i < 7 ? M.m.w[i + 1] << 31 : 0u);
        half = sub(half, sub(small(0), small(1)));
        U256 p255{};
        p255.w[7] = 0x80000000u;
        const U256 edge[8] = {small(0), small(1), small(2), sub(M.m, small(1)), sub(M.m, small(2)), half, p255,
                              sub(small(0), M.m)};  // 2^256 mod m = 2^256 - m
        std::vector<U256> vals(edge, edge + 8);
        vals.push_back(rand_residue(M.m));
        vals.push_back(rand_residue(M.m));
        for (int k = 0; k < 2000; ++k) vals.push_back(rand_residue(M.m));
        for (size_t k = 0; k + 4 < vals.size(); k += 5) {
            Row R;
            for (int t = 0; t < 5; ++t) R.x[t] = vals[k + t];
            rows.push_back(R);
        }
        for (int k = 0; k < 10; ++k) {  // one value in all five trios
            Row R;
            const U256 v = k < 8 ? edge[k] : rand_residue(M.m);
            for (int t = 0; t < 5; ++t) R.x[t] = v;
            rows.push_back(R);
        }
        for (int k = 0; k < 15; ++k) {  // zeros and values that finish early around one live trio
            Row R;
            for (int t = 0; t < 5; ++t) R.x[t] = (k % 3 == 0 && t != k % 5) ? small(1) : small(0);
            R.x[k % 5] = k < 5 ? rand_residue(M.m) : k < 10 ? edge[3 + k % 5] : rand_residue(M.m);
            rows.push_back(R);
        }
        for (Row& R : rows) fill_phantoms(R, M.m);
        nrows += check_rows(M);
    }
    printf("modinv trio ok %zu divstep batches + %zu rows of five inversions, each twice\n", nsteps, nrows);
    return 0;
}
