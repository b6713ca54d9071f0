// merkle_plan.h -- which path launch_merkle (hash_kernels.hip) takes for a tree and with what launch geometry.
// Host-only plain C++17, no HIP include: plan_merkle is a pure function of the tree's shape, the CU count and the
// switches (tests/test_merkle_plan.py pins it without a GPU).  It fills in the kernels' plain argument structs.
#pragma once
#include <cstdint>
#include <cstdlib>

namespace bcosgpu {

constexpr int kPlanKeccak256 = 0, kPlanSm3 = 1;  // hash_device.h's Hasher values

struct TreeLevels {
    uint64_t pos[64];  // tree entry of the count record of level l + 1 (level 0 = leaves)
    uint64_t cnt[64];  // nodes of level l + 1
    int nlev;          // levels above the leaves (the last has one node)
};
struct FusedTree {  // merkle_fused_kernel
    TreeLevels t;
    uint32_t ctr_off[64];  // first counter of level l (levels a + 1 .. nlev - 1)
    int a;                 // levels above level 1 computed inside a wave (S = width^a)
    uint32_t S;
};
struct ClimbTree {  // merkle_climb_kernel
    TreeLevels t;
    uint32_t ctr_off[64];  // first arrival counter of level l (the top level of a climb step)
    int kin;               // levels above level 1 inside a workgroup (B = width^kin)
    int B;
    int g;                 // levels per climb step: width^(g - 1) <= 8 first-level nodes (SM3: <= 64)
    uint32_t coop_max;     // in-workgroup levels of at most this many nodes run on 25-lane groups
    uint32_t pair_max;     // ... of at most this many (and more than coop_max) on lane pairs, else one lane
    int pair;
};

constexpr uint32_t kFusedCounters = 16384;   // arrival counters of a counter slot (one slot per launch queue)
constexpr uint64_t kFusedMaxWaves = 2048;    // level-1 waves (two per SIMD) up to which the one-launch path runs
constexpr uint64_t kClimbMaxWgs = 4096;      // level-1 workgroups up to which the four-wave path runs
constexpr int kClimbMaxWidth = 4;  // widths the four-wave path takes at latency sizes (wider: the one-wave one)
constexpr uint64_t kTopKernelMaxIn = 16384;  // inputs per level the single-workgroup kernel takes
constexpr uint64_t kPairMaxNodes = 32768;    // level-1 nodes up to which Keccak levels use lane pairs

// The BCOSGPU_MERKLE_<switch> environment variables (A/B hooks and forced paths; every path writes the same output
// vector), read once per process.  0/1: the value's first character, anything else is automatic; 1: first character.
//   LEVELWISE  atoi = 1  one merkle_level_kernel launch per level, nothing else
//   FUSED      0/1       the one-wave one-launch path off / on at any size and hasher (on: no climb path)
//   CLIMB      0/1       the four-wave one-launch path off / on
//   SM3CLIMB   1         SM3 of width > 2 at latency sizes on the climb kernel with expanded blocks
//   PAIR       0/1       two-launch path: Keccak levels on lane pairs
//   SM3X       0/1       two-launch path: SM3 blocks expanded in parallel (automatic: the top kernel always)
//   NOSUB      1         climb path: never the subtree kernel first (the climb kernel takes the leaves itself)
//   LATSCHED   1         climb path: the latency schedule even with more workgroups than CUs
struct MerkleSwitches {
    bool levelwise = false;
    int fused = -1, climb = -1, pair = -1, sm3x = -1;  // -1 automatic, 0 / 1 forced off / on
    bool sm3climb = false, nosub = false, latsched = false;
};
inline MerkleSwitches parse_merkle_switches() {
    const auto tri = [](const char* name) {
        const char* e = std::getenv(name);
        return e && (e[0] == '0' || e[0] == '1') ? e[0] - '0' : -1;
    };
    const char* lw = std::getenv("BCOSGPU_MERKLE_LEVELWISE");
    return {lw && std::atoi(lw) == 1, tri("BCOSGPU_MERKLE_FUSED"), tri("BCOSGPU_MERKLE_CLIMB"),
            tri("BCOSGPU_MERKLE_PAIR"), tri("BCOSGPU_MERKLE_SM3X"), tri("BCOSGPU_MERKLE_SM3CLIMB") == 1,
            tri("BCOSGPU_MERKLE_NOSUB") == 1, tri("BCOSGPU_MERKLE_LATSCHED") == 1};
}

enum MerklePath : int { kPathClimb, kPathFused, kPathTwoLaunch, kPathLevelwise };
struct MerklePlan {
    enum Kind : int { kArgError = 0, kCopy, kTree } kind;  // kCopy: one leaf is its own tree and root (Merkle.h:177-182)
    TreeLevels t;
    // what to try, in order (a one-launch path that gets no counter slot at run time moves on to the next; the last,
    // two-launch or levelwise, always runs); only the listed paths' geometry below is set
    int npaths;
    MerklePath paths[3];
    struct Climb {  // merkle_subtree_kernel for levels 0 .. k (k >= 0; -1: none), then merkle_climb_kernel
        int k;
        unsigned sub_grid, wgs;  // x 256 threads
        ClimbTree f;             // f.t: the levels above level k
        uint32_t counters;
        bool latency, x;  // the latency schedule (else throughput); merkle_climb_kernel<SM3, W, true>
    } climb;
    struct Fused {  // merkle_fused_kernel on grid x 64 threads
        FusedTree f;
        unsigned grid;
        uint32_t counters;
    } fused;
    struct TwoLaunch {  // merkle_wg_kernel, a merkle_level_kernel per wide middle level, merkle_top_kernel
        int kin, pair;
        uint32_t B;
        unsigned grid, threads;
        bool sm3x, sm3x_top;  // the X variants of the workgroup / top kernel
        int nmid, top;        // middle levels kin + 1 .. top - 1; the top kernel from level `top` (if < t.nlev)
    } two;
};

// the largest power of width that is <= cap, and its exponent
inline uint32_t merkle_pow_le(int width, uint32_t cap, int& exp) {
    uint32_t p = 1;
    for (exp = 0; p * static_cast<uint32_t>(width) <= cap; ++exp) p *= width;
    return p;
}
// ctr_off[l] = first arrival counter of level l (levels up to `inside`, inside one wave or workgroup, take none)
inline uint32_t merkle_counter_offsets(const TreeLevels& t, int inside, uint32_t ctr_off[64]) {
    uint32_t off = 0;
    for (int l = 0; l < t.nlev; ++l) {
        ctr_off[l] = off;
        if (l > inside) off += static_cast<uint32_t>(t.cnt[l]);
    }
    return off;
}

// false when the four-wave path does not apply (too many workgroups or counters)
inline bool plan_climb(int hasher, int width, const TreeLevels& t0, uint64_t cus, const MerkleSwitches& sw, bool sm3x,
                       MerklePlan::Climb& c) {
    ClimbTree& f = c.f;
    f.B = static_cast<int>(merkle_pow_le(width, 256, f.kin));
    // more workgroups than CUs: the subtree kernel first for levels 0..k (width^k <= 64 level-0 nodes per thread),
    // so that the climb kernel starts with one workgroup per CU
    c.k = -1;
    if (!sw.nosub && (t0.cnt[0] + f.B - 1) / f.B > cus) {
        uint64_t span = 1;
        for (int q = 0; q + 2 < t0.nlev && span <= 64; ++q, span *= width)
            if ((t0.cnt[q + 1] + f.B - 1) / f.B <= cus) {
                c.k = q;
                break;
            }
    }
    f.t = t0;  // the climb kernel's levels: those above level k, whose nodes are its leaves
    if (c.k >= 0) {
        f.t.nlev = t0.nlev - (c.k + 1);
        for (int l = 0; l < f.t.nlev; ++l) {
            f.t.pos[l] = t0.pos[l + c.k + 1];
            f.t.cnt[l] = t0.cnt[l + c.k + 1];
        }
        c.sub_grid = static_cast<unsigned>((t0.cnt[c.k] + 255) / 256);
    }
    // width^(g - 1) <= 8 (SM3: 64) first-level nodes per step, and the step's width^g gathered children fit one
    // LDS half (lds[0], 256 nodes): the step's first level writes lds[1] while reading them
    f.g = 1;
    for (int q = width; q <= (hasher == kPlanKeccak256 ? 8 : 64) && q * width <= 256; q *= width) ++f.g;
    const uint64_t wgs = (f.t.cnt[0] + f.B - 1) / f.B;
    if (wgs > kClimbMaxWgs) return false;
    c.wgs = static_cast<unsigned>(wgs);
    // one workgroup per CU: the latency schedule (25-lane groups from eight nodes down, lane pairs above, one lane
    // per node only for level 1's 256); more: every SIMD runs several waves, so each level takes the fewest
    // wave-cycles -- one lane per node (a wave pass of 64 nodes: 22k cycles) down to 64 nodes, lane pairs (32 nodes:
    // 15k) down to 4, 25-lane groups (2 nodes: 9.4k) below
    c.latency = wgs <= cus || sw.latsched;
    f.coop_max = c.latency ? 8u : 2u;
    f.pair_max = c.latency ? 128u : 32u;
    f.pair = 1;
    c.x = hasher == kPlanSm3 && sm3x && width > 2 && c.latency;
    c.counters = merkle_counter_offsets(f.t, f.kin, f.ctr_off);
    return c.counters <= kFusedCounters;
}

// false when the one-wave path does not apply (too many counters, or, unless forced, waves)
inline bool plan_fused(int hasher, int width, const TreeLevels& t, bool force, MerklePlan::Fused& p) {
    p.f.t = t;
    // S = width^a: Keccak level 0 on lane pairs (S <= 32), SM3 one lane per node (S <= 64)
    p.f.S = merkle_pow_le(width, hasher == kPlanKeccak256 ? 32u : 64u, p.f.a);
    p.counters = merkle_counter_offsets(t, p.f.a, p.f.ctr_off);
    const uint64_t waves = (t.cnt[0] + p.f.S - 1) / p.f.S;
    p.grid = static_cast<unsigned>(waves);
    return p.counters <= kFusedCounters && (force || waves <= kFusedMaxWaves);
}

inline void plan_two_launch(int hasher, int width, const TreeLevels& t, uint64_t cus, const MerkleSwitches& sw,
                            MerklePlan::TwoLaunch& w) {
    w.B = merkle_pow_le(width, 256, w.kin);
    w.grid = static_cast<unsigned>((t.cnt[0] + w.B - 1) / w.B);
    // Keccak levels on lane pairs while level 1 is latency-sized: at most one pair per lane of a wave per SIMD
    // (kPairMaxNodes); beyond that one lane per node, which issues fewer instructions per node.
    w.pair = hasher == kPlanKeccak256 && (sw.pair >= 0 ? sw.pair : t.cnt[0] <= kPairMaxNodes) ? 1 : 0;
    // Keccak: enough 32-lane groups that the second level runs one cooperative pass (B / width nodes), two lanes
    // per level-1 node in pair mode
    w.threads = w.pair ? 2u * w.B : w.B;
    if (hasher == kPlanKeccak256 && w.kin >= 1 && 32u * (w.B / width) > w.threads && 32u * (w.B / width) <= 512u)
        w.threads = 32u * (w.B / width);
    // SM3 at latency sizes (a workgroup per CU at most): the LDS levels' and the top kernel's blocks expanded in
    // parallel (sm3_level_x; its 70 KB of LDS would cost a throughput-sized level 1 occupancy).
    w.sm3x = hasher == kPlanSm3 && (sw.sm3x >= 0 ? sw.sm3x == 1 : w.grid <= static_cast<unsigned>(cus));
    w.sm3x_top = hasher == kPlanSm3 && sw.sm3x != 0;
    w.top = w.kin + 1;
    while (w.top < t.nlev && t.cnt[w.top - 1] > kTopKernelMaxIn) ++w.top;  // wide middle levels: one launch each
    w.nmid = w.top - (w.kin + 1);
}

// `cus`: compute units of the device
inline MerklePlan plan_merkle(int hasher, int width, uint64_t n, uint64_t cus, const MerkleSwitches& sw) {
    MerklePlan p{};
    if (n == 0 || width < 2 || width > 64) return p;
    p.kind = n == 1 ? MerklePlan::kCopy : MerklePlan::kTree;
    TreeLevels& t = p.t;
    uint64_t pos = 0;
    for (uint64_t m = n; m > 1;) {
        if (t.nlev >= 64) return MerklePlan{};
        m = (m + width - 1) / width;
        t.pos[t.nlev] = pos;
        t.cnt[t.nlev] = m;
        pos += m + 1;
        ++t.nlev;
    }
    if (n == 1) return p;
    if (sw.levelwise) {
        p.paths[p.npaths++] = kPathLevelwise;
        return p;
    }
    // Throughput-sized trees (more level-1 nodes than 256 per CU), where the subtree kernel runs first, take the
    // climb path at every width up to 16 and both hashers (16M leaves, width 16: Keccak 0.62 vs 0.94 ms on the
    // two-launch path, SM3 0.56 vs 0.71); at latency sizes only narrow Keccak trees do (SM3's one-lane levels measured
    // no faster than the two-launch path; width 16 has the one-wave kernel).  SM3 of width > 2 at latency sizes on
    // the climb kernel with expanded blocks, one launch instead of two, measured no faster either (C1 0.1058 vs
    // 0.1038 ms: 38 serial compressions on the critical path either way), so it is opt-in.  DESIGN.md section 6 has
    // the measurements (profiles/r04_merkle_paths_ab_*.json, profiles/r06_merkle_sm3_climbx_ab.json).
    const bool big = t.cnt[0] > 256ull * cus;
    const bool sm3_climb = hasher == kPlanSm3 && width > 2 && !big && sw.sm3climb;
    if (sw.fused != 1 &&
        (sw.climb == 1 || sm3_climb ||
         (sw.climb < 0 && ((width <= kClimbMaxWidth && (hasher == kPlanKeccak256 || big)) || (width <= 16 && big)))) &&
        plan_climb(hasher, width, t, cus, sw, sm3_climb, p.climb))
        p.paths[p.npaths++] = kPathClimb;
    // latency-sized trees: one launch, one wave per workgroup
    if ((sw.fused == 1 || (sw.fused < 0 && hasher == kPlanKeccak256)) && plan_fused(hasher, width, t, sw.fused == 1, p.fused))
        p.paths[p.npaths++] = kPathFused;
    plan_two_launch(hasher, width, t, cus, sw, p.two);
    p.paths[p.npaths++] = kPathTwoLaunch;
    return p;
}

}  // namespace bcosgpu
