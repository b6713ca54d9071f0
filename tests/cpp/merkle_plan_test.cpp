// Prints plan_merkle's answer (csrc/merkle_plan.h, host-only) as one JSON line per argument
//   HASHER:WIDTH:N:CUS[:SWITCH=VALUE[,SWITCH=VALUE...]]      SWITCH without the BCOSGPU_MERKLE_ prefix
// The switches go through the environment and parse_merkle_switches, as in the library.
// tests/test_merkle_plan.py compiles this with g++ and pins the plans.
#include <cstdio>
#include <cstdlib>
#include <string>
#include "../../fisco-bcos_amd/csrc/merkle_plan.h"

using namespace bcosgpu;

static const char* const kSwitches[] = {"LEVELWISE", "FUSED", "CLIMB", "SM3CLIMB", "PAIR", "SM3X", "NOSUB", "LATSCHED"};

static void print_tree(const char* name, const TreeLevels& t) {
    std::printf("\"%s\": {\"nlev\": %d, \"cnt0\": %llu, \"pos0\": %llu}", name, t.nlev,
                static_cast<unsigned long long>(t.cnt[0]), static_cast<unsigned long long>(t.pos[0]));
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        int hasher = 0, width = 0, used = 0;
        unsigned long long n = 0, cus = 0;
        if (std::sscanf(argv[i], "%d:%d:%llu:%llu%n", &hasher, &width, &n, &cus, &used) != 4) return 2;
        for (const char* s : kSwitches) unsetenv((std::string("BCOSGPU_MERKLE_") + s).c_str());
        std::string rest = argv[i][used] == ':' ? argv[i] + used + 1 : "";
        while (!rest.empty()) {
            const std::string kv = rest.substr(0, rest.find(','));
            rest.erase(0, kv.size() + 1);
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) return 2;
            setenv(("BCOSGPU_MERKLE_" + kv.substr(0, eq)).c_str(), kv.c_str() + eq + 1, 1);
        }
        const MerkleSwitches sw = parse_merkle_switches();
        const MerklePlan p = plan_merkle(hasher, width, n, cus, sw);
        static const char* const kinds[] = {"arg_error", "copy", "tree"};
        static const char* const names[] = {"climb", "fused", "two_launch", "levelwise"};
        std::printf("{\"kind\": \"%s\", \"switches\": [%d, %d, %d, %d, %d, %d, %d, %d], \"nlev\": %d, \"paths\": [",
                    kinds[p.kind], sw.levelwise, sw.fused, sw.climb, sw.sm3climb, sw.pair, sw.sm3x, sw.nosub,
                    sw.latsched, p.t.nlev);
        for (int k = 0; k < p.npaths; ++k) std::printf("%s\"%s\"", k ? ", " : "", names[p.paths[k]]);
        std::printf("]");
        for (int k = 0; k < p.npaths; ++k) {
            if (p.paths[k] == kPathClimb) {
                const MerklePlan::Climb& c = p.climb;
                std::printf(", \"climb\": {\"k\": %d, \"sub_grid\": %u, \"wgs\": %u, \"counters\": %u, \"latency\": %d, "
                            "\"x\": %d, \"B\": %d, \"kin\": %d, \"g\": %d, \"coop_max\": %u, \"pair_max\": %u, \"pair\": %d, ",
                            c.k, c.sub_grid, c.wgs, c.counters, c.latency, c.x, c.f.B, c.f.kin, c.f.g, c.f.coop_max,
                            c.f.pair_max, c.f.pair);
                print_tree("t", c.f.t);
                std::printf("}");
            } else if (p.paths[k] == kPathFused) {
                const MerklePlan::Fused& f = p.fused;
                std::printf(", \"fused\": {\"S\": %u, \"a\": %d, \"grid\": %u, \"counters\": %u, ", f.f.S, f.f.a, f.grid,
                            f.counters);
                print_tree("t", f.f.t);
                std::printf("}");
            } else if (p.paths[k] == kPathTwoLaunch) {
                const MerklePlan::TwoLaunch& w = p.two;
                std::printf(", \"two_launch\": {\"kin\": %d, \"B\": %u, \"grid\": %u, \"threads\": %u, \"pair\": %d, "
                            "\"sm3x\": %d, \"sm3x_top\": %d, \"nmid\": %d, \"top\": %d}",
                            w.kin, w.B, w.grid, w.threads, w.pair, w.sm3x, w.sm3x_top, w.nmid, w.top);
            }
        }
        std::printf("}\n");
    }
    return 0;
}
