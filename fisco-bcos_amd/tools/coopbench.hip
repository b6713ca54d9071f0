// coopbench.hip -- phase timestamps (s_memtime cycles) of tx_verify_coop_kernel's (argv[1] = 26:
// tx_verify_coop26_kernel's, trio: tx_verify_trio26_kernel's) workgroup 0 on a
// 10k-tx batch of random inputs (the schedule is input-independent), to see where C2's latency goes.
// trio prints eight waves (0..3 the chains, 4..7 the helpers): the tx pairs' products before the inversion / the
// inversion / split / scalars posted / r^-1 posted on wave 0, the
// table's hand-offs on waves 1 .. 3, chain start and
// phase C per chain wave, the Z^-1, each helper's last result posted, kernel end.
#define BCOSGPU_COOP_TIMING 1
#include "../csrc/ecc_tables.hip"
#include "../csrc/ecc_coop.hip"
#include <cstdio>
#include <vector>

namespace bcosgpu {
// ecc_coop.hip's launcher names the row kernel's (ecc_row.hip), which this probe neither builds nor runs
template <class IO>
int launch_recover_row(const IO&, uint64_t, hipStream_t) {
    return BCOSGPU_E_ARG;
}
}  // namespace bcosgpu

int main(int argc, char** argv) {
    using namespace bcosgpu;
    const bool f26 = argc > 1 && argv[1][0] == '2';  // "26": tx_verify_coop26_kernel
    const bool trio = argc > 1 && argv[1][0] == 't';  // "trio": tx_verify_trio26_kernel (16-bit comb)
    if (ecc_init_tables(0, trio ? 0 : 1)) { printf("no device\n"); return 77; }
    const uint64_t n = 10000;
    std::vector<uint8_t> pre(n * 151), sig(n * 65);
    std::vector<uint64_t> po(n + 1), so(n + 1);
    uint32_t x = 12345;
    for (auto& b : pre) b = (x = x * 1103515245u + 12345u) >> 24;
    for (auto& b : sig) b = (x = x * 1103515245u + 12345u) >> 24;
    for (uint64_t i = 0; i <= n; ++i) { po[i] = 151 * i; so[i] = 65 * i; }
    for (uint64_t i = 0; i < n; ++i) sig[65 * i + 64] = 0;
    uint8_t *dp, *ds, *dh, *dsn, *dst;
    uint64_t *dpo, *dso;
    hipMalloc(&dp, pre.size()); hipMalloc(&ds, sig.size()); hipMalloc(&dpo, 8 * (n + 1)); hipMalloc(&dso, 8 * (n + 1));
    hipMalloc(&dh, 32 * n); hipMalloc(&dsn, 20 * n); hipMalloc(&dst, n);
    hipMemcpy(dp, pre.data(), pre.size(), hipMemcpyHostToDevice);
    hipMemcpy(ds, sig.data(), sig.size(), hipMemcpyHostToDevice);
    hipMemcpy(dpo, po.data(), 8 * (n + 1), hipMemcpyHostToDevice);
    hipMemcpy(dso, so.data(), 8 * (n + 1), hipMemcpyHostToDevice);
    const uint32_t *k1, *sm2;
    tables8(&k1, &sm2);
    const TxIO io{dp, dpo, ds, dso, dh, dsn, dst};
    for (int rep = 0; rep < 3; ++rep) {
        if (trio) {
            const uint32_t *w1, *w2;
            int bits = 8;
            tables(&w1, &w2, &bits);
            hipLaunchKernelGGL(tx_verify_trio26_kernel<TxIO>, dim3((n + 39) / 40), dim3(kTrioRecoverThreads), 0, 0, io, n, w1,
                               bits);
        } else if (f26)
            hipLaunchKernelGGL(tx_verify_coop26_kernel<TxIO>, dim3((n + 63) / 64), dim3(256), 0, 0, io, n, k1);
        else
            hipLaunchKernelGGL(tx_verify_coop_kernel, dim3((n + 63) / 64), dim3(256), 0, 0, dp, dpo, ds, dso, n, k1, dh,
                               dsn, dst);
        hipDeviceSynchronize();
    }
    uint64_t t[8][12];
    hipMemcpyFromSymbol(t, HIP_SYMBOL(g_coop_t), sizeof(t));
    if (trio) {
        // eight waves (0..3 the chains, 4..7 the helpers), all stamps since wave 0's start; 0 = not stamped
        // (signed: a wave can start a few cycles before wave 0)
        const auto at = [&](int w, int k) { return t[w][k] ? (long long)(t[w][k] - t[0][0]) : 0ll; };
        printf("{\"trio_stamps_since_wave0_start\": {");
        for (int w = 0; w < 8; ++w) {
            printf("%s\"wave%d\": {\"start\": %lld, \"phase_a_work_end\": %lld", w ? ", " : "", w, at(w, 0), at(w, 1));
            if (w == 0)
                printf(", \"pre_products_done\": %lld, \"inversion_done\": %lld, \"split_done\": %lld, "
                       "\"scalars_posted\": %lld, \"rinv_posted\": %lld",
                       at(w, 6), at(w, 10), at(w, 11), at(w, 8), at(w, 7));
            // the table on waves 1 .. 3 (trio_table_shared): wave 1 and 3 their multiples, wave 2 the prefix products
            // and Zc, wave 1 the suffix products, each its entries ("table_posted": its "done" flag)
            if (w == 1 || w == 3) printf(", \"multiples_posted\": %lld", at(w, 10));
            if (w == 2) printf(", \"prefix_posted\": %lld", at(w, 10));
            if (w == 1) printf(", \"suffix_posted\": %lld", at(w, 11));
            if (w >= 1 && w <= 3) printf(", \"table_posted\": %lld", at(w, 6));
            if (w < 4)
                printf(", \"chain_start\": %lld, \"phase_c_end\": %lld, \"phase_c\": %lld, \"phase_d_4\": %lld, "
                       "\"phase_d_5\": %lld",
                       at(w, 9), at(w, 2), at(w, 2) - at(w, 9), at(w, 4), at(w, 5));
            if (w == 1 || w == 3) printf(", \"root_wait_reached\": %lld", at(w, 8));
            if (w == 7) printf(", \"root_posted\": %lld", at(w, 6));
            if (w == 6) printf(", \"digest_posted\": %lld", at(w, 7));
            if (w >= 4) printf(", \"last_result_posted\": %lld", at(w, 10));
            printf(", \"kernel_end\": %lld}", at(w, 3));
        }
        printf("}, \"probes\": \"waves 0 / 2: phase_d_4 / 5 = start / end of Z^-1; waves 1 / 3: y loaded (the wait for the root's "
               "flag, reached at root_wait_reached, is over) / the last addition stored\"}\n");
        return 0;
    }
    printf("{\"cycles_since_start\": {");
    for (int w = 0; w < 4; ++w)
        printf("%s\"wave%d\": [%llu, %llu, %llu]", w ? ", " : "", w, (unsigned long long)(t[w][1] - t[w][0]),
               (unsigned long long)(t[w][2] - t[w][0]), (unsigned long long)(t[w][3] - t[w][0]));
    printf("}, \"probes6_7\": [");
    for (int w = 0; w < 4; ++w)
        printf("%s[%llu, %llu]", w ? ", " : "", (unsigned long long)(t[w][6] - t[w][0]), (unsigned long long)(t[w][7] - t[w][0]));
    uint64_t dt[4][8];
    hipMemcpyFromSymbol(dt, HIP_SYMBOL(g_dbl_t), sizeof(dt));
    printf("], \"dbl\": [");
    for (int w = 0; w < 4; ++w)
        printf("%s[%llu, %llu, %llu, %llu, %llu, %llu, %llu]", w ? ", " : "", (unsigned long long)(dt[w][1] - dt[w][0]),
               (unsigned long long)(dt[w][2] - dt[w][0]), (unsigned long long)(dt[w][3] - dt[w][0]),
               (unsigned long long)(dt[w][4] - dt[w][0]), (unsigned long long)(dt[w][5] - dt[w][0]),
               (unsigned long long)(dt[w][6] - dt[w][0]), (unsigned long long)(dt[w][7] - dt[w][0]));
    // trio with the split square root: waves 0 / 2 stamp the Z^-1 (start, end), waves 1 / 3 the end of the
    // root's tail and the end of the last addition
    printf("], \"phase_d_4_5\": [");
    for (int w = 0; w < 4; ++w)
        printf("%s[%llu, %llu]", w ? ", " : "", (unsigned long long)(t[w][4] - t[w][0]), (unsigned long long)(t[w][5] - t[w][0]));
    printf("], \"wave0_phase_d\": [%llu, %llu], \"probes\": \"end of phase A work, end of phase C loop, end of kernel; wave 0: before / after the affine inversion\"}\n",
           (unsigned long long)(t[0][4] - t[0][0]), (unsigned long long)(t[0][5] - t[0][0]));
    return 0;
}
