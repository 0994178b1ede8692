// dcn_entropy.h -- the index side's scaled-entropy floor (src/minimizers.rs:73-121) for the kernels that insert dumped
// minimizers (index_table.hip, index_builder.hip).  Everything here is local to the including file: each has its own
// copy of the table on each device and fills it before its first launch there that reads it (dcn_entropy_table_ready).
#pragma once

#include "dcn_internal.h"

#include <cmath>

// p * log2(p) for p = count/total, computed on the HOST in f32 exactly as calculate_scaled_entropy does
// (src/minimizers.rs:110-116), so the device only subtracts table entries in the reference's order
constexpr int ENT_MAX = 57;
static __device__ float g_plogp[ENT_MAX][ENT_MAX];

__device__ inline float scaled_entropy_dev(const uint8_t *kmer, uint32_t k) { // src/minimizers.rs:73-121
    if (k < 10) return 1.0f;
    uint32_t cnt[4] = {0, 0, 0, 0};
    uint32_t total = 0;
    for (uint32_t i = 0; i < k; ++i) {
        uint32_t c = kmer[i] | 0x20u;
        int j = c == 'a' ? 0 : c == 'c' ? 1 : c == 'g' ? 2 : c == 't' ? 3 : -1;
        if (j >= 0) {
            cnt[j]++;
            total++;
        }
    }
    if (total == 0) return 1.0f;
    float entropy = 0.0f;
    for (int j = 0; j < 4; ++j)
        if (cnt[j] > 0) entropy = __fsub_rn(entropy, g_plogp[total][cnt[j]]);
    return __fdiv_rn(entropy, 2.0f);
}

// (the table lives in device memory: one copy per device, filled on the device that is current when it is first needed)
static int dcn_entropy_table_ready() {
    constexpr int MAX_DEVICES = 64;
    static bool table_ready[MAX_DEVICES] = {};
    int dev = 0;
    DCN_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= MAX_DEVICES) return dcn_fail(DCN_ERR_ARG, "entropy table: device number out of range");
    if (table_ready[dev]) return DCN_OK;
    static float host_tab[ENT_MAX][ENT_MAX];
    for (int t = 1; t < ENT_MAX; ++t)
        for (int c = 1; c <= t; ++c) {
            float p = (float)c / (float)t;
            host_tab[t][c] = p * log2f(p);
        }
    DCN_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_plogp), host_tab, sizeof(host_tab)));
    table_ready[dev] = true;
    return DCN_OK;
}
