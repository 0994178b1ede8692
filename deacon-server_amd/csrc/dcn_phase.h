// dcn_phase.h -- what the host and the device share of a phase (THE DEFINITION OF A PHASE, include/deacon_hip_phase.h): the
// observation of a column at a site (H2), the decision over a link's four counters (H5), and the element and operator of the
// segmented scan that turns decisions into sets (H6); kernels in phase.hip, the C ABI in phase_api.hip.  Plain integer
// arithmetic: compiles for the host as well (tests/cpp/phase_rule_test.cpp), as dcn_pileup.h does.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DCN_PHASE_FN __host__ __device__ inline
#else
#define DCN_PHASE_FN inline
#endif

// ---- rule H2: the observation of a pileup column at a site with alleles (a0, a1) --------------------------------------
constexpr uint32_t DCN_PHASE_NONE = 2;
// a site's alleles as the device keeps them: a0 | a1 << 2
DCN_PHASE_FN uint32_t dcn_phase_pack_alleles(uint32_t a0, uint32_t a1) { return (a0 & 3u) | (a1 & 3u) << 2; }
// column: what dcn_pile_column / dcn_pile_qual_column give (A C G T N), or DEL
DCN_PHASE_FN uint32_t dcn_phase_observation(uint32_t column, uint32_t alleles) {
    return column > 3u ? DCN_PHASE_NONE : column == (alleles & 3u) ? 0u : column == ((alleles >> 2) & 3u) ? 1u : DCN_PHASE_NONE;
}
// rule H3: the counter of a pair of defined observations among the four of a link
DCN_PHASE_FN uint32_t dcn_phase_counter(uint32_t x, uint32_t y) { return x * 2u + y; }

// ---- rule H5: the decision over n00 n01 n10 n11 -----------------------------------------------------------------------
constexpr uint32_t DCN_PHASE_DEC_JOINED = 1, DCN_PHASE_DEC_TRANS = 2; // TRANS: r = 1 (only ever set beside JOINED)
DCN_PHASE_FN uint32_t dcn_phase_decide(const uint32_t *n, uint32_t min_reads, uint32_t max_minor_permille) {
    const uint64_t c = (uint64_t)n[0] + n[3], t = (uint64_t)n[1] + n[2], total = c + t, minor = c < t ? c : t;
    const uint64_t need = min_reads > 1u ? min_reads : 1u;
    if (total < need || c == t || minor * 1000u > total * max_minor_permille) return 0u;
    return DCN_PHASE_DEC_JOINED | (t > c ? DCN_PHASE_DEC_TRANS : 0u);
}

// ---- rule H6: the segmented scan ---------------------------------------------------------------------------------------
// The element of a stretch of sites: the heads in it, the XOR of the relations behind its last head (behind its start when
// it has none), and the index of its last head (0 when it has none).
struct dcn_phase_elem {
    uint32_t heads, x;
    uint64_t last;
};
// what site s alone is: dec_before = the decision of link s - 1, 0 where there is none (s == 0, a record change)
DCN_PHASE_FN dcn_phase_elem dcn_phase_site_elem(uint64_t s, uint32_t dec_before) {
    const bool head = !(dec_before & DCN_PHASE_DEC_JOINED);
    dcn_phase_elem r;
    r.heads = head ? 1u : 0u;
    r.x = !head && (dec_before & DCN_PHASE_DEC_TRANS) ? 1u : 0u;
    r.last = head ? s : 0u;
    return r;
}
DCN_PHASE_FN dcn_phase_elem dcn_phase_identity() {
    dcn_phase_elem r;
    r.heads = 0u, r.x = 0u, r.last = 0u;
    return r;
}
// a stretch followed by the stretch behind it: associative, and the right operand's x and last win when it holds a head
DCN_PHASE_FN dcn_phase_elem dcn_phase_combine(const dcn_phase_elem &a, const dcn_phase_elem &b) {
    dcn_phase_elem r; // (selects, not branches: the scan kernels keep the three fields in registers)
    r.heads = a.heads + b.heads;
    r.x = b.heads ? b.x : a.x ^ b.x;
    r.last = b.heads ? b.last : a.last;
    return r;
}

// sites of one workgroup of the scan kernels (a site per thread); tests/test_gpu_phase_seams.py reads it from here
constexpr uint32_t DCN_PHASE_SCAN_BLOCK = 256;
