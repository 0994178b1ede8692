// dcn_blocks.h -- what the host and the device share of a reference block (THE DEFINITION OF A REFERENCE BLOCK,
// include/deacon_hip_blocks.h): the class of one position (rule B2) and the merge of two touching blocks (rule B6); kernels
// in blocks.hip, the C ABI in blocks_api.hip.  Plain integer arithmetic on top of dcn_genotype_decide: compiles for the
// host alone (tests/cpp/blocks_rule_test.cpp), as dcn_genotype.h does.  Nothing here is indexed by a runtime value: the GQ
// edges travel as sixteen bytes in two 64-bit words and are compared at constant shifts.
#pragma once

#include <stdint.h>

#include "dcn_genotype.h"

constexpr uint32_t DCN_BLK_NO_COVERAGE = 0, DCN_BLK_UNCALLED = 1, DCN_BLK_REF = 2, DCN_BLK_VARIANT = 255; // DCN_BLOCK_* of the header
constexpr uint32_t DCN_BLK_MAX_EDGES = 15;

// The edges as the rule takes them: byte i of lo | hi << 64 is e[i] for i < n_edges and 255 behind them, which no GQ reaches.
struct dcn_blk_edges {
    uint64_t lo, hi;
};

// edges[0 .. 16) as the API has checked them (entries from n_edges on are 0) -> the packed form
inline dcn_blk_edges dcn_blocks_pack_edges(const uint8_t *edges, uint32_t n_edges) {
    dcn_blk_edges e = {0, 0};
    for (uint32_t i = 0; i < 16; ++i) {
        const uint64_t byte = i < n_edges ? edges[i] : 255u;
        if (i < 8) e.lo |= byte << (8 * i);
        else e.hi |= byte << (8 * (i - 8));
    }
    return e;
}

// rule B2's b: the number of edges <= gq
DCN_GENO_FN uint32_t dcn_blocks_band(uint32_t gq, const dcn_blk_edges &e) {
    uint32_t b = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 8; ++i) {
        b += ((uint32_t)(e.lo >> (8 * i)) & 0xFFu) <= gq ? 1u : 0u;
        b += ((uint32_t)(e.hi >> (8 * i)) & 0xFFu) <= gq ? 1u : 0u;
    }
    return b;
}

struct dcn_blk_position {
    uint32_t cls;   // B2
    uint32_t gq;    // G4's, called or not
    uint32_t depth; // G1's D: the four base columns
};

// Rule B2 at one position that is not a break (a break is VARIANT whatever is here): n[A..T], Q[A..T], the N and DEL
// counters, ref_column = the column of the record's base (above T: invalid).
DCN_GENO_FN dcn_blk_position dcn_blocks_classify(const uint32_t *n, const uint32_t *Q, uint32_t n_n, uint32_t n_del, uint32_t ref_column,
                                                 const dcn_geno_params &p, const dcn_blk_edges &e) {
    uint8_t pl[DCN_GENO_GENOTYPES]; // (not looked at: the compiler drops the ten quotients)
    const dcn_geno_result r = dcn_genotype_decide(n, Q, ref_column, p, pl);
    const uint32_t D = n[0] + n[1] + n[2] + n[3];
    const uint64_t depth = (uint64_t)n[0] + n[1] + n[2] + n[3] + n_n + n_del; // P4's, six columns
    const uint32_t ref_hom = ref_column == 0 ? 0u : ref_column == 1 ? 2u : ref_column == 2 ? 5u : 9u;
    const uint32_t ref_gt = p.ploidy == 2 ? ref_hom : ref_column;
    dcn_blk_position out;
    out.gq = r.gq;
    out.depth = D;
    if (r.site) out.cls = DCN_BLK_VARIANT;
    else if (depth == 0) out.cls = DCN_BLK_NO_COVERAGE;
    else if (r.gt != DCN_GENO_NONE && ref_column <= 3u && r.best == ref_gt) out.cls = DCN_BLK_REF + dcn_blocks_band(r.gq, e);
    else out.cls = DCN_BLK_UNCALLED;
    return out;
}

// a dcn_reference_block of the public header, which tests/cpp does not include
struct dcn_blk_block {
    uint64_t pos, sum_depth;
    uint32_t len, min_depth, max_depth, min_gq, cls, reserved;
};

// rule B6: the two touch and have one class
DCN_GENO_FN bool dcn_blocks_mergeable(const dcn_blk_block &a, const dcn_blk_block &b) { return a.pos + a.len == b.pos && a.cls == b.cls; }

// rule B6: b into a (the caller has seen dcn_blocks_mergeable and that the lengths' sum fits 32 bits)
DCN_GENO_FN void dcn_blocks_merge_into(dcn_blk_block &a, const dcn_blk_block &b) {
    a.len += b.len;
    a.sum_depth += b.sum_depth;
    a.min_depth = b.min_depth < a.min_depth ? b.min_depth : a.min_depth;
    a.max_depth = b.max_depth > a.max_depth ? b.max_depth : a.max_depth;
    a.min_gq = b.min_gq < a.min_gq ? b.min_gq : a.min_gq;
}
