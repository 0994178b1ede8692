// dcn_pileup.h -- what the host and the device share of a pileup (THE DEFINITION OF A PILEUP, include/deacon_hip.h): where a
// counter lies, how far a run moves on S and on T, the adds of one run, and the call of one position (kernels in
// pileup.hip, the C ABI in pileup_api.hip).  Plain integer arithmetic: compiles for the host as well
// (tests/cpp/pileup_walk_test.cpp), as dcn_align.h does.
#pragma once

#include <stdint.h>

#include "dcn_align.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DCN_PILE_FN __host__ __device__ inline
#else
#define DCN_PILE_FN inline
#endif

// the columns (DCN_PILEUP_* of the public header, which tests/cpp does not include)
constexpr uint32_t DCN_PILE_A = 0, DCN_PILE_C = 1, DCN_PILE_G = 2, DCN_PILE_T = 3, DCN_PILE_N = 4, DCN_PILE_DEL = 5, DCN_PILE_INS = 6,
                   DCN_PILE_REV = 7, DCN_PILE_COLUMNS = 8;

// Where counter (column, base) lies among the 8 * bases words of a map's pileup; `base` is a position of the base store.
// Column-major: eight planes of `bases` words, so the lanes of one wave instruction, which add to consecutive positions
// of one column, add to consecutive words.  -DDCN_PILEUP_POSITION_MAJOR is the other form, for measuring (DESIGN.md
// section 17): eight words per position.
DCN_PILE_FN uint64_t dcn_pile_index(uint32_t column, uint64_t base, uint64_t bases) {
#if defined(DCN_PILEUP_POSITION_MAJOR)
    (void)bases;
    return base * DCN_PILE_COLUMNS + column;
#else
    return (uint64_t)column * bases + base;
#endif
}

// the step of a run len << 4 | op: how far it moves on S (i) and on T (j)
DCN_PILE_FN uint32_t dcn_pile_step_s(uint32_t run) { return (run & 15u) == DCN_ALN_D ? 0u : run >> 4; }
DCN_PILE_FN uint32_t dcn_pile_step_t(uint32_t run) { return (run & 15u) == DCN_ALN_I ? 0u : run >> 4; }

// the column of a base of S: the pack kernel's codes are A C T G, the columns A C G T; an invalid base counts as N
DCN_PILE_FN uint32_t dcn_pile_column(uint32_t code, uint32_t invalid) { return invalid ? DCN_PILE_N : (code ^ (code >> 1)) & 3u; }

// Rule P3 for one run that starts at (i, j), as lane `lane` of `lanes` sees it: the lanes stride over the run's bases.
// column_of(i) is the column of S[i]; add(column, j) adds 1 at base j of T.  An I run is one add, by lane 0, at the base of
// T in front of it (at base 0 when there is none: the caller has n > 0).
template <typename ColumnOf, typename Add>
DCN_PILE_FN void dcn_pile_run(uint32_t run, uint32_t i, uint32_t j, uint32_t reverse, uint32_t lane, uint32_t lanes, ColumnOf column_of,
                              Add add) {
    const uint32_t op = run & 15u, len = run >> 4;
    if (op == DCN_ALN_I) {
        if (lane == 0) add(DCN_PILE_INS, j > 0 ? j - 1 : 0u);
        return;
    }
    for (uint32_t q = lane; q < len; q += lanes) {
        add(op == DCN_ALN_D ? DCN_PILE_DEL : column_of(i + q), j + q);
        if (reverse) add(DCN_PILE_REV, j + q);
    }
}

// ---- rule P6: the call of one position --------------------------------------------------------------------------------
constexpr uint32_t DCN_PILE_SITE_SUB = 1, DCN_PILE_SITE_DEL = 2, DCN_PILE_SITE_INS = 4, DCN_PILE_NO_CODE = 7;

// counts[0 .. 7) of a position (REV is not looked at), ref_column = the column of the record's base (N: invalid)
// -> site_info = flags | call_code << 8 | ref_code << 16
DCN_PILE_FN uint32_t dcn_pile_call(const uint32_t *counts, uint32_t ref_column, uint32_t min_depth, uint32_t min_permille) {
    uint64_t depth = 0;
    for (uint32_t c = 0; c <= DCN_PILE_DEL; ++c) depth += counts[c];
    uint32_t best = DCN_PILE_A, best_count = counts[DCN_PILE_A]; // the first of A, C, G, T, DEL with the largest count
    for (uint32_t c = DCN_PILE_C; c <= DCN_PILE_T; ++c)
        if (counts[c] > best_count) best = c, best_count = counts[c];
    if (counts[DCN_PILE_DEL] > best_count) best = DCN_PILE_DEL, best_count = counts[DCN_PILE_DEL];
    const bool deep = depth > 0 && depth >= min_depth;
    const bool called = deep && (uint64_t)best_count * 1000u >= depth * min_permille;
    const uint32_t call_code = !called ? DCN_PILE_NO_CODE : best == DCN_PILE_DEL ? 4u : best;
    const uint32_t ref_code = ref_column <= DCN_PILE_T ? ref_column : DCN_PILE_NO_CODE;
    uint32_t flags = 0;
    if (called && best != DCN_PILE_DEL && best != ref_code) flags |= DCN_PILE_SITE_SUB;
    if (called && best == DCN_PILE_DEL) flags |= DCN_PILE_SITE_DEL;
    if (deep && (uint64_t)counts[DCN_PILE_INS] * 1000u >= depth * min_permille) flags |= DCN_PILE_SITE_INS;
    return flags | call_code << 8 | ref_code << 16;
}

// the character of a call code
DCN_PILE_FN uint8_t dcn_pile_call_char(uint32_t site_info) {
    const uint32_t code = (site_info >> 8) & 0xFFu;
    return code == 0 ? 'A' : code == 1 ? 'C' : code == 2 ? 'G' : code == 3 ? 'T' : code == 4 ? '-' : 'N';
}
