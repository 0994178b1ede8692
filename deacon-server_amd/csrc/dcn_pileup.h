// dcn_pileup.h -- what the host and the device share of a pileup (THE DEFINITION OF A PILEUP, include/deacon_hip.h): where a
// counter lies, how far a run moves on S and on T, the adds of one run, the same with base qualities (THE DEFINITION OF A
// QUALITY-AWARE PILEUP), and the call of one position (kernels in pileup.hip, the C ABI in pileup_api.hip).  Plain integer
// arithmetic: compiles for the host as well (tests/cpp/pileup_walk_test.cpp, pileup_qual_walk_test.cpp), as dcn_align.h does.
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

// rule S2 (THE DEFINITION OF STRAND EVIDENCE): a map that keeps no strand planes adds nothing
struct dcn_pile_no_strand {
    DCN_PILE_FN void operator()(uint32_t, uint32_t) const {}
};

// Where reverse counter (column, base) lies among the 4 * bases words of a map's strand planes RA RC RG RT: four planes, as
// the counters'; four words per position under -DDCN_PILEUP_POSITION_MAJOR.
constexpr uint32_t DCN_PILE_STRAND_COLUMNS = 4;
DCN_PILE_FN uint64_t dcn_pile_strand_index(uint32_t column, uint64_t base, uint64_t bases) {
#if defined(DCN_PILEUP_POSITION_MAJOR)
    (void)bases;
    return base * DCN_PILE_STRAND_COLUMNS + column;
#else
    return (uint64_t)column * bases + base;
#endif
}

// Rule P3 for one run that starts at (i, j), as lane `lane` of `lanes` sees it: the lanes stride over the run's bases.
// column_of(i) is the column of S[i]; add(column, j) adds 1 at base j of T.  An I run is one add, by lane 0, at the base of
// T in front of it (at base 0 when there is none: the caller has n > 0).  add_strand(column, j) is rule S2's add: called on
// a reverse row alone, for an '=' or X step counted in A, C, G or T.
template <typename ColumnOf, typename Add, typename AddStrand = dcn_pile_no_strand>
DCN_PILE_FN void dcn_pile_run(uint32_t run, uint32_t i, uint32_t j, uint32_t reverse, uint32_t lane, uint32_t lanes, ColumnOf column_of,
                              Add add, AddStrand add_strand = AddStrand()) {
    const uint32_t op = run & 15u, len = run >> 4;
    if (op == DCN_ALN_I) {
        if (lane == 0) add(DCN_PILE_INS, j > 0 ? j - 1 : 0u);
        return;
    }
    for (uint32_t q = lane; q < len; q += lanes) {
        const uint32_t column = op == DCN_ALN_D ? DCN_PILE_DEL : column_of(i + q);
        add(column, j + q);
        if (reverse) {
            add(DCN_PILE_REV, j + q);
            if (column <= DCN_PILE_T) add_strand(column, j + q);
        }
    }
}

// ---- rules Q2 - Q4: base qualities (THE DEFINITION OF A QUALITY-AWARE PILEUP) -------------------------------------------
constexpr uint32_t DCN_PILE_SUM_COLUMNS = 4; // QA QC QG QT

// rule Q2: the quality of a byte of the quality array; a byte below the offset is quality 0
DCN_PILE_FN uint32_t dcn_pile_quality(uint32_t byte, uint32_t qual_offset) { return byte >= qual_offset ? byte - qual_offset : 0u; }

// rule Q2: where in the batch the quality of S[i] lies.  s_origin is the row's (dcn_verify_item): the first base of the read
// interval, or its end on a reverse row, where S[i] is the complement of the base at s_origin - 1 - i.
DCN_PILE_FN int64_t dcn_pile_qual_pos(int64_t s_origin, uint32_t reverse, uint32_t i) {
    return reverse ? s_origin - 1 - (int64_t)i : s_origin + (int64_t)i;
}

// rule Q3: a base column under the threshold counts as N; N stays N
DCN_PILE_FN uint32_t dcn_pile_qual_column(uint32_t column, uint32_t q, uint32_t min_base_qual) {
    return column <= DCN_PILE_T && q < min_base_qual ? DCN_PILE_N : column;
}

// Where sum (column, base) lies among the 4 * bases words of a map's quality sums: four planes, as the counters'; four
// words per position under -DDCN_PILEUP_POSITION_MAJOR.
DCN_PILE_FN uint64_t dcn_pile_sum_index(uint32_t column, uint64_t base, uint64_t bases) {
#if defined(DCN_PILEUP_POSITION_MAJOR)
    (void)bases;
    return base * DCN_PILE_SUM_COLUMNS + column;
#else
    return (uint64_t)column * bases + base;
#endif
}

// Rules Q3 and Q4 for one run: dcn_pile_run with the quality of every '=' / X base looked at.  quality_of(i) is q(S[i]);
// add_sum(column, j, q) adds q to the sum of a base column at base j of T.  I and D runs are dcn_pile_run's.
// add_strand is dcn_pile_run's, with the column of rule Q3.
template <typename ColumnOf, typename QualityOf, typename Add, typename AddSum, typename AddStrand = dcn_pile_no_strand>
DCN_PILE_FN void dcn_pile_run_qual(uint32_t run, uint32_t i, uint32_t j, uint32_t reverse, uint32_t min_base_qual, uint32_t lane, uint32_t lanes,
                                   ColumnOf column_of, QualityOf quality_of, Add add, AddSum add_sum, AddStrand add_strand = AddStrand()) {
    const uint32_t op = run & 15u, len = run >> 4;
    if (op == DCN_ALN_I) {
        if (lane == 0) add(DCN_PILE_INS, j > 0 ? j - 1 : 0u);
        return;
    }
    for (uint32_t q = lane; q < len; q += lanes) {
        uint32_t column = DCN_PILE_DEL;
        if (op == DCN_ALN_D) {
            add(DCN_PILE_DEL, j + q);
        } else {
            const uint32_t quality = quality_of(i + q);
            column = dcn_pile_qual_column(column_of(i + q), quality, min_base_qual);
            add(column, j + q);
            if (column <= DCN_PILE_T) add_sum(column, j + q, quality);
        }
        if (reverse) {
            add(DCN_PILE_REV, j + q);
            if (column <= DCN_PILE_T) add_strand(column, j + q);
        }
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
