// dcn_extend.h -- what the host and the device share of an extended placement (THE DEFINITION OF AN EXTENDED PLACEMENT,
// include/deacon_hip.h): the value of a candidate and the order among candidates, the stop of the loop, the score cap of
// a flank, and the whole flank on one thread (kernel in extend.hip, the C ABI in extend_api.hip).  The diagonals of the
// flank's wavefront are dcn_wavefront.h's (dcn_wf_diagonal with m = f, n = g), loaded by dcn_wf_guarded: a fetch that never
// reads in front of a stream.  Plain integer arithmetic: compiles for the host as well (tests/cpp/extend_flank_test.cpp),
// as dcn_pileup.h does.
//   A flank is two sequences that both begin at the placement's edge: U of the read, f bases, and V of the record, g
//   bases.  Each is a dcn_wf_side of its stream.  The right flank reads both forwards (the read backwards and
//   complemented when the row is reverse); the left flank reads both backwards.  A side that is read backwards comes
//   complemented out of dcn_wavefront.h; on the left flank either both sides are complemented or the read is read
//   forwards instead of backwards and complemented, and EQUAL does not change when both bases are complemented.
#pragma once

#include <stdint.h>

#include "dcn_wavefront.h"

// rule X4: the value of cell (i, i + k) at cost s
DCN_WF_FN int64_t dcn_ext_value(int64_t i, int64_t k, int64_t s, int64_t f, int64_t penalty, int64_t end_bonus) {
    return 2 * i + k - penalty * s + (i == f ? end_bonus : 0);
}

// rule X5 among the cells of one score: the larger value, then the larger i
DCN_WF_FN bool dcn_ext_better(int64_t value, int64_t i, int64_t than_value, int64_t than_i) {
    return value > than_value || (value == than_value && i > than_i);
}

// No cell of cost s + 1 or more can win: such a cell has j - i <= D, so its value is at most 2 f + end_bonus -
// (penalty - 1) D, and among equal values the smaller D wins.
DCN_WF_FN bool dcn_ext_done(int64_t s, int64_t f, int64_t penalty, int64_t end_bonus, int64_t best_value) {
    return 2 * f + end_bonus - (penalty - 1) * (s + 1) <= best_value;
}

// The largest cost a flank's wavefront is run to: rule X4's max_edits; no cell costs more than max(f, g); and (0, 0) has
// value >= 0, which no cell with (penalty - 1) D > 2 f + end_bonus reaches.
DCN_WF_FN uint32_t dcn_ext_cap(uint64_t f, uint64_t g, uint32_t penalty, uint32_t end_bonus, uint32_t max_edits) {
    uint64_t cap = max_edits;
    const uint64_t longest = f > g ? f : g, by_value = (2 * f + end_bonus) / (penalty - 1);
    if (longest < cap) cap = longest;
    if (by_value < cap) cap = by_value;
    return (uint32_t)cap;
}

// the best candidate of a flank so far: (i, i + k) at cost s
struct dcn_ext_best {
    int64_t value;
    int64_t s, i, k;
};

// One flank on one thread: rules X3-X5 by the wavefront.  `wave` holds two arrays of 2 * cap + 1 words.  This is the loop
// of the kernel without its lanes: there the diagonals of a score are dealt out and the best of a score is reduced.
DCN_WF_FN void dcn_ext_flank(const dcn_wf_side &U, const dcn_wf_side &V, uint32_t f, uint32_t g, uint32_t cap, uint32_t penalty,
                              uint32_t end_bonus, uint32_t *wave, uint32_t *i_out, uint32_t *j_out, uint32_t *d_out) {
    uint32_t *prev = wave, *cur = wave + (2 * (uint64_t)cap + 1);
    dcn_ext_best best = {INT64_MIN, 0, 0, 0};
    for (int64_t s = 0;; ++s) {
        const int64_t lo = dcn_wf_max(-s, -(int64_t)f), hi = dcn_wf_min(s, g);
        int64_t v_s = INT64_MIN, i_s = 0, k_s = 0;
        for (int64_t k = lo; k <= hi; ++k) {
            const int64_t i = dcn_wf_diagonal<dcn_wf_guarded>(prev, cap, s, k, f, g, U, V);
            cur[k + cap] = (uint32_t)i;
            const int64_t v = dcn_ext_value(i, k, s, f, penalty, end_bonus);
            if (dcn_ext_better(v, i, v_s, i_s)) v_s = v, i_s = i, k_s = k;
        }
        if (v_s > best.value) best = {v_s, s, i_s, k_s}; // (an equal value at a larger cost loses)
        if (s >= (int64_t)cap || dcn_ext_done(s, f, penalty, end_bonus, best.value)) break;
        uint32_t *const t = prev;
        prev = cur;
        cur = t;
    }
    *i_out = (uint32_t)best.i;
    *j_out = (uint32_t)(best.i + best.k);
    *d_out = (uint32_t)best.s;
}
