// dcn_extend.h -- what the host and the device share of an extended placement (THE DEFINITION OF AN EXTENDED PLACEMENT,
// include/deacon_hip.h): a fetch that never reads in front of a stream, one diagonal of the flank's wavefront, the value
// of a candidate and the order among candidates, the stop of the loop, the score cap of a flank, and the whole flank on
// one thread (kernel in extend.hip, the C ABI in extend_api.hip).  Plain integer arithmetic: compiles for the host as well
// (tests/cpp/extend_flank_test.cpp), as dcn_pileup.h does.
//   A flank is two sequences that both begin at the placement's edge: U of the read, f bases, and V of the record, g
//   bases.  Each is a dcn_vfy_side of its stream.  The right flank reads both forwards (the read backwards and
//   complemented when the row is reverse); the left flank reads both backwards.  A side that is read backwards comes
//   complemented out of dcn_verify_words.h; on the left flank either both sides are complemented or the read is read
//   forwards instead of backwards and complemented, and EQUAL does not change when both bases are complemented.
#pragma once

#include <stdint.h>

#include "dcn_verify_words.h"

#define DCN_EXT_FN DCN_VFY_FN

// dcn_vfy_fetch16 / dcn_vfy_mask16 for a stream that has no pad words in front (the base store): a side that is read
// backwards asks for the 16 bases in front of a base, which begin up to 15 bases in front of base 0 of the stream when
// the base is one of its first 16.  Words in front of word 0 read as 0: the bases they would hold lie in front of the
// flank's last base, where no match run looks (every run is limited to the flank).
DCN_EXT_FN uint32_t dcn_ext_word(const uint32_t *words, int64_t w) { return w < 0 ? 0u : words[w]; }

DCN_EXT_FN uint32_t dcn_ext_fetch16(const uint32_t *packed, int64_t b) {
    const int64_t w = b >> 4; // (floor)
    const uint32_t sh = (uint32_t)(b & 15) * 2u;
    const uint64_t two = (uint64_t)dcn_ext_word(packed, w) | ((uint64_t)dcn_ext_word(packed, w + 1) << 32);
    return (uint32_t)(two >> sh);
}

DCN_EXT_FN uint32_t dcn_ext_mask16(const uint32_t *invmask, int64_t b) {
    const int64_t w = b >> 5;
    const uint32_t sh = (uint32_t)(b & 31);
    const uint64_t two = (uint64_t)dcn_ext_word(invmask, w) | ((uint64_t)dcn_ext_word(invmask, w + 1) << 32);
    return (uint32_t)(two >> sh) & 0xFFFFu;
}

// dcn_vfy_side16 over those two
DCN_EXT_FN void dcn_ext_side16(const dcn_vfy_side &s, int64_t i, uint32_t *x, uint32_t *inv) {
    if (s.reverse) {
        const int64_t b = s.origin - i - 16;
        *x = dcn_vfy_revcomp16(dcn_ext_fetch16(s.packed, b));
        *inv = dcn_vfy_rev16(dcn_ext_mask16(s.invmask, b));
    } else {
        *x = dcn_ext_fetch16(s.packed, s.origin + i);
        *inv = dcn_ext_mask16(s.invmask, s.origin + i);
    }
}

// the length of the run of EQUAL bases U[i + t] == V[j + t], t = 0, 1, ..., at most `limit`.  The caller's limit is
// min(f - i, g - j): behind a flank lies another read of the batch or another record of the store, whose bases may well
// continue the match.
DCN_EXT_FN uint64_t dcn_ext_match_run(const dcn_vfy_side &U, int64_t i, const dcn_vfy_side &V, int64_t j, uint64_t limit) {
    uint64_t t = 0;
    while (t < limit) {
        uint32_t xu, iu, xv, iv;
        dcn_ext_side16(U, i + (int64_t)t, &xu, &iu);
        dcn_ext_side16(V, j + (int64_t)t, &xv, &iv);
        const uint32_t r = dcn_vfy_run16(xu, xv, iu | iv);
        t += r;
        if (r < 16u) break;
    }
    return t < limit ? t : limit;
}

DCN_EXT_FN int64_t dcn_ext_min(int64_t a, int64_t b) { return a < b ? a : b; }
DCN_EXT_FN int64_t dcn_ext_max(int64_t a, int64_t b) { return a > b ? a : b; }

// F_s[k]: the furthest base i of U that a path of cost <= s reaches on diagonal k = j - i, for max(-s, -f) <= k <=
// min(s, g).  `prev` holds F_{s-1}, diagonal k at prev[k + center]; it is not read at s = 0.  The recurrence, the cut to
// the rectangle and why no position is negative: verify.hip, with m = f and n = g.
DCN_EXT_FN int64_t dcn_ext_diagonal(const uint32_t *prev, int64_t center, int64_t s, int64_t k, int64_t f, int64_t g,
                                    const dcn_vfy_side &U, const dcn_vfy_side &V) {
    int64_t i = 0;
    if (s > 0) {
        const int64_t plo = dcn_ext_max(1 - s, -f), phi = dcn_ext_min(s - 1, g); // the diagonals of score s - 1
        i = -1;
        if (k >= plo && k <= phi) i = (int64_t)prev[k + center] + 1;
        if (k - 1 >= plo && k - 1 <= phi) i = dcn_ext_max(i, (int64_t)prev[k - 1 + center]);
        if (k + 1 >= plo && k + 1 <= phi) i = dcn_ext_max(i, (int64_t)prev[k + 1 + center] + 1);
        i = dcn_ext_min(i, dcn_ext_min(f, g - k));
    }
    const int64_t j = i + k;
    if (i >= 0 && j >= 0) { // (always; a position that were not would read nothing)
        const int64_t room = dcn_ext_min(f - i, g - j);
        if (room > 0) i += (int64_t)dcn_ext_match_run(U, i, V, j, (uint64_t)room);
    }
    return dcn_ext_max(i, 0);
}

// rule X4: the value of cell (i, i + k) at cost s
DCN_EXT_FN int64_t dcn_ext_value(int64_t i, int64_t k, int64_t s, int64_t f, int64_t penalty, int64_t end_bonus) {
    return 2 * i + k - penalty * s + (i == f ? end_bonus : 0);
}

// rule X5 among the cells of one score: the larger value, then the larger i
DCN_EXT_FN bool dcn_ext_better(int64_t value, int64_t i, int64_t than_value, int64_t than_i) {
    return value > than_value || (value == than_value && i > than_i);
}

// No cell of cost s + 1 or more can win: such a cell has j - i <= D, so its value is at most 2 f + end_bonus -
// (penalty - 1) D, and among equal values the smaller D wins.
DCN_EXT_FN bool dcn_ext_done(int64_t s, int64_t f, int64_t penalty, int64_t end_bonus, int64_t best_value) {
    return 2 * f + end_bonus - (penalty - 1) * (s + 1) <= best_value;
}

// The largest cost a flank's wavefront is run to: rule X4's max_edits; no cell costs more than max(f, g); and (0, 0) has
// value >= 0, which no cell with (penalty - 1) D > 2 f + end_bonus reaches.
DCN_EXT_FN uint32_t dcn_ext_cap(uint64_t f, uint64_t g, uint32_t penalty, uint32_t end_bonus, uint32_t max_edits) {
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
DCN_EXT_FN void dcn_ext_flank(const dcn_vfy_side &U, const dcn_vfy_side &V, uint32_t f, uint32_t g, uint32_t cap, uint32_t penalty,
                              uint32_t end_bonus, uint32_t *wave, uint32_t *i_out, uint32_t *j_out, uint32_t *d_out) {
    uint32_t *prev = wave, *cur = wave + (2 * (uint64_t)cap + 1);
    dcn_ext_best best = {INT64_MIN, 0, 0, 0};
    for (int64_t s = 0;; ++s) {
        const int64_t lo = dcn_ext_max(-s, -(int64_t)f), hi = dcn_ext_min(s, g);
        int64_t v_s = INT64_MIN, i_s = 0, k_s = 0;
        for (int64_t k = lo; k <= hi; ++k) {
            const int64_t i = dcn_ext_diagonal(prev, cap, s, k, f, g, U, V);
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
