// dcn_indels.h -- what the host and the device share of a deletion ledger and of an indel genotype (THE DEFINITION OF A
// DELETION LEDGER and THE DEFINITION OF AN INDEL GENOTYPE, include/deacon_hip.h): an event as the device keeps it, what a
// run adds to a row's total, the event of one D run, the winner rule R5, and the costs and the decision of rules I2 - I5
// for one candidate (kernels in indels.hip, the C ABI in indels_api.hip).  Plain integer arithmetic, no division but the
// quotients by 100 of I4: compiles for the host alone (tests/cpp/indel_rule_test.cpp), as dcn_genotype.h does.
#pragma once

#include <stdint.h>

#include "dcn_pileup.h"

// the flag of an event (DCN_DELETION_REVERSE of the public header, which tests/cpp does not include)
constexpr uint32_t DCN_DEL_REVERSE = 1;
// the flags of a site (DCN_INDEL_* of the public header)
constexpr uint32_t DCN_INDEL_SITE_DELETION = 1, DCN_INDEL_SITE_FRONT = 2;

// One event of a ledger on the device: `base` is rule R2's p as a position of the base store.
struct dcn_del_event {
    uint64_t base;
    uint32_t len, flags;
};
static_assert(sizeof(dcn_del_event) == 16, "ledger event");

// what a run adds to its row's total: one event when it is a D run
DCN_PILE_FN uint32_t dcn_del_run_events(uint32_t run) { return (run & 15u) == DCN_ALN_D ? 1u : 0u; }

// Rule R2 for one D run that starts at j of a row whose T begins at store base t0
DCN_PILE_FN dcn_del_event dcn_del_event_of(uint32_t run, uint32_t j, uint32_t reverse, uint64_t t0) {
    dcn_del_event e;
    e.base = t0 + j;
    e.len = run >> 4;
    e.flags = reverse ? DCN_DEL_REVERSE : 0u;
    return e;
}

// Rule R5: the allele of length len_a with count_a beats the one of length len_b with count_b
DCN_PILE_FN bool dcn_del_beats(uint32_t count_a, uint32_t len_a, uint32_t count_b, uint32_t len_b) {
    if (count_a != count_b) return count_a > count_b;
    return len_a < len_b;
}

// Rule R5 over the `count` events of one start, slots[0 .. count) naming them among `events`, as lane `lane` of `lanes`
// sees it: each of the lane's events is counted against all of the position's (quadratic in the events of one position,
// as dcn_ins_lane_winner).  -> the length of the lane's best, *best_count its count, 0 when the lane has no event.  The
// caller reduces the lanes with dcn_del_beats.
DCN_PILE_FN uint32_t dcn_del_lane_winner(const uint64_t *slots, uint32_t count, uint32_t lane, uint32_t lanes, const dcn_del_event *events,
                                         uint32_t *best_count) {
    uint32_t best_len = 0, best_c = 0;
    for (uint32_t k = lane; k < count; k += lanes) {
        const uint32_t len = events[slots[k]].len;
        uint32_t c = 0;
        for (uint32_t t = 0; t < count; ++t) c += events[slots[t]].len == len ? 1u : 0u;
        if (best_c == 0 || dcn_del_beats(c, len, best_c, best_len)) best_len = len, best_c = c;
    }
    *best_count = best_c;
    return best_len;
}

// ---- rules I1 - I5: one candidate ----------------------------------------------------------------------------------------
// the fields of dcn_indel_params that the rule reads (the API has checked them)
struct dcn_indel_prm {
    uint32_t ploidy, min_depth, min_gq, min_qual, min_count, indel_centi, het_centi;
};

struct dcn_indel_result {
    uint32_t gt;   // I4's best: the genotype's index in I3's order
    uint32_t gq;   // I4
    uint32_t qual; // I4
    uint32_t site; // I5: 0 or 1
};

// rule I1: a candidate with count a stays
DCN_PILE_FN bool dcn_indel_candidate(uint32_t a, uint32_t min_count) { return a >= (min_count > 1u ? min_count : 1u); }

// min(cap, diff / 100) for cap < 2^32 / 100, with a 32-bit quotient: diff / 100 >= cap exactly when diff >= 100 cap
DCN_PILE_FN uint32_t dcn_indel_centi_capped(uint64_t diff, uint32_t cap) {
    const uint64_t top = (uint64_t)cap * 100u + 99u;
    return (uint32_t)(diff < top ? diff : top) / 100u;
}

// a = the reads that carry the allele, depth = P4's depth -> the result and pl[0 .. 3) (rules I2 - I5).  Every cost is at
// most 100000 * 2^33 < 2^50.
DCN_PILE_FN dcn_indel_result dcn_indel_decide(uint32_t a, uint32_t depth, const dcn_indel_prm &p, uint8_t *pl) {
    const uint64_t A = a, O = depth >= a ? depth - a : 0u; // I2
    const bool diploid = p.ploidy == 2;
    const uint64_t absent = UINT64_MAX; // a genotype the ploidy does not have: never the best, never the second
    // I3, in VCF order
    const uint64_t c0 = (uint64_t)p.indel_centi * A;
    const uint64_t c1 = diploid ? (uint64_t)p.het_centi * (A + O) : (uint64_t)p.indel_centi * O;
    const uint64_t c2 = diploid ? (uint64_t)p.indel_centi * O : absent;
    // I4: the first smallest wins
    uint64_t best_cost = c0, second = absent;
    uint32_t best = 0;
    if (c1 < best_cost) second = best_cost, best_cost = c1, best = 1;
    else if (c1 < second) second = c1;
    if (c2 < best_cost) second = best_cost, best_cost = c2, best = 2;
    else if (c2 < second) second = c2;
    dcn_indel_result r;
    r.gt = best;
    r.gq = dcn_indel_centi_capped(second - best_cost, 99u);
    pl[0] = (uint8_t)dcn_indel_centi_capped(c0 - best_cost, 255u);
    pl[1] = (uint8_t)dcn_indel_centi_capped(c1 - best_cost, 255u);
    pl[2] = diploid ? (uint8_t)dcn_indel_centi_capped(c2 - best_cost, 255u) : (uint8_t)0;
    const uint64_t qual64 = (c0 - best_cost) / 100u;
    r.qual = qual64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)qual64;
    // I5
    const bool called = depth >= (p.min_depth > 1u ? p.min_depth : 1u) && r.gq >= p.min_gq;
    r.site = called && best != 0u && r.qual >= p.min_qual ? 1u : 0u;
    return r;
}
