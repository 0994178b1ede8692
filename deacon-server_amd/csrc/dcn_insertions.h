// dcn_insertions.h -- what the host and the device share of an insertion ledger (THE DEFINITION OF AN INSERTION LEDGER,
// include/deacon_hip.h): an event as the device keeps it, what a run adds to a row's totals, the write of one I run, the
// order of alleles and the winner rule (kernels in insertions.hip, the C ABI in insertions_api.hip).  Plain integer
// arithmetic: compiles for the host as well (tests/cpp/insertion_walk_test.cpp), as dcn_pileup.h does.
#pragma once

#include <stdint.h>

#include "dcn_pileup.h"

// the flags of an event (DCN_INSERTION_* of the public header, which tests/cpp does not include)
constexpr uint32_t DCN_INS_FRONT = 1, DCN_INS_REVERSE = 2;

// One event of a ledger on the device: `base` is rule L2's p as a position of the base store, bases_offset where its
// bases begin among the ledger's.
struct dcn_ins_event {
    uint64_t base, bases_offset;
    uint32_t len, flags;
};
static_assert(sizeof(dcn_ins_event) == 24, "ledger event");

// what a run adds to its row's totals: one event, and its bases, when it is an I run
DCN_PILE_FN uint32_t dcn_ins_run_events(uint32_t run) { return (run & 15u) == DCN_ALN_I ? 1u : 0u; }
DCN_PILE_FN uint32_t dcn_ins_run_bases(uint32_t run) { return (run & 15u) == DCN_ALN_I ? run >> 4 : 0u; }

// the character of a base of S: upper case, N for an invalid one (dcn_pile_column's order is A C G T N)
DCN_PILE_FN uint8_t dcn_ins_char(uint32_t code, uint32_t invalid) {
    const uint32_t column = dcn_pile_column(code, invalid);
    return column == DCN_PILE_A ? 'A' : column == DCN_PILE_C ? 'C' : column == DCN_PILE_G ? 'G' : column == DCN_PILE_T ? 'T' : 'N';
}

// Rule L2 for one I run that starts at (i, j) of a row whose T begins at store base t0, as lane `lane` of `lanes` sees
// it: lane 0 stores the event at events[event_at], the lanes stride over the run's bases into bases[base_at ..).
// char_of(i) is the character of S[i].  The position is P3's: the base of T in front, or base 0 with FRONT when j = 0.
template <typename CharOf>
DCN_PILE_FN void dcn_ins_write_run(uint32_t run, uint32_t i, uint32_t j, uint32_t reverse, uint64_t t0, uint64_t event_at, uint64_t base_at,
                                   uint32_t lane, uint32_t lanes, CharOf char_of, dcn_ins_event *events, uint8_t *bases) {
    const uint32_t len = run >> 4;
    if (lane == 0) {
        dcn_ins_event e;
        e.base = t0 + (j > 0 ? j - 1 : 0u);
        e.bases_offset = base_at;
        e.len = len;
        e.flags = (j == 0 ? DCN_INS_FRONT : 0u) | (reverse ? DCN_INS_REVERSE : 0u);
        events[event_at] = e;
    }
    for (uint32_t q = lane; q < len; q += lanes) bases[base_at + q] = char_of(i + q);
}

// Rule L4 without the position and the strand, which is the order of the alleles of one position (L5): front 0 before 1,
// then the shorter, then the bases as bytes.  < 0, 0, > 0 as a comes before, equals, comes behind b.
DCN_PILE_FN int dcn_ins_allele_cmp(const dcn_ins_event &a, const dcn_ins_event &b, const uint8_t *bases) {
    const uint32_t fa = a.flags & DCN_INS_FRONT, fb = b.flags & DCN_INS_FRONT;
    if (fa != fb) return fa < fb ? -1 : 1;
    if (a.len != b.len) return a.len < b.len ? -1 : 1;
    const uint8_t *pa = bases + a.bases_offset, *pb = bases + b.bases_offset;
    for (uint32_t q = 0; q < a.len; ++q)
        if (pa[q] != pb[q]) return pa[q] < pb[q] ? -1 : 1;
    return 0;
}

// Rule L5: allele a with count_a beats allele b with count_b
DCN_PILE_FN bool dcn_ins_beats(uint32_t count_a, const dcn_ins_event &a, uint32_t count_b, const dcn_ins_event &b, const uint8_t *bases) {
    if (count_a != count_b) return count_a > count_b;
    return dcn_ins_allele_cmp(a, b, bases) < 0;
}

// Rule L5 over the `count` events of one position, slots[0 .. count) naming them among `events`, as lane `lane` of `lanes`
// sees it: the lane's events are slots[lane], slots[lane + lanes], ...; each is counted against all of the position's
// (quadratic in the events of one position).  -> the lane's best as an index into slots, or UINT32_MAX when it has no
// event; *best_count its count.  The caller reduces the lanes with dcn_ins_beats.
DCN_PILE_FN uint32_t dcn_ins_lane_winner(const uint64_t *slots, uint32_t count, uint32_t lane, uint32_t lanes, const dcn_ins_event *events,
                                         const uint8_t *bases, uint32_t *best_count) {
    uint32_t best = UINT32_MAX, best_c = 0;
    for (uint32_t k = lane; k < count; k += lanes) {
        const dcn_ins_event mine = events[slots[k]];
        uint32_t c = 0;
        for (uint32_t t = 0; t < count; ++t) c += dcn_ins_allele_cmp(mine, events[slots[t]], bases) == 0 ? 1u : 0u;
        if (best == UINT32_MAX || dcn_ins_beats(c, mine, best_c, events[slots[best]], bases)) best = k, best_c = c;
    }
    *best_count = best_c;
    return best;
}
