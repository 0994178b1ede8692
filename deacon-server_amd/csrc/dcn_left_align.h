// dcn_left_align.h -- the left alignment of one row's runs (THE DEFINITION OF A LEFT-ALIGNED PLACEMENT, include/deacon_hip.h):
// the procedure of rules N1 - N5 over a run list, given the two sides of the row, the backward self-match that says how many
// steps a gap may take, and the run writer that merges equal neighbours (kernel in left_align.hip).  Plain integer
// arithmetic over two pointers: compiles for the host as well (tests/cpp/left_align_test.cpp), as dcn_align.h does.
//   The runs are fed in order.  What is final so far is a stack, `out`: its top run is kept in registers, the rest lies
// in memory from `lo` upwards.  A gap (a run of I or of D) looks at the top of the stack:
//     nothing            the gap is the row's first run and stays (N4)
//     a gap of its kind  the two merge, and the gap goes on with the sum of their lengths (N4)
//     the other kind     the gap stops (N4)
//     an '=' or X run    of L columns.  The gap may pass t of them, t = the backward self-match of its sequence at the
//                        distance of its length (N2: T[j - 1 - u] EQUAL T[j + len - 1 - u], u = 0, 1, ...; N3 likewise in S),
//                        at most L, and at most L - 1 when the run is the bottom of the stack (its first column is the
//                        row's first, which no gap passes).  t columns leave the run and wait on a second stack, `behind`;
//                        the gap goes on while a whole run was passed.
// Then the gap is pushed, and behind it the waiting runs, last passed first: they stand in their old order, and each keeps
// its op.  Every push merges with an equal top, so the list is A4's at every moment.
//   Room.  Both stacks share the row's 2 d + 1 words, `out` from the bottom and `behind` from the top.  The runs of `out`
// are the merged runs of columns that cost d_o, at most 2 d_o + 1; the waiting runs are '=' and X runs that were apart in a
// merged list, and what stood between two neighbours that are both '=' is a gap that merged into the current one, so with
// d_b the cost of their X columns and of those gaps they are at most 2 d_b + 1; the gap itself costs at least 1 more:
// d_o + d_b + 1 <= d, and both stacks together hold at most 2 d words.  The stores check it all the same: a row that would
// pass its words is left as it was (`ok`).
#pragma once

#include <stdint.h>

#include "dcn_align.h"
#include "dcn_wavefront.h"

// how a row's words are read and written, and who compares bases: the host's form (one thread).  left_align.hip has the
// wave's: lane 0 reads and writes, all lanes compare.
struct dcn_la_serial {
    static DCN_WF_FN uint32_t load(const uint32_t *p) { return *p; }
    static DCN_WF_FN void store(uint32_t *p, uint32_t v) { *p = v; }
    // rules N2 / N3: the steps that a gap of `len` bases which begins at base g of `side` may take, at most `limit`
    static DCN_WF_FN uint64_t steps(const dcn_wf_side &side, int64_t g, int64_t len, uint64_t limit) {
        return dcn_wf_match_run_back<dcn_wf_guarded>(side, g - 1, side, g + len - 1, limit);
    }
};

// what the rows of a call add up to (dcn_left_align_info's four totals)
struct dcn_la_totals {
    unsigned long long rows_changed, gaps_shifted, columns_passed, gaps_merged;
};

struct dcn_la_row {
    uint32_t *lo;      // out: lo[0 .. n_out) and the top in (op, len)
    uint32_t bound;    // the row's words; behind: lo[bound - 1], lo[bound - 2], ...
    uint32_t n_out, n_behind;
    uint32_t op, len;  // the top of out (len = 0: out is empty)
    int64_t i, j;      // the bases of S and of T in front of the next run that is fed
    dcn_wf_side S, T;
    unsigned long long shifted, passed, merged;
    bool ok;
};

DCN_WF_FN dcn_la_row dcn_la_begin(uint32_t *lo, uint32_t bound, const dcn_wf_side &S, const dcn_wf_side &T) {
    dcn_la_row r;
    r.lo = lo;
    r.bound = bound;
    r.n_out = r.n_behind = 0;
    r.op = DCN_ALN_EQ;
    r.len = 0;
    r.i = r.j = 0;
    r.S = S;
    r.T = T;
    r.shifted = r.passed = r.merged = 0;
    r.ok = true;
    return r;
}

// the run writer: a run on top of out, merged with an equal top
template <typename W>
DCN_WF_FN void dcn_la_push(dcn_la_row &r, uint32_t op, uint32_t len) {
    if (len == 0) return;
    if (r.len != 0 && r.op == op) {
        r.len += len;
        return;
    }
    if (r.len != 0) {
        if (r.n_out + r.n_behind >= r.bound) { // (never: see Room above)
            r.ok = false;
            return;
        }
        W::store(r.lo + r.n_out++, (r.len << 4) | r.op);
    }
    r.op = op;
    r.len = len;
}

// the top of out goes: the run below it becomes the top
template <typename W>
DCN_WF_FN void dcn_la_pop(dcn_la_row &r) {
    r.len = 0;
    if (r.n_out == 0) return;
    const uint32_t v = W::load(r.lo + --r.n_out);
    r.op = v & 15u;
    r.len = v >> 4;
}

// what a gap does on its way to the front (the loop of the file's head).  -> its steps
template <typename W>
DCN_WF_FN unsigned long long dcn_la_gap(dcn_la_row &r, uint32_t op, uint32_t len, const dcn_wf_side &side, int64_t g) {
    uint32_t glen = len;
    unsigned long long steps = 0;
    while (r.len != 0 && r.ok) {
        if (r.op == op) { // N4: directly behind a gap of its kind
            glen += r.len;
            g -= r.len;
            r.merged += 1;
            dcn_la_pop<W>(r);
            continue;
        }
        if (r.op == DCN_ALN_I || r.op == DCN_ALN_D) break; // N4: the other kind
        const uint32_t L = r.len, limit = r.n_out == 0 ? L - 1u : L; // (the bottom run begins with the row's first column)
        const uint32_t t = limit ? (uint32_t)W::steps(side, g, glen, limit) : 0u;
        if (t == 0) break;
        steps += t;
        g -= t;
        if (r.n_out + r.n_behind + (t < L ? 1u : 0u) >= r.bound) { // (never)
            r.ok = false;
            break;
        }
        W::store(r.lo + (r.bound - ++r.n_behind), (t << 4) | r.op);
        if (t < L) {
            r.len = L - t;
            break;
        }
        dcn_la_pop<W>(r);
    }
    dcn_la_push<W>(r, op, glen);
    while (r.n_behind != 0 && r.ok) { // the last passed stands first
        const uint32_t v = W::load(r.lo + (r.bound - r.n_behind--));
        dcn_la_push<W>(r, v & 15u, v >> 4);
    }
    return steps;
}

// one run of the row, in order
template <typename W>
DCN_WF_FN void dcn_la_feed(dcn_la_row &r, uint32_t run) {
    const uint32_t op = run & 15u, len = run >> 4;
    const bool ins = op == DCN_ALN_I, del = op == DCN_ALN_D;
    unsigned long long steps = 0;
    if (ins || del) {
        // (values first, then the choice, and one place that adds to the row: a choice between two of its members would
        // put the row in memory on the device)
        const dcn_wf_side rS = r.S, rT = r.T;
        const int64_t ri = r.i, rj = r.j;
        const dcn_wf_side side = {del ? rT.packed : rS.packed, del ? rT.invmask : rS.invmask, del ? rT.origin : rS.origin,
                                  del ? rT.reverse : rS.reverse};
        steps = dcn_la_gap<W>(r, op, len, side, del ? rj : ri);
    } else {
        dcn_la_push<W>(r, op, len);
    }
    r.i += del ? 0u : len;
    r.j += ins ? 0u : len;
    r.shifted += steps != 0 ? 1u : 0u;
    r.passed += steps;
}

// behind the last run: the top goes to memory.  -> the number of runs at lo[0 ..), or 0 for a row that is to stay as it was
// (no gap took a step, or -- never -- the row's words would not hold it)
template <typename W>
DCN_WF_FN uint32_t dcn_la_end(dcn_la_row &r) {
    if (!r.ok || r.passed == 0) return 0;
    if (r.len != 0) {
        if (r.n_out >= r.bound) return 0; // (never)
        W::store(r.lo + r.n_out++, (r.len << 4) | r.op);
        r.len = 0;
    }
    return r.n_out;
}
