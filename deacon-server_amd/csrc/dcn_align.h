// dcn_align.h -- the trace of the align kernel (align.hip) and the walk back over it (THE DEFINITION OF AN ALIGNED
// PLACEMENT, include/deacon_hip.h).  Plain integer arithmetic over a trace pointer: compiles for the host as well
// (tests/cpp/align_trace_test.cpp), as dcn_wavefront.h does.
//   The trace of one row holds every wavefront of its edit distance d, triangular, without padding: F_s[k], the furthest
// base of S that a path of cost <= s reaches on diagonal k = j - i, is trace[s * s + (k + s)], s = 0 .. d, k = -s .. +s:
// (d + 1)^2 words.  A diagonal outside [max(-s, -m), min(s, n)] is neither written nor read.
//   The walk needs no base: with D the table of rule A2, D[i][j] <= s exactly when F_s[j - i] >= i (along a diagonal D
// never falls, and F_s[k] is the last i with D[i][i + k] <= s).  So "D[i - 1][j - 1] == s - 1" at a cell of cost s is
// "F_{s-1}[k] + 1 >= i", and likewise for the two gaps; a cell where none holds is an EQUAL pair on the same diagonal
// (unit costs), and the walk jumps over all of them at once, to the first cell that an edit reaches.
#pragma once

#include <stdint.h>

#include "dcn_wavefront.h"

// BAM's codes of the four ops; a run is len << 4 | op
constexpr uint32_t DCN_ALN_I = 1, DCN_ALN_D = 2, DCN_ALN_EQ = 7, DCN_ALN_X = 8;

// words of a row's trace, and the most runs its alignment can have (between two edits at most one run of '=')
DCN_WF_FN uint64_t dcn_aln_trace_words(uint64_t d) { return (d + 1) * (d + 1); }
DCN_WF_FN uint64_t dcn_aln_ops_bound(uint64_t d) { return 2 * d + 1; }

// where F_s[k] lies in a row's trace
DCN_WF_FN uint64_t dcn_aln_trace_at(int64_t s, int64_t k) { return (uint64_t)(s * s + k + s); }

// One word of a trace.  On the device the wave that walks has written the trace itself, through the cache of its compute
// unit's neighbours as well: the load is an agent-scope one, which no stale line can answer.
DCN_WF_FN int64_t dcn_aln_trace_load(const uint32_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (int64_t)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return (int64_t)*p;
#endif
}

// F_s[k], or -1 for a diagonal that score s does not have
DCN_WF_FN int64_t dcn_aln_trace_get(const uint32_t *trace, int64_t s, int64_t k, int64_t m, int64_t n) {
    if (k < dcn_wf_max(-s, -m) || k > dcn_wf_min(s, n)) return -1;
    return dcn_aln_trace_load(trace + dcn_aln_trace_at(s, k));
}

// The runs of a row, written from `slot_end` downwards as the walk meets them (from the end of both intervals to their
// start), so that they read forwards in memory: equal neighbours merge.
struct dcn_aln_writer {
    uint32_t *at; // the next run goes to at[-1]
    uint32_t op, len;
};
DCN_WF_FN void dcn_aln_flush(dcn_aln_writer &w) {
    if (w.len) *--w.at = (w.len << 4) | w.op;
    w.len = 0;
}
DCN_WF_FN void dcn_aln_emit(dcn_aln_writer &w, uint32_t op, uint32_t len) {
    if (len == 0) return;
    if (op != w.op) dcn_aln_flush(w), w.op = op;
    w.len += len;
}

// The walk of rule A3 from (m, n) at cost d back to (0, 0): d steps.  The runs end at slot_end[-1]; -> their number,
// at most 2 d + 1 (the caller's slot holds that many).  m, n < 2^28.
DCN_WF_FN uint32_t dcn_aln_traceback(const uint32_t *trace, int64_t m, int64_t n, int64_t d, uint32_t *slot_end) {
    dcn_aln_writer w = {slot_end, DCN_ALN_EQ, 0};
    int64_t k = n - m, i = m;
    for (int64_t s = d; s > 0; --s) {
        // the furthest cell of this diagonal that each edit reaches from cost s - 1 (-1: from a diagonal that is not there)
        const int64_t fX = dcn_aln_trace_get(trace, s - 1, k, m, n), fI = dcn_aln_trace_get(trace, s - 1, k + 1, m, n);
        const int64_t vX = fX < 0 ? -1 : fX + 1, vI = fI < 0 ? -1 : fI + 1, vD = dcn_aln_trace_get(trace, s - 1, k - 1, m, n);
        const int64_t e = dcn_wf_max(vX, dcn_wf_max(vI, vD));
        if (i > e) { // EQUAL pairs down to the first cell an edit reaches: no cell between has an edit predecessor
            dcn_aln_emit(w, DCN_ALN_EQ, (uint32_t)(i - e));
            i = e;
        }
        const int64_t j = i + k;
        if (vX >= i && i >= 1 && j >= 1) {
            dcn_aln_emit(w, DCN_ALN_X, 1);
            i -= 1;
        } else if (vI >= i && i >= 1) {
            dcn_aln_emit(w, DCN_ALN_I, 1);
            i -= 1;
            k += 1;
        } else { // vD >= i and j >= 1: one of the three holds at a cell of cost s > 0
            dcn_aln_emit(w, DCN_ALN_D, 1);
            k -= 1;
        }
    }
    dcn_aln_emit(w, DCN_ALN_EQ, (uint32_t)i); // cost 0: diagonal 0, and the rest is EQUAL
    dcn_aln_flush(w);
    return (uint32_t)(slot_end - w.at);
}
