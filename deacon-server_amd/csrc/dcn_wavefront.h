// dcn_wavefront.h -- the wavefront edit distance that verify.hip, align.hip and extend.hip run, written once: the word
// helpers (16 bases of a 2-bit stream and of its invalid-base bits at any base offset, the reverse complement of such a
// word, the run of EQUAL bases of two streams) and one diagonal of one score.  Plain integer arithmetic: compiles for the
// host as well (tests/cpp/wavefront_test.cpp, verify_helpers_test.cpp, align_trace_test.cpp, extend_flank_test.cpp), as
// dcn_pack.h does.
// Layout (pack.hip): base b is bits [2(b%16), 2(b%16)+2) of packed[b/16] and bit b%32 of invmask[b/32]; A=0 C=1 T=2 G=3, so
// the complement of a code is the code ^ 2.  Every fetch reads the word that holds base b and the one behind it: a stream
// is readable one word past the last base a caller asks about, and -- for a side that is read backwards -- one word in
// front of the first, unless the words are loaded by dcn_wf_guarded.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DCN_WF_FN __host__ __device__ inline
#else
#define DCN_WF_FN inline
#endif

DCN_WF_FN int64_t dcn_wf_min(int64_t a, int64_t b) { return a < b ? a : b; }
DCN_WF_FN int64_t dcn_wf_max(int64_t a, int64_t b) { return a > b ? a : b; }

DCN_WF_FN uint32_t dcn_wf_brev32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bitreverse32(x); // (what __brev is, without the need for the HIP headers in front of this one)
#else
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
    return (x >> 16) | (x << 16);
#endif
}

// trailing zeros of x != 0
DCN_WF_FN uint32_t dcn_wf_ctz32(uint32_t x) { return (uint32_t)__builtin_ctz(x); }

// How a word of a stream is loaded, chosen at compile time.
//   dcn_wf_plain    the stream has readable pad words in front (the batch behind DCN_FRONT_PAD; the store, of which verify
//                   and align read no base in front of a record interval's first): the word as it stands.
//   dcn_wf_guarded  a stream with no word in front of word 0 (the base store, read backwards by extend's left flanks: the
//                   16 bases in front of a base begin up to 15 bases in front of base 0 when the base is one of the first
//                   16).  Words in front of word 0 read as 0: the bases they would hold lie in front of the sequence's
//                   last base, where no match run looks (every run is limited to the sequence).
struct dcn_wf_plain {
    static DCN_WF_FN uint32_t word(const uint32_t *words, int64_t w) { return words[w]; }
};
struct dcn_wf_guarded {
    static DCN_WF_FN uint32_t word(const uint32_t *words, int64_t w) { return w < 0 ? 0u : words[w]; }
};

// 16 bases from base b on: base b + u in bits [2u, 2u + 2)
template <typename Load>
DCN_WF_FN uint32_t dcn_wf_fetch16(const uint32_t *packed, int64_t b) {
    const int64_t w = b >> 4; // (floor: b may lie in front of the stream)
    const uint32_t sh = (uint32_t)(b & 15) * 2u;
    const uint64_t two = (uint64_t)Load::word(packed, w) | ((uint64_t)Load::word(packed, w + 1) << 32);
    return (uint32_t)(two >> sh);
}

// their 16 invalid-base bits: base b + u in bit u
template <typename Load>
DCN_WF_FN uint32_t dcn_wf_mask16(const uint32_t *invmask, int64_t b) {
    const int64_t w = b >> 5;
    const uint32_t sh = (uint32_t)(b & 31);
    const uint64_t two = (uint64_t)Load::word(invmask, w) | ((uint64_t)Load::word(invmask, w + 1) << 32);
    return (uint32_t)(two >> sh) & 0xFFFFu;
}

// the reverse complement of 16 bases: group u of the result is the complement of group 15 - u.  A bit reverse turns the
// groups round and swaps the two bits of each; the swap within pairs undoes that; ^ 2 per group complements.
DCN_WF_FN uint32_t dcn_wf_revcomp16(uint32_t x) {
    const uint32_t y = dcn_wf_brev32(x);
    return (((y >> 1) & 0x55555555u) | ((y & 0x55555555u) << 1)) ^ 0xAAAAAAAAu;
}

// 16 invalid-base bits turned round (the complement of an invalid base is invalid)
DCN_WF_FN uint32_t dcn_wf_rev16(uint32_t m) { return dcn_wf_brev32(m) >> 16; }

// how many of the 16 bases of xs and xt are EQUAL from base 0 on, before the first that differs or is invalid (inv: the
// OR of both sides' invalid bits): 0 .. 16
DCN_WF_FN uint32_t dcn_wf_run16(uint32_t xs, uint32_t xt, uint32_t inv) {
    const uint32_t d = xs ^ xt;
    const uint32_t differ = (d | (d >> 1)) & 0x55555555u; // bit 2u: group u differs
    const uint32_t by_code = differ ? dcn_wf_ctz32(differ) >> 1 : 16u;
    const uint32_t by_mask = dcn_wf_ctz32(inv | 0x10000u);
    return by_code < by_mask ? by_code : by_mask;
}

// One side of a comparison: a stream and where base 0 of the sequence lies in it.  Forward: sequence base i is stream base
// origin + i.  Reverse: sequence base i is the complement of stream base origin - 1 - i (origin = the end of the interval).
struct dcn_wf_side {
    const uint32_t *packed, *invmask;
    int64_t origin;
    uint32_t reverse;
};

// 16 bases of a side from sequence base i on, and their invalid bits
template <typename Load>
DCN_WF_FN void dcn_wf_side16(const dcn_wf_side &s, int64_t i, uint32_t *x, uint32_t *inv) {
    if (s.reverse) {
        const int64_t b = s.origin - i - 16;
        *x = dcn_wf_revcomp16(dcn_wf_fetch16<Load>(s.packed, b));
        *inv = dcn_wf_rev16(dcn_wf_mask16<Load>(s.invmask, b));
    } else {
        *x = dcn_wf_fetch16<Load>(s.packed, s.origin + i);
        *inv = dcn_wf_mask16<Load>(s.invmask, s.origin + i);
    }
}

// the length of the run of EQUAL bases S[i + t] == T[j + t], t = 0, 1, ..., at most `limit`.  The caller's limit is what
// is left of both sequences: behind them lies another read of the batch or another record of the store, whose bases may
// well continue the match.
template <typename Load>
DCN_WF_FN uint64_t dcn_wf_match_run(const dcn_wf_side &S, int64_t i, const dcn_wf_side &T, int64_t j, uint64_t limit) {
    uint64_t t = 0;
    while (t < limit) {
        uint32_t xs, is, xt, it;
        dcn_wf_side16<Load>(S, i + (int64_t)t, &xs, &is);
        dcn_wf_side16<Load>(T, j + (int64_t)t, &xt, &it);
        const uint32_t r = dcn_wf_run16(xs, xt, is | it);
        t += r;
        if (r < 16u) break;
    }
    return t < limit ? t : limit;
}

// A side read backwards from its sequence base a: base k of the result is the complement of the side's base a - k, and
// its invalid bit.  Both sides of a comparison turned this way compare as they did (the complement of a code is the
// code ^ 2 on both).  A forward side becomes a reverse one and the other way round: no new fetch is needed.
DCN_WF_FN dcn_wf_side dcn_wf_side_back(const dcn_wf_side &s, int64_t a) {
    dcn_wf_side b = s;
    b.reverse = s.reverse ? 0u : 1u;
    b.origin = s.reverse ? s.origin - 1 - a : s.origin + a + 1;
    return b;
}

// the backward form of dcn_wf_match_run: the length of the run S[i - t] == T[j - t], t = 0, 1, ..., at most `limit`.  The
// 16 bases of the last group may begin up to 15 bases in front of base i - limit + 1: Load says what is readable there.
template <typename Load>
DCN_WF_FN uint64_t dcn_wf_match_run_back(const dcn_wf_side &S, int64_t i, const dcn_wf_side &T, int64_t j, uint64_t limit) {
    return dcn_wf_match_run<Load>(dcn_wf_side_back(S, i), 0, dcn_wf_side_back(T, j), 0, limit);
}

// One diagonal of one score.  F_s[k] is the furthest base i of S (m bases) that a path of cost <= s reaches on diagonal
// k = j - i (j: the base of T, n bases), for max(-s, -m) <= k <= min(s, n).  It comes from F_{s-1}[k] + 1 (substitution),
// F_{s-1}[k - 1] (a base of T alone) and F_{s-1}[k + 1] + 1 (a base of S alone), cut to the rectangle, then runs on while
// the bases are EQUAL.  `prev` holds F_{s-1}, diagonal k at prev[k + center]; it is not read at s = 0.
//   Along a diagonal the distance never falls, so every point in front of a reached one is reached at no more cost: the
//   cut to min(m, n - k) is exact, and within max(-s, -m) <= k <= min(s, n) some source is always in range (k itself for
//   |k| < s, k - 1 for k = s, k + 1 for k = -s), which leaves i >= max(0, -k): no position is ever negative, and the
//   max(i, 0) of the result changes nothing.
// The edit distance is the first s with F_s[n - m] == m, and a path of cost <= E never leaves the diagonals [-E, +E].
template <typename Load>
DCN_WF_FN int64_t dcn_wf_diagonal(const uint32_t *prev, int64_t center, int64_t s, int64_t k, int64_t m, int64_t n, const dcn_wf_side &S,
                                  const dcn_wf_side &T) {
    int64_t i = 0;
    if (s > 0) {
        const int64_t plo = dcn_wf_max(1 - s, -m), phi = dcn_wf_min(s - 1, n); // the diagonals of score s - 1
        i = -1;
        if (k >= plo && k <= phi) i = (int64_t)prev[k + center] + 1;
        if (k - 1 >= plo && k - 1 <= phi) i = dcn_wf_max(i, (int64_t)prev[k - 1 + center]);
        // (k + 1 within [plo, phi], in the form that keeps plo - 1 in a scalar register: spelled with k + 1 it cost
        // align_kernel a vector add per diagonal and 1 % on long reads, profiles/wavefront_refactor_ab.txt)
        if (k >= plo - 1 && k < phi) i = dcn_wf_max(i, (int64_t)prev[k + 1 + center] + 1);
        i = dcn_wf_min(i, dcn_wf_min(m, n - k));
    }
    const int64_t j = i + k;
    if (i >= 0 && j >= 0) { // (always: see above; a position that were not would read nothing)
        const int64_t room = dcn_wf_min(m - i, n - j);
        if (room > 0) i += (int64_t)dcn_wf_match_run<Load>(S, i, T, j, (uint64_t)room);
    }
    return dcn_wf_max(i, 0);
}
