// dcn_verify_words.h -- the word helpers of the verify kernel (verify.hip): 16 bases of a 2-bit stream and of its
// invalid-base bits at any base offset, the reverse complement of such a word, and the length of the run of EQUAL bases of
// two streams.  Plain integer arithmetic: compiles for the host as well (tests/cpp/verify_helpers_test.cpp), as dcn_pack.h does.
// Layout (pack.hip): base b is bits [2(b%16), 2(b%16)+2) of packed[b/16] and bit b%32 of invmask[b/32]; A=0 C=1 T=2 G=3, so
// the complement of a code is the code ^ 2.  Every fetch reads the word that holds base b and the one behind it: a stream
// is readable one word past the last base a caller asks about, and -- for the reverse strand -- one word in front of the first.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DCN_VFY_FN __host__ __device__ inline
#else
#define DCN_VFY_FN inline
#endif

DCN_VFY_FN uint32_t dcn_vfy_brev32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(x);
#else
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
    return (x >> 16) | (x << 16);
#endif
}

// trailing zeros of x != 0
DCN_VFY_FN uint32_t dcn_vfy_ctz32(uint32_t x) { return (uint32_t)__builtin_ctz(x); }

// 16 bases from base b on: base b + u in bits [2u, 2u + 2)
DCN_VFY_FN uint32_t dcn_vfy_fetch16(const uint32_t *packed, int64_t b) {
    const int64_t w = b >> 4; // (floor: b may lie in the pad in front of the stream)
    const uint32_t sh = (uint32_t)(b & 15) * 2u;
    const uint64_t two = (uint64_t)packed[w] | ((uint64_t)packed[w + 1] << 32);
    return (uint32_t)(two >> sh);
}

// their 16 invalid-base bits: base b + u in bit u
DCN_VFY_FN uint32_t dcn_vfy_mask16(const uint32_t *invmask, int64_t b) {
    const int64_t w = b >> 5;
    const uint32_t sh = (uint32_t)(b & 31);
    const uint64_t two = (uint64_t)invmask[w] | ((uint64_t)invmask[w + 1] << 32);
    return (uint32_t)(two >> sh) & 0xFFFFu;
}

// the reverse complement of 16 bases: group u of the result is the complement of group 15 - u.  A bit reverse turns the
// groups round and swaps the two bits of each; the swap within pairs undoes that; ^ 2 per group complements.
DCN_VFY_FN uint32_t dcn_vfy_revcomp16(uint32_t x) {
    const uint32_t y = dcn_vfy_brev32(x);
    return (((y >> 1) & 0x55555555u) | ((y & 0x55555555u) << 1)) ^ 0xAAAAAAAAu;
}

// 16 invalid-base bits turned round (the complement of an invalid base is invalid)
DCN_VFY_FN uint32_t dcn_vfy_rev16(uint32_t m) { return dcn_vfy_brev32(m) >> 16; }

// how many of the 16 bases of xs and xt are EQUAL from base 0 on, before the first that differs or is invalid (inv: the
// OR of both sides' invalid bits): 0 .. 16
DCN_VFY_FN uint32_t dcn_vfy_run16(uint32_t xs, uint32_t xt, uint32_t inv) {
    const uint32_t d = xs ^ xt;
    const uint32_t differ = (d | (d >> 1)) & 0x55555555u; // bit 2u: group u differs
    const uint32_t by_code = differ ? dcn_vfy_ctz32(differ) >> 1 : 16u;
    const uint32_t by_mask = dcn_vfy_ctz32(inv | 0x10000u);
    return by_code < by_mask ? by_code : by_mask;
}

// One side of a comparison: a stream and where base 0 of the sequence lies in it.  Forward: sequence base i is stream base
// origin + i.  Reverse: sequence base i is the complement of stream base origin - 1 - i (origin = the end of the interval).
struct dcn_vfy_side {
    const uint32_t *packed, *invmask;
    int64_t origin;
    uint32_t reverse;
};

// 16 bases of a side from sequence base i on, and their invalid bits
DCN_VFY_FN void dcn_vfy_side16(const dcn_vfy_side &s, int64_t i, uint32_t *x, uint32_t *inv) {
    if (s.reverse) {
        const int64_t b = s.origin - i - 16;
        *x = dcn_vfy_revcomp16(dcn_vfy_fetch16(s.packed, b));
        *inv = dcn_vfy_rev16(dcn_vfy_mask16(s.invmask, b));
    } else {
        *x = dcn_vfy_fetch16(s.packed, s.origin + i);
        *inv = dcn_vfy_mask16(s.invmask, s.origin + i);
    }
}

// the length of the run of EQUAL bases S[i + t] == T[j + t], t = 0, 1, ..., at most `limit`
DCN_VFY_FN uint64_t dcn_vfy_match_run(const dcn_vfy_side &S, int64_t i, const dcn_vfy_side &T, int64_t j, uint64_t limit) {
    uint64_t t = 0;
    while (t < limit) {
        uint32_t xs, is, xt, it;
        dcn_vfy_side16(S, i + (int64_t)t, &xs, &is);
        dcn_vfy_side16(T, j + (int64_t)t, &xt, &it);
        const uint32_t r = dcn_vfy_run16(xs, xt, is | it);
        t += r;
        if (r < 16u) break;
    }
    return t < limit ? t : limit;
}
