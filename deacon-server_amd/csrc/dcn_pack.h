// dcn_pack.h -- ASCII -> 2-bit codes and invalid-base bits, four bytes at a time: the one copy that pack.hip's kernels and
// the scan kernel's short path (scan.hip) share.  Plain integer arithmetic: compiles for the host as well (tests/cpp).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DCN_PACK_FN __host__ __device__ inline
#else
#define DCN_PACK_FN inline
#endif

// 4 ASCII bytes -> 8 bits of 2-bit codes (byte 0 in bits 0..1): code = (c >> 1) & 3, A=0 C=1 T=2 G=3, for EVERY byte
DCN_PACK_FN uint32_t dcn_pack4(uint32_t x) {
    uint32_t y = (x >> 1) & 0x03030303u;
    return (y * ((1u << 24) | (1u << 18) | (1u << 12) | (1u << 6))) >> 24;
}

// 4 ASCII bytes -> 4 bits, bit j = byte j is not in ACGTacgt.  All four bytes at once: with y = byte | 0x20 and
// T = y.bit2 & ~y.bit1 (set for 't' only among a c g t), a valid byte is 0 1 1 T 0 y2 y1 ~T -- bits 1 and 2 are
// free (they are the 2-bit code), every other bit is fixed by them.  17 instructions instead of 4 x 10: the pack
// kernel was bound by its compares (12 VALU instructions per base), not by HBM.
DCN_PACK_FN uint32_t dcn_invalid4(uint32_t x) {
    const uint32_t y = x | 0x20202020u;
    const uint32_t T = (y >> 2) & ~(y >> 1) & 0x01010101u;
    const uint32_t expect = 0x60606060u | (T << 4) | (T ^ 0x01010101u);
    const uint32_t diff = (y & 0xF9F9F9F9u) ^ expect;                       // non-zero byte <=> invalid byte
    const uint32_t nz = ((diff & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | diff;        // bit 7 of each byte: byte != 0 (no carries across bytes)
    return (((nz >> 7) & 0x01010101u) * 0x01020408u) >> 24;                 // bits 0,8,16,24 -> bits 0..3
}
