// dcn_duplicates.h -- what the host and the device share of duplicate marking (THE DEFINITION OF A DUPLICATE, rules D1 - D7
// of include/deacon_hip.h): the end of a read from its first placed row (D3), the key of a unit from its ends (D4), the
// exact comparison of two keys and the hash that only chooses where a probe begins (kernels in duplicates.hip, the C ABI
// in duplicates_api.hip).  Plain integer arithmetic: compiles for the host alone (tests/cpp/duplicate_key_test.cpp), as
// dcn_genotype.h does.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DCN_DUP_FN __host__ __device__ inline
#else
#define DCN_DUP_FN inline
#endif

constexpr uint64_t DCN_DUP_EMPTY = ~0ull;      // a slot of the table that holds no ordinal
constexpr uint64_t DCN_DUP_NO_FIRST = ~0ull;   // rule D5: the `first` of a unit without a key
constexpr uint32_t DCN_DUP_NO_RECORD = ~0u;    // an item of a read without a placed row

// One read as the kernel takes it: the fields of its first row with record != UINT32_MAX, which the host has checked and
// picked while it walked the rows, and the read's length.  record = DCN_DUP_NO_RECORD: the read has no end.
struct dcn_dup_item {
    uint64_t ref_start, ref_end;
    uint32_t record, reverse;
    uint32_t read_start, read_end;
    uint32_t read_len, reserved;
};
static_assert(sizeof(dcn_dup_item) == 40, "duplicate item");

// rule D3's end
struct dcn_dup_end {
    uint32_t record, reverse;
    int64_t pos5, pos3; // pos3 is 0 without both_ends
};

// Rule D4's key, 48 bytes of the key log per unit.  Every field that a key does not have is 0, so that two keys are equal
// exactly when their six words are.
//   w[0]  bit 0 paired, bit 1 both_ends, bits 2-3 the number of ends (0: the unit has no key), bit 4 / 5 the strand of
//         end 0 / 1
//   w[1]  the record of end 0, and of end 1 in the high half
//   w[2], w[3]  pos5 and pos3 of end 0;  w[4], w[5]  of end 1
struct dcn_dup_key {
    uint64_t w[6];
};
static_assert(sizeof(dcn_dup_key) == 48, "duplicate key");

// D3.  The differences wrap in 64 bits and are read as signed: a clipped read at the start of a record has a negative pos5.
DCN_DUP_FN dcn_dup_end dcn_dup_end_of(const dcn_dup_item &it, uint32_t both_ends) {
    dcn_dup_end e;
    e.record = it.record;
    e.reverse = it.reverse;
    const uint64_t tail = (uint64_t)it.read_len - it.read_end; // L - read_end: the bases clipped behind the row's interval
    if (!it.reverse) {
        e.pos5 = (int64_t)(it.ref_start - it.read_start);
        e.pos3 = both_ends ? (int64_t)(it.ref_end + tail) : 0;
    } else {
        e.pos5 = (int64_t)(it.ref_end + it.read_start);
        e.pos3 = both_ends ? (int64_t)(it.ref_start - tail) : 0;
    }
    return e;
}

// D4's order of two ends: ascending as tuples (record, pos5, reverse, pos3)
DCN_DUP_FN bool dcn_dup_end_less(const dcn_dup_end &a, const dcn_dup_end &b) {
    if (a.record != b.record) return a.record < b.record;
    if (a.pos5 != b.pos5) return a.pos5 < b.pos5;
    if (a.reverse != b.reverse) return a.reverse < b.reverse;
    return a.pos3 < b.pos3;
}

// D4.  n_ends is 0, 1 or 2; two ends are sorted here.  No end: the key with w[0]'s count 0, which dcn_dup_has_key refuses.
DCN_DUP_FN dcn_dup_key dcn_dup_key_of(uint32_t paired, uint32_t both_ends, dcn_dup_end e0, dcn_dup_end e1, uint32_t n_ends) {
    dcn_dup_key k;
    k.w[0] = k.w[1] = k.w[2] = k.w[3] = k.w[4] = k.w[5] = 0;
    if (n_ends == 0) return k;
    if (n_ends == 2 && dcn_dup_end_less(e1, e0)) {
        const dcn_dup_end t = e0;
        e0 = e1;
        e1 = t;
    }
    k.w[0] = (uint64_t)(paired ? 1u : 0u) | (uint64_t)(both_ends ? 2u : 0u) | (uint64_t)n_ends << 2 | (uint64_t)(e0.reverse & 1u) << 4;
    k.w[1] = e0.record;
    k.w[2] = (uint64_t)e0.pos5;
    k.w[3] = (uint64_t)e0.pos3;
    if (n_ends == 2) {
        k.w[0] |= (uint64_t)(e1.reverse & 1u) << 5;
        k.w[1] |= (uint64_t)e1.record << 32;
        k.w[4] = (uint64_t)e1.pos5;
        k.w[5] = (uint64_t)e1.pos3;
    }
    return k;
}

// the key of unit u of a call over `items` (D2: read u, or reads 2 u and 2 u + 1)
DCN_DUP_FN dcn_dup_key dcn_dup_unit_key(const dcn_dup_item *items, uint64_t u, uint32_t paired, uint32_t both_ends) {
    dcn_dup_end e[2];
    e[0].record = e[1].record = 0, e[0].reverse = e[1].reverse = 0, e[0].pos5 = e[1].pos5 = 0, e[0].pos3 = e[1].pos3 = 0;
    uint32_t n = 0;
    const uint64_t r0 = paired ? 2 * u : u, r1 = paired ? 2 * u + 2 : u + 1;
    for (uint64_t r = r0; r < r1; ++r)
        if (items[r].record != DCN_DUP_NO_RECORD) {
            const dcn_dup_end x = dcn_dup_end_of(items[r], both_ends);
            if (n == 0) e[0] = x;
            else e[1] = x;
            ++n;
        }
    return dcn_dup_key_of(paired, both_ends, e[0], e[1], n);
}

DCN_DUP_FN bool dcn_dup_has_key(const dcn_dup_key &k) { return ((k.w[0] >> 2) & 3u) != 0; }

// exact: every component
DCN_DUP_FN bool dcn_dup_key_equal(const dcn_dup_key &a, const dcn_dup_key &b) {
    return ((a.w[0] ^ b.w[0]) | (a.w[1] ^ b.w[1]) | (a.w[2] ^ b.w[2]) | (a.w[3] ^ b.w[3]) | (a.w[4] ^ b.w[4]) | (a.w[5] ^ b.w[5])) == 0;
}

// where a probe begins, before the table's mask.  No decision rests on it (D4): equal keys hash alike, and that is all.
DCN_DUP_FN uint64_t dcn_dup_key_hash(const dcn_dup_key &k) {
    uint64_t h = 0x243F6A8885A308D3ull;
    for (int i = 0; i < 6; ++i) {
        h = (h ^ k.w[i]) * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
    }
    h *= 0xBF58476D1CE4E5B9ull;
    return h ^ (h >> 32);
}
