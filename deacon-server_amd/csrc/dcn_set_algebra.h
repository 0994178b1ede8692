// dcn_set_algebra.h -- sweeps over a labelled set's member masks and the intersection of tables (set_algebra.hip; not
// part of the public ABI).  The entry points are in set_algebra_api.hip.
#pragma once

#include "dcn_classify.h"

// dcn_index_set_select's predicate on a member mask L, with the defaults resolved: 1 <= min_members <= max_members <= 32
struct dcn_select_pred {
    uint32_t all_of, any_of, none_of, min_members, max_members;
};

__host__ __device__ inline bool dcn_select_pass(uint32_t L, const dcn_select_pred &p) {
    const uint32_t c = (uint32_t)__builtin_popcount(L);
    return (L & p.all_of) == p.all_of && (p.any_of == 0 || (L & p.any_of) != 0) && (L & p.none_of) == 0 &&
           c >= p.min_members && c <= p.max_members; // (an empty slot has c == 0 < min_members)
}

// What the overlap sweep adds into (u64 each, zeroed by the caller):
//   [i * 32 + j], i <= j   slots whose mask has SEVERAL bits, among them i and j (the upper triangle, diagonal included)
//   [SINGLE + j]           slots whose mask is exactly 1 << j
//   [COUNT + c - 1]        slots whose mask has c >= 2 bits
constexpr uint32_t DCN_OVL_SINGLE = DCN_MAX_SET_MEMBERS * DCN_MAX_SET_MEMBERS;
constexpr uint32_t DCN_OVL_COUNT = DCN_OVL_SINGLE + DCN_MAX_SET_MEMBERS;
constexpr uint32_t DCN_OVL_WORDS = DCN_OVL_COUNT + DCN_MAX_SET_MEMBERS;

// All four run on the null stream of the current device (the set's) and return after the launch; key 0, which has no
// slot, is left to the caller.
int dcn_set_overlap_sweep(const dcn_index *set, unsigned long long *d_tally);
// dst == null: *d_n += slots whose mask passes; else their keys are inserted into dst's table and *d_n += fresh inserts
int dcn_set_select_sweep(const dcn_index *set, const dcn_select_pred &pred, dcn_index *dst, unsigned long long *d_n);
// bit s of d_bits (one u64 per 64 slots of src, every word written) = slot s holds a key that every one of d_others has;
// *d_n += those slots
int dcn_intersect_mark(const dcn_index *src, const dcn_table_view *d_others, uint32_t n_others, unsigned long long *d_bits,
                       unsigned long long *d_n);
// the keys of src's marked slots into dst's table; *d_n += fresh inserts
int dcn_intersect_build(const dcn_index *src, const unsigned long long *d_bits, dcn_index *dst, unsigned long long *d_n);
