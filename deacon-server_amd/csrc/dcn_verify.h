// dcn_verify.h -- kept reference bases of an anchor map and the verify kernel's arguments (internal; verify.hip,
// verify_api.hip, and place_api.hip for the append of dcn_anchor_map_add).
#pragma once

#include "dcn_internal.h"

#include <vector>

// The bases of every record added to a map after dcn_anchor_map_keep_bases, as the pack kernel leaves them: one 2-bit
// stream and one invalid-base bit per base (0.375 B per base).  Every add call starts at a 32-base-aligned offset of the
// store, so its append is two device-to-device copies of whole words; record R starts at rec_start[R] = that offset +
// offsets[r] of its call, anywhere within a word.  cap and used are bases, multiples of 32; both arrays end in
// DCN_STORE_PAD_WORDS readable words (dcn_verify_words.h reads one word past a base).
constexpr uint64_t DCN_STORE_PAD_WORDS = 8;
constexpr uint64_t DCN_STORE_INITIAL_BASES = 1ull << 24;
struct dcn_base_store {
    uint32_t *d_packed = nullptr, *d_invmask = nullptr;
    uint64_t cap = 0, used = 0;
    std::vector<uint64_t> rec_start; // per record: its first base in the store
    std::vector<uint32_t> rec_len;   // ... and its length (the host's copy: what rows are checked against)
};
void dcn_base_store_free(dcn_base_store *s);
// Appends the batch that the front end has just packed into `packed` / `invmask` (views behind DCN_FRONT_PAD) on `stream`:
// grows the store, enqueues the two copies and returns where the batch begins.  Nothing of the store's host state
// changes: the caller commits with dcn_base_store_commit once the run has succeeded.
int dcn_base_store_append(dcn_base_store *s, const uint32_t *packed, const uint32_t *invmask, uint64_t n_bases, hipStream_t stream,
                          uint64_t *batch_start);
void dcn_base_store_commit(dcn_base_store *s, uint64_t batch_start, const uint64_t *offsets, uint32_t n_records);

// One row as the kernel takes it: the host has checked the row against the read and the record and resolved both
// intervals to stream positions (the kernel trusts nothing the host has not checked).
struct dcn_verify_item {
    int64_t s_origin; // the read interval in the batch stream: its first base, or its end when reverse
    int64_t t_origin; // the first base of the record interval in the store
    uint32_t m, n;    // |S|, |T|
    uint32_t E;       // rule 4's threshold
    uint32_t flags;   // bit 0: reverse; bit 1: unplaced (nothing else is read)
};
static_assert(sizeof(dcn_verify_item) == 32, "verify item");

struct dcn_verify_args {
    const dcn_verify_item *items;
    uint64_t n_rows;
    const uint32_t *s_packed, *s_invmask; // the batch: views behind DCN_FRONT_PAD
    const uint32_t *t_packed, *t_invmask; // the store
    uint32_t lds_stride;                  // words of one wavefront array: >= 2 * (the largest E of the call) + 1
    uint32_t *out;
};
int dcn_launch_verify(const dcn_verify_args &args, hipStream_t stream);
