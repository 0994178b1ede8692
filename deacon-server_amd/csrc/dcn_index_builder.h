// dcn_index_builder.h -- an index that is built over several calls and counts how often each key occurs
// (dcn_index_builder_*; the definition is in include/deacon_hip.h; kernels in index_builder.hip, the C ABI in
// index_builder_api.hip; not part of the public ABI).
//
// State: the table of a plain dcn_index, and beside it u32 words of two saturating 16-bit counters (slot s in word s >> 1,
// half s & 1 -- the layout of a set's depth counters, dcn_depth.h) with one more word for key 0, which has no slot.
#pragma once

#include "dcn_depth.h"
#include "dcn_internal.h"

struct dcn_ctx;

constexpr uint32_t DCN_BUILDER_THREADS = 256;
constexpr uint32_t DCN_BUILDER_MAX_SEAM = 320; // >= l - 1 = k + w - 2 for k <= 56, w <= 255

struct dcn_index_builder {
    dcn_index idx; // the table, with k, w, device and the minimizer rule captured at create
    float entropy_threshold = 0.0f;
    uint32_t *d_counts = nullptr; // count_words + 1 words
    uint64_t count_words = 0;
    // the front end, made by the first add: a dump-mode context of chunk_bases bases, one bit per base of a chunk, and the
    // bits of a chunk's last l-1 bases for the chunk after it (seam_words words)
    dcn_ctx *ctx = nullptr;
    uint64_t chunk_bases = 0;
    uint32_t *d_bits = nullptr, *d_seam = nullptr;
    unsigned long long *d_tally = nullptr; // [0] fresh keys, [1] occurrences, [2] key 0 met -- of one sweep
    uint64_t n_occurrences = 0, n_bases = 0;
    // DCN_INDEX_TIMING (read by the first add): host seconds since create, printed by every finish that makes an index
    bool timing = false;
    double front_end_s = 0, staging_s = 0, growth_s = 0;
};

constexpr uint32_t DCN_BUILDER_SEAM_WORDS = DCN_BUILDER_MAX_SEAM / 32;

inline uint64_t dcn_builder_count_words(const dcn_index *idx) { return (idx->n_groups * DCN_GROUP_SLOTS + 1) / 2; }

// the count-and-insert sweep over the dump of one chunk (scan in dump mode with dump_abs = 1)
struct dcn_builder_count_args {
    uint64_t *slots; // the builder's table, with room for every valid entry of the chunk
    uint32_t group_shift, group_mask;
    const uint64_t *dump_hash;
    const uint8_t *dump_valid;
    const uint32_t *dump_pos; // the minimizer's base index in the chunk
    uint64_t n_bases;
    const uint8_t *ascii; // the chunk's bases as given: the entropy floor reads the k-mer
    uint32_t k;
    float entropy_threshold;
    uint32_t *bits;         // one bit per base of the chunk: a position counts once
    uint32_t *counts;       // the slots' counters
    uint32_t *counts_zero;  // key 0's word
    unsigned long long *tally; // += fresh keys, occurrences, (key 0 met ? 1 : 0)
};
int dcn_launch_builder_count(const dcn_builder_count_args &a, hipStream_t stream);
// n <= DCN_BUILDER_MAX_SEAM bits from bit src0 of src to bit dst0 of dst, whose words are zero there
int dcn_launch_builder_seam(const uint32_t *src, uint64_t src0, uint32_t *dst, uint64_t dst0, uint32_t n, hipStream_t stream);
// every key of old_slots into `slots` (empty, large enough), its counter into the half of its new slot (new_counts zero)
int dcn_builder_rehash(const uint64_t *old_slots, const uint32_t *old_counts, uint64_t old_n_slots, uint64_t *slots,
                       uint32_t group_shift, uint32_t group_mask, uint32_t *new_counts, hipStream_t stream);

// sweeps over slots and counters together, four slots per lane; key 0 is left to the caller in all of them
// d_hist[min(count, n_bins - 1)] += occupied slots
int dcn_builder_hist(const dcn_index_builder *b, uint32_t n_bins, unsigned long long *d_hist, hipStream_t stream);
// (key, count) of every occupied slot to d_keys / d_counts[*d_n ...] in no particular order; cap entries
int dcn_builder_export(const dcn_index_builder *b, uint64_t *d_keys, uint32_t *d_counts, uint64_t cap, unsigned long long *d_n,
                       hipStream_t stream);
// occupied slots with lo <= count <= hi: *d_n += their number (dst == null), or their keys go into dst and *d_n += the
// fresh inserts
int dcn_builder_select(const dcn_index_builder *b, uint32_t lo, uint32_t hi, dcn_index *dst, unsigned long long *d_n,
                       hipStream_t stream);
