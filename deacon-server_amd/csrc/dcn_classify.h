// dcn_classify.h -- labelled index sets and the classification kernels (classify.hip; not part of the public ABI).
#pragma once

#include "dcn_internal.h"

// A labelled set is a dcn_index whose table has the usual slot layout plus a parallel u32 array of member masks
// (dcn_index::d_labels).  A probe reads the key's home group exactly as dcn_table_contains_dev does; only a hit reads the
// 4-byte label at the slot it matched.
constexpr uint32_t DCN_MAX_SET_MEMBERS = 32;

// classify_units_kernel: one lane per unit, up to DCN_CLS_LANE_HITS distinct hits in LDS; a unit with more dump entries
// than DCN_CLS_LANE_ENTRIES (or more distinct hits than the lane holds) goes to classify_big_kernel, one workgroup per unit
// with an LDS hash set of DCN_CLS_SET slots swept in hash partitions (exact for any unit size, no global scratch).
constexpr uint32_t DCN_CLS_LANES = 128;
constexpr uint32_t DCN_CLS_LANE_HITS = 32;
constexpr uint32_t DCN_CLS_LANE_ENTRIES = 64;
constexpr uint32_t DCN_CLS_BIG_THREADS = 256;
constexpr uint32_t DCN_CLS_SET = 4096;

// classify_big_kernel's hash partition of key h among P: the top 32 bits of a 64-bit multiplicative mix, scaled to [0, P)
__host__ __device__ inline uint32_t dcn_cls_partition(uint64_t h, uint32_t P) {
    const uint32_t x = (uint32_t)((h * 0x9E3779B97F4A7C15ull) >> 32);
#ifdef __HIP_DEVICE_COMPILE__
    return __umulhi(x, P);
#else
    return (uint32_t)(((uint64_t)x * P) >> 32);
#endif
}

struct dcn_classify_args {
    dcn_table_view table;   // the set's slots
    const uint32_t *labels; // one mask per slot
    uint32_t zero_label;
    uint32_t n_members;
    // plan + minimizer dump of the batch (scan_kernel<..., DUMP=true>)
    const dcn_tile *tiles;
    const uint32_t *n_tiles;
    const uint64_t *offsets;         // n_reads + 1 base offsets of the batch stream
    const uint32_t *read_tiles;      // per read: tile count
    const uint32_t *read_tile_first; // per read: first tile
    const uint32_t *unit_first_read; // n_units + 1, null: unit == read
    const uint64_t *dump_hash;
    const uint8_t *dump_valid;
    const uint32_t *dump_count; // per tile: entries at [tile's read offset + j * tile_windows, + count)
    uint32_t tile_windows;
    uint32_t n_units;
    uint64_t abs_threshold;
    double rel_threshold;
    // outputs (hits / total may be null)
    uint32_t *match;
    uint32_t *hits; // n_units * n_members
    uint32_t *total;
    // units handed to the workgroup kernel
    uint32_t *big;
    uint32_t *n_big;
    const dcn_status *status;  // bad_offsets: the plan refused the batch, every output is written as zero
    dcn_batch_report *report;  // receives bad_offsets (reported at the next dcn_ctx_synchronize)
    // coverage (dcn_index_set_coverage_enable; null = off, the COV = false kernels): bit s of the bitmap = slot s's key
    // was among a unit's counted minimizers; key 0, which has no slot, has a word of its own (bit 0)
    uint32_t *cov_bits;
    uint32_t *cov_zero;
};

int dcn_launch_classify_units(const dcn_classify_args &a, hipStream_t stream);
int dcn_launch_classify_big(const dcn_classify_args &a, hipStream_t stream);

// coverage sweeps of a set with a bitmap (dcn_index::d_cov): per member j, observed[j] += marked slots whose label has
// bit j (keys[j] += occupied slots whose label has bit j, when all_slots); key 0 is left to the caller
int dcn_coverage_count(const dcn_index *set, bool all_slots, unsigned long long *d_counts, hipStream_t stream);
// *d_n += the marked slots whose label meets `mask` (any bit); collect writes their keys to d_out (cap entries, sized by
// a count pass) in no particular order, *d_n counting from 0.  Key 0 is left to the caller.
int dcn_coverage_count_mask(const dcn_index *set, uint32_t mask, unsigned long long *d_n, hipStream_t stream);
int dcn_coverage_collect(const dcn_index *set, uint32_t mask, uint64_t *d_out, uint64_t cap, unsigned long long *d_n,
                         hipStream_t stream);

// set->d_slots / d_labels allocated and clear: insert every key of `member`, OR-ing (1 << bit) into its label
int dcn_set_add_member(dcn_index *set, const dcn_index *member, uint32_t bit);
