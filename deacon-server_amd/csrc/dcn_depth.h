// dcn_depth.h -- depth of a labelled set's keys: how often each key occurred among the minimizers classify calls counted
// (depth.hip; not part of the public ABI).
//
// State (dcn_index::d_depth): u32 words of two 16-bit counters, slot s in word s >> 1, half s & 1, and one more word for
// key 0, which has no slot.  A counter saturates at 65,535.  2 B per slot: 8 GiB at the panhuman-sized set.
#pragma once

#include "dcn_dump_sweep.h"

constexpr uint32_t DCN_DEPTH_THREADS = 256; // (the read-out sweeps; the counting sweep's geometry is dcn_dump_sweep.h's)
constexpr uint32_t DCN_DEPTH_MAX = 0xFFFFu;
constexpr uint32_t DCN_DEPTH_MAX_BINS = 4096;

// +1 on the 16-bit half at `shift` of *word, saturating at DCN_DEPTH_MAX and never carrying into the other half.  A
// saturated counter costs a load and no atomic: a key that thousands of lanes hit at once issues at most 65,535 successful
// compare-and-swaps per reset.
__device__ inline void dcn_depth_add(uint32_t *word, uint32_t shift) {
    uint32_t cur = __atomic_load_n(word, __ATOMIC_RELAXED);
    for (;;) {
        if (((cur >> shift) & DCN_DEPTH_MAX) == DCN_DEPTH_MAX) return;
        const uint32_t old = atomicCAS(word, cur, cur + (1u << shift));
        if (old == cur) return;
        cur = old;
    }
}

// the counting sweep over the minimizer dump of a batch
struct dcn_depth_args {
    dcn_table_view table; // the set's slots
    dcn_dump_view dump;
    const dcn_status *status; // bad_offsets: the plan refused the batch, nothing is counted
    uint32_t *bits;           // one bit per base of the batch stream, zero before the sweep: a position counts once
    uint32_t *depth;          // the set's counters
    uint32_t *depth_zero;     // key 0's word (null: key 0 is not in the set)
};

int dcn_launch_depth_count(const dcn_depth_args &a, hipStream_t stream);

// sweeps over labels and counters together; key 0 is left to the caller in all of them
// per member j < n_members: d_out[j] += keys with depth > 0, d_out[32 + j] += the sum of their depths,
// d_out[64 + j] += keys at 65,535
int dcn_depth_stats(const dcn_index *set, unsigned long long *d_out, hipStream_t stream);
// d_hist[min(depth, n_bins - 1)] += occupied slots whose label meets `mask` (bin 0: the unobserved ones)
int dcn_depth_hist(const dcn_index *set, uint32_t mask, uint32_t n_bins, unsigned long long *d_hist, hipStream_t stream);
// slots with depth > 0 whose label meets `mask`: counted (d_keys == null: *d_n += the count) or written to
// d_keys / d_depths[*d_n ...] in no particular order (cap entries: a position at or past cap is not written)
int dcn_depth_keys(const dcn_index *set, uint32_t mask, uint64_t *d_keys, uint32_t *d_depths, uint64_t cap,
                   unsigned long long *d_n, hipStream_t stream);
