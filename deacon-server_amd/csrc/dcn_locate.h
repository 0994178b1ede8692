// dcn_locate.h -- the kernels behind dcn_locate_batch (locate.hip; not part of the public ABI).
#pragma once

#include "dcn_dump_sweep.h"

// (the mark kernel is a dump sweep: its geometry is dcn_dump_sweep.h's)
constexpr uint32_t DCN_LOC_THREADS = 256;
// segments: a read of at most this many bases is walked by one lane, bit by bit; a longer one by one wave, a bitmap word
// per lane, which needs every word to hold hits of one segment only: k + max_gap >= 31 (else every read takes the lane path)
constexpr uint32_t DCN_LOC_LANE_BASES = 1024;

struct dcn_locate_args {
    dcn_table_view table;
    const uint32_t *labels; // one member mask per slot (a labelled set); null: a plain index, every hit's label is 1
    uint32_t zero_label;    // key 0's mask (plain index: has_zero)
    uint32_t member_mask;   // ~0 for a plain index
    dcn_dump_view dump;
    const uint64_t *offsets; // n_reads + 1
    uint32_t n_reads;
    uint32_t k;
    uint32_t join;     // a hit at p continues the segment whose last hit is q when p - q <= join (= k + max_gap, saturated)
    uint32_t min_hits;
    uint32_t *bits;          // one bit per base of the batch stream, zero before the mark kernel
    uint32_t *label_scratch; // per base: the label of the hit there (sets only; read only where a bit is set)
    uint32_t *counts;        // per read: segments
    unsigned long long *block_sums; // scratch of dcn_launch_offsets_scan
    uint64_t *seg_offsets;   // n_reads + 1
    dcn_segment *segs;
    uint64_t seg_cap; // entries of segs: a segment at or past it is not written (the host grows the buffer and writes again)
    uint32_t *big;    // reads of the wave path (found by the count pass, reused by the write pass)
    uint32_t *n_big;
};

int dcn_launch_locate_mark(const dcn_locate_args &a, hipStream_t stream);
// counts per read -> seg_offsets (exclusive scan, seg_offsets[n_reads] = the total); zeroes *n_big first
int dcn_launch_locate_count(const dcn_locate_args &a, hipStream_t stream);
int dcn_launch_locate_write(const dcn_locate_args &a, hipStream_t stream);
