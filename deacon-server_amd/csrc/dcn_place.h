// dcn_place.h -- anchor maps and placement: the kernels behind dcn_anchor_map_* and the mark sweep (place.hip), the vote
// of dcn_place_batch, dcn_place_split_batch and dcn_place_pair_batch (place_vote.hip), and what consumes its rounds: the
// CSR tail of the split call (place_split.hip) and the pairing (place_pair.hip); not part of the public ABI.
#pragma once

#include "dcn_dump_sweep.h"

// (the add and mark kernels are dump sweeps: their geometry is dcn_dump_sweep.h's)
constexpr uint32_t DCN_PLC_THREADS = 256;

// The word of a slot of an anchor map (dcn_index::d_anchor; key 0's word follows the slots' words):
//   DCN_ANCHOR_EMPTY   no occurrence of the key among the records added so far
//   DCN_ANCHOR_REPEAT  two or more distinct occurrences
//   else               bits 63..33 = record + 1 (1 .. 2^31 - 1), bits 32..1 = position, bit 0 = the strand bit (1: the
//                      forward k-mer at the position is the canonical one)
// record + 1 is never 0, so a value is never EMPTY.  REPEAT would be record + 1 == 2^31 - 1 at position 2^32 - 1 with
// the strand bit set, and a record of at most 2^32 - 1 bases has no k-mer that starts at base 2^32 - 1: a value is
// never REPEAT either.
// The same layout is the word per base of a placed batch (dcn_ctx::d_plc_words), with bit 0 = the XOR of the record's
// and the read's strand bits (1: orientation '-'); it is written only at the positions of the anchor bitmap.
constexpr uint64_t DCN_ANCHOR_EMPTY = 0;
constexpr uint64_t DCN_ANCHOR_REPEAT = ~0ull;
constexpr uint32_t DCN_ANCHOR_MAX_RECORDS = 0x7FFFFFFFu;
constexpr uint64_t DCN_ANCHOR_MAX_RECORD_BASES = 0xFFFFFFFFull;
__host__ __device__ inline uint64_t dcn_anchor_word(uint32_t record, uint32_t position, uint32_t strand) {
    return ((uint64_t)(record + 1) << 33) | ((uint64_t)position << 1) | (strand & 1u);
}
__host__ __device__ inline bool dcn_anchor_is_value(uint64_t w) { return w != DCN_ANCHOR_EMPTY && w != DCN_ANCHOR_REPEAT; }
__host__ __device__ inline uint32_t dcn_anchor_record(uint64_t w) { return (uint32_t)(w >> 33) - 1; }
__host__ __device__ inline uint32_t dcn_anchor_position(uint64_t w) { return (uint32_t)(w >> 1); }

// vote: a read of at most DCN_PLC_LANE_BASES bases (DCN_PLACE_LANE_BASES at call time) is placed by one lane, which
// counts every candidate cell against all of the read's anchor hits; a longer read goes to the work list and gets a
// workgroup, which counts cells in an LDS set of DCN_PLC_LDS_CELLS slots (DCN_PLACE_LDS_CELLS at call time, 16 ..
// DCN_PLC_LDS_CELLS): 8 bytes of key (record + 1, j) and two 4-byte counters ('+', '-') per slot.
constexpr uint32_t DCN_PLC_LANE_BASES = 512;
constexpr uint32_t DCN_PLC_LDS_CELLS = 2048; // 32 KB of LDS
constexpr uint32_t DCN_PLC_LDS_CELLS_MIN = 16;
constexpr uint32_t DCN_PLC_MAX_PARTS = 1u << 30; // partitions of the cell keys double up to here

struct dcn_place_args {
    dcn_table_view table;   // the map's slots
    uint64_t *anchor;       // one word per slot, then key 0's (written by the add sweep only)
    uint64_t n_slots;
    uint32_t k;
    uint32_t first_record;  // add: record number of read 0 of the batch
    const uint32_t *packed; // 2-bit stream of the batch (offset by DCN_FRONT_PAD words)
    const dcn_status *status;
    dcn_dump_view dump;
    const uint64_t *offsets; // n_reads + 1
    uint32_t n_reads;
    // placement
    uint32_t band, min_votes;
    uint32_t lane_bases, lds_cells;
    uint32_t any_big; // 1: some read of the batch is longer than lane_bases (known on the host: the workgroup kernel is
                      // launched only then)
    uint32_t *bits;   // one bit per base of the batch stream, zero before the mark kernel: the positions of the list
    uint32_t *abits;  // the same, zero before the mark kernel: the positions whose hash is an anchor
    uint64_t *words;  // per base, written and read only where a bit of abits is set
    uint32_t *big;    // work list of the workgroup kernel
    uint32_t *n_big;  // its length, zero before the lane kernel
    dcn_placement *out; // n_reads
};

int dcn_launch_anchor_add(const dcn_place_args &a, hipStream_t stream);
// tally[0] = anchors, tally[1] = repeats over the n_slots + 1 words
int dcn_anchor_tally(const dcn_index *map, unsigned long long *d_tally, hipStream_t stream);
// anchors in no particular order; *d_n counts them all, the first cap are written
int dcn_anchor_export(const dcn_index *map, uint64_t *d_keys, uint32_t *d_records, uint32_t *d_positions, uint64_t cap,
                      unsigned long long *d_n, hipStream_t stream);
int dcn_launch_place_mark(const dcn_place_args &a, hipStream_t stream);
int dcn_launch_place_vote(const dcn_place_args &a, hipStream_t stream);

// ---- split placements (dcn_place_split_batch: place_vote.hip, place_split.hip) ------------------------------------
// The vote runs the rounds of "THE DEFINITION OF A SPLIT PLACEMENT" over a copy of the anchor bitmap, `rbits`: a round
// counts the cells of the hits whose bit is still set, and clears the bits of the winning cell's hits.  The anchor
// bitmap itself stays as the mark left it (n_anchors is counted there).  A read's first and last word of the copy are
// shared with its neighbours: those are cleared with atomicAnd, the words inside with a store, and every word is
// loaded at device scope so that a round sees what the round before cleared.
// One computed round of a read (max_placements + 1 per read, n_rounds[r] of them computed):
struct dcn_split_round {
    uint32_t votes, rec1, o;
    uint32_t q0, q1, P0, P1; // extents over the cell's hits of the round (min q, max q, min P, max P)
    uint32_t pad;
};
struct dcn_place_split_args {
    dcn_place_args p;        // what the mark filled and the vote's parameters (p.out is not used)
    uint32_t *rbits;         // the copy of p.abits that the rounds clear
    uint32_t max_placements; // N: rounds 0 .. N are computed, 0 .. N - 1 reported
    dcn_split_round *rounds; // n_reads * (N + 1)
    uint32_t *n_rounds;      // per read: computed rounds
    uint32_t *read_counts;   // per read: n_anchors, n_positions
    uint32_t *counts;        // per read: reported placements
    unsigned long long *block_sums; // scratch of dcn_launch_offsets_scan
    uint64_t *place_offsets; // n_reads + 1
    dcn_split_placement *out; // n_reads * N entries: the CSR rows are written at place_offsets
};

// rounds per read (dcn_launch_place_vote's kernels, switch and work list, instantiated with the clearing bitmap) ->
// rounds, n_rounds, counts, read_counts; *p.n_big is zero before
int dcn_launch_place_split_rounds(const dcn_place_split_args &s, hipStream_t stream);
// the CSR tail: counts -> place_offsets (exclusive scan, place_offsets[n_reads] = the total) -> out
int dcn_launch_place_split_rows(const dcn_place_split_args &s, hipStream_t stream);
// both, in that order on the one stream
int dcn_launch_place_split_vote(const dcn_place_split_args &s, hipStream_t stream);

// ---- paired placements (dcn_place_pair_batch, place_pair.hip) ------------------------------------------------------
// A consumer of the rounds beside place_split_write_kernel: one lane per pair reads the two mates' computed rounds
// (reads 2u and 2u + 1) where the round launcher left them and writes both rows of "THE DEFINITION OF A PAIRED
// PLACEMENT".
struct dcn_place_pair_args {
    const dcn_split_round *rounds; // n_reads * (max_placements + 1)
    const uint32_t *n_rounds;      // per read: computed rounds
    const uint32_t *read_counts;   // per read: n_anchors, n_positions
    const uint32_t *counts;        // per read: n_placed of the split call
    uint32_t n_pairs;
    uint32_t max_placements, k, min_votes, max_insert, hist_bin_bases;
    dcn_pair_placement *out;       // 2 * n_pairs
    unsigned long long *hist;      // DCN_PAIR_HIST_BINS counters, zero before; NULL: no histogram
};
int dcn_launch_place_pair(const dcn_place_pair_args &a, hipStream_t stream);
