// dcn_track.h -- the kernels behind dcn_depth_track_batch (track.hip; not part of the public ABI).
#pragma once

#include "dcn_depth.h"
#include "dcn_dump_sweep.h"

// (the mark kernel is a dump sweep: its geometry is dcn_dump_sweep.h's)
constexpr uint32_t DCN_TRK_THREADS = 256;
// value[p] of a marked position p: 0 = its hash is no key under the mask, else DCN_TRK_KEY | depth (capped)
constexpr uint32_t DCN_TRK_KEY = 0x10000u;
// reduce: a read whose widest bin (min(bin_bases, its length); its length when bin_bases == 0) has at most this many
// bases has every bin walked by one lane; the bins of a wider read are cut into pieces of DCN_TRK_PIECE_BASES bases from
// the bin's first base, a wave per piece, a bitmap word per lane and iteration
constexpr uint32_t DCN_TRK_LANE_BASES = 1024;
constexpr uint32_t DCN_TRK_PIECE_BASES = 4 * DCN_WAVE * 32; // four iterations of a wave when the piece starts a word
// (a piece's depths are summed in 32 bits and added to the bin's 64 with one atomic)
static_assert((uint64_t)DCN_TRK_PIECE_BASES * DCN_DEPTH_MAX <= 0xFFFFFFFFull, "a piece's sum of depths fits 32 bits");
static_assert((uint64_t)DCN_TRK_LANE_BASES * DCN_DEPTH_MAX <= 0xFFFFFFFFull, "a lane's sum of depths fits 32 bits");

struct dcn_track_args {
    dcn_table_view table;   // the set's slots
    const uint32_t *labels; // one member mask per slot
    uint32_t zero_label;    // key 0's mask
    uint32_t member_mask;
    const uint32_t *depth;      // the set's counters: read, never written
    const uint32_t *depth_zero; // key 0's word (null: key 0 is not in the set)
    uint32_t depth_cap;         // 0: none
    dcn_dump_view dump;
    const uint64_t *offsets; // n_reads + 1
    uint32_t n_reads;
    uint32_t bin_bases;            // 0: one bin per read
    const uint64_t *bin_offsets;   // n_reads + 1: read r owns bins [bin_offsets[r], bin_offsets[r + 1])
    const uint64_t *piece_offsets; // n_reads + 1: pieces of read r (none for a read of the lane path; a wide read has
                                   // ceil(widest bin / DCN_TRK_PIECE_BASES) per bin, its short last bin included)
    uint64_t n_bins, n_pieces;
    uint32_t *bits;  // one bit per base of the batch stream, zero before the mark kernel: the positions of the list
    uint32_t *value; // per base, read only where a bit is set
    dcn_track_bin *bins;
};

int dcn_launch_track_mark(const dcn_track_args &a, hipStream_t stream);
// every bin is written: by its lane, or zeroed by its lane and then added to by its pieces' waves
int dcn_launch_track_reduce(const dcn_track_args &a, hipStream_t stream);

// the widest bin of a read of len bases, and whether its bins take the wave path (host and device agree through these)
__host__ __device__ inline uint64_t dcn_track_bin_width(uint64_t len, uint32_t bin_bases) {
    return (bin_bases == 0 || bin_bases > len) ? len : bin_bases;
}
__host__ __device__ inline uint64_t dcn_track_read_bins(uint64_t len, uint32_t bin_bases) {
    return bin_bases == 0 ? 1 : (len + bin_bases - 1) / bin_bases;
}
__host__ __device__ inline uint64_t dcn_track_bin_pieces(uint64_t len, uint32_t bin_bases) {
    const uint64_t bw = dcn_track_bin_width(len, bin_bases);
    return bw > DCN_TRK_LANE_BASES ? (bw + DCN_TRK_PIECE_BASES - 1) / DCN_TRK_PIECE_BASES : 0;
}
