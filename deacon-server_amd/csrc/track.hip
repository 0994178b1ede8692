// track.hip -- depth tracks: per bin of every read, a summary of the set's depth counters at the read's minimizer
// positions (dcn_depth_track_batch; the definition is in include/deacon_hip.h).
//
// Runs behind the dump front end (dump_front_end, ctx.hip: pack -> plan -> scan in dump mode with batch-absolute
// positions):
//   track_mark_kernel    the flat sweep over the dump entries (dcn_dump_sweep.h): every valid entry sets bit
//                        `position` of the batch's position bitmap (dcn_bit_mark), finds its slot
//                        (dcn_table_find_slot) and stores value[position] = 0 when the hash
//                        is no key under the mask, else DCN_TRK_KEY | the slot's counter (capped).  Entries that repeat a
//                        position store the same word.  Nothing of the set is written.
//   track_bins_kernel    one lane per bin: a bin of a read of the lane path (dcn_track.h) is walked word by word, the first
//                        and last word cut to the bin; a bin of a wide read is zeroed.
//   track_pieces_kernel  one wave per piece of a wide read's bin: a bitmap word per lane and iteration, the five figures
//                        reduced across the wave in registers, one set of integer atomics per piece into the bin.
// Integers only: the result does not depend on the order of anything.
#include "dcn_track.h"
#include "dcn_probe.h"

#include <algorithm>

namespace {

__global__ __launch_bounds__(DCN_SWEEP_THREADS) void track_mark_kernel(dcn_track_args a) {
    dcn_for_dump_entries(a.dump, [&](uint64_t s) {
        const uint64_t p = dcn_dump_position(a.dump, s);
        if (p >= a.dump.n_bases) return;
        const uint64_t h = a.dump.hash[s];
        uint32_t v = 0;
        if (h == 0) {
            if (a.depth_zero && (a.zero_label & a.member_mask)) v = DCN_TRK_KEY | (*a.depth_zero & DCN_DEPTH_MAX);
        } else {
            const uint32_t g = dcn_group_of(h, a.table.group_shift, a.table.group_mask);
            const uint64_t at = dcn_table_find_slot(a.table, h, g, dcn_load_group(a.table, g));
            if (at != ~0ull && (a.labels[at] & a.member_mask))
                v = DCN_TRK_KEY | ((a.depth[at >> 1] >> ((uint32_t)(at & 1) * 16)) & DCN_DEPTH_MAX);
        }
        if (v && a.depth_cap) v = DCN_TRK_KEY | min(v & DCN_DEPTH_MAX, a.depth_cap);
        dcn_bit_mark(a.bits, p);
        a.value[p] = v; // (windows that share a position share its hash: the same value)
    });
}

struct trk_acc {
    uint32_t n_pos = 0, n_keys = 0, n_obs = 0, max_d = 0, sum = 0;
};

// the positions of one bitmap word
__device__ inline void trk_add_word(const dcn_track_args &a, uint64_t wi, uint32_t word, trk_acc &c) {
    c.n_pos += __popc(word);
    for (; word; word &= word - 1) {
        const uint32_t v = a.value[wi * 32 + (__ffs(word) - 1)];
        const uint32_t d = v & DCN_DEPTH_MAX;
        c.n_keys += v >> 16;
        c.n_obs += d ? 1u : 0u;
        c.sum += d;
        c.max_d = max(c.max_d, d);
    }
}

// one lane per bin
__global__ __launch_bounds__(DCN_TRK_THREADS) void track_bins_kernel(dcn_track_args a) {
    const uint64_t i = (uint64_t)blockIdx.x * DCN_TRK_THREADS + threadIdx.x;
    if (i >= a.n_bins) return;
    const uint32_t r = dcn_owner_of(a.bin_offsets, a.n_reads, i);
    const uint64_t o0 = a.offsets[r], o1 = a.offsets[r + 1];
    const uint64_t bw = dcn_track_bin_width(o1 - o0, a.bin_bases);
    trk_acc c;
    if (bw <= DCN_TRK_LANE_BASES && bw > 0) { // (a wider bin is zeroed here and filled by its pieces)
        const uint64_t b0 = o0 + (i - a.bin_offsets[r]) * bw, b1 = min(b0 + bw, o1);
        for (uint64_t wi = b0 >> 5; wi <= ((b1 - 1) >> 5); ++wi) trk_add_word(a, wi, dcn_bits_cut(a.bits, wi, b0, b1), c);
    }
    dcn_track_bin out;
    out.n_positions = c.n_pos;
    out.n_keys = c.n_keys;
    out.n_observed = c.n_obs;
    out.max_depth = c.max_d;
    out.sum_depth = c.sum;
    a.bins[i] = out;
}

// one wave per piece
__global__ __launch_bounds__(DCN_TRK_THREADS) void track_pieces_kernel(dcn_track_args a) {
    const uint32_t lane = threadIdx.x & (DCN_WAVE - 1);
    const uint32_t waves = DCN_TRK_THREADS / DCN_WAVE;
    for (uint64_t q = (uint64_t)blockIdx.x * waves + threadIdx.x / DCN_WAVE; q < a.n_pieces; q += (uint64_t)gridDim.x * waves) {
        const uint32_t r = dcn_owner_of(a.piece_offsets, a.n_reads, q);
        const uint64_t o0 = a.offsets[r], o1 = a.offsets[r + 1];
        const uint64_t bw = dcn_track_bin_width(o1 - o0, a.bin_bases); // (> DCN_TRK_LANE_BASES: the read has pieces)
        const uint64_t per_bin = (bw + DCN_TRK_PIECE_BASES - 1) / DCN_TRK_PIECE_BASES;
        const uint64_t local = q - a.piece_offsets[r];
        const uint64_t bin = local / per_bin;
        const uint64_t b0 = o0 + bin * bw, b1 = min(b0 + bw, o1);
        const uint64_t p0 = b0 + (local % per_bin) * DCN_TRK_PIECE_BASES;
        if (p0 >= b1) continue; // (the read's short last bin has fewer pieces than the others)
        const uint64_t p1 = min(p0 + DCN_TRK_PIECE_BASES, b1);
        const uint64_t w1 = (p1 - 1) >> 5;
        trk_acc c;
        for (uint64_t wb = p0 >> 5; wb <= w1; wb += DCN_WAVE) {
            const uint64_t wi = wb + lane;
            if (wi <= w1) trk_add_word(a, wi, dcn_bits_cut(a.bits, wi, p0, p1), c);
        }
        for (uint32_t d = DCN_WAVE / 2; d; d >>= 1) {
            c.n_pos += __shfl_xor(c.n_pos, d);
            c.n_keys += __shfl_xor(c.n_keys, d);
            c.n_obs += __shfl_xor(c.n_obs, d);
            c.sum += __shfl_xor(c.sum, d); // (at most DCN_TRK_PIECE_BASES positions of at most 65,535: 32 bits hold it)
            c.max_d = max(c.max_d, __shfl_xor(c.max_d, d));
        }
        if (lane == 0 && c.n_pos) {
            dcn_track_bin *out = a.bins + (a.bin_offsets[r] + bin);
            atomicAdd(&out->n_positions, c.n_pos);
            if (c.n_keys) atomicAdd(&out->n_keys, c.n_keys);
            if (c.n_obs) {
                atomicAdd(&out->n_observed, c.n_obs);
                atomicMax(&out->max_depth, c.max_d);
                atomicAdd(reinterpret_cast<unsigned long long *>(&out->sum_depth), (unsigned long long)c.sum);
            }
        }
    }
}

uint32_t trk_piece_blocks(uint64_t n_pieces) {
    const uint32_t waves = DCN_TRK_THREADS / DCN_WAVE;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n_pieces + waves - 1) / waves, (uint64_t)dcn_cu_count() * 8));
}

} // namespace

int dcn_launch_track_mark(const dcn_track_args &a, hipStream_t stream) {
    return dcn_launch_dump_sweep(track_mark_kernel, a, "track: tile count", stream);
}

int dcn_launch_track_reduce(const dcn_track_args &a, hipStream_t stream) {
    if (a.n_bins == 0) return DCN_OK;
    const uint64_t blocks = (a.n_bins + DCN_TRK_THREADS - 1) / DCN_TRK_THREADS;
    if (blocks > 0x7FFFFFFFull) return dcn_fail(DCN_ERR_INTERNAL, "track: bin count");
    hipLaunchKernelGGL(track_bins_kernel, dim3((uint32_t)blocks), dim3(DCN_TRK_THREADS), 0, stream, a);
    if (a.n_pieces)
        hipLaunchKernelGGL(track_pieces_kernel, dim3(trk_piece_blocks(a.n_pieces)), dim3(DCN_TRK_THREADS), 0, stream, a);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}
