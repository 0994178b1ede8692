// place.hip -- anchor maps (dcn_anchor_map_*) and the mark sweep of the placement calls (dcn_place_batch,
// dcn_place_split_batch, dcn_place_pair_batch); the definitions are in include/deacon_hip.h, the word layouts in dcn_place.h.
//
// Both run behind the dump front end (dump_front_end, ctx.hip: pack -> plan -> scan in dump mode with batch-absolute
// positions):
//   place_sweep_kernel<true>  (add) the flat sweep over the dump entries (dcn_dump_sweep.h): a valid entry whose hash
//                         is a key of the map computes (record, position, strand bit) and moves the slot's word EMPTY -> value -> REPEAT: atomicCAS(EMPTY, v) sets it, an
//                         old word that is neither EMPTY nor v makes the lane store REPEAT (an atomicMax: REPEAT is the
//                         largest word).  The same (record, position) emitted twice is the same v: one occurrence.
//   anchor_tally_kernel / anchor_export_kernel
//                         grid-stride sweeps over the words: counts of anchors and repeats; the anchors themselves, a
//                         wave's share of the output claimed with one returning atomicAdd.
//   place_sweep_kernel<false> (mark) the same sweep over a batch of reads: every valid entry sets bit `position` of the batch's
//                         position bitmap; where the hash is an anchor it also sets the bit of the anchor bitmap and
//                         stores words[position] = the anchor with bit 0 replaced by the XOR of the anchor's and the
//                         read's strand bits (no store for the positions without an anchor, most of them).  Entries
//                         that repeat a position store the same word.  Nothing of the map is written.
// The vote behind the mark sweep is place_vote.hip's.
// Integers only: the result does not depend on the order of anything.
#include "dcn_place.h"
#include "dcn_probe.h"

#include <algorithm>

namespace {

// 1: the forward k-mer at absolute base p is the canonical one (kmer <= revcomp(kmer), the compare of
// dcn_kmer_hash64_bits / dcn_kmer_hash128_bits: they hash the smaller of the two)
__device__ inline uint32_t plc_strand(const uint32_t *packed, uint64_t p, uint32_t k) {
    if (k <= 32) {
        const uint32_t sh = 64 - 2 * k;
        const uint64_t a = (dcn_packed_u64(packed, p) << sh) >> sh;
        const uint64_t b = dcn_revcomp64(a) >> sh;
        return a <= b ? 1u : 0u;
    }
    const uint64_t lo = dcn_packed_u64(packed, p);
    uint64_t hi = dcn_packed_u64(packed, p + 32);
    const uint32_t hb = 2 * k - 64;
    hi &= (~0ull) >> (64 - hb);
    const uint64_t rl = dcn_revcomp64(hi), rh = dcn_revcomp64(lo);
    const uint32_t sh = 128 - 2 * k;
    const uint64_t blo = (rl >> sh) | (rh << (64 - sh));
    const uint64_t bhi = rh >> sh;
    return (hi < bhi || (hi == bhi && lo <= blo)) ? 1u : 0u;
}

// the word of the key `h` in the map (null: not a key)
__device__ inline uint64_t *plc_word_of(const dcn_place_args &a, uint64_t h) {
    if (h == 0) return a.table.has_zero ? a.anchor + a.n_slots : nullptr;
    const uint32_t g = dcn_group_of(h, a.table.group_shift, a.table.group_mask);
    const uint64_t at = dcn_table_find_slot(a.table, h, g, dcn_load_group(a.table, g));
    return at == ~0ull ? nullptr : a.anchor + at;
}

template <bool ADD>
__global__ __launch_bounds__(DCN_SWEEP_THREADS) void place_sweep_kernel(dcn_place_args a) {
    if (a.status->bad_offsets) return; // the scan looked at no tile: the dump is not this batch's
    dcn_for_dump_entries(a.dump, [&](uint64_t s) {
        const uint64_t p = dcn_dump_position(a.dump, s);
        if (p >= a.dump.n_bases) return;
        uint64_t *word = plc_word_of(a, a.dump.hash[s]);
        if (ADD) {
            if (!word) return;
            const uint32_t r = dcn_owner_of(a.offsets, a.n_reads, p);
            const uint64_t v = dcn_anchor_word(a.first_record + r, (uint32_t)(p - a.offsets[r]), plc_strand(a.packed, p, a.k));
            if (*word == DCN_ANCHOR_REPEAT) return; // (a word never leaves REPEAT)
            const uint64_t old = atomicCAS(reinterpret_cast<unsigned long long *>(word), (unsigned long long)DCN_ANCHOR_EMPTY,
                                           (unsigned long long)v);
            if (old != DCN_ANCHOR_EMPTY && old != v && old != DCN_ANCHOR_REPEAT)
                atomicMax(reinterpret_cast<unsigned long long *>(word), (unsigned long long)DCN_ANCHOR_REPEAT);
        } else {
            uint64_t v = 0;
            if (word) {
                const uint64_t w = *word;
                if (dcn_anchor_is_value(w)) v = w ^ (uint64_t)plc_strand(a.packed, p, a.k);
            }
            dcn_bit_mark(a.bits, p);
            if (v) { // (windows that share a position share its hash: the same word)
                dcn_bit_mark(a.abits, p);
                a.words[p] = v;
            }
        }
    });
}

// ---- sweeps over a map's words ------------------------------------------------------------------------------------
__global__ __launch_bounds__(DCN_PLC_THREADS) void anchor_tally_kernel(const uint64_t *anchor, uint64_t n_words,
                                                                       unsigned long long *tally) {
    unsigned long long n_a = 0, n_r = 0;
    const uint64_t stride = (uint64_t)gridDim.x * DCN_PLC_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * DCN_PLC_THREADS + threadIdx.x; i < n_words; i += stride) {
        const uint64_t w = anchor[i];
        n_a += dcn_anchor_is_value(w) ? 1 : 0;
        n_r += w == DCN_ANCHOR_REPEAT ? 1 : 0;
    }
    for (uint32_t d = DCN_WAVE / 2; d; d >>= 1) {
        n_a += __shfl_xor(n_a, d);
        n_r += __shfl_xor(n_r, d);
    }
    if ((threadIdx.x & (DCN_WAVE - 1)) == 0) {
        if (n_a) atomicAdd(&tally[0], n_a);
        if (n_r) atomicAdd(&tally[1], n_r);
    }
}

__global__ __launch_bounds__(DCN_PLC_THREADS) void anchor_export_kernel(const uint64_t *anchor, const uint64_t *slots,
                                                                        uint64_t n_slots, uint64_t *keys, uint32_t *records,
                                                                        uint32_t *positions, uint64_t cap,
                                                                        unsigned long long *n_out) {
    const uint32_t lane = threadIdx.x & (DCN_WAVE - 1);
    const uint64_t n_words = n_slots + 1;
    const uint64_t stride = (uint64_t)gridDim.x * DCN_PLC_THREADS;
    // (wave-uniform trip count: every lane of a wave takes part in the ballot)
    for (uint64_t i0 = (uint64_t)blockIdx.x * DCN_PLC_THREADS + (threadIdx.x - lane); i0 < n_words; i0 += stride) {
        const uint64_t i = i0 + lane;
        const uint64_t w = i < n_words ? anchor[i] : 0;
        const bool is = dcn_anchor_is_value(w);
        const unsigned long long m = __ballot(is);
        if (!m) continue;
        unsigned long long at = 0;
        if (lane == 0) at = atomicAdd(n_out, (unsigned long long)__popcll(m));
        at = __shfl(at, 0) + __popcll(m & ((1ull << lane) - 1));
        if (is && at < cap) {
            keys[at] = i < n_slots ? slots[i] : 0; // (the word behind the slots' is key 0's)
            records[at] = dcn_anchor_record(w);
            positions[at] = dcn_anchor_position(w);
        }
    }
}

uint32_t plc_sweep_blocks(uint64_t n) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + DCN_PLC_THREADS - 1) / DCN_PLC_THREADS, (uint64_t)dcn_cu_count() * 8));
}

} // namespace

int dcn_launch_anchor_add(const dcn_place_args &a, hipStream_t stream) {
    return dcn_launch_dump_sweep(place_sweep_kernel<true>, a, "place: tile count", stream);
}
int dcn_launch_place_mark(const dcn_place_args &a, hipStream_t stream) {
    return dcn_launch_dump_sweep(place_sweep_kernel<false>, a, "place: tile count", stream);
}

int dcn_anchor_tally(const dcn_index *map, unsigned long long *d_tally, hipStream_t stream) {
    const uint64_t n_words = map->n_groups * DCN_GROUP_SLOTS + 1;
    hipLaunchKernelGGL(anchor_tally_kernel, dim3(plc_sweep_blocks(n_words)), dim3(DCN_PLC_THREADS), 0, stream, map->d_anchor,
                       n_words, d_tally);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_anchor_export(const dcn_index *map, uint64_t *d_keys, uint32_t *d_records, uint32_t *d_positions, uint64_t cap,
                      unsigned long long *d_n, hipStream_t stream) {
    const uint64_t n_slots = map->n_groups * DCN_GROUP_SLOTS;
    hipLaunchKernelGGL(anchor_export_kernel, dim3(plc_sweep_blocks(n_slots + 1)), dim3(DCN_PLC_THREADS), 0, stream,
                       map->d_anchor, (const uint64_t *)map->d_slots, n_slots, d_keys, d_records, d_positions, cap, d_n);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}
