// place.hip -- anchor maps (dcn_anchor_map_*) and placement (dcn_place_batch); the definitions are in
// include/deacon_hip.h, the word layouts in dcn_place.h.
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
//   place_lane_kernel     one lane per read of at most lane_bases bases: it walks the read's words of both bitmaps (first and last
//                         cut to the read), and for every anchor hit counts the hit's two cells against all hits of the
//                         read, until a cell holds them all; the extents are taken in the same inner walk.  A longer read
//                         goes to the work list.
//   place_big_kernel      one workgroup per listed read: cells are counted in an LDS set keyed by (record, j) with a
//                         counter per orientation, in hash partitions of the key: when a partition does not fit the set,
//                         the partition count doubles and the read starts over, so any number of distinct cells is exact
//                         without global scratch.  One more sweep takes the four extents of the winning cell.
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

// ---- vote ---------------------------------------------------------------------------------------------------------
__device__ inline void plc_write(const dcn_place_args &a, uint32_t r, const plc_cell &best, const plc_extent &x,
                                 uint32_t n_anchors, uint32_t n_positions) {
    dcn_placement out;
    const bool placed = best.votes >= a.min_votes && best.votes > 0;
    out.record = placed ? best.rec1 - 1 : 0xFFFFFFFFu;
    out.reverse = placed ? best.o : 0;
    out.votes = placed ? best.votes : 0;
    out.n_anchors = n_anchors;
    out.n_positions = n_positions;
    out.read_start = placed ? x.q0 : 0;
    out.read_end = placed ? x.q1 + a.k : 0;
    out.reserved = 0;
    out.ref_start = placed ? (uint64_t)x.P0 : 0;
    out.ref_end = placed ? (uint64_t)x.P1 + a.k : 0;
    a.out[r] = out;
}

// one lane per read
__global__ __launch_bounds__(DCN_PLC_THREADS) void place_lane_kernel(dcn_place_args a) {
    const uint64_t r = (uint64_t)blockIdx.x * DCN_PLC_THREADS + threadIdx.x;
    if (r >= a.n_reads) return;
    const uint64_t o0 = a.offsets[r], o1 = a.offsets[r + 1];
    const uint64_t len = o1 - o0;
    if (len > a.lane_bases) {
        a.big[atomicAdd(a.n_big, 1u)] = (uint32_t)r;
        return;
    }
    plc_cell best = plc_no_cell();
    plc_extent bx;
    uint32_t n_anchors = 0, n_positions = 0;
    if (len > 0) {
        const uint64_t w0 = o0 >> 5, w1 = (o1 - 1) >> 5;
        for (uint64_t wi = w0; wi <= w1; ++wi) { // the two counts first
            n_positions += __popc(dcn_bits_cut(a.bits, wi, o0, o1));
            n_anchors += __popc(dcn_bits_cut(a.abits, wi, o0, o1));
        }
        // A cell that holds every anchor hit of the read ends the search: a cell that holds them all holds the hit it was
        // found from, h, so it is one of h's two cells, and both have been compared (the common case: a read of one place).
        for (uint64_t wi = w0; wi <= w1 && best.votes < n_anchors; ++wi) {
            uint32_t word = dcn_bits_cut(a.abits, wi, o0, o1);
            for (; word && best.votes < n_anchors; word &= word - 1) {
                const uint64_t p = wi * 32 + (__ffs(word) - 1);
                const uint64_t v = a.words[p];
                const plc_hit h = plc_decode(v, (uint32_t)(p - o0), len, a.band);
                // the hit's two cells against every hit of the read (cell j + 1 holds the hits of j and j + 1 ... of
                // D / W in {j, j + 1}; cell j those in {j - 1, j})
                uint32_t c_lo = 0, c_hi = 0;
                plc_extent x_lo, x_hi;
                for (uint64_t vi = w0; vi <= w1; ++vi) {
                    uint32_t inner = dcn_bits_cut(a.abits, vi, o0, o1);
                    for (; inner; inner &= inner - 1) {
                        const uint64_t p2 = vi * 32 + (__ffs(inner) - 1);
                        const uint64_t v2 = a.words[p2];
                        const plc_hit g = plc_decode(v2, (uint32_t)(p2 - o0), len, a.band);
                        if (g.rec1 != h.rec1 || g.o != h.o) continue;
                        if (g.j == h.j || g.j + 1 == h.j) {
                            ++c_lo;
                            x_lo.q0 = min(x_lo.q0, g.q), x_lo.q1 = max(x_lo.q1, g.q);
                            x_lo.P0 = min(x_lo.P0, g.P), x_lo.P1 = max(x_lo.P1, g.P);
                        }
                        if (g.j == h.j || g.j == h.j + 1) {
                            ++c_hi;
                            x_hi.q0 = min(x_hi.q0, g.q), x_hi.q1 = max(x_hi.q1, g.q);
                            x_hi.P0 = min(x_hi.P0, g.P), x_hi.P1 = max(x_hi.P1, g.P);
                        }
                    }
                }
                if (plc_better(c_lo, h.rec1, h.o, h.j, best)) {
                    best.votes = c_lo, best.rec1 = h.rec1, best.o = h.o, best.j = h.j;
                    bx = x_lo;
                }
                if (plc_better(c_hi, h.rec1, h.o, h.j + 1, best)) {
                    best.votes = c_hi, best.rec1 = h.rec1, best.o = h.o, best.j = h.j + 1;
                    bx = x_hi;
                }
            }
        }
    }
    plc_write(a, (uint32_t)r, best, bx, n_anchors, n_positions);
}

// one workgroup per listed read
__global__ __launch_bounds__(DCN_PLC_THREADS) void place_big_kernel(dcn_place_args a) {
    __shared__ unsigned long long s_key[DCN_PLC_LDS_CELLS]; // (record + 1) << 33 | j; 0: free
    __shared__ uint32_t s_cnt[2][DCN_PLC_LDS_CELLS];
    __shared__ uint32_t s_overflow, s_n_anchors, s_n_positions;
    __shared__ uint32_t s_x[4];
    __shared__ plc_cell s_best; // the best cell of the partitions done so far
    const uint32_t tid = threadIdx.x;
    const uint32_t S = a.lds_cells;
    const uint32_t n_big = *a.n_big;
    for (uint32_t item = blockIdx.x; item < n_big; item += gridDim.x) {
        const uint32_t r = a.big[item];
        const uint64_t o0 = a.offsets[r], o1 = a.offsets[r + 1];
        const uint64_t len = o1 - o0; // (> lane_bases >= 0: the read has bases)
        const uint64_t w0 = o0 >> 5, w1 = (o1 - 1) >> 5;
        uint32_t parts = 1;
        for (;;) { // until every partition of the cell keys fitted the set
            __syncthreads();
            if (tid == 0) {
                s_best = plc_no_cell();
                s_overflow = 0;
            }
            bool redo = false;
            for (uint32_t part = 0; part < parts && !redo; ++part) {
                for (uint32_t i = tid; i < S; i += DCN_PLC_THREADS) {
                    s_key[i] = 0;
                    s_cnt[0][i] = 0;
                    s_cnt[1][i] = 0;
                }
                __syncthreads();
                for (uint64_t wi = w0 + tid; wi <= w1; wi += DCN_PLC_THREADS) {
                    uint32_t word = dcn_bits_cut(a.abits, wi, o0, o1);
                    for (; word; word &= word - 1) {
                        const uint64_t p = wi * 32 + (__ffs(word) - 1);
                        const uint64_t v = a.words[p];
                        const plc_hit h = plc_decode(v, (uint32_t)(p - o0), len, a.band);
                        for (uint32_t c = 0; c < 2; ++c) {
                            const unsigned long long key = ((unsigned long long)h.rec1 << 33) | (h.j + c);
                            const uint64_t m = plc_mix(key);
                            if ((uint32_t)(m & (parts - 1)) != part) continue;
                            uint32_t at = (uint32_t)((m >> 32) % S);
                            uint32_t tries = 0;
                            for (; tries < S; ++tries) {
                                if (*(volatile uint32_t *)&s_overflow) break;
                                unsigned long long old = s_key[at];
                                if (old == 0) old = atomicCAS(&s_key[at], 0ull, key);
                                if (old == 0 || old == key) {
                                    atomicAdd(&s_cnt[h.o][at], 1u);
                                    break;
                                }
                                at = at + 1 == S ? 0 : at + 1;
                            }
                            if (tries == S) s_overflow = 1;
                        }
                    }
                }
                __syncthreads();
                if (s_overflow) {
                    redo = true;
                    break;
                }
                // the partition's best cell: every thread's best over its slots, a wave's by shuffles, then one lane per
                // wave merges into s_best in turn (the order of plc_better is total: the result is the set's maximum)
                {
                    plc_cell mine = plc_no_cell();
                    for (uint32_t i = tid; i < S; i += DCN_PLC_THREADS) {
                        const unsigned long long key = s_key[i];
                        if (!key) continue;
                        for (uint32_t o = 0; o < 2; ++o) {
                            const uint32_t cv = s_cnt[o][i];
                            if (cv && plc_better(cv, (uint32_t)(key >> 33), o, key & 0x1FFFFFFFFull, mine))
                                mine.votes = cv, mine.rec1 = (uint32_t)(key >> 33), mine.o = o, mine.j = key & 0x1FFFFFFFFull;
                        }
                    }
                    for (uint32_t d = DCN_WAVE / 2; d; d >>= 1) {
                        plc_cell other = plc_no_cell();
                        other.votes = __shfl_xor(mine.votes, d);
                        other.rec1 = __shfl_xor(mine.rec1, d);
                        other.o = __shfl_xor(mine.o, d);
                        other.j = __shfl_xor((unsigned long long)mine.j, d);
                        if (plc_better(other.votes, other.rec1, other.o, other.j, mine)) mine = other;
                    }
                    for (uint32_t wv = 0; wv < DCN_PLC_THREADS / DCN_WAVE; ++wv) {
                        if (tid == wv * DCN_WAVE && mine.votes && plc_better(mine.votes, mine.rec1, mine.o, mine.j, s_best))
                            s_best = mine;
                        __syncthreads();
                    }
                }
                __syncthreads();
            }
            if (!redo) break;
            if (parts >= DCN_PLC_MAX_PARTS) break; // (not reached: 2^30 partitions of a 64-bit mix)
            parts *= 2;
        }
        // the extents of the winning cell, and the two counts
        __syncthreads();
        const plc_cell best = s_best;
        if (tid == 0) {
            s_n_anchors = 0, s_n_positions = 0;
            s_x[0] = ~0u, s_x[1] = 0, s_x[2] = ~0u, s_x[3] = 0;
        }
        __syncthreads();
        uint32_t n_anchors = 0, n_positions = 0;
        plc_extent x;
        for (uint64_t wi = w0 + tid; wi <= w1; wi += DCN_PLC_THREADS) {
            n_positions += __popc(dcn_bits_cut(a.bits, wi, o0, o1));
            uint32_t word = dcn_bits_cut(a.abits, wi, o0, o1);
            n_anchors += __popc(word);
            for (; word; word &= word - 1) {
                const uint64_t p = wi * 32 + (__ffs(word) - 1);
                const uint64_t v = a.words[p];
                const plc_hit h = plc_decode(v, (uint32_t)(p - o0), len, a.band);
                if (h.rec1 != best.rec1 || h.o != best.o || !(h.j == best.j || h.j + 1 == best.j)) continue;
                x.q0 = min(x.q0, h.q), x.q1 = max(x.q1, h.q);
                x.P0 = min(x.P0, h.P), x.P1 = max(x.P1, h.P);
            }
        }
        if (n_positions) atomicAdd(&s_n_positions, n_positions);
        if (n_anchors) atomicAdd(&s_n_anchors, n_anchors);
        if (x.q0 != ~0u) {
            atomicMin(&s_x[0], x.q0), atomicMax(&s_x[1], x.q1);
            atomicMin(&s_x[2], x.P0), atomicMax(&s_x[3], x.P1);
        }
        __syncthreads();
        if (tid == 0) {
            plc_extent bx;
            bx.q0 = s_x[0], bx.q1 = s_x[1], bx.P0 = s_x[2], bx.P1 = s_x[3];
            plc_write(a, r, best, bx, s_n_anchors, s_n_positions);
        }
    }
}

uint32_t plc_cus() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return (uint32_t)std::max(cus, 1);
}

uint32_t plc_sweep_blocks(uint64_t n) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + DCN_PLC_THREADS - 1) / DCN_PLC_THREADS, (uint64_t)plc_cus() * 8));
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

int dcn_launch_place_vote(const dcn_place_args &a, hipStream_t stream) {
    if (a.n_reads == 0) return DCN_OK;
    const uint32_t blocks = (a.n_reads + DCN_PLC_THREADS - 1) / DCN_PLC_THREADS;
    hipLaunchKernelGGL(place_lane_kernel, dim3(blocks), dim3(DCN_PLC_THREADS), 0, stream, a);
    DCN_HIP(hipGetLastError());
    if (!a.any_big) return DCN_OK; // (no read is longer than lane_bases: the work list stays empty)
    // (the work list's length is on the device: a fixed grid walks it)
    const uint32_t big_blocks = std::min<uint32_t>(a.n_reads, plc_cus() * 4);
    hipLaunchKernelGGL(place_big_kernel, dim3(big_blocks), dim3(DCN_PLC_THREADS), 0, stream, a);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}
