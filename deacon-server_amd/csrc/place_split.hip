// place_split.hip -- the vote of dcn_place_split_batch: up to max_placements placements per read, each with its rival
// and quality (the definition is in include/deacon_hip.h, the buffers in dcn_place.h).  It runs behind the dump front
// end and the mark sweep of place.hip, which are called as they are.
//   place_split_lane_kernel  one lane per read of at most lane_bases bases.  A round is place_lane_kernel's search (every
//                         remaining hit's two cells counted against all remaining hits, until a cell holds them all)
//                         over the bits still set in the read's words of `rbits`; the lane then clears the bits of the
//                         winning cell's hits and stores the round.  A longer read goes to the work list.
//   place_split_big_kernel   one workgroup per listed read.  A round is place_big_kernel's partitioned LDS count over the
//                         remaining hits, then one sweep that takes the four extents of the winning cell and clears its
//                         hits.  The partition count CARRIES OVER from round to round: the hits of a round are a subset
//                         of the round before, so are its cell keys, and a partition count at which every partition
//                         fitted the set fits again.
//   place_split_scan_*    the exclusive scan of the per-read counts (the three kernels of locate's scan).
//   place_split_write_kernel one lane per read: the rival and quality of every reported round from the read's computed
//                         rounds (at most 9), written at the read's CSR offset.
// Rounds are bounded by max_placements + 1 <= 9, partitions by DCN_PLC_MAX_PARTS.  Integers only: the result does not
// depend on the order of anything.
#include "dcn_place.h"

#include <algorithm>

namespace {

// word wi of the remaining-hits bitmap, cut to [b0, b1): loaded at device scope (other lanes clear bits of the words a
// read shares with its neighbours, and this lane's own atomicAnd is performed in L2)
__device__ __forceinline__ uint32_t pls_cut(const uint32_t *rbits, uint64_t wi, uint64_t b0, uint64_t b1) {
    uint32_t word = __hip_atomic_load(rbits + wi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (wi == (b0 >> 5)) word &= ~0u << (b0 & 31);
    if (wi == (b1 >> 5)) word &= ~(~0u << (b1 & 31));
    return word;
}

// clears `gone` (bits of this read) in word wi; `word` is the word as pls_cut gave it.  Only the read's first and last
// word can hold bits of other reads
__device__ __forceinline__ void pls_clear(uint32_t *rbits, uint64_t wi, uint32_t word, uint32_t gone, uint64_t w0, uint64_t w1) {
    if (wi == w0 || wi == w1) atomicAnd(rbits + wi, ~gone);
    else __hip_atomic_store(rbits + wi, word & ~gone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline bool pls_in_cell(const plc_hit &h, const plc_cell &c) {
    return h.rec1 == c.rec1 && h.o == c.o && (h.j == c.j || h.j + 1 == c.j);
}

__device__ inline void pls_store_round(dcn_split_round *at, const plc_cell &best, const plc_extent &x) {
    dcn_split_round rd;
    rd.votes = best.votes, rd.rec1 = best.rec1, rd.o = best.o;
    rd.q0 = x.q0, rd.q1 = x.q1, rd.P0 = x.P0, rd.P1 = x.P1;
    rd.pad = 0;
    *at = rd;
}

// one lane per read
__global__ __launch_bounds__(DCN_PLC_THREADS) void place_split_lane_kernel(dcn_place_split_args s) {
    const dcn_place_args &a = s.p;
    const uint64_t r = (uint64_t)blockIdx.x * DCN_PLC_THREADS + threadIdx.x;
    if (r >= a.n_reads) return;
    const uint64_t o0 = a.offsets[r], o1 = a.offsets[r + 1];
    const uint64_t len = o1 - o0;
    if (len > a.lane_bases) {
        a.big[atomicAdd(a.n_big, 1u)] = (uint32_t)r;
        return;
    }
    const uint32_t N = s.max_placements;
    dcn_split_round *rounds = s.rounds + r * (N + 1);
    uint32_t n_anchors = 0, n_positions = 0, t = 0, n_placed = 0;
    if (len > 0) {
        const uint64_t w0 = o0 >> 5, w1 = (o1 - 1) >> 5;
        for (uint64_t wi = w0; wi <= w1; ++wi) {
            n_positions += __popc(dcn_bits_cut(a.bits, wi, o0, o1));
            n_anchors += __popc(dcn_bits_cut(a.abits, wi, o0, o1));
        }
        uint32_t n_rem = n_anchors; // hits no round has taken yet
        for (; t <= N && n_rem; ++t) {
            plc_cell best = plc_no_cell();
            plc_extent bx;
            // (as in place_lane_kernel: a cell that holds every remaining hit ends the round)
            for (uint64_t wi = w0; wi <= w1 && best.votes < n_rem; ++wi) {
                uint32_t word = pls_cut(s.rbits, wi, o0, o1);
                for (; word && best.votes < n_rem; word &= word - 1) {
                    const uint64_t p = wi * 32 + (__ffs(word) - 1);
                    const plc_hit h = plc_decode(a.words[p], (uint32_t)(p - o0), len, a.band);
                    uint32_t c_lo = 0, c_hi = 0;
                    plc_extent x_lo, x_hi;
                    for (uint64_t vi = w0; vi <= w1; ++vi) {
                        uint32_t inner = pls_cut(s.rbits, vi, o0, o1);
                        for (; inner; inner &= inner - 1) {
                            const uint64_t p2 = vi * 32 + (__ffs(inner) - 1);
                            const plc_hit g = plc_decode(a.words[p2], (uint32_t)(p2 - o0), len, a.band);
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
            if (best.votes == 0) break; // (not reached: a remaining hit gives both of its cells a vote)
            pls_store_round(rounds + t, best, bx);
            if (t < N && best.votes >= a.min_votes) ++n_placed; // (votes never rise: the reported rounds are a prefix)
            n_rem -= best.votes;
            if (n_rem == 0 || t == N) continue; // (nothing left to count, or no round follows)
            for (uint64_t wi = w0; wi <= w1; ++wi) {
                const uint32_t word = pls_cut(s.rbits, wi, o0, o1);
                uint32_t gone = 0;
                for (uint32_t rest = word; rest; rest &= rest - 1) {
                    const uint32_t b = __ffs(rest) - 1;
                    const uint64_t p = wi * 32 + b;
                    if (pls_in_cell(plc_decode(a.words[p], (uint32_t)(p - o0), len, a.band), best)) gone |= 1u << b;
                }
                if (gone) pls_clear(s.rbits, wi, word, gone, w0, w1);
            }
        }
    }
    s.n_rounds[r] = t;
    s.counts[r] = n_placed;
    s.read_counts[2 * r] = n_anchors;
    s.read_counts[2 * r + 1] = n_positions;
}

// one workgroup per listed read
__global__ __launch_bounds__(DCN_PLC_THREADS) void place_split_big_kernel(dcn_place_split_args s) {
    __shared__ unsigned long long s_key[DCN_PLC_LDS_CELLS]; // (record + 1) << 33 | j; 0: free
    __shared__ uint32_t s_cnt[2][DCN_PLC_LDS_CELLS];
    __shared__ uint32_t s_overflow, s_n_anchors, s_n_positions;
    __shared__ uint32_t s_x[4];
    __shared__ plc_cell s_best; // the best cell of the partitions done so far
    const dcn_place_args &a = s.p;
    const uint32_t tid = threadIdx.x;
    const uint32_t S = a.lds_cells;
    const uint32_t N = s.max_placements;
    const uint32_t n_big = *a.n_big;
    for (uint32_t item = blockIdx.x; item < n_big; item += gridDim.x) {
        const uint32_t r = a.big[item];
        const uint64_t o0 = a.offsets[r], o1 = a.offsets[r + 1];
        const uint64_t len = o1 - o0; // (> lane_bases >= 0: the read has bases)
        const uint64_t w0 = o0 >> 5, w1 = (o1 - 1) >> 5;
        dcn_split_round *rounds = s.rounds + (uint64_t)r * (N + 1);
        // the two counts, from the bitmaps as the mark left them
        __syncthreads();
        if (tid == 0) s_n_anchors = 0, s_n_positions = 0;
        __syncthreads();
        {
            uint32_t n_anchors = 0, n_positions = 0;
            for (uint64_t wi = w0 + tid; wi <= w1; wi += DCN_PLC_THREADS) {
                n_positions += __popc(dcn_bits_cut(a.bits, wi, o0, o1));
                n_anchors += __popc(dcn_bits_cut(a.abits, wi, o0, o1));
            }
            if (n_positions) atomicAdd(&s_n_positions, n_positions);
            if (n_anchors) atomicAdd(&s_n_anchors, n_anchors);
        }
        __syncthreads();
        uint32_t n_rem = s_n_anchors; // (the same in every thread, as t, parts and n_placed are)
        uint32_t parts = 1, t = 0, n_placed = 0;
        for (; t <= N && n_rem; ++t) {
            // A thread walks the same words wi = w0 + tid, + DCN_PLC_THREADS ... in every sweep of every round, so the
            // bits it loads are the ones it cleared itself.
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
                        uint32_t word = pls_cut(s.rbits, wi, o0, o1);
                        for (; word; word &= word - 1) {
                            const uint64_t p = wi * 32 + (__ffs(word) - 1);
                            const plc_hit h = plc_decode(a.words[p], (uint32_t)(p - o0), len, a.band);
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
                    // the partition's best cell, merged into s_best (as in place_big_kernel)
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
            // the extents of the winning cell; its hits leave the remaining ones
            __syncthreads();
            const plc_cell best = s_best;
            if (best.votes == 0) break; // (not reached: see the lane kernel; uniform, s_best is read behind a barrier)
            if (tid == 0) s_x[0] = ~0u, s_x[1] = 0, s_x[2] = ~0u, s_x[3] = 0;
            __syncthreads();
            plc_extent x;
            for (uint64_t wi = w0 + tid; wi <= w1; wi += DCN_PLC_THREADS) {
                const uint32_t word = pls_cut(s.rbits, wi, o0, o1);
                uint32_t gone = 0;
                for (uint32_t rest = word; rest; rest &= rest - 1) {
                    const uint32_t b = __ffs(rest) - 1;
                    const uint64_t p = wi * 32 + b;
                    const plc_hit h = plc_decode(a.words[p], (uint32_t)(p - o0), len, a.band);
                    if (!pls_in_cell(h, best)) continue;
                    gone |= 1u << b;
                    x.q0 = min(x.q0, h.q), x.q1 = max(x.q1, h.q);
                    x.P0 = min(x.P0, h.P), x.P1 = max(x.P1, h.P);
                }
                if (gone) pls_clear(s.rbits, wi, word, gone, w0, w1);
            }
            if (x.q0 != ~0u) {
                atomicMin(&s_x[0], x.q0), atomicMax(&s_x[1], x.q1);
                atomicMin(&s_x[2], x.P0), atomicMax(&s_x[3], x.P1);
            }
            __syncthreads();
            if (tid == 0) {
                plc_extent bx;
                bx.q0 = s_x[0], bx.q1 = s_x[1], bx.P0 = s_x[2], bx.P1 = s_x[3];
                pls_store_round(rounds + t, best, bx);
            }
            if (t < N && best.votes >= a.min_votes) ++n_placed;
            n_rem -= best.votes;
        }
        if (tid == 0) {
            s.n_rounds[r] = t;
            s.counts[r] = n_placed;
            s.read_counts[2 * (uint64_t)r] = s_n_anchors;
            s.read_counts[2 * (uint64_t)r + 1] = s_n_positions;
        }
    }
}

// ---- exclusive scan of counts[0..n) into place_offsets[0..n], place_offsets[n] = the total ---------------------------
__device__ inline uint32_t pls_thread_sum(const dcn_place_split_args &s, uint32_t i0) {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t i = 0; i < DCN_PLS_SCAN_ITEMS; ++i)
        if (i0 + i < s.p.n_reads) v += s.counts[i0 + i];
    return v;
}

// inclusive scan of one value per thread over the workgroup
__device__ inline uint32_t pls_block_scan(uint32_t v, uint32_t *s_wave) {
    const uint32_t lane = threadIdx.x & (DCN_WAVE - 1), wave = threadIdx.x / DCN_WAVE;
    for (uint32_t d = 1; d < DCN_WAVE; d <<= 1) {
        const uint32_t o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    if (lane == DCN_WAVE - 1) s_wave[wave] = v;
    __syncthreads();
    for (uint32_t q = 0; q < wave; ++q) v += s_wave[q];
    return v;
}

__global__ __launch_bounds__(DCN_PLC_THREADS) void place_split_scan_sums_kernel(dcn_place_split_args s) {
    __shared__ uint32_t s_wave[DCN_PLC_THREADS / DCN_WAVE];
    const uint32_t i0 = blockIdx.x * DCN_PLS_SCAN_BLOCK + threadIdx.x * DCN_PLS_SCAN_ITEMS;
    const uint32_t incl = pls_block_scan(pls_thread_sum(s, i0), s_wave);
    if (threadIdx.x == DCN_PLC_THREADS - 1) s.block_sums[blockIdx.x] = incl;
}

// one workgroup: block_sums[] -> their exclusive prefix
__global__ __launch_bounds__(DCN_PLC_THREADS) void place_split_scan_blocks_kernel(dcn_place_split_args s, uint32_t n_blocks) {
    __shared__ unsigned long long s_part[DCN_PLC_THREADS];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (n_blocks + DCN_PLC_THREADS - 1) / DCN_PLC_THREADS;
    const uint32_t b0 = min(tid * per, n_blocks), b1 = min(b0 + per, n_blocks);
    unsigned long long mine = 0;
    for (uint32_t b = b0; b < b1; ++b) mine += s.block_sums[b];
    s_part[tid] = mine;
    __syncthreads();
    unsigned long long before = 0;
    for (uint32_t q = 0; q < tid; ++q) before += s_part[q];
    for (uint32_t b = b0; b < b1; ++b) {
        const unsigned long long v = s.block_sums[b];
        s.block_sums[b] = before;
        before += v;
    }
}

__global__ __launch_bounds__(DCN_PLC_THREADS) void place_split_scan_write_kernel(dcn_place_split_args s) {
    __shared__ uint32_t s_wave[DCN_PLC_THREADS / DCN_WAVE];
    const uint32_t i0 = blockIdx.x * DCN_PLS_SCAN_BLOCK + threadIdx.x * DCN_PLS_SCAN_ITEMS;
    const uint32_t mine = pls_thread_sum(s, i0);
    uint64_t at = s.block_sums[blockIdx.x] + (pls_block_scan(mine, s_wave) - mine);
    if (i0 == 0) s.place_offsets[0] = 0;
    for (uint32_t i = 0; i < DCN_PLS_SCAN_ITEMS && i0 + i < s.p.n_reads; ++i) {
        at += s.counts[i0 + i];
        s.place_offsets[i0 + i + 1] = at;
    }
}

// ---- the CSR rows: rival and quality ---------------------------------------------------------------------------------
__global__ __launch_bounds__(DCN_PLC_THREADS) void place_split_write_kernel(dcn_place_split_args s) {
    const uint64_t r = (uint64_t)blockIdx.x * DCN_PLC_THREADS + threadIdx.x;
    if (r >= s.p.n_reads) return;
    const uint32_t n_placed = s.counts[r];
    if (n_placed == 0) return;
    const uint32_t n_rounds = min(s.n_rounds[r], s.max_placements + 1);
    const dcn_split_round *rounds = s.rounds + r * (s.max_placements + 1);
    const uint32_t k = s.p.k;
    const uint32_t n_anchors = s.read_counts[2 * r], n_positions = s.read_counts[2 * r + 1];
    dcn_split_placement *out = s.out + s.place_offsets[r];
    for (uint32_t t = 0; t < n_placed; ++t) {
        const dcn_split_round me = rounds[t];
        // the strongest other computed round whose read interval [q0, q1 + k) intersects this one's
        uint32_t rival = 0;
        for (uint32_t u = 0; u < n_rounds; ++u) {
            if (u == t) continue;
            const dcn_split_round other = rounds[u];
            const uint64_t start = max(me.q0, other.q0), end = min((uint64_t)me.q1, (uint64_t)other.q1) + k;
            if (start < end) rival = max(rival, other.votes);
        }
        dcn_split_placement o;
        o.record = me.rec1 - 1;
        o.reverse = me.o;
        o.votes = me.votes;
        o.n_anchors = n_anchors;
        o.n_positions = n_positions;
        o.read_start = me.q0;
        o.read_end = me.q1 + k;
        o.reserved = 0;
        o.ref_start = me.P0;
        o.ref_end = (uint64_t)me.P1 + k;
        o.rank = t;
        o.n_placed = n_placed;
        o.rival_votes = rival;
        o.mapq = rival >= me.votes ? 0u : (uint32_t)(60ull * (me.votes - rival) / me.votes);
        out[t] = o;
    }
}

uint32_t pls_cus() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return (uint32_t)std::max(cus, 1);
}

} // namespace

// the rounds (what dcn_place_pair_batch consumes too), then the CSR tail; dcn_launch_place_split_vote is both, in order
int dcn_launch_place_split_rounds(const dcn_place_split_args &s, hipStream_t stream) {
    const uint32_t n_reads = s.p.n_reads;
    if (n_reads == 0) return DCN_OK;
    const uint32_t blocks = (n_reads + DCN_PLC_THREADS - 1) / DCN_PLC_THREADS;
    hipLaunchKernelGGL(place_split_lane_kernel, dim3(blocks), dim3(DCN_PLC_THREADS), 0, stream, s);
    DCN_HIP(hipGetLastError());
    if (s.p.any_big) { // (the work list's length is on the device: a fixed grid walks it)
        const uint32_t big_blocks = std::min<uint32_t>(n_reads, pls_cus() * 4);
        hipLaunchKernelGGL(place_split_big_kernel, dim3(big_blocks), dim3(DCN_PLC_THREADS), 0, stream, s);
        DCN_HIP(hipGetLastError());
    }
    return DCN_OK;
}

int dcn_launch_place_split_rows(const dcn_place_split_args &s, hipStream_t stream) {
    const uint32_t n_reads = s.p.n_reads;
    if (n_reads == 0) return DCN_OK;
    const uint32_t blocks = (n_reads + DCN_PLC_THREADS - 1) / DCN_PLC_THREADS;
    const uint32_t scan_blocks = (n_reads + DCN_PLS_SCAN_BLOCK - 1) / DCN_PLS_SCAN_BLOCK;
    hipLaunchKernelGGL(place_split_scan_sums_kernel, dim3(scan_blocks), dim3(DCN_PLC_THREADS), 0, stream, s);
    hipLaunchKernelGGL(place_split_scan_blocks_kernel, dim3(1), dim3(DCN_PLC_THREADS), 0, stream, s, scan_blocks);
    hipLaunchKernelGGL(place_split_scan_write_kernel, dim3(scan_blocks), dim3(DCN_PLC_THREADS), 0, stream, s);
    hipLaunchKernelGGL(place_split_write_kernel, dim3(blocks), dim3(DCN_PLC_THREADS), 0, stream, s);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_place_split_vote(const dcn_place_split_args &s, hipStream_t stream) {
    const int rc = dcn_launch_place_split_rounds(s, stream);
    return rc != DCN_OK ? rc : dcn_launch_place_split_rows(s, stream);
}
