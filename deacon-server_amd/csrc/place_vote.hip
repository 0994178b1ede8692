// place_vote.hip -- the vote of the placement family: one round, written once, behind dcn_place_batch (one round per
// read, the placement written), dcn_place_split_batch and dcn_place_pair_batch (up to max_placements + 1 rounds per
// read, each stored for the CSR tail of place_split.hip and the pairing of place_pair.hip).  The definitions are in
// include/deacon_hip.h, the buffers in dcn_place.h.  It runs behind the dump front end and the mark sweep of place.hip.
//
// A ROUND finds the best cell of a read over the anchor hits whose bit is set in a bitmap, and the four extents of that
// cell's hits.  The two instantiations differ in the bitmap only (plc_cut, pls_clear):
//   single  `abits` as the mark left it, plain loads, never written: one round
//   split   `rbits`, the copy that the rounds clear, loaded at device scope: a round clears the bits of its winning
//           cell's hits, so the next round counts what is left
//   place_lane_kernel  one lane per read of at most lane_bases bases.  plc_lane_round walks the read's words of the
//                      bitmap and counts every hit's two cells against all hits, until a cell holds them all; the
//                      extents are taken in the same inner walk.  A longer read goes to the work list.
//   place_wg_kernel    one workgroup per listed read; it declares the LDS set.  plc_wg_count counts cells in it, keyed
//                      by (record, j) with a counter per orientation, in hash partitions of the key: when a partition
//                      does not fit the set, the partition count doubles and the count starts over, so any number of
//                      distinct cells is exact without global scratch.  plc_wg_extents is one more sweep for the four
//                      extents of the winning cell; split clears the cell's hits in it, single takes n_anchors /
//                      n_positions in it (split needs n_anchors before its first round and counts both up front).
//                      The partition count of a split read CARRIES OVER from round to round: the hits of a round are a
//                      subset of the round before, so are its cell keys, and a partition count at which every partition
//                      fitted the set fits again.
// Rounds are bounded by max_placements + 1 <= 9, partitions by DCN_PLC_MAX_PARTS.  Integers only: the result does not
// depend on the order of anything.
#include "dcn_place.h"

#include <algorithm>
#include <type_traits>

namespace {

// an anchor hit of a read: the word of base p = o0 + q of a read of len bases
struct plc_hit {
    uint32_t rec1; // record + 1
    uint32_t o;    // 0: '+', 1: '-'
    uint32_t q, P;
    uint64_t j;    // D / W: the hit votes for cells j and j + 1 of (record, o)
};
__device__ inline plc_hit plc_decode(uint64_t w, uint32_t q, uint64_t len, uint32_t band) {
    plc_hit h;
    h.rec1 = (uint32_t)(w >> 33);
    h.o = (uint32_t)(w & 1);
    h.q = q;
    h.P = dcn_anchor_position(w);
    const uint64_t D = h.o ? (uint64_t)h.P + q : (uint64_t)h.P + len - q;
    h.j = D / band;
    return h;
}

// a cell and its votes; better(): more votes, then the smaller (record, o, j)
struct plc_cell {
    uint32_t votes, rec1, o;
    uint64_t j;
};
__device__ inline plc_cell plc_no_cell() { return plc_cell{0, 0, 0, 0}; }
__device__ inline bool plc_better(uint32_t votes, uint32_t rec1, uint32_t o, uint64_t j, const plc_cell &b) {
    if (votes != b.votes) return votes > b.votes;
    if (rec1 != b.rec1) return rec1 < b.rec1;
    if (o != b.o) return o < b.o;
    return j < b.j;
}
__device__ inline bool plc_in_cell(const plc_hit &h, const plc_cell &c) {
    return h.rec1 == c.rec1 && h.o == c.o && (h.j == c.j || h.j + 1 == c.j);
}

// min q, max q, min P, max P over the hits added
struct plc_extent {
    uint32_t q0 = ~0u, q1 = 0, P0 = ~0u, P1 = 0;
    __device__ void add(const plc_hit &h) {
        q0 = min(q0, h.q), q1 = max(q1, h.q);
        P0 = min(P0, h.P), P1 = max(P1, h.P);
    }
};

__device__ inline uint64_t plc_mix(uint64_t x) {
    x ^= x >> 33;
    x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33;
    x *= 0xC4CEB9FE1A85EC53ull;
    return x ^ (x >> 33);
}

// ---- the two instantiations: arguments, bitmap, result -----------------------------------------------------------------
template <bool SPLIT>
using plc_args = std::conditional_t<SPLIT, dcn_place_split_args, dcn_place_args>;
__device__ __host__ inline const dcn_place_args &plc_base(const dcn_place_args &a) { return a; }
__device__ __host__ inline const dcn_place_args &plc_base(const dcn_place_split_args &s) { return s.p; }
__device__ inline uint32_t *plc_bitmap(const dcn_place_args &a) { return a.abits; }
__device__ inline uint32_t *plc_bitmap(const dcn_place_split_args &s) { return s.rbits; }

// a read's bases [o0, o1) of the batch stream and its words [w0, w1] of a bitmap (len > 0)
struct plc_read {
    uint64_t o0, o1, len, w0, w1;
};
__device__ inline plc_read plc_read_of(const dcn_place_args &a, uint64_t r) {
    plc_read rd;
    rd.o0 = a.offsets[r], rd.o1 = a.offsets[r + 1];
    rd.len = rd.o1 - rd.o0;
    rd.w0 = rd.o0 >> 5, rd.w1 = (rd.o1 - 1) >> 5;
    return rd;
}

// word wi of the round's bitmap, cut to the read.  Split loads at device scope: other lanes clear bits of the words a
// read shares with its neighbours, and this lane's own atomicAnd is performed in L2 (see dcn_place.h)
template <bool SPLIT>
__device__ __forceinline__ uint32_t plc_cut(const uint32_t *bits, uint64_t wi, const plc_read &rd) {
    if constexpr (!SPLIT) return dcn_bits_cut(bits, wi, rd.o0, rd.o1);
    uint32_t word = __hip_atomic_load(bits + wi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (wi == (rd.o0 >> 5)) word &= ~0u << (rd.o0 & 31);
    if (wi == (rd.o1 >> 5)) word &= ~(~0u << (rd.o1 & 31));
    return word;
}

// clears `gone` (bits of this read) in word wi of rbits; `word` is the word as plc_cut gave it.  Only the read's first
// and last word can hold bits of other reads
__device__ __forceinline__ void pls_clear(uint32_t *rbits, uint64_t wi, uint32_t word, uint32_t gone, const plc_read &rd) {
    if (wi == rd.w0 || wi == rd.w1) atomicAnd(rbits + wi, ~gone);
    else __hip_atomic_store(rbits + wi, word & ~gone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

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

__device__ inline void pls_store_round(dcn_split_round *at, const plc_cell &best, const plc_extent &x) {
    dcn_split_round rd;
    rd.votes = best.votes, rd.rec1 = best.rec1, rd.o = best.o;
    rd.q0 = x.q0, rd.q1 = x.q1, rd.P0 = x.P0, rd.P1 = x.P1;
    rd.pad = 0;
    *at = rd;
}

// ---- lane form ----------------------------------------------------------------------------------------------------------
// One round over the n_rem hits whose bit is set: the best cell, its extents in *bx.  A cell that holds every remaining
// hit ends the search: a cell that holds them all holds the hit it was found from, h, so it is one of h's two cells, and
// both have been compared (the common case: a read of one place).
template <bool SPLIT>
__device__ inline plc_cell plc_lane_round(const dcn_place_args &a, const uint32_t *bits, const plc_read &rd, uint32_t n_rem,
                                          plc_extent *bx) {
    plc_cell best = plc_no_cell();
    for (uint64_t wi = rd.w0; wi <= rd.w1 && best.votes < n_rem; ++wi) {
        uint32_t word = plc_cut<SPLIT>(bits, wi, rd);
        for (; word && best.votes < n_rem; word &= word - 1) {
            const uint64_t p = wi * 32 + (__ffs(word) - 1);
            const plc_hit h = plc_decode(a.words[p], (uint32_t)(p - rd.o0), rd.len, a.band);
            // the hit's two cells against every hit of the round (cell j + 1 holds the hits of j and j + 1 ... of
            // D / W in {j, j + 1}; cell j those in {j - 1, j})
            uint32_t c_lo = 0, c_hi = 0;
            plc_extent x_lo, x_hi;
            for (uint64_t vi = rd.w0; vi <= rd.w1; ++vi) {
                uint32_t inner = plc_cut<SPLIT>(bits, vi, rd);
                for (; inner; inner &= inner - 1) {
                    const uint64_t p2 = vi * 32 + (__ffs(inner) - 1);
                    const plc_hit g = plc_decode(a.words[p2], (uint32_t)(p2 - rd.o0), rd.len, a.band);
                    if (g.rec1 != h.rec1 || g.o != h.o) continue;
                    if (g.j == h.j || g.j + 1 == h.j) ++c_lo, x_lo.add(g);
                    if (g.j == h.j || g.j == h.j + 1) ++c_hi, x_hi.add(g);
                }
            }
            if (plc_better(c_lo, h.rec1, h.o, h.j, best)) {
                best.votes = c_lo, best.rec1 = h.rec1, best.o = h.o, best.j = h.j;
                *bx = x_lo;
            }
            if (plc_better(c_hi, h.rec1, h.o, h.j + 1, best)) {
                best.votes = c_hi, best.rec1 = h.rec1, best.o = h.o, best.j = h.j + 1;
                *bx = x_hi;
            }
        }
    }
    return best;
}

// one lane per read
template <bool SPLIT>
__global__ __launch_bounds__(DCN_PLC_THREADS) void place_lane_kernel(plc_args<SPLIT> s) {
    const dcn_place_args &a = plc_base(s);
    const uint64_t r = (uint64_t)blockIdx.x * DCN_PLC_THREADS + threadIdx.x;
    if (r >= a.n_reads) return;
    const plc_read rd = plc_read_of(a, r);
    if (rd.len > a.lane_bases) {
        a.big[atomicAdd(a.n_big, 1u)] = (uint32_t)r;
        return;
    }
    uint32_t *bits = plc_bitmap(s);
    uint32_t n_anchors = 0, n_positions = 0;
    if (rd.len > 0) // the two counts first, from the bitmaps as the mark left them
        for (uint64_t wi = rd.w0; wi <= rd.w1; ++wi) {
            n_positions += __popc(dcn_bits_cut(a.bits, wi, rd.o0, rd.o1));
            n_anchors += __popc(dcn_bits_cut(a.abits, wi, rd.o0, rd.o1));
        }
    if constexpr (!SPLIT) {
        plc_extent bx;
        const plc_cell best = plc_lane_round<false>(a, bits, rd, n_anchors, &bx); // (no anchors: no walk)
        plc_write(a, (uint32_t)r, best, bx, n_anchors, n_positions);
    } else {
        const uint32_t N = s.max_placements;
        dcn_split_round *rounds = s.rounds + r * (N + 1);
        uint32_t t = 0, n_placed = 0;
        uint32_t n_rem = n_anchors; // hits no round has taken yet
        for (; t <= N && n_rem; ++t) {
            plc_extent bx;
            const plc_cell best = plc_lane_round<true>(a, bits, rd, n_rem, &bx);
            if (best.votes == 0) break; // (not reached: a remaining hit gives both of its cells a vote)
            pls_store_round(rounds + t, best, bx);
            if (t < N && best.votes >= a.min_votes) ++n_placed; // (votes never rise: the reported rounds are a prefix)
            n_rem -= best.votes;
            if (n_rem == 0 || t == N) continue; // (nothing left to count, or no round follows)
            for (uint64_t wi = rd.w0; wi <= rd.w1; ++wi) {
                const uint32_t word = plc_cut<true>(bits, wi, rd);
                uint32_t gone = 0;
                for (uint32_t rest = word; rest; rest &= rest - 1) {
                    const uint32_t b = __ffs(rest) - 1;
                    const uint64_t p = wi * 32 + b;
                    if (plc_in_cell(plc_decode(a.words[p], (uint32_t)(p - rd.o0), rd.len, a.band), best)) gone |= 1u << b;
                }
                if (gone) pls_clear(bits, wi, word, gone, rd);
            }
        }
        s.n_rounds[r] = t;
        s.counts[r] = n_placed;
        s.read_counts[2 * r] = n_anchors;
        s.read_counts[2 * r + 1] = n_positions;
    }
}

// ---- workgroup form -----------------------------------------------------------------------------------------------------
// What a workgroup keeps in LDS, as place_wg_kernel declares it: the cell set, and what the sweeps sum up for thread 0.
// (Separate variables behind pointers and not one struct in LDS: that layout costs the single-placement kernel registers.)
struct plc_lds {
    unsigned long long *key; // (record + 1) << 33 | j; 0: free
    uint32_t (*cnt)[DCN_PLC_LDS_CELLS];
    uint32_t *overflow, *n_anchors, *n_positions;
    uint32_t *x;    // plc_extent's fields
    plc_cell *best; // the best cell of the partitions done so far
};

// The best cell of a round, counted by the whole workgroup in the LDS set; the same value in every thread.  `parts` is
// the partition count to start from, and on return the one at which every partition fitted.
template <bool SPLIT>
__device__ inline plc_cell plc_wg_count(const dcn_place_args &a, const uint32_t *bits, const plc_read &rd, uint32_t &parts,
                                        const plc_lds &s) {
    const uint32_t tid = threadIdx.x;
    const uint32_t S = a.lds_cells;
    for (;;) { // until every partition of the cell keys fitted the set
        __syncthreads();
        if (tid == 0) {
            *s.best = plc_no_cell();
            *s.overflow = 0;
        }
        bool redo = false;
        for (uint32_t part = 0; part < parts && !redo; ++part) {
            for (uint32_t i = tid; i < S; i += DCN_PLC_THREADS) {
                s.key[i] = 0;
                s.cnt[0][i] = 0;
                s.cnt[1][i] = 0;
            }
            __syncthreads();
            // (a thread walks the same words wi = w0 + tid, + DCN_PLC_THREADS ... in every sweep of every round, so the
            // bits it loads are the ones it cleared itself)
            for (uint64_t wi = rd.w0 + tid; wi <= rd.w1; wi += DCN_PLC_THREADS) {
                uint32_t word = plc_cut<SPLIT>(bits, wi, rd);
                for (; word; word &= word - 1) {
                    const uint64_t p = wi * 32 + (__ffs(word) - 1);
                    const plc_hit h = plc_decode(a.words[p], (uint32_t)(p - rd.o0), rd.len, a.band);
                    for (uint32_t c = 0; c < 2; ++c) {
                        const unsigned long long key = ((unsigned long long)h.rec1 << 33) | (h.j + c);
                        const uint64_t m = plc_mix(key);
                        if ((uint32_t)(m & (parts - 1)) != part) continue;
                        uint32_t at = (uint32_t)((m >> 32) % S);
                        uint32_t tries = 0;
                        for (; tries < S; ++tries) {
                            if (*(volatile uint32_t *)s.overflow) break;
                            unsigned long long old = s.key[at];
                            if (old == 0) old = atomicCAS(&s.key[at], 0ull, key);
                            if (old == 0 || old == key) {
                                atomicAdd(&s.cnt[h.o][at], 1u);
                                break;
                            }
                            at = at + 1 == S ? 0 : at + 1;
                        }
                        if (tries == S) *s.overflow = 1;
                    }
                }
            }
            __syncthreads();
            if (*s.overflow) {
                redo = true;
                break;
            }
            // the partition's best cell: every thread's best over its slots, a wave's by shuffles, then one lane per
            // wave merges into *s.best in turn (the order of plc_better is total: the result is the set's maximum)
            plc_cell mine = plc_no_cell();
            for (uint32_t i = tid; i < S; i += DCN_PLC_THREADS) {
                const unsigned long long key = s.key[i];
                if (!key) continue;
                for (uint32_t o = 0; o < 2; ++o) {
                    const uint32_t cv = s.cnt[o][i];
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
                if (tid == wv * DCN_WAVE && mine.votes && plc_better(mine.votes, mine.rec1, mine.o, mine.j, *s.best))
                    *s.best = mine;
                __syncthreads();
            }
            __syncthreads();
        }
        if (!redo) break;
        if (parts >= DCN_PLC_MAX_PARTS) break; // (not reached: 2^30 partitions of a 64-bit mix)
        parts *= 2;
    }
    __syncthreads();
    return *s.best;
}

// The sweep behind the count: the extents of `best` over the round's hits (thread 0 reads them from sums.x behind the
// barrier this ends with).  Split clears those hits; single adds the read's two counts to sums, zeroed here.
template <bool SPLIT>
__device__ inline void plc_wg_extents(const dcn_place_args &a, uint32_t *bits, const plc_read &rd, const plc_cell &best,
                                      const plc_lds &sums) {
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        if constexpr (!SPLIT) *sums.n_anchors = 0, *sums.n_positions = 0;
        sums.x[0] = ~0u, sums.x[1] = 0, sums.x[2] = ~0u, sums.x[3] = 0;
    }
    __syncthreads();
    uint32_t n_anchors = 0, n_positions = 0;
    plc_extent x;
    for (uint64_t wi = rd.w0 + tid; wi <= rd.w1; wi += DCN_PLC_THREADS) {
        const uint32_t word = plc_cut<SPLIT>(bits, wi, rd);
        if constexpr (!SPLIT) {
            n_positions += __popc(dcn_bits_cut(a.bits, wi, rd.o0, rd.o1));
            n_anchors += __popc(word);
        }
        uint32_t gone = 0;
        for (uint32_t rest = word; rest; rest &= rest - 1) {
            const uint32_t b = __ffs(rest) - 1;
            const uint64_t p = wi * 32 + b;
            const plc_hit h = plc_decode(a.words[p], (uint32_t)(p - rd.o0), rd.len, a.band);
            if (!plc_in_cell(h, best)) continue;
            gone |= 1u << b;
            x.add(h);
        }
        if constexpr (SPLIT)
            if (gone) pls_clear(bits, wi, word, gone, rd);
    }
    if (n_positions) atomicAdd(sums.n_positions, n_positions);
    if (n_anchors) atomicAdd(sums.n_anchors, n_anchors);
    if (x.q0 != ~0u) {
        atomicMin(&sums.x[0], x.q0), atomicMax(&sums.x[1], x.q1);
        atomicMin(&sums.x[2], x.P0), atomicMax(&sums.x[3], x.P1);
    }
    __syncthreads();
}

__device__ inline plc_extent plc_wg_extent(const plc_lds &sums) {
    plc_extent bx;
    bx.q0 = sums.x[0], bx.q1 = sums.x[1], bx.P0 = sums.x[2], bx.P1 = sums.x[3];
    return bx;
}

// one workgroup per listed read
template <bool SPLIT>
__global__ __launch_bounds__(DCN_PLC_THREADS) void place_wg_kernel(plc_args<SPLIT> s) {
    __shared__ unsigned long long s_key[DCN_PLC_LDS_CELLS];
    __shared__ uint32_t s_cnt[2][DCN_PLC_LDS_CELLS];
    __shared__ uint32_t s_overflow, s_n_anchors, s_n_positions;
    __shared__ uint32_t s_x[4];
    __shared__ plc_cell s_best;
    const plc_lds lds{s_key, s_cnt, &s_overflow, &s_n_anchors, &s_n_positions, s_x, &s_best};
    const dcn_place_args &a = plc_base(s);
    uint32_t *bits = plc_bitmap(s);
    const uint32_t tid = threadIdx.x;
    const uint32_t n_big = *a.n_big;
    for (uint32_t item = blockIdx.x; item < n_big; item += gridDim.x) {
        const uint32_t r = a.big[item];
        const plc_read rd = plc_read_of(a, r); // (len > lane_bases >= 0: the read has bases)
        uint32_t parts = 1;
        if constexpr (!SPLIT) {
            const plc_cell best = plc_wg_count<false>(a, bits, rd, parts, lds);
            plc_wg_extents<false>(a, bits, rd, best, lds);
            if (tid == 0) plc_write(a, r, best, plc_wg_extent(lds), s_n_anchors, s_n_positions);
        } else {
            const uint32_t N = s.max_placements;
            dcn_split_round *rounds = s.rounds + (uint64_t)r * (N + 1);
            // the two counts, from the bitmaps as the mark left them
            __syncthreads();
            if (tid == 0) s_n_anchors = 0, s_n_positions = 0;
            __syncthreads();
            {
                uint32_t n_anchors = 0, n_positions = 0;
                for (uint64_t wi = rd.w0 + tid; wi <= rd.w1; wi += DCN_PLC_THREADS) {
                    n_positions += __popc(dcn_bits_cut(a.bits, wi, rd.o0, rd.o1));
                    n_anchors += __popc(dcn_bits_cut(a.abits, wi, rd.o0, rd.o1));
                }
                if (n_positions) atomicAdd(&s_n_positions, n_positions);
                if (n_anchors) atomicAdd(&s_n_anchors, n_anchors);
            }
            __syncthreads();
            uint32_t n_rem = s_n_anchors; // (the same in every thread, as t, parts and n_placed are)
            uint32_t t = 0, n_placed = 0;
            for (; t <= N && n_rem; ++t) {
                const plc_cell best = plc_wg_count<true>(a, bits, rd, parts, lds);
                if (best.votes == 0) break; // (not reached: see the lane kernel; uniform, the cell is read behind a barrier)
                plc_wg_extents<true>(a, bits, rd, best, lds); // its hits leave the remaining ones
                if (tid == 0) pls_store_round(rounds + t, best, plc_wg_extent(lds));
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
}

// lane grid, then the fixed grid that walks the work list (its length is on the device)
template <bool SPLIT>
int plc_launch_vote(const plc_args<SPLIT> &s, hipStream_t stream) {
    const dcn_place_args &a = plc_base(s);
    if (a.n_reads == 0) return DCN_OK;
    const uint32_t blocks = (a.n_reads + DCN_PLC_THREADS - 1) / DCN_PLC_THREADS;
    hipLaunchKernelGGL(place_lane_kernel<SPLIT>, dim3(blocks), dim3(DCN_PLC_THREADS), 0, stream, s);
    DCN_HIP(hipGetLastError());
    if (!a.any_big) return DCN_OK; // (no read is longer than lane_bases: the work list stays empty)
    const uint32_t big_blocks = std::min<uint32_t>(a.n_reads, dcn_cu_count() * 4);
    hipLaunchKernelGGL(place_wg_kernel<SPLIT>, dim3(big_blocks), dim3(DCN_PLC_THREADS), 0, stream, s);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

} // namespace

int dcn_launch_place_vote(const dcn_place_args &a, hipStream_t stream) { return plc_launch_vote<false>(a, stream); }
int dcn_launch_place_split_rounds(const dcn_place_split_args &s, hipStream_t stream) { return plc_launch_vote<true>(s, stream); }
