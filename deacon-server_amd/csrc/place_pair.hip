// place_pair.hip -- the pairing of dcn_place_pair_batch: the two mates of a pair placed jointly from the rounds that
// the vote of place_vote.hip computed per mate (the definition is in include/deacon_hip.h, the buffers in dcn_place.h).
// It runs behind the dump front end, the mark sweep of place.hip and the round launcher of place_vote.hip, which are
// called as they are.
//   place_pair_kernel  one lane per pair.  It reads the two mates' round counts and rounds (at most 9 x 32 bytes per
//                      mate) straight from global memory: no per-lane array exists, so nothing can spill.  The at most
//                      8 x 8 combinations of candidates are evaluated for the chosen one; the paired votes of a mate's
//                      reported round and of the rounds that intersect it are computed on the fly (at most 9 rounds x 8
//                      candidates of the partner per mate).  Both 80-byte rows are written, unplaced ones included.
//                      The insert histogram is kept in 256 LDS counters per workgroup (a workgroup adds at most 256
//                      counts) and leaves with one device atomic per non-zero bin and workgroup.
// Loops are bounded by max_placements + 1 <= 9.  Integers only: the result does not depend on the order of anything.
#include "dcn_place.h"

namespace {

static_assert(DCN_PAIR_HIST_BINS == DCN_PLC_THREADS, "one histogram counter per thread of a workgroup");

struct ppr_params {
    uint32_t k, min_votes, max_insert;
};

// rule 2; *T is written only when the two rounds are concordant
__device__ __forceinline__ bool ppr_concordant(const dcn_split_round &x, const dcn_split_round &y, const ppr_params &p,
                                               uint64_t *T) {
    if (x.rec1 != y.rec1 || x.o == y.o) return false;
    if (max(x.votes, y.votes) < p.min_votes) return false;
    // F: the '+' round, V: the '-' round
    const uint64_t f0 = x.o ? y.P0 : x.P0, f1 = (uint64_t)(x.o ? y.P1 : x.P1) + p.k;
    const uint64_t v0 = x.o ? x.P0 : y.P0, v1 = (uint64_t)(x.o ? x.P1 : y.P1) + p.k;
    if (f0 >= v1) return false;
    const uint64_t t = max(f1, v1) - min(f0, v0);
    if (t > p.max_insert) return false;
    *T = t;
    return true;
}

// rule 4: the paired votes of round t of a mate (`mine`, n_cand candidates) against the other mate's candidates
__device__ __forceinline__ uint32_t ppr_paired_votes(const dcn_split_round *mine, uint32_t t, uint32_t n_cand,
                                                     const dcn_split_round *theirs, uint32_t their_cand, const ppr_params &p) {
    const dcn_split_round me = mine[t];
    uint32_t add = 0;
    if (t < n_cand)
        for (uint32_t b = 0; b < their_cand; ++b) {
            const dcn_split_round other = theirs[b];
            uint64_t T;
            if (ppr_concordant(me, other, p, &T)) add = max(add, other.votes);
        }
    return me.votes + add;
}

// one row: round t of a mate when `placed`, else the unplaced row (rule 3)
__device__ __forceinline__ void ppr_write_row(dcn_pair_placement *at, bool placed, const dcn_split_round *mine, uint32_t t,
                                              uint32_t n_rounds, uint32_t n_cand, const dcn_split_round *theirs,
                                              uint32_t their_cand, const ppr_params &p, uint32_t n_anchors, uint32_t n_positions,
                                              uint32_t n_placed, uint32_t flags, int64_t tlen) {
    dcn_pair_placement o;
    o.n_anchors = n_anchors;
    o.n_positions = n_positions;
    o.reserved = 0;
    if (!placed) {
        o.record = 0xFFFFFFFFu;
        o.reverse = 0, o.votes = 0, o.read_start = 0, o.read_end = 0, o.ref_start = 0, o.ref_end = 0;
        o.rank = 0, o.n_placed = 0, o.rival_votes = 0, o.mapq = 0, o.flags = 0, o.pair_votes = 0, o.tlen = 0;
        *at = o;
        return;
    }
    const dcn_split_round me = mine[t];
    const uint32_t pv = ppr_paired_votes(mine, t, n_cand, theirs, their_cand, p);
    // rule 5: the strongest other computed round, by paired votes, whose read interval intersects this one's
    uint32_t rival = 0;
    for (uint32_t u = 0; u < n_rounds; ++u) {
        if (u == t) continue;
        const dcn_split_round other = mine[u];
        const uint64_t start = max(me.q0, other.q0), end = min((uint64_t)me.q1, (uint64_t)other.q1) + p.k;
        if (start < end) rival = max(rival, ppr_paired_votes(mine, u, n_cand, theirs, their_cand, p));
    }
    o.record = me.rec1 - 1;
    o.reverse = me.o;
    o.votes = me.votes;
    o.read_start = me.q0;
    o.read_end = me.q1 + p.k;
    o.ref_start = me.P0;
    o.ref_end = (uint64_t)me.P1 + p.k;
    o.rank = t;
    o.n_placed = n_placed;
    o.rival_votes = rival;
    o.mapq = rival >= pv ? 0u : (uint32_t)(60ull * (pv - rival) / pv);
    o.flags = flags;
    o.pair_votes = pv;
    o.tlen = tlen;
    *at = o;
}

// one lane per pair
__global__ __launch_bounds__(DCN_PLC_THREADS) void place_pair_kernel(dcn_place_pair_args a) {
    __shared__ uint32_t s_hist[DCN_PAIR_HIST_BINS];
    const bool want_hist = a.hist != nullptr; // (uniform: a kernel argument)
    if (want_hist) {
        s_hist[threadIdx.x] = 0;
        __syncthreads();
    }
    const uint64_t u = (uint64_t)blockIdx.x * DCN_PLC_THREADS + threadIdx.x;
    if (u < a.n_pairs) {
        const uint32_t N = a.max_placements;
        const ppr_params p = {a.k, a.min_votes, a.max_insert};
        const uint64_t r1 = 2 * u, r2 = 2 * u + 1;
        const dcn_split_round *m1 = a.rounds + r1 * (N + 1), *m2 = a.rounds + r2 * (N + 1);
        const uint32_t n1 = min(a.n_rounds[r1], N + 1), n2 = min(a.n_rounds[r2], N + 1); // computed rounds
        const uint32_t c1 = min(n1, N), c2 = min(n2, N);                                  // candidates
        // rule 3: the concordant combination with the most votes, then the smallest a, then the smallest b
        bool proper = false;
        uint32_t best_a = 0, best_b = 0, best_sum = 0;
        uint64_t best_T = 0;
        for (uint32_t i = 0; i < c1; ++i) {
            const dcn_split_round x = m1[i];
            for (uint32_t j = 0; j < c2; ++j) {
                const dcn_split_round y = m2[j];
                uint64_t T;
                if (!ppr_concordant(x, y, p, &T)) continue;
                const uint32_t sum = x.votes + y.votes;
                if (!proper || sum > best_sum) proper = true, best_a = i, best_b = j, best_sum = sum, best_T = T;
            }
        }
        bool placed1, placed2;
        uint32_t f1 = 0, f2 = 0;
        int64_t tl1 = 0, tl2 = 0;
        if (proper) {
            placed1 = placed2 = true;
            const dcn_split_round x = m1[best_a], y = m2[best_b];
            f1 = f2 = DCN_PAIR_PROPER | DCN_PAIR_MATE_PLACED;
            if (x.votes < a.min_votes) f1 |= DCN_PAIR_RESCUED;
            if (y.votes < a.min_votes) f2 |= DCN_PAIR_RESCUED;
            const bool first = x.P0 <= y.P0; // (the smaller ref_start gets +T; a tie goes to mate 1)
            tl1 = first ? (int64_t)best_T : -(int64_t)best_T;
            tl2 = -tl1;
            if (want_hist) atomicAdd(&s_hist[min(best_T / a.hist_bin_bases, (uint64_t)DCN_PAIR_HIST_BINS - 1)], 1u);
        } else {
            placed1 = n1 > 0 && m1[0].votes >= a.min_votes;
            placed2 = n2 > 0 && m2[0].votes >= a.min_votes;
            if (placed1 && placed2) f1 = f2 = DCN_PAIR_MATE_PLACED;
        }
        ppr_write_row(a.out + r1, placed1, m1, best_a, n1, c1, m2, c2, p, a.read_counts[2 * r1], a.read_counts[2 * r1 + 1],
                      a.counts[r1], f1, tl1);
        ppr_write_row(a.out + r2, placed2, m2, best_b, n2, c2, m1, c1, p, a.read_counts[2 * r2], a.read_counts[2 * r2 + 1],
                      a.counts[r2], f2, tl2);
    }
    if (want_hist) {
        __syncthreads();
        const uint32_t mine = s_hist[threadIdx.x];
        if (mine) atomicAdd(a.hist + threadIdx.x, (unsigned long long)mine);
    }
}

} // namespace

int dcn_launch_place_pair(const dcn_place_pair_args &a, hipStream_t stream) {
    if (a.n_pairs == 0) return DCN_OK;
    const uint32_t blocks = (a.n_pairs + DCN_PLC_THREADS - 1) / DCN_PLC_THREADS;
    hipLaunchKernelGGL(place_pair_kernel, dim3(blocks), dim3(DCN_PLC_THREADS), 0, stream, a);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}
