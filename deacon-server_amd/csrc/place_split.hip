// place_split.hip -- the CSR tail of dcn_place_split_batch: the reported placements of every read, each with its rival
// and quality (the definition is in include/deacon_hip.h, the buffers in dcn_place.h).  It runs behind the rounds of
// place_vote.hip, which leave per read its computed rounds, their number and the number of reported ones.
//   dcn_launch_offsets_scan   the exclusive scan of the per-read counts (offsets_scan.hip).
//   place_split_write_kernel  one lane per read: the rival and quality of every reported round from the read's computed
//                             rounds (at most 9), written at the read's CSR offset.
// Integers only: the result does not depend on the order of anything.
#include "dcn_place.h"

namespace {

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

} // namespace

int dcn_launch_place_split_rows(const dcn_place_split_args &s, hipStream_t stream) {
    const uint32_t n_reads = s.p.n_reads;
    if (n_reads == 0) return DCN_OK;
    const int rc = dcn_launch_offsets_scan(s.counts, n_reads, s.block_sums, s.place_offsets, stream);
    if (rc != DCN_OK) return rc;
    const uint32_t blocks = (n_reads + DCN_PLC_THREADS - 1) / DCN_PLC_THREADS;
    hipLaunchKernelGGL(place_split_write_kernel, dim3(blocks), dim3(DCN_PLC_THREADS), 0, stream, s);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_place_split_vote(const dcn_place_split_args &s, hipStream_t stream) {
    const int rc = dcn_launch_place_split_rounds(s, stream);
    return rc != DCN_OK ? rc : dcn_launch_place_split_rows(s, stream);
}
