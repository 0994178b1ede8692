// left_align.hip -- the left alignment of aligned rows (THE DEFINITION OF A LEFT-ALIGNED PLACEMENT, include/deacon_hip.h;
// the procedure is dcn_left_align.h's, which the host compiles as well).
//   left_align_kernel  behind the last align kernel and in front of the scan of the run counts: a wave per aligned row
//                      over the call's work list.  The wave reads the row's runs in chunks of 64 and asks by a ballot
//                      whether a chunk holds a gap: a row without one costs that read and nothing else.  A row with one
//                      is fed run by run to dcn_la_feed, the same in every lane: the gaps of a row are serial (N1, N4).
//                      The new runs grow in the row's words of a second slot array (dcn_left_align.h: out from the
//                      bottom, the passed runs from the top); lane 0 alone writes and reads them back, so every read
//                      sees its write.  Within a gap the wave compares together: lane g takes the g-th group of 16
//                      bases of the backward self-match, a ballot finds the first group that stops.  A row in which a
//                      gap took a step is copied to the end of its slot, where the gather looks, and its n_ops is
//                      written again; any other row is not written at all.  A wave adds what its rows had to the four
//                      totals once, and only what is not zero.
// Integers only; nothing depends on lanes or on the grid.
#include "dcn_left_align.h"
#include "dcn_verify.h"

#include <algorithm>

namespace {

constexpr uint32_t LA_THREADS = 256; // four waves

// how a wave reads and writes a row's words and compares bases (dcn_la_serial is the host's form)
struct la_wave {
    static __device__ uint32_t load(const uint32_t *p) {
        uint32_t v = 0;
        if ((threadIdx.x & 63u) == 0) v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
    }
    static __device__ void store(uint32_t *p, uint32_t v) {
        if ((threadIdx.x & 63u) == 0) *p = v;
    }
    // dcn_wf_match_run_back with the groups of 16 spread over the lanes, 1024 bases a round.  A lane whose group begins at
    // or past the limit reads nothing and stops the run there.
    static __device__ uint64_t steps(const dcn_wf_side &side, int64_t g, int64_t len, uint64_t limit) {
        const uint32_t lane = threadIdx.x & 63u;
        const dcn_wf_side A = dcn_wf_side_back(side, g - 1), B = dcn_wf_side_back(side, g + len - 1);
        for (uint64_t t0 = 0; t0 < limit; t0 += 1024) {
            const uint64_t off = t0 + 16u * lane;
            uint32_t r = 0;
            if (off < limit) {
                uint32_t xa, ia, xb, ib;
                dcn_wf_side16<dcn_wf_guarded>(A, (int64_t)off, &xa, &ia);
                dcn_wf_side16<dcn_wf_guarded>(B, (int64_t)off, &xb, &ib);
                r = dcn_wf_run16(xa, xb, ia | ib);
            }
            const unsigned long long stops = __ballot(r < 16u);
            if (stops) {
                const uint32_t first = (uint32_t)__ffsll((long long)stops) - 1u;
                const uint64_t t = t0 + 16u * first + (uint32_t)__shfl((int)r, (int)first);
                return t < limit ? t : limit;
            }
        }
        return limit;
    }
};

__device__ inline bool is_gap(uint32_t run) { return (run & 15u) == DCN_ALN_I || (run & 15u) == DCN_ALN_D; }

__global__ __launch_bounds__(LA_THREADS) void left_align_kernel(dcn_left_align_args a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (LA_THREADS / 64);
    unsigned long long rows = 0, shifted = 0, passed = 0, merged = 0; // of this wave's rows (the same in every lane)
    for (uint64_t w = (uint64_t)blockIdx.x * (LA_THREADS / 64) + threadIdx.x / 64; w < a.n_work; w += waves) {
        const dcn_align_work wk = a.work[w];
        const uint32_t count = a.n_ops[wk.row];
        const uint32_t bound = (uint32_t)dcn_aln_ops_bound(wk.d);
        if (count == 0 || count > bound) continue; // (count <= bound always: the traceback's promise)
        const uint32_t *const in = a.slots + (wk.slot_end - count);
        bool gap = false;
        for (uint32_t c0 = 0; c0 < count && !gap; c0 += 64) gap = __ballot(c0 + lane < count && is_gap(in[c0 + lane])) != 0;
        if (!gap) continue;
        const dcn_verify_item it = a.items[wk.row];
        const dcn_wf_side S = {a.s_packed, a.s_invmask, it.s_origin, it.flags & 1u};
        const dcn_wf_side T = {a.t_packed, a.t_invmask, it.t_origin, 0u};
        uint32_t *const lo = a.scratch + (wk.slot_end - bound);
        dcn_la_row row = dcn_la_begin(lo, bound, S, T);
        for (uint32_t c0 = 0; c0 < count; c0 += 64) {
            const uint32_t here = min(64u, count - c0);
            const uint32_t mine = lane < here ? in[c0 + lane] : 0u;
            for (uint32_t q = 0; q < here; ++q) dcn_la_feed<la_wave>(row, (uint32_t)__shfl((int)mine, (int)q));
        }
        const uint32_t n = dcn_la_end<la_wave>(row);
        if (n == 0) continue; // no gap took a step: the row stays as the traceback left it
        __threadfence();      // lane 0's runs are in memory before the other lanes read them
        uint32_t *const to = a.slots + (wk.slot_end - n); // (n <= bound: dcn_la_end)
        for (uint32_t q = lane; q < n; q += 64) to[q] = __hip_atomic_load(lo + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 0) a.n_ops[wk.row] = n;
        rows += 1;
        shifted += row.shifted;
        passed += row.passed;
        merged += row.merged;
    }
    if (lane == 0 && rows != 0) { // (a changed row has a shifted gap and a passed column)
        atomicAdd(a.totals, rows);
        atomicAdd(a.totals + 1, shifted);
        atomicAdd(a.totals + 2, passed);
        if (merged != 0) atomicAdd(a.totals + 3, merged);
    }
}

} // namespace

int dcn_launch_left_align(const dcn_left_align_args &args, hipStream_t stream) {
    if (args.n_work == 0) return DCN_OK;
    const uint64_t per_block = LA_THREADS / 64;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((args.n_work + per_block - 1) / per_block, (uint64_t)dcn_cu_count() * 32);
    hipLaunchKernelGGL(left_align_kernel, dim3(blocks), dim3(LA_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}
