// extend.hip -- the extension of a placement over one flank of its read (THE DEFINITION OF AN EXTENDED PLACEMENT,
// include/deacon_hip.h): the wavefront of dcn_wavefront.h (dcn_wf_diagonal, the guarded load: the store has no word in front
// of base 0) over the flank's two sequences U and V, which both begin at the placement's edge, with the best candidate of
// rule X5 tracked over the scores.  Value, order, stop and cap are dcn_extend.h's, shared with the host.
//   Shape: 16 lanes per flank, four flanks per wave, one wave per workgroup; items 4 q .. 4 q + 3 are both flanks of two
//   consecutive rows.  Most flanks are 10-20 bases and end at score 0 or 1 with one to three diagonals, so a wave per
//   flank would leave 61 lanes idle; 16 lanes cover every score up to 7 in one pass, and at the default penalty a flank
//   of f bases is never run further than (2 f + end_bonus) / 5.  The lanes of a flank stride over the diagonals of a score
//   beyond that.  The four flanks of a wave step through the scores together: a flank that is finished idles until the
//   last of the four is, which for two flanks of one row and its neighbour is a score or two.
//   Each flank has its own two wavefront arrays in LDS (8 x lds_stride words per workgroup, 64 KB at the largest cap).
//   The best candidate of a score is reduced over the flank's 16 lanes with shuffles; every lane of the flank then holds
//   the same best, so the stop of dcn_ext_done is uniform over the flank and the barriers are met by the whole wave.
#include "dcn_verify.h"
#include "dcn_extend.h"

namespace {

constexpr uint32_t FLANK_LANES = 16, WAVE_FLANKS = 64 / FLANK_LANES;

__global__ __launch_bounds__(64) void extend_kernel(dcn_extend_args a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t group = threadIdx.x / FLANK_LANES, lane = threadIdx.x % FLANK_LANES;
    uint32_t *const mine = lds + (size_t)group * 2 * a.lds_stride;
    const int64_t penalty = a.penalty, end_bonus = a.end_bonus;
    for (uint64_t t0 = (uint64_t)blockIdx.x * WAVE_FLANKS; t0 < a.n_items; t0 += (uint64_t)gridDim.x * WAVE_FLANKS) {
        const uint64_t t = t0 + group;
        dcn_extend_item it = {};
        bool active = false;
        if (t < a.n_items) {
            it = a.items[t];
            // (a cap that the arrays do not hold is the host's error: such a flank stays at (0, 0) and nothing is read)
            active = !(it.flags & 4u) && 2 * (uint64_t)it.cap + 1 <= a.lds_stride;
            if (!active && lane == 0) a.out[t] = dcn_extend_result{0u, 0u, 0u, 0u};
        }
        const int64_t f = it.f, g = it.g, cap = it.cap;
        const dcn_wf_side U = {a.s_packed, a.s_invmask, it.u_origin, it.flags & 1u};
        const dcn_wf_side V = {a.t_packed, a.t_invmask, it.v_origin, (it.flags >> 1) & 1u};
        uint32_t *prev = mine, *cur = mine + a.lds_stride;
        dcn_ext_best best = {INT64_MIN, 0, 0, 0};
        __syncthreads(); // the flanks before these have been read to their end
        for (int64_t s = 0;; ++s) {
            if (active) {
                const int64_t lo = dcn_wf_max(-s, -f), hi = dcn_wf_min(s, g);
                long long v_s = INT64_MIN;
                unsigned i_s = 0;
                int k_s = 0;
                for (int64_t k0 = lo; k0 <= hi; k0 += FLANK_LANES) {
                    const int64_t k = k0 + lane;
                    if (k > hi) continue;
                    const int64_t i = dcn_wf_diagonal<dcn_wf_guarded>(prev, cap, s, k, f, g, U, V);
                    cur[k + cap] = (uint32_t)i;
                    const int64_t v = dcn_ext_value(i, k, s, f, penalty, end_bonus);
                    if (dcn_ext_better(v, i, v_s, i_s)) v_s = v, i_s = (unsigned)i, k_s = (int)k;
                }
                // the best of this score over the flank's lanes (a lane without a diagonal holds INT64_MIN)
                for (uint32_t d = FLANK_LANES / 2; d >= 1; d >>= 1) {
                    const long long v_o = __shfl_xor(v_s, (int)d, (int)FLANK_LANES);
                    const unsigned i_o = __shfl_xor(i_s, (int)d, (int)FLANK_LANES);
                    const int k_o = __shfl_xor(k_s, (int)d, (int)FLANK_LANES);
                    if (dcn_ext_better(v_o, i_o, v_s, i_s)) v_s = v_o, i_s = i_o, k_s = k_o;
                }
                if (v_s > best.value) best = {v_s, s, (int64_t)i_s, (int64_t)k_s}; // (an equal value at a larger cost loses)
                if (s >= cap || dcn_ext_done(s, f, penalty, end_bonus, best.value)) {
                    active = false;
                    if (lane == 0) a.out[t] = dcn_extend_result{(uint32_t)best.i, (uint32_t)(best.i + best.k), (uint32_t)best.s, 0u};
                }
            }
            if (!__any(active)) break; // (one wave per workgroup: the same for every lane that meets the barrier)
            __syncthreads();
            uint32_t *const x = prev;
            prev = cur;
            cur = x;
        }
    }
}

} // namespace

int dcn_launch_extend(const dcn_extend_args &args, hipStream_t stream) {
    if (args.n_items == 0) return DCN_OK;
    // two wavefront arrays per flank of the wave; 64 KB at DCN_VERIFY_MAX_EDITS, a few hundred bytes for short reads
    const dcn_wave_grid g = dcn_wave_grid_for((args.n_items + WAVE_FLANKS - 1) / WAVE_FLANKS, 2 * WAVE_FLANKS, args.lds_stride);
    hipLaunchKernelGGL(extend_kernel, dim3(g.blocks), dim3(64), g.lds_bytes, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}
