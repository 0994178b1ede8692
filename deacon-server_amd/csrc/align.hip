// align.hip -- the alignment of a verified placement (THE DEFINITION OF AN ALIGNED PLACEMENT, include/deacon_hip.h).
//   align_kernel         one wave per aligned row.  The wavefront of dcn_wavefront.h (dcn_wf_diagonal, the plain load) with
//                        E = the row's distance d (known from verify_kernel), prev / cur in LDS; every wavefront is also stored to the
//                        row's trace in global memory (dcn_align.h: F_s[k] at s * s + k + s, (d + 1)^2 words).  Behind a
//                        fence lane 0 walks back over the trace (dcn_aln_traceback, d dependent steps, no base read) and
//                        writes the runs from the end of the row's slot downwards, then the row's n_ops.
//   align_gather_kernel  a wave per aligned row: its runs from the tail of its slot to cigar[cigar_offsets[row] ..].
// The wavefront runs twice per aligned row (once in verify_kernel): keeping the first pass's wavefronts would size the
// trace by E instead of d.  Integers only; nothing depends on lanes, the LDS size or the groups the host cuts.
#include "dcn_align.h"
#include "dcn_verify.h"
#include "dcn_wavefront.h"

#include <algorithm>

namespace {

__global__ __launch_bounds__(64) void align_kernel(dcn_align_args a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int64_t lane = threadIdx.x;
    for (uint64_t w = a.w0 + blockIdx.x; w < a.w1; w += gridDim.x) {
        const dcn_align_work wk = a.work[w];
        const dcn_verify_item it = a.items[wk.row];
        const int64_t m = it.m, n = it.n, E = wk.d, k_end = n - m;
        uint32_t *const trace = a.trace + (wk.trace_base - a.trace_origin);
        // (every condition down to the lanes' own diagonals is the same for the whole wave: the barriers are met by all)
        bool reached = E == 0; // (d = 0: the alignment is m '=', no wavefront is read)
        if (E > 0 && 2 * E + 1 <= (int64_t)a.lds_stride) {
            const dcn_wf_side S = {a.s_packed, a.s_invmask, it.s_origin, it.flags & 1u};
            const dcn_wf_side T = {a.t_packed, a.t_invmask, it.t_origin, 0u};
            uint32_t *prev = lds, *cur = lds + a.lds_stride;
            __syncthreads(); // the row before this one has been read to its end
            for (int64_t s = 0; s <= E; ++s) {
                const int64_t lo = dcn_wf_max(-s, -m), hi = dcn_wf_min(s, n);
                bool found = false;
                for (int64_t k0 = lo; k0 <= hi; k0 += 64) {
                    const int64_t k = k0 + lane;
                    if (k > hi) continue;
                    const uint32_t f = (uint32_t)dcn_wf_diagonal<dcn_wf_plain>(prev, E, s, k, m, n, S, T);
                    cur[k + E] = f;
                    trace[dcn_aln_trace_at(s, k)] = f; // (-s <= k <= s: within the (d + 1)^2 words)
                    if (k == k_end && f >= it.m) found = true;
                }
                if (__any(found)) {
                    reached = s == E; // (the distance is d: verify_kernel found it by the same wavefront)
                    break;
                }
                __syncthreads();
                uint32_t *const t = prev;
                prev = cur;
                cur = t;
            }
            __threadfence(); // the trace is in memory before lane 0 reads it back
            __syncthreads();
        }
        if (lane == 0) a.n_ops[wk.row] = reached ? dcn_aln_traceback(trace, m, n, E, a.slots + wk.slot_end) : 0u;
    }
}

constexpr uint32_t GATHER_THREADS = 256;

__global__ __launch_bounds__(GATHER_THREADS) void align_gather_kernel(dcn_align_gather_args a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (GATHER_THREADS / 64);
    for (uint64_t w = (uint64_t)blockIdx.x * (GATHER_THREADS / 64) + threadIdx.x / 64; w < a.n_work; w += waves) {
        const dcn_align_work wk = a.work[w];
        const uint32_t count = a.n_ops[wk.row];
        const uint32_t *const from = a.slots + (wk.slot_end - count);
        uint32_t *const to = a.cigar + a.cigar_offsets[wk.row];
        for (uint32_t q = lane; q < count; q += 64) to[q] = from[q];
    }
}

} // namespace

int dcn_launch_align(const dcn_align_args &args, hipStream_t stream) {
    if (args.w1 <= args.w0) return DCN_OK;
    const dcn_wave_grid g = dcn_wave_grid_for(args.w1 - args.w0, 2, args.lds_stride);
    hipLaunchKernelGGL(align_kernel, dim3(g.blocks), dim3(64), g.lds_bytes, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_align_gather(const dcn_align_gather_args &args, hipStream_t stream) {
    if (args.n_work == 0) return DCN_OK;
    const uint64_t per_block = GATHER_THREADS / 64;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((args.n_work + per_block - 1) / per_block, (uint64_t)dcn_cu_count() * 32);
    hipLaunchKernelGGL(align_gather_kernel, dim3(blocks), dim3(GATHER_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}
