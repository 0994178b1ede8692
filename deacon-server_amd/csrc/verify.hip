// verify.hip -- the Levenshtein distance of a placement's two extents, thresholded (THE DEFINITION OF A VERIFIED PLACEMENT,
// include/deacon_hip.h).  One wave per row, a wavefront edit distance: F_s[k], its three sources, the cut to the rectangle
// and the run over EQUAL bases are dcn_wavefront.h's (dcn_wf_diagonal, which also says why no position goes negative).
// d is the first s with F_s[n - m] == m.  A path of cost <= E never leaves the diagonals [-E, +E], so stopping at s = E is
// exact: every d <= E is found, everything else is OVER.
// The previous and the current wavefront live in LDS, 2 x lds_stride words; lanes stride over the diagonals of a score
// (E <= 31: one pass per score).  Both streams have readable words in front: the plain load.
#include "dcn_verify.h"
#include "dcn_wavefront.h"

namespace {

__global__ __launch_bounds__(64) void verify_kernel(dcn_verify_args a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int64_t lane = threadIdx.x;
    for (uint64_t row = blockIdx.x; row < a.n_rows; row += gridDim.x) {
        const dcn_verify_item it = a.items[row];
        uint32_t result = DCN_VERIFY_UNPLACED;
        if (!(it.flags & 2u)) {
            const int64_t m = it.m, n = it.n, E = it.E, k_end = n - m;
            result = DCN_VERIFY_OVER;
            // (every condition down to the lanes' own diagonals is the same for the whole wave: the barriers are met by all)
            if (k_end <= E && -k_end <= E && 2 * E + 1 <= (int64_t)a.lds_stride) {
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
                        const int64_t i = dcn_wf_diagonal<dcn_wf_plain>(prev, E, s, k, m, n, S, T);
                        cur[k + E] = (uint32_t)i;
                        if (k == k_end && i >= m) found = true;
                    }
                    if (__any(found)) {
                        result = (uint32_t)s;
                        break;
                    }
                    __syncthreads();
                    uint32_t *const t = prev;
                    prev = cur;
                    cur = t;
                }
            }
        }
        if (lane == 0) a.out[row] = result;
    }
}

} // namespace

int dcn_launch_verify(const dcn_verify_args &args, hipStream_t stream) {
    if (args.n_rows == 0) return DCN_OK;
    // two wavefront arrays; 16 KB at DCN_VERIFY_MAX_EDITS, a few hundred bytes for short reads
    const dcn_wave_grid g = dcn_wave_grid_for(args.n_rows, 2, args.lds_stride);
    hipLaunchKernelGGL(verify_kernel, dim3(g.blocks), dim3(64), g.lds_bytes, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}
