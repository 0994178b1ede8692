// verify.hip -- the Levenshtein distance of a placement's two extents, thresholded (THE DEFINITION OF A VERIFIED PLACEMENT,
// include/deacon_hip.h).  One wave per row, a wavefront edit distance: F_s[k] = the furthest base i of S that a path of
// cost <= s reaches on diagonal k = j - i (j: the base of T).  F_s[k] comes from F_{s-1}[k] + 1 (substitution),
// F_{s-1}[k - 1] (a base of T alone) and F_{s-1}[k + 1] + 1 (a base of S alone), cut to the rectangle, then runs on
// while the bases are EQUAL.  d is the first s with F_s[n - m] == m.  A path of cost <= E never leaves the diagonals
// [-E, +E], so stopping at s = E is exact: every d <= E is found, everything else is OVER.
//   Along a diagonal the distance never falls, so every point in front of a reached one is reached at no more cost: the
//   cut to min(m, n - k) is exact, and within max(-s, -m) <= k <= min(s, n) some source is always in range (k itself for
//   |k| < s, k - 1 for k = s, k + 1 for k = -s), which leaves i >= max(0, -k): no position is ever negative.
// The previous and the current wavefront live in LDS, 2 x lds_stride words; lanes stride over the diagonals of a score
// (E <= 31: one pass per score).  Bases are compared 16 at a time by dcn_verify_words.h.
#include "dcn_verify.h"
#include "dcn_verify_words.h"

#include <algorithm>

namespace {

__device__ inline int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ inline int64_t imax(int64_t a, int64_t b) { return a > b ? a : b; }

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
                const dcn_vfy_side S = {a.s_packed, a.s_invmask, it.s_origin, it.flags & 1u};
                const dcn_vfy_side T = {a.t_packed, a.t_invmask, it.t_origin, 0u};
                uint32_t *prev = lds, *cur = lds + a.lds_stride;
                __syncthreads(); // the row before this one has been read to its end
                for (int64_t s = 0; s <= E; ++s) {
                    const int64_t lo = imax(-s, -m), hi = imin(s, n);
                    const int64_t plo = imax(1 - s, -m), phi = imin(s - 1, n); // the diagonals of score s - 1
                    bool found = false;
                    for (int64_t k0 = lo; k0 <= hi; k0 += 64) {
                        const int64_t k = k0 + lane;
                        if (k > hi) continue;
                        int64_t i = 0;
                        if (s > 0) {
                            i = -1;
                            if (k >= plo && k <= phi) i = (int64_t)prev[k + E] + 1;
                            if (k - 1 >= plo && k - 1 <= phi) i = imax(i, (int64_t)prev[k - 1 + E]);
                            if (k + 1 >= plo && k + 1 <= phi) i = imax(i, (int64_t)prev[k + 1 + E] + 1);
                            i = imin(i, imin(m, n - k));
                        }
                        const int64_t j = i + k;
                        if (i >= 0 && j >= 0) { // (always: see above; a position that were not would read nothing)
                            const int64_t room = imin(m - i, n - j);
                            if (room > 0) i += (int64_t)dcn_vfy_match_run(S, i, T, j, (uint64_t)room);
                        }
                        cur[k + E] = (uint32_t)imax(i, (int64_t)0);
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
    const size_t lds_bytes = ((size_t)args.lds_stride * 2 * sizeof(uint32_t) + 15) / 16 * 16;
    const uint64_t resident = (uint64_t)dcn_cu_count() * 32; // one-wave workgroups: at most 32 per CU
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(args.n_rows, resident * 4);
    hipLaunchKernelGGL(verify_kernel, dim3(blocks), dim3(64), lds_bytes, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}
