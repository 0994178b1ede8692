// pileup.hip -- the per-base counts of aligned rows and the calls over them (THE DEFINITION OF A PILEUP and THE DEFINITION
// OF A QUALITY-AWARE PILEUP, include/deacon_hip.h; what the host shares is in dcn_pileup.h).
//   pileup_kernel        one wave per aligned row, over align's work list.  The row's runs in chunks of 64: lane r loads
//                        run r and its steps on S and T, a wave prefix sum gives each run its (i, j); then, run by run,
//                        the lanes stride over the run's bases, read S[i] (dcn_wavefront.h, with the strand flag) and
//                        add 1 with atomicAdd on uint32_t.  A row with n = 0 adds nothing.
//                        <true> (dcn_pileup_batch_qual) also loads the byte of S[i]'s quality from the staged qualities:
//                        the lanes of a run read consecutive bytes, ascending on a forward row and descending on a reverse
//                        one.  A base column under the threshold becomes N (rule Q3), and on a map that keeps sums a second
//                        atomicAdd adds the quality to the column's sum (rule Q4).  <false> is the kernel it was.
//                        <., true> (a map that keeps strand planes, rule S2) takes the planes behind the other arguments:
//                        on a reverse row a base counted in A, C, G or T adds 1 to the plane of its column as well, the
//                        lanes again to consecutive words.  `reverse` is the wave's, so a forward row branches round the
//                        add as it does round REV's: no memory operation more.  <., false> are the kernels they were.
//   pileup_call_kernel   one thread per position of a range: rule P6.  <false> writes the call characters and the
//                        workgroup's number of sites; <true>, behind the scan of those numbers, writes the sites compactly
//                        in ascending position.  Both passes decide in the same code.
// Integers only; the adds commute, so nothing depends on the grid, the lanes or the order of rows.
#include "dcn_dump_sweep.h"
#include "dcn_pileup.h"
#include "dcn_verify.h"
#include "dcn_wavefront.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr uint32_t PILE_THREADS = 256; // four waves, a row each

__device__ inline const dcn_pileup_args &rows_of(const dcn_pileup_args &a) { return a; }
__device__ inline const dcn_pileup_args &rows_of(const dcn_pileup_qual_args &a) { return a.rows; }

template <bool QUAL>
using pile_rows_t = std::conditional_t<QUAL, dcn_pileup_qual_args, dcn_pileup_args>;
template <bool QUAL, bool STRAND>
using pile_args_t = std::conditional_t<STRAND, dcn_pileup_strand_args<pile_rows_t<QUAL>>, pile_rows_t<QUAL>>;

template <bool QUAL>
__device__ inline const pile_rows_t<QUAL> &call_of(const pile_rows_t<QUAL> &a) { return a; }
template <bool QUAL>
__device__ inline const pile_rows_t<QUAL> &call_of(const dcn_pileup_strand_args<pile_rows_t<QUAL>> &a) { return a.rows; }

template <bool QUAL, bool STRAND>
__global__ __launch_bounds__(PILE_THREADS) void pileup_kernel(pile_args_t<QUAL, STRAND> all) {
    const pile_rows_t<QUAL> &args = call_of<QUAL>(all);
    const dcn_pileup_args &a = rows_of(args);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (PILE_THREADS / 64);
    for (uint64_t w = (uint64_t)blockIdx.x * (PILE_THREADS / 64) + threadIdx.x / 64; w < a.n_work; w += waves) {
        const dcn_align_work wk = a.work[w];
        const dcn_verify_item it = a.items[wk.row];
        const uint32_t count = a.n_ops[wk.row];
        if (it.n == 0 || count == 0) continue; // (the same for the whole wave)
        const uint32_t *const runs = a.cigar + a.cigar_offsets[wk.row];
        const dcn_wf_side S = {a.s_packed, a.s_invmask, it.s_origin, it.flags & 1u};
        const uint32_t reverse = it.flags & 1u, m = it.m, n = it.n;
        const uint64_t t0 = (uint64_t)it.t_origin;
        uint32_t *const counters = a.counters;
        const uint64_t bases = a.bases;
        const auto column_of = [&](uint32_t i) {
            if (i >= m) return DCN_PILE_N; // (never: the runs cover exactly m bases of S)
            uint32_t x, inv;
            dcn_wf_side16<dcn_wf_plain>(S, (int64_t)i, &x, &inv);
            return dcn_pile_column(x & 3u, inv & 1u);
        };
        const auto add = [&](uint32_t column, uint32_t j) {
            if (j < n) atomicAdd(counters + dcn_pile_index(column, t0 + j, bases), 1u); // (always: '=', X and D cover exactly n)
        };
        const auto quality_of = [&](uint32_t i) -> uint32_t { // rule Q2: the byte at the base's batch position
            if constexpr (QUAL) {
                if (i >= m) return 0u; // (never, as above: nothing outside the read interval is loaded)
                return dcn_pile_quality(args.quals[dcn_pile_qual_pos(it.s_origin, reverse, i)], args.qual_offset);
            } else {
                return 0u;
            }
        };
        const auto add_sum = [&](uint32_t column, uint32_t j, uint32_t q) { // rule Q4
            if constexpr (QUAL) {
                if (args.sums && j < n) atomicAdd(args.sums + dcn_pile_sum_index(column, t0 + j, bases), q);
            }
        };
        const auto add_strand = [&](uint32_t column, uint32_t j) { // rule S2 (the runs call it on a reverse row alone)
            if constexpr (STRAND) {
                if (j < n) atomicAdd(all.strands + dcn_pile_strand_index(column, t0 + j, bases), 1u);
            }
        };
        uint32_t i0 = 0, j0 = 0; // where the chunk begins
        for (uint32_t c0 = 0; c0 < count; c0 += 64) {
            const uint32_t here = min(64u, count - c0);
            const uint32_t run = lane < here ? runs[c0 + lane] : 0u;
            uint32_t si = dcn_pile_step_s(run), sj = dcn_pile_step_t(run); // -> inclusive sums over the lanes
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint32_t oi = __shfl_up(si, d), oj = __shfl_up(sj, d);
                if (lane >= d) si += oi, sj += oj;
            }
            const uint32_t my_i = i0 + si - dcn_pile_step_s(run), my_j = j0 + sj - dcn_pile_step_t(run);
            for (uint32_t r = 0; r < here; ++r) {
                if constexpr (QUAL && STRAND)
                    dcn_pile_run_qual(__shfl(run, r), __shfl(my_i, r), __shfl(my_j, r), reverse, args.min_base_qual, lane, 64u, column_of,
                                      quality_of, add, add_sum, add_strand);
                else if constexpr (QUAL)
                    dcn_pile_run_qual(__shfl(run, r), __shfl(my_i, r), __shfl(my_j, r), reverse, args.min_base_qual, lane, 64u, column_of,
                                      quality_of, add, add_sum);
                else if constexpr (STRAND)
                    dcn_pile_run(__shfl(run, r), __shfl(my_i, r), __shfl(my_j, r), reverse, lane, 64u, column_of, add, add_strand);
                else
                    dcn_pile_run(__shfl(run, r), __shfl(my_i, r), __shfl(my_j, r), reverse, lane, 64u, column_of, add);
            }
            i0 += __shfl(si, 63);
            j0 += __shfl(sj, 63);
        }
    }
}

constexpr uint32_t CALL_THREADS = 256;

template <bool WRITE>
__global__ __launch_bounds__(CALL_THREADS) void pileup_call_kernel(dcn_pileup_call_args a) {
    __shared__ uint32_t s_wave[CALL_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x / 64;
    const uint64_t q = (uint64_t)blockIdx.x * CALL_THREADS + threadIdx.x;
    uint32_t info = 0;
    if (q < a.n) {
        const uint64_t b = a.base0 + q;
        uint32_t counts[DCN_PILE_COLUMNS - 1];
#pragma unroll
        for (uint32_t c = 0; c < DCN_PILE_COLUMNS - 1; ++c) counts[c] = a.counters[dcn_pile_index(c, b, a.bases)];
        const uint32_t code = (a.t_packed[b >> 4] >> (2 * (b & 15))) & 3u, inv = (a.t_invmask[b >> 5] >> (b & 31)) & 1u;
        info = dcn_pile_call(counts, dcn_pile_column(code, inv), a.min_depth, a.min_permille);
        if (!WRITE) a.calls[q] = dcn_pile_call_char(info);
    }
    const bool site = (info & 0xFFu) != 0; // (a position past the range has info = 0)
    const unsigned long long sites = __ballot(site);
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(sites);
    __syncthreads();
    if (!WRITE) {
        if (threadIdx.x == 0) a.block_counts[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    } else if (site) {
        uint64_t at = a.block_offsets[blockIdx.x] + (uint64_t)__popcll(sites & ((1ull << lane) - 1ull));
        for (uint32_t v = 0; v < wave; ++v) at += s_wave[v];
        a.site_pos[at] = a.pos0 + q;
        a.site_info[at] = info;
    }
}

// the grid of every form of pileup_kernel
uint32_t pileup_blocks(uint64_t n_work) {
    const uint64_t per_block = PILE_THREADS / 64;
    return (uint32_t)std::min<uint64_t>((n_work + per_block - 1) / per_block, (uint64_t)dcn_cu_count() * 32);
}
} // namespace

int dcn_launch_pileup(const dcn_pileup_args &args, hipStream_t stream) {
    if (args.n_work == 0) return DCN_OK;
    hipLaunchKernelGGL((pileup_kernel<false, false>), dim3(pileup_blocks(args.n_work)), dim3(PILE_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_pileup_qual(const dcn_pileup_qual_args &args, hipStream_t stream) {
    if (args.rows.n_work == 0) return DCN_OK;
    hipLaunchKernelGGL((pileup_kernel<true, false>), dim3(pileup_blocks(args.rows.n_work)), dim3(PILE_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_pileup_strand(const dcn_pileup_args &args, uint32_t *strands, hipStream_t stream) {
    if (args.n_work == 0) return DCN_OK;
    const dcn_pileup_strand_args<dcn_pileup_args> all = {args, strands};
    hipLaunchKernelGGL((pileup_kernel<false, true>), dim3(pileup_blocks(args.n_work)), dim3(PILE_THREADS), 0, stream, all);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_pileup_qual_strand(const dcn_pileup_qual_args &args, uint32_t *strands, hipStream_t stream) {
    if (args.rows.n_work == 0) return DCN_OK;
    const dcn_pileup_strand_args<dcn_pileup_qual_args> all = {args, strands};
    hipLaunchKernelGGL((pileup_kernel<true, true>), dim3(pileup_blocks(args.rows.n_work)), dim3(PILE_THREADS), 0, stream, all);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

uint32_t dcn_pileup_call_blocks(uint64_t n) { return (uint32_t)((n + CALL_THREADS - 1) / CALL_THREADS); }

int dcn_launch_pileup_call(const dcn_pileup_call_args &args, bool write, hipStream_t stream) {
    if (args.n == 0) return DCN_OK;
    const uint32_t blocks = dcn_pileup_call_blocks(args.n);
    if (write) hipLaunchKernelGGL(pileup_call_kernel<true>, dim3(blocks), dim3(CALL_THREADS), 0, stream, args);
    else hipLaunchKernelGGL(pileup_call_kernel<false>, dim3(blocks), dim3(CALL_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}
