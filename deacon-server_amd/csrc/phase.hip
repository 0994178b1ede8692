// phase.hip -- the links between listed sites that aligned rows show, and the phase sets over them (THE DEFINITION OF A
// PHASE, include/deacon_hip_phase.h; what the host shares is in dcn_phase.h).
//   phase_link_kernel     one wave per aligned row, over align's work list, in the pileup kernel's grid and loop.  The wave
//                         searches the first site at or behind the row's interval (wave-uniform loads) and ends there when
//                         fewer than two sites lie in the interval: the row's runs are not read.  Otherwise the runs in
//                         chunks of 64 with the pileup kernel's prefix sums; the lanes take the chunk's sites, one each, in
//                         groups of 64: a lane finds its run among the chunk's 64 inclusive sums on T (six __shfl steps),
//                         reads S[i] and, <true>, its quality byte, and forms its observation with the pileup's own column
//                         functions.  The neighbour's observation comes by __shfl_down; the observation of a group's last
//                         site is carried, wave-uniform, to the next group of the chunk or of the next chunk.  One
//                         atomicAdd without a result per defined pair, one per linking row on the call's two counters.
//   phase_decide_kernel   a thread per site: rule H5 over the four counters of link s.
//   phase_aggregate_kernel, phase_prefix_kernel, phase_apply_kernel
//                         rule H6 as a segmented inclusive scan over the sites (element and operator in dcn_phase.h): in the
//                         wave by __shfl_up, across the workgroup's waves in LDS, across workgroups in three passes: every
//                         workgroup's aggregate, one workgroup that turns the aggregates into the elements in front of each
//                         (any number of them: a thread takes a stretch), and the pass that writes the results.
// Integers only; the adds commute and the scan's order is fixed, so nothing depends on the grid, the lanes or the rows' order.
#include "../../include/deacon_hip_phase.h"
#include "dcn_dump_sweep.h"
#include "dcn_phase.h"
#include "dcn_pileup.h"
#include "dcn_verify.h"
#include "dcn_wavefront.h"

#include <algorithm>

namespace {

constexpr uint32_t LINK_THREADS = 256; // four waves, a row each (pileup_kernel's shape)

template <bool QUAL>
__global__ __launch_bounds__(LINK_THREADS) void phase_link_kernel(dcn_phase_link_args a) {
    const dcn_pileup_args &r = a.rows;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64); // (the row, and every load by it, is the wave's)
    const uint64_t waves = (uint64_t)gridDim.x * (LINK_THREADS / 64);
    const uint64_t n_sites = a.n_sites;
    for (uint64_t w = (uint64_t)blockIdx.x * (LINK_THREADS / 64) + wave; w < r.n_work; w += waves) {
        const dcn_align_work wk = r.work[w];
        const dcn_verify_item it = r.items[wk.row];
        const uint32_t count = r.n_ops[wk.row];
        if (it.n == 0 || count == 0) continue; // rule H2: a counted row
        const uint64_t t0 = (uint64_t)it.t_origin, t1 = t0 + it.n;
        uint64_t lo = 0, hi = n_sites; // the first site at or behind t0
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (a.site_base[mid] < t0) lo = mid + 1;
            else hi = mid;
        }
        if (lo + 1 >= n_sites || a.site_base[lo + 1] >= t1) continue; // fewer than two sites in [t0, t1): no pair
        const uint32_t *const runs = r.cigar + r.cigar_offsets[wk.row];
        const dcn_wf_side S = {r.s_packed, r.s_invmask, it.s_origin, it.flags & 1u};
        const uint32_t reverse = it.flags & 1u, m = it.m, n = it.n;
        uint64_t cur = lo;               // the next site of the row
        uint32_t carry = DCN_PHASE_NONE; // the observation at site cur - 1 (looked at when cur > lo)
        uint32_t adds = 0;
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
            const uint32_t incl = j0 + sj;                         // the first base of T behind run `lane`
            const uint32_t j_end = min(j0 + __shfl(sj, 63), n);    // ... and behind the chunk (never past the interval)
            for (;;) { // the chunk's sites, 64 at a time
                const uint64_t idx = cur + lane;
                const uint64_t base = idx < n_sites ? a.site_base[idx] : ~0ull;
                const bool valid = base < t0 + j_end; // (base >= t0: idx >= lo.  The sites ascend: the valid lanes are the first ones)
                const unsigned long long mask = __ballot(valid);
                if (!mask) break;
                const uint32_t cnt = (uint32_t)__popcll(mask);
                const uint32_t rel = valid ? (uint32_t)(base - t0) : j0;
                uint32_t p = 0; // the runs of the chunk that end at or in front of rel: the index of the run that holds it
                for (uint32_t step = 32; step; step >>= 1) {
                    const uint32_t v = __shfl(incl, (int)(p + step - 1));
                    if (v <= rel) p += step;
                }
                const uint32_t run_p = __shfl(run, (int)p), i_p = __shfl(my_i, (int)p), j_p = __shfl(my_j, (int)p);
                uint32_t obs = DCN_PHASE_NONE;
                const uint32_t op = run_p & 15u;
                if (valid && op != DCN_ALN_D && op != DCN_ALN_I) { // (an I run holds no base of T: never found)
                    const uint32_t i = i_p + (rel - j_p);
                    if (i < m) { // (always: the runs cover exactly m bases of S)
                        uint32_t x, inv;
                        dcn_wf_side16<dcn_wf_plain>(S, (int64_t)i, &x, &inv);
                        uint32_t column = dcn_pile_column(x & 3u, inv & 1u);
                        if constexpr (QUAL) {
                            const uint32_t q = dcn_pile_quality(a.quals[dcn_pile_qual_pos(it.s_origin, reverse, i)], a.qual_offset);
                            column = dcn_pile_qual_column(column, q, a.min_base_qual);
                        }
                        obs = dcn_phase_observation(column, a.site_alleles[idx]);
                    }
                }
                const uint32_t nxt = __shfl_down(obs, 1);
                const bool pair = lane + 1 < cnt && obs < DCN_PHASE_NONE && nxt < DCN_PHASE_NONE;
                if (pair) atomicAdd(a.links + 4 * idx + dcn_phase_counter(obs, nxt), 1u);
                const bool seam = lane == 0 && cur > lo && carry < DCN_PHASE_NONE && obs < DCN_PHASE_NONE;
                if (seam) atomicAdd(a.links + 4 * (cur - 1) + dcn_phase_counter(carry, obs), 1u);
                adds += (uint32_t)__popcll(__ballot(pair)) + (uint32_t)__popcll(__ballot(seam));
                carry = __shfl(obs, (int)(cnt - 1));
                cur += cnt;
                if (cnt < 64) break; // the next site lies behind the chunk
            }
            if (cur >= n_sites || a.site_base[cur] >= t1) break; // the row's last site is behind us: its other runs are not read
            i0 += __shfl(si, 63);
            j0 += __shfl(sj, 63);
        }
        if (adds && lane < 2) atomicAdd(a.call + lane, lane ? (unsigned long long)adds : 1ull);
    }
}

// the grid of phase_link_kernel: pileup_kernel's
uint32_t link_blocks(uint64_t n_work) {
    const uint64_t per_block = LINK_THREADS / 64;
    return (uint32_t)std::min<uint64_t>((n_work + per_block - 1) / per_block, (uint64_t)dcn_cu_count() * 32);
}

// ---- rules H5 - H7 ----------------------------------------------------------------------------------------------------
constexpr uint32_t SOLVE_THREADS = DCN_PHASE_SCAN_BLOCK;
constexpr uint32_t SOLVE_WAVES = SOLVE_THREADS / 64;

__global__ __launch_bounds__(SOLVE_THREADS) void phase_decide_kernel(dcn_phase_solve_args a) {
    const uint64_t s = (uint64_t)blockIdx.x * SOLVE_THREADS + threadIdx.x;
    if (s >= a.n_sites) return;
    uint32_t dec = 0;
    if (a.site_alleles[s] & DCN_PHASE_LINK_BIT) {
        const uint4 v = *reinterpret_cast<const uint4 *>(a.links + 4 * s);
        const uint32_t n[4] = {v.x, v.y, v.z, v.w};
        dec = dcn_phase_decide(n, a.min_reads, a.max_minor_permille);
    }
    a.decisions[s] = (uint8_t)dec;
}

__device__ inline dcn_phase_elem elem_shfl_up(const dcn_phase_elem &v, uint32_t d) {
    dcn_phase_elem o;
    o.heads = __shfl_up(v.heads, d);
    o.x = __shfl_up(v.x, d);
    o.last = ((uint64_t)__shfl_up((uint32_t)(v.last >> 32), d) << 32) | __shfl_up((uint32_t)v.last, d);
    return o;
}

// the element of site s of the list; the identity behind the list's end
__device__ inline dcn_phase_elem elem_of(const dcn_phase_solve_args &a, uint64_t s) {
    if (s >= a.n_sites) return dcn_phase_identity();
    return dcn_phase_site_elem(s, s > 0 ? a.decisions[s - 1] : 0u);
}

// inclusive scan of one element per thread over the workgroup
__device__ inline dcn_phase_elem scan_block(dcn_phase_elem v, dcn_phase_elem *s_wave) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x / 64;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const dcn_phase_elem o = elem_shfl_up(v, d);
        if (lane >= d) v = dcn_phase_combine(o, v);
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    dcn_phase_elem before = dcn_phase_identity();
#pragma unroll
    for (uint32_t q = 0; q + 1 < SOLVE_WAVES; ++q)
        if (q < wave) before = dcn_phase_combine(before, s_wave[q]);
    return dcn_phase_combine(before, v);
}

__global__ __launch_bounds__(SOLVE_THREADS) void phase_aggregate_kernel(dcn_phase_solve_args a) {
    __shared__ dcn_phase_elem s_wave[SOLVE_WAVES];
    const uint64_t s = (uint64_t)blockIdx.x * SOLVE_THREADS + threadIdx.x;
    const dcn_phase_elem incl = scan_block(elem_of(a, s), s_wave);
    if (threadIdx.x == SOLVE_THREADS - 1) a.aggregates[blockIdx.x] = incl;
}

// one workgroup: aggregates[] -> for every workgroup the element of all sites in front of it (offsets_scan_blocks_kernel's shape)
__global__ __launch_bounds__(SOLVE_THREADS) void phase_prefix_kernel(dcn_phase_elem *aggregates, uint64_t n_blocks) {
    __shared__ dcn_phase_elem s_part[SOLVE_THREADS];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (n_blocks + SOLVE_THREADS - 1) / SOLVE_THREADS;
    const uint64_t b0 = min((uint64_t)tid * per, n_blocks), b1 = min(b0 + per, n_blocks);
    dcn_phase_elem mine = dcn_phase_identity();
    for (uint64_t b = b0; b < b1; ++b) mine = dcn_phase_combine(mine, aggregates[b]);
    s_part[tid] = mine;
    __syncthreads();
    dcn_phase_elem before = dcn_phase_identity();
    for (uint32_t q = 0; q < tid; ++q) before = dcn_phase_combine(before, s_part[q]);
    for (uint64_t b = b0; b < b1; ++b) {
        const dcn_phase_elem v = aggregates[b];
        aggregates[b] = before;
        before = dcn_phase_combine(before, v);
    }
}

__global__ __launch_bounds__(SOLVE_THREADS) void phase_apply_kernel(dcn_phase_solve_args a) {
    __shared__ dcn_phase_elem s_wave[SOLVE_WAVES];
    const uint64_t s = (uint64_t)blockIdx.x * SOLVE_THREADS + threadIdx.x;
    const dcn_phase_elem mine = elem_of(a, s);
    const dcn_phase_elem incl = dcn_phase_combine(a.aggregates[blockIdx.x], scan_block(mine, s_wave));
    if (s >= a.n_sites) return;
    dcn_phase_result out;
    out.set_pos = a.site_pos[incl.last]; // (site 0 is a head: incl.heads >= 1 and incl.last <= s)
    const bool link = a.site_alleles[s] & DCN_PHASE_LINK_BIT;
    const uint4 v = link ? *reinterpret_cast<const uint4 *>(a.links + 4 * s) : make_uint4(0, 0, 0, 0);
    out.link[0] = v.x, out.link[1] = v.y, out.link[2] = v.z, out.link[3] = v.w;
    out.set_index = incl.heads - 1;
    out.hap = (uint8_t)incl.x;
    out.flags = (uint8_t)((mine.heads ? DCN_PHASE_HEAD : 0u) | ((a.decisions[s] & DCN_PHASE_DEC_JOINED) ? DCN_PHASE_JOINED : 0u));
    out.reserved[0] = out.reserved[1] = 0;
    static_cast<dcn_phase_result *>(a.results)[s] = out;
}

} // namespace

int dcn_launch_phase_link(const dcn_phase_link_args &args, bool qual, hipStream_t stream) {
    if (args.rows.n_work == 0 || args.n_sites < 2) return DCN_OK; // (a list of one site has no link)
    const uint32_t blocks = link_blocks(args.rows.n_work);
    if (qual) hipLaunchKernelGGL(phase_link_kernel<true>, dim3(blocks), dim3(LINK_THREADS), 0, stream, args);
    else hipLaunchKernelGGL(phase_link_kernel<false>, dim3(blocks), dim3(LINK_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

uint64_t dcn_phase_solve_blocks(uint64_t n_sites) { return (n_sites + SOLVE_THREADS - 1) / SOLVE_THREADS; }

int dcn_launch_phase_solve(const dcn_phase_solve_args &args, hipStream_t stream) {
    if (args.n_sites == 0) return DCN_OK;
    const uint64_t blocks = dcn_phase_solve_blocks(args.n_sites);
    hipLaunchKernelGGL(phase_decide_kernel, dim3((uint32_t)blocks), dim3(SOLVE_THREADS), 0, stream, args);
    hipLaunchKernelGGL(phase_aggregate_kernel, dim3((uint32_t)blocks), dim3(SOLVE_THREADS), 0, stream, args);
    hipLaunchKernelGGL(phase_prefix_kernel, dim3(1), dim3(SOLVE_THREADS), 0, stream, args.aggregates, blocks);
    hipLaunchKernelGGL(phase_apply_kernel, dim3((uint32_t)blocks), dim3(SOLVE_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}
