// indels.hip -- the kernels of a deletion ledger and of an indel genotype (THE DEFINITION OF A DELETION LEDGER and THE
// DEFINITION OF AN INDEL GENOTYPE, include/deacon_hip.h; what the host shares is in dcn_indels.h).
//   Append, behind pileup_kernel on the context's stream (one wave per aligned row, ins_walk_kernel's plan: the runs in
//   chunks of 64, a wave prefix sum for every run's j):
//     del_walk_kernel<false>  per row the number of its D runs; a wave adds what its rows had, and the sum of the runs'
//                             lengths, to the call's two totals once, and only when there was something.
//     del_walk_kernel<true>   behind the scan: every D run's event at its row's offset.  No bases are moved, so the lane
//                             that holds a D run writes its event itself: there is no loop over the runs of a chunk.
//   Fetch and genotype, on the null stream, over a range of one record:
//     del_plane_kernel        one thread per event of the ledger: an atomic add to STARTS of its position in the range (no
//                             pileup column holds STARTS); the plane's scan gives every position a bucket.
//     del_scatter_kernel      one thread per event: into its position's bucket, by a per-position cursor.
//     del_gather_kernel       fetch: the bucketed events as dcn_deletion (the host sorts each bucket by rule R4).
//     del_winner_kernel       genotype: a wave per 64 positions, for each with STARTS > 0 the lanes stride over the bucket,
//                             each counts the events as long as its own, a wave reduction picks the winner (R5).  Quadratic
//                             in the events of one position.
//     indel_flags_kernel      the insertion side's flag, INS > 0, from the INS plane of the range.
//     indel_site_kernel       one thread per position: the six counters and the two candidates (a, e), rules I1 - I5 of
//                             dcn_indels.h, 0, 1 or 2 sites.  <false> counts the sites per workgroup and adds the inserted
//                             bases of its sites to a total; <true>, behind the scan of those counts, decides again and
//                             writes the sites in I6's order.
//     indel_bases_kernel      behind the scan of the sites' inserted lengths: a wave per site sets bases_offset and copies
//                             an insertion's bases.
// Integers and bytes only.  Which slot of a bucket an event takes depends on the order of the atomic adds; nothing that is
// returned does (R5 is order-free, and fetch sorts).
#include "dcn_dump_sweep.h"
#include "dcn_indels.h"
#include "dcn_insertions.h"
#include "dcn_verify.h"

#include <algorithm>

static_assert(sizeof(dcn_deletion) == 16 && sizeof(dcn_indel_site) == 48, "ledger events and indel sites are ABI");
static_assert(DCN_DELETION_REVERSE == DCN_DEL_REVERSE && DCN_INDEL_DELETION == DCN_INDEL_SITE_DELETION && DCN_INDEL_FRONT == DCN_INDEL_SITE_FRONT,
              "the flags of the header and of dcn_indels.h");

namespace {

constexpr uint32_t DEL_THREADS = 256; // four waves

__device__ inline uint32_t wave_sum(uint32_t v) {
    for (uint32_t d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

template <bool WRITE>
__global__ __launch_bounds__(DEL_THREADS) void del_walk_kernel(dcn_del_append_args a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (DEL_THREADS / 64);
    unsigned long long sum_events = 0, sum_deleted = 0; // of this wave's rows (the same in every lane)
    for (uint64_t w = (uint64_t)blockIdx.x * (DEL_THREADS / 64) + threadIdx.x / 64; w < a.rows.n_work; w += waves) {
        const dcn_align_work wk = a.rows.work[w];
        const dcn_verify_item it = a.rows.items[wk.row];
        const uint32_t count = a.rows.n_ops[wk.row];
        if (it.n == 0 || count == 0) { // rule P2 (the same for the whole wave)
            if (!WRITE && lane == 0) a.row_events[w] = 0;
            continue;
        }
        const uint32_t *const runs = a.rows.cigar + a.rows.cigar_offsets[wk.row];
        if (!WRITE) {
            uint32_t ev = 0, nd = 0;
            for (uint32_t c0 = lane; c0 < count; c0 += 64) {
                const uint32_t run = runs[c0];
                ev += dcn_del_run_events(run);
                nd += dcn_del_run_events(run) ? run >> 4 : 0u; // (a row's T is shorter than 2^28 bases: no overflow)
            }
            ev = wave_sum(ev);
            nd = wave_sum(nd);
            if (lane == 0) a.row_events[w] = ev;
            sum_events += ev;
            sum_deleted += nd;
            continue;
        }
        if (a.row_events[w] == 0) continue;
        const uint32_t reverse = it.flags & 1u;
        const uint64_t t0 = (uint64_t)it.t_origin;
        // where the row's events go, and where they end: a run that would pass the end is not written
        uint64_t event_at = a.event0 + a.event_offsets[w];
        const uint64_t event_end = a.event0 + a.event_offsets[w + 1];
        uint32_t j0 = 0;
        for (uint32_t c0 = 0; c0 < count; c0 += 64) {
            const uint32_t here = min(64u, count - c0);
            const uint32_t run = lane < here ? runs[c0 + lane] : 0u;
            uint32_t sj = dcn_pile_step_t(run), se = dcn_del_run_events(run);
            for (uint32_t d = 1; d < 64; d <<= 1) { // -> inclusive sums over the lanes
                const uint32_t oj = __shfl_up(sj, d), oe = __shfl_up(se, d);
                if (lane >= d) sj += oj, se += oe;
            }
            const uint32_t my_j = j0 + sj - dcn_pile_step_t(run);
            const uint64_t my_e = event_at + se - dcn_del_run_events(run);
            if (dcn_del_run_events(run) != 0 && my_e < event_end) // (always: the counting pass walked the same runs)
                a.events[my_e] = dcn_del_event_of(run, my_j, reverse, t0);
            j0 += __shfl(sj, 63);
            event_at += __shfl(se, 63);
        }
    }
    if (!WRITE && lane == 0 && sum_events != 0) {
        atomicAdd(a.totals, sum_events);
        atomicAdd(a.totals + 1, sum_deleted);
    }
}

__global__ __launch_bounds__(DEL_THREADS) void del_plane_kernel(dcn_del_range_args a) {
    const uint64_t e = (uint64_t)blockIdx.x * DEL_THREADS + threadIdx.x;
    if (e >= a.n_events) return;
    const uint64_t base = a.events[e].base;
    if (base < a.base0 || base - a.base0 >= a.n) return; // rule: an event belongs to the range by its p alone
    atomicAdd(a.counts + (base - a.base0), 1u);
}

__global__ __launch_bounds__(DEL_THREADS) void del_scatter_kernel(dcn_del_range_args a) {
    const uint64_t e = (uint64_t)blockIdx.x * DEL_THREADS + threadIdx.x;
    if (e >= a.n_events) return;
    const uint64_t base = a.events[e].base;
    if (base < a.base0 || base - a.base0 >= a.n) return;
    const uint64_t q = base - a.base0;
    const uint32_t room = a.counts[q];
    const uint32_t k = atomicAdd(a.cursor + q, 1u);
    if (k < room) a.slots[a.bucket_offsets[q] + k] = e; // (always: the plane counted the same events)
}

__global__ __launch_bounds__(DEL_THREADS) void del_gather_kernel(dcn_del_range_args a) {
    const uint64_t s = (uint64_t)blockIdx.x * DEL_THREADS + threadIdx.x;
    if (s >= a.n_slots) return;
    const dcn_del_event e = a.events[a.slots[s]];
    dcn_deletion o;
    o.pos = a.pos0 + (e.base - a.base0);
    o.len = e.len;
    o.flags = e.flags;
    static_cast<dcn_deletion *>(a.out_events)[s] = o;
}

__global__ __launch_bounds__(DEL_THREADS) void del_winner_kernel(dcn_del_range_args a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (DEL_THREADS / 64), chunks = (a.n + 63) / 64;
    for (uint64_t ch = (uint64_t)blockIdx.x * (DEL_THREADS / 64) + threadIdx.x / 64; ch < chunks; ch += waves) {
        const uint64_t mine = ch * 64 + lane;
        unsigned long long todo = __ballot(mine < a.n && a.counts[mine] != 0);
        while (todo) { // (win_count and win_len are zero before: a position without an event stays so)
            const uint64_t q = ch * 64 + (uint64_t)__ffsll((long long)todo) - 1u;
            todo &= todo - 1ull;
            const uint64_t s0 = a.bucket_offsets[q];
            const uint32_t count = (uint32_t)(a.bucket_offsets[q + 1] - s0);
            uint32_t best_count = 0;
            uint32_t best_len = dcn_del_lane_winner(a.slots + s0, count, lane, 64u, a.events, &best_count);
            for (uint32_t d = 32; d > 0; d >>= 1) {
                const uint32_t other_len = __shfl_xor(best_len, d), other_count = __shfl_xor(best_count, d);
                if (other_count != 0 && (best_count == 0 || dcn_del_beats(other_count, other_len, best_count, best_len)))
                    best_len = other_len, best_count = other_count;
            }
            if (lane == 0) a.win_count[q] = best_count, a.win_len[q] = best_len;
        }
    }
}

__global__ __launch_bounds__(DEL_THREADS) void indel_flags_kernel(const uint32_t *counts, uint32_t *flags, uint64_t n) {
    const uint64_t q = (uint64_t)blockIdx.x * DEL_THREADS + threadIdx.x;
    if (q < n) flags[q] = counts[q] > 0 ? 1u : 0u;
}

// one candidate of a position: a = 0 when there is none
struct candidate {
    uint32_t a, e, len, flags;
    uint64_t event;
};

__device__ inline dcn_indel_prm params_of(const dcn_indel_site_args &a) {
    return {a.ploidy, a.min_depth, a.min_gq, a.min_qual, a.min_count, a.indel_centi, a.het_centi};
}

__device__ inline void write_site(const dcn_indel_site_args &a, uint64_t at, uint64_t q, uint32_t depth, const candidate &c,
                                  const dcn_indel_prm &prm) {
    uint8_t pl[3];
    const dcn_indel_result r = dcn_indel_decide(c.a, depth, prm, pl);
    dcn_indel_site s;
    s.pos = a.pos0 + q;
    s.bases_offset = 0; // (indel_bases_kernel)
    s.len = c.len;
    s.flags = c.flags;
    s.qual = r.qual;
    s.depth = depth;
    s.count = c.a;
    s.events = c.e;
    s.gt = (uint8_t)r.gt;
    s.gq = (uint8_t)r.gq;
    s.pl[0] = pl[0], s.pl[1] = pl[1], s.pl[2] = pl[2];
    s.reserved[0] = s.reserved[1] = s.reserved[2] = 0;
    static_cast<dcn_indel_site *>(a.sites)[at] = s;
    const bool del = (c.flags & DCN_INDEL_SITE_DELETION) != 0;
    a.site_lens[at] = del ? 0u : c.len;
    a.site_event[at] = del ? 0ull : c.event;
}

template <bool WRITE>
__global__ __launch_bounds__(DEL_THREADS) void indel_site_kernel(dcn_indel_site_args a) {
    __shared__ uint32_t s_wave[DEL_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x / 64;
    const uint64_t q = (uint64_t)blockIdx.x * DEL_THREADS + threadIdx.x;
    const dcn_indel_prm prm = params_of(a);
    candidate ins = {0, 0, 0, 0, 0}, del = {0, 0, 0, DCN_INDEL_SITE_DELETION, 0};
    uint32_t depth = 0;
    bool ins_site = false, del_site = false;
    if (q < a.n) {
        const uint64_t b = a.base0 + q;
#pragma unroll
        for (uint32_t c = 0; c <= DCN_PILE_DEL; ++c) depth += a.counters[dcn_pile_index(c, b, a.bases)]; // P4 (wraps as the counters do)
        if (a.ins_flags && a.ins_flags[q]) { // I1: L5's winner, e = INS(p)
            const uint64_t at = a.ins_offsets[q];
            ins.a = a.ins_count[at];
            ins.e = a.ins_events[at];
            ins.len = a.ins_len[at];
            ins.event = a.ins_event[at];
            ins.flags = a.ins_ledger[ins.event].flags & DCN_INS_FRONT ? DCN_INDEL_SITE_FRONT : 0u;
        }
        if (a.del_starts && a.del_starts[q]) { // I1: R5's winner, e = STARTS(p)
            del.a = a.del_count[q];
            del.e = a.del_starts[q];
            del.len = a.del_len[q];
        }
        uint8_t pl[3]; // (not looked at here)
        ins_site = ins.a != 0 && dcn_indel_candidate(ins.a, prm.min_count) && dcn_indel_decide(ins.a, depth, prm, pl).site;
        del_site = del.a != 0 && dcn_indel_candidate(del.a, prm.min_count) && dcn_indel_decide(del.a, depth, prm, pl).site;
    }
    // the sites of the lanes in front of this one in its wave, and of the waves in front of that
    const uint32_t mine = (ins_site ? 1u : 0u) + (del_site ? 1u : 0u);
    uint32_t incl = mine;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    if (!WRITE) {
        if (threadIdx.x == 0) a.block_counts[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        const uint32_t bases = wave_sum(ins_site ? ins.len : 0u);
        if (lane == 0 && bases != 0) atomicAdd(a.n_inserted, (unsigned long long)bases);
    } else if (mine) {
        uint64_t at = a.block_offsets[blockIdx.x] + (incl - mine);
        for (uint32_t v = 0; v < wave; ++v) at += s_wave[v];
        // I6: a front insertion, then the deletion, then an insertion behind
        if (ins_site && (ins.flags & DCN_INDEL_SITE_FRONT)) write_site(a, at++, q, depth, ins, prm);
        if (del_site) write_site(a, at++, q, depth, del, prm);
        if (ins_site && !(ins.flags & DCN_INDEL_SITE_FRONT)) write_site(a, at++, q, depth, ins, prm);
    }
}

__global__ __launch_bounds__(DEL_THREADS) void indel_bases_kernel(dcn_indel_site_args a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (DEL_THREADS / 64);
    dcn_indel_site *const sites = static_cast<dcn_indel_site *>(a.sites);
    for (uint64_t s = (uint64_t)blockIdx.x * (DEL_THREADS / 64) + threadIdx.x / 64; s < a.n_sites; s += waves) {
        const uint64_t at = a.site_offsets[s];
        const uint32_t len = (uint32_t)(a.site_offsets[s + 1] - at); // (0 for a deletion)
        if (lane == 0) sites[s].bases_offset = at;
        if (len == 0) continue;
        const uint64_t from = a.ins_ledger[a.site_event[s]].bases_offset;
        for (uint32_t k = lane; k < len; k += 64) a.out_bases[at + k] = a.ins_ledger_bases[from + k];
    }
}

// workgroups of a grid with one thread per item
uint32_t thread_blocks(uint64_t n) { return (uint32_t)((n + DEL_THREADS - 1) / DEL_THREADS); }
// ... and of one whose waves stride over n items
uint32_t wave_blocks(uint64_t n) {
    const uint64_t per_block = DEL_THREADS / 64;
    return (uint32_t)std::min<uint64_t>((n + per_block - 1) / per_block, (uint64_t)dcn_cu_count() * 32);
}

} // namespace

int dcn_launch_del_count(const dcn_del_append_args &args, hipStream_t stream) {
    if (args.rows.n_work == 0) return DCN_OK;
    hipLaunchKernelGGL(del_walk_kernel<false>, dim3(wave_blocks(args.rows.n_work)), dim3(DEL_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_del_write(const dcn_del_append_args &args, hipStream_t stream) {
    if (args.rows.n_work == 0) return DCN_OK;
    hipLaunchKernelGGL(del_walk_kernel<true>, dim3(wave_blocks(args.rows.n_work)), dim3(DEL_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_del_plane(const dcn_del_range_args &args, hipStream_t stream) {
    if (args.n_events == 0) return DCN_OK;
    hipLaunchKernelGGL(del_plane_kernel, dim3(thread_blocks(args.n_events)), dim3(DEL_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_del_scatter(const dcn_del_range_args &args, hipStream_t stream) {
    if (args.n_events == 0) return DCN_OK;
    hipLaunchKernelGGL(del_scatter_kernel, dim3(thread_blocks(args.n_events)), dim3(DEL_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_del_gather(const dcn_del_range_args &args, hipStream_t stream) {
    if (args.n_slots == 0) return DCN_OK;
    hipLaunchKernelGGL(del_gather_kernel, dim3(thread_blocks(args.n_slots)), dim3(DEL_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_del_winner(const dcn_del_range_args &args, hipStream_t stream) {
    if (args.n == 0) return DCN_OK;
    hipLaunchKernelGGL(del_winner_kernel, dim3(wave_blocks((args.n + 63) / 64)), dim3(DEL_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

uint32_t dcn_indel_site_blocks(uint64_t n) { return thread_blocks(n); }

int dcn_launch_indel_flags(const uint32_t *counts, uint32_t *flags, uint64_t n, hipStream_t stream) {
    if (n == 0) return DCN_OK;
    hipLaunchKernelGGL(indel_flags_kernel, dim3(thread_blocks(n)), dim3(DEL_THREADS), 0, stream, counts, flags, n);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_indel_sites(const dcn_indel_site_args &args, bool write, hipStream_t stream) {
    if (args.n == 0) return DCN_OK;
    const dim3 grid(dcn_indel_site_blocks(args.n)), block(DEL_THREADS);
    if (write) hipLaunchKernelGGL(indel_site_kernel<true>, grid, block, 0, stream, args);
    else hipLaunchKernelGGL(indel_site_kernel<false>, grid, block, 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_indel_bases(const dcn_indel_site_args &args, hipStream_t stream) {
    if (args.n_sites == 0) return DCN_OK;
    hipLaunchKernelGGL(indel_bases_kernel, dim3(wave_blocks(args.n_sites)), dim3(DEL_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}
