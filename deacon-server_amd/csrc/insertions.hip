// insertions.hip -- the kernels of an insertion ledger (THE DEFINITION OF AN INSERTION LEDGER, include/deacon_hip.h; what
// the host shares is in dcn_insertions.h).  Count, scan, gather, twice.
//   Append, behind pileup_kernel on the context's stream (one wave per aligned row, pileup_kernel's walk: the runs in
//   chunks of 64, a wave prefix sum for every run's (i, j)):
//     ins_walk_kernel<false>  per row the number of its I runs and of their bases; a wave adds what its rows had to the
//                             call's two totals once, and only when there was something.
//     ins_walk_kernel<true>   behind the scans of both: every I run's event at its row's offset, the lanes striding over
//                             its bases, read through dcn_wf_side16 with the strand flag as pileup_kernel's column_of does.
//   Fetch and call, on the null stream, over a range of one record:
//     ins_plane_kernel<CALL>  one thread per position: the INS counter (rule L2: the number of events there), for a call
//                             only where rule L6 holds; their scan gives every position a bucket.
//     ins_scatter_kernel      one thread per event of the ledger: into its position's bucket, by a per-position cursor.
//     ins_slot_lens_kernel, ins_gather_kernel   fetch: the lengths of the bucketed events, and behind their scan the
//                             events and their bases in bucket order (the host sorts each bucket by rule L4).
//     ins_winner_kernel       call: a wave per 64 positions, for each with a called insertion the lanes stride over the
//                             bucket, each counts the events equal to its own, a wave reduction picks the winner (L5).
//                             Quadratic in the events of one position.
//     ins_alleles_kernel      behind the scan of the winners' lengths: a wave per allele writes it and copies its bases.
// Integers and bytes only.  Which slot of a bucket an event takes depends on the order of the atomic adds; nothing that
// is returned does (L5 is order-free, and fetch sorts).
#include "dcn_dump_sweep.h"
#include "dcn_insertions.h"
#include "dcn_verify.h"
#include "dcn_wavefront.h"

#include <algorithm>

namespace {

constexpr uint32_t INS_THREADS = 256; // four waves

__device__ inline uint32_t wave_sum(uint32_t v) {
    for (uint32_t d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

template <bool WRITE>
__global__ __launch_bounds__(INS_THREADS) void ins_walk_kernel(dcn_ins_append_args a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (INS_THREADS / 64);
    unsigned long long sum_events = 0, sum_bases = 0; // of this wave's rows (the same in every lane)
    for (uint64_t w = (uint64_t)blockIdx.x * (INS_THREADS / 64) + threadIdx.x / 64; w < a.rows.n_work; w += waves) {
        const dcn_align_work wk = a.rows.work[w];
        const dcn_verify_item it = a.rows.items[wk.row];
        const uint32_t count = a.rows.n_ops[wk.row];
        if (it.n == 0 || count == 0) { // rule P2 (the same for the whole wave)
            if (!WRITE && lane == 0) a.row_events[w] = 0, a.row_bases[w] = 0;
            continue;
        }
        const uint32_t *const runs = a.rows.cigar + a.rows.cigar_offsets[wk.row];
        if (!WRITE) {
            uint32_t ev = 0, nb = 0;
            for (uint32_t c0 = lane; c0 < count; c0 += 64) {
                const uint32_t run = runs[c0];
                ev += dcn_ins_run_events(run);
                nb += dcn_ins_run_bases(run);
            }
            ev = wave_sum(ev);
            nb = wave_sum(nb);
            if (lane == 0) a.row_events[w] = ev, a.row_bases[w] = nb;
            sum_events += ev;
            sum_bases += nb;
            continue;
        }
        if (a.row_events[w] == 0) continue;
        const dcn_wf_side S = {a.rows.s_packed, a.rows.s_invmask, it.s_origin, it.flags & 1u};
        const uint32_t reverse = it.flags & 1u, m = it.m;
        const uint64_t t0 = (uint64_t)it.t_origin;
        const auto char_of = [&](uint32_t i) -> uint8_t {
            if (i >= m) return 'N'; // (never: the runs cover exactly m bases of S)
            uint32_t x, inv;
            dcn_wf_side16<dcn_wf_plain>(S, (int64_t)i, &x, &inv);
            return dcn_ins_char(x & 3u, inv & 1u);
        };
        // where the row's events and bases go, and where they end: a run that would pass either is not written
        uint64_t event_at = a.event0 + a.event_offsets[w], base_at = a.base0 + a.base_offsets[w];
        const uint64_t event_end = a.event0 + a.event_offsets[w + 1], base_end = a.base0 + a.base_offsets[w + 1];
        uint32_t i0 = 0, j0 = 0;
        for (uint32_t c0 = 0; c0 < count; c0 += 64) {
            const uint32_t here = min(64u, count - c0);
            const uint32_t run = lane < here ? runs[c0 + lane] : 0u;
            uint32_t si = dcn_pile_step_s(run), sj = dcn_pile_step_t(run), se = dcn_ins_run_events(run), sb = dcn_ins_run_bases(run);
            for (uint32_t d = 1; d < 64; d <<= 1) { // -> inclusive sums over the lanes
                const uint32_t oi = __shfl_up(si, d), oj = __shfl_up(sj, d), oe = __shfl_up(se, d), ob = __shfl_up(sb, d);
                if (lane >= d) si += oi, sj += oj, se += oe, sb += ob;
            }
            const uint32_t my_i = i0 + si - dcn_pile_step_s(run), my_j = j0 + sj - dcn_pile_step_t(run);
            const uint64_t my_e = event_at + se - dcn_ins_run_events(run), my_b = base_at + sb - dcn_ins_run_bases(run);
            unsigned long long todo = __ballot(dcn_ins_run_events(run) != 0);
            while (todo) {
                const uint32_t r = (uint32_t)__ffsll((long long)todo) - 1u;
                todo &= todo - 1ull;
                const uint32_t rr = __shfl(run, r), ri = __shfl(my_i, r), rj = __shfl(my_j, r);
                const uint64_t re = ((uint64_t)__shfl((uint32_t)(my_e >> 32), r) << 32) | __shfl((uint32_t)my_e, r);
                const uint64_t rb = ((uint64_t)__shfl((uint32_t)(my_b >> 32), r) << 32) | __shfl((uint32_t)my_b, r);
                if (re < event_end && rb + (rr >> 4) <= base_end) // (always: the counting pass walked the same runs)
                    dcn_ins_write_run(rr, ri, rj, reverse, t0, re, rb, lane, 64u, char_of, a.events, a.bases);
            }
            i0 += __shfl(si, 63);
            j0 += __shfl(sj, 63);
            event_at += __shfl(se, 63);
            base_at += __shfl(sb, 63);
        }
    }
    if (!WRITE && lane == 0 && sum_events != 0) {
        atomicAdd(a.totals, sum_events);
        atomicAdd(a.totals + 1, sum_bases);
    }
}

template <bool CALL>
__global__ __launch_bounds__(INS_THREADS) void ins_plane_kernel(dcn_ins_range_args a) {
    const uint64_t q = (uint64_t)blockIdx.x * INS_THREADS + threadIdx.x;
    if (q >= a.n) return;
    const uint64_t b = a.base0 + q;
    uint32_t ins = a.counters[dcn_pile_index(DCN_PILE_INS, b, a.bases)];
    if (CALL) {
        uint32_t counts[DCN_PILE_COLUMNS - 1];
#pragma unroll
        for (uint32_t c = 0; c < DCN_PILE_COLUMNS - 1; ++c) counts[c] = a.counters[dcn_pile_index(c, b, a.bases)];
        const uint32_t code = (a.t_packed[b >> 4] >> (2 * (b & 15))) & 3u, inv = (a.t_invmask[b >> 5] >> (b & 31)) & 1u;
        const uint32_t info = dcn_pile_call(counts, dcn_pile_column(code, inv), a.min_depth, a.min_permille);
        if (!(info & DCN_PILE_SITE_INS)) ins = 0; // rule L6
        a.flags[q] = ins > 0 ? 1u : 0u;
    }
    a.counts[q] = ins;
}

__global__ __launch_bounds__(INS_THREADS) void ins_scatter_kernel(dcn_ins_range_args a) {
    const uint64_t e = (uint64_t)blockIdx.x * INS_THREADS + threadIdx.x;
    if (e >= a.n_events) return;
    const uint64_t base = a.events[e].base;
    if (base < a.base0 || base - a.base0 >= a.n) return;
    const uint64_t q = base - a.base0;
    const uint32_t room = a.counts[q];
    if (room == 0) return;
    const uint32_t k = atomicAdd(a.cursor + q, 1u);
    if (k < room) a.slots[a.bucket_offsets[q] + k] = e; // (always, by L2: the bucket has a slot per event)
}

__global__ __launch_bounds__(INS_THREADS) void ins_slot_lens_kernel(dcn_ins_range_args a) {
    const uint64_t s = (uint64_t)blockIdx.x * INS_THREADS + threadIdx.x;
    if (s < a.n_slots) a.slot_lens[s] = a.events[a.slots[s]].len;
}

__global__ __launch_bounds__(INS_THREADS) void ins_gather_kernel(dcn_ins_range_args a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (INS_THREADS / 64);
    dcn_insertion *const out = static_cast<dcn_insertion *>(a.out_events);
    for (uint64_t s = (uint64_t)blockIdx.x * (INS_THREADS / 64) + threadIdx.x / 64; s < a.n_slots; s += waves) {
        const dcn_ins_event e = a.events[a.slots[s]];
        const uint64_t at = a.slot_offsets[s];
        const uint32_t len = (uint32_t)(a.slot_offsets[s + 1] - at); // (= e.len: what the scan was given)
        if (lane == 0) {
            dcn_insertion o;
            o.pos = a.pos0 + (e.base - a.base0);
            o.bases_offset = at;
            o.len = len;
            o.flags = e.flags;
            out[s] = o;
        }
        for (uint32_t q = lane; q < len; q += 64) a.out_bases[at + q] = a.ledger_bases[e.bases_offset + q];
    }
}

__global__ __launch_bounds__(INS_THREADS) void ins_winner_kernel(dcn_ins_range_args a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (INS_THREADS / 64), chunks = (a.n + 63) / 64;
    for (uint64_t ch = (uint64_t)blockIdx.x * (INS_THREADS / 64) + threadIdx.x / 64; ch < chunks; ch += waves) {
        const uint64_t mine = ch * 64 + lane;
        unsigned long long todo = __ballot(mine < a.n && a.flags[mine] != 0);
        while (todo) {
            const uint64_t q = ch * 64 + (uint64_t)__ffsll((long long)todo) - 1u;
            todo &= todo - 1ull;
            const uint64_t s0 = a.bucket_offsets[q];
            const uint32_t count = (uint32_t)(a.bucket_offsets[q + 1] - s0);
            const uint64_t *const slots = a.slots + s0;
            uint32_t best_count = 0;
            uint32_t best = dcn_ins_lane_winner(slots, count, lane, 64u, a.events, a.ledger_bases, &best_count);
            for (uint32_t d = 32; d > 0; d >>= 1) {
                const uint32_t other = __shfl_xor(best, d), other_count = __shfl_xor(best_count, d);
                if (other != UINT32_MAX &&
                    (best == UINT32_MAX || dcn_ins_beats(other_count, a.events[slots[other]], best_count, a.events[slots[best]], a.ledger_bases)))
                    best = other, best_count = other_count;
            }
            if (lane == 0 && best != UINT32_MAX) { // (always: a called insertion has INS > 0 events)
                const uint64_t at = a.allele_offsets[q];
                const uint64_t e = slots[best];
                a.win_event[at] = e;
                a.win_count[at] = best_count;
                a.win_events[at] = count;
                a.win_len[at] = a.events[e].len;
                a.win_pos[at] = a.pos0 + q;
            }
        }
    }
}

__global__ __launch_bounds__(INS_THREADS) void ins_alleles_kernel(dcn_ins_range_args a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (INS_THREADS / 64);
    dcn_insertion_allele *const out = static_cast<dcn_insertion_allele *>(a.out_alleles);
    for (uint64_t s = (uint64_t)blockIdx.x * (INS_THREADS / 64) + threadIdx.x / 64; s < a.n_alleles; s += waves) {
        const dcn_ins_event e = a.events[a.win_event[s]];
        const uint64_t at = a.win_offsets[s];
        const uint32_t len = (uint32_t)(a.win_offsets[s + 1] - at);
        if (lane == 0) {
            dcn_insertion_allele o;
            o.pos = a.win_pos[s];
            o.bases_offset = at;
            o.len = len;
            o.count = a.win_count[s];
            o.events = a.win_events[s];
            o.flags = e.flags & DCN_INS_FRONT;
            out[s] = o;
        }
        for (uint32_t q = lane; q < len; q += 64) a.out_bases[at + q] = a.ledger_bases[e.bases_offset + q];
    }
}

// workgroups of a grid with one thread per item
uint32_t thread_blocks(uint64_t n) { return (uint32_t)((n + INS_THREADS - 1) / INS_THREADS); }
// ... and of one whose waves stride over n items
uint32_t wave_blocks(uint64_t n) {
    const uint64_t per_block = INS_THREADS / 64;
    return (uint32_t)std::min<uint64_t>((n + per_block - 1) / per_block, (uint64_t)dcn_cu_count() * 32);
}

} // namespace

int dcn_launch_ins_count(const dcn_ins_append_args &args, hipStream_t stream) {
    if (args.rows.n_work == 0) return DCN_OK;
    hipLaunchKernelGGL(ins_walk_kernel<false>, dim3(wave_blocks(args.rows.n_work)), dim3(INS_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_ins_write(const dcn_ins_append_args &args, hipStream_t stream) {
    if (args.rows.n_work == 0) return DCN_OK;
    hipLaunchKernelGGL(ins_walk_kernel<true>, dim3(wave_blocks(args.rows.n_work)), dim3(INS_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_ins_plane(const dcn_ins_range_args &args, bool call, hipStream_t stream) {
    if (args.n == 0) return DCN_OK;
    if (call) hipLaunchKernelGGL(ins_plane_kernel<true>, dim3(thread_blocks(args.n)), dim3(INS_THREADS), 0, stream, args);
    else hipLaunchKernelGGL(ins_plane_kernel<false>, dim3(thread_blocks(args.n)), dim3(INS_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_ins_scatter(const dcn_ins_range_args &args, hipStream_t stream) {
    if (args.n_events == 0) return DCN_OK;
    hipLaunchKernelGGL(ins_scatter_kernel, dim3(thread_blocks(args.n_events)), dim3(INS_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_ins_slot_lens(const dcn_ins_range_args &args, hipStream_t stream) {
    if (args.n_slots == 0) return DCN_OK;
    hipLaunchKernelGGL(ins_slot_lens_kernel, dim3(thread_blocks(args.n_slots)), dim3(INS_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_ins_gather(const dcn_ins_range_args &args, hipStream_t stream) {
    if (args.n_slots == 0) return DCN_OK;
    hipLaunchKernelGGL(ins_gather_kernel, dim3(wave_blocks(args.n_slots)), dim3(INS_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_ins_winner(const dcn_ins_range_args &args, hipStream_t stream) {
    if (args.n == 0) return DCN_OK;
    hipLaunchKernelGGL(ins_winner_kernel, dim3(wave_blocks((args.n + 63) / 64)), dim3(INS_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_ins_alleles(const dcn_ins_range_args &args, hipStream_t stream) {
    if (args.n_alleles == 0) return DCN_OK;
    hipLaunchKernelGGL(ins_alleles_kernel, dim3(wave_blocks(args.n_alleles)), dim3(INS_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}
