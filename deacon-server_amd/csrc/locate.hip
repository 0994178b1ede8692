// locate.hip -- where in each read the index matched (dcn_locate_batch; the definition is in include/deacon_hip.h).
//
// Runs behind the dump front end (dump_front_end, ctx.hip: pack -> plan -> scan in dump mode with batch-absolute
// positions):
//   locate_mark_kernel      the flat sweep over the dump entries (dcn_dump_sweep.h): probe the table (for a
//                           set: read the label of the slot that matched) and, on a hit that passes member_mask, set bit
//                           `position` of the batch's hit bitmap (dcn_bit_mark) and, for a set, store the label at
//                           label_scratch[position].  No per-read state: a position that several windows emitted is one
//                           bit, which is the "counts once" of the definition.
//   locate_segments_kernel  read r's segments from its slice [offsets[r], offsets[r+1]) of the bitmap.  A hit starts a
//                           segment iff no hit lies in the k + max_gap positions before it.  COUNT pass -> exclusive
//                           scan over reads (dcn_launch_offsets_scan) -> WRITE pass: reads in order, segments ascending, no sorting and no atomics
//                           on the output.  One lane walks a short read bit by bit; a long read goes to a work list and
//                           locate_segments_wave_kernel, a wave per read, a bitmap word per lane: the word's hits are one
//                           partial segment (k + max_gap >= 31), joined to the previous lane's by a max-scan of the last
//                           hit positions and summed by a segmented scan, with the open segment carried in wave-uniform
//                           registers across the wave's iterations.
// min_hits is applied by both passes in the same code (the WRITE template flag only adds the stores).
#include "dcn_locate.h"
#include "dcn_probe.h"

#include <algorithm>

namespace {

// label of `key` in the table: the slot's member mask for a set, 1 for a plain index; 0 = absent
__device__ inline uint32_t loc_label(const dcn_locate_args &a, uint64_t key) {
    if (key == 0) return a.zero_label;
    uint32_t g = dcn_group_of(key, a.table.group_shift, a.table.group_mask);
    for (;;) {
        const dcn_group grp = dcn_load_group(a.table, g);
        const uint64_t s0 = (uint64_t)g * DCN_GROUP_SLOTS;
        if (grp.a.x == key) return a.labels ? a.labels[s0] : 1u;
        if (grp.a.y == key) return a.labels ? a.labels[s0 + 1] : 1u;
#if DCN_GROUP_SLOTS == 4
        if (grp.b.x == key) return a.labels ? a.labels[s0 + 2] : 1u;
        if (grp.b.y == key) return a.labels ? a.labels[s0 + 3] : 1u;
        if (grp.a.x == 0 || grp.a.y == 0 || grp.b.x == 0 || grp.b.y == 0) return 0;
#else
        if (grp.a.x == 0 || grp.a.y == 0) return 0;
#endif
        g = (g + 1) & a.table.group_mask;
    }
}

__global__ __launch_bounds__(DCN_SWEEP_THREADS) void locate_mark_kernel(dcn_locate_args a) {
    dcn_for_dump_entries(a.dump, [&](uint64_t s) {
        const uint32_t L = loc_label(a, a.dump.hash[s]) & a.member_mask;
        if (!L) return;
        const uint64_t p = dcn_dump_position(a.dump, s);
        if (p >= a.dump.n_bases) return;
        dcn_bit_mark(a.bits, p);
        if (a.labels) a.label_scratch[p] = L; // (windows that share a position share its hash: the same value)
    });
}

__device__ inline uint32_t loc_word_labels(const dcn_locate_args &a, uint64_t wi, uint32_t word) {
    if (!a.labels) return word ? 1u : 0u;
    uint32_t L = 0;
    for (uint32_t b = word; b; b &= b - 1) L |= a.label_scratch[wi * 32 + (__ffs(b) - 1)];
    return L;
}

__device__ inline bool loc_is_big(const dcn_locate_args &a, uint64_t len) {
    return len > DCN_LOC_LANE_BASES && a.join >= 31;
}

template <bool WRITE>
__device__ inline void loc_emit(const dcn_locate_args &a, uint64_t at, uint32_t start, uint32_t last, uint32_t n, uint32_t lab) {
    if constexpr (WRITE) {
        if (at < a.seg_cap) {
            dcn_segment s;
            s.start = start;
            s.end = last + a.k;
            s.n_hits = n;
            s.members = lab;
            a.segs[at] = s;
        }
    }
}

// one lane per read
template <bool WRITE>
__global__ __launch_bounds__(DCN_LOC_THREADS) void locate_segments_kernel(dcn_locate_args a) {
    const uint32_t r = blockIdx.x * DCN_LOC_THREADS + threadIdx.x;
    if (r >= a.n_reads) return;
    const uint64_t o0 = a.offsets[r], o1 = a.offsets[r + 1];
    if (loc_is_big(a, o1 - o0)) {
        if constexpr (!WRITE) a.big[atomicAdd(a.n_big, 1u)] = r;
        return;
    }
    uint32_t n_seg = 0;
    const uint64_t out = WRITE ? a.seg_offsets[r] : 0;
    bool open = false;
    uint32_t start = 0, last = 0, cnt = 0, lab = 0;
    if (o1 > o0) {
        for (uint64_t wi = o0 >> 5; wi <= ((o1 - 1) >> 5); ++wi) {
            for (uint32_t word = dcn_bits_cut(a.bits, wi, o0, o1); word; word &= word - 1) {
                const uint64_t q = wi * 32 + (__ffs(word) - 1);
                const uint32_t p = (uint32_t)(q - o0), L = a.labels ? a.label_scratch[q] : 1u;
                if (open && p - last <= a.join) {
                    last = p;
                    ++cnt;
                    lab |= L;
                    continue;
                }
                if (open && cnt >= a.min_hits) loc_emit<WRITE>(a, out + n_seg++, start, last, cnt, lab);
                open = true;
                start = last = p;
                cnt = 1;
                lab = L;
            }
        }
    }
    if (open && cnt >= a.min_hits) loc_emit<WRITE>(a, out + n_seg++, start, last, cnt, lab);
    if constexpr (!WRITE) a.counts[r] = n_seg;
}

// one wave per listed read
template <bool WRITE>
__global__ __launch_bounds__(DCN_LOC_THREADS) void locate_segments_wave_kernel(dcn_locate_args a) {
    const uint32_t lane = threadIdx.x & (DCN_WAVE - 1);
    const uint32_t waves = DCN_LOC_THREADS / DCN_WAVE;
    const uint32_t n_big = *a.n_big;
    for (uint32_t item = blockIdx.x * waves + threadIdx.x / DCN_WAVE; item < n_big; item += gridDim.x * waves) {
        const uint32_t r = a.big[item];
        const uint64_t o0 = a.offsets[r], o1 = a.offsets[r + 1]; // (o1 - o0 > DCN_LOC_LANE_BASES)
        const uint64_t w1 = (o1 - 1) >> 5;
        const uint64_t out = WRITE ? a.seg_offsets[r] : 0;
        uint32_t n_seg = 0;
        // the segment that is open at the end of the words seen so far (the same in every lane)
        bool c_open = false;
        uint32_t c_start = 0, c_last = 0, c_cnt = 0, c_lab = 0;
        for (uint64_t wb = o0 >> 5; wb <= w1; wb += DCN_WAVE) {
            const uint64_t wi = wb + lane;
            const uint32_t word = wi <= w1 ? dcn_bits_cut(a.bits, wi, o0, o1) : 0u;
            const bool ne = word != 0;
            const uint32_t f = ne ? (uint32_t)(wi * 32 + (__ffs(word) - 1) - o0) : 0u;
            const uint32_t l = ne ? (uint32_t)(wi * 32 + (31 - __clz(word)) - o0) : 0u;
            // last hit position + 1 of the lanes before this one (0: none), then of the carried segment
            uint32_t incl = ne ? l + 1 : 0u;
            for (uint32_t d = 1; d < DCN_WAVE; d <<= 1) {
                const uint32_t v = __shfl_up(incl, d);
                if (lane >= d) incl = max(incl, v);
            }
            uint32_t prev = __shfl_up(incl, 1);
            if (lane == 0) prev = 0;
            if (prev == 0 && c_open) prev = c_last + 1;
            const bool head = ne && (prev == 0 || f - (prev - 1) > a.join);
            // segmented inclusive scan: (start of the head, hits, labels) from the nearest head at or before this lane;
            // flag clear = no head so far in this iteration, the sums continue the carried segment
            uint32_t s_start = f, s_cnt = __popc(word), s_lab = loc_word_labels(a, wi, word);
            bool s_flag = head;
            for (uint32_t d = 1; d < DCN_WAVE; d <<= 1) {
                const uint32_t o_start = __shfl_up(s_start, d), o_cnt = __shfl_up(s_cnt, d), o_lab = __shfl_up(s_lab, d);
                const bool o_flag = __shfl_up((int)s_flag, d) != 0;
                if (lane >= d && !s_flag) {
                    s_start = o_start;
                    s_cnt += o_cnt;
                    s_lab |= o_lab;
                    s_flag = o_flag;
                }
            }
            if (!s_flag) { // continues the carried segment (a lane with hits and no head before it implies c_open)
                s_start = c_start;
                s_cnt += c_cnt;
                s_lab |= c_lab;
            }
            const unsigned long long ne_mask = __ballot(ne), head_mask = __ballot(head);
            if (ne_mask == 0) continue;
            // the carried segment ends where this iteration's first hits start a new one
            const uint32_t first_ne = __ffsll((long long)ne_mask) - 1;
            uint32_t base = n_seg;
            if (c_open && ((head_mask >> first_ne) & 1ull) && c_cnt >= a.min_hits) {
                if (lane == 0) loc_emit<WRITE>(a, out + base, c_start, c_last, c_cnt, c_lab);
                ++base;
            }
            // a lane closes its segment when the next lane with hits is a head
            const unsigned long long above = lane == DCN_WAVE - 1 ? 0ull : ne_mask & (~0ull << (lane + 1));
            const bool tail = ne && above != 0 && ((head_mask >> (__ffsll((long long)above) - 1)) & 1ull);
            const bool emit = tail && s_cnt >= a.min_hits;
            const unsigned long long emit_mask = __ballot(emit);
            if (emit) loc_emit<WRITE>(a, out + base + __popcll(emit_mask & ((1ull << lane) - 1)), s_start, l, s_cnt, s_lab);
            n_seg = base + __popcll(emit_mask);
            // what stays open: the sums at the last lane with hits
            const uint32_t last_ne = 63 - __clzll((long long)ne_mask);
            c_open = true;
            c_start = __shfl(s_start, last_ne);
            c_last = __shfl(l, last_ne);
            c_cnt = __shfl(s_cnt, last_ne);
            c_lab = __shfl(s_lab, last_ne);
        }
        if (c_open && c_cnt >= a.min_hits) {
            if (lane == 0) loc_emit<WRITE>(a, out + n_seg, c_start, c_last, c_cnt, c_lab);
            ++n_seg;
        }
        if constexpr (!WRITE)
            if (lane == 0) a.counts[r] = n_seg;
    }
}

uint32_t loc_wave_blocks(uint32_t n_reads) {
    const uint32_t waves = DCN_LOC_THREADS / DCN_WAVE;
    return std::max(1u, std::min((n_reads + waves - 1) / waves, dcn_cu_count() * 8));
}

} // namespace

int dcn_launch_locate_mark(const dcn_locate_args &a, hipStream_t stream) {
    return dcn_launch_dump_sweep(locate_mark_kernel, a, "locate: tile count", stream);
}

int dcn_launch_locate_count(const dcn_locate_args &a, hipStream_t stream) {
    if (a.n_reads == 0) return DCN_OK;
    DCN_HIP(hipMemsetAsync(a.n_big, 0, sizeof(uint32_t), stream));
    const uint32_t blocks = (a.n_reads + DCN_LOC_THREADS - 1) / DCN_LOC_THREADS;
    hipLaunchKernelGGL(locate_segments_kernel<false>, dim3(blocks), dim3(DCN_LOC_THREADS), 0, stream, a);
    hipLaunchKernelGGL(locate_segments_wave_kernel<false>, dim3(loc_wave_blocks(a.n_reads)), dim3(DCN_LOC_THREADS), 0, stream, a);
    DCN_HIP(hipGetLastError());
    return dcn_launch_offsets_scan(a.counts, a.n_reads, a.block_sums, a.seg_offsets, stream);
}

int dcn_launch_locate_write(const dcn_locate_args &a, hipStream_t stream) {
    if (a.n_reads == 0) return DCN_OK;
    const uint32_t blocks = (a.n_reads + DCN_LOC_THREADS - 1) / DCN_LOC_THREADS;
    hipLaunchKernelGGL(locate_segments_kernel<true>, dim3(blocks), dim3(DCN_LOC_THREADS), 0, stream, a);
    hipLaunchKernelGGL(locate_segments_wave_kernel<true>, dim3(loc_wave_blocks(a.n_reads)), dim3(DCN_LOC_THREADS), 0, stream, a);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}
