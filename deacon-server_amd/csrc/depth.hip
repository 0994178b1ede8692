// depth.hip -- how often each key of a labelled set occurred among the minimizers classify calls counted
// (dcn_index_set_depth_*; the definition is in include/deacon_hip.h, the layout in dcn_depth.h).
//
// Runs behind the dump front end (dump_front_end, ctx.hip: pack -> plan -> scan in dump mode with batch-absolute
// positions), beside the classification kernels and without touching them:
//   depth_count_kernel  the flat sweep over the dump entries (dcn_dump_sweep.h): find the entry's slot
//                       (dcn_table_find_slot); on a hit claim the entry's position in the batch's position bitmap
//                       (dcn_bit_claim) and add 1 to the slot's 16-bit counter, saturating.  The dump may hold a
//                       position more than once (two windows of a read can choose the same k-mer with another between
//                       them; the classification totals count both), an occurrence is a (read, position) pair: hence
//                       the bitmap rather than a count of entries.
//   depth_stats_kernel / depth_hist_kernel / depth_keys_kernel
//                       sweeps over labels and counters together, four slots per lane (one 16-byte load of labels, one
//                       8-byte load of counters), grid-stride in wave-uniform steps, tallies in LDS, one global atomic per
//                       output cell per workgroup (keys: one returning atomicAdd per wave).
#include "dcn_depth.h"
#include "dcn_probe.h"

#include <algorithm>

namespace {

__global__ __launch_bounds__(DCN_SWEEP_THREADS) void depth_count_kernel(dcn_depth_args a) {
    if (a.status->bad_offsets) return; // the scan looked at no tile: the dump is not this batch's
    dcn_for_dump_entries(a.dump, [&](uint64_t s) {
        const uint64_t h = a.dump.hash[s];
        uint32_t *word;
        uint32_t shift = 0;
        if (h == 0) {
            if (!a.depth_zero) return;
            word = a.depth_zero;
        } else {
            const uint32_t g = dcn_group_of(h, a.table.group_shift, a.table.group_mask);
            const uint64_t at = dcn_table_find_slot(a.table, h, g, dcn_load_group(a.table, g));
            if (at == ~0ull) return;
            word = a.depth + (at >> 1);
            shift = (uint32_t)(at & 1) * 16;
        }
        const uint64_t p = dcn_dump_position(a.dump, s);
        if (p >= a.dump.n_bases) return;
        if (dcn_bit_claim(a.bits, p)) dcn_depth_add(word, shift);
    });
}

// ---- sweeps -------------------------------------------------------------------------------------------------------
// labels and depths of slots 4q .. 4q+3 (zero past the table)
struct depth_quad {
    uint32_t L[4], D[4];
};

__device__ inline depth_quad depth_load_quad(const uint32_t *labels, const uint32_t *depth, uint64_t q, uint64_t n_quads,
                                             uint64_t n_slots) {
    depth_quad r;
    const uint64_t s = q * 4;
    if (q < n_quads && s + 4 <= n_slots) {
        const uint4 l = *reinterpret_cast<const uint4 *>(labels + s);
        const uint2 d = *reinterpret_cast<const uint2 *>(depth + (s >> 1));
        r.L[0] = l.x, r.L[1] = l.y, r.L[2] = l.z, r.L[3] = l.w;
        r.D[0] = d.x & DCN_DEPTH_MAX, r.D[1] = d.x >> 16, r.D[2] = d.y & DCN_DEPTH_MAX, r.D[3] = d.y >> 16;
    } else { // a table of fewer than four slots, or a lane past the table
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const bool in = q < n_quads && s + i < n_slots;
            r.L[i] = in ? labels[s + i] : 0u;
            r.D[i] = in ? (depth[(s + i) >> 1] >> (((s + i) & 1) * 16)) & DCN_DEPTH_MAX : 0u;
        }
    }
    return r;
}

// the wave-uniform grid-stride loop of the sweeps: body(i, qd) sees this lane's quad index (maybe past the table) and its
// labels and depths
template <typename F>
__device__ inline void depth_for_quads(const uint32_t *labels, const uint32_t *depth, uint64_t n_slots, uint32_t tid,
                                       uint32_t lane, F body) {
    const uint64_t n_quads = (n_slots + 3) / 4;
    const uint64_t stride = (uint64_t)gridDim.x * DCN_DEPTH_THREADS;
    for (uint64_t q0 = (uint64_t)blockIdx.x * DCN_DEPTH_THREADS + (tid - lane); q0 < n_quads; q0 += stride) {
        const uint64_t i = q0 + lane;
        body(i, depth_load_quad(labels, depth, i, n_quads, n_slots));
    }
}

__global__ __launch_bounds__(DCN_DEPTH_THREADS) void depth_stats_kernel(const uint32_t *labels, const uint32_t *depth,
                                                                        uint64_t n_slots, uint32_t n,
                                                                        unsigned long long *out) {
    __shared__ unsigned long long s_acc[3][32]; // observed, sum, saturated per member
    const uint32_t tid = threadIdx.x, lane = tid & (DCN_WAVE - 1);
    if (tid < 96) s_acc[tid >> 5][tid & 31] = 0;
    __syncthreads();
    depth_for_quads(labels, depth, n_slots, tid, lane, [&](uint64_t, const depth_quad &qd) {
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            if (!qd.D[q]) continue;
            for (uint32_t mm = qd.L[q]; mm; mm &= mm - 1) {
                const uint32_t j = __ffs(mm) - 1;
                atomicAdd(&s_acc[0][j], 1ull);
                atomicAdd(&s_acc[1][j], (unsigned long long)qd.D[q]);
                if (qd.D[q] == DCN_DEPTH_MAX) atomicAdd(&s_acc[2][j], 1ull);
            }
        }
    });
    __syncthreads();
    if (tid < 96 && (tid & 31) < n && s_acc[tid >> 5][tid & 31]) atomicAdd(&out[tid], s_acc[tid >> 5][tid & 31]);
}

__global__ __launch_bounds__(DCN_DEPTH_THREADS) void depth_hist_kernel(const uint32_t *labels, const uint32_t *depth,
                                                                       uint64_t n_slots, uint32_t mask, uint32_t n_bins,
                                                                       unsigned long long *hist) {
    __shared__ uint32_t s_hist[DCN_DEPTH_MAX_BINS];
    __shared__ unsigned long long s_zero; // bin 0, the unobserved keys: most of a set, kept out of the LDS atomics
    const uint32_t tid = threadIdx.x, lane = tid & (DCN_WAVE - 1);
    for (uint32_t b = tid; b < n_bins; b += DCN_DEPTH_THREADS) s_hist[b] = 0;
    if (tid == 0) s_zero = 0;
    __syncthreads();
    unsigned long long zero = 0;
    depth_for_quads(labels, depth, n_slots, tid, lane, [&](uint64_t, const depth_quad &qd) {
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            if (!(qd.L[q] & mask)) continue;
            if (!qd.D[q]) ++zero;
            else atomicAdd(&s_hist[min(qd.D[q], n_bins - 1)], 1u);
        }
    });
    if (zero) atomicAdd(&s_zero, zero);
    __syncthreads();
    for (uint32_t b = tid; b < n_bins; b += DCN_DEPTH_THREADS) {
        const unsigned long long v = s_hist[b] + (b == 0 ? s_zero : 0ull);
        if (v) atomicAdd(&hist[b], v);
    }
}

__global__ __launch_bounds__(DCN_DEPTH_THREADS) void depth_keys_kernel(const uint32_t *labels, const uint32_t *depth,
                                                                       const uint64_t *slots, uint64_t n_slots,
                                                                       uint32_t mask, uint64_t *keys, uint32_t *depths,
                                                                       uint64_t cap, unsigned long long *n_out) {
    __shared__ unsigned long long s_n;
    const uint32_t tid = threadIdx.x, lane = tid & (DCN_WAVE - 1);
    if (tid == 0) s_n = 0;
    __syncthreads();
    unsigned long long mine = 0;
    depth_for_quads(labels, depth, n_slots, tid, lane, [&](uint64_t i, const depth_quad &qd) {
        uint32_t c = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) c += (qd.D[q] && (qd.L[q] & mask)) ? 1u : 0u;
        if (!keys) {
            mine += c;
            return;
        }
        // the wave's exclusive prefix of c, its total, and one atomicAdd by lane 0 for the wave's range of the outputs
        uint32_t incl = c;
        for (uint32_t d = 1; d < DCN_WAVE; d <<= 1) {
            const uint32_t v = __shfl_up(incl, d);
            if (lane >= d) incl += v;
        }
        const uint32_t wave_total = __shfl(incl, DCN_WAVE - 1);
        if (!wave_total) return;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(n_out, (unsigned long long)wave_total);
        base = __shfl(base, 0);
        uint64_t pos = base + (incl - c);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            if (!(qd.D[q] && (qd.L[q] & mask))) continue;
            if (pos < cap) {
                keys[pos] = slots[i * 4 + q];
                depths[pos] = qd.D[q];
            }
            ++pos;
        }
    });
    if (!keys) {
        if (mine) atomicAdd(&s_n, mine);
        __syncthreads();
        if (tid == 0 && s_n) atomicAdd(n_out, s_n);
    }
}

uint32_t depth_blocks(uint64_t n_slots) {
    const uint64_t quads = (n_slots + 3) / 4;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((quads + DCN_DEPTH_THREADS - 1) / DCN_DEPTH_THREADS,
                                                             (uint64_t)dcn_cu_count() * 8));
}

} // namespace

int dcn_launch_depth_count(const dcn_depth_args &a, hipStream_t stream) {
    return dcn_launch_dump_sweep(depth_count_kernel, a, "depth: tile count", stream);
}

int dcn_depth_stats(const dcn_index *set, unsigned long long *d_out, hipStream_t stream) {
    const uint64_t n_slots = set->n_groups * DCN_GROUP_SLOTS;
    hipLaunchKernelGGL(depth_stats_kernel, dim3(depth_blocks(n_slots)), dim3(DCN_DEPTH_THREADS), 0, stream, set->d_labels,
                       set->d_depth, n_slots, set->n_members, d_out);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_depth_hist(const dcn_index *set, uint32_t mask, uint32_t n_bins, unsigned long long *d_hist, hipStream_t stream) {
    if (n_bins < 2 || n_bins > DCN_DEPTH_MAX_BINS) return dcn_fail(DCN_ERR_INTERNAL, "depth: bin count");
    const uint64_t n_slots = set->n_groups * DCN_GROUP_SLOTS;
    hipLaunchKernelGGL(depth_hist_kernel, dim3(depth_blocks(n_slots)), dim3(DCN_DEPTH_THREADS), 0, stream, set->d_labels,
                       set->d_depth, n_slots, mask, n_bins, d_hist);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_depth_keys(const dcn_index *set, uint32_t mask, uint64_t *d_keys, uint32_t *d_depths, uint64_t cap,
                   unsigned long long *d_n, hipStream_t stream) {
    const uint64_t n_slots = set->n_groups * DCN_GROUP_SLOTS;
    hipLaunchKernelGGL(depth_keys_kernel, dim3(depth_blocks(n_slots)), dim3(DCN_DEPTH_THREADS), 0, stream, set->d_labels,
                       set->d_depth, (const uint64_t *)set->d_slots, n_slots, mask, d_keys, d_depths, cap, d_n);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}
