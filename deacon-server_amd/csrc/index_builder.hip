// index_builder.hip -- the kernels of the counting index build (dcn_index_builder_*; the definition is in
// include/deacon_hip.h, the layout in dcn_index_builder.h).
//
// Runs behind the index side's front end (pack with the index-side codes -> plan -> scan in dump mode with chunk-absolute
// positions), where the plain build runs insert_dump_kernel:
//   builder_count_kernel  a flat grid-stride sweep over all slots of dump_valid, as insert_dump_kernel.  Per valid entry that
//                         passes the entropy floor: claim the entry's position in the chunk's position bitmap
//                         (dcn_bit_claim, dcn_dump_sweep.h), make the key a member
//                         (dcn_table_insert_dev gives the slot) and add 1 to the slot's 16-bit counter, saturating.  The dump
//                         may hold a position more than once (two windows can choose the same k-mer with another between
//                         them; two pieces of a cut sequence can choose the same k-mer of their overlap): an occurrence is a
//                         (sequence, position) pair, hence the bitmap rather than a count of entries.
//   builder_seam_kernel   the bits of a chunk's last l-1 bases, to and from the builder's seam words (the next chunk opens
//                         with the piece that continues there)
//   builder_rehash_kernel growth: every key into the larger table, its counter into its new slot's half
//   builder_hist_kernel / builder_export_kernel / builder_select_kernel
//                         sweeps over slots and counters together, four slots per lane (two 16-byte loads of keys, one
//                         8-byte load of counters), grid-stride in wave-uniform steps, tallies in LDS, one global atomic per
//                         output cell per workgroup (export: one returning atomicAdd per wave).
#include "dcn_index_builder.h"
#include "dcn_entropy.h"
#include "dcn_table_insert.h"

#include <algorithm>

namespace {

// the end of a counting sweep: the waves' sums meet in LDS, one global add per workgroup
__device__ inline void builder_flush(unsigned long long mine, unsigned long long *s_n, unsigned long long *n_out) {
    for (int d = DCN_WAVE / 2; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, DCN_WAVE);
    if ((threadIdx.x & (DCN_WAVE - 1)) == 0 && mine) atomicAdd(s_n, mine);
    __syncthreads();
    if (threadIdx.x == 0 && *s_n) atomicAdd(n_out, *s_n);
}

__global__ __launch_bounds__(DCN_BUILDER_THREADS) void builder_count_kernel(dcn_builder_count_args a) {
    __shared__ unsigned long long s_fresh, s_occ;
    if (threadIdx.x == 0) s_fresh = 0, s_occ = 0;
    __syncthreads();
    unsigned long long fresh = 0, occ = 0;
    const uint64_t stride = (uint64_t)gridDim.x * DCN_BUILDER_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * DCN_BUILDER_THREADS + threadIdx.x; i < a.n_bases; i += stride) {
        if (a.dump_valid[i] != 1) continue;
        const uint64_t p = a.dump_pos[i];
        if (p + a.k > a.n_bases) continue; // (a k-mer of the chunk lies inside it)
        if (a.entropy_threshold != 0.0f && scaled_entropy_dev(a.ascii + p, a.k) < a.entropy_threshold) continue;
        if (!dcn_bit_claim(a.bits, p)) continue;
        ++occ;
        const uint64_t key = a.dump_hash[i];
        if (key == 0) {
            if (__atomic_load_n(&a.tally[2], __ATOMIC_RELAXED) == 0) atomicExch(&a.tally[2], 1ull);
            dcn_depth_add(a.counts_zero, 0);
            continue;
        }
        const uint64_t slot = dcn_table_insert_dev(a.slots, a.group_shift, a.group_mask, key, &fresh);
        dcn_depth_add(a.counts + (slot >> 1), (uint32_t)(slot & 1) * 16);
    }
    builder_flush(fresh, &s_fresh, &a.tally[0]);
    builder_flush(occ, &s_occ, &a.tally[1]);
}

__global__ __launch_bounds__(DCN_BUILDER_MAX_SEAM) void builder_seam_kernel(const uint32_t *src, uint64_t src0, uint32_t *dst,
                                                                           uint64_t dst0, uint32_t n) {
    const uint32_t t = threadIdx.x;
    if (t >= n) return;
    const uint64_t s = src0 + t, d = dst0 + t;
    if ((src[s >> 5] >> (s & 31)) & 1u) atomicOr(dst + (d >> 5), 1u << (d & 31));
}

__global__ __launch_bounds__(DCN_BUILDER_THREADS) void builder_rehash_kernel(const uint64_t *old_slots, const uint32_t *old_counts,
                                                                             uint64_t old_n, uint64_t *slots, uint32_t group_shift,
                                                                             uint32_t group_mask, uint32_t *new_counts) {
    const uint64_t stride = (uint64_t)gridDim.x * DCN_BUILDER_THREADS;
    unsigned long long fresh = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * DCN_BUILDER_THREADS + threadIdx.x; i < old_n; i += stride) {
        const uint64_t key = old_slots[i];
        if (key == 0) continue;
        const uint32_t c = (old_counts[i >> 1] >> ((i & 1) * 16)) & DCN_DEPTH_MAX;
        const uint64_t slot = dcn_table_insert_dev(slots, group_shift, group_mask, key, &fresh);
        // (a key has one slot and one mover: the other half of the word belongs to another lane, hence the atomic)
        atomicOr(new_counts + (slot >> 1), c << ((slot & 1) * 16));
    }
}

// ---- sweeps -------------------------------------------------------------------------------------------------------
// keys and counts of slots 4q .. 4q+3 (an empty slot: key 0, count 0)
struct builder_quad {
    uint64_t K[4];
    uint32_t C[4];
};

// the wave-uniform grid-stride loop of the sweeps: body(qd) sees this lane's quad (all empty past the table)
template <typename F>
__device__ inline void builder_for_quads(const uint64_t *slots, const uint32_t *counts, uint64_t n_quads, uint32_t tid,
                                         uint32_t lane, F body) {
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    const uint64_t stride = (uint64_t)gridDim.x * DCN_BUILDER_THREADS;
    for (uint64_t q0 = (uint64_t)blockIdx.x * DCN_BUILDER_THREADS + (tid - lane); q0 < n_quads; q0 += stride) {
        const uint64_t q = q0 + lane;
        builder_quad r = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        if (q < n_quads) {
            const u64x2 a = *reinterpret_cast<const u64x2 *>(slots + 4 * q), b = *reinterpret_cast<const u64x2 *>(slots + 4 * q + 2);
            const uint2 d = *reinterpret_cast<const uint2 *>(counts + 2 * q);
            r.K[0] = a.x, r.K[1] = a.y, r.K[2] = b.x, r.K[3] = b.y;
            r.C[0] = d.x & DCN_DEPTH_MAX, r.C[1] = d.x >> 16, r.C[2] = d.y & DCN_DEPTH_MAX, r.C[3] = d.y >> 16;
        }
        body(r);
    }
}

__global__ __launch_bounds__(DCN_BUILDER_THREADS) void builder_hist_kernel(const uint64_t *slots, const uint32_t *counts,
                                                                           uint64_t n_quads, uint32_t n_bins,
                                                                           unsigned long long *hist) {
    __shared__ uint32_t s_hist[DCN_DEPTH_MAX_BINS];
    __shared__ unsigned long long s_one; // bin 1, the keys seen once: most of a genome's, kept out of the LDS atomics
    const uint32_t tid = threadIdx.x, lane = tid & (DCN_WAVE - 1);
    for (uint32_t b = tid; b < n_bins; b += DCN_BUILDER_THREADS) s_hist[b] = 0;
    if (tid == 0) s_one = 0;
    __syncthreads();
    unsigned long long one = 0;
    builder_for_quads(slots, counts, n_quads, tid, lane, [&](const builder_quad &qd) {
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
            if (!qd.K[u]) continue;
            if (qd.C[u] == 1) ++one;
            else atomicAdd(&s_hist[min(qd.C[u], n_bins - 1)], 1u);
        }
    });
    if (one) atomicAdd(&s_one, one);
    __syncthreads();
    for (uint32_t b = tid; b < n_bins; b += DCN_BUILDER_THREADS) {
        const unsigned long long v = s_hist[b] + (b == 1 ? s_one : 0ull);
        if (v) atomicAdd(&hist[b], v);
    }
}

__global__ __launch_bounds__(DCN_BUILDER_THREADS) void builder_export_kernel(const uint64_t *slots, const uint32_t *counts,
                                                                             uint64_t n_quads, uint64_t *keys, uint32_t *out_counts,
                                                                             uint64_t cap, unsigned long long *n_out) {
    const uint32_t tid = threadIdx.x, lane = tid & (DCN_WAVE - 1);
    builder_for_quads(slots, counts, n_quads, tid, lane, [&](const builder_quad &qd) {
        uint32_t c = 0;
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) c += qd.K[u] ? 1u : 0u;
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
        for (uint32_t u = 0; u < 4; ++u) {
            if (!qd.K[u]) continue;
            if (pos < cap) {
                keys[pos] = qd.K[u];
                out_counts[pos] = qd.C[u];
            }
            ++pos;
        }
    });
}

// BUILD = false: *n_out += occupied slots with lo <= count <= hi.  BUILD = true: their keys go into dst, *n_out += fresh inserts.
template <bool BUILD>
__global__ __launch_bounds__(DCN_BUILDER_THREADS) void builder_select_kernel(const uint64_t *slots, const uint32_t *counts,
                                                                             uint64_t n_quads, uint32_t lo, uint32_t hi, uint64_t *dst,
                                                                             uint32_t dst_shift, uint32_t dst_mask,
                                                                             unsigned long long *n_out) {
    __shared__ unsigned long long s_n;
    const uint32_t tid = threadIdx.x, lane = tid & (DCN_WAVE - 1);
    if (tid == 0) s_n = 0;
    __syncthreads();
    unsigned long long mine = 0;
    builder_for_quads(slots, counts, n_quads, tid, lane, [&](const builder_quad &qd) {
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
            if (!qd.K[u] || qd.C[u] < lo || qd.C[u] > hi) continue;
            if constexpr (BUILD)
                dcn_table_insert_dev(dst, dst_shift, dst_mask, qd.K[u], &mine);
            else
                ++mine;
        }
    });
    builder_flush(mine, &s_n, n_out);
}

// a grid over the device's CUs, a few workgroups each; the loops stride over the rest
uint32_t builder_blocks(uint64_t items) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + DCN_BUILDER_THREADS - 1) / DCN_BUILDER_THREADS,
                                                             (uint64_t)dcn_cu_count() * 8));
}

// the table as quads: it has a power-of-two number of groups, at least 64, so its slots come in fours
int builder_quads(const dcn_index_builder *b, uint64_t *n_quads) {
    const uint64_t n_slots = b->idx.n_groups * DCN_GROUP_SLOTS;
    if (n_slots % 4 != 0) return dcn_fail(DCN_ERR_INTERNAL, "index builder: the table's slot count is not a multiple of 4");
    *n_quads = n_slots / 4;
    return DCN_OK;
}

} // namespace

int dcn_launch_builder_count(const dcn_builder_count_args &a, hipStream_t stream) {
    if (a.n_bases == 0) return DCN_OK;
    if (a.entropy_threshold != 0.0f) {
        const int rc = dcn_entropy_table_ready();
        if (rc != DCN_OK) return rc;
    }
    hipLaunchKernelGGL(builder_count_kernel, dim3(builder_blocks(a.n_bases)), dim3(DCN_BUILDER_THREADS), 0, stream, a);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_builder_seam(const uint32_t *src, uint64_t src0, uint32_t *dst, uint64_t dst0, uint32_t n, hipStream_t stream) {
    if (n == 0) return DCN_OK;
    if (n > DCN_BUILDER_MAX_SEAM) return dcn_fail(DCN_ERR_INTERNAL, "index builder: seam longer than k + w allows");
    hipLaunchKernelGGL(builder_seam_kernel, dim3(1), dim3(DCN_BUILDER_MAX_SEAM), 0, stream, src, src0, dst, dst0, n);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_builder_rehash(const uint64_t *old_slots, const uint32_t *old_counts, uint64_t old_n_slots, uint64_t *slots,
                       uint32_t group_shift, uint32_t group_mask, uint32_t *new_counts, hipStream_t stream) {
    hipLaunchKernelGGL(builder_rehash_kernel, dim3(builder_blocks(old_n_slots)), dim3(DCN_BUILDER_THREADS), 0, stream, old_slots,
                       old_counts, old_n_slots, slots, group_shift, group_mask, new_counts);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_builder_hist(const dcn_index_builder *b, uint32_t n_bins, unsigned long long *d_hist, hipStream_t stream) {
    if (n_bins < 2 || n_bins > DCN_DEPTH_MAX_BINS) return dcn_fail(DCN_ERR_INTERNAL, "index builder: bin count");
    uint64_t n_quads = 0;
    int rc = builder_quads(b, &n_quads);
    if (rc != DCN_OK) return rc;
    hipLaunchKernelGGL(builder_hist_kernel, dim3(builder_blocks(n_quads)), dim3(DCN_BUILDER_THREADS), 0, stream, b->idx.d_slots,
                       b->d_counts, n_quads, n_bins, d_hist);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_builder_export(const dcn_index_builder *b, uint64_t *d_keys, uint32_t *d_counts, uint64_t cap, unsigned long long *d_n,
                       hipStream_t stream) {
    uint64_t n_quads = 0;
    int rc = builder_quads(b, &n_quads);
    if (rc != DCN_OK) return rc;
    hipLaunchKernelGGL(builder_export_kernel, dim3(builder_blocks(n_quads)), dim3(DCN_BUILDER_THREADS), 0, stream, b->idx.d_slots,
                       b->d_counts, n_quads, d_keys, d_counts, cap, d_n);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_builder_select(const dcn_index_builder *b, uint32_t lo, uint32_t hi, dcn_index *dst, unsigned long long *d_n,
                       hipStream_t stream) {
    uint64_t n_quads = 0;
    int rc = builder_quads(b, &n_quads);
    if (rc != DCN_OK) return rc;
    const dim3 grid(builder_blocks(n_quads)), block(DCN_BUILDER_THREADS);
    if (dst) {
        const dcn_table_view dv = dst->view();
        hipLaunchKernelGGL(builder_select_kernel<true>, grid, block, 0, stream, b->idx.d_slots, b->d_counts, n_quads, lo, hi,
                           dst->d_slots, dv.group_shift, dv.group_mask, d_n);
    } else {
        hipLaunchKernelGGL(builder_select_kernel<false>, grid, block, 0, stream, b->idx.d_slots, b->d_counts, n_quads, lo, hi,
                           (uint64_t *)nullptr, 0u, 0u, d_n);
    }
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}
