// set_algebra.hip -- set algebra on device tables beyond union and diff: keys of a labelled set
// chosen by their member mask, the overlap matrix of a set's members, and the intersection of indexes.
//
// The set sweeps stream d_labels only (4 bytes per slot, a lane taking 4 consecutive masks with one dwordx4); a key is
// read from d_slots only where its mask passed.  Every sweep is a grid-stride loop in wave-uniform steps, so that the
// ballots inside see whole waves.
#include "dcn_set_algebra.h"
#include "dcn_probe.h"
#include "dcn_table_insert.h"

#include <algorithm>

namespace {
constexpr uint32_t SA_THREADS = 256;

// the end of a counting sweep: the waves' sums meet in LDS, one global add per workgroup
__device__ inline void sa_flush_count(unsigned long long mine, unsigned long long *s_n, unsigned long long *n_out) {
    for (int d = DCN_WAVE / 2; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, DCN_WAVE);
    if ((threadIdx.x & (DCN_WAVE - 1)) == 0 && mine) atomicAdd(s_n, mine);
    __syncthreads();
    if (threadIdx.x == 0 && *s_n) atomicAdd(n_out, *s_n);
}

// BUILD = false: *n_out += slots whose mask passes.  BUILD = true: their keys go into dst, *n_out += fresh inserts.
template <bool BUILD>
__global__ __launch_bounds__(SA_THREADS) void set_select_kernel(const uint4 *labels4, uint64_t n_quads, dcn_select_pred p,
                                                               const uint64_t *src, uint64_t *dst, uint32_t dst_shift,
                                                               uint32_t dst_mask, unsigned long long *n_out) {
    __shared__ unsigned long long s_n;
    const uint32_t tid = threadIdx.x, lane = tid & (DCN_WAVE - 1);
    if (tid == 0) s_n = 0;
    __syncthreads();
    unsigned long long mine = 0;
    const uint64_t stride = (uint64_t)gridDim.x * SA_THREADS;
    for (uint64_t q0 = (uint64_t)blockIdx.x * SA_THREADS + (tid - lane); q0 < n_quads; q0 += stride) {
        const uint64_t q = q0 + lane;
        if (q >= n_quads) continue;
        const uint4 L = labels4[q];
        if ((L.x | L.y | L.z | L.w) == 0) continue;
        const uint32_t l[4] = {L.x, L.y, L.z, L.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!dcn_select_pass(l[u], p)) continue;
            if constexpr (BUILD)
                dcn_table_insert_dev(dst, dst_shift, dst_mask, src[4 * q + u], &mine);
            else
                ++mine;
        }
    }
    sa_flush_count(mine, &s_n, n_out);
}

// Masks with ONE bit (most of them) are tallied per member from ballots: lane j of the wave keeps member j's count, one
// add per wave and member, as cov_tally does (classify.hip).  Masks with several bits add into the workgroup's 32 x 32
// matrix in LDS, upper triangle only, and into its by-count row.  One global add per non-zero cell per workgroup.
__global__ __launch_bounds__(SA_THREADS) void set_overlap_kernel(const uint4 *labels4, uint64_t n_quads, uint32_t n,
                                                                unsigned long long *tally) {
    __shared__ unsigned long long s_tally[DCN_OVL_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & (DCN_WAVE - 1);
    for (uint32_t c = tid; c < DCN_OVL_WORDS; c += SA_THREADS) s_tally[c] = 0;
    __syncthreads();
    unsigned long long mine = 0; // lane j < n: slots whose mask is exactly 1 << j
    const uint64_t stride = (uint64_t)gridDim.x * SA_THREADS;
    for (uint64_t q0 = (uint64_t)blockIdx.x * SA_THREADS + (tid - lane); q0 < n_quads; q0 += stride) {
        const uint64_t q = q0 + lane;
        const uint4 L = q < n_quads ? labels4[q] : uint4{0, 0, 0, 0};
        if (!__ballot((L.x | L.y | L.z | L.w) != 0)) continue;
        const uint32_t l[4] = {L.x, L.y, L.z, L.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t v = l[u];
            const bool several = (v & (v - 1)) != 0;
            const uint32_t one = several ? 0u : v;
            if (__ballot(one != 0)) {
                for (uint32_t j = 0; j < n; ++j) {
                    const unsigned long long b = __ballot((one >> j) & 1u);
                    if (lane == j) mine += __popcll(b);
                }
            }
            if (several) {
                atomicAdd(&s_tally[DCN_OVL_COUNT + __popc(v) - 1], 1ull);
                for (uint32_t a = v; a; a &= a - 1) {
                    const uint32_t i = __ffs(a) - 1;
                    for (uint32_t b = a; b; b &= b - 1) atomicAdd(&s_tally[i * DCN_MAX_SET_MEMBERS + (__ffs(b) - 1)], 1ull);
                }
            }
        }
    }
    if (lane < n && mine) atomicAdd(&s_tally[DCN_OVL_SINGLE + lane], mine);
    __syncthreads();
    for (uint32_t c = tid; c < DCN_OVL_WORDS; c += SA_THREADS)
        if (s_tally[c]) atomicAdd(&tally[c], s_tally[c]);
}

// one wave per 64 slots of src: a lane's key is probed in every other table, the wave's ballot is the bitmap word
__global__ __launch_bounds__(SA_THREADS) void intersect_mark_kernel(const uint64_t *src, uint64_t n_slots,
                                                                   const dcn_table_view *others, uint32_t n_others,
                                                                   unsigned long long *bits, unsigned long long *n_out) {
    __shared__ unsigned long long s_n;
    const uint32_t tid = threadIdx.x, lane = tid & (DCN_WAVE - 1);
    if (tid == 0) s_n = 0;
    __syncthreads();
    unsigned long long mine = 0;
    const uint64_t stride = (uint64_t)gridDim.x * SA_THREADS;
    for (uint64_t s0 = (uint64_t)blockIdx.x * SA_THREADS + (tid - lane); s0 < n_slots; s0 += stride) {
        const uint64_t i = s0 + lane;
        const uint64_t key = i < n_slots ? src[i] : 0;
        bool hit = key != 0;
        for (uint32_t o = 0; o < n_others && __ballot(hit); ++o)
            if (hit) hit = dcn_table_contains_dev(others[o], key);
        const unsigned long long m = __ballot(hit);
        if (lane == 0) {
            bits[s0 >> 6] = m;
            mine += __popcll(m);
        }
    }
    sa_flush_count(mine, &s_n, n_out);
}

__global__ __launch_bounds__(SA_THREADS) void intersect_build_kernel(const uint64_t *src, uint64_t n_slots,
                                                                    const unsigned long long *bits, uint64_t *dst,
                                                                    uint32_t dst_shift, uint32_t dst_mask,
                                                                    unsigned long long *n_out) {
    __shared__ unsigned long long s_n;
    const uint32_t tid = threadIdx.x, lane = tid & (DCN_WAVE - 1);
    if (tid == 0) s_n = 0;
    __syncthreads();
    unsigned long long mine = 0;
    const uint64_t stride = (uint64_t)gridDim.x * SA_THREADS;
    for (uint64_t s0 = (uint64_t)blockIdx.x * SA_THREADS + (tid - lane); s0 < n_slots; s0 += stride) {
        const unsigned long long m = bits[s0 >> 6];
        if ((m >> lane) & 1ull) dcn_table_insert_dev(dst, dst_shift, dst_mask, src[s0 + lane], &mine);
    }
    sa_flush_count(mine, &s_n, n_out);
}

// a grid over the device's CUs, a few workgroups each; the loops stride over the rest
uint32_t sa_blocks(uint64_t items) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + SA_THREADS - 1) / SA_THREADS, (uint64_t)dcn_cu_count() * 8));
}

// the set's masks as quads: the table has a power-of-two number of groups, at least 64, so its slots come in fours
int label_quads(const dcn_index *set, uint64_t *n_quads) {
    const uint64_t n_slots = set->n_groups * DCN_GROUP_SLOTS;
    if (n_slots % 4 != 0) return dcn_fail(DCN_ERR_INTERNAL, "set algebra: the set's slot count is not a multiple of 4");
    *n_quads = n_slots / 4;
    return DCN_OK;
}
} // namespace

int dcn_set_overlap_sweep(const dcn_index *set, unsigned long long *d_tally) {
    uint64_t n_quads = 0;
    int rc = label_quads(set, &n_quads);
    if (rc != DCN_OK) return rc;
    hipLaunchKernelGGL(set_overlap_kernel, dim3(sa_blocks(n_quads)), dim3(SA_THREADS), 0, 0, (const uint4 *)set->d_labels,
                       n_quads, set->n_members, d_tally);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_set_select_sweep(const dcn_index *set, const dcn_select_pred &pred, dcn_index *dst, unsigned long long *d_n) {
    uint64_t n_quads = 0;
    int rc = label_quads(set, &n_quads);
    if (rc != DCN_OK) return rc;
    const uint4 *labels4 = (const uint4 *)set->d_labels;
    if (dst) {
        const dcn_table_view dv = dst->view();
        hipLaunchKernelGGL(set_select_kernel<true>, dim3(sa_blocks(n_quads)), dim3(SA_THREADS), 0, 0, labels4, n_quads, pred,
                           set->d_slots, dst->d_slots, dv.group_shift, dv.group_mask, d_n);
    } else {
        hipLaunchKernelGGL(set_select_kernel<false>, dim3(sa_blocks(n_quads)), dim3(SA_THREADS), 0, 0, labels4, n_quads, pred,
                           (const uint64_t *)nullptr, (uint64_t *)nullptr, 0u, 0u, d_n);
    }
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_intersect_mark(const dcn_index *src, const dcn_table_view *d_others, uint32_t n_others, unsigned long long *d_bits,
                       unsigned long long *d_n) {
    const uint64_t n_slots = src->n_groups * DCN_GROUP_SLOTS;
    if (n_slots % DCN_WAVE != 0) return dcn_fail(DCN_ERR_INTERNAL, "intersect: the table's slot count is not a multiple of 64");
    hipLaunchKernelGGL(intersect_mark_kernel, dim3(sa_blocks(n_slots)), dim3(SA_THREADS), 0, 0, src->d_slots, n_slots, d_others,
                       n_others, d_bits, d_n);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_intersect_build(const dcn_index *src, const unsigned long long *d_bits, dcn_index *dst, unsigned long long *d_n) {
    const uint64_t n_slots = src->n_groups * DCN_GROUP_SLOTS;
    const dcn_table_view dv = dst->view();
    hipLaunchKernelGGL(intersect_build_kernel, dim3(sa_blocks(n_slots)), dim3(SA_THREADS), 0, 0, src->d_slots, n_slots, d_bits,
                       dst->d_slots, dv.group_shift, dv.group_mask, d_n);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}
