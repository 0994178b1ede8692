// classify.hip -- labelled index sets and per-member classification of a batch (dcn_index_set_create,
// dcn_classify_batch*).
//
// A set is one open-addressing table over the union of its members' keys (the slot layout of index_table.hip) with a
// parallel u32 array of member masks.  A probe reads the home group as dcn_table_contains_dev does; a hit reads the
// 4-byte label at the slot it matched, so one probe answers "which members hold this key" for up to 32 members.
//
// Classification runs on the minimizer dump of the batch (scan_kernel<..., DUMP=true>, which leaves every window's
// minimizer hash and its ACGT flag in the dump arrays) and then:
//   classify_units_kernel  one lane per unit: walks the unit's tiles, counts the valid entries (total), probes the set
//                          for each, keeps the distinct hits of the unit in an LDS list and their member bits in LDS
//                          counters, applies the thresholds per member.  A unit with more entries than the lane takes,
//                          or more distinct hits than its list holds, is appended to a work list instead.
//   classify_big_kernel    one workgroup per listed unit: the same counts with an LDS hash set, in hash partitions
//                          sized so that each fits the set (more partitions if one overflows): exact for any unit size,
//                          without global scratch.
// Both take COV: with a coverage bitmap on the set (dcn_index_set_coverage_enable), every hit a unit counts as fresh
// also sets its slot's bit; the COV = false instantiations are the kernels without coverage, instruction for instruction.
// The coverage sweeps (dcn_index_set_coverage*) count and list the marked slots per member.
#include "dcn_classify.h"
#include "dcn_probe.h"
#include "dcn_table_insert.h"

#include <algorithm>

namespace {

__device__ inline uint32_t set_slot_label(const dcn_classify_args &a, uint32_t g, uint32_t s) {
    return a.labels[(uint64_t)g * DCN_GROUP_SLOTS + s];
}

// member mask of `key` (non-zero) whose home group g has been loaded into grp: 0 = in no member
__device__ inline uint32_t set_label_from(const dcn_classify_args &a, uint64_t key, uint32_t g, dcn_group grp) {
    for (;;) {
        if (grp.a.x == key) return set_slot_label(a, g, 0);
        if (grp.a.y == key) return set_slot_label(a, g, 1);
#if DCN_GROUP_SLOTS == 4
        if (grp.b.x == key) return set_slot_label(a, g, 2);
        if (grp.b.y == key) return set_slot_label(a, g, 3);
        if (grp.a.x == 0 || grp.a.y == 0 || grp.b.x == 0 || grp.b.y == 0) return 0;
#else
        if (grp.a.x == 0 || grp.a.y == 0) return 0;
#endif
        g = (g + 1) & a.table.group_mask;
        grp = dcn_load_group(a.table, g);
    }
}

// slot index of `key` (non-zero) in the set, ~0 when it is in no member (the walk is dcn_probe.h's, shared with depth.hip)
__device__ inline uint64_t set_find_slot(const dcn_classify_args &a, uint64_t key, uint32_t g, dcn_group grp) {
    return dcn_table_find_slot(a.table, key, g, grp);
}

__device__ inline uint32_t set_label(const dcn_classify_args &a, uint64_t key) {
    if (key == 0) return a.zero_label;
    const uint32_t g = dcn_group_of(key, a.table.group_shift, a.table.group_mask);
    return set_label_from(a, key, g, dcn_load_group(a.table, g));
}

// coverage: the bitmap word and bit of slot `at` (~0 = key 0, whose word is its own)
__device__ inline uint32_t *cov_word(const dcn_classify_args &a, uint64_t at) {
    return at == ~0ull ? a.cov_zero : a.cov_bits + (at >> 5);
}
__device__ inline uint32_t cov_bit(uint64_t at) { return at == ~0ull ? 1u : 1u << (at & 31); }
// test, then set: `seen` is a plain load of the word; the atomic is issued only for a bit that was clear there (a key
// that repeats across the batch's units -- most of them on host-heavy input -- costs a load and no atomic).  A stale
// `seen` only costs a redundant OR, and OR is idempotent: a unit marked twice (the lane kernel's hand-off of an `over`
// unit to the workgroup kernel, a partition retry there) marks what it marked once.
__device__ inline void cov_mark(const dcn_classify_args &a, uint64_t at, uint32_t seen) {
    const uint32_t bit = cov_bit(at);
    if (!(seen & bit)) atomicOr(cov_word(a, at), bit);
}

__device__ inline void unit_reads(const dcn_classify_args &a, uint32_t u, uint32_t *r0, uint32_t *r1) {
    *r0 = a.unit_first_read ? a.unit_first_read[u] : u;
    *r1 = a.unit_first_read ? a.unit_first_read[u + 1] : u + 1;
}

__device__ inline void write_unit(const dcn_classify_args &a, uint32_t u, uint32_t total, uint32_t match) {
    if (a.total) a.total[u] = total;
    a.match[u] = match;
}

template <bool COV>
__global__ __launch_bounds__(DCN_CLS_LANES) void classify_units_kernel(dcn_classify_args a) {
    __shared__ uint64_t s_hash[DCN_CLS_LANE_HITS][DCN_CLS_LANES];
    __shared__ uint8_t s_cnt[DCN_MAX_SET_MEMBERS][DCN_CLS_LANES];
    const uint32_t lane = threadIdx.x, u = blockIdx.x * DCN_CLS_LANES + lane;
    if (u >= a.n_units) return;
    const uint32_t n = a.n_members;
    if (a.status->bad_offsets) { // tiles and read ranges are not looked at (ctx.hip reports DCN_ERR_ARG)
        if (u == 0) a.report->bad_offsets = 1;
        write_unit(a, u, 0, 0);
        if (a.hits)
            for (uint32_t j = 0; j < n; ++j) a.hits[(uint64_t)u * n + j] = 0;
        return;
    }
    const uint32_t NT = *a.n_tiles, tw = a.tile_windows;
    uint32_t r0, r1;
    unit_reads(a, u, &r0, &r1);
    uint32_t n_entries = 0;
    for (uint32_t r = r0; r < r1; ++r) {
        const uint32_t first = a.read_tile_first[r], ntl = a.read_tiles[r];
        for (uint32_t j = 0; j < ntl && first + j < NT; ++j) n_entries += a.dump_count[first + j];
    }
    if (n_entries > DCN_CLS_LANE_ENTRIES) {
        a.big[atomicAdd(a.n_big, 1u)] = u;
        return;
    }
    for (uint32_t j = 0; j < n; ++j) s_cnt[j][lane] = 0;
    uint32_t tot = 0, nh = 0;
    bool over = false;
    uint64_t hb[4];
    uint32_t nb = 0;
    // probes of up to four entries are issued together: their home groups are loaded before any is resolved, and the
    // labels of the hits among them before any is counted
    auto flush = [&]() {
        dcn_group gr[4];
        uint32_t gi[4];
        uint32_t m[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            if (i < nb && hb[i] != 0) {
                gi[i] = dcn_group_of(hb[i], a.table.group_shift, a.table.group_mask);
                gr[i] = dcn_load_group(a.table, gi[i]);
            }
        }
        uint64_t at[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) at[i] = (i < nb && hb[i] != 0) ? set_find_slot(a, hb[i], gi[i], gr[i]) : ~0ull;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) m[i] = at[i] != ~0ull ? a.labels[at[i]] : (i < nb && hb[i] == 0 ? a.zero_label : 0u);
        // COV: the bitmap words of the hits among them, loaded together (key 0 hits with at == ~0: its own word)
        uint32_t seen[4];
        if constexpr (COV) {
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) seen[i] = (i < nb && m[i]) ? *cov_word(a, at[i]) : ~0u;
        }
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            if (i >= nb || over || !m[i]) continue;
            const uint64_t h = hb[i];
            bool dup = false;
            for (uint32_t q = 0; q < nh && !dup; ++q) dup = s_hash[q][lane] == h;
            if (dup) continue;
            if (nh == DCN_CLS_LANE_HITS) {
                over = true;
                continue;
            }
            s_hash[nh++][lane] = h;
            if constexpr (COV) cov_mark(a, at[i], seen[i]);
            for (uint32_t mm = m[i]; mm; mm &= mm - 1) s_cnt[__ffs(mm) - 1][lane]++;
        }
        nb = 0;
    };
    for (uint32_t r = r0; r < r1 && !over; ++r) {
        const uint64_t off = a.offsets[r];
        const uint32_t first = a.read_tile_first[r], ntl = a.read_tiles[r];
        for (uint32_t j = 0; j < ntl && first + j < NT && !over; ++j) {
            const uint64_t base = off + (uint64_t)j * tw; // the tile's entries (scan_start + carry)
            const uint32_t cnt = a.dump_count[first + j];
            for (uint32_t e0 = 0; e0 < cnt && !over; e0 += 4) {
                // four entries' flags and hashes loaded before any is looked at
                uint8_t v[4];
                uint64_t hv[4];
#pragma unroll
                for (uint32_t i = 0; i < 4; ++i) {
                    const bool in = e0 + i < cnt;
                    v[i] = in ? a.dump_valid[base + e0 + i] : 0;
                    hv[i] = in ? a.dump_hash[base + e0 + i] : 0;
                }
#pragma unroll
                for (uint32_t i = 0; i < 4; ++i) {
                    if (!v[i] || over) continue;
                    ++tot;
#pragma unroll
                    for (uint32_t q = 0; q < 4; ++q) // (constant indices: hb stays in registers)
                        if (q == nb) hb[q] = hv[i];
                    if (++nb == 4) flush();
                }
            }
        }
    }
    if (nb && !over) flush();
    if (over) {
        a.big[atomicAdd(a.n_big, 1u)] = u;
        return;
    }
    uint32_t match = 0;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t c = s_cnt[j][lane];
        if (a.hits) a.hits[(uint64_t)u * n + j] = c;
        if (dcn_decide(c, tot, a.abs_threshold, a.rel_threshold, 0)) match |= 1u << j;
    }
    write_unit(a, u, tot, match);
}

// every valid dump entry of unit u's reads, spread over the workgroup's threads: BODY sees `h` (its hash)
#define DCN_CLS_FOR_ENTRIES(BODY)                                                                                  \
    for (uint32_t r = r0; r < r1; ++r) {                                                                           \
        const uint64_t off = a.offsets[r];                                                                         \
        const uint32_t first = a.read_tile_first[r];                                                               \
        const uint64_t span = (uint64_t)a.read_tiles[r] * tw;                                                      \
        for (uint64_t s = tid; s < span; s += DCN_CLS_BIG_THREADS) {                                               \
            const uint32_t j = (uint32_t)(s / tw), e = (uint32_t)(s - (uint64_t)j * tw);                           \
            if (first + j >= NT || e >= a.dump_count[first + j] || !a.dump_valid[off + s]) continue;               \
            const uint64_t h = a.dump_hash[off + s];                                                               \
            BODY                                                                                                   \
        }                                                                                                          \
    }

// COV: the member mask of h through set_find_slot, whose slot (~0 for key 0 or a miss) *at receives; else set_label
template <bool COV>
__device__ inline uint32_t big_label(const dcn_classify_args &a, uint64_t h, uint64_t *at) {
    if constexpr (COV) {
        *at = ~0ull;
        if (h == 0) return a.zero_label;
        const uint32_t g = dcn_group_of(h, a.table.group_shift, a.table.group_mask);
        *at = set_find_slot(a, h, g, dcn_load_group(a.table, g));
        return *at != ~0ull ? a.labels[*at] : 0u;
    } else {
        (void)at;
        return set_label(a, h);
    }
}

template <bool COV>
__global__ __launch_bounds__(DCN_CLS_BIG_THREADS) void classify_big_kernel(dcn_classify_args a) {
    __shared__ unsigned long long s_set[DCN_CLS_SET];
    __shared__ uint32_t s_cnt[DCN_MAX_SET_MEMBERS];
    __shared__ uint32_t s_tot, s_fill, s_over, s_zero;
    if (a.status->bad_offsets) return;
    const uint32_t tid = threadIdx.x, n = a.n_members, NB = *a.n_big;
    const uint32_t NT = *a.n_tiles, tw = a.tile_windows;
    constexpr uint32_t HALF = DCN_CLS_SET / 2, FULL = DCN_CLS_SET * 3 / 4;
    for (uint32_t item = blockIdx.x; item < NB; item += gridDim.x) {
        const uint32_t u = a.big[item];
        uint32_t r0, r1;
        unit_reads(a, u, &r0, &r1);
        if (tid == 0) s_tot = 0;
        __syncthreads();
        uint32_t mine = 0;
        DCN_CLS_FOR_ENTRIES({ (void)h; ++mine; })
        if (mine) atomicAdd(&s_tot, mine);
        __syncthreads();
        const uint32_t tot = s_tot;
        // hash partitions of at most ~HALF entries each: partition p takes the hashes whose mixed top bits fall in it
        uint32_t P = max(1u, (tot + HALF - 1) / HALF);
        for (;;) {
            if (tid < DCN_MAX_SET_MEMBERS) s_cnt[tid] = 0;
            if (tid == 0) {
                s_over = 0;
                s_zero = 0;
            }
            for (uint32_t p = 0; p < P; ++p) {
                for (uint32_t i = tid; i < DCN_CLS_SET; i += DCN_CLS_BIG_THREADS) s_set[i] = 0;
                if (tid == 0) s_fill = 0;
                __syncthreads();
                DCN_CLS_FOR_ENTRIES({
                    if (P > 1 && dcn_cls_partition(h, P) != p) continue;
                    uint64_t at;
                    uint32_t m = big_label<COV>(a, h, &at);
                    if (!m) continue;
                    bool fresh = false;
                    if (h == 0) {
                        fresh = atomicExch(&s_zero, 1u) == 0u;
                    } else {
                        uint32_t slot = (uint32_t)h & (DCN_CLS_SET - 1);
                        for (;;) {
                            const unsigned long long cur = s_set[slot];
                            if (cur == h) break;
                            if (cur == 0) {
                                // a fill limit below the set size keeps every walk finite; crossing it redoes the
                                // unit with twice the partitions
                                if (atomicAdd(&s_fill, 1u) >= FULL) {
                                    s_over = 1;
                                    break;
                                }
                                const unsigned long long old = atomicCAS(&s_set[slot], 0ull, (unsigned long long)h);
                                if (old == 0) {
                                    fresh = true;
                                    break;
                                }
                                if (old == h) break;
                            }
                            slot = (slot + 1) & (DCN_CLS_SET - 1);
                        }
                    }
                    if (fresh) {
                        if constexpr (COV) cov_mark(a, at, *cov_word(a, at));
                        while (m) {
                            atomicAdd(&s_cnt[__ffs(m) - 1], 1u);
                            m &= m - 1;
                        }
                    }
                })
                __syncthreads();
                if (s_over) break;
            }
            const bool again = s_over != 0;
            __syncthreads();
            if (!again) break;
            P *= 2;
        }
        if (tid < n && a.hits) a.hits[(uint64_t)u * n + tid] = s_cnt[tid];
        if (tid == 0) {
            uint32_t match = 0;
            for (uint32_t j = 0; j < n; ++j)
                if (dcn_decide(s_cnt[j], tot, a.abs_threshold, a.rel_threshold, 0)) match |= 1u << j;
            write_unit(a, u, tot, match);
        }
        __syncthreads();
    }
}
#undef DCN_CLS_FOR_ENTRIES

// ---- coverage sweeps ---------------------------------------------------------------------------------------------
constexpr uint32_t DCN_COV_THREADS = 256;

// lane j of the wave (j < n) adds the wave's count of labels with bit j: one ballot per member (a bit-slice of the 64
// lanes' labels), its popcount kept by the lane of that member
__device__ inline void cov_tally(uint32_t L, uint32_t n, uint32_t lane, unsigned long long *mine) {
    if (!__ballot(L != 0)) return;
#pragma unroll
    for (uint32_t j = 0; j < DCN_MAX_SET_MEMBERS; ++j) {
        if (j < n) {
            const unsigned long long b = __ballot((L >> j) & 1u);
            if (lane == j) *mine += __popcll(b);
        }
    }
}

// per member j: counts[j] += marked slots (ALL: occupied slots) whose label has bit j.  Grid-stride in wave-uniform
// steps over bitmap words (ALL: over slots); one LDS add per member per wave, one global add per member per workgroup.
template <bool ALL>
__global__ __launch_bounds__(DCN_COV_THREADS) void coverage_count_kernel(const uint32_t *bits, uint64_t n_words,
                                                                         const uint32_t *labels, uint64_t n_slots,
                                                                         uint32_t n, unsigned long long *counts) {
    __shared__ unsigned long long s_cnt[DCN_MAX_SET_MEMBERS];
    const uint32_t tid = threadIdx.x, lane = tid & (DCN_WAVE - 1);
    if (tid < DCN_MAX_SET_MEMBERS) s_cnt[tid] = 0;
    __syncthreads();
    unsigned long long mine = 0;
    const uint64_t stride = (uint64_t)gridDim.x * DCN_COV_THREADS;
    const uint64_t end = ALL ? n_slots : n_words;
    for (uint64_t w0 = (uint64_t)blockIdx.x * DCN_COV_THREADS + (tid - lane); w0 < end; w0 += stride) {
        const uint64_t i = w0 + lane;
        if constexpr (ALL) {
            cov_tally(i < n_slots ? labels[i] : 0u, n, lane, &mine);
        } else {
            uint32_t word = i < n_words ? bits[i] : 0u;
            while (__ballot(word != 0)) {
                uint32_t L = 0;
                if (word) {
                    L = labels[i * 32 + (__ffs(word) - 1)];
                    word &= word - 1;
                }
                cov_tally(L, n, lane, &mine);
            }
        }
    }
    if (lane < n && mine) atomicAdd(&s_cnt[lane], mine);
    __syncthreads();
    if (tid < n && s_cnt[tid]) atomicAdd(&counts[tid], s_cnt[tid]);
}

// marked slots whose label meets `mask`: counted (out == null: *n_out += the count) or written to out[*n_out ...] with
// one returning atomicAdd per wave (out holds cap keys: a position at or past cap is not written)
__global__ __launch_bounds__(DCN_COV_THREADS) void coverage_keys_kernel(const uint32_t *bits, uint64_t n_words,
                                                                        const uint32_t *labels, const uint64_t *slots,
                                                                        uint32_t mask, uint64_t *out, uint64_t cap,
                                                                        unsigned long long *n_out) {
    __shared__ unsigned long long s_n;
    const uint32_t tid = threadIdx.x, lane = tid & (DCN_WAVE - 1);
    if (tid == 0) s_n = 0;
    __syncthreads();
    unsigned long long mine = 0;
    const uint64_t stride = (uint64_t)gridDim.x * DCN_COV_THREADS;
    for (uint64_t w0 = (uint64_t)blockIdx.x * DCN_COV_THREADS + (tid - lane); w0 < n_words; w0 += stride) {
        const uint64_t i = w0 + lane;
        const uint32_t word = i < n_words ? bits[i] : 0u;
        uint32_t c = 0;
        for (uint32_t b = word; b; b &= b - 1)
            if (labels[i * 32 + (__ffs(b) - 1)] & mask) ++c;
        if (!out) {
            mine += c;
            continue;
        }
        // the wave's exclusive prefix of c, its total, and one atomicAdd by lane 0 for the wave's range of out
        uint32_t incl = c;
        for (uint32_t d = 1; d < DCN_WAVE; d <<= 1) {
            const uint32_t v = __shfl_up(incl, d);
            if (lane >= d) incl += v;
        }
        const uint32_t wave_total = __shfl(incl, DCN_WAVE - 1);
        if (!wave_total) continue;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(n_out, (unsigned long long)wave_total);
        base = __shfl(base, 0);
        uint64_t pos = base + (incl - c);
        for (uint32_t b = word; b; b &= b - 1) {
            const uint64_t s = i * 32 + (__ffs(b) - 1);
            if (labels[s] & mask) {
                if (pos < cap) out[pos] = slots[s];
                ++pos;
            }
        }
    }
    if (!out) {
        if (mine) atomicAdd(&s_n, mine);
        __syncthreads();
        if (tid == 0 && s_n) atomicAdd(n_out, s_n);
    }
}

uint32_t cov_blocks(uint64_t items) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + DCN_COV_THREADS - 1) / DCN_COV_THREADS,
                                                             (uint64_t)dcn_cu_count() * 8));
}

// insert-or-OR: every key of a member's slot array into the set, its bit into the label of the slot that holds it
__global__ void set_add_member_kernel(uint64_t *slots, uint32_t *labels, uint32_t shift, uint32_t mask, const uint64_t *src,
                                      uint64_t src_slots, uint32_t bit, unsigned long long *n_new) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long fresh = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < src_slots; i += stride) {
        const uint64_t key = src[i];
        if (key == 0) continue;
        atomicOr(&labels[dcn_table_insert_dev(slots, shift, mask, key, &fresh)], bit);
    }
    if (fresh) atomicAdd(n_new, fresh);
}

} // namespace

int dcn_launch_classify_units(const dcn_classify_args &a, hipStream_t stream) {
    if (a.n_units == 0) return DCN_OK;
    if (a.n_members == 0 || a.n_members > DCN_MAX_SET_MEMBERS) return dcn_fail(DCN_ERR_INTERNAL, "classify: member count");
    const uint32_t blocks = (a.n_units + DCN_CLS_LANES - 1) / DCN_CLS_LANES;
    if (a.cov_bits)
        hipLaunchKernelGGL(classify_units_kernel<true>, dim3(blocks), dim3(DCN_CLS_LANES), 0, stream, a);
    else
        hipLaunchKernelGGL(classify_units_kernel<false>, dim3(blocks), dim3(DCN_CLS_LANES), 0, stream, a);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_classify_big(const dcn_classify_args &a, hipStream_t stream) {
    if (a.n_units == 0) return DCN_OK;
    // a grid over the device's CUs (a few workgroups each), looping over the work list whose length is on the device
    const uint32_t blocks = std::min<uint32_t>(a.n_units, dcn_cu_count() * 4);
    if (a.cov_bits)
        hipLaunchKernelGGL(classify_big_kernel<true>, dim3(blocks), dim3(DCN_CLS_BIG_THREADS), 0, stream, a);
    else
        hipLaunchKernelGGL(classify_big_kernel<false>, dim3(blocks), dim3(DCN_CLS_BIG_THREADS), 0, stream, a);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_coverage_count(const dcn_index *set, bool all_slots, unsigned long long *d_counts, hipStream_t stream) {
    const uint64_t n_slots = set->n_groups * DCN_GROUP_SLOTS;
    if (all_slots)
        hipLaunchKernelGGL(coverage_count_kernel<true>, dim3(cov_blocks(n_slots)), dim3(DCN_COV_THREADS), 0, stream,
                           set->d_cov, set->cov_words, set->d_labels, n_slots, set->n_members, d_counts);
    else
        hipLaunchKernelGGL(coverage_count_kernel<false>, dim3(cov_blocks(set->cov_words)), dim3(DCN_COV_THREADS), 0, stream,
                           set->d_cov, set->cov_words, set->d_labels, n_slots, set->n_members, d_counts);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_coverage_count_mask(const dcn_index *set, uint32_t mask, unsigned long long *d_n, hipStream_t stream) {
    hipLaunchKernelGGL(coverage_keys_kernel, dim3(cov_blocks(set->cov_words)), dim3(DCN_COV_THREADS), 0, stream, set->d_cov,
                       set->cov_words, set->d_labels, set->d_slots, mask, nullptr, 0, d_n);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_coverage_collect(const dcn_index *set, uint32_t mask, uint64_t *d_out, uint64_t cap, unsigned long long *d_n,
                         hipStream_t stream) {
    hipLaunchKernelGGL(coverage_keys_kernel, dim3(cov_blocks(set->cov_words)), dim3(DCN_COV_THREADS), 0, stream, set->d_cov,
                       set->cov_words, set->d_labels, set->d_slots, mask, d_out, cap, d_n);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_set_add_member(dcn_index *set, const dcn_index *member, uint32_t bit) {
    DCN_HIP(hipSetDevice(set->device));
    unsigned long long *d_new = nullptr;
    DCN_HIP(hipMalloc((void **)&d_new, sizeof(unsigned long long)));
    hipError_t e = hipMemset(d_new, 0, sizeof(unsigned long long));
    const dcn_table_view v = set->view();
    const uint64_t src_slots = member->n_groups * DCN_GROUP_SLOTS;
    if (e == hipSuccess && src_slots) {
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((src_slots + 255) / 256, 256 * 16);
        hipLaunchKernelGGL(set_add_member_kernel, dim3(blocks), dim3(256), 0, 0, set->d_slots, set->d_labels, v.group_shift,
                           v.group_mask, member->d_slots, src_slots, 1u << bit, d_new);
        e = hipGetLastError();
    }
    unsigned long long h_new = 0;
    if (e == hipSuccess) e = hipMemcpy(&h_new, d_new, sizeof(h_new), hipMemcpyDeviceToHost);
    hipFree(d_new);
    if (e != hipSuccess) return dcn_fail(e == hipErrorOutOfMemory ? DCN_ERR_NOMEM : DCN_ERR_HIP, std::string("index set: ") + hipGetErrorString(e));
    set->n_keys += h_new;
    if (member->has_zero) {
        if (!set->has_zero) set->n_keys += 1;
        set->has_zero = true;
        set->zero_label |= 1u << bit;
    }
    return DCN_OK;
}
