// duplicates.hip -- the kernels of duplicate marking (THE DEFINITION OF A DUPLICATE, include/deacon_hip.h; the arithmetic of
// rules D3 and D4, shared with the host, is in dcn_duplicates.h).  One thread per unit (per old slot in the rehash), grids
// sized by the batch and not capped: DCN_GRID_CUS does not apply.
//   dup_keys_kernel     the key of every unit of the call into the key log, at the unit's ordinal.
//   dup_insert_kernel   behind it, so that the log is complete.  A unit with a key probes linearly from its hash.  An
//                       empty slot is claimed by compare-and-swap with the unit's ordinal.  In an occupied slot the
//                       resident ordinal's key is read from the log and compared word by word with the unit's own: equal,
//                       and the slot takes the smaller ordinal (atomicMin) and the unit is done; else the next slot.  The
//                       key of a slot never changes once it is claimed (an atomicMin replaces an ordinal by one with the
//                       same key), so a comparison made against any ordinal the slot has held is the comparison against
//                       the one it holds now, and two units of one key cannot end up in two slots: both walk the same
//                       chain and neither passes a slot that is empty or holds their key.  No multi-word claim.
//   dup_lookup_kernel   behind the insert.  Probes again, finds the slot of the unit's key, reads the smallest ordinal that
//                       the call and everything before it left there: `first`, `dup` = first < own ordinal, and the
//                       number of duplicates through one atomic per wave (a ballot and a population count).
//   dup_rehash_kernel   one thread per slot of the old table: an occupied slot's ordinal is claimed into the new table from
//                       the hash of its key in the log.  The keys of a table are distinct, so nothing is compared.
// The host keeps slots >= 2 * (keys + units of the call) before the insert, so every chain ends at an empty slot.
// These are latency-bound random 8-byte (slot) and 48-byte (log) accesses; there is no LDS and no barrier.
#include "dcn_duplicates.h"
#include "dcn_verify.h"

namespace {

constexpr uint32_t DUP_THREADS = 256;

__device__ inline uint64_t unit_of() { return (uint64_t)blockIdx.x * DUP_THREADS + threadIdx.x; }

__device__ inline unsigned long long slot_load(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(DUP_THREADS) void dup_keys_kernel(dcn_dup_args a) {
    const uint64_t u = unit_of();
    if (u >= a.n_units) return;
    a.log[a.ord0 + u] = dcn_dup_unit_key(a.items, u, a.paired, a.both_ends);
}

__global__ __launch_bounds__(DUP_THREADS) void dup_insert_kernel(dcn_dup_args a) {
    const uint64_t u = unit_of();
    if (u >= a.n_units) return;
    const unsigned long long ord = a.ord0 + u;
    const dcn_dup_key key = a.log[ord];
    if (!dcn_dup_has_key(key)) return;
    uint64_t i = dcn_dup_key_hash(key) & a.mask;
    for (;;) {
        unsigned long long cur = slot_load(a.slots + i);
        if (cur == DCN_DUP_EMPTY) {
            cur = atomicCAS(a.slots + i, (unsigned long long)DCN_DUP_EMPTY, ord);
            if (cur == DCN_DUP_EMPTY) return; // claimed
        }
        if (dcn_dup_key_equal(a.log[cur], key)) {
            if (ord < cur) atomicMin(a.slots + i, ord);
            return;
        }
        i = (i + 1) & a.mask;
    }
}

__global__ __launch_bounds__(DUP_THREADS) void dup_lookup_kernel(dcn_dup_args a) {
    const uint64_t u = unit_of();
    const bool live = u < a.n_units;
    const unsigned long long ord = a.ord0 + u;
    uint64_t first = DCN_DUP_NO_FIRST;
    if (live) {
        const dcn_dup_key key = a.log[ord];
        if (dcn_dup_has_key(key)) {
            uint64_t i = dcn_dup_key_hash(key) & a.mask;
            for (;;) {
                const unsigned long long cur = a.slots[i];
                if (cur == DCN_DUP_EMPTY) break; // (not reached: the insert kernel has put the key in this chain)
                if (dcn_dup_key_equal(a.log[cur], key)) {
                    first = cur;
                    break;
                }
                i = (i + 1) & a.mask;
            }
        }
    }
    const bool is_dup = live && first < ord;
    if (live) {
        if (a.dup) a.dup[u] = is_dup ? 1 : 0;
        if (a.first) a.first[u] = first;
    }
    const unsigned long long votes = __ballot(is_dup);
    if ((threadIdx.x & 63u) == 0 && votes) atomicAdd(a.n_dup, (unsigned long long)__popcll(votes));
}

__global__ __launch_bounds__(DUP_THREADS) void dup_rehash_kernel(dcn_dup_args a, const unsigned long long *old_slots, uint64_t n_old) {
    const uint64_t s = unit_of();
    if (s >= n_old) return;
    const unsigned long long ord = old_slots[s];
    if (ord == DCN_DUP_EMPTY) return;
    uint64_t i = dcn_dup_key_hash(a.log[ord]) & a.mask;
    while (atomicCAS(a.slots + i, (unsigned long long)DCN_DUP_EMPTY, ord) != DCN_DUP_EMPTY) i = (i + 1) & a.mask;
}

dim3 grid_of(uint64_t n) { return dim3((uint32_t)((n + DUP_THREADS - 1) / DUP_THREADS)); }
} // namespace

int dcn_launch_dup_keys(const dcn_dup_args &args, hipStream_t stream) {
    if (args.n_units == 0) return DCN_OK;
    hipLaunchKernelGGL(dup_keys_kernel, grid_of(args.n_units), dim3(DUP_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_dup_insert(const dcn_dup_args &args, hipStream_t stream) {
    if (args.n_units == 0) return DCN_OK;
    hipLaunchKernelGGL(dup_insert_kernel, grid_of(args.n_units), dim3(DUP_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_dup_lookup(const dcn_dup_args &args, hipStream_t stream) {
    if (args.n_units == 0) return DCN_OK;
    hipLaunchKernelGGL(dup_lookup_kernel, grid_of(args.n_units), dim3(DUP_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_dup_rehash(const dcn_dup_args &args, const unsigned long long *old_slots, uint64_t n_old, hipStream_t stream) {
    if (n_old == 0) return DCN_OK;
    hipLaunchKernelGGL(dup_rehash_kernel, grid_of(n_old), dim3(DUP_THREADS), 0, stream, args, old_slots, n_old);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}
