// dcn_ledger_range.h -- what the range calls over the two ledgers share on the host (insertions_api.hip defines them;
// indels_api.hip uses them too): the device memory of one call, the scan of counts with its total, the refusal of a range
// with 2^32 events, and the buckets of the insertion events of a range.
#pragma once

#include "dcn_ctx.h"
#include "dcn_verify.h"

#include <algorithm>
#include <vector>

#pragma GCC visibility push(hidden)
namespace dcn_ledger_api {
// Device memory of one call, freed when it ends.  reserve() makes one allocation from which the get() calls behind it are
// carved, 256 bytes apart at least, for as long as it lasts: a call whose arrays are sized by the range knows most of what it
// needs before its first kernel, and a device allocation costs far more than the kernels of a range with few events.  What
// does not fit (arrays sized by a total that a read-back brings) is allocated on its own, as without a reserve.
struct scratch {
    std::vector<void *> p;
    uint8_t *arena = nullptr;
    uint64_t arena_bytes = 0, arena_used = 0;
    int reserve(uint64_t bytes, const char *what) {
        if (arena || bytes == 0) return DCN_OK;
        DCN_TRY(dcn_impl::dev_alloc(&arena, bytes, what));
        p.push_back(arena);
        arena_bytes = bytes;
        return DCN_OK;
    }
    template <typename T>
    int get(T **out, uint64_t count, const char *what) {
        const uint64_t bytes = (std::max<uint64_t>(count, 1) * sizeof(T) + 255) / 256 * 256;
        if (arena && bytes <= arena_bytes - arena_used) {
            *out = reinterpret_cast<T *>(arena + arena_used);
            arena_used += bytes;
            return DCN_OK;
        }
        DCN_TRY(dcn_impl::dev_alloc(out, std::max<uint64_t>(count, 1), what));
        p.push_back(*out);
        return DCN_OK;
    }
    template <typename T>
    int get_zeroed(T **out, uint64_t count, const char *what) {
        DCN_TRY(get(out, count, what));
        DCN_HIP(hipMemset(*out, 0, std::max<uint64_t>(count, 1) * sizeof(T)));
        return DCN_OK;
    }
    ~scratch() {
        for (void *q : p) hipFree(q);
    }
};

// the scan of n counts into n + 1 offsets of the call's scratch, and its total
int scan_counts(scratch &mem, const uint32_t *d_counts, uint64_t n, uint64_t **d_offsets, uint64_t *total, const char *what);
// DCN_ERR_ARG: a range with 2^32 events or more
int too_many(const char *who, uint64_t total);
// What the range calls over an insertion ledger share: the range's checks, the counts of the range (the INS plane, under rule
// L6 with its flags for `call`), their scan and the scatter of the ledger's events into the buckets.  *n_slots = 0: nothing
// in the range (ra->counts is null then when the range or the ledger is empty).
int range_buckets(const dcn_index *map, const char *who, bool call, uint32_t record, uint64_t start, uint64_t n_bases, uint32_t min_depth,
                  uint32_t min_permille, scratch &mem, dcn_ins_range_args *ra, uint64_t *n_slots);
} // namespace dcn_ledger_api
#pragma GCC visibility pop
