// dcn_derive.h -- what the entry points that derive a new index from device tables in two passes (count, then insert
// into a table sized for the count) share: set_algebra_api.hip and index_builder_api.hip.  Internal, like dcn_ctx.h (whose DevMem and read_count they use).
#pragma once

#include "dcn_ctx.h"

#include <new>

#pragma GCC visibility push(hidden)
namespace dcn_impl {
// an empty plain index with the parameters of `like` and a table for n_keys keys
inline int new_index_like(const dcn_index *like, uint64_t n_keys, dcn_index **idx) {
    *idx = new (std::nothrow) dcn_index();
    if (!*idx) return dcn_fail(DCN_ERR_NOMEM, "host allocation failed");
    (*idx)->device = like->device;
    (*idx)->variant = like->variant;
    (*idx)->k = like->k;
    (*idx)->w = like->w;
    return dcn_table_alloc(*idx, n_keys);
}

// the end of a build pass (idx may be null when rc says so): every key counted was inserted once
inline int finish_build(int rc, const DevMem &d_n, unsigned long long counted, bool zero, const char *what, dcn_index *idx,
                 dcn_index **out) {
    unsigned long long fresh = 0;
    if (rc == DCN_OK) rc = read_count(d_n, what, &fresh);
    if (rc == DCN_OK && fresh != counted)
        rc = dcn_fail(DCN_ERR_INTERNAL, std::string(what) + ": " + std::to_string(counted) + " keys counted, " + std::to_string(fresh) + " inserted");
    if (rc != DCN_OK) {
        dcn_index_destroy(idx);
        return rc;
    }
    idx->n_keys = fresh + (zero ? 1 : 0);
    idx->has_zero = zero;
    *out = idx;
    return DCN_OK;
}
} // namespace dcn_impl
#pragma GCC visibility pop
