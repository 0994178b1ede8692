// dcn_derive.h -- what the entry points that derive a new index from device tables in two passes (count, then insert
// into a table sized for the count) share: set_algebra_api.hip and index_builder_api.hip.  Internal, like dcn_ctx.h.
#pragma once

#include "dcn_ctx.h"

#include <new>

#pragma GCC visibility push(hidden)
namespace dcn_impl {
// device scratch that goes back on every way out
struct DevMem {
    void *p = nullptr;
    ~DevMem() {
        if (p) hipFree(p);
    }
    int alloc(uint64_t bytes, bool zero, const char *what) {
        hipError_t e = hipMalloc(&p, std::max<uint64_t>(bytes, 8));
        if (e == hipSuccess && zero) e = hipMemset(p, 0, std::max<uint64_t>(bytes, 8));
        if (e == hipSuccess) return DCN_OK;
        return dcn_fail(e == hipErrorOutOfMemory ? DCN_ERR_NOMEM : DCN_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    }
    int clear(const char *what) { // the first 8 bytes: a counter between two sweeps
        const hipError_t e = hipMemset(p, 0, 8);
        return e == hipSuccess ? DCN_OK : dcn_fail(DCN_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    }
    template <typename T>
    T *as() const {
        return (T *)p;
    }
};

// the counter of a sweep, after the sweep (the copy waits for the null stream)
inline int read_count(const DevMem &d_n, const char *what, unsigned long long *n) {
    const hipError_t e = hipMemcpy(n, d_n.p, sizeof(*n), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return dcn_fail(DCN_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return DCN_OK;
}

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
