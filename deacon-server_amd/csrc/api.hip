// api.hip -- C ABI of include/deacon_hip.h: error plumbing, version, and the index entry points (build, load, union,
// diff, clone, queries), plus the host helpers that need no context (dcn_host_alloc, dcn_pack_ascii).  The context and
// the batch pipeline are in ctx.hip, host_batch.hip, dump.hip and classify_api.hip (see dcn_ctx.h).
#include "dcn_ctx.h"
#include "dcn_host_pool.h"

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

using dcn_host::HostPool;

#define DCN_VERSION_STRING "deacon-hip 0.4.0 (gfx950)"

// ----------------------------------------------------------------------------------------------------
// errors
// ----------------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

void dcn_set_error(const std::string &msg) { g_last_error = msg; }
int dcn_fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

extern "C" const char *dcn_last_error(void) { return g_last_error.c_str(); }
extern "C" const char *dcn_version(void) { return DCN_VERSION_STRING; }

extern "C" int dcn_abi_version(uint32_t *major, uint32_t *minor) {
    if (!major || !minor) return dcn_fail(DCN_ERR_ARG, "dcn_abi_version: NULL output");
    *major = DCN_ABI_MAJOR;
    *minor = DCN_ABI_MINOR;
    return DCN_OK;
}

extern "C" int dcn_device_count(int *count) {
    if (!count) return dcn_fail(DCN_ERR_ARG, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return dcn_fail(DCN_ERR_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *count = n;
    return DCN_OK;
}

// ----------------------------------------------------------------------------------------------------
// index
// ----------------------------------------------------------------------------------------------------
int dcn_read_index_file(const char *path, uint8_t *k, uint8_t *w, std::vector<uint64_t> *keys); // index_file.cpp

int dcn_impl::check_kw(uint8_t k, uint8_t w) {
    if (k < 1 || k > 56) return dcn_fail(DCN_ERR_ARG, "k must be in 1..=56 (src/filter_common.rs:269-272)");
    if (w < 1) return dcn_fail(DCN_ERR_ARG, "w must be >= 1");
    if (((uint32_t)k + w - 1) % 2 == 0)
        return dcn_fail(DCN_ERR_ARG, "Constraint violated: k + w - 1 must be odd (src/index.rs:186-194)");
    // every index passes through here when it is made, and captures the process's rule then: a rule other than the default
    // runs the generic kernel, whose window ring holds two u64 keys per slot in LDS (scan.hip) -- refused now, not at the
    // first filter call
    if (dcn_current_variant() != DCN_VARIANT_DEFAULT && w > 128)
        return dcn_fail(DCN_ERR_ARG, "minimizer variant: w <= 128 under a non-default rule (dcn_set_minimizer_variant)");
    return DCN_OK;
}

using dcn_impl::check_kw;

// the end of every entry point that makes an index: hand it over, or release it with the error
static int publish_index(int rc, dcn_index *idx, dcn_index **out) {
    if (rc != DCN_OK) {
        if (idx->d_slots) hipFree(idx->d_slots);
        delete idx;
        return rc;
    }
    *out = idx;
    return DCN_OK;
}

extern "C" int dcn_index_from_keys(const uint64_t *keys, uint64_t n, uint8_t k, uint8_t w, int device,
                                   dcn_index **out) {
    if (!out) return dcn_fail(DCN_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (n > 0 && !keys) return dcn_fail(DCN_ERR_ARG, "keys is NULL");
    int rc = check_kw(k, w);
    if (rc != DCN_OK) return rc;
    int ndev = 0;
    rc = dcn_device_count(&ndev);
    if (rc != DCN_OK) return rc;
    if (device < 0 || device >= ndev) return dcn_fail(DCN_ERR_ARG, "no such HIP device");
    dcn_index *idx = new (std::nothrow) dcn_index();
    if (!idx) return dcn_fail(DCN_ERR_NOMEM, "host allocation failed");
    idx->device = device;
    idx->k = k;
    idx->w = w;
    rc = dcn_table_build(idx, keys, n);
    return publish_index(rc, idx, out);
}

// Index file whose remaining bytes after the count are exactly 9 per hash: every hash is `0xFD + u64 LE`
// (nothing shorter fits, 9 is the longest u64 varint), so record i is at a fixed offset.  The file is mapped,
// copied chunk by chunk into pinned memory by the host copy threads, and decoded + inserted by
// table_insert_varint9_kernel while the next chunk is being copied (load_minimizer_hashes, src/index.rs:80-107).
// *handled stays false when the file is not of that shape (or cannot be mapped): the caller then runs the
// general host decoder, which also produces the reference's error messages.
int dcn_load_index_fixed9(const char *path, int device, dcn_index **out, bool *handled) {
    *handled = false;
    int fd = open(path, O_RDONLY);
    if (fd < 0) return DCN_OK;
    struct stat st;
    uint8_t head[12];
    ssize_t got = 0;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || (got = pread(fd, head, sizeof head, 0)) < 4 || head[0] != 2) {
        close(fd);
        return DCN_OK;
    }
    const uint8_t k = head[1], w = head[2], b = head[3];
    size_t len = b < 251 ? 1 : b == 0xFB ? 3 : b == 0xFC ? 5 : b == 0xFD ? 9 : 0;
    uint64_t count = b;
    if (len == 0 || (size_t)got < 3 + len) {
        close(fd);
        return DCN_OK;
    }
    if (len > 1) {
        count = 0;
        memcpy(&count, head + 4, len - 1);
    }
    const uint64_t pos = 3 + len, size = (uint64_t)st.st_size;
    int ndev = 0;
    // DCN_LOAD_TIMING=1: where the load's wall time goes, one line on stderr (runtime start-up = the first HIP call)
    const bool timing = getenv("DCN_LOAD_TIMING") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    double t_marks[6] = {0, 0, 0, 0, 0, 0};
    auto mark = [&](int i) { t_marks[i] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };
    if (count == 0 || count > (1ull << 40) || size - pos != 9 * count || check_kw(k, w) != DCN_OK ||
        dcn_device_count(&ndev) != DCN_OK || device < 0 || device >= ndev) {
        close(fd);
        return DCN_OK;
    }
    mark(0);  // runtime up (dcn_device_count)
    // The host threads pread() their slices of a chunk straight into the page-locked buffer.  (Until round 3 the file was
    // mapped and copied out of the mapping: unmapping its 900 k pages and releasing two 72 MB staging buffers took
    // 0.06-0.11 s of a 0.32-0.43 s load of panhuman-1's 3.7 GB, pinning the buffers 0.04-0.06 s; now 0.00 and 0.02-0.03 s.
    // DCN_LOAD_TIMING=1 prints the split.)
    (void)posix_fadvise(fd, 0, 0, POSIX_FADV_SEQUENTIAL);
    const uint64_t CH = std::min<uint64_t>(count, 7ull << 19); // records per chunk (33 MB)
    const uint64_t ch_bytes = 9 * CH + 16;
    dcn_index *idx = new (std::nothrow) dcn_index();
    uint8_t *h_buf[2] = {nullptr, nullptr};
    uint64_t *d_raw[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipStream_t st_ = nullptr;
    unsigned long long *d_new = nullptr;
    uint32_t *d_flags = nullptr; // [0] has_zero, [1] bad marker
    int rc = idx ? DCN_OK : dcn_fail(DCN_ERR_NOMEM, "host allocation failed");
    auto hip_ok = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && rc == DCN_OK) rc = dcn_fail(DCN_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
        return e == hipSuccess;
    };
    if (rc == DCN_OK) {
        idx->device = device;
        idx->k = k;
        idx->w = w;
        hip_ok(hipSetDevice(device), "hipSetDevice");
    }
    if (rc == DCN_OK) rc = dcn_table_alloc(idx, count);
    if (rc == DCN_OK) {
        hip_ok(hipDeviceSynchronize(), "table clear"); // the table's memset ran on the null stream
        mark(1);  // table allocated and cleared
        hip_ok(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking), "stream");
        for (int i = 0; i < 2 && rc == DCN_OK; ++i) {
            hip_ok(hipHostMalloc((void **)&h_buf[i], ch_bytes, hipHostMallocDefault), "hipHostMalloc");
            hip_ok(hipMalloc((void **)&d_raw[i], ch_bytes), "hipMalloc");
            hip_ok(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming), "event");
            if (rc == DCN_OK) hip_ok(hipMemsetAsync(d_raw[i], 0, ch_bytes, st_), "memset");
        }
        hip_ok(hipMalloc((void **)&d_new, sizeof(unsigned long long)), "hipMalloc");
        hip_ok(hipMalloc((void **)&d_flags, 2 * sizeof(uint32_t)), "hipMalloc");
        if (rc == DCN_OK) {
            hip_ok(hipMemsetAsync(d_new, 0, sizeof(unsigned long long), st_), "memset");
            hip_ok(hipMemsetAsync(d_flags, 0, 2 * sizeof(uint32_t), st_), "memset");
        }
    }
    mark(2);  // staging buffers
    bool read_failed = false;  // (the general decoder then reports what is wrong with the file)
    int which = 0;
    for (uint64_t off = 0; off < count && rc == DCN_OK; off += CH, which ^= 1) {
        const uint64_t m = std::min<uint64_t>(CH, count - off);
        if (!hip_ok(hipEventSynchronize(ev[which]), "event wait")) break; // the copy out of this buffer is done
        std::atomic<int> bad{0};
        HostPool::get().run([&](int i, int nt) {
            const uint64_t n = 9 * m, per = ((n / nt) + 4095) & ~4095ull;
            uint64_t lo = std::min(n, per * i);
            const uint64_t hi = i == nt - 1 ? n : std::min(n, per * (i + 1));
            while (lo < hi) {
                const ssize_t g = pread(fd, h_buf[which] + lo, hi - lo, (off_t)(pos + 9 * off + lo));
                if (g < 0 && errno == EINTR) continue;
                if (g <= 0) {
                    bad.store(1);
                    return;
                }
                lo += (uint64_t)g;
            }
        });
        if (bad.load()) {
            read_failed = true;
            break;
        }
        if (!hip_ok(hipMemcpyAsync(d_raw[which], h_buf[which], 9 * m, hipMemcpyHostToDevice, st_), "hipMemcpyAsync")) break;
        rc = dcn_table_insert_varint9(idx, d_raw[which], m, d_new, d_flags, d_flags + 1, st_);
        if (rc == DCN_OK) hip_ok(hipEventRecord(ev[which], st_), "event record");
    }
    unsigned long long h_new = 0;
    uint32_t h_flags[2] = {0, 0};
    close(fd);
    if (rc == DCN_OK && !read_failed) {
        hip_ok(hipStreamSynchronize(st_), "index load");
        hip_ok(hipMemcpy(&h_new, d_new, sizeof h_new, hipMemcpyDeviceToHost), "hipMemcpy");
        hip_ok(hipMemcpy(h_flags, d_flags, sizeof h_flags, hipMemcpyDeviceToHost), "hipMemcpy");
    }
    if (rc == DCN_OK && h_flags[1]) rc = dcn_fail(DCN_ERR_FORMAT, "Failed to deserialise minimizer hash");
    mark(3);  // every chunk copied, decoded and inserted
    if (st_) hipStreamSynchronize(st_);
    for (int i = 0; i < 2; ++i) {
        if (h_buf[i]) hipHostFree(h_buf[i]);
        if (d_raw[i]) hipFree(d_raw[i]);
        if (ev[i]) hipEventDestroy(ev[i]);
    }
    if (d_new) hipFree(d_new);
    if (d_flags) hipFree(d_flags);
    if (st_) hipStreamDestroy(st_);
    if (rc != DCN_OK || read_failed) {
        if (idx && idx->d_slots) hipFree(idx->d_slots);
        delete idx;
        return rc;
    }
    idx->n_keys = h_new;
    idx->has_zero = h_flags[0] != 0;
    *out = idx;
    *handled = true;
    mark(4);
    if (timing)
        fprintf(stderr, "load timing: runtime up %.3f s, table of %.1f GB allocated + cleared %.3f, staging buffers %.3f, %.2f GB copied / "
                        "decoded / inserted %.3f, buffers released %.3f\n",
                t_marks[0], (double)idx->n_groups * 16 / 1e9, t_marks[1] - t_marks[0], t_marks[2] - t_marks[1], 9.0 * count / 1e9,
                t_marks[3] - t_marks[2], t_marks[4] - t_marks[3]);
    return DCN_OK;
}

extern "C" int dcn_index_from_file(const char *path, int device, dcn_index **out) {
    if (!out) return dcn_fail(DCN_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!path) return dcn_fail(DCN_ERR_ARG, "path is NULL");
    // The reference's file format has no room for the rule its keys were selected by (src/index.rs:17-31: version, k, w):
    // a file is taken to have been built under the rule in force now.  Under the default that is what every existing
    // file was built by; under any other setting (the parity-pinning switch) say so once, since a mismatch would probe
    // with the wrong minimizers and raise no error.
    if (dcn_current_variant() != DCN_VARIANT_DEFAULT && !getenv("DCN_QUIET")) {
        static std::atomic<bool> said{false};
        if (!said.exchange(true))
            std::fprintf(stderr, "deacon-hip: loading an index file under a non-default minimizer rule (dcn_set_minimizer_variant): "
                                 "the file carries no marker of the rule it was built by and is assumed to match\n");
    }
    // files whose hashes are all 9-byte varints (every hash >= 2^32: all of them, in practice) are decoded on
    // the device while they stream in; anything else takes the host decoder below
    bool handled = false;
    int rc = dcn_load_index_fixed9(path, device, out, &handled);
    if (rc != DCN_OK || handled) return rc;
    uint8_t k = 0, w = 0;
    std::vector<uint64_t> keys;
    rc = dcn_read_index_file(path, &k, &w, &keys);
    if (rc != DCN_OK) return rc;
    return dcn_index_from_keys(keys.data(), keys.size(), k, w, device, out);
}

int dcn_write_index_file(const char *path, uint8_t k, uint8_t w, const uint64_t *keys, uint64_t n); // index_file.cpp
int dcn_build_index_impl(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seqs, float entropy_threshold,
                         dcn_index *idx); // dump.hip

extern "C" int dcn_index_build(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seqs, uint8_t k, uint8_t w,
                               float entropy_threshold, uint64_t capacity_keys, int device, dcn_index **out) {
    if (!out) return dcn_fail(DCN_ERR_ARG, "out is NULL");
    *out = nullptr;
    int rc = check_kw(k, w);
    if (rc != DCN_OK) return rc;
    if (n_seqs > 0 && !offsets) return dcn_fail(DCN_ERR_ARG, "offsets is NULL");
    if (n_seqs > 0 && offsets[n_seqs] > 0 && !bases) return dcn_fail(DCN_ERR_ARG, "bases is NULL");
    if (!(entropy_threshold >= 0.0f && entropy_threshold <= 1.0f)) return dcn_fail(DCN_ERR_ARG, "entropy_threshold must be in [0, 1]");
    int ndev = 0;
    rc = dcn_device_count(&ndev);
    if (rc != DCN_OK) return rc;
    if (device < 0 || device >= ndev) return dcn_fail(DCN_ERR_ARG, "no such HIP device");
    dcn_index *idx = new (std::nothrow) dcn_index();
    if (!idx) return dcn_fail(DCN_ERR_NOMEM, "host allocation failed");
    idx->device = device;
    idx->k = k;
    idx->w = w;
    rc = dcn_table_alloc(idx, std::max<uint64_t>(capacity_keys, 1024));
    if (rc == DCN_OK) rc = dcn_build_index_impl(bases, offsets, n_seqs, entropy_threshold, idx);
    return publish_index(rc, idx, out);
}

int dcn_impl::same_params(const dcn_index *a, const dcn_index *b) {
    if (a->k != b->k || a->w != b->w)
        return dcn_fail(DCN_ERR_ARG, "Incompatible headers: k=" + std::to_string((int)b->k) + ", w=" + std::to_string((int)b->w) +
                                         " vs k=" + std::to_string((int)a->k) + ", w=" + std::to_string((int)a->w));
    if (a->device != b->device) return dcn_fail(DCN_ERR_ARG, "indexes live on different devices");
    if (a->variant != b->variant)
        return dcn_fail(DCN_ERR_ARG, "indexes were created under different minimizer rules (dcn_set_minimizer_variant)");
    return DCN_OK;
}

using dcn_impl::same_params;

extern "C" int dcn_index_union(const dcn_index *const *inputs, uint32_t n, dcn_index **out) {
    if (!out) return dcn_fail(DCN_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!inputs || n == 0 || !inputs[0]) return dcn_fail(DCN_ERR_ARG, "at least one input index is required");
    uint64_t sum = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!inputs[i]) return dcn_fail(DCN_ERR_ARG, "input index is NULL");
        int rc = same_params(inputs[0], inputs[i]);
        if (rc != DCN_OK) return rc;
        sum += inputs[i]->n_keys;  // worst-case capacity, as the reference pre-allocates (src/index.rs:579-594)
    }
    dcn_index *idx = new (std::nothrow) dcn_index();
    if (!idx) return dcn_fail(DCN_ERR_NOMEM, "host allocation failed");
    idx->device = inputs[0]->device;
    idx->variant = inputs[0]->variant;
    idx->k = inputs[0]->k;
    idx->w = inputs[0]->w;
    int rc = dcn_table_alloc(idx, std::max<uint64_t>(sum, 16));
    for (uint32_t i = 0; i < n && rc == DCN_OK; ++i) rc = dcn_table_merge(idx, inputs[i], nullptr);
    return publish_index(rc, idx, out);
}

extern "C" int dcn_index_diff(const dcn_index *first, const dcn_index *second, dcn_index **out) {
    if (!out) return dcn_fail(DCN_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!first || !second) return dcn_fail(DCN_ERR_ARG, "index is NULL");
    int rc = same_params(first, second);
    if (rc != DCN_OK) return rc;
    dcn_index *idx = new (std::nothrow) dcn_index();
    if (!idx) return dcn_fail(DCN_ERR_NOMEM, "host allocation failed");
    idx->device = first->device;
    idx->variant = first->variant;
    idx->k = first->k;
    idx->w = first->w;
    rc = dcn_table_alloc(idx, std::max<uint64_t>(first->n_keys, 16));
    if (rc == DCN_OK) rc = dcn_table_merge(idx, first, second);
    return publish_index(rc, idx, out);
}

extern "C" int dcn_index_keys(const dcn_index *index, uint64_t *out, uint64_t capacity, uint64_t *n) {
    if (!index || !n) return dcn_fail(DCN_ERR_ARG, "index/n is NULL");
    if (capacity > 0 && !out) return dcn_fail(DCN_ERR_ARG, "out is NULL");
    return dcn_table_export(index, out, capacity, n);
}

extern "C" int dcn_index_write_file(const dcn_index *index, const char *path) {
    if (!index || !path) return dcn_fail(DCN_ERR_ARG, "index/path is NULL");
    // (not a std::vector: its resize() writes 8 bytes of zero per key before the keys are copied over them)
    std::unique_ptr<uint64_t[]> keys(new (std::nothrow) uint64_t[std::max<uint64_t>(index->n_keys, 1)]);
    if (!keys) return dcn_fail(DCN_ERR_NOMEM, "index too large for host memory");
    uint64_t n = 0;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = dcn_table_export(index, keys.get(), index->n_keys, &n);
    if (rc != DCN_OK) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    rc = dcn_write_index_file(path, index->k, index->w, keys.get(), n);
    if (getenv("DCN_INDEX_TIMING"))
        fprintf(stderr, "index write timing: keys out of the table %.3f s, encoded and written %.3f s\n", std::chrono::duration<double>(t1 - t0).count(),
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count());
    return rc;
}

extern "C" int dcn_index_header(const dcn_index *index, uint8_t *k, uint8_t *w, uint64_t *n_keys) {
    if (!index) return dcn_fail(DCN_ERR_ARG, "index is NULL");
    if (k) *k = index->k;
    if (w) *w = index->w;
    if (n_keys) *n_keys = index->n_keys;
    return DCN_OK;
}

extern "C" int dcn_index_memory(const dcn_index *index, uint64_t *table_bytes) {
    if (!index || !table_bytes) return dcn_fail(DCN_ERR_ARG, "index/table_bytes is NULL");
    *table_bytes = index->n_groups * DCN_GROUP_SLOTS * sizeof(uint64_t);
    return DCN_OK;
}

extern "C" int dcn_index_device(const dcn_index *index, int *device) {
    if (!index || !device) return dcn_fail(DCN_ERR_ARG, "index/device is NULL");
    *device = index->device;
    return DCN_OK;
}

extern "C" int dcn_index_contains(const dcn_index *index, const uint64_t *keys, uint64_t n, uint8_t *out) {
    if (!index) return dcn_fail(DCN_ERR_ARG, "index is NULL");
    if (n > 0 && (!keys || !out)) return dcn_fail(DCN_ERR_ARG, "keys/out is NULL");
    return dcn_table_contains(index, keys, n, out);
}

extern "C" int dcn_index_contains_device(const dcn_index *index, const uint64_t *d_keys, uint64_t n, uint8_t *d_out,
                                         void *stream) {
    if (!index) return dcn_fail(DCN_ERR_ARG, "index is NULL");
    if (n > 0 && (!d_keys || !d_out)) return dcn_fail(DCN_ERR_ARG, "d_keys/d_out is NULL");
    return dcn_table_contains_device(index, d_keys, n, d_out, (hipStream_t)stream);
}

extern "C" int dcn_index_probe_ceiling(const dcn_index *index, const uint64_t *d_keys, uint64_t n, uint32_t reps,
                                       double *probes_per_s) {
    if (!index || !probes_per_s) return dcn_fail(DCN_ERR_ARG, "index/probes_per_s is NULL");
    return dcn_table_probe_ceiling(index, d_keys, n, reps, probes_per_s, nullptr);
}

extern "C" int dcn_index_clone(const dcn_index *index, int device, dcn_index **out) {
    if (!out) return dcn_fail(DCN_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!index) return dcn_fail(DCN_ERR_ARG, "index is NULL");
    int ndev = 0;
    DCN_TRY(dcn_device_count(&ndev));
    if (device < 0 || device >= ndev) return dcn_fail(DCN_ERR_ARG, "no such HIP device");
    dcn_index *idx = new (std::nothrow) dcn_index(*index);
    if (!idx) return dcn_fail(DCN_ERR_NOMEM, "host allocation failed");
    idx->device = device;
    idx->d_slots = nullptr;
    idx->d_labels = nullptr; // a replica of a labelled set is a plain index over the union of its members
    idx->n_members = 0;
    idx->zero_label = 0;
    idx->d_cov = nullptr; // ... without coverage
    idx->cov_words = 0;
    idx->d_depth = nullptr; // ... and without depth counters
    idx->depth_words = 0;
    idx->d_anchor = nullptr; // ... and a replica of an anchor map has no words
    idx->anchor_records = 0;
    idx->store = nullptr; // ... and keeps no bases
    idx->d_pileup = nullptr; // ... and has no pileup
    idx->pileup_bases = 0;
    idx->pileup_rows = 0;
    idx->ledger = nullptr; // ... nor an insertion ledger
    idx->del_ledger = nullptr; // ... nor a deletion ledger
    idx->d_pileup_qsums = nullptr; // ... nor quality sums
    idx->d_pileup_strands = nullptr; // ... nor strand planes
    idx->dups = nullptr; // ... nor a duplicate set
    idx->phase = nullptr; // ... nor phase sites
    const uint64_t bytes = idx->n_groups * DCN_GROUP_SLOTS * sizeof(uint64_t);
    // Another GPU: the keys cross the link, not the table (a tenth of the bytes at the default 8 slots per key; dcn_table_clone_by_keys).
    // The same GPU: a device-to-device copy of the table at HBM's pace.  DCN_CLONE_BY_KEYS=1 / DCN_CLONE_BY_COPY=1 force one form
    // (the first is how the one-GPU tests reach the cross-device code).
    const bool by_keys = std::getenv("DCN_CLONE_BY_KEYS") || (device != index->device && !std::getenv("DCN_CLONE_BY_COPY"));
    if (by_keys) {
        if (device != index->device) {
            int can = 0;
            if (hipSetDevice(device) == hipSuccess && hipDeviceCanAccessPeer(&can, device, index->device) == hipSuccess && can)
                if (hipDeviceEnablePeerAccess(index->device, 0) != hipSuccess) (void)hipGetLastError(); // already enabled
        }
        const int rc = dcn_table_clone_by_keys(index, idx);
        if (rc != DCN_OK) {
            delete idx;
            return rc;
        }
        *out = idx;
        return DCN_OK;
    }
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = dcn_table_malloc(&idx->d_slots, std::max<uint64_t>(bytes, 16));
    if (e == hipSuccess && bytes) {
        if (device == index->device) {
            e = hipMemcpy(idx->d_slots, index->d_slots, bytes, hipMemcpyDeviceToDevice);
        } else {
            int can = 0;
            (void)hipDeviceCanAccessPeer(&can, device, index->device);
            if (can) {
                hipError_t pe = hipDeviceEnablePeerAccess(index->device, 0);
                if (pe != hipSuccess) (void)hipGetLastError(); // already enabled
            }
            e = hipMemcpyPeer(idx->d_slots, device, index->d_slots, index->device, bytes);
        }
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        if (idx->d_slots) hipFree(idx->d_slots);
        delete idx;
        return dcn_fail(e == hipErrorOutOfMemory ? DCN_ERR_NOMEM : DCN_ERR_HIP, std::string("index clone: ") + hipGetErrorString(e));
    }
    *out = idx;
    return DCN_OK;
}

extern "C" void dcn_index_destroy(dcn_index *index) {
    if (!index) return;
    hipSetDevice(index->device);
    if (index->d_slots) hipFree(index->d_slots);
    if (index->d_labels) hipFree(index->d_labels);
    if (index->d_cov) hipFree(index->d_cov);
    if (index->d_depth) hipFree(index->d_depth);
    if (index->d_anchor) hipFree(index->d_anchor);
    dcn_base_store_free(index->store);
    if (index->d_pileup) hipFree(index->d_pileup);
    dcn_ins_ledger_free(index->ledger);
    dcn_del_ledger_free(index->del_ledger);
    if (index->d_pileup_qsums) hipFree(index->d_pileup_qsums);
    if (index->d_pileup_strands) hipFree(index->d_pileup_strands);
    dcn_dup_set_free(index->dups);
    dcn_phase_list_free(index->phase);
    delete index;
}

// ---- host helpers without a context ----
void dcn_host_parallel_copy(void *dst, const void *src, size_t n) { HostPool::get().copy(dst, src, n); }

extern "C" int dcn_pack_ascii(const uint8_t *bases, uint64_t n_bases, uint32_t *packed, uint32_t *invmask,
                              uint32_t *saw_newline) {
    if (saw_newline) *saw_newline = 0;
    if (n_bases > 0 && (!bases || !packed || !invmask)) return dcn_fail(DCN_ERR_ARG, "bases/packed/invmask is NULL");
    const uint64_t G = (n_bases + 31) / 32;
    std::atomic<uint32_t> nl{0};
    HostPool::get().run([&](int i, int nt) {
        const uint64_t per = (G + nt - 1) / nt, lo = std::min<uint64_t>(G, per * i), hi = std::min<uint64_t>(G, lo + per);
        if (dcn_host_pack_groups(bases, n_bases, lo, hi, packed + 2 * lo, invmask + lo)) nl.store(1, std::memory_order_relaxed);
    }, G < 4096);
    if (saw_newline) *saw_newline = nl.load();
    return DCN_OK;
}

extern "C" int dcn_host_alloc(uint64_t bytes, void **out) {
    if (!out) return dcn_fail(DCN_ERR_ARG, "out is NULL");
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, std::max<uint64_t>(bytes, 1), hipHostMallocDefault);
    if (e != hipSuccess) {
        *out = nullptr;
        return dcn_fail(DCN_ERR_NOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    }
    return DCN_OK;
}

extern "C" void dcn_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}
