// dcn_short_lane.h -- how many windows a read has, and which 16-byte chunks of the batch's ASCII a lane of the scan kernel's
// short path (scan.hip, scan_short) needs for it: the one copy that plan.hip's tile planning and the short path share.
// Plain integer arithmetic: compiles for the host as well (tests/cpp).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DCN_LANE_FN __host__ __device__ inline
#else
#define DCN_LANE_FN inline
#endif

// effective sequence -> number of windows (src/filter_common.rs:217-229).  `len` is the whole read, `n` what a prefix cut
// leaves of it (n == len without one), `ends_in_newline` says that byte n - 1 of the read is '\n'; l = k + w - 1.
DCN_LANE_FN uint32_t dcn_window_count(uint64_t len, uint64_t n, bool ends_in_newline, uint32_t k, uint32_t l) {
    if (len < k) return 0;                 // :217 -- tested on the full read, before the prefix cut
    if (ends_in_newline && n > 0) n -= 1;  // :229
    return n >= l ? (uint32_t)(n - l + 1) : 0;
}

// A read [off, end) of the stream, whose byte 0 sits a16 bytes into a 16-byte chunk of the address space: stream base p
// lies in chunk (a16 + p) >> 4.  The lane scans from w - 1 bases in front of the read (the lead-in of the rolling window
// state) to the read's last byte, the newline included.
struct dcn_short_span {
    uint32_t windows;    // dcn_window_count of the read, no prefix
    int64_t chunk_first; // chunk of base off - (w - 1); -1 when that lies in front of chunk 0
    int64_t chunk_last;  // chunk of base end - 1 (of the base in front of an empty read); -1 as above
};

DCN_LANE_FN dcn_short_span dcn_short_lane(uint64_t off, uint64_t end, bool ends_in_newline, uint32_t k, uint32_t w, uint32_t a16) {
    dcn_short_span s;
    s.windows = dcn_window_count(end - off, end - off, ends_in_newline, k, k + w - 1);
    s.chunk_first = ((int64_t)(a16 + off) - (int64_t)(w - 1)) >> 4;
    s.chunk_last = ((int64_t)(a16 + end) - 1) >> 4;
    return s;
}
