// dcn_short_lane / dcn_window_count (deacon-server_amd/csrc/dcn_short_lane.h, shared by plan.hip and scan.hip) compiled for
// the host, against a plain model that walks the read byte by byte: every length 0..153, with and without a trailing
// newline, at all 16 alignments of the stream and at several places in it (the stream's front included).  Built and run by
// tests/test_short_offsets_cases.py.
#include "dcn_short_lane.h"
#include <cstdio>
#include <string>

// src/filter_common.rs:217-229 on an actual byte string, then windows counted one by one
static unsigned model_windows(const std::string &read, unsigned k, unsigned w) {
    if (read.size() < k) return 0;
    std::string eff = read;
    if (!eff.empty() && eff.back() == '\n') eff.pop_back();
    unsigned n = 0;
    for (size_t s = 0; s + (k + w - 1) <= eff.size(); ++s) ++n;
    return n;
}

// the 16-byte chunk of the address space that holds stream base p, the stream starting a16 bytes into chunk 0
static long long model_chunk(long long p, unsigned a16) {
    const long long byte = (long long)a16 + p; // may be negative: floor division
    return byte >= 0 ? byte / 16 : -((-byte + 15) / 16);
}

int main() {
    const unsigned geometries[][2] = {{31, 15}, {21, 15}, {32, 15}, {15, 15}};
    const unsigned long long starts[] = {0, 1, 13, 14, 15, 16, 17, 150, 4096, (1ull << 32) - 7, (1ull << 33) + 5};
    for (const auto &kw : geometries) {
        const unsigned k = kw[0], w = kw[1];
        for (unsigned len = 0; len <= 153; ++len)
            for (int nl = 0; nl < 2; ++nl) {
                if (nl && len == 0) continue; // (an empty read ends in nothing)
                std::string read(len, 'C');
                if (nl) read[len - 1] = '\n';
                const unsigned want = model_windows(read, k, w);
                for (unsigned a16 = 0; a16 < 16; ++a16)
                    for (unsigned long long off : starts) {
                        const dcn_short_span s = dcn_short_lane(off, off + len, nl != 0, k, w, a16);
                        const long long first = model_chunk((long long)off - (long long)(w - 1), a16);
                        const long long last = model_chunk((long long)off + (long long)len - 1, a16);
                        if (s.windows != want || s.chunk_first != first || s.chunk_last != last) {
                            std::printf("k %u w %u len %u nl %d a16 %u off %llu: windows %u chunks %lld..%lld, want %u %lld..%lld\n", k, w, len,
                                        nl, a16, off, s.windows, (long long)s.chunk_first, (long long)s.chunk_last, want, first, last);
                            return 1;
                        }
                        // what the scan kernel relies on: the lead-in lies inside the span, and the span of a full wave of
                        // such reads fits the staging area's 612 words
                        if (s.chunk_first > model_chunk((long long)off, a16) || (s.chunk_last - s.chunk_first + 1) * 16 < (long long)len) {
                            std::printf("span of len %u a16 %u off %llu does not cover the read\n", len, a16, off);
                            return 1;
                        }
                    }
                // the prefix form plan.hip uses: n = what the prefix leaves, the newline flag describes byte n - 1
                for (unsigned prefix = 1; prefix <= len + 1; prefix += 7) {
                    const unsigned n = len > prefix ? prefix : len;
                    std::string cut = read.substr(0, n);
                    const bool cut_nl = !cut.empty() && cut.back() == '\n';
                    unsigned want_p = 0;
                    if (len >= k) {
                        if (cut_nl) cut.pop_back();
                        want_p = cut.size() >= k + w - 1 ? (unsigned)(cut.size() - (k + w - 1) + 1) : 0;
                    }
                    if (dcn_window_count(len, n, cut_nl, k, k + w - 1) != want_p) {
                        std::printf("k %u w %u len %u nl %d prefix %u: %u, want %u\n", k, w, len, nl, prefix,
                                    dcn_window_count(len, n, cut_nl, k, k + w - 1), want_p);
                        return 1;
                    }
                }
            }
    }
    return 0;
}
