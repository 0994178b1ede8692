// dcn_pack4 / dcn_invalid4 (deacon-server_amd/csrc/dcn_pack.h, shared by pack.hip and scan.hip) compiled for the host:
// all 256 byte values in all four byte lanes against a byte-by-byte model.  Built and run by tests/test_short_fused_cases.py.
#include "dcn_pack.h"
#include <cstdio>
int main() {
    for (unsigned lane = 0; lane < 4; ++lane)
        for (unsigned c = 0; c < 256; ++c) {
            const unsigned others[4] = {'A', 'c', 'N', '\n'};
            unsigned x = 0;
            for (unsigned j = 0; j < 4; ++j) x |= (j == lane ? c : others[j]) << (8 * j);
            unsigned want_p = 0, want_m = 0;
            for (unsigned j = 0; j < 4; ++j) {
                const unsigned b = (x >> (8 * j)) & 0xFF;
                want_p |= ((b >> 1) & 3) << (2 * j);
                const bool ok = b == 'A' || b == 'C' || b == 'G' || b == 'T' || b == 'a' || b == 'c' || b == 'g' || b == 't';
                want_m |= (ok ? 0u : 1u) << j;
            }
            if (dcn_pack4(x) != want_p || dcn_invalid4(x) != want_m) {
                std::printf("lane %u byte %u: %x %x, want %x %x\n", lane, c, dcn_pack4(x), dcn_invalid4(x), want_p, want_m);
                return 1;
            }
        }
    return 0;
}
