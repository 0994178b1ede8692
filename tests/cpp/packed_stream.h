// A text as the pack kernel leaves it (dcn_pack.h, as on the device): the 2-bit stream and the invalid-base bits, in heap
// arrays of exactly `front` words in front of base 0, the words of the text's 32-base groups and `back` words behind them.
// Under the address sanitizer a read outside those words ends the program.
#pragma once

#include "dcn_pack.h"

#include <cstdint>
#include <string>
#include <vector>

struct PackedStream {
    std::vector<uint32_t> packed, mask;
    size_t front;
    PackedStream(const std::string &s, size_t front_words, size_t back_words) : front(front_words) {
        const size_t groups = (s.size() + 31) / 32;
        packed.assign(front + 2 * groups + back_words, 0);
        mask.assign(front + groups + back_words, 0);
        for (size_t g = 0; g < groups; ++g) {
            for (int q = 0; q < 8; ++q) {
                uint32_t w = 0;
                for (int j = 0; j < 4; ++j) {
                    const size_t i = g * 32 + 4 * q + j;
                    w |= (uint32_t)(uint8_t)(i < s.size() ? s[i] : 'A') << (8 * j);
                }
                packed[front + 2 * g + q / 4] |= dcn_pack4(w) << (8 * (q % 4));
                mask[front + g] |= dcn_invalid4(w) << (4 * q);
            }
        }
    }
    const uint32_t *p() const { return packed.data() + front; }
    const uint32_t *m() const { return mask.data() + front; }
};
