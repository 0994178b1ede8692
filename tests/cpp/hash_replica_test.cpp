// Host-only driver for tests/test_classify_replicas.py: prints dcn_group_of (dcn_internal.h) and dcn_cls_partition
// (dcn_classify.h) of every key, so the Python restatements the classification tests construct their inputs with are
// pinned to the functions the kernels use.
//   hash_replica_test KEYS_FILE GROUP_BITS... -- P...
// KEYS_FILE: one hexadecimal key per line.  Output: one line per key, the group of the key for every GROUP_BITS (number
// of groups = 2^bits, as dcn_index::view() derives group_shift and group_mask), then its partition for every P.
#include "dcn_classify.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s KEYS_FILE GROUP_BITS... -- P...\n", argv[0]);
        return 2;
    }
    std::vector<uint32_t> bits, parts;
    bool after = false;
    for (int i = 2; i < argc; ++i) {
        if (!strcmp(argv[i], "--")) after = true;
        else (after ? parts : bits).push_back((uint32_t)strtoul(argv[i], nullptr, 10));
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    uint64_t key;
    while (fscanf(f, "%" SCNx64, &key) == 1) {
        for (uint32_t b : bits) {
            const uint64_t n_groups = 1ull << b;
            printf("%u ", dcn_group_of(key, 32 - b, (uint32_t)(n_groups - 1)));
        }
        for (uint32_t p : parts) printf("%u ", dcn_cls_partition(key, p));
        printf("\n");
    }
    fclose(f);
    return 0;
}
