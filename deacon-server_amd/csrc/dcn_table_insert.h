// dcn_table_insert.h -- the insert step of the device table, shared by the kernels that add keys to one
// (table_copy_filtered_kernel, set_add_member_kernel, and the select / intersect kernels of set_algebra.hip).
#pragma once

#include "dcn_internal.h"

// Make `key` (not 0) a member of the table: walk the groups from its home group and claim the first empty slot with a
// CAS, unless a slot on the way already holds it.  Returns the slot (index into `slots`) that holds the key afterwards;
// *fresh is incremented when this call claimed it.  The table must keep an empty slot (dcn_table_groups_for sizes it so).
__device__ inline uint64_t dcn_table_insert_dev(uint64_t *slots, uint32_t group_shift, uint32_t group_mask, uint64_t key,
                                                unsigned long long *fresh) {
    uint32_t g = dcn_group_of(key, group_shift, group_mask);
    for (;;) {
        unsigned long long *grp = (unsigned long long *)(slots + (uint64_t)g * DCN_GROUP_SLOTS);
        for (int s = 0; s < DCN_GROUP_SLOTS; ++s) {
            unsigned long long cur = __hip_atomic_load(&grp[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == 0) {
                cur = atomicCAS(&grp[s], 0ull, (unsigned long long)key);
                if (cur == 0) {
                    ++*fresh;
                    cur = key;
                }
                // else: another lane claimed the slot first -- for this key (done) or for another one (keep walking)
            }
            if (cur == key) return (uint64_t)g * DCN_GROUP_SLOTS + s;
        }
        g = (g + 1) & group_mask;
    }
}
