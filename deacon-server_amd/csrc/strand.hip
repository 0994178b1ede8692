// strand.hip -- the read-outs of strand evidence (THE DEFINITION OF STRAND EVIDENCE, include/deacon_hip.h; the rule is in
// dcn_strand.h, the C ABI in strand_api.hip; the planes are filled by pileup_kernel<., true>, pileup.hip).
//   strand_evidence_kernel  one thread per query: a gather of the position's eight counters and, on a base query, its four
//                           reverse counters, then rules S3 - S6.
//   indel_strand_kernel     one thread per event of a ledger (<true>: the insertion ledger, <false>: the deletion ledger).
//                           The event looks for the site of its (base, kind, front) by binary search in the call's sites,
//                           which are in I6's order; compares its len, and on an insertion its bases, with the site's
//                           allele; and when it is a reverse event of that allele adds 1 to the site's number.
// Integers only; the adds commute.
#include "dcn_indels.h"
#include "dcn_insertions.h"
#include "dcn_pileup.h"
#include "dcn_strand.h"
#include "dcn_verify.h"

namespace {

constexpr uint32_t STRAND_THREADS = 256;

__global__ __launch_bounds__(STRAND_THREADS) void strand_evidence_kernel(dcn_strand_evidence_args a) {
    const uint64_t q = (uint64_t)blockIdx.x * STRAND_THREADS + threadIdx.x;
    if (q >= a.n) return;
    const dcn_strand_query_item it = a.queries[q]; // (the host has checked base < bases, ref_code, alt_mask and the counts)
    const uint32_t n0 = a.counters[dcn_pile_index(DCN_PILE_A, it.base, a.bases)], n1 = a.counters[dcn_pile_index(DCN_PILE_C, it.base, a.bases)],
                   n2 = a.counters[dcn_pile_index(DCN_PILE_G, it.base, a.bases)], n3 = a.counters[dcn_pile_index(DCN_PILE_T, it.base, a.bases)];
    dcn_strand_site_item out;
    dcn_strand_table t;
    if (it.kind == 0) {
        const uint32_t r0 = a.strands[dcn_pile_strand_index(DCN_PILE_A, it.base, a.bases)],
                       r1 = a.strands[dcn_pile_strand_index(DCN_PILE_C, it.base, a.bases)],
                       r2 = a.strands[dcn_pile_strand_index(DCN_PILE_G, it.base, a.bases)],
                       r3 = a.strands[dcn_pile_strand_index(DCN_PILE_T, it.base, a.bases)];
        out.fwd[0] = dcn_strand_forward(n0, r0), out.fwd[1] = dcn_strand_forward(n1, r1);
        out.fwd[2] = dcn_strand_forward(n2, r2), out.fwd[3] = dcn_strand_forward(n3, r3);
        out.rev[0] = r0, out.rev[1] = r1, out.rev[2] = r2, out.rev[3] = r3;
        t = dcn_strand_base_table(n0, n1, n2, n3, r0, r1, r2, r3, it.ref_code, it.alt_mask);
    } else {
        const uint32_t depth = n0 + n1 + n2 + n3 + a.counters[dcn_pile_index(DCN_PILE_N, it.base, a.bases)] +
                               a.counters[dcn_pile_index(DCN_PILE_DEL, it.base, a.bases)]; // P4 (wraps as the counters do)
        const uint32_t rev = a.counters[dcn_pile_index(DCN_PILE_REV, it.base, a.bases)];
        out.fwd[0] = out.fwd[1] = out.fwd[2] = out.fwd[3] = 0;
        out.rev[0] = out.rev[1] = out.rev[2] = out.rev[3] = 0;
        t = dcn_strand_indel_table(depth, rev, it.count, it.count_reverse);
    }
    out.table[0] = t.a, out.table[1] = t.b, out.table[2] = t.c, out.table[3] = t.d;
    out.sb_centi = dcn_strand_score(t);
    const dcn_strand_prm prm = {a.max_sb_centi, a.min_alt_strand, a.min_strand_depth};
    out.flags = dcn_strand_flags(t, out.sb_centi, prm);
    out.reserved[0] = out.reserved[1] = 0;
    a.out[q] = out;
}

template <bool INS>
__global__ __launch_bounds__(STRAND_THREADS) void indel_strand_kernel(dcn_indel_strand_args a) {
    const uint64_t e = (uint64_t)blockIdx.x * STRAND_THREADS + threadIdx.x;
    if (e >= (INS ? a.n_ins_events : a.n_del_events)) return;
    uint64_t base, bases_offset = 0;
    uint32_t len, reverse, order;
    if constexpr (INS) {
        const dcn_ins_event ev = a.ins_events[e];
        base = ev.base, len = ev.len, bases_offset = ev.bases_offset;
        reverse = (ev.flags & DCN_INS_REVERSE) != 0;
        order = (ev.flags & DCN_INS_FRONT) ? 0u : 2u;
    } else {
        const dcn_del_event ev = a.del_events[e];
        base = ev.base, len = ev.len;
        reverse = (ev.flags & DCN_DEL_REVERSE) != 0;
        order = 1u;
    }
    if (!reverse) return;
    const uint64_t key = dcn_indel_strand_key(base, order);
    uint64_t lo = 0, hi = a.n_sites; // the first site whose key is not below the event's
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a.site_keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= a.n_sites || a.site_keys[lo] != key || a.site_len[lo] != len) return;
    if constexpr (INS) {
        const uint8_t *mine = a.ins_ledger_bases + bases_offset, *theirs = a.site_bases + a.site_bases_offset[lo];
        for (uint32_t x = 0; x < len; ++x)
            if (mine[x] != theirs[x]) return;
    }
    atomicAdd(a.count_reverse + lo, 1u);
}

uint32_t strand_blocks(uint64_t n) { return (uint32_t)((n + STRAND_THREADS - 1) / STRAND_THREADS); }
} // namespace

int dcn_launch_strand_evidence(const dcn_strand_evidence_args &args, hipStream_t stream) {
    if (args.n == 0) return DCN_OK;
    hipLaunchKernelGGL(strand_evidence_kernel, dim3(strand_blocks(args.n)), dim3(STRAND_THREADS), 0, stream, args);
    DCN_HIP(hipGetLastError());
    return DCN_OK;
}

int dcn_launch_indel_strand(const dcn_indel_strand_args &args, hipStream_t stream) {
    if (args.n_sites == 0) return DCN_OK;
    if (args.n_ins_events) {
        hipLaunchKernelGGL(indel_strand_kernel<true>, dim3(strand_blocks(args.n_ins_events)), dim3(STRAND_THREADS), 0, stream, args);
        DCN_HIP(hipGetLastError());
    }
    if (args.n_del_events) {
        hipLaunchKernelGGL(indel_strand_kernel<false>, dim3(strand_blocks(args.n_del_events)), dim3(STRAND_THREADS), 0, stream, args);
        DCN_HIP(hipGetLastError());
    }
    return DCN_OK;
}
