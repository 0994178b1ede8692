/*
 * deacon_hip_phase.h -- read-backed phasing of heterozygous sites: the part of the C ABI added with ABI 1.25.
 *
 * (no reference counterpart.)  The pileup's counters are sums per position: the right sufficient statistic for a genotype,
 * and one that destroys co-occurrence by construction.  Which allele of one heterozygous site travels with which allele of
 * the next on one molecule is what compound-heterozygote analysis, allele-specific work and every haplotype tool ask, and
 * the reads that answer it are the aligned rows themselves: every row that covers two sites shows one combination.  This
 * header defines that evidence (links), the decision over it and the phase sets that follow, and computes all three on the
 * device: a second look at the rows once the sites are known, which touches memory only at the listed sites.
 *
 * The conventions are those of deacon_hip.h, which this header includes.  The functions are declared here and not there
 * so that the set of deacon_hip.h stays what bindings of ABI 1.23 enumerate; the library exports them like any other.
 *
 * THE DEFINITION OF A PHASE.  Rules P1-P6, Q1-Q6 and N1-N8 stand.  Added:
 *   H1.  Sites.  A map holds at most one site list: entries (record, pos, a0, a1), strictly ascending in (record, pos),
 *        a0 != a1 and both in A C G T (columns 0 .. 3), pos inside the record.  Setting a list replaces the old one and
 *        zeroes all links; n = 0 frees it.
 *   H2.  Observation.  A row is what P2 calls a counted row: it has an alignment and n > 0.  Its observation at a listed
 *        site is defined only if the site lies in its record interval, and is the pileup column that P3 (with Q3, when
 *        qualities are given) would have incremented there for that row: allele 0 if that column is a0, allele 1 if it is
 *        a1, otherwise NONE (another base, N, a base under min_base_qual, DEL).  Inserted runs do not observe.  While the
 *        map's left-align switch is on the runs are N5's, exactly as for the pileup (N8): phase and pileup see the same
 *        columns.
 *   H3.  Link.  Link s joins site s and site s + 1 of the list when both are of one record.  It has four 32-bit counters
 *        n[x][y].  A row adds 1 to n[x][y] of link s when its observations at s and s + 1 are x and y, both defined.  A
 *        site with observation NONE does not bridge its neighbours.  Each row counts on its own.
 *   H4.  The adds commute: links do not depend on batch cuts, on the order of rows, or on grid and lanes.
 *   H5.  Decision.  c = n00 + n11, t = n01 + n10, N = c + t, minor = min(c, t), all in 64 bits.  Link s is JOINED when
 *        N >= max(1, min_reads), c != t and minor * 1000 <= N * max_minor_permille.  Its relation is r = (t > c).
 *   H6.  Sets.  Site s is a HEAD when s == 0, when link s - 1 does not exist (record change), or when link s - 1 is not
 *        joined.  hap[head] = 0; hap[s] = hap[s - 1] XOR r[s - 1].  set_pos[s] is the pos of its head, set_index[s] the
 *        number of heads before its head.  Haplotype 1 carries a[hap], haplotype 2 a[1 - hap].
 *   H7.  A set of one site is unphased.
 *   H8.  Integers only.  The result is a function of the link counters and the three parameters, unique while no counter
 *        has wrapped.
 *   H9.  Cuts do not matter for the solve: it is defined on the whole list.
 *   H10. Stated limits.  Adjacent-in-list links only: a false heterozygous site between two true ones splits a set.  No
 *        links across mates or across split rows of one read, which are separate rows.  SNV sites only.  Per-read
 *        haplotype tags are not produced.  min_reads = 2 and max_minor_permille = 200 of the layers above are
 *        conventions, not measured optima.
 */
#ifndef DEACON_HIP_PHASE_H
#define DEACON_HIP_PHASE_H

#include "deacon_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCN_PHASE_HEAD 1u   /* dcn_phase_result.flags: the site is the head of its set (H6) */
#define DCN_PHASE_JOINED 2u /* ... and: link s, to the next site, is joined (H5) */
typedef struct dcn_phase_site {
    uint64_t pos;         /* record-relative, 0-based */
    uint32_t record;
    uint8_t a0, a1;       /* columns 0 .. 3 (DCN_PILEUP_A .. DCN_PILEUP_T), a0 != a1 */
    uint8_t reserved[2];  /* must be 0 */
} dcn_phase_site;         /* 16 bytes */
typedef struct dcn_phase_params {
    uint32_t min_reads;
    uint32_t max_minor_permille; /* 0 .. 1000 */
    uint32_t reserved[2];        /* must be 0 */
} dcn_phase_params;              /* 16 bytes */
typedef struct dcn_phase_result {
    uint64_t set_pos;     /* H6: the pos of the head of the site's set */
    uint32_t link[4];     /* n00 n01 n10 n11 of link s; 0 where there is none */
    uint32_t set_index;   /* H6: heads in front of the set's head, over the whole list */
    uint8_t hap;          /* H6 */
    uint8_t flags;        /* DCN_PHASE_HEAD | DCN_PHASE_JOINED */
    uint8_t reserved[2];  /* 0 */
} dcn_phase_result;       /* 32 bytes */

/* Rule H1: the site list of an anchor map that keeps bases; n_sites dcn_phase_site entries (declared void * for the reason
 * given at dcn_locate_batch).  DCN_ERR_ARG, each naming the first offending entry as sites[i]: reserved bytes that are not
 * 0, a record that was not added, a pos outside the record, an allele above 3, a0 == a1, an entry that does not lie behind
 * the one in front of it.  A list holds at most 2^32 - 2 sites.  An error leaves the old list as it was.  n_sites = 0
 * frees the list (sites may be NULL).  33 B of device memory per site.  Blocking. */
int dcn_anchor_map_phase_sites(dcn_index *map, const void *sites, uint64_t n_sites);

/* info[0 .. 4): the sites of the list, the rows handed in since the list was set that P2 counts, those of them that added
 * to at least one link, and the link adds.  All 0 on a map without a list. */
int dcn_anchor_map_phase_info(const dcn_index *map, uint64_t info[4]);

/* Rules H2-H4: dcn_pileup_batch_qual's rows looked at once more, at the listed sites alone.  Arguments, checks and messages
 * are dcn_pileup_batch_qual's, in its order, with these differences: the map needs a site list in place of a pileup
 * (DCN_ERR_ARG "the map has no phase sites"); quals and qual_params are both NULL (no Q3) or both given, one without the
 * other is DCN_ERR_ARG; *n_linking (may be NULL) receives the rows of this call that added to at least one link.  `edits`
 * come back as dcn_align_batch gives them.  It needs no pileup and writes to no pileup counter, ledger or plane; the
 * left-align switch of the map (N8) holds as for the pileup.
 * One context at a time adds to a map's links, as to its pileup: the two counters behind n_linking and the info live with
 * the list and are cleared and read by each call.
 * One wave per aligned row over align's work list, DCN_GRID_CUS as for the pileup kernel: a search for the first site in the
 * row's interval, and a row with fewer than two sites there ends without reading its runs. */
int dcn_phase_batch(dcn_ctx *ctx, dcn_index *map, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets, uint32_t n_reads,
                    const void *params, const void *qual_params, const uint64_t *row_offsets, const void *rows, uint64_t n_rows,
                    uint32_t *edits, uint64_t *n_linking);

/* The counters of sites [first, first + n) of the list: four per site, n00 n01 n10 n11 of link s (H3), 0 where the link
 * does not exist.  DCN_ERR_ARG on a map without a list, a range past the list, links NULL with n > 0.  Blocking. */
int dcn_anchor_map_phase_links(const dcn_index *map, uint64_t first, uint64_t n, uint32_t *links);

/* Rules H5-H7 over the whole list: params a dcn_phase_params, results one dcn_phase_result per site of the list (both
 * declared void * likewise).  DCN_ERR_ARG, in this order: params NULL, reserved != 0, max_minor_permille above 1000, a map
 * without a list, results NULL.  Blocking, on the null stream with scratch of the call: a pass that decides every link, and
 * a segmented scan over the sites in three passes (per workgroup, over the workgroups' aggregates, apply), deterministic. */
int dcn_anchor_map_phase_solve(const dcn_index *map, const void *params, void *results);

#ifdef __cplusplus
}
#endif
#endif /* DEACON_HIP_PHASE_H */
