/*
 * deacon_hip_blocks.h -- reference blocks over a pileup: the part of the C ABI added with ABI 1.24.
 *
 * (no reference counterpart.)  dcn_anchor_map_genotype reports the positions where a record's sample differs from it.  It
 * says nothing about the others, and a reader of its sites cannot tell "homozygous reference, forty reads, GQ 99" from "no
 * read landed here" or from "three reads, no call".  Joint calling, comparison with a truth set, "is my gene covered" and a
 * consensus that must not invent reference bases all need that distinction; the usual carriers are a gVCF (reference blocks
 * between the variant lines) and a BED of callable regions.  Both are a segmentation of a record into maximal runs of equal
 * confidence, which is what this header defines and computes on the device, from the counters and sums already there.
 *
 * The conventions are those of deacon_hip.h, which this header includes.  The functions are declared here and not there
 * so that the set of deacon_hip.h stays what bindings of ABI 1.23 enumerate; the library exports them like any other.
 *
 * THE DEFINITION OF A REFERENCE BLOCK.  Rules P1-P6, Q1-Q6 and G1-G8 stand.  Added:
 *   B1. Inputs.  A map that keeps quality sums (Q1); a range [start, start + n) of one record; the genotype parameters of
 *       G1-G8; n_edges (0 .. 15) GQ edges e[0] < e[1] < ..., each in 1 .. 99; and a list of break positions inside the
 *       range, in any order, duplicates allowed.
 *   B2. Class of a position p.  g is the result of G1-G7 at p, depth is P4's (six columns), D is G1's (four columns).
 *         DCN_BLOCK_VARIANT (255)   when p is a break or g is a site (G7);
 *         DCN_BLOCK_NO_COVERAGE (0) otherwise, when depth == 0;
 *         DCN_BLOCK_REF + b (2 + b) otherwise, when the position is called (G6), the reference base is valid and the best
 *                                   genotype is ref/ref (ref at ploidy 1); b is the number of edges <= GQ, 0 <= b <= n_edges;
 *         DCN_BLOCK_UNCALLED (1)    otherwise: D below min_depth, GQ below min_gq, a called non-reference genotype with
 *                                   QUAL below min_qual, a covered position whose reference base is invalid, a position
 *                                   covered only by N or DEL.
 *   B3. Blocks.  A block is a maximal run of consecutive positions of the range with one class other than VARIANT.
 *       VARIANT positions belong to no block; two runs of one class with a VARIANT position between them are two blocks.
 *   B4. A block's numbers, all over the block's positions: pos and len; cls; min_gq, the minimum of G4's GQ, called or
 *       not; min_depth, max_depth and sum_depth over D, the last in 64 bits.
 *   B5. Order.  Blocks come in ascending pos; the count is always reported.
 *   B6. Merge.  Two blocks TOUCH when a.pos + a.len == b.pos.  Touching blocks of one class merge into one: len and
 *       sum_depth add, the minima and the maximum combine.
 *   B7. Cuts do not matter.  The blocks of [s, s + n), with the breaks inside it, equal the blocks of [s, s + m) followed
 *       by the blocks of [s + m, s + n), each half with the breaks inside it, merged by B6 -- for every m.  This is what
 *       lets a caller work stretch by stretch.
 *   B8. Integers only.  The result is a function of the ten counters and sums per position, the reference bases, the
 *       parameters and the set of breaks, unique while nothing has wrapped.  It does not depend on grid, lanes or order.
 *   B9. Stated limits.  The positions under a deletion that most reads carry have D = 0 and depth > 0: they show as
 *       UNCALLED and are not excluded.  Indel candidates do not influence a class except through the breaks the caller
 *       passes.  The default edges of the layers above (20, 40, 60, 80, 99) are a convention, not a measured optimum.
 */
#ifndef DEACON_HIP_BLOCKS_H
#define DEACON_HIP_BLOCKS_H

#include "deacon_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCN_BLOCK_NO_COVERAGE 0u
#define DCN_BLOCK_UNCALLED 1u
#define DCN_BLOCK_REF 2u /* + band, 2 .. 17 */
#define DCN_BLOCK_VARIANT 255u
typedef struct dcn_block_params {
    uint32_t ploidy;      /* the six of dcn_genotype_params, with its limits */
    uint32_t min_depth;
    uint32_t min_gq;
    uint32_t min_qual;
    uint32_t err_centi;
    uint32_t het_centi;
    uint32_t n_edges;     /* 0 .. 15 */
    uint32_t reserved;    /* must be 0 */
    uint8_t edges[16];    /* strictly ascending, 1 .. 99; entries from n_edges on must be 0 */
} dcn_block_params;       /* 48 bytes */
typedef struct dcn_reference_block {
    uint64_t pos;         /* record-relative, 0-based */
    uint64_t sum_depth;   /* B4: the sum of D */
    uint32_t len;
    uint32_t min_depth;
    uint32_t max_depth;
    uint32_t min_gq;
    uint32_t cls;         /* DCN_BLOCK_NO_COVERAGE, DCN_BLOCK_UNCALLED or DCN_BLOCK_REF + band */
    uint32_t reserved;    /* 0 */
} dcn_reference_block;    /* 40 bytes */

/* Rules B1-B9 over positions [start, start + n_bases) of a record.
 *   params      a dcn_block_params (declared void * for the reason given at dcn_locate_batch).  DCN_ERR_ARG, in this order:
 *               NULL, reserved != 0, a ploidy other than 1 or 2, min_gq > 99, err_centi or het_centi above 100000 (the
 *               messages of dcn_anchor_map_genotype); then n_edges > 15, an edge outside 1 .. 99, edges that do not ascend
 *               strictly, an entry from n_edges on that is not 0
 *   breaks      n_breaks record positions inside the range (NULL when n_breaks is 0); one outside is DCN_ERR_ARG naming the
 *               first such index, and nothing is written
 *   cls         NULL, or n_bases bytes (B2)
 *   blocks      dcn_reference_block entries in ascending pos (declared void * likewise), capacity of them
 *   n_blocks    always receives the number of blocks there is
 * The checks run in this order: the parameters', the map's as dcn_anchor_map_genotype makes them (no pileup, no quality
 * sums), the range errors as for dcn_anchor_map_fetch, n_blocks NULL, the breaks.  A range of more than 2^32 - 1 positions
 * is DCN_ERR_ARG (len is 32 bits: ask stretch by stretch and merge).  n_bases = 0 succeeds.  DCN_ERR_CAPACITY when
 * capacity is smaller: cls is complete and no block is written; NULL with capacity 0 asks for the count
 * (dcn_anchor_map_genotype's protocol).
 * Blocking, on the null stream with scratch of the call (two bytes per position and the blocks): a pass that classifies
 * (40 B read per position), a thread per break, a pass that counts the block heads per workgroup, a scan of those counts,
 * and a pass that reduces by block index inside each wave and combines with atomics, one set per wave segment.  The grids
 * are sized by the range (DCN_GRID_CUS does not apply).  No memory on the map and no pass over reads. */
int dcn_anchor_map_reference_blocks(const dcn_index *map, const void *params, uint32_t record, uint64_t start, uint64_t n_bases,
                                    const uint64_t *breaks, uint64_t n_breaks, uint8_t *cls, void *blocks, uint64_t capacity,
                                    uint64_t *n_blocks);

/* Rule B6 in place over n blocks in ascending pos (dcn_reference_block entries, declared void * likewise): *n_merged
 * receives how many remain, at the front of the array.  Host only; it makes no device call.  DCN_ERR_ARG when blocks is
 * NULL with n > 0, n_merged is NULL, the blocks are not in ascending, non-overlapping order (a.pos + a.len > b.pos), or a
 * merged len would pass 2^32 - 1; the array is unchanged then. */
int dcn_reference_blocks_merge(void *blocks, uint64_t n, uint64_t *n_merged);

#ifdef __cplusplus
}
#endif
#endif /* DEACON_HIP_BLOCKS_H */
