// dcn_verify.h -- kept reference bases of an anchor map, the launch shape of the wavefront kernels, the verify kernel's
// arguments, the host side that every row call shares (checks, walk, front end), the align kernels' arguments, the host side that align and pileup share, the pileup kernels' arguments and
// the extend kernel's (internal; verify.hip, verify_api.hip, align.hip, align_api.hip, pileup.hip, pileup_api.hip,
// extend.hip, extend_api.hip, and place_api.hip for the append of dcn_anchor_map_add).
#pragma once

#include "dcn_internal.h"

#include <cstring>
#include <vector>

// The bases of every record added to a map after dcn_anchor_map_keep_bases, as the pack kernel leaves them: one 2-bit
// stream and one invalid-base bit per base (0.375 B per base).  Every add call starts at a 32-base-aligned offset of the
// store, so its append is two device-to-device copies of whole words; record R starts at rec_start[R] = that offset +
// offsets[r] of its call, anywhere within a word.  cap and used are bases, multiples of 32; both arrays end in
// DCN_STORE_PAD_WORDS readable words (dcn_wavefront.h reads one word past a base).
constexpr uint64_t DCN_STORE_PAD_WORDS = 8;
constexpr uint64_t DCN_STORE_INITIAL_BASES = 1ull << 24;
struct dcn_base_store {
    uint32_t *d_packed = nullptr, *d_invmask = nullptr;
    uint64_t cap = 0, used = 0;
    std::vector<uint64_t> rec_start; // per record: its first base in the store
    std::vector<uint32_t> rec_len;   // ... and its length (the host's copy: what rows are checked against)
};
void dcn_base_store_free(dcn_base_store *s);
// Appends the batch that the front end has just packed into `packed` / `invmask` (views behind DCN_FRONT_PAD) on `stream`:
// grows the store, enqueues the two copies and returns where the batch begins.  Nothing of the store's host state
// changes: the caller commits with dcn_base_store_commit once the run has succeeded.
int dcn_base_store_append(dcn_base_store *s, const uint32_t *packed, const uint32_t *invmask, uint64_t n_bases, hipStream_t stream,
                          uint64_t *batch_start);
void dcn_base_store_commit(dcn_base_store *s, uint64_t batch_start, const uint64_t *offsets, uint32_t n_records);

// The launch of a wavefront kernel (verify.hip, align.hip, extend.hip): one-wave workgroups that stride over n work items
// (at most 32 are resident per CU; four times that many), each with `arrays` wavefront arrays of lds_stride words of
// dynamic LDS.
struct dcn_wave_grid {
    uint32_t blocks;
    size_t lds_bytes;
};
#pragma GCC visibility push(hidden)
inline dcn_wave_grid dcn_wave_grid_for(uint64_t n, uint32_t arrays, uint32_t lds_stride) {
    const uint64_t resident = (uint64_t)dcn_cu_count() * 32;
    return {(uint32_t)(n < resident * 4 ? n : resident * 4), ((size_t)lds_stride * arrays * sizeof(uint32_t) + 15) / 16 * 16};
}
#pragma GCC visibility pop

// One row as the kernel takes it: the host has checked the row against the read and the record and resolved both
// intervals to stream positions (the kernel trusts nothing the host has not checked).
struct dcn_verify_item {
    int64_t s_origin; // the read interval in the batch stream: its first base, or its end when reverse
    int64_t t_origin; // the first base of the record interval in the store
    uint32_t m, n;    // |S|, |T|
    uint32_t E;       // rule 4's threshold
    uint32_t flags;   // bit 0: reverse; bit 1: unplaced (nothing else is read)
};
static_assert(sizeof(dcn_verify_item) == 32, "verify item");

struct dcn_verify_args {
    const dcn_verify_item *items;
    uint64_t n_rows;
    const uint32_t *s_packed, *s_invmask; // the batch: views behind DCN_FRONT_PAD
    const uint32_t *t_packed, *t_invmask; // the store
    uint32_t lds_stride;                  // words of one wavefront array: >= 2 * (the largest E of the call) + 1
    uint32_t *out;
};
int dcn_launch_verify(const dcn_verify_args &args, hipStream_t stream);

// ---- the host side of a row call: dcn_verify_batch, dcn_align_batch, dcn_pileup_batch, dcn_extend_batch (verify_api.hip) ----
// What every row call is given.  max_permille is rule 4's and has no say in dcn_extend_batch, which leaves it 0.
struct dcn_row_call {
    dcn_ctx *ctx;
    const dcn_index *map;
    const uint8_t *bases;
    const uint64_t *offsets;
    uint32_t n_reads;
    uint32_t max_edits, max_permille, row_stride;
    const uint64_t *row_offsets;
    const void *rows;
    uint64_t n_rows;
};

#pragma GCC visibility push(hidden)
namespace dcn_impl {
// the map is an anchor map that keeps bases
int check_store(const dcn_index *map);
// the range [start, start + n_bases) of a record of such a map -> its first base in the store; `who` begins the messages
int check_range(const dcn_index *map, const char *who, uint32_t record, uint64_t start, uint64_t n_bases, uint64_t *base0);

// The checks that a row call makes once, behind those of its own parameters' other fields, in the order their messages
// promise: max_edits, max_permille, row_stride, the context, the map, the batch and row_offsets.  *run is whether there is
// anything to walk (reads and rows; `rows` is not NULL then); *n_bases the bases of the batch.
int rows_check(const dcn_row_call &call, bool *run, uint64_t *n_bases);
// Two parts of rows_check for a call that has no context and no bases (dcn_mark_duplicates_batch): the row_stride, and
// everything behind the context and the map -- n_rows against n_reads, offsets, row_offsets, rows.  With call.ctx NULL
// the offsets are walked without a context's limits and call.bases is not looked at.
int rows_stride_check(uint32_t row_stride);
int rows_shape_check(const dcn_row_call &call, bool *run, uint64_t *n_bases);

// The walk over the rows of a checked call: every placed row against its read and its record, then
// row_fn(row, placement, read_offset, read_length, record_start, record_length), which makes of the row what its kernel
// takes.  An unplaced row (record == UINT32_MAX) is handed over unchecked, with a record of 0 bases at 0.
// A map that keeps no bases (dcn_mark_duplicates_batch alone walks one) has no record lengths on the host: its rows are
// checked against the number of records added, ref_end against nothing, and row_fn gets a record of 0 bases at 0.
template <typename RowFn>
int rows_walk(const dcn_row_call &call, RowFn &&row_fn) {
    const dcn_base_store *store = call.map->store;
    const uint64_t n_records = store ? store->rec_len.size() : call.map->anchor_records;
    uint64_t row = 0;
    for (uint32_t r = 0; r < call.n_reads; ++r) {
        const uint64_t row_end = call.row_offsets ? call.row_offsets[r + 1] : (uint64_t)r + 1;
        const uint64_t read_len = call.offsets[r + 1] - call.offsets[r];
        for (; row < row_end; ++row) {
            dcn_placement p;
            memcpy(&p, static_cast<const uint8_t *>(call.rows) + row * call.row_stride, sizeof(p));
            if (p.record == UINT32_MAX) {
                row_fn(row, p, call.offsets[r], read_len, (uint64_t)0, (uint64_t)0);
                continue;
            }
            // (the message is put together only when a row is wrong: ten million rows are walked here per call)
            const auto bad = [row](const std::string &what) { return dcn_fail(DCN_ERR_ARG, "row " + std::to_string(row) + ": " + what); };
            if (p.record >= n_records)
                return bad("record " + std::to_string(p.record) + " of " + std::to_string(n_records) + " added");
            if (p.reverse > 1) return bad("reverse must be 0 or 1");
            if (p.read_start > p.read_end) return bad("read_start is behind read_end");
            if (p.read_end > read_len)
                return bad("read_end " + std::to_string(p.read_end) + " is past the read's " + std::to_string(read_len) + " bases");
            if (p.ref_start > p.ref_end) return bad("ref_start is behind ref_end");
            if (!store) {
                row_fn(row, p, call.offsets[r], read_len, (uint64_t)0, (uint64_t)0);
                continue;
            }
            const uint64_t rec_len = store->rec_len[p.record];
            if (p.ref_end > rec_len)
                return bad("ref_end " + std::to_string(p.ref_end) + " is past the record's " + std::to_string(rec_len) + " bases");
            row_fn(row, p, call.offsets[r], read_len, store->rec_start[p.record], rec_len);
        }
    }
    return DCN_OK;
}

// The front end of a row call on the context's device: the items go to d_items, the batch is staged, the status cleared,
// the run begun (*prof_slot_out) and the batch packed, with the marks of the four stages up to DISTINCT (no plan, no
// scan: their slots stay empty).  The run stays open: the caller launches its kernels, marks FINISH and calls finish_run.
int rows_front(dcn_ctx *c, void *d_items, const void *items, uint64_t item_bytes, const uint8_t *bases, uint64_t n_bases,
               const uint64_t *offsets, uint32_t n_reads, int *prof_slot_out);
} // namespace dcn_impl
#pragma GCC visibility pop

// What verify's walk over a call's rows leaves: one checked item per row, the largest threshold of a row that needs a
// wavefront, and the bases of the batch.
struct dcn_verify_plan {
    std::vector<dcn_verify_item> items;
    uint32_t e_max = 0;
    uint64_t n_bases = 0;
};
// every check of dcn_verify_batch, in its order and with its messages; items stays empty when there is nothing to run
int dcn_verify_walk(dcn_ctx *ctx, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                    const void *params, const uint64_t *row_offsets, const void *rows, uint64_t n_rows, const uint32_t *edits,
                    dcn_verify_plan *plan);
// rows_front and the verify kernel: the run stays open behind the DISTINCT mark (the caller marks FINISH and calls
// finish_run), the edits are in ctx->d_vfy_out and the items in ctx->d_vfy_items
int dcn_verify_enqueue(dcn_ctx *c, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                       const dcn_verify_plan &plan, int *prof_slot_out);

// ---- aligned placements (align.hip, align_api.hip; the trace and the walk back are in dcn_align.h) ------------------
// One aligned row (edits = d <= E) of a call, in row order.  The host has summed the trace sizes (d + 1)^2 and the op
// bounds 2 d + 1 of the rows in front of it.
struct dcn_align_work {
    uint64_t trace_base; // words of trace in front of this row, over the whole call (a group subtracts its first row's)
    uint64_t slot_end;   // the end of this row's slot of 2 d + 1 runs: the runs are written downwards from here
    uint32_t row, d;
};
static_assert(sizeof(dcn_align_work) == 24, "align work item");

struct dcn_align_args {
    const dcn_verify_item *items; // the call's rows, as the verify kernel took them
    const dcn_align_work *work;
    uint64_t w0, w1;              // the group: work items [w0, w1)
    const uint32_t *s_packed, *s_invmask, *t_packed, *t_invmask;
    uint32_t lds_stride;          // words of one wavefront array: >= 2 * (the largest d of the call) + 1
    uint32_t *trace;              // the group's trace: item w's begins at work[w].trace_base - trace_origin
    uint64_t trace_origin;        // work[w0].trace_base
    uint32_t *slots;              // the call's run slots
    uint32_t *n_ops;              // per row of the call (zero before: a row that is not aligned has no runs)
};
int dcn_launch_align(const dcn_align_args &args, hipStream_t stream);

struct dcn_align_gather_args {
    const dcn_align_work *work;
    uint64_t n_work;
    const uint32_t *slots, *n_ops;
    const uint64_t *cigar_offsets; // n_rows + 1: the scan of n_ops
    uint32_t *cigar;
};
int dcn_launch_align_gather(const dcn_align_gather_args &args, hipStream_t stream);

// the left alignment of the rows' runs in their slots, behind the last align kernel (left_align.hip, dcn_left_align.h)
struct dcn_left_align_args {
    const dcn_verify_item *items;
    const dcn_align_work *work;
    uint64_t n_work;
    const uint32_t *s_packed, *s_invmask, *t_packed, *t_invmask;
    uint32_t *slots;            // the call's run slots: a changed row's runs end at its slot_end again
    uint32_t *scratch;          // as many words as the slots: a row builds its new runs in the words of its own slot
    uint32_t *n_ops;            // per row of the call: a changed row's is written again
    unsigned long long *totals; // rows changed, gaps shifted, columns passed, gaps merged: added to
};
int dcn_launch_left_align(const dcn_left_align_args &args, hipStream_t stream);

// ---- the host side that dcn_align_batch and dcn_pileup_batch share (align_api.hip) -----------------------------------
// align's own rules over a walked call: fewer than 2^32 rows, and no placed row with an interval of 2^28 bases or more
int dcn_align_check_rows(const dcn_verify_plan &plan);
// verify, the read-back of the edits, the work list, the align kernel of every trace group and the scan of the run
// counts, then a wait: the edits are in `edits`, the run counts in c->d_aln_n_ops, their offsets in c->d_aln_offsets, the
// runs in the slots.  The run stays open behind the DISTINCT mark, as dcn_verify_enqueue leaves it.
// `left` not null: the left-align kernel runs behind the last align kernel and in front of the scan, and its four totals
// are read back into *left.  Null: not one launch, copy or allocation more than before.
struct dcn_la_totals; // (dcn_left_align.h)
int dcn_align_runs(dcn_ctx *c, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                   const dcn_verify_plan &plan, uint32_t *edits, int *prof_slot_out, uint64_t *n_work_out, dcn_la_totals *left);
// the gather of `total` > 0 runs from the slots into c->d_aln_cigar, which grows to hold them
int dcn_align_gather_runs(dcn_ctx *c, uint64_t n_work, uint64_t total);

// ---- pileup (pileup.hip, pileup_api.hip; the shared arithmetic is in dcn_pileup.h) ----------------------------------
struct dcn_pileup_args {
    const dcn_verify_item *items; // the call's rows, as the verify kernel took them
    const dcn_align_work *work;   // the aligned ones
    uint64_t n_work;
    const uint32_t *s_packed, *s_invmask; // the batch: views behind DCN_FRONT_PAD
    const uint32_t *n_ops;                // per row of the call
    const uint64_t *cigar_offsets;        // ... and where its runs begin
    const uint32_t *cigar;
    uint32_t *counters; // the map's pileup: dcn_pile_index(column, store base, bases)
    uint64_t bases;
};
int dcn_launch_pileup(const dcn_pileup_args &args, hipStream_t stream);

// the same walk with base qualities (dcn_pileup_batch_qual): rules Q2 - Q4
struct dcn_pileup_qual_args {
    dcn_pileup_args rows;
    const uint8_t *quals; // one byte per base of the batch, parallel to the stream behind s_packed
    uint32_t *sums;       // the map's quality sums: dcn_pile_sum_index(column, store base, rows.bases); null: none are kept
    uint32_t qual_offset, min_base_qual;
};
int dcn_launch_pileup_qual(const dcn_pileup_qual_args &args, hipStream_t stream);

// either walk on a map that keeps strand planes (rule S2): the planes ride behind the arguments of the kernel it was, so
// that the kernels of a map without planes take the arguments they took
template <typename Rows>
struct dcn_pileup_strand_args {
    Rows rows;
    uint32_t *strands; // the map's strand planes: dcn_pile_strand_index(column, store base, bases)
};
int dcn_launch_pileup_strand(const dcn_pileup_args &args, uint32_t *strands, hipStream_t stream);
int dcn_launch_pileup_qual_strand(const dcn_pileup_qual_args &args, uint32_t *strands, hipStream_t stream);

struct dcn_pileup_call_args {
    const uint32_t *counters;
    uint64_t bases;
    const uint32_t *t_packed, *t_invmask; // the store
    uint64_t base0, n;                    // the range: store bases [base0, base0 + n)
    uint64_t pos0;                        // ... and the record position of its first base
    uint32_t min_depth, min_permille;
    uint8_t *calls;                // n characters (the counting pass)
    uint32_t *block_counts;        // sites per workgroup (the counting pass)
    const uint64_t *block_offsets; // their scan (the writing pass)
    uint64_t *site_pos;
    uint32_t *site_info;
};
uint32_t dcn_pileup_call_blocks(uint64_t n); // workgroups of a range of n positions
int dcn_launch_pileup_call(const dcn_pileup_call_args &args, bool write, hipStream_t stream);

// what the range calls over a pileup share on the host (pileup_api.hip defines the checks; genotype_api.hip uses them too)
#pragma GCC visibility push(hidden)
namespace dcn_pile_api {
// the map is an anchor map that keeps bases and has a pileup
int check_pileup(const dcn_index *map);
// ... and keeps quality sums
int check_qsums(const dcn_index *map);
// ... or keeps strand planes
int check_strands(const dcn_index *map);
// (their scratch holder, dcn_pile_api::scratch, is in dcn_ctx.h, where dev_alloc is)
} // namespace dcn_pile_api
#pragma GCC visibility pop

// ---- phase (phase.hip, phase_api.hip; the shared arithmetic is in dcn_phase.h) -----------------------------------------
// The site list of a map (dcn_anchor_map_phase_sites, rule H1) and the links over it, all on the device: per site its
// base-store position (ascending: the store's records begin in the order they were added), its record position, a byte of
// alleles (dcn_phase_pack_alleles, and DCN_PHASE_LINK_BIT when link s exists) and the four counters of link s; the two
// counters of a call (rows that linked, link adds); and on the host rule H1's info, summed over the calls.
constexpr uint32_t DCN_PHASE_LINK_BIT = 16;
struct dcn_phase_list {
    uint64_t n = 0;
    uint64_t *d_base = nullptr, *d_pos = nullptr;
    uint8_t *d_alleles = nullptr;
    uint32_t *d_links = nullptr;
    unsigned long long *d_call = nullptr;
    uint64_t rows = 0, rows_linking = 0, link_adds = 0;
};
void dcn_phase_list_free(dcn_phase_list *l);

struct dcn_phase_link_args {
    dcn_pileup_args rows; // the pileup kernel's view of the call's rows; counters and bases are not looked at
    const uint8_t *quals; // as dcn_pileup_qual_args (the <true> kernel alone reads the three)
    uint32_t qual_offset, min_base_qual;
    const uint64_t *site_base;
    const uint8_t *site_alleles;
    uint64_t n_sites;
    uint32_t *links;
    unsigned long long *call; // [0] += rows that added to a link, [1] += link adds
};
int dcn_launch_phase_link(const dcn_phase_link_args &args, bool qual, hipStream_t stream);

struct dcn_phase_elem; // (dcn_phase.h)
struct dcn_phase_solve_args {
    const uint64_t *site_pos;
    const uint8_t *site_alleles;
    const uint32_t *links;
    uint64_t n_sites;
    uint32_t min_reads, max_minor_permille;
    uint8_t *decisions;         // per site: dcn_phase_decide of link s, 0 where there is none
    dcn_phase_elem *aggregates; // per workgroup of the scan: its sites' element, then the element of all sites in front
    void *results;              // dcn_phase_result per site
};
uint64_t dcn_phase_solve_blocks(uint64_t n_sites); // workgroups of the scan: entries of `aggregates`
int dcn_launch_phase_solve(const dcn_phase_solve_args &args, hipStream_t stream);

// ---- genotypes (genotype.hip, genotype_api.hip; the shared arithmetic is in dcn_genotype.h) ---------------------------
struct dcn_genotype_args {
    const uint32_t *counters, *sums; // the map's pileup and its quality sums
    uint64_t bases;
    const uint32_t *t_packed, *t_invmask; // the store
    uint64_t base0, n;                    // the range: store bases [base0, base0 + n)
    uint64_t pos0;                        // ... and the record position of its first base
    uint32_t ploidy, min_depth, min_gq, min_qual, err_centi, het_centi;
    // per position of the range, each behind a pad of base0 & 3 bytes: byte (base0 & 3) + q belongs to position q, so that
    // the byte of a store base divisible by 4 lies on a word of the buffer (the counting pass; dcn_genotype_out_bytes each)
    uint8_t *gt, *gq;
    uint32_t *block_counts;        // sites per workgroup (the counting pass)
    const uint64_t *block_offsets; // their scan (the writing pass)
    void *sites;                   // dcn_genotype_site per site
};
uint32_t dcn_genotype_blocks(uint64_t base0, uint64_t n);    // workgroups of a range
uint64_t dcn_genotype_out_bytes(uint64_t base0, uint64_t n); // bytes of args.gt and of args.gq
int dcn_launch_genotype(const dcn_genotype_args &args, bool write, hipStream_t stream);

// ---- duplicate marking (duplicates.hip, duplicates_api.hip; the shared arithmetic is in dcn_duplicates.h) ---------------
struct dcn_dup_item; // (dcn_duplicates.h)
struct dcn_dup_key;
// The duplicate set of a map (dcn_anchor_map_duplicates_enable): the key log, one 48-byte key per unit handed in since the
// last reset, indexed by ordinal and growing geometrically; the table of 8-byte slots, each an ordinal or DCN_DUP_EMPTY, a
// power of two of them that starts at DCN_DUPLICATE_TABLE_SLOTS (read when the set first grows) and doubles; rule D1's
// three counters, which live on the host; and the buffers of a call, which live with the set and only grow.
struct dcn_dup_set {
    dcn_dup_key *d_log = nullptr;
    uint64_t log_cap = 0;
    unsigned long long *d_slots = nullptr;
    uint64_t n_slots = 0;
    uint64_t seen = 0, keyed = 0, keys = 0;
    dcn_dup_item *d_items = nullptr;
    uint64_t items_cap = 0;
    uint8_t *d_dup = nullptr;
    uint64_t dup_cap = 0;
    uint64_t *d_first = nullptr;
    uint64_t first_cap = 0;
    unsigned long long *d_n_dup = nullptr;
};
void dcn_dup_set_free(dcn_dup_set *d);

struct dcn_dup_args {
    const dcn_dup_item *items; // one per read of the call
    uint64_t n_units, ord0;    // unit u has ordinal ord0 + u
    uint32_t paired, both_ends;
    dcn_dup_key *log;          // by ordinal
    unsigned long long *slots;
    uint64_t mask;             // slots - 1
    uint8_t *dup;              // per unit
    uint64_t *first;
    unsigned long long *n_dup; // added to
};
int dcn_launch_dup_keys(const dcn_dup_args &args, hipStream_t stream);
int dcn_launch_dup_insert(const dcn_dup_args &args, hipStream_t stream);
int dcn_launch_dup_lookup(const dcn_dup_args &args, hipStream_t stream);
// every occupied slot of old_slots[0, n_old) into args.slots, which is empty or holds other keys
int dcn_launch_dup_rehash(const dcn_dup_args &args, const unsigned long long *old_slots, uint64_t n_old, hipStream_t stream);

// ---- extended placements (extend.hip, extend_api.hip; the shared arithmetic is in dcn_extend.h) ----------------------
// One flank of one row as the kernel takes it: item 2 r is the left flank of row r, item 2 r + 1 its right flank.  The
// host has checked the row and resolved both sequences of the flank to stream positions, as dcn_verify_item has them.
struct dcn_extend_item {
    int64_t u_origin; // U in the batch stream: its first base, or the end of its bases when it is read backwards
    int64_t v_origin; // V in the store, likewise
    uint32_t f, g;    // |U|, |V|
    uint32_t cap;     // dcn_ext_cap: the last score of the wavefront
    uint32_t flags;   // bit 0: U is read backwards; bit 1: V is; bit 2: the row is unplaced (nothing else is read)
};
static_assert(sizeof(dcn_extend_item) == 32, "extend item");

// what the kernel leaves per flank: rule X5's (i*, j*, D*)
struct dcn_extend_result {
    uint32_t i, j, d, reserved;
};
static_assert(sizeof(dcn_extend_result) == 16, "extend result");

struct dcn_extend_args {
    const dcn_extend_item *items;
    uint64_t n_items;
    const uint32_t *s_packed, *s_invmask; // the batch: views behind DCN_FRONT_PAD
    const uint32_t *t_packed, *t_invmask; // the store
    uint32_t lds_stride;                  // words of one wavefront array: >= 2 * (the largest cap of the call) + 1
    uint32_t penalty, end_bonus;
    dcn_extend_result *out;
};
int dcn_launch_extend(const dcn_extend_args &args, hipStream_t stream);

// ---- insertion ledger (insertions.hip, insertions_api.hip; the shared arithmetic is in dcn_insertions.h) --------------
struct dcn_ins_event; // (dcn_insertions.h)
// The ledger of a map (dcn_anchor_map_pileup_keep_insertions): the events and their bases on the device, both arrays
// growing geometrically from DCN_INSERTION_LEDGER_EVENTS (read when the ledger first grows), and the scratch of the append
// inside dcn_pileup_batch, which lives with the ledger: per aligned row of a call its events and bases, their offsets and
// the scan's sums, and the two totals, which are zero between calls.
struct dcn_ins_ledger {
    dcn_ins_event *d_events = nullptr;
    uint8_t *d_bases = nullptr;
    uint64_t event_cap = 0, base_cap = 0, n_events = 0, n_bases = 0;
    uint32_t *d_row_events = nullptr, *d_row_bases = nullptr;
    uint64_t rows_cap = 0;
    uint64_t *d_event_offsets = nullptr, *d_base_offsets = nullptr;
    unsigned long long *d_event_sums = nullptr, *d_base_sums = nullptr;
    uint64_t offsets_cap = 0;
    unsigned long long *d_totals = nullptr; // events, bases
};
void dcn_ins_ledger_free(dcn_ins_ledger *l);

// the walk of pileup_kernel over the same work list (args.counters is not looked at)
struct dcn_ins_append_args {
    dcn_pileup_args rows;
    uint32_t *row_events, *row_bases; // per work item (the counting pass)
    unsigned long long *totals;       // ... and their sums over the call, added to
    const uint64_t *event_offsets, *base_offsets; // their scans (the writing pass)
    dcn_ins_event *events;                        // the ledger's arrays, from where this call appends
    uint8_t *bases;
    uint64_t event0, base0;
};
int dcn_launch_ins_count(const dcn_ins_append_args &args, hipStream_t stream);
int dcn_launch_ins_write(const dcn_ins_append_args &args, hipStream_t stream);
// the append of dcn_pileup_batch on a map that keeps a ledger, behind the pileup kernel on the context's stream
int dcn_insertions_append(dcn_ctx *c, dcn_index *map, const dcn_pileup_args &rows);

// fetch and call over the range [base0, base0 + n) of the store
struct dcn_ins_range_args {
    const uint32_t *counters; // the map's pileup
    uint64_t bases;
    const uint32_t *t_packed, *t_invmask;
    uint64_t base0, n, pos0;
    uint32_t min_depth, min_permille;
    uint32_t *counts, *flags;       // per position: the events that count (L2, L6), and whether it has a called insertion
    const uint64_t *bucket_offsets; // the scan of counts
    uint32_t *cursor;               // per position, zero before the scatter
    uint64_t *slots;                // per bucket entry: the event of the ledger
    const dcn_ins_event *events;
    const uint8_t *ledger_bases;
    uint64_t n_events;
    // fetch
    uint64_t n_slots;
    uint32_t *slot_lens;
    const uint64_t *slot_offsets; // their scan
    void *out_events;             // dcn_insertion per slot
    uint8_t *out_bases;
    // call
    const uint64_t *allele_offsets; // the scan of flags
    uint64_t n_alleles;
    uint64_t *win_event;
    uint32_t *win_count, *win_events, *win_len;
    uint64_t *win_pos;
    const uint64_t *win_offsets; // the scan of win_len
    void *out_alleles;           // dcn_insertion_allele per allele
};
int dcn_launch_ins_plane(const dcn_ins_range_args &args, bool call, hipStream_t stream);
int dcn_launch_ins_scatter(const dcn_ins_range_args &args, hipStream_t stream);
int dcn_launch_ins_slot_lens(const dcn_ins_range_args &args, hipStream_t stream);
int dcn_launch_ins_gather(const dcn_ins_range_args &args, hipStream_t stream);
int dcn_launch_ins_winner(const dcn_ins_range_args &args, hipStream_t stream);
int dcn_launch_ins_alleles(const dcn_ins_range_args &args, hipStream_t stream);

// ---- deletion ledger and indel genotypes (indels.hip, indels_api.hip; the shared arithmetic is in dcn_indels.h) ----------
struct dcn_del_event; // (dcn_indels.h)
// The deletion ledger of a map (dcn_anchor_map_pileup_keep_deletions): the events on the device, growing geometrically from
// DCN_DELETION_LEDGER_EVENTS (read when the ledger first grows), and the scratch of the append, which lives with the ledger:
// per aligned row of a call its events, their offsets and the scan's sums, and the total, which is zero between calls.
struct dcn_del_ledger {
    dcn_del_event *d_events = nullptr;
    uint64_t event_cap = 0, n_events = 0, n_deleted = 0;
    uint32_t *d_row_events = nullptr;
    uint64_t rows_cap = 0;
    uint64_t *d_event_offsets = nullptr;
    unsigned long long *d_event_sums = nullptr;
    uint64_t offsets_cap = 0;
    unsigned long long *d_totals = nullptr; // events, their lengths
};
void dcn_del_ledger_free(dcn_del_ledger *l);

// the walk of pileup_kernel over the same work list (args.counters is not looked at)
struct dcn_del_append_args {
    dcn_pileup_args rows;
    uint32_t *row_events;          // per work item (the counting pass)
    unsigned long long *totals;    // the events of the call and the sum of their lengths, added to
    const uint64_t *event_offsets; // the scan of row_events (the writing pass)
    dcn_del_event *events;         // the ledger's array, from where this call appends
    uint64_t event0;
};
int dcn_launch_del_count(const dcn_del_append_args &args, hipStream_t stream);
int dcn_launch_del_write(const dcn_del_append_args &args, hipStream_t stream);
// the append of dcn_pileup_batch on a map that keeps a deletion ledger, behind the pileup kernel on the context's stream
int dcn_deletions_append(dcn_ctx *c, dcn_index *map, const dcn_pileup_args &rows);

// fetch and the deletion side of a genotype call over the range [base0, base0 + n) of the store
struct dcn_del_range_args {
    uint64_t base0, n, pos0;
    const dcn_del_event *events;
    uint64_t n_events;
    uint32_t *counts;               // per position: STARTS (rule R5), zero before the plane kernel
    const uint64_t *bucket_offsets; // the scan of counts
    uint32_t *cursor;               // per position, zero before the scatter
    uint64_t *slots;                // per bucket entry: the event of the ledger
    uint64_t n_slots;
    void *out_events;               // fetch: dcn_deletion per slot
    uint32_t *win_count, *win_len;  // genotype: per position the winner's count and length (0 where STARTS is 0)
};
int dcn_launch_del_plane(const dcn_del_range_args &args, hipStream_t stream);
int dcn_launch_del_scatter(const dcn_del_range_args &args, hipStream_t stream);
int dcn_launch_del_gather(const dcn_del_range_args &args, hipStream_t stream);
int dcn_launch_del_winner(const dcn_del_range_args &args, hipStream_t stream);

// rules I1 - I6 over the range: count, scan, write (genotype.hip's shape), then the inserted bases of the insertion sites
struct dcn_indel_site_args {
    const uint32_t *counters; // the map's pileup
    uint64_t bases;
    uint64_t base0, n, pos0;
    uint32_t ploidy, min_depth, min_gq, min_qual, min_count, indel_centi, het_centi;
    // the insertion candidates (null: the map keeps no insertion ledger, or the range has no event): per position whether
    // INS > 0, its scan, and per flagged position ins_winner_kernel's arrays
    const uint32_t *ins_flags;
    const uint64_t *ins_offsets;
    const uint64_t *ins_event;
    const uint32_t *ins_count, *ins_events, *ins_len;
    const dcn_ins_event *ins_ledger;
    const uint8_t *ins_ledger_bases;
    // the deletion candidates (null likewise): per position STARTS, the winner's count and its length
    const uint32_t *del_starts, *del_count, *del_len;
    uint32_t *block_counts;         // sites per workgroup (the counting pass)
    unsigned long long *n_inserted; // the inserted bases of all sites, added to (the counting pass)
    const uint64_t *block_offsets;  // the scan of block_counts (the writing pass)
    void *sites;                    // dcn_indel_site per site; bases_offset is written by the bases pass
    uint32_t *site_lens;            // per site: the inserted bases (0 for a deletion)
    uint64_t *site_event;           // per site: the winning event of an insertion
    uint64_t n_sites;
    const uint64_t *site_offsets;   // the scan of site_lens
    uint8_t *out_bases;
};
uint32_t dcn_indel_site_blocks(uint64_t n); // workgroups of a range of n positions
int dcn_launch_indel_flags(const uint32_t *counts, uint32_t *flags, uint64_t n, hipStream_t stream);
int dcn_launch_indel_sites(const dcn_indel_site_args &args, bool write, hipStream_t stream);
int dcn_launch_indel_bases(const dcn_indel_site_args &args, hipStream_t stream);

// ---- strand evidence (strand.hip, strand_api.hip; the shared arithmetic is in dcn_strand.h) ---------------------------
// one checked query as the kernel takes it: the store base of its position behind the fields of a dcn_strand_query
struct dcn_strand_query_item {
    uint64_t base;
    uint32_t kind, ref_code, alt_mask, count, count_reverse, reserved;
};
static_assert(sizeof(dcn_strand_query_item) == 32, "strand query item");
struct dcn_strand_site_item { // a dcn_strand_site
    uint32_t fwd[4], rev[4], table[4], sb_centi, flags, reserved[2];
};
static_assert(sizeof(dcn_strand_site_item) == 64, "strand site item");
struct dcn_strand_evidence_args {
    const uint32_t *counters, *strands; // the map's pileup and its strand planes
    uint64_t bases;
    const dcn_strand_query_item *queries;
    uint64_t n;
    uint32_t max_sb_centi, min_alt_strand, min_strand_depth;
    dcn_strand_site_item *out;
};
int dcn_launch_strand_evidence(const dcn_strand_evidence_args &args, hipStream_t stream);

// The key of an indel site and of a ledger event: the store base of its position, then I6's order at one position (0 a
// front insertion, 1 the deletion, 2 an insertion behind).  Ascending keys are I6's order.
__host__ __device__ inline uint64_t dcn_indel_strand_key(uint64_t base, uint32_t order) { return base * 4u + order; }
struct dcn_indel_strand_args {
    const uint64_t *site_keys;         // ascending, n_sites of them
    const uint32_t *site_len;          // the allele's length
    const uint64_t *site_bases_offset; // an insertion site's bases in site_bases
    const uint8_t *site_bases;
    uint64_t n_sites;
    const dcn_ins_event *ins_events;   // the ledgers; n_*_events = 0: no site of that kind
    const uint8_t *ins_ledger_bases;
    uint64_t n_ins_events;
    const dcn_del_event *del_events;
    uint64_t n_del_events;
    uint32_t *count_reverse;           // per site, zero before
};
int dcn_launch_indel_strand(const dcn_indel_strand_args &args, hipStream_t stream);

// ---- reference blocks (blocks.hip, blocks_api.hip; the shared rule is in dcn_blocks.h) --------------------------------
struct dcn_blocks_args {
    const uint32_t *counters, *sums; // the map's pileup and its quality sums
    uint64_t bases;
    const uint32_t *t_packed, *t_invmask; // the store
    uint64_t base0, n;                    // the range: store bases [base0, base0 + n)
    uint64_t pos0;                        // ... and the record position of its first base
    uint32_t ploidy, min_depth, min_gq, min_qual, err_centi, het_centi;
    uint64_t edges_lo, edges_hi; // dcn_blk_edges
    // per position of the range, each behind a pad of dcn_blocks_pad(base0) bytes, dcn_blocks_out_bytes each; the bytes of
    // the pad and behind the range are DCN_BLK_VARIANT in cls
    uint8_t *cls, *gq;
    const uint64_t *breaks; // positions of the range, relative to its first
    uint64_t n_breaks;
    uint32_t *block_counts;        // heads per workgroup (the counting pass)
    const uint64_t *block_offsets; // their scan (the reducing pass)
    void *blocks;                  // dcn_reference_block per head, filled by dcn_launch_blocks_fill before the reducing pass
    uint64_t n_blocks;
};
uint32_t dcn_blocks_groups(uint64_t base0, uint64_t n);    // workgroups of a range
uint64_t dcn_blocks_pad(uint64_t base0);                   // bytes in front of the range's first in args.cls and args.gq
uint64_t dcn_blocks_out_bytes(uint64_t base0, uint64_t n); // bytes of args.cls and of args.gq
int dcn_launch_blocks_classify(const dcn_blocks_args &args, hipStream_t stream);
int dcn_launch_blocks_breaks(const dcn_blocks_args &args, hipStream_t stream);
int dcn_launch_blocks_heads(const dcn_blocks_args &args, bool reduce, hipStream_t stream);
int dcn_launch_blocks_fill(const dcn_blocks_args &args, hipStream_t stream);
