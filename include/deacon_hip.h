/*
 * deacon_hip.h -- C ABI of the MI355X-native read-filtering core for Deacon.
 *
 * This is the drop-in boundary for ONE path of the reference (crate deacon 0.10.0): the per-read
 * "pack -> canonical minimizer scan -> k-mer hash -> index probe -> distinct-hit count -> threshold"
 * loop that `deacon filter` runs on CPU worker threads.  The reference has no FFI of its own; each
 * entry point below names the Rust item (file:line under the reference's src/) it replaces.  A Rust
 * maintainer binds them with a plain `extern "C"` block.
 *
 * Conventions
 *   - every function returns DCN_OK (0) or a negative DCN_ERR_* code and never aborts;
 *     dcn_last_error() returns a thread-local message for the last failure on this thread;
 *   - plain pointers and sizes only; "host" pointers are ordinary process memory, "device" pointers are
 *     HIP device allocations on the context's GPU;
 *   - a dcn_index is immutable after creation and may be shared by any number of contexts/threads
 *     (the reference shares its set through an Arc: src/local_filter.rs:156,631);
 *   - a dcn_ctx owns one HIP stream pair plus staging/scratch buffers and is NOT thread-safe: use one
 *     per host thread (the reference clones one FilterProcessor per worker: src/local_filter.rs:153).
 */
#ifndef DEACON_HIP_H
#define DEACON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCN_OK 0
#define DCN_ERR_ARG (-1)      /* invalid argument (NULL, k/w out of range, k+w-1 even, ...) */
#define DCN_ERR_HIP (-2)      /* a HIP runtime call failed (message has the HIP error string) */
#define DCN_ERR_NOMEM (-3)    /* host or device allocation failed */
#define DCN_ERR_IO (-4)       /* index file could not be opened / read */
#define DCN_ERR_FORMAT (-5)   /* index file is not a format-version-2 deacon index */
#define DCN_ERR_CAPACITY (-6) /* batch larger than the context was created for, or output too small */
#define DCN_ERR_INTERNAL (-7)

typedef struct dcn_index dcn_index; /* device-resident minimizer set: replaces Arc<FxHashSet<u64>> */
typedef struct dcn_ctx dcn_ctx;     /* per-thread pipeline context */

/* Filter-time parameters: the fields of FilterProcessor that the decision depends on
 * (src/local_filter.rs:159-162; CLI defaults -a 2 -r 0.01 -p 0, src/main.rs:43-60).
 * k and w are NOT here: like the reference they come from the index header
 * (src/local_filter.rs:633-634). */
typedef struct dcn_params {
    uint64_t abs_threshold; /* -a: minimum absolute number of distinct minimizer hits */
    double rel_threshold;   /* -r: minimum hits relative to the unit's minimizer count */
    uint64_t prefix_length; /* -p: 0 = whole read, else only the first prefix_length bases */
    uint32_t deplete;       /* -d: 0 = keep matching units, 1 = keep non-matching units */
    uint32_t reserved;      /* must be 0 */
} dcn_params;

/* The six ProcessingStats counters of src/local_filter.rs:179-187, in that order. */
enum {
    DCN_STAT_TOTAL_SEQS = 0,
    DCN_STAT_FILTERED_SEQS = 1,
    DCN_STAT_TOTAL_BP = 2,
    DCN_STAT_OUTPUT_BP = 3,
    DCN_STAT_FILTERED_BP = 4,
    DCN_STAT_OUTPUT_SEQ_COUNTER = 5,
    DCN_N_STATS = 6
};

/* ---- library ------------------------------------------------------------------------------------ */
/* ABI version of this header.  MAJOR changes whenever the signature of an exported function or the layout of a struct
 * changes (a binding built against another major must refuse to run: its calls would pass the wrong arguments), MINOR
 * when entry points are added.  History: 0.x = the headers before versioning (dcn_pack_ascii took four arguments there);
 * 1.0 = dcn_pack_ascii(bases, n_bases, packed, invmask, saw_newline); 1.1 = dcn_abi_version, dcn_comm_* / dcn_stats_allreduce_rccl;
 * 1.2 = dcn_index_set_* / dcn_classify_batch*; 1.3 = dcn_index_set_coverage*; 1.4 = dcn_locate_batch;
 * 1.5 = dcn_index_set_select / _overlap, dcn_index_intersect;
 * 1.6 = dcn_index_set_depth_enable / _reset / _stats / _hist / _keys;
 * 1.7 = dcn_index_builder_create / _add / _info / _hist / _counts / _finish / _destroy;
 * 1.8 = dcn_depth_track_batch;
 * 1.9 = dcn_anchor_map_create / _add / _info / _anchors, dcn_place_batch.
 * 1.10 = dcn_place_split_batch.
 * 1.11 = dcn_place_pair_batch.
 * 1.12 = dcn_ctx_last_batch_short.
 * 1.13 = dcn_anchor_map_keep_bases / _fetch, dcn_verify_batch.
 * 1.14 = dcn_align_batch.
 * 1.15 = dcn_anchor_map_pileup_* / dcn_pileup_batch.
 * 1.16 = dcn_extend_batch.
 * 1.17 = dcn_anchor_map_pileup_keep_insertions, dcn_anchor_map_insertions_info / _fetch / _call.
 * 1.18 = dcn_anchor_map_pileup_keep_qualities / _fetch_qualities, dcn_pileup_batch_qual.
 * 1.19 = dcn_anchor_map_genotype.
 * 1.20 = dcn_anchor_map_duplicates_enable / _reset / _info, dcn_mark_duplicates_batch.
 * 1.21 = dcn_anchor_map_pileup_keep_deletions, dcn_anchor_map_deletions_info / _fetch, dcn_anchor_map_indels_genotype.
 * 1.22 = dcn_left_align_batch, dcn_anchor_map_pileup_left_align / _left_align_info.
 * 1.23 = dcn_anchor_map_pileup_keep_strands / _fetch_strands, dcn_anchor_map_strand_evidence, dcn_anchor_map_indels_strand.
 * 1.24 = dcn_anchor_map_reference_blocks, dcn_reference_blocks_merge: declared in deacon_hip_blocks.h, not here.
 * 1.25 = dcn_anchor_map_phase_sites / _info / _links / _solve, dcn_phase_batch: declared in deacon_hip_phase.h, not here. */
#define DCN_ABI_MAJOR 1
#define DCN_ABI_MINOR 25
/* What the loaded library was built as: a binding asserts *major == DCN_ABI_MAJOR it was written against and
 * *minor >= the minor it needs, before its first other call (no reference counterpart: the reference is one crate). */
int dcn_abi_version(uint32_t *major, uint32_t *minor);
const char *dcn_version(void);
const char *dcn_last_error(void);
int dcn_device_count(int *count);

/* ---- parity-pinning switch ------------------------------------------------------------------------------
 * The minimizer rule itself lives in a crate the reference only calls: simd_minimizers::canonical_minimizer_positions
 * (src/filter_common.rs:261-267, src/minimizers.rs:143-148; simd-minimizers 1.3.0 in Cargo.lock:1954-1957).  Three
 * of its details could not be executed where this library was written ("Notes on A4"): the ntHash
 * rotation per base (1, or 7 as in the crate's later line), how many hash bits the window minimum compares (the top
 * 16, or all 32) and how the two strands' hashes are combined (wrapping add, or xor).  The defaults are (1, 16, 0).
 * The setting is process-wide and is CAPTURED by every index when it is created (built, loaded, merged, cloned): the
 * rule an index's keys were selected by travels with it, every context filters by its index's rule whatever the
 * setting has become since, and union / diff refuse operands created under different rules.  Set it before the first
 * index is built or loaded.  Any other setting than the default runs a generic kernel (slower, counting mode only); tests/golden/
 * dump_crate_vectors prints vectors from the real crates, and tests/test_crate_vectors.py names the setting that
 * reproduces them. */
int dcn_set_minimizer_variant(uint32_t nt_rot, uint32_t cmp_bits, uint32_t combine /* 0: fw + rc, 1: fw ^ rc */);
int dcn_get_minimizer_variant(uint32_t *nt_rot, uint32_t *cmp_bits, uint32_t *combine);

/* ---- index: replaces index::load_minimizer_hashes (src/index.rs:80-107) ----------------------------- */

/* Build the device set from `n` host u64 minimizer hashes (duplicates allowed; they are merged, as by
 * FxHashSet::insert at src/index.rs:104).  k, w as in IndexHeader (src/index.rs:17-31): 1<=k<=56
 * (the filter path asserts k<=56 at src/filter_common.rs:269), w>=1, k+w-1 odd (src/index.rs:186-194). */
int dcn_index_from_keys(const uint64_t *keys, uint64_t n, uint8_t k, uint8_t w, int device, dcn_index **out);

/* Load a deacon index file (bincode 2 "standard" varint layout written by write_minimizers,
 * src/index.rs:130-164; header validation as IndexHeader::validate, src/index.rs:34-43). */
int dcn_index_from_file(const char *path, int device, dcn_index **out);

/* Build the index from sequences held in host memory: index::build (src/index.rs:167-308) minus FASTX parsing.
 * Every sequence goes through the index-side rule (minimizers::fill_minimizer_hashes, src/minimizers.rs:125-191:
 * IUPAC codes canonicalised to ACGT before the scan, minimizers whose k-mer has a non-ACGT base in the ORIGINAL
 * bytes dropped, optional scaled-entropy floor) and the hashes are merged into one device set.
 *   bases / offsets   concatenated sequences and n_seqs+1 byte offsets, as for dcn_filter_batch
 *   entropy_threshold 0 = off (the reference's default, src/lib.rs:224)
 *   capacity_keys     pre-allocation hint (IndexConfig::capacity_millions, src/lib.rs:200); 0 = grow as needed */
int dcn_index_build(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seqs, uint8_t k, uint8_t w,
                    float entropy_threshold, uint64_t capacity_keys, int device, dcn_index **out);

/* Copy the distinct keys to host memory in arbitrary order (the reference iterates its FxHashSet, src/index.rs:159);
 * *n receives the key count; DCN_ERR_CAPACITY if capacity is smaller. */
int dcn_index_keys(const dcn_index *index, uint64_t *out, uint64_t capacity, uint64_t *n);

/* Write the index in the reference's file format: write_minimizers (src/index.rs:130-164). */
int dcn_index_write_file(const dcn_index *index, const char *path);

/* Set union of n >= 1 indexes on the same device: index::union (src/index.rs:563-664).  All inputs must have the
 * same k and w (the reference refuses otherwise, :611-626). */
int dcn_index_union(const dcn_index *const *inputs, uint32_t n, dcn_index **out);

/* Set difference first \ second: index::diff (src/index.rs:421-536); k and w must match (:478-490). */
int dcn_index_diff(const dcn_index *first, const dcn_index *second, dcn_index **out);

/* Set intersection of n >= 1 indexes on the same device: the keys present in EVERY input (no reference counterpart: the
 * reference composes indexes with union and diff only, and A n B took two diffs and two intermediate indexes).  The
 * refusals on k, w, minimizer rule and device are dcn_index_union's; a labelled set counts as the union of its members.
 * Any n works: the smallest input is swept once and its keys probed in the others.  The result's table is sized for its
 * own key count, not for the inputs'; an empty intersection is a valid index with 0 keys. */
int dcn_index_intersect(const dcn_index *const *inputs, uint32_t n, dcn_index **out);

/* Header fields and the number of DISTINCT keys (what `deacon index info` prints, src/index.rs:539-560). */
int dcn_index_header(const dcn_index *index, uint8_t *k, uint8_t *w, uint64_t *n_keys);

/* The HIP device the index lives on. */
int dcn_index_device(const dcn_index *index, int *device);

/* Bytes of device memory the index's hash table occupies (a power-of-two number of 16-byte groups with at least
 * four slots per key, eight while that stays within 34 GB and a third of the device's free memory:
 * DESIGN.md section 3; the reference's FxHashSet<u64> is ~9-18 bytes per key of host memory). */
int dcn_index_memory(const dcn_index *index, uint64_t *table_bytes);

/* Set membership for `n` host keys -> out[i] in {0,1}: FxHashSet::contains (src/filter_common.rs:144). */
int dcn_index_contains(const dcn_index *index, const uint64_t *keys, uint64_t n, uint8_t *out);

/* Same for keys already in device memory (d_keys, d_out are DEVICE pointers on the index's GPU); enqueued on
 * `stream` (a hipStream_t, NULL = default stream) without waiting. */
int dcn_index_contains_device(const dcn_index *index, const uint64_t *d_keys, uint64_t n, uint8_t *d_out,
                              void *stream);

/* Measurement: the rate (home-group reads per second) at which this table serves a stream of keys when nothing else
 * runs -- every key's home group is read (one 16-byte request), nothing is resolved or written; the best of several
 * launch shapes over `reps` repetitions.  d_keys (DEVICE pointer) is the stream to replay, e.g. a batch's minimizer
 * hashes; NULL probes n uniformly random groups instead (every request an L2 miss).  This is the ceiling the probe
 * stage of the filter kernel is measured against (bench.py: roofline.probe_ceiling_*; the counterpart of timing
 * FxHashSet::contains alone, src/filter_common.rs:144).  Blocks until done. */
int dcn_index_probe_ceiling(const dcn_index *index, const uint64_t *d_keys, uint64_t n, uint32_t reps,
                            double *probes_per_s);

/* Replica of an index on another (or the same) device, made device to device: the reference shares ONE set between its
 * workers through an Arc (src/local_filter.rs:630-631); a multi-GPU host loads or builds the index once and clones it to
 * every other device instead of repeating the host-to-device copy.  To another device the compacted KEYS cross xGMI
 * (hipMemcpyPeer of 8 bytes per key, a tenth of the sparse table) and are inserted into an empty table there; on the same
 * device the table itself is copied.  Same key set, k, w and minimizer rule either way. */
int dcn_index_clone(const dcn_index *index, int device, dcn_index **out);

void dcn_index_destroy(dcn_index *index);

/* ---- context -------------------------------------------------------------------------------------- */

/* max_batch_bases / max_batch_reads bound one call of dcn_filter_batch*; buffers are sized once here. */
int dcn_ctx_create(const dcn_index *index, uint64_t max_batch_bases, uint32_t max_batch_reads, dcn_ctx **out);
void dcn_ctx_destroy(dcn_ctx *ctx);

/* ---- the hot path -------------------------------------------------------------------------------- */

/* Filter one batch of reads held in host memory.  Replaces, for every unit of the batch,
 * FilterProcessor::should_keep_sequence (src/local_filter.rs:221-252) or ::should_keep_pair (:254-285),
 * i.e. get_minimizer_hashes_and_positions (src/filter_common.rs:211-310) + sequence_matches /
 * pair_matches (:129-198) + meets_filtering_criteria (:99-112).
 *
 *   bases    concatenated ASCII sequences (record.seq() bytes, no separators), offsets[n_reads] bytes
 *   offsets  n_reads+1 byte offsets into `bases`, offsets[0] == 0, non-decreasing
 *   unit_id  NULL: every read is its own unit.  Otherwise n_reads entries, unit_id[0]==0, each
 *            entry equal to its predecessor or predecessor+1: consecutive reads with equal id form
 *            one unit (a pair: mate 1 then mate 2 -- src/filter_common.rs:312-348)
 *   keep     out, one byte per unit: 1 = write the unit's records to the output, 0 = drop
 *   hits     out (may be NULL), distinct minimizer hits per unit
 *   total    out (may be NULL), minimizer count per unit (duplicates included) -- the
 *            (bool, usize, usize) of should_keep_*
 * With hits == NULL and total == NULL only the decisions are produced, which is all `deacon filter` consumes
 * outside --debug (src/local_filter.rs:350-371): the kernels may then stop probing a unit as soon as its
 * decision is fixed (abs_threshold distinct hits reached while the relative threshold cannot ask for more).
 * keep and the six counters are identical in both forms.
 *
 * Blocking (= dcn_filter_batch_submit + dcn_filter_batch_wait).  Inside, the batch is cut at unit boundaries into
 * chunks of ~64 Mbp (DCN_CHUNK_BASES): chunk i's kernels run while chunk i+1 crosses PCIe on a side stream and chunk i-1's results
 * travel back on a third.  What crosses the link:
 *   pageable memory   host threads pack it to 2 bits + 1 mask bit per base straight into the context's pinned
 *                     staging ring (0.375 instead of 1 byte per base on the link -- the reference packs on the host
 *                     too: src/filter_common.rs:238-258);
 *   page-locked memory (dcn_host_alloc / hipHostRegister)  the same where the host packs fast enough to beat the
 *                     link's 1 byte per base (AVX-512BW hosts), else -- and always with DCN_PINNED_ASCII_DMA=1 -- the
 *                     ASCII is DMA'd as it is and packed on the device (no host work at all).
 * A batch that needed more hit-record scratch than the context has is re-run after growing it: callers never see
 * DCN_ERR_CAPACITY for that. */
int dcn_filter_batch(dcn_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, const uint32_t *unit_id,
                     uint32_t n_reads, const dcn_params *params, uint8_t *keep, uint32_t *hits,
                     uint32_t *total);

/* Asynchronous form: the paraseq workers of the reference overlap reading, filtering and writing across threads
 * (src/local_filter.rs:696-709); here ONE caller thread keeps up to two batches in flight per context.
 * submit validates the batch, enqueues its copies and kernels and returns a ticket; wait(ticket) blocks until the
 * batch is done, delivers keep/hits/total and adds the batch's six counters to the context's.  All input and
 * output arrays must stay valid and unmodified until wait returns, and the CONTENTS of keep/hits/total are undefined
 * until then: results of early chunks are copied out while later chunks are still being prepared, and a batch that
 * has to be run again (a newline found while packing, a run of the record array that overflowed) overwrites them.
 * A third submit without a wait fails with DCN_ERR_CAPACITY.  Tickets may be waited for in any order. */
int dcn_filter_batch_submit(dcn_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, const uint32_t *unit_id,
                            uint32_t n_reads, const dcn_params *params, uint8_t *keep, uint32_t *hits,
                            uint32_t *total, uint64_t *ticket);
int dcn_filter_batch_wait(dcn_ctx *ctx, uint64_t ticket);

/* The same batch handed over already packed, as the reference holds it after PackedSeqVec::from_ascii and its mask
 * loop (src/filter_common.rs:238-258) -- for the concatenated batch instead of one read at a time:
 *   packed   2 bits per base, code (c >> 1) & 3 of the ASCII byte (A=0 C=1 T=2 G=3, non-ACGT mapped the same
 *            lossy way); base i of the batch = bits [2(i%16), +2) of packed[i/16], i.e. bits 2(i%4) of byte i/4:
 *            packed-seq's own byte order
 *   invmask  1 bit per base, bit i%32 of invmask[i/32] set iff byte i is not one of ACGTacgt
 *   offsets / unit_id / outputs as for dcn_filter_batch (offsets are BASE indices into the stream)
 * Both arrays must be allocated in whole 32-base groups: 2 * ceil(n_bases/32) and ceil(n_bases/32) words
 * (dcn_pack_ascii fills them).  Reads must not end in a newline byte, 0x0A (src/filter_common.rs:229 strips one from
 * the ASCII; a packed stream cannot show it: dcn_pack_ascii reports whether it met one).  The pack kernel is skipped;
 * 0.25 bytes per base cross the link, plus the non-zero words of invmask (the rest of it is a memset on the device). */
int dcn_filter_batch_packed(dcn_ctx *ctx, const uint32_t *packed, const uint32_t *invmask, const uint64_t *offsets,
                            const uint32_t *unit_id, uint32_t n_reads, const dcn_params *params, uint8_t *keep,
                            uint32_t *hits, uint32_t *total);
int dcn_filter_batch_packed_submit(dcn_ctx *ctx, const uint32_t *packed, const uint32_t *invmask,
                                   const uint64_t *offsets, const uint32_t *unit_id, uint32_t n_reads,
                                   const dcn_params *params, uint8_t *keep, uint32_t *hits, uint32_t *total,
                                   uint64_t *ticket);

/* Host-side packer producing exactly that layout from concatenated ASCII (AVX2 + BMI2 where the CPU has them,
 * split over the library's host threads, DCN_HOST_THREADS).  Input formatting only: nothing here hashes or
 * decides.  packed / invmask: 2 * ceil(n_bases/32) and ceil(n_bases/32) u32 words.  saw_newline (may be NULL)
 * receives 1 if some byte of the input was 0x0A, else 0: a read that ENDS in one is shortened by the ASCII entry
 * points (src/filter_common.rs:229) and cannot be by the packed ones, so a caller whose record buffers may carry
 * line ends must strip them, or send that batch through dcn_filter_batch, when the flag comes back set. */
int dcn_pack_ascii(const uint8_t *bases, uint64_t n_bases, uint32_t *packed, uint32_t *invmask, uint32_t *saw_newline);

/* Same computation on inputs already resident in device memory (all pointers are DEVICE pointers on the
 * context's GPU; d_unit_id / d_hits / d_total may be NULL).  n_bases = offsets[n_reads], n_units = number
 * of units (n_reads when d_unit_id is NULL).  Enqueues on the context's stream and returns without
 * waiting; call dcn_ctx_synchronize() before reading the outputs.  The arrays are read WHEN THE KERNELS RUN, on the
 * context's stream: a producer on another stream must be ordered before it (event or synchronize).  Nothing on the
 * host has seen d_offsets / d_unit_id, so the planning kernel checks them: a read with offsets[r] > offsets[r+1] or
 * offsets[r+1] > n_bases is planned as empty, unit ids that are not 0, then equal or +1, ending at n_units - 1 are
 * flagged, and the next dcn_ctx_synchronize() returns DCN_ERR_ARG (never tiles or read ranges that point outside
 * the batch's buffers). */
int dcn_filter_batch_device(dcn_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offsets,
                            const uint32_t *d_unit_id, uint32_t n_reads, uint64_t n_bases, uint32_t n_units,
                            const dcn_params *params, uint8_t *d_keep, uint32_t *d_hits, uint32_t *d_total);

/* Wait for everything enqueued on the context by dcn_filter_batch_device; reports deferred errors of the device
 * pipeline.  DCN_ERR_CAPACITY: the hit-record scratch overflowed in SOME batch enqueued since the previous
 * synchronize (the flag is sticky across batches); results and counters of all of them are then unspecified:
 * dcn_ctx_reserve_records(), dcn_ctx_reset_stats() and enqueue them again.  DCN_ERR_ARG: the device found the
 * d_offsets / d_unit_id of some batch since the previous synchronize inconsistent (see above); outputs and counters
 * of those batches are undefined, the context itself stays usable (reported once). */
int dcn_ctx_synchronize(dcn_ctx *ctx);

/* Which path the last batch that dcn_ctx_synchronize() waited for took (ABI 1.12): *was_short = 1 when the device found it
 * to be a batch of short unpaired reads (device-resident ASCII, no unit ids, no prefix, every read at most 152 bases) and
 * packed its bases inside the scan kernel instead of in a pack pass of its own, 0 for the classic path.  The results are
 * the same either way; DCN_NO_SHORT_FUSED=1 in the environment when the context is created keeps every batch on the
 * classic path.  Only batches of dcn_filter_batch_device are reported: the host entry points wait for their batches
 * themselves and leave the answer as it was. */
int dcn_ctx_last_batch_short(dcn_ctx *ctx, uint32_t *was_short);

/* Grow the scratch that holds (unit, hash) hit records of units spanning several tiles (long reads). */
int dcn_ctx_reserve_records(dcn_ctx *ctx, uint64_t n_records);

/* Raw HIP stream (hipStream_t) the context enqueues on, so a caller can time or order against it. */
void *dcn_ctx_stream(dcn_ctx *ctx);

/* Page-locked host memory for batch buffers.  dcn_filter_batch copies from such memory (or any memory the
 * caller registered with hipHostRegister) straight over PCIe; pageable memory goes through the context's
 * pinned staging buffers first.  Stands for nothing in the reference (its batches never leave the host). */
int dcn_host_alloc(uint64_t bytes, void **out);
void dcn_host_free(void *p);

/* Minimizer hashes and positions of every read of a host batch: the (Vec<u64>, Vec<u32>) of
 * get_minimizer_hashes_and_positions (src/filter_common.rs:211-310), concatenated read by read.
 *   out_offsets  n_reads+1 entries: read r owns [out_offsets[r], out_offsets[r+1]) of the two arrays
 *   capacity     entries available in out_hashes / out_positions; on DCN_ERR_CAPACITY
 *                out_offsets[n_reads] holds the required size */
int dcn_minimizer_hashes_batch(dcn_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                               uint64_t prefix_length, uint64_t *out_offsets, uint64_t *out_hashes,
                               uint32_t *out_positions, uint64_t capacity);

/* Batch seam of the server engine: unpaired_should_keep / paired_should_keep
 * (src/remote_filter.rs:230-301) -- minimizer hashes precomputed by the client, unit u owns
 * hashes[hash_offsets[u] .. hash_offsets[u+1]) (for a pair: both mates' hashes concatenated).
 * Host pointers; hits/total may be NULL.  prefix_length of params is ignored here. */
int dcn_should_keep_hashes(dcn_ctx *ctx, const uint64_t *hashes, const uint64_t *hash_offsets, uint32_t n_units,
                           const dcn_params *params, uint8_t *keep, uint32_t *hits, uint32_t *total);

/* ---- classification against several indexes in one pass ------------------------------------------------
 * (no reference counterpart: the reference filters against one index, and index::union drops which input a key came
 * from.)  A labelled index set is ONE device table over the union of 1..32 member indexes -- same k, w, minimizer rule
 * and device, else DCN_ERR_ARG as for dcn_index_union -- in which every key carries a u32 mask: bit j = the key is in
 * members[j].  A probe reads the key's home group exactly as the filter does; only a hit reads the 4-byte mask.  The set
 * is built on the device from the members' tables (no key crosses to the host), sized for the sum of their keys, and owns
 * its memory: the members may be destroyed afterwards.
 * A set is a dcn_index: every dcn_index_* call that reads an index (keys, header, memory, contains, write_file, union,
 * clone, a context) sees the union of its members.  dcn_index_set_destroy and dcn_index_destroy are the same call. */
int dcn_index_set_create(const dcn_index *const *members, uint32_t n, dcn_index **out);
void dcn_index_set_destroy(dcn_index *set);
/* member count, k, w, distinct keys of the union, device bytes of slots + masks; DCN_ERR_ARG for an index that is not a set */
int dcn_index_set_info(const dcn_index *set, uint32_t *n_members, uint8_t *k, uint8_t *w, uint64_t *n_keys,
                       uint64_t *table_bytes);

/* ---- set algebra on a labelled set: its member masks answer every membership question about its keys ------------
 * (no reference counterpart.)  Both calls are blocking sweeps over the set's masks on its device, leave the set -- its
 * coverage marks included -- as it is, and return DCN_ERR_ARG for an index that is not a set.  Key 0 takes part.
 *
 * Keys of a labelled set chosen by their member mask L (c = popcount(L)):
 *   (L & all_of) == all_of  &&  (any_of == 0 || (L & any_of) != 0)  &&  (L & none_of) == 0
 *   && min_members <= c <= max_members
 * -> a new PLAIN index (k, w, minimizer rule and device of the set; neither masks nor coverage), sized for exactly the
 * selected keys.  max_members == 0: no upper bound; min_members == 0 behaves as 1 (every key of a set is in at least one
 * member).  *n_selected (may be NULL) receives the count.  out == NULL: count only, nothing is allocated.
 * DCN_ERR_ARG: a mask with a bit at or above the set's member count, min_members > max_members != 0, out and n_selected
 * both NULL.  A well-formed predicate that nothing satisfies (all_of & none_of != 0, say) is no error: the result is a
 * valid index with 0 keys.  Recipes: the keys only member j holds = all_of 1 << j, max_members 1; the core held by at
 * least m members = min_members m. */
int dcn_index_set_select(const dcn_index *set, uint32_t all_of, uint32_t any_of, uint32_t none_of, uint32_t min_members,
                         uint32_t max_members, uint64_t *n_selected, dcn_index **out);
/* How much the members share.  n = the set's member count; any output may be NULL, but not all three.
 *   shared[i*n + j]  keys whose mask has bits i and j (symmetric; shared[j*n + j] = keys of member j in the set)
 *   exclusive[j]     keys whose mask is exactly 1 << j
 *   by_count[c-1]    keys held by exactly c members, c = 1..n (sums to the set's key count) */
int dcn_index_set_overlap(const dcn_index *set, uint64_t *shared, uint64_t *exclusive, uint64_t *by_count);

/* Classify one batch against every member of `set` at once.  Inputs as for dcn_filter_batch (a unit is a read, or a
 * pair through unit_id; params->prefix_length applies; params->deplete is ignored).  Per unit u, with n members:
 *   total[u]          minimizer count of the unit, as dcn_filter_batch's total (may be NULL)
 *   hits[u * n + j]   DISTINCT minimizer hashes of the unit that are in member j: what a counting dcn_filter_batch on a
 *                     context over member j alone returns as hits (may be NULL)
 *   match[u]          bit j = dcn_decide(hits[u*n+j], total[u], abs, rel, deplete = 0): the unit meets the thresholds
 *                     against member j
 * The context's index must have the set's k, w, minimizer rule and device (the set itself may be the context's index);
 * refused while batches are in flight.  The six counters of the context are left unchanged.  A unit of any length is
 * counted exactly (no DCN_ERR_CAPACITY).  Blocking. */
int dcn_classify_batch(dcn_ctx *ctx, const dcn_index *set, const uint8_t *bases, const uint64_t *offsets,
                       const uint32_t *unit_id, uint32_t n_reads, const dcn_params *params, uint32_t *match,
                       uint32_t *hits, uint32_t *total);
/* The same on DEVICE pointers, enqueued on the context's stream (n_bases / n_units and the validation of d_offsets /
 * d_unit_id as for dcn_filter_batch_device): dcn_ctx_synchronize waits for it and reports a bad batch. */
int dcn_classify_batch_device(dcn_ctx *ctx, const dcn_index *set, const uint8_t *d_bases, const uint64_t *d_offsets,
                              const uint32_t *d_unit_id, uint32_t n_reads, uint64_t n_bases, uint32_t n_units,
                              const dcn_params *params, uint32_t *d_match, uint32_t *d_hits, uint32_t *d_total);

/* ---- coverage: which keys of each member a run of classify calls observed --------------------------------------
 * (no reference counterpart.)  Breadth next to match counts: how many DISTINCT keys of each member the whole input
 * touched.  After coverage is enabled on a set, every dcn_classify_batch / dcn_classify_batch_device call against that
 * set, from any context, marks keys: key K is OBSERVED when some unit of such a call has K among the minimizer hashes
 * counted in its total[u] -- after params->prefix_length and the ACGT filter -- and K is in the set.  That is exactly the
 * union over units of the hashes behind hits[u*n+j], whether or not the unit matched anything.  The observed keys of
 * member j are the observed keys whose mask has bit j.  Marks accumulate until dcn_index_set_coverage_reset or disable;
 * a batch the plan refuses (bad offsets) marks nothing.  Key 0 has a mark of its own.
 * The state (one bit per slot of the set's table, 1/64 of its slot bytes) belongs to the set: every context on the set's
 * device marks the same bits.  dcn_index_set_create allocates none, dcn_index_set_info / dcn_index_memory do not count
 * it, a dcn_index_clone of the set has none, dcn_index_destroy frees it.
 * The reads below are blocking and order after nothing: the caller has waited for its classify calls first (the host
 * form returns complete; the device form needs dcn_ctx_synchronize).  Every call returns DCN_ERR_ARG for an index that
 * is not a set, and the reset, read and keys calls for a set without coverage. */
/* allocate (enable != 0) a zeroed observed-bitmap for the set, or free it (0); not while classify calls on the set are
 * in flight.  Enabling a set that has coverage keeps its marks. */
int dcn_index_set_coverage_enable(dcn_index *set, int enable);
/* clear every mark */
int dcn_index_set_coverage_reset(dcn_index *set);
/* n_members entries each: keys[j] = distinct keys of member j held by the set, observed[j] = how many of them are
 * marked.  Neither may be NULL. */
int dcn_index_set_coverage(const dcn_index *set, uint64_t *observed, uint64_t *keys);
/* observed keys of member `member` (UINT32_MAX = of any member), arbitrary order; *n = count; DCN_ERR_CAPACITY if
 * capacity < count (out may be NULL with capacity 0: *n still receives the count) */
int dcn_index_set_coverage_keys(const dcn_index *set, uint32_t member, uint64_t *out, uint64_t capacity, uint64_t *n);

/* ---- depth: how often each key of a set occurred in the input ------------------------------------------------------
 * (no reference counterpart.)  Coverage says that a member's keys were touched; depth says how often.  An OCCURRENCE is
 * one (read, position) pair of a batch whose minimizer k-mer is counted in its unit's total[u] -- after
 * params->prefix_length and the ACGT filter, each position of a read once, mates of a pair independently.  The DEPTH of
 * key K is the number of occurrences whose hash is K, over all dcn_classify_batch / dcn_classify_batch_device calls
 * against the set, from any context, since depth was enabled or last reset.  It is held per slot of the set's table as a
 * 16-bit counter that SATURATES at 65,535; it does not depend on the thresholds, on match[], or on the unit's size; a
 * batch the plan refuses (bad offsets) counts nothing.  Depth and coverage are independent (either, both or neither);
 * with both on over the same calls a key has depth > 0 exactly when it is observed.  Key 0 has a counter of its own.
 * The state costs 2 bytes per slot of the set's table (1/4 of its slot bytes: 8 GiB for a set of 2^32 slots) and belongs
 * to the set like the coverage bitmap: dcn_index_set_create allocates none, dcn_index_set_info / dcn_index_memory do not
 * count it, a dcn_index_clone has none, dcn_index_destroy frees it.  A context that classifies against a set with depth
 * also holds max_batch_bases / 8 bytes of position bitmap (shared with dcn_locate_batch).
 * The reads below are blocking and order after nothing: the caller has waited for its classify calls first.  Every call
 * returns DCN_ERR_ARG -- before any device work -- for an index that is not a set, a NULL output, a member at or above
 * the set's member count (UINT32_MAX = any member), n_bins outside 2..4096, and (all but enable) a set without depth. */
/* allocate (enable != 0) zeroed counters for the set, or free them (0); not while classify calls on the set are in
 * flight.  Enabling a set that has depth keeps its counts.  DCN_ERR_NOMEM leaves the set as it was. */
int dcn_index_set_depth_enable(dcn_index *set, int enable);
/* zero every counter */
int dcn_index_set_depth_reset(dcn_index *set);
/* n_members entries each, over the keys of member j: observed[j] = keys with depth > 0, sum[j] = the sum of their depths
 * (saturated counters add 65,535), saturated[j] = keys at 65,535 */
int dcn_index_set_depth_stats(const dcn_index *set, uint64_t *observed, uint64_t *sum, uint64_t *saturated);
/* hist[min(depth, n_bins - 1)] = keys of member `member` (UINT32_MAX: of any member) at that depth, n_bins entries,
 * 2 <= n_bins <= 4096; hist[0] = its unobserved keys, so the entries sum to the member's key count */
int dcn_index_set_depth_hist(const dcn_index *set, uint32_t member, uint32_t n_bins, uint64_t *hist);
/* (key, depth) of every key of member `member` (UINT32_MAX: any) with depth > 0, arbitrary order; *n = count;
 * DCN_ERR_CAPACITY if capacity < count (keys / depths may be NULL with capacity 0: *n still receives the count) */
int dcn_index_set_depth_keys(const dcn_index *set, uint32_t member, uint64_t *keys, uint32_t *depths, uint64_t capacity,
                             uint64_t *n);

/* ---- index builder: add sequences call by call, keep keys by how often they occur ------------------------------------
 * (no reference counterpart: index::build reads one input whole and its set keeps no multiplicity.)  A builder is a
 * device table that lives across calls and counts as it inserts; dcn_index_builder_finish hands out plain indexes chosen
 * by count: a minimum for indexes built from reads (every sequencing error mints a key that occurs once), a maximum for
 * repeat-aware indexes.  THE DEFINITION: for every sequence given to dcn_index_builder_add, take the list that
 * fill_minimizer_hashes walks (src/minimizers.rs:125-191), which is what dcn_index_build inserts: IUPAC codes
 * canonicalised before the scan, positions whose k-mer has a non-ACGT byte in the ORIGINAL bytes dropped, the entropy
 * floor applied, sequences shorter than k or k+w-1 contributing nothing.  An OCCURRENCE is a distinct (sequence, position)
 * pair of that list.  The COUNT of key K is the number of occurrences whose hash is K, over all add calls since create.
 * It is held per slot of the table as a 16-bit counter that SATURATES at 65,535; key 0 has a counter of its own.  The count
 * does not depend on how the sequences are split over calls, nor on how a long sequence is cut into pieces inside the
 * library (pieces of a chunk's size that overlap by k+w-2 bases: a position of an overlap is counted once).
 * Device memory: 8 + 2 bytes per slot of the builder's table (sized and grown by dcn_index_memory's rule: a power-of-two
 * number of 16-byte groups, at least four slots per key), and from the first add on one dump-mode context for chunks of
 * 2^27 bases (DCN_BUILD_CHUNK_BASES, as dcn_index_build; about 18 bytes per base of a chunk) plus chunk / 8 bytes of
 * position bitmap.  Growth holds the old and the new table for a moment, as dcn_index_build's does.
 * A builder is NOT thread-safe; all calls are blocking.  Argument errors (the k / w rule and entropy range of
 * dcn_index_build, NULLs, bad bounds, bad n_bins) return DCN_ERR_ARG before any device work.  After an add that failed
 * the counts are unspecified: destroy the builder.
 * (The handle is declared void * in the prototypes: every prototype of this header uses only scalar types and the handle
 * types its bindings are generated and checked against; a C caller keeps a dcn_index_builder * and passes it as is,
 * with (void **)&builder for create.) */
typedef struct dcn_index_builder dcn_index_builder;
/* k, w, entropy_threshold, capacity_keys (a pre-allocation hint; 0 = grow as needed) and device as for dcn_index_build; the
 * minimizer rule in force is captured here, as by every index */
int dcn_index_builder_create(uint8_t k, uint8_t w, float entropy_threshold, uint64_t capacity_keys, int device, void **out);
/* bases / offsets: concatenated sequences and n_seqs+1 byte offsets in host memory, as for dcn_index_build; any number of
 * calls, each with whole sequences */
int dcn_index_builder_add(void *builder, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seqs);
/* any output may be NULL: distinct keys so far; occurrences so far (the true number as a u64, not the saturated sum);
 * bases of all sequences given to add; device bytes of table, counters and position bitmap (not the context's buffers) */
int dcn_index_builder_info(const void *builder, uint64_t *n_keys, uint64_t *n_occurrences, uint64_t *n_bases,
                           uint64_t *device_bytes);
/* hist[min(count, n_bins - 1)] = keys with that count, n_bins entries, 2 <= n_bins <= 4096, as dcn_index_set_depth_hist;
 * hist[0] is always 0 (a key of the builder occurred), the entries sum to n_keys */
int dcn_index_builder_hist(const void *builder, uint32_t n_bins, uint64_t *hist);
/* (key, count) of every key, arbitrary order; *n = n_keys; DCN_ERR_CAPACITY if capacity < n_keys (keys / counts may be
 * NULL with capacity 0: *n still receives the count), as dcn_index_set_depth_keys */
int dcn_index_builder_counts(const void *builder, uint64_t *keys, uint32_t *counts, uint64_t capacity, uint64_t *n);
/* The keys with min_count <= count <= max_count -> a new PLAIN index with the builder's k, w, device and the minimizer
 * rule captured at create, sized for exactly the selected keys.  max_count == 0: no upper bound; min_count == 0 behaves as
 * 1; a saturated key counts as 65,535 in both comparisons.  *n_selected (may be NULL) receives the count; out == NULL:
 * count only, nothing is allocated.  DCN_ERR_ARG: min_count > max_count != 0, either bound above 65,535, out and
 * n_selected both NULL.  The builder stays as it is: finish may be called again with other bounds, and add may follow
 * it.  An empty result is a valid index with 0 keys.  With bounds (1, 0) the key set equals that of dcn_index_build on
 * the same sequences. */
int dcn_index_builder_finish(const void *builder, uint32_t min_count, uint32_t max_count, uint64_t *n_selected,
                             dcn_index **out);
void dcn_index_builder_destroy(void *builder);

/* ---- locate: where in each read the index matched ----------------------------------------------------------
 * (no reference counterpart: the reference answers one verdict per record.)  Segments of every read of a host batch,
 * from the same probes the filter and the classifier make.  THE DEFINITION, per read (mates are independent here:
 * there is no unit_id), with the index's k and w:
 *   1. (hashes, positions) = what get_minimizer_hashes_and_positions yields for the read (src/filter_common.rs:211-310;
 *      here dcn_minimizer_hashes_batch): after the len < k rule, the prefix cut, the stripped trailing newline and the
 *      ACGT filter of positions.
 *   2. A position p is a HIT when its hash is in the index.  On a labelled set its label is the key's member mask and it
 *      is a hit when label & member_mask != 0; on a plain index the label is 1 and member_mask is ignored.  Positions
 *      may repeat in the list; a position is one k-mer, has one hash and one label, and counts once.
 *   3. Walk the distinct hit positions in ascending order.  A hit at p extends the current segment when
 *      p <= segment.end + max_gap, else it starts a new one.  start = the segment's first hit position, end = its last
 *      hit position + k (half-open, in bases of the read as given), n_hits = its distinct hit positions, members = OR of
 *      their labels.
 *   4. Segments with n_hits < min_hits are dropped (after merging: dropping never splits or joins anything).
 *   5. A read's segments are reported in ascending start; they are disjoint and more than max_gap apart.
 * max_gap = 2*w - 1 is the derived default of the layers above (an isolated substituted base leaves at most 2w - 1
 * bases between the minimizer k-mers on its two sides, so that gap joins them and claims nothing larger); with w <= k
 * the hits inside an exactly matching stretch overlap or abut, so max_gap = 0 already yields one segment there. */
typedef struct dcn_locate_params {
    uint32_t max_gap;       /* bases a segment may bridge between the end of one hit k-mer and the start of the next */
    uint32_t min_hits;      /* >= 1: segments with fewer distinct hit positions are dropped */
    uint32_t member_mask;   /* labelled set: only hits whose label meets this mask; ignored for a plain index */
    uint32_t reserved;      /* must be 0 */
    uint64_t prefix_length; /* 0 = whole read, else only the first prefix_length bases */
} dcn_locate_params;
typedef struct dcn_segment {
    uint32_t start, end, n_hits, members;
} dcn_segment; /* 16 bytes */

/*   index        a plain index or a labelled set with the k, w, minimizer rule and device of the context's index
 *   params       a dcn_locate_params; min_hits == 0 or reserved != 0 is DCN_ERR_ARG
 *   seg_offsets  n_reads+1 entries: read r owns segs[seg_offsets[r] .. seg_offsets[r+1])
 *   segs         an array of dcn_segment
 *   capacity     entries available in segs; on DCN_ERR_CAPACITY seg_offsets[] is complete, seg_offsets[n_reads] is the
 *                size needed and segs is not written (segs may be NULL with capacity 0 to ask for the count only)
 * (params and segs are declared void *: every prototype of this header uses only scalar and handle types, which is
 * what lets bindings be generated and checked from it; a C caller passes its dcn_locate_params * / dcn_segment * as is.)
 * Host pointers, blocking, batch limits as for dcn_classify_batch; refused while batches are in flight; the six
 * counters of the context are left unchanged.  Device memory, allocated on the first call and freed with the context:
 * max_batch_bases / 8 bytes of hit bitmap, 4 * max_batch_bases bytes of labels when the index is a set, 16 bytes per
 * read of counts and offsets, and a segment buffer grown to the largest batch's count.  dcn_ctx_set_profiling covers it:
 * pack, plan, scan (minimizer dump), DISTINCT = the probe sweep that marks hits, FINISH = the segment passes. */
int dcn_locate_batch(dcn_ctx *ctx, const dcn_index *index, const uint8_t *bases, const uint64_t *offsets,
                     uint32_t n_reads, const void *params, uint64_t *seg_offsets, void *segs, uint64_t capacity);

/* ---- depth tracks: a set's depth counters, binned along a sequence ------------------------------------------------------
 * (no reference counterpart.)  Depth says how often each key occurred in the sample; a track says where on a sequence --
 * a reference record, or a read -- those keys lie and how deep the sample covered each stretch of it.  It READS a set's
 * depth state and never changes it.  THE DEFINITION, per read r of the batch (mates are independent here: there is no
 * unit_id), with the set's k and w:
 *   1. (hashes, positions) = what get_minimizer_hashes_and_positions yields for the read (src/filter_common.rs:211-310;
 *      here dcn_minimizer_hashes_batch): after the len < k rule, the prefix cut, the stripped trailing newline and the
 *      ACGT filter of positions.  A position the list repeats counts once; it has one hash.
 *   2. Bins.  With bin_bases = B > 0 read r owns ceil(len_r / B) bins (len_r: the read as given, so none for an empty
 *      read); bin b covers bases [b*B, min((b+1)*B, len_r)) and a position p belongs to bin p / B, by where its k-mer
 *      starts.  With B == 0 every read owns exactly one bin, an empty read too.  Bins past a prefix cut exist and are
 *      all zero.
 *   3. Per bin, over its distinct positions: n_positions = how many there are; n_keys = those whose hash is in the set
 *      with label & member_mask != 0; n_observed = those of n_keys whose depth is > 0; sum_depth = the sum over n_keys of
 *      d and max_depth = the maximum of d, where d = depth when depth_cap == 0, else min(depth, depth_cap).  A
 *      saturated counter contributes 65,535.  Key 0 uses its own counter word.
 *   4. Nothing depends on thresholds, on earlier track calls, or on how the library cuts the work. */
typedef struct dcn_track_params {
    uint32_t bin_bases;     /* 0: one bin per read */
    uint32_t member_mask;   /* keys whose label meets it; 0 is DCN_ERR_ARG */
    uint32_t depth_cap;     /* 0: none; else 1..65535: each depth counts as min(depth, cap) */
    uint32_t reserved;      /* must be 0 */
    uint64_t prefix_length; /* 0 = whole read, else only the first prefix_length bases */
} dcn_track_params; /* 24 bytes */
typedef struct dcn_track_bin {
    uint32_t n_positions, n_keys, n_observed, max_depth;
    uint64_t sum_depth;
} dcn_track_bin; /* 24 bytes */

/*   set          a labelled set with depth enabled and the k, w, minimizer rule and device of the context's index
 *   params       a dcn_track_params
 *   bin_offsets  n_reads+1 entries, always complete: read r owns bins[bin_offsets[r] .. bin_offsets[r+1])
 *   bins         an array of dcn_track_bin
 *   capacity     entries available in bins; on DCN_ERR_CAPACITY bin_offsets[n_reads] is the size needed and bins is not
 *                written (bins may be NULL with capacity 0 to ask for the count only).  bin_offsets follows from offsets
 *                alone: the capacity is checked before anything is enqueued.
 * (params and bins are declared void * for the reason given at dcn_locate_batch.)  Host pointers, blocking, batch limits
 * as for dcn_classify_batch; refused while batches are in flight; the six counters of the context are left unchanged.
 * DCN_ERR_ARG, before any device work: NULLs, reserved != 0, member_mask == 0 or with a bit at or above the set's member
 * count, depth_cap > 65535, an index that is not a labelled set, a set without depth.  The caller has waited for the
 * classify calls whose counts it wants to see.  Device memory, allocated on the first call and freed with the context:
 * max_batch_bases / 8 bytes of position bitmap and 4 * max_batch_bases bytes of values (both shared with
 * dcn_locate_batch), 16 bytes per read of offsets, and a bin buffer grown to the largest batch's count.
 * dcn_ctx_set_profiling covers it: pack, plan, scan (minimizer dump), DISTINCT = the probe sweep that marks positions and
 * reads the counters, FINISH = the reduction into bins. */
int dcn_depth_track_batch(dcn_ctx *ctx, const dcn_index *set, const uint8_t *bases, const uint64_t *offsets,
                          uint32_t n_reads, const void *params, uint64_t *bin_offsets, void *bins, uint64_t capacity);

/* ---- place: which record of a reference, at which coordinate, on which strand (ABI 1.9) -----------------------------
 * (no reference counterpart.)  Two parts: an ANCHOR MAP, a dcn_index whose slots know where on a reference their key
 * lies, and dcn_place_batch, in which a read's anchor hits vote on a diagonal.
 *
 * THE DEFINITION OF AN ANCHOR.  Records are numbered 0, 1, ... in the order they are added, over all dcn_anchor_map_add
 * calls.  The occurrence list of record R is the distinct positions P of get_minimizer_hashes_and_positions(record, k,
 * w, prefix_length = 0) (src/filter_common.rs:211-310: after the len < k rule, the stripped trailing newline and the ACGT
 * filter; the filter-side list, the one depth tracks use), each with its hash.  An occurrence whose hash is not a key of
 * the map is ignored.  A key of the map is an ANCHOR when, over everything added so far, exactly one (R, P) has its
 * hash; the anchor carries one strand bit: whether the forward k-mer at (R, P) is the canonical one (kmer <=
 * revcomp(kmer) as the packed values the k-mer hash compares: the hash is taken of the smaller one).  A key with two
 * or more distinct occurrences is a REPEAT and never votes; a key with none is UNSEEN.  The state does not depend on the
 * order of records within a call, on how the library cuts a record, or on how many calls the records were spread over.
 * Limits: at most 2^31 - 1 records, a record of at most 2^32 - 1 bases.
 *
 * An anchor map is a copy of an index's slot table (it owns its memory; the source may be destroyed) with one 64-bit
 * word per slot beside it (8 bytes per slot, which dcn_index_memory does not count).  It is a dcn_index: a context can
 * be created over it and every call that reads an index sees its keys; dcn_index_clone of it gives a plain index
 * without the words; dcn_index_destroy frees everything.  The table never grows: the caller chooses which keys may
 * anchor by what it builds the map from (the reference's own index, that index minus a host, the member-specific keys
 * of a set).  Every call below returns DCN_ERR_ARG for an index that is not a map. */
int dcn_anchor_map_create(const dcn_index *index, dcn_index **out);
/* Add n_records records (host pointers, offsets[n_records + 1], blocking).  ctx: an idle context whose index has the
 * map's k, w, minimizer rule and device (the map itself may be that index); batch limits as for dcn_classify_batch.
 * Whole records are used.  *first_record (may be NULL) receives the number of the batch's first record.  DCN_ERR_ARG
 * before any device work when the records would exceed the limits above.  A batch that is refused adds nothing and
 * does not advance the record count. */
int dcn_anchor_map_add(dcn_index *map, dcn_ctx *ctx, const uint8_t *bases, const uint64_t *offsets,
                       uint32_t n_records, uint32_t *first_record);
/* Records added, keys of the map, and how many of them are anchors and repeats (a blocking sweep; outputs may be NULL). */
int dcn_anchor_map_info(const dcn_index *map, uint32_t *n_records, uint64_t *n_keys, uint64_t *n_anchors,
                        uint64_t *n_repeats);
/* The anchors, in arbitrary order (a blocking sweep).  *n is always the number there is; DCN_ERR_CAPACITY when that is
 * more than capacity, and nothing is written then (capacity 0 with NULL arrays asks for the count). */
int dcn_anchor_map_anchors(const dcn_index *map, uint64_t *keys, uint32_t *records, uint32_t *positions,
                           uint64_t capacity, uint64_t *n);

/* THE DEFINITION OF A PLACEMENT.  Mates are independent (no unit_id).  Per read of length len (the read as given), with
 * the map's k and w, band_bases = W:
 *   1. (hashes, positions) = what get_minimizer_hashes_and_positions yields for the read: after the len < k rule, the
 *      prefix cut, the stripped trailing newline and the ACGT filter.  A position the list repeats counts once;
 *      n_positions = the number of distinct positions.
 *   2. A position q is an ANCHOR HIT when its hash is an anchor of the map, at (R, P); n_anchors = how many there are.
 *      Its orientation o is '+' when the read's k-mer at q and the record's k-mer at P are canonical on the same side
 *      (both strand bits equal; equivalently the two k-mers' texts are equal -- a k-mer that is its own reverse
 *      complement counts as '+'), else '-' (the read's k-mer is the reverse complement).
 *   3. Its diagonal is D = P - q + len for '+' and D = P + q for '-' (non-negative, 64 bits).  A read cut from the
 *      record's forward strand at a has D = a + len at every hit, the reverse complement of that cut D = a + len - k.
 *   4. The hit votes for the two cells (R, o, j) with j = D / W and j = D / W + 1: cell j collects the diagonals in
 *      [(j-1)*W, (j+1)*W), so any group of hits whose diagonals differ by less than W shares a cell.
 *   5. The best cell has the most votes; ties go to the smallest (R, o, j), '+' before '-'.
 *   6. With votes >= min_votes the read is placed: record = R, reverse = (o == '-'), votes, and over the best cell's
 *      hits read_start = min q, read_end = max q + k, ref_start = min P, ref_end = max P + k.
 *   7. Otherwise record = UINT32_MAX and every field but n_anchors and n_positions is 0.
 *   8. Nothing depends on thresholds of the filter, on earlier calls, or on how the library cuts the work.  Integers only.
 * n_anchors - votes is the number of anchor hits the placement does not explain (a chimera shows there); no second-best
 * cell is reported (dcn_place_split_batch below reports further placements, a rival and a quality).  band_bases = 256 and min_votes = 2 are the conventions of the layers above (the 2 is the filter's
 * -a 2), not measured optima. */
typedef struct dcn_place_params {
    uint32_t band_bases;    /* W >= 1: width of a diagonal band */
    uint32_t min_votes;     /* >= 1: a read whose best cell has fewer votes is unplaced */
    uint64_t prefix_length; /* 0 = whole read */
    uint32_t reserved[2];   /* must be 0 */
} dcn_place_params; /* 24 bytes */
typedef struct dcn_placement {
    uint32_t record;  /* UINT32_MAX: unplaced */
    uint32_t reverse; /* 0 | 1 */
    uint32_t votes, n_anchors, n_positions;
    uint32_t read_start, read_end; /* bases of the read as given, half-open */
    uint32_t reserved;             /* 0 */
    uint64_t ref_start, ref_end;   /* bases of the record, half-open */
} dcn_placement; /* 48 bytes */

/*   map         an anchor map with the k, w, minimizer rule and device of the context's index
 *   params      a dcn_place_params
 *   placements  n_reads entries of dcn_placement
 * (params and placements are declared void * for the reason given at dcn_locate_batch.)  Host pointers, blocking, batch
 * limits as for dcn_classify_batch; refused while batches are in flight; the six counters of the context are left
 * unchanged.  DCN_ERR_ARG, before any device work: NULLs, reserved != 0, band_bases == 0, min_votes == 0, an index that
 * is not a map.  Device memory, allocated on the first call and freed with the context: max_batch_bases / 8 bytes of
 * position bitmap (shared with dcn_locate_batch), as much again for the anchor bitmap, 8 * max_batch_bases bytes of one
 * word per base (12 GB for a context of 1.5 Gbp; written only where a position is an anchor hit), and 52 bytes per read.  dcn_ctx_set_profiling covers it: pack, plan, scan (minimizer dump), DISTINCT = the
 * probe sweep that marks positions and stores the anchor of each anchor hit, FINISH = the vote. */
int dcn_place_batch(dcn_ctx *ctx, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets,
                    uint32_t n_reads, const void *params, void *placements);

/* ---- split placements: several per read, each with its rival and a quality (ABI 1.10) -------------------------------
 * THE DEFINITION OF A SPLIT PLACEMENT.  Steps 1-4 are those of THE DEFINITION OF A PLACEMENT (positions, anchor hits,
 * orientation, diagonal D, the two cells D / W and D / W + 1 of a hit).  With N = max_placements:
 *   1. ROUNDS.  H_0 = the read's anchor hits.  In round t = 0, 1, ...: cells are counted over H_t only; C_t is the best
 *      cell by rule 5 above (most votes, ties to the smallest (R, o, j), '+' before '-') and v_t its votes; H_{t+1} is
 *      H_t without the hits of C_t, those with its (R, o) and D / W in {j - 1, j}.  Rounds end when H_t is empty or after
 *      round t = N; that last round is computed and never reported.  v_t never rises: a cell's count over H_{t+1}, a
 *      subset of H_t, is at most its count over H_t, which is at most v_t.
 *   2. REPORTED are the rounds t < N with v_t >= min_votes (a prefix of the rounds, by the above).  Each carries record,
 *      reverse, votes, read_start/_end and ref_start/_end exactly as rule 6 defines them, over the hits of C_t in H_t;
 *      rank = t; n_placed = how many the read has; and the read's n_anchors and n_positions.
 *   3. RIVAL.  The read interval of a computed round, reported or not, is [min q, max q + k) over its cell's hits.  Two
 *      intervals intersect when max(starts) < min(ends): touching is not intersecting.  rival_votes of placement t is
 *      the largest v_u over all computed rounds u != t whose interval intersects t's; 0 when there is none.
 *   4. QUALITY.  mapq = 0 when rival_votes >= votes, else 60 * (votes - rival_votes) / votes by integer division: 0 .. 60.
 *      It is a convention, like band_bases = 256 and min_votes = 2, and NOT a calibrated probability.
 *   5. Integers only.  Nothing depends on tiles, on which kernel places a read, on partitions of the count, or on how
 *      a batch is cut.  Round 0 is dcn_place_batch's placement: max_placements = 1 reports that placement and its rival.
 * Two parts of a chimera that do not overlap on the read each get mapq 60; a weaker cell on the same stretch of the read
 * as a stronger one gets 0. */
#define DCN_PLACE_SPLIT_MAX 8
typedef struct dcn_place_split_params {
    uint32_t band_bases, min_votes; /* as dcn_place_params */
    uint64_t prefix_length;
    uint32_t max_placements;        /* 1 .. DCN_PLACE_SPLIT_MAX */
    uint32_t reserved[3];           /* must be 0 */
} dcn_place_split_params; /* 32 bytes */
typedef struct dcn_split_placement {
    /* the 48 bytes of dcn_placement, field for field */
    uint32_t record;
    uint32_t reverse;
    uint32_t votes, n_anchors, n_positions;
    uint32_t read_start, read_end;
    uint32_t reserved; /* 0 */
    uint64_t ref_start, ref_end;
    /* then */
    uint32_t rank, n_placed, rival_votes, mapq;
} dcn_split_placement; /* 64 bytes */

/*   map            as for dcn_place_batch
 *   params         a dcn_place_split_params
 *   place_offsets  n_reads + 1 entries: read r owns placements[place_offsets[r] .. place_offsets[r + 1]), ranks
 *                  ascending; an unplaced read owns nothing
 *   placements     capacity entries of dcn_split_placement
 *   read_counts    NULL, or 2 * n_reads entries: n_anchors and n_positions of every read, unplaced ones included; filled
 *                  whenever place_offsets is
 * (params and placements are declared void * for the reason given at dcn_locate_batch.)  DCN_ERR_CAPACITY follows the
 * contract stated at dcn_locate_batch: the offsets are complete, the total is place_offsets[n_reads], no placement is
 * written, and NULL with capacity 0 asks for the count.  Host pointers, blocking, batch limits as for
 * dcn_classify_batch; refused while batches are in flight; the six counters of the context are left unchanged.
 * DCN_ERR_ARG, before any device work: NULLs, reserved != 0, band_bases == 0, min_votes == 0, max_placements 0 or above
 * DCN_PLACE_SPLIT_MAX, an index that is not a map.  Device memory, allocated on the first call and freed with the
 * context: what dcn_place_batch states per base (shared with it, all but its 48 bytes per read of placements), one more
 * max_batch_bases / 8 bytes for the copy of the anchor bitmap that the rounds clear, and per read 28 bytes of counts
 * and offsets, for the max_batch_reads of the context, plus 32 * (max_placements + 1) bytes of rounds and
 * 64 * max_placements bytes of rows, for the largest batch so far (444 bytes per read at max_placements = 4).
 * dcn_ctx_set_profiling covers it: pack, plan, scan (minimizer dump), DISTINCT = the mark sweep of dcn_place_batch,
 * FINISH = the vote and the compaction into rows. */
int dcn_place_split_batch(dcn_ctx *ctx, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets,
                          uint32_t n_reads, const void *params, uint64_t *place_offsets, void *placements,
                          uint64_t capacity, uint32_t *read_counts);

/* ---- paired placements: mates placed jointly, proper pairs, rescue, insert sizes (ABI 1.11) --------------------------
 * THE DEFINITION OF A PAIRED PLACEMENT.  Pair u is read 2u (mate 1) and read 2u + 1 (mate 2) of the batch: n_reads is
 * even.  N = max_placements, I = max_insert.  Positions, anchor hits, cells and rounds are exactly those of THE
 * DEFINITION OF A SPLIT PLACEMENT: rounds 0 .. N are computed per mate, each with its votes, its (R, o), its read
 * interval [min q, max q + k) and its reference extent [ref_start, ref_end) = [min P, max P + k) of placement rule 6.
 *   1. CANDIDATES of a mate are its computed rounds t < N, whatever their votes.
 *   2. CONCORDANT.  A combination (a, b) is a candidate a of mate 1 with a candidate b of mate 2.  It is concordant when
 *      the two rounds lie on the same record; their orientations differ (call the '+' round F and the '-' round V);
 *      F.ref_start < V.ref_end (the forward mate begins before the reverse mate ends: touching is not enough, mates
 *      that overlap fully are fine); T = max(F.ref_end, V.ref_end) - min(F.ref_start, V.ref_start) <= I; and
 *      max(votes_a, votes_b) >= min_votes (one mate must stand on its own, the other may have a single hit).
 *   3. CHOSEN is the concordant combination with the largest votes_a + votes_b, ties to the smallest a, then the
 *      smallest b.  If one exists the pair is PROPER and the mates report rounds a and b.  Otherwise each mate reports
 *      its round 0 when its votes reach min_votes, and else is unplaced as in placement rule 7: record = UINT32_MAX and
 *      every field but n_anchors and n_positions is 0 (flags included: an unplaced row carries none).
 *   4. PAIRED VOTES.  For a computed round t of a mate, pv(t) = votes_t + the most votes of any candidate of the other
 *      mate that is concordant with t: + 0 when there is none, and + 0 for t = N, which is not a candidate.  Both rows
 *      of a proper pair so carry pair_votes = votes_a + votes_b.
 *   5. RIVAL AND QUALITY.  rival_votes of a reported round t is the largest pv(u) over the same mate's computed rounds
 *      u != t (u up to N) whose read interval intersects t's (split rule 3); 0 when there is none.  mapq = 0 when
 *      rival_votes >= pv(t), else 60 * (pv(t) - rival_votes) / pv(t) by integer division.  It is a convention, as
 *      before, and NOT a calibrated probability.  A pair with no concordant combination gives each mate exactly the
 *      rank-0 row of dcn_place_split_batch, or no row's worth.
 *   6. FLAGS AND TEMPLATE LENGTH.  flags bit 0 is PROPER; bit 1 is RESCUED: the pair is proper and this mate's reported
 *      round has votes < min_votes; bit 2 is MATE_PLACED: this row is placed and so is the other mate's.  tlen: in a
 *      proper pair the mate with the smaller ref_start gets +T, a tie goes to mate 1, and the other mate gets -T;
 *      otherwise 0.  rank is the reported round's index; pair_votes = pv(rank); n_placed, n_anchors and n_positions are
 *      dcn_place_split_batch's values for that read.
 *   7. INSERT HISTOGRAM.  tlen_hist[min(T / hist_bin_bases, DCN_PAIR_HIST_BINS - 1)] counts the proper pairs of this
 *      call.  The array is overwritten by every call: the caller sums across calls.
 *   8. Integers only.  Nothing depends on tiles, on which vote kernel served which mate, on LDS partitions or on how a
 *      batch is cut (as long as no pair is cut).
 * The orientation library is FR only.  A mate's candidates are its first N rounds: a mate with many stray single hits
 * may not compute its concordant one (there is no windowed recount around the partner).  max_insert = 1000 and
 * hist_bin_bases = 8 are conventions of the layers above, like band_bases = 256, not measured optima. */
#define DCN_PAIR_HIST_BINS 256
#define DCN_PAIR_PROPER 1u
#define DCN_PAIR_RESCUED 2u
#define DCN_PAIR_MATE_PLACED 4u
typedef struct dcn_place_pair_params {
    uint32_t band_bases, min_votes; /* as dcn_place_params */
    uint64_t prefix_length;
    uint32_t max_placements;        /* 1 .. DCN_PLACE_SPLIT_MAX */
    uint32_t max_insert;            /* >= 1 */
    uint32_t hist_bin_bases;        /* >= 1 */
    uint32_t reserved[3];           /* must be 0 */
} dcn_place_pair_params; /* 40 bytes */
typedef struct dcn_pair_placement {
    /* the 64 bytes of dcn_split_placement, field for field (rival_votes and mapq by rule 5) */
    uint32_t record;
    uint32_t reverse;
    uint32_t votes, n_anchors, n_positions;
    uint32_t read_start, read_end;
    uint32_t reserved; /* 0 */
    uint64_t ref_start, ref_end;
    uint32_t rank, n_placed, rival_votes, mapq;
    /* then */
    uint32_t flags;      /* DCN_PAIR_* */
    uint32_t pair_votes; /* pv(rank) */
    int64_t tlen;
} dcn_pair_placement; /* 80 bytes */

/*   map        as for dcn_place_batch
 *   params     a dcn_place_pair_params
 *   rows       n_reads entries of dcn_pair_placement: row 2u is mate 1 of pair u, row 2u + 1 mate 2; unplaced mates
 *              have a row too (fixed size: no CSR and no DCN_ERR_CAPACITY)
 *   tlen_hist  NULL, or DCN_PAIR_HIST_BINS entries
 * (params and rows are declared void * for the reason given at dcn_locate_batch.)  Host pointers, blocking, batch limits
 * as for dcn_place_split_batch; refused while batches are in flight; the six counters of the context are left
 * unchanged.  DCN_ERR_ARG, before any device work: NULLs, reserved != 0, band_bases, min_votes, max_insert or
 * hist_bin_bases == 0, max_placements 0 or above DCN_PLACE_SPLIT_MAX, an odd n_reads, an index that is not a map.
 * n_reads = 0 succeeds and zeroes the histogram when one is given.  Device memory: what dcn_place_split_batch states
 * (shared with it, all but its rows), plus 80 bytes per read of max_batch_reads for the rows and 2 KB of histogram.
 * dcn_ctx_set_profiling covers it: pack, plan, scan (minimizer dump), DISTINCT = the mark sweep, FINISH = the bitmap
 * copy, the rounds and the pairing. */
int dcn_place_pair_batch(dcn_ctx *ctx, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets,
                         uint32_t n_reads, const void *params, void *rows, uint64_t *tlen_hist);

/* ---- verified placements: kept reference bases, edit distance (ABI 1.13) ---------------------------------------------
 * (no reference counterpart.)  The placement calls above compare minimizers only.  An anchor map that KEEPS BASES holds
 * its records' bases on the device, and dcn_verify_batch compares each placement's read interval with its record
 * interval base by base.
 *
 * dcn_anchor_map_keep_bases: from then on every dcn_anchor_map_add also appends the batch's 2-bit stream and invalid-base
 * bits (what the context's front end has packed) to a store the map owns.  It comes before the first add: DCN_ERR_ARG once
 * the map has records, and for an index that is not a map; calling it again changes nothing.  The store costs 0.375 B per
 * base of device memory, which dcn_index_memory does not count (like the anchor words); it grows geometrically (the test
 * hook DCN_ANCHOR_STORE_BASES, read at call time, sets the capacity it starts with); a refused add appends nothing;
 * dcn_index_clone gives an index without it, dcn_index_destroy frees it.  The lengths of the records stay on the host.  A
 * map that keeps no bases behaves exactly as before in every call. */
int dcn_anchor_map_keep_bases(dcn_index *map);
/* Bases [start, start + n_bases) of a record, as text: ACGT for a valid base (upper case whatever was added), N for every
 * base that was not in ACGTacgt.  Blocking.  DCN_ERR_ARG for a map that keeps no bases, a record not added yet, or a range
 * that goes past the record's end. */
int dcn_anchor_map_fetch(const dcn_index *map, uint32_t record, uint64_t start, uint64_t n_bases, uint8_t *out);

/* THE DEFINITION OF A VERIFIED PLACEMENT.  For a row with record != UINT32_MAX:
 *   1. S = read[read_start, read_end) of the read as given; when reverse is set, S is its reverse complement.
 *      T = record[ref_start, ref_end).  m = |S|, n = |T|; either may be 0.
 *   2. Two bases are EQUAL when both are in ACGTacgt and are the same letter regardless of case.  A base outside that
 *      alphabet equals nothing, not even itself (it is the pack kernel's invalid bit); the complement of an invalid base
 *      is invalid.
 *   3. d = the Levenshtein distance of S and T: substitution, insertion and deletion at cost 1 each, global over both
 *      whole intervals.
 *   4. E = min(max_edits, max(m, n) * max_permille / 1000), by integer division.
 *   5. edits = d when d <= E, else DCN_VERIFY_OVER.
 *   6. A row with record == UINT32_MAX gets DCN_VERIFY_UNPLACED; its other fields are not looked at.
 *   7. Integers only.  Nothing depends on the band a kernel uses, on lanes, on LDS sizes or on how a batch is cut.
 * Global over the extents: both intervals start and end on a k-mer of an anchor hit of the placement's cell, and rule 6 of
 * placement puts the first and the last hit's diagonals within the cell's range, so |n - m| < 2 W.  The threshold: an
 * alignment of cost <= E never leaves the diagonals [-E, +E], which makes a banded or wavefront kernel exact, not
 * approximate.  max_edits = 1023 and max_permille = 200 are the conventions of the layers above, not measured optima. */
#define DCN_VERIFY_MAX_EDITS 1023u
#define DCN_VERIFY_OVER 0xFFFFFFFEu
#define DCN_VERIFY_UNPLACED 0xFFFFFFFFu
typedef struct dcn_verify_params {
    uint32_t max_edits;    /* 0 .. DCN_VERIFY_MAX_EDITS */
    uint32_t max_permille; /* 0 .. 1000 */
    uint32_t row_stride;   /* bytes from one row to the next: >= 48, a multiple of 8 (48, 64, 80 for the three row types) */
    uint32_t reserved;     /* must be 0 */
} dcn_verify_params; /* 16 bytes */

/*   map          an anchor map that keeps bases, with the k, w, minimizer rule and device of the context's index
 *   params       a dcn_verify_params
 *   row_offsets  NULL: row r belongs to read r and n_rows == n_reads (dcn_place_batch's and dcn_place_pair_batch's rows);
 *                else n_reads + 1 entries: read r owns rows[row_offsets[r] .. row_offsets[r + 1]) -- place_offsets as
 *                dcn_place_split_batch returns it
 *   rows         n_rows placements, row_stride bytes apart; only the 48 bytes of dcn_placement at the head of each are
 *                read, which the three row types share field for field
 *   edits        n_rows entries
 * (params and rows are declared void * for the reason given at dcn_locate_batch.)  Host pointers, blocking, batch limits
 * as for dcn_place_batch; refused while batches are in flight; the six counters of the context are left unchanged.
 * DCN_ERR_ARG, before any device work: NULLs, reserved != 0, max_edits above DCN_VERIFY_MAX_EDITS, max_permille > 1000, a
 * row_stride below 48 or not a multiple of 8, a map that keeps no bases, row_offsets that do not start at 0, ascend and
 * end at n_rows, and a placed row with record >= the records added, reverse > 1, read_start > read_end, read_end > the
 * read's length, ref_start > ref_end or ref_end > the record's length: the message names the first such row.  The kernel
 * trusts nothing the host has not checked.  The batch is staged and packed again (no plan, no scan), so the call may
 * follow any placement call on the same context.  Device memory, freed with the context: 36 bytes per row of the largest
 * call.  dcn_ctx_set_profiling covers it: pack in its slot, the verify kernel in FINISH; plan, scan and DISTINCT are empty. */
int dcn_verify_batch(dcn_ctx *ctx, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                     const void *params, const uint64_t *row_offsets, const void *rows, uint64_t n_rows, uint32_t *edits);

/* ---- aligned placements: the CIGAR of each verified placement (ABI 1.14) ---------------------------------------------
 * (no reference counterpart.)  dcn_verify_batch ends at a number; dcn_align_batch also says where the edits are.
 *
 * THE DEFINITION OF AN ALIGNED PLACEMENT.  Rules 1-6 of a verified placement stand: S, T, m, n, EQUAL, d, E, OVER,
 * UNPLACED.  Added:
 *   A1. A row with edits = d <= E has an alignment.  A row that is OVER or UNPLACED has zero ops.
 *   A2. D[i][j] is the Levenshtein distance of S[0, i) and T[0, j) under rule 2's equality.
 *   A3. Walk from (m, n) to (0, 0).  At (i, j) != (0, 0) with s = D[i][j], take the first that applies:
 *         X  if i > 0, j > 0 and D[i-1][j-1] = s - 1.  Go to (i-1, j-1).
 *         I  (a base of S alone) if i > 0 and D[i-1][j] = s - 1.  Go to (i-1, j).
 *         D  (a base of T alone) if j > 0 and D[i][j-1] = s - 1.  Go to (i, j-1).
 *         =  otherwise.  Go to (i-1, j-1).  Then S[i-1] EQUAL T[j-1] and D[i-1][j-1] = s, a property of unit costs.
 *   A4. The steps reversed are the alignment from the start of both intervals.  Equal neighbours merge into runs.  A run
 *       is one uint32_t, len << 4 | op, with BAM's codes: I = 1, D = 2, '=' = 7, X = 8.  #X + #I + #D = d; '=' + X + I
 *       covers m; '=' + X + D covers n; n_ops <= 2 d + 1.  A row with max(m, n) >= 2^28 is DCN_ERR_ARG, naming the row.
 *   A5. S is the reverse complement when the row says so, and T is always forward.  So the ops are in the record's
 *       direction, as PAF's cg wants them.
 *   A6. Integers only.  The result is unique.  Nothing depends on lanes, LDS sizes, the scratch budget or how a batch is
 *       cut.
 * A3 is stated in D alone: a model needs no wavefront.  The kernel reads no base for it, because D[i][j] <= s - 1 exactly
 * when F_{s-1}[j - i] >= i, where F_s[k] is the furthest base of S that a path of cost <= s reaches on diagonal k = j - i:
 * what the wavefront of the verify kernel computes.  The align kernel runs that wavefront once more with E = d and keeps
 * every F_s (4 (d + 1)^2 bytes per row, 4 MiB at d = 1023), then walks back in d steps. */
#define DCN_CIGAR_INS 1u
#define DCN_CIGAR_DEL 2u
#define DCN_CIGAR_EQUAL 7u
#define DCN_CIGAR_DIFF 8u

/*   ctx .. n_rows   as for dcn_verify_batch: the same checks in the same order with the same messages and row numbers
 *   edits           n_rows entries: exactly what dcn_verify_batch returns
 *   cigar_offsets   n_rows + 1 entries: row r's runs are cigar[cigar_offsets[r] .. cigar_offsets[r + 1])
 *   cigar           `capacity` entries, or NULL with capacity 0
 * DCN_ERR_ARG beyond dcn_verify_batch's: cigar_offsets is NULL; a placed row with max(m, n) >= 2^28 (the message names
 * the first such row); more than 2^32 - 1 rows (the runs are counted per row in 32 bits and scanned to 64-bit offsets);
 * cigar is NULL although the runs fit `capacity` and there are some.  DCN_ERR_CAPACITY when the rows have more than
 * `capacity` runs: edits and cigar_offsets are complete, cigar_offsets[n_rows] is the size needed, and cigar is not
 * written (dcn_locate_batch's convention: call again with that capacity).  Host pointers, blocking, refused while batches
 * are in flight; the six counters of the context are left unchanged.
 * The traces of the aligned rows go through one device buffer, in groups of consecutive rows: a group closes when the
 * next row's trace would pass the budget, and always holds at least one row.  The budget is 1 GiB, or the bytes that the
 * environment variable DCN_ALIGN_TRACE_BYTES names, read at call time (tests set a few hundred bytes).  The default is a
 * convention, not a measured optimum: nobody has tuned it, and in the one run recorded in DESIGN.md section 17 a budget of
 * 8 GiB was more than twice as fast on 10 kbp reads, because 1 GiB of their traces is fewer rows than the device holds waves.
 * The results do not depend on it.  Device memory, freed with the context, each sized by
 * the largest call: the trace buffer, max(min(budget, the call's traces), the largest row's trace); 36 bytes per row as
 * for dcn_verify_batch and 12 more; 24 bytes per aligned row; 4 (2 d + 1) bytes of run slots per aligned row; the runs.
 * The wavefront runs twice per aligned row, once to find d and once to keep its wavefronts.
 * dcn_ctx_set_profiling covers it: pack in its slot; the verify kernel, the align kernel of every group, the scan of the
 * run counts and the gather in FINISH (with the two read-backs between them); plan, scan and DISTINCT are empty. */
int dcn_align_batch(dcn_ctx *ctx, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                    const void *params, const uint64_t *row_offsets, const void *rows, uint64_t n_rows, uint32_t *edits,
                    uint64_t *cigar_offsets, uint32_t *cigar, uint64_t capacity);

/* ---- pileup: per-base counts of the aligned rows on the reference, and site calls (ABI 1.15) --------------------------
 * (no reference counterpart.)  dcn_align_batch's results are per read; a pileup sums them per reference position.
 *
 * THE DEFINITION OF A PILEUP.  Rules 1-6 of a verified placement and A1-A6 of an aligned placement stand.  Added:
 *   P1. A map that keeps bases may hold a pileup: for every base of every record added so far, eight uint32_t counters,
 *       all zero when enabled: the columns DCN_PILEUP_A .. DCN_PILEUP_REV below.
 *   P2. Only a row with an alignment (A1: edits = d <= E) adds.  An OVER row, an UNPLACED row and a row with n = 0 add
 *       nothing.  The library has no policy on which rows count: a caller leaves a row out by setting its record to
 *       UINT32_MAX.
 *   P3. Walk the row's runs from the start of both intervals; i counts bases of S (already reverse-complemented when the
 *       row says so), j bases of T.
 *         An '=' or X step at (i, j) adds 1 at record position ref_start + j, in the column of S[i]: A, C, G, T by rule
 *           2's alphabet regardless of case, or N when S[i] is invalid.
 *         A D step adds 1 to DEL at ref_start + j.
 *         Every '=', X and D step of a row with reverse = 1 also adds 1 to REV at its position.
 *         An I RUN, of whatever length, adds 1 to INS: at ref_start + j - 1, the base of T in front of it, if j > 0, else
 *           at ref_start.  This is always inside T, since n > 0.  The inserted bases are recorded only by an insertion
 *           ledger (below).
 *   P4. depth(p) is the sum of columns 0-5.  Over one row, each position of T receives exactly one add among columns 0-5.
 *   P5. Integers only.  Adds commute: the counters after any sequence of calls depend only on the multiset of rows added,
 *       not on how batches are cut, on align's trace groups, on lanes or on order.  A counter wraps above 2^32 - 1;
 *       nothing saturates.
 *   P6. Calls, with the parameters min_depth and min_permille (0 .. 1000).  At a position:
 *         best is the first of A, C, G, T, DEL with the largest count; N never wins.
 *         The position is CALLED when depth > 0, depth >= min_depth and best_count * 1000 >= depth * min_permille
 *           (64-bit products).  The call character is then one of ACGT-; otherwise it is N.
 *         ref is the record's base, where an invalid base differs from everything.
 *         Flags: DCN_PILEUP_SITE_SUB when the position is called, the call is a base and it differs from ref;
 *           DCN_PILEUP_SITE_DEL when it is called and the call is '-'; DCN_PILEUP_SITE_INS when depth > 0,
 *           depth >= min_depth and INS * 1000 >= depth * min_permille, whether or not the position is called.
 *         A SITE is a position with flags != 0; site_info = flags | call_code << 8 | ref_code << 16, with the codes
 *           0-3 = A, C, G, T, 4 = DEL and DCN_PILEUP_NO_CODE = no call, or an invalid reference base.
 *       min_depth = 3 and min_permille = 500 are conventions of the layers above, not measured optima. */
#define DCN_PILEUP_A 0
#define DCN_PILEUP_C 1
#define DCN_PILEUP_G 2
#define DCN_PILEUP_T 3
#define DCN_PILEUP_N 4
#define DCN_PILEUP_DEL 5
#define DCN_PILEUP_INS 6
#define DCN_PILEUP_REV 7
#define DCN_PILEUP_COLUMNS 8
#define DCN_PILEUP_SITE_SUB 1u
#define DCN_PILEUP_SITE_DEL 2u
#define DCN_PILEUP_SITE_INS 4u
#define DCN_PILEUP_NO_CODE 7u
typedef struct dcn_pileup_call_params {
    uint32_t min_depth;
    uint32_t min_permille; /* 0 .. 1000 */
    uint32_t reserved[2];  /* must be 0 */
} dcn_pileup_call_params;  /* 16 bytes */

/* dcn_anchor_map_pileup_enable comes after the records: it allocates 32 bytes of device memory per kept base (whole
 * 32-base groups, as the store counts them) and zeroes them; dcn_index_memory does not count this memory, as it does not
 * count the base store.  DCN_ERR_ARG for an index that is not a map and for a map that keeps no bases.  Enabling again
 * changes nothing; enable = 0 frees.  While a pileup is enabled dcn_anchor_map_add on that map is DCN_ERR_ARG (a pileup
 * does not grow); a map without one behaves exactly as before in every call.  dcn_index_clone gives an index without the
 * pileup, dcn_index_destroy frees it.  dcn_anchor_map_pileup_reset zeroes every counter. */
int dcn_anchor_map_pileup_enable(dcn_index *map, int enable);
int dcn_anchor_map_pileup_reset(dcn_index *map);

/*   ctx .. n_rows   as for dcn_verify_batch: the same checks in the same order with the same messages and row numbers
 *   edits           n_rows entries: exactly what dcn_verify_batch returns
 *   n_added         may be NULL: the number of rows that added, by P2
 * DCN_ERR_ARG beyond dcn_verify_batch's: a map with no pileup enabled; dcn_align_batch's rules on a row with
 * max(m, n) >= 2^28 and on more than 2^32 - 1 rows.  Any DCN_ERR_ARG leaves the counters untouched.  Host pointers,
 * blocking, refused while batches are in flight; the six counters of the context are left unchanged.  One call at a time
 * per map: overlapping calls on one map (from two contexts) are not supported.
 * The call runs dcn_align_batch's passes: verify, the align kernel of every trace group (DCN_ALIGN_TRACE_BYTES applies as
 * it does there), the scan of the run counts and the gather.  The runs stay on the device, in a buffer of the context
 * that grows to the size the scan reports (no capacity protocol); then the pileup kernel walks them, one wave per aligned
 * row, and adds with atomic adds on the map's counters.  Device memory: dcn_align_batch's.
 * dcn_ctx_set_profiling covers it: pack in its slot, everything else in FINISH; plan, scan and DISTINCT are empty. */
int dcn_pileup_batch(dcn_ctx *ctx, dcn_index *map, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                     const void *params, const uint64_t *row_offsets, const void *rows, uint64_t n_rows, uint32_t *edits,
                     uint64_t *n_added);

/* The counters of positions [start, start + n_bases) of a record, position-major: counts[8 q + column] belongs to
 * position start + q (on the device they lie column by column; the call transposes).  Blocking.  Errors as for
 * dcn_anchor_map_fetch, and DCN_ERR_ARG for a map with no pileup enabled.  n_bases = 0 succeeds. */
int dcn_anchor_map_pileup_fetch(const dcn_index *map, uint32_t record, uint64_t start, uint64_t n_bases, uint32_t *counts);

/* Rule P6 over positions [start, start + n_bases) of a record.
 *   params      a dcn_pileup_call_params (declared void * for the reason given at dcn_locate_batch); reserved != 0 or
 *               min_permille > 1000 is DCN_ERR_ARG
 *   calls       NULL, or n_bases characters of ACGT-N
 *   site_pos    the sites in ascending position, record-relative and 0-based; site_info as P6 packs it
 *   capacity    entries of site_pos and of site_info
 *   n_sites     always receives the number of sites there is
 * DCN_ERR_CAPACITY when capacity is smaller: calls is complete and no site is written; NULLs with capacity 0 ask for the
 * count (dcn_locate_batch's convention: call again with that capacity).  Range errors as for dcn_anchor_map_fetch.
 * Blocking; one thread per position, a scan of the per-workgroup site counts, and a second pass that writes the sites. */
int dcn_anchor_map_pileup_call(const dcn_index *map, const void *params, uint32_t record, uint64_t start, uint64_t n_bases,
                               uint8_t *calls, uint64_t *site_pos, uint32_t *site_info, uint64_t capacity, uint64_t *n_sites);

/* ---- insertion ledger: the inserted bases beside a pileup, insertion alleles (ABI 1.17) --------------------------------
 * (no reference counterpart.)  The INS column of a pileup says that an insertion sits at a base, not what it is.  A ledger
 * keeps every insertion's bases, so that the sequence the reads support can be written out.
 *
 * THE DEFINITION OF AN INSERTION LEDGER.  Rules 1-6 of a verified placement, A1-A6 and P1-P6 stand.  Added:
 *   L1. A map with a pileup enabled may keep an insertion ledger: a multiset of events, empty when switched on.  Switching
 *       it on is DCN_ERR_ARG once any row has added to the pileup (P2) since the pileup was enabled or last reset, so the
 *       ledger and the INS column always describe the same rows.
 *   L2. While the ledger is kept, every I run that P3 counts in INS also appends one event (p, front, len, bases, reverse):
 *         p is the position P3 adds to: ref_start + j - 1, or ref_start when j = 0;
 *         front is 1 exactly in the j = 0 case: the run then lies in front of p, not behind it;
 *         len is the run's length;
 *         bases are S[i .. i + len) as upper-case ASCII A C G T, with N for an invalid base (S is already
 *           reverse-complemented on a reverse row: the bases are in the record's direction);
 *         reverse is the row's strand.
 *       Hence at every position the number of events equals INS, while no counter has wrapped.
 *   L3. Events commute: the ledger depends on the multiset of rows added, not on how batches are cut, on align's trace
 *       groups, on lanes or on order.
 *   L4. The canonical order, used wherever events are returned: ascending p; then front 0 before 1; then the shorter len;
 *       then bases as bytes (so A < C < G < N < T); then reverse 0 before 1.  Equal events are indistinguishable, so the
 *       output is fully determined.
 *   L5. An ALLELE at p is a class of events equal in (front, len, bases); its count is the size of the class.  The WINNER
 *       is the allele with the largest count; ties go to the allele that comes first in L4's order.
 *   L6. With P6's parameters, position p HAS A CALLED INSERTION when P6 sets DCN_PILEUP_SITE_INS there and INS > 0 (which
 *       matters at min_permille = 0, where P6 flags every deep position).  The call is the winner, reported with its count
 *       and with events = INS(p).  The winner's own count is not thresholded: the caller has both numbers.
 *   L7. The consensus of a range, position by position: the bases of a called insertion with front = 1 there; then the
 *       base P6 calls, nothing when P6 calls '-', and fill(p) when the position is not called (N, or with "fill from the
 *       reference" the record's own base in upper case, N for an invalid one); then the bases of a called insertion with
 *       front = 0.  An insertion applies whether or not the position itself is called or deleted.
 *   L8. Integers and bytes only.  The result is unique.
 * The winner of a position is found by counting every event of the position against every other: quadratic in the events
 * of ONE position, which is fine at the depths the pileup is measured at and unmeasured beyond. */
#define DCN_INSERTION_FRONT 1u
#define DCN_INSERTION_REVERSE 2u
typedef struct dcn_insertion {
    uint64_t pos;          /* record-relative, 0-based */
    uint64_t bases_offset; /* into the bases array of the same call */
    uint32_t len;
    uint32_t flags;        /* DCN_INSERTION_FRONT, DCN_INSERTION_REVERSE */
} dcn_insertion;           /* 24 bytes */
typedef struct dcn_insertion_allele {
    uint64_t pos, bases_offset;
    uint32_t len, count, events, flags; /* flags: DCN_INSERTION_FRONT only */
} dcn_insertion_allele;                 /* 32 bytes */

/* keep != 0 switches the ledger on (L1; keeping again changes nothing), keep = 0 drops it and leaves the counters.
 * DCN_ERR_ARG for a map without a pileup, and by rule L1; dcn_anchor_map_pileup_reset also empties a kept ledger,
 * dcn_anchor_map_pileup_enable(map, 0) also frees it, dcn_index_clone gives an index without it, dcn_index_memory does not
 * count it.  On a map that keeps a ledger dcn_pileup_batch also appends, in the same call and behind the same checks (any
 * DCN_ERR_ARG leaves the counters and the ledger untouched): a counting pass over the aligned rows, one read-back of the
 * two totals, and only when there is an I run the two scans, the growth of the ledger (geometric, from
 * DCN_INSERTION_LEDGER_EVENTS events, read when the ledger first grows) and the writing pass.  A map on which no ledger is
 * kept behaves byte for byte as before; with one, the eight counters are exactly what they were.  Blocking. */
int dcn_anchor_map_pileup_keep_insertions(dcn_index *map, int keep);
/* the events of the ledger and the sum of their lengths (either pointer may be NULL).  Blocking. */
int dcn_anchor_map_insertions_info(const dcn_index *map, uint64_t *n_events, uint64_t *n_bases);

/* The events anchored in [start, start + n_bases) of a record, in L4's order, with bases_offset ascending and dense.
 *   events      dcn_insertion entries (declared void * for the reason given at dcn_locate_batch), event_capacity of them
 *   bases       base_capacity bytes
 *   n_events, n_inserted   always receive the number of events and the sum of their lengths
 * DCN_ERR_CAPACITY when either capacity is too small: nothing else is written then; NULLs with capacity 0 ask for the
 * sizes.  Range errors as for dcn_anchor_map_fetch; DCN_ERR_ARG for a map that keeps no ledger and for a range with 2^32
 * events or more.  Blocking: the INS plane of the range, its scan, a pass over the whole ledger that scatters the events
 * of the range into their positions' buckets, a gather, and a sort of each bucket on the host. */
int dcn_anchor_map_insertions_fetch(const dcn_index *map, uint32_t record, uint64_t start, uint64_t n_bases, void *events,
                                    uint64_t event_capacity, uint8_t *bases, uint64_t base_capacity, uint64_t *n_events,
                                    uint64_t *n_inserted);

/* Rule L6 over [start, start + n_bases) of a record: one dcn_insertion_allele per position with a called insertion, in
 * ascending pos, under the same capacity protocol.  params is a dcn_pileup_call_params, with the checks, the order and the
 * messages of dcn_anchor_map_pileup_call.  Blocking. */
int dcn_anchor_map_insertions_call(const dcn_index *map, const void *params, uint32_t record, uint64_t start, uint64_t n_bases,
                                   void *alleles, uint64_t allele_capacity, uint8_t *bases, uint64_t base_capacity,
                                   uint64_t *n_alleles, uint64_t *n_inserted);

/* ---- quality-aware pileup: base qualities, low-quality bases as N, quality sums (ABI 1.18) -----------------------------
 * (no reference counterpart.)  dcn_pileup_batch counts every base of a read alike.  With the quality line of a FASTQ record
 * a base the sequencer doubted can be kept out of the base columns, and the sums say how good the bases of a column were.
 *
 * THE DEFINITION OF A QUALITY-AWARE PILEUP.  Rules 1-6 of a verified placement, A1-A6, P1-P6 and L1-L8 stand.  Added:
 *   Q1. A map with a pileup enabled may keep quality sums: four more uint32_t per kept base, the columns QA QC QG QT, all
 *       zero when switched on.  Switching them on is DCN_ERR_ARG once a row has added since the pileup was enabled or last
 *       reset (L1's rule), so the sums and the counters always describe the same rows; for the same reason
 *       dcn_pileup_batch, whose rows have no qualities, is DCN_ERR_ARG on a map that keeps sums.
 *   Q2. dcn_pileup_batch_qual takes quals: one byte per base of the batch, parallel to bases; quals[offsets[r] + x]
 *       belongs to bases[offsets[r] + x].  The quality of a base is q = byte >= qual_offset ? byte - qual_offset : 0, so
 *       0 .. 255; a byte below the offset is no error, and the host does not look at the bytes.  On a forward row S[i] is
 *       the batch base at s_origin + i; on a reverse row it is the complement of the batch base at s_origin - 1 - i (s_origin
 *       being the first base of the read interval, or its end when reverse).  q(S[i]) is the quality at that same batch
 *       position: qualities are not complemented.
 *   Q3. An '=' or X step at (i, j) whose column by P3 is A, C, G or T adds to N instead when q(S[i]) < min_base_qual.  A
 *       base that is N by P3 stays N.  REV, D steps and I runs are exactly P3's, so P4 holds unchanged.  With
 *       min_base_qual = 0 the eight counters equal dcn_pileup_batch's for the same rows.
 *   Q4. On a map that keeps sums, every step that adds to column c of A, C, G, T also adds q(S[i]) to Qc at that position.
 *       A sum wraps above 2^32 - 1.
 *   Q5. An insertion ledger receives the same events as from dcn_pileup_batch: qualities do not touch inserted bases.
 *   Q6. Integers only.  Adds commute: counters and sums depend only on the multiset of (row, its qualities).  edits are
 *       dcn_verify_batch's: the call never changes what aligns.  P6, L6 and L7 are unchanged: they read the counters and do
 *       not care how those were made. */
typedef struct dcn_pileup_qual_params {
    uint32_t qual_offset;   /* 0 .. 255; 33 for FASTQ */
    uint32_t min_base_qual; /* 0 .. 255 */
    uint32_t reserved[2];   /* must be 0 */
} dcn_pileup_qual_params;   /* 16 bytes */

/* keep != 0 switches the sums on (Q1; keeping again changes nothing): 16 bytes of device memory per base of the pileup,
 * allocated and zeroed here; keep = 0 frees them and leaves the counters.  DCN_ERR_ARG for a map without a pileup, and by
 * rule Q1; dcn_anchor_map_pileup_reset zeroes the sums too, dcn_anchor_map_pileup_enable(map, 0) also frees them,
 * dcn_index_clone gives an index without them, dcn_index_memory does not count them. */
int dcn_anchor_map_pileup_keep_qualities(dcn_index *map, int keep);

/* dcn_pileup_batch under rules Q2 to Q6: its checks come first, in their order and with their messages; then
 *   qual_params   a dcn_pileup_qual_params (declared void * for the reason given at dcn_locate_batch): NULL, reserved != 0,
 *                 qual_offset > 255 and min_base_qual > 255 are DCN_ERR_ARG
 *   quals         NULL is DCN_ERR_ARG when there is anything to run
 * Any DCN_ERR_ARG leaves the counters, the sums and a kept ledger untouched.  A map that keeps no sums takes the call as
 * well: rule Q3 alone then.  The call runs dcn_pileup_batch's passes; the qualities go to a buffer of the context of one
 * byte per base of the largest such batch, copied in front of the pileup kernel, whose lanes load one byte per '=' / X base
 * and add a second time where sums are kept.  dcn_ctx_set_profiling: as dcn_pileup_batch, the copy with FINISH. */
int dcn_pileup_batch_qual(dcn_ctx *ctx, dcn_index *map, const uint8_t *bases, const uint8_t *quals, const uint64_t *offsets,
                          uint32_t n_reads, const void *params, const void *qual_params, const uint64_t *row_offsets,
                          const void *rows, uint64_t n_rows, uint32_t *edits, uint64_t *n_added);

/* The sums of positions [start, start + n_bases) of a record, position-major: sums[4 q + column] belongs to position
 * start + q, the columns being DCN_PILEUP_A .. DCN_PILEUP_T.  Blocking.  Errors as for dcn_anchor_map_pileup_fetch, and
 * DCN_ERR_ARG for a map that keeps no sums. */
int dcn_anchor_map_pileup_fetch_qualities(const dcn_index *map, uint32_t record, uint64_t start, uint64_t n_bases, uint32_t *sums);

/* ---- genotypes: likelihoods from the counters and the quality sums, per position (ABI 1.19) ---------------------------
 * (no reference counterpart.)  Rule P6 calls the single most frequent column: a haploid majority vote that does not say
 * how sure it is.  In phred units a mismatching base of quality q costs q + 10 log10 3, so the sums of rule Q4 together
 * with the counters are the sufficient statistic of the textbook genotype likelihood: no pass over the reads is needed.
 *
 * THE DEFINITION OF A GENOTYPE.  Rules P1-P6, L1-L8 and Q1-Q6 stand.  Added:
 *   G1. Inputs.  A genotype is computed at one position of a map that keeps quality sums (Q1), from two sets of numbers
 *       only: the four base counters n[A..T] and the four sums Q[A..T].  N, DEL, INS and REV do not vote.
 *       D = n[A] + n[C] + n[G] + n[T].
 *   G2. Column cost.  All costs are unsigned 64-bit integers in hundredths of a phred.  M[c] = 100 Q[c] + err_centi n[c]:
 *       the cost of explaining every base of column c as an error.  The default err_centi is 477: 1000 log10 3, rounded.
 *   G3. Genotype costs and order.  Ploidy 2 has ten genotypes x/y, x <= y, in VCF order (index y (y + 1) / 2 + x over
 *       A, C, G, T): AA, AC, CC, AG, CG, GG, AT, CT, GT, TT.
 *         cost(x/x) = the sum of M[c] over c != x.
 *         cost(x/y) = the sum of M[c] over c not in {x, y}, plus het_centi (n[x] + n[y]).  The default het_centi is 301:
 *           1000 log10 2, rounded.
 *       Ploidy 1 has four genotypes A, C, G, T, with cost(x) = the sum of M[c] over c != x.
 *       The cost of a matching base, -10 log10(1 - e), is taken as 0: the stated approximation that makes counts and sums
 *       sufficient.
 *   G4. Best genotype, GQ, PL.  best is the first genotype in G3's order with the smallest cost.  second is the smallest
 *       cost among the others; it may equal the best cost.  GQ = min(99, (second - cost[best]) / 100),
 *       PL[g] = min(255, (cost[g] - cost[best]) / 100): integer quotients both.
 *   G5. QUAL = (cost(ref/ref) - cost[best]) / 100, saturated at 2^32 - 1, where ref/ref is the homozygous genotype of the
 *       record's base (just ref at ploidy 1).  QUAL is 0 where the reference base is invalid.
 *   G6. Called.  A position is CALLED when D >= max(1, min_depth) and GQ >= min_gq.  Its gt byte is the genotype's index
 *       when called and DCN_GENOTYPE_NONE otherwise; its gq byte is GQ either way.
 *   G7. Site.  A position is a SITE when it is called, the reference base is valid, best is not ref/ref and
 *       QUAL >= min_qual.
 *   G8. Integers only.  The result is a function of the twelve numbers (the counters, the sums, the reference base and
 *       P4's depth, which a site only reports) and the parameters, unique while no counter or sum has wrapped.
 *       min_depth = 3, min_gq = 20, min_qual = 20, err_centi = 477 and het_centi = 301 are conventions of the layers
 *       above, not measured optima. */
#define DCN_GENOTYPE_NONE 255u
typedef struct dcn_genotype_params {
    uint32_t ploidy;      /* 1 or 2 */
    uint32_t min_depth;
    uint32_t min_gq;      /* 0 .. 99 */
    uint32_t min_qual;
    uint32_t err_centi;   /* 0 .. 100000, so that every cost fits 64 bits */
    uint32_t het_centi;   /* 0 .. 100000 */
    uint32_t reserved[2]; /* must be 0 */
} dcn_genotype_params;    /* 32 bytes */
typedef struct dcn_genotype_site {
    uint64_t pos;         /* record-relative, 0-based */
    uint32_t qual;        /* G5 */
    uint32_t depth;       /* P4's depth: all six columns */
    uint32_t ad[4];       /* n[A..T] */
    uint8_t gt, gq;
    uint8_t ref_code;     /* 0 .. 3 */
    uint8_t reserved0;
    uint8_t pl[10];       /* G3's order; the entries past the ploidy's genotypes are 0 */
    uint8_t reserved1[2];
} dcn_genotype_site;      /* 48 bytes */

/* Rules G1-G8 over positions [start, start + n_bases) of a record.
 *   params      a dcn_genotype_params (declared void * for the reason given at dcn_locate_batch): NULL, reserved != 0,
 *               a ploidy other than 1 or 2, min_gq > 99, err_centi or het_centi above 100000 are DCN_ERR_ARG, in this order
 *   gt, gq      each NULL, or n_bases bytes (G6)
 *   sites       dcn_genotype_site entries in ascending position (declared void * likewise), capacity of them
 *   n_sites     always receives the number of sites there is
 * DCN_ERR_ARG then for a map without a pileup and for one that keeps no quality sums; range errors as for
 * dcn_anchor_map_fetch.  n_bases = 0 succeeds.  DCN_ERR_CAPACITY when capacity is smaller: gt and gq are complete and no
 * site is written; NULL with capacity 0 asks for the count (dcn_anchor_map_pileup_call's protocol).
 * Blocking, on the null stream with scratch of the call: a pass that writes gt and gq and counts the sites per workgroup,
 * a scan of those counts, and a second pass that recomputes the costs and writes the sites.  The grid is sized by the
 * range (DCN_GRID_CUS does not apply).  No new memory on the map and no pass over reads. */
int dcn_anchor_map_genotype(const dcn_index *map, const void *params, uint32_t record, uint64_t start, uint64_t n_bases,
                            uint8_t *gt, uint8_t *gq, void *sites, uint64_t capacity, uint64_t *n_sites);

/* ---- duplicates: a first-seen key set on the map, kept across batches (ABI 1.20) --------------------------------------
 * (no reference counterpart.)  Rule G2 charges every counted base as an independent observation, and rule P2 leaves to the
 * caller which rows count: "a caller leaves a row out by setting its record to UINT32_MAX".  Copies of one fragment (PCR,
 * optical) are not independent, and what tells them apart from two fragments is where their ends lie.  This is the
 * device-side answer to "has a fragment with these ends been seen before?".
 *
 * THE DEFINITION OF A DUPLICATE.  Rules 1-2 of a verified placement stand for what a row is.  Added:
 *   D1. The set.  An anchor map may keep a DUPLICATE SET: keys, for each key the smallest ordinal of a unit that carried
 *       it, and a counter `seen` of the units handed in.  It is empty with seen = 0 when switched on and after a reset.  It
 *       needs neither kept bases nor a pileup.
 *   D2. Units.  A call hands in the rows of n_reads reads, with row_offsets as in dcn_verify_batch (NULL: row r belongs to
 *       read r).  In single mode unit u is read u.  In paired mode n_reads is even and unit u is reads 2u and 2u + 1.  Unit
 *       u of a call has ordinal seen + u, and after the call seen has grown by the number of units, keyed or not: with one
 *       call per input batch an ordinal is the read's (the pair's) number in the input.
 *   D3. Ends.  The END of a read is taken from its first row with record != UINT32_MAX; a read with no such row has no
 *       end.  With L the read's length from `offsets`:
 *         pos5 = ref_start - read_start on a forward row, ref_end + read_start on a reverse row:
 *       the unclipped 5' coordinate, a signed 64-bit number that may be negative or lie past the record's end.  The end is
 *       (record, reverse, pos5).  With both_ends it also has
 *         pos3 = ref_end + (L - read_end) on a forward row, ref_start - (L - read_end) on a reverse row.
 *       Clips therefore do not matter: (ref_start 100, read_start 0) and (ref_start 105, read_start 5) on one strand are
 *       the same end.
 *   D4. Key.  The key has three parts: the mode bits (paired, both_ends), the number of ends, and the ends.  A single unit
 *       with an end has one end.  A paired unit has the ends of whichever mates have one, two of them sorted ascending as
 *       tuples (record, pos5, reverse[, pos3]): a pair and the same pair with its mates swapped have one key.  A unit with
 *       no end has no key.  Two keys are equal only when every component is equal; keys of different modes or with
 *       different numbers of ends never match.  Comparison is exact: no decision rests on a hash alone.
 *   D5. Duplicate.  After the call's units are in the set, first(u) is the smallest ordinal that carries u's key, over
 *       everything since the last reset, this call included.  Unit u is a DUPLICATE when first(u) is smaller than its own
 *       ordinal.  A unit without a key is never a duplicate, and its first is UINT64_MAX.
 *   D6. Determinism.  First seen wins: a streaming rule, not a best-quality rule.  The flags depend on the order of the
 *       units in the input.  They do not depend on how the input is cut into calls (as long as no pair is cut), on lanes,
 *       on the table's size or on the hash.  Integers only.
 *   D7. Stated limits.  A lone mate is not matched against the ends of pairs.  The orientation is whatever the rows say.
 *       There is no optical-distance rule.  Nothing is read from the bases or the qualities. */
typedef struct dcn_duplicate_params {
    uint32_t row_stride; /* as in dcn_verify_params */
    uint32_t paired;     /* 0 | 1 */
    uint32_t both_ends;  /* 0 | 1 */
    uint32_t reserved;   /* must be 0 */
} dcn_duplicate_params;  /* 16 bytes */

/* Switches the duplicate set of an anchor map on (enable != 0: again changes nothing) or off (0: frees it).  DCN_ERR_ARG
 * for an index that is not a map.  Device memory, which dcn_index_memory does not count, from the first call that hands
 * units in: 48 bytes per unit handed in since the last reset (the key log, growing geometrically) and 8 bytes per slot of
 * a table that keeps at least two slots per key and doubles (a power of two; the test hook DCN_DUPLICATE_TABLE_SLOTS, read
 * when the set first grows, sets the capacity it starts with, 2^20 otherwise), and 40 bytes per read plus 9 per unit of the
 * largest call.  dcn_index_clone gives an index without the set, dcn_index_destroy frees it; dcn_anchor_map_add stays
 * allowed while a set is kept. */
int dcn_anchor_map_duplicates_enable(dcn_index *map, int enable);
/* Empties the set and puts seen back to 0; the memory stays.  DCN_ERR_ARG for a map without a set. */
int dcn_anchor_map_duplicates_reset(dcn_index *map);
/* seen: units handed in since the last reset; keyed: those with a key; keys: the distinct keys.  The number of duplicates
 * so far is keyed - keys.  Any pointer may be NULL.  DCN_ERR_ARG for a map without a set.  No device work. */
int dcn_anchor_map_duplicates_info(const dcn_index *map, uint64_t *seen, uint64_t *keyed, uint64_t *keys);
/* Rules D1-D7 over the rows of n_reads reads.
 *   offsets       n_reads + 1 entries, as in dcn_verify_batch: only the reads' lengths are taken from them (no bases)
 *   params        a dcn_duplicate_params (declared void * for the reason given at dcn_locate_batch)
 *   row_offsets, rows, n_rows   as in dcn_verify_batch; only the 48 bytes at the head of a row are read
 *   dup, first    each NULL, or one entry per unit (n_reads units, n_reads / 2 in paired mode): D5's flag (0 | 1) and first
 *   n_duplicates  NULL, or receives the number of duplicates among the call's units
 * DCN_ERR_ARG, before any device work and with the set and seen untouched: params NULL, reserved != 0, paired > 1,
 * both_ends > 1, then dcn_verify_batch's checks in its order and with its messages (row_stride; the map, which here must be
 * an anchor map with a duplicate set and need not keep bases; n_rows against n_reads -- and here an odd n_reads in paired
 * mode; offsets; row_offsets; rows; then every placed row, the message naming the first wrong one).  A map that keeps no
 * bases knows no record lengths: ref_end is then checked against nothing.  Host pointers, blocking, on the null stream;
 * one call at a time per map.  Three kernels, one thread per unit, grids sized by the batch (DCN_GRID_CUS does not apply):
 * the keys into the log, the insert, the lookup; in front of them the table grows, by a rehash kernel, so that it has at
 * least 2 * (keys + units of the call) slots. */
int dcn_mark_duplicates_batch(dcn_index *map, const uint64_t *offsets, uint32_t n_reads, const void *params,
                              const uint64_t *row_offsets, const void *rows, uint64_t n_rows, uint8_t *dup, uint64_t *first,
                              uint64_t *n_duplicates);

/* ---- indels: a deletion ledger beside the pileup, genotypes of insertions and deletions (ABI 1.21) --------------------
 * (no reference counterpart.)  The DEL column of a pileup says that a position is deleted in some reads, not which runs the
 * reads carry: three reads with a 2-base deletion at 100 look like one read with a 3-base deletion at 100 under two reads
 * with a 1-base deletion at 101.  A deletion ledger keeps every run, and with it and the insertion ledger an indel allele
 * can be given a genotype against everything else, as rule G4 gives one to a base.
 *
 * THE DEFINITION OF A DELETION LEDGER.  Rules 1-6 of a verified placement, A1-A6, P1-P6 and L1-L8 stand.  Added:
 *   R1. A map with a pileup enabled may keep a deletion ledger: a multiset of events, empty when switched on.  Switching it
 *       on is DCN_ERR_ARG once a row has added since the pileup was enabled or last reset (L1's rule), so the ledger and the
 *       DEL column always describe the same rows.  It is independent of the insertion ledger and of the quality sums.
 *   R2. While the ledger is kept, every D run of a row that adds (P2) appends one event (p, len, reverse):
 *         p = ref_start + j is the position of the run's first D step;
 *         len is the run's length (runs are maximal, by A4);
 *         reverse is the row's strand.
 *       Hence, while no counter has wrapped, DEL(q) equals the number of events with p <= q < p + len at every position q,
 *       and the sum of all len is the DEL column's total.  A D run may be the first or the last run of a row.
 *   R3. Events commute, as in L3: the ledger depends on the multiset of rows added, not on how batches are cut, on align's
 *       trace groups, on lanes or on order.
 *   R4. The canonical order, used wherever events are returned: ascending p; then the shorter len; then reverse 0 before 1.
 *   R5. STARTS(p) is the number of events with that p.  An ALLELE at p is the class of its events with one len; its count
 *       is the size of the class.  The WINNER is the allele with the largest count; ties go to the shorter.
 *   R6. Integers only.  The result is unique.
 *
 * THE DEFINITION OF AN INDEL GENOTYPE.  Rules P1-P6, L1-L8, R1-R6 and G4 stand.  Added:
 *   I1. Candidates.  At position p the insertion candidate is L5's winner, with a = its count and e = INS(p); it exists when
 *       the map keeps an insertion ledger and INS(p) > 0 (L6's thresholds do not apply here).  The deletion candidate is
 *       R5's winner, with a = its count and e = STARTS(p); it exists when the map keeps a deletion ledger and STARTS(p) > 0.
 *       A candidate with a < max(1, min_count) is dropped.  A position has at most two candidates.
 *   I2. Depth.  depth is P4's depth(p), and o = depth >= a ? depth - a : 0.  A row carries one allele at most once at one p,
 *       and it adds exactly one of columns 0-5 at p, so a <= depth while nothing has wrapped.  Reads that carry another
 *       allele count in o; so do reads with a D at p that began earlier.
 *   I3. Costs, in unsigned 64-bit hundredths of a phred.  Ploidy 2, in VCF order R/R, R/V, V/V:
 *         indel_centi a,  het_centi (a + o),  indel_centi o.
 *       Ploidy 1, R then V: indel_centi a, indel_centi o.  indel_centi is what one read that contradicts the genotype
 *       costs: a gap has no base quality, so it is a constant.
 *   I4. The best genotype, GQ and PL[0 .. 3) follow G4: the first genotype in I3's order with the smallest cost is best, GQ
 *       is capped at 99 and PL at 255, both by integer quotients.  QUAL = (cost(R/R) - cost[best]) / 100, saturated at
 *       2^32 - 1 (cost(R) at ploidy 1).
 *   I5. A candidate is CALLED when depth >= max(1, min_depth) and GQ >= min_gq.  It is a SITE when it is called, best is
 *       not R/R (R at ploidy 1) and QUAL >= min_qual.
 *   I6. Sites come in ascending pos.  At one pos the order is a front insertion (L2), then the deletion, then an insertion
 *       behind.
 *   I7. Stated limits.  One candidate per kind and position: there are no multi-allelic indel records.  Overlapping
 *       deletions with different starts are independent sites.  The position is where A3 puts the gap: A3 takes an edit as
 *       soon as one is available when it walks back from the end, so in a repeat the gap lies at the repeat's far end in
 *       the record's direction.  Both strands agree on that, since T is always forward.  VCF's convention is the near end;
 *       this is not normalised here.
 *   I8. Integers only; a function of the counters, the two ledgers and the parameters.  indel_centi = 2000, min_count = 2
 *       and the defaults shared with G8 are conventions, not measured optima. */
#define DCN_DELETION_REVERSE 1u
typedef struct dcn_deletion {
    uint64_t pos;   /* record-relative, 0-based: R2's p */
    uint32_t len;
    uint32_t flags; /* DCN_DELETION_REVERSE */
} dcn_deletion;     /* 16 bytes */
#define DCN_INDEL_DELETION 1u
#define DCN_INDEL_FRONT 2u /* an insertion in front of pos (L2) */
typedef struct dcn_indel_params {
    uint32_t ploidy;      /* 1 or 2 */
    uint32_t min_depth;
    uint32_t min_gq;      /* 0 .. 99 */
    uint32_t min_qual;
    uint32_t min_count;
    uint32_t indel_centi; /* 0 .. 100000 */
    uint32_t het_centi;   /* 0 .. 100000 */
    uint32_t reserved;    /* must be 0 */
} dcn_indel_params;       /* 32 bytes */
typedef struct dcn_indel_site {
    uint64_t pos;          /* record-relative, 0-based */
    uint64_t bases_offset; /* into the bases array of the same call */
    uint32_t len;          /* inserted or deleted bases */
    uint32_t flags;        /* DCN_INDEL_DELETION, DCN_INDEL_FRONT */
    uint32_t qual;         /* I4 */
    uint32_t depth;        /* P4's depth */
    uint32_t count;        /* a */
    uint32_t events;       /* e */
    uint8_t gt;            /* the best genotype's index in I3's order */
    uint8_t gq;
    uint8_t pl[3];         /* I3's order; pl[2] is 0 at ploidy 1 */
    uint8_t reserved[3];
} dcn_indel_site;          /* 48 bytes */

/* The twin of dcn_anchor_map_pileup_keep_insertions.  keep != 0 switches the deletion ledger on (R1; keeping again changes
 * nothing), keep = 0 drops it and leaves the counters.  DCN_ERR_ARG for a map without a pileup, and by rule R1;
 * dcn_anchor_map_pileup_reset also empties a kept ledger, dcn_anchor_map_pileup_enable(map, 0) and dcn_index_destroy free it,
 * dcn_index_clone gives an index without it, dcn_index_memory does not count it.  On a map that keeps one, dcn_pileup_batch
 * and dcn_pileup_batch_qual also append, in the same call and behind the same checks (any DCN_ERR_ARG leaves counters and
 * ledgers untouched), on the context's stream and accounted in FINISH: a counting pass over the aligned rows, one read-back
 * of the totals, and only when there is a D run the scan, the growth of the ledger (16 bytes per event, geometric from
 * DCN_DELETION_LEDGER_EVENTS events, 2^20 by default, read when the ledger first grows) and the writing pass.  A map on
 * which no deletion ledger is kept behaves byte for byte as before; with one, the eight counters, the quality sums and the
 * insertion ledger are exactly what they were.  Blocking. */
int dcn_anchor_map_pileup_keep_deletions(dcn_index *map, int keep);
/* the events of the ledger and the sum of their lengths (either pointer may be NULL).  No device work.  DCN_ERR_ARG for a
 * map that keeps no deletion ledger. */
int dcn_anchor_map_deletions_info(const dcn_index *map, uint64_t *n_events, uint64_t *n_deleted);

/* The events with p in [start, start + n_bases) of a record, in R4's order.  An event belongs to the range by its p alone,
 * even when its run leaves the range.
 *   events      dcn_deletion entries (declared void * for the reason given at dcn_locate_batch), capacity of them
 *   n_events    always receives the number of events there is
 * DCN_ERR_CAPACITY when capacity is smaller: nothing else is written then; NULL with capacity 0 asks for the size.  Range
 * errors as for dcn_anchor_map_fetch; DCN_ERR_ARG for a map that keeps no deletion ledger and for a range with 2^32 events
 * or more.  Blocking: a pass over the whole ledger that counts the events of the range per position (no pileup column holds
 * STARTS), the scan, a second pass that scatters them into their positions' buckets, a gather, and a sort of each bucket
 * on the host. */
int dcn_anchor_map_deletions_fetch(const dcn_index *map, uint32_t record, uint64_t start, uint64_t n_bases, void *events,
                                   uint64_t capacity, uint64_t *n_events);

/* Rules I1-I8 over positions [start, start + n_bases) of a record.
 *   params      a dcn_indel_params (declared void * likewise): NULL, reserved != 0, a ploidy other than 1 or 2, min_gq > 99,
 *               indel_centi or het_centi above 100000 are DCN_ERR_ARG, in this order
 *   sites       dcn_indel_site entries in I6's order (declared void * likewise), site_capacity of them
 *   bases       base_capacity bytes: the inserted bases of the insertion sites.  bases_offset is ascending and dense; a
 *               deletion site has len = the deleted length and bases_offset = the offset reached so far
 *   n_sites, n_inserted   always receive the number of sites and the sum of the insertion sites' lengths
 * DCN_ERR_ARG then for n_sites / n_inserted NULL, for a map without a pileup and for one that keeps neither ledger (one is
 * enough: the other kind then has no candidates); then the range errors of dcn_anchor_map_fetch.  Quality sums are not
 * needed.  DCN_ERR_CAPACITY when either capacity is too small: nothing else is written then; NULLs with capacity 0 ask for
 * the sizes (dcn_anchor_map_insertions_call's protocol).  Blocking, on the null stream with scratch of the call, no memory
 * on the map: the insertion side is dcn_anchor_map_insertions_call's buckets and winner kernel with "INS > 0" as the flag,
 * the deletion side dcn_anchor_map_deletions_fetch's buckets and a winner by len; then one thread per position counts its
 * sites, a scan of the per-workgroup counts, a second pass that decides again and writes the sites, the scan of the
 * insertion sites' lengths and the copy of their bases. */
int dcn_anchor_map_indels_genotype(const dcn_index *map, const void *params, uint32_t record, uint64_t start, uint64_t n_bases,
                                   void *sites, uint64_t site_capacity, uint8_t *bases, uint64_t base_capacity, uint64_t *n_sites,
                                   uint64_t *n_inserted);

/* ---- left-aligned placements: the gaps of an alignment at a repeat's near end (ABI 1.22) -------------------------------
 * (no reference counterpart.)  A3 leaves a gap at the far end of a repeat (I7); VCF's convention is the near end.
 *
 * THE DEFINITION OF A LEFT-ALIGNED PLACEMENT.  Rules 1-6 of a verified placement and A1-A6 of an aligned placement stand.
 * Read the alignment column by column: an '=' or X column pairs S[i] with T[j], an I column is S[i] alone, a D column is
 * T[j] alone.  Added:
 *   N1. A GAP is a maximal run of I or of D.  The gaps are taken in order from the start of both intervals.  A gap is final
 *       before the next one is looked at.
 *   N2. One STEP for a D gap over T[j, j+len), where the column in front pairs S[x] with T[j-1] and is an '=' or X column:
 *       the step is allowed if T[j-1] EQUAL T[j+len-1] by rule 2 (an invalid base equals nothing, so such a column is never
 *       passed), and not if that column is the row's first column.  After the step the gap covers T[j-1, j+len-1); the
 *       column follows the gap, pairs S[x] with T[j+len-1] and keeps its op.
 *   N3. One step for an I gap over S[i, i+len), where the column in front pairs S[i-1] with T[y]: allowed if S[i-1] EQUAL
 *       S[i+len-1] and the column is not the row's first.  After the step the gap covers S[i-1, i+len-1); the column
 *       follows the gap, pairs S[i+len-1] with T[y] and keeps its op.  S is the reverse complement when the row says so
 *       (A5): the comparison is on S as aligned.
 *   N4. A gap takes steps until none is allowed.  If it comes to lie directly behind an earlier gap of the same kind, the
 *       two become one gap, which goes on taking steps with its new length.  A gap directly behind a gap of the other kind
 *       stops (this cannot arise from an A3 alignment, where an I next to a D costs more than an X, and N2 / N3 preserve
 *       the cost: the rule is stated so that the definition is total).  A gap that A3 put first in the row stays first, and
 *       no step makes a gap first.
 *   N5. Afterwards equal neighbouring ops merge into runs, as in A4.  The result has the same multiset of column ops and
 *       the same d, so it is still an optimal alignment; '=' + X + I covers m, '=' + X + D covers n, and n_ops <= 2 d + 1
 *       still holds.  n_ops may be larger or smaller than before.  A row without a gap is unchanged.
 *   N6. The procedure is idempotent and its result unique.  It depends only on S, T and A3's ops: not on lanes, chunking,
 *       trace groups or how a batch is cut.  Integers only.
 *   N7. Stated limits.  A row that begins inside a repeat cannot carry its gap past its own first column: such rows report
 *       the gap further right than rows that cover the repeat (the mirror of I7's limit at the far end).  An insertion in
 *       front of which the read has an X column is stopped by the read's base, not by the record's: its VCF line can
 *       therefore still end in the anchor's base.
 *   N8. A map's pileup either left-aligns every row that adds to it or none: dcn_anchor_map_pileup_left_align changes the
 *       switch only while no row has added since the pileup was enabled or reset (Q1's spirit).
 * The totals count, over the rows of a call: ROWS CHANGED, the rows in which a gap took a step; GAPS SHIFTED, the gaps of
 * A3's alignment that took at least one step, a gap that merged into an earlier one counting for itself; COLUMNS PASSED, the
 * steps of all gaps; GAPS MERGED, the times two gaps became one. */
typedef struct dcn_left_align_info {
    uint64_t rows_aligned;   /* the rows with an alignment (A1) */
    uint64_t rows_changed;
    uint64_t gaps_shifted;
    uint64_t columns_passed;
    uint64_t gaps_merged;
} dcn_left_align_info;       /* 40 bytes */

/* dcn_align_batch with rules N1-N7 applied to every aligned row: the arguments, the checks, their order, their messages
 * and row numbers, and the capacity protocol are dcn_align_batch's.  edits is identical; cigar_offsets and cigar are those
 * of N5 (cigar_offsets[n_rows] is the size needed, counted behind the left alignment).
 *   info   a dcn_left_align_info (declared void * for the reason given at dcn_locate_batch), or NULL; it is zeroed first
 *          and complete whenever cigar_offsets is (DCN_ERR_CAPACITY included)
 * One kernel more than dcn_align_batch, behind the align kernel of the last trace group and in front of the scan of the run
 * counts, accounted in FINISH: a wave per aligned row, which reads the row's runs once and does nothing more when none is
 * a gap.  Device memory beyond dcn_align_batch's, freed with the context: a second array of run slots (4 (2 d + 1) bytes
 * per aligned row of the largest call) and 32 bytes. */
int dcn_left_align_batch(dcn_ctx *ctx, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                         const void *params, const uint64_t *row_offsets, const void *rows, uint64_t n_rows, uint32_t *edits,
                         uint64_t *cigar_offsets, uint32_t *cigar, uint64_t capacity, void *info);

/* Rule N8's switch.  While it is on, dcn_pileup_batch and dcn_pileup_batch_qual pile up the runs of N5 and append N5's
 * events to both ledgers: counters, quality sums and ledgers are those of a caller who had handed in left-aligned
 * alignments.  on != 0 sets it, on = 0 clears it; setting it to what it is changes nothing and always succeeds.
 * DCN_ERR_ARG for a map without a pileup, and when rows have added since the pileup was enabled or reset (the message names
 * dcn_anchor_map_pileup_reset).  dcn_anchor_map_pileup_enable(map, 0) clears it; dcn_anchor_map_pileup_reset keeps it and
 * zeroes the totals.  A map that never sets it behaves exactly as before in every call: not one launch or copy more. */
int dcn_anchor_map_pileup_left_align(dcn_index *map, int on);
/* A dcn_left_align_info (declared void * likewise) summed over the map's pileup calls that ran with the switch on, since
 * the pileup was enabled or reset.  No device work.  DCN_ERR_ARG for a map without a pileup, then for info NULL. */
int dcn_anchor_map_pileup_left_align_info(const dcn_index *map, void *info);

/* ---- strand evidence: per-allele reverse counts, a bias score and two flags (ABI 1.23) ---------------------------------
 * (no reference counterpart.)  The REV column says how many reverse rows covered a base, not which allele they showed, and
 * rule G1 keeps it out of the vote.  A heterozygote seen on both strands and an artefact carried by reads of one
 * orientation look alike in the counters.  Four more planes tell them apart; the two ledgers already carry each event's
 * strand.
 *
 * THE DEFINITION OF STRAND EVIDENCE.  Rules P1-P6, Q1-Q6, L1-L8, R1-R6, G1-G8 and I1-I8 stand.  Added:
 *   S1. A map with a pileup may keep STRAND PLANES: four more uint32_t counters per kept base, RA RC RG RT, all zero when
 *       switched on.  They cost 16 bytes per base and are laid out as the counters are, planes of one column each (four
 *       words per position under -DDCN_PILEUP_POSITION_MAJOR).  Switching them on is DCN_ERR_ARG once a row has added
 *       since the pileup was enabled or last reset (L1's rule).  dcn_anchor_map_pileup_reset zeroes them,
 *       dcn_anchor_map_pileup_enable(map, 0) and dcn_index_destroy free them, dcn_index_clone gives an index without them,
 *       dcn_index_memory does not count them.
 *   S2. While the planes are kept, every '=' or X step of a row with reverse = 1 also adds 1 to R[c] at that position,
 *       where c is the column the step is counted in: P3's, or with qualities Q3's.  This applies only when c is one of A,
 *       C, G, T: a base that counts as N (an invalid base, a base under min_base_qual) adds to no plane, and neither do D
 *       and I runs.  Hence R[c] <= n[c] everywhere, F[c] = n[c] - R[c] is the forward count, and
 *       RA + RC + RG + RT <= REV.  The adds commute (P5).  Left alignment (N8) applies first, as to everything counted.
 *   S3. The TABLE of a base site.  Given a position, the record's base ref (valid) and a non-empty set ALT of columns
 *       other than ref:  a = F[ref], b = R[ref], c = the sum of F[x] over x in ALT, d = the same sum of R[x].
 *   S4. The TABLE of an indel site of rule I5, with a_all = its count and a_rev = the number of the winner's events with
 *       reverse = 1:  d = a_rev;  c = a_all - a_rev;  b = REV(p) >= d ? REV(p) - d : 0;
 *       a = (depth - REV(p)) >= c ? depth - REV(p) - c : 0, with depth - REV(p) taken as 0 when depth < REV(p).  So the
 *       first row is "every read there that does not carry the allele", which is what rule I2 calls o.
 *   S5. The SCORE, in integers only, in hundredths of a chi-square with one degree of freedom.  Let m = max(a, b, c, d),
 *       s = 0 when m < 1024 and (the bit length of m) - 10 otherwise.  All four are shifted right by s, so that each is
 *       below 1024 (GATK shrinks large tables the same way before its Fisher test).  N = a + b + c + d, r1 = a + b,
 *       r2 = c + d, c1 = a + c, c2 = b + d.  If r1 r2 c1 c2 = 0 the score is 0.  Otherwise
 *         sb_centi = min(65535, 100 N (ad - bc)^2 / (r1 r2 c1 c2)),
 *       an integer quotient of unsigned 64-bit numbers: N < 2^12 and |ad - bc| < 2^20, so the numerator stays below
 *       2^7 * 2^12 * 2^40 = 2^59, and the denominator below 2^44.
 *   S6. FLAGS.  DCN_STRAND_BIAS when max_sb_centi > 0 and sb_centi >= max_sb_centi.  DCN_STRAND_ONE_SIDED when
 *       min(c, d) < min_alt_strand and both a + c and b + d are at least min_strand_depth: both strands cover the site,
 *       yet the allele is on one.  This flag uses the unshifted table.  A site with no flag passes.
 *   S7. Stated limits.  A hom-alt site has an empty reference row and scores 0.  There is no Yates correction and no exact
 *       test.  Only the winner of each indel kind is counted.  max_sb_centi = 1083 is a convention, not a measured optimum:
 *       chi-square 10.83, p = 0.001 at one degree of freedom.  min_alt_strand = 1 and min_strand_depth = 3 are conventions
 *       too.
 *   S8. The result is unique while no counter has wrapped: a function of the counters, the planes, the ledgers and the
 *       parameters. */
#define DCN_STRAND_BIAS 1u
#define DCN_STRAND_ONE_SIDED 2u
typedef struct dcn_strand_params {
    uint32_t max_sb_centi;     /* 0: the bias flag is off */
    uint32_t min_alt_strand;
    uint32_t min_strand_depth;
    uint32_t reserved;         /* must be 0 */
} dcn_strand_params;           /* 16 bytes */
typedef struct dcn_strand_query {
    uint64_t pos;           /* record-relative, 0-based */
    uint32_t kind;          /* 0 a base site (S3), 1 an indel site (S4) */
    uint32_t ref_code;      /* base: the record's base, 0 .. 3 */
    uint32_t alt_mask;      /* base: ALT, bits 0 .. 3 */
    uint32_t count;         /* indel: a_all */
    uint32_t count_reverse; /* indel: a_rev */
    uint32_t reserved;      /* must be 0 */
} dcn_strand_query;         /* 32 bytes */
typedef struct dcn_strand_site {
    uint32_t fwd[4];      /* base: F[A..T]; indel: 0 */
    uint32_t rev[4];      /* base: R[A..T]; indel: 0 */
    uint32_t table[4];    /* a, b, c, d, unshifted */
    uint32_t sb_centi;    /* S5 */
    uint32_t flags;       /* S6: DCN_STRAND_BIAS, DCN_STRAND_ONE_SIDED */
    uint32_t reserved[2]; /* 0 */
} dcn_strand_site;        /* 64 bytes */

/* The twin of dcn_anchor_map_pileup_keep_deletions for rule S1's planes.  keep != 0 switches them on (keeping again changes
 * nothing): 16 bytes of device memory per base of the pileup, allocated and zeroed here; keep = 0 frees them and leaves the
 * counters.  DCN_ERR_ARG for a map without a pileup, and by rule S1; on a map that keeps planes dcn_pileup_batch and
 * dcn_pileup_batch_qual launch the strand form of the pileup kernel instead of the plain one: the same walk, with one
 * more add per counted base of a reverse row, and not one memory operation more on a forward row.  A map on which the
 * switch is off issues exactly the launches and copies it issued before.  Blocking. */
int dcn_anchor_map_pileup_keep_strands(dcn_index *map, int keep);

/* The planes of positions [start, start + n_bases) of a record, position-major: rev[4 q + column] belongs to position
 * start + q, the columns being DCN_PILEUP_A .. DCN_PILEUP_T.  Blocking.  Errors as for dcn_anchor_map_pileup_fetch, and
 * DCN_ERR_ARG for a map that keeps no planes. */
int dcn_anchor_map_pileup_fetch_strands(const dcn_index *map, uint32_t record, uint64_t start, uint64_t n_bases, uint32_t *rev);

/* Rules S3-S6 at n_queries sites of a record.
 *   params    a dcn_strand_params (declared void * for the reason given at dcn_locate_batch)
 *   queries   dcn_strand_query entries (declared void * likewise), in any order
 *   out       dcn_strand_site entries (declared void * likewise), one per query
 * DCN_ERR_ARG, in this order: params NULL or reserved != 0; a map without a pileup or without planes; a record out of
 * range; then, when n_queries > 0, queries or out NULL; then the first wrong query, with its index in the message: a pos
 * past the record, a kind above 1 (or reserved != 0), a base query with ref_code > 3, an empty alt_mask, bits above 3 in it
 * or ref's bit in it, an indel query with count_reverse > count.  n_queries = 0 succeeds with no device work.  Blocking, on
 * the null stream with scratch of the call: the queries go up, one thread per query gathers the position's counters (and on
 * a base query its four reverse counters) and applies dcn_strand.h's rule, and the sites come back. */
int dcn_anchor_map_strand_evidence(const dcn_index *map, const void *params, uint32_t record, const void *queries, uint64_t n_queries,
                                   void *out);

/* a_rev of rule S4 for the sites that dcn_anchor_map_indels_genotype returned: count_reverse[s] receives the number of
 * events with reverse = 1 among the winning allele of sites[s].
 *   sites, bases   dcn_indel_site entries and the inserted bases, as that call wrote them (sites declared void *)
 * DCN_ERR_ARG for a map without a pileup, a record out of range, sites or count_reverse NULL when n_sites > 0, then for the
 * first wrong site with its index in the message: a pos past the record, sites not in I6's order, an insertion site whose
 * bases_offset is not the sum of the insertion sites' lengths in front of it (and bases NULL then), a site whose kind has no
 * ledger on the map.  It needs no strand planes: the ledgers carry the strand.  n_sites = 0 succeeds with no device work.
 * Blocking, on the null stream with scratch of the call: the sites' keys, lengths and bases go up, then one thread per event
 * of each ledger that has a site finds the site of its (pos, kind, front) by binary search, compares len, and on an
 * insertion the bases, and when it is a reverse event adds 1 atomically.  The winner and site kernels of
 * dcn_anchor_map_indels_genotype are not involved. */
int dcn_anchor_map_indels_strand(const dcn_index *map, uint32_t record, const void *sites, uint64_t n_sites, const uint8_t *bases,
                                 uint32_t *count_reverse);

/* ---- extended placements: each placement carried over the read's flanks, with soft clips (ABI 1.16) -------------------
 * (no reference counterpart.)  A placement's two intervals begin and end on the k-mer of an anchor hit: the read's bases
 * outside the outermost hits are never compared with the reference by the calls above.  dcn_extend_batch grows the
 * interval pair of each row over both flanks as far as the bases support it; what is left of the read is the soft clip.
 * The result is again a row that dcn_verify_batch, dcn_align_batch and dcn_pileup_batch accept as they are.
 *
 * THE DEFINITION OF AN EXTENDED PLACEMENT.  Rules 1-2 of a verified placement stand: S, T, EQUAL, and an invalid base
 * equals nothing.  For a row with record != UINT32_MAX:
 *   X1. Orientation.  L is the read's length.  R' is the read as given, or its reverse complement when the row says
 *       reverse.  S = R'[a, b): forward (a, b) = (read_start, read_end); reverse (a, b) = (L - read_end, L - read_start).
 *       T = record[ref_start, ref_end).  Lr is the record's length.
 *   X2. The two flanks are treated separately and identically.  Right: U = R'[b, L), V = record[ref_end, Lr).  Left: U is
 *       R'[0, a) read backwards, V is record[0, ref_start) read backwards.  f = |U|, g = |V|; either may be 0.  A flank
 *       never reaches into another read of the batch or into another record of the map.
 *   X3. D[i][j] is the Levenshtein distance of U[0, i) and V[0, j) at unit costs, under rule 2's equality.
 *   X4. A cell (i, j) with 0 <= i <= f, 0 <= j <= g and D[i][j] <= max_edits is a candidate.  Its value is
 *       i + j - penalty * D[i][j], plus end_bonus when i = f.  Arithmetic is 64-bit and signed.  (0, 0) is always a
 *       candidate.
 *   X5. The flank's extension is the candidate of largest value; among equals the one with the smaller D, then the one
 *       with the larger i.  This is unique.  Call it (i*, j*, D*).
 *   X6. The extended row: S' = R'[a - i_left, b + i_right), T' = record[ref_start - j_left, ref_end + j_right).  Mapped
 *       back to the read as given: forward read_start' = read_start - i_left, read_end' = read_end + i_right; reverse
 *       read_start' = read_start - i_right, read_end' = read_end + i_left.  left and right are in the record's
 *       direction, as rule A5 has the ops.  The soft clips are what remains: a - i_left bases of R' in front and
 *       L - b - i_right behind.
 *   X7. A row with record == UINT32_MAX comes back with its four coordinates as given and both edit counts 0.
 *   X8. Integers only.  Nothing depends on lanes, LDS sizes, a band, an early stop or how a batch is cut.
 * Consequences, which a kernel may use (they are not rules).  With penalty >= 2 a winning cell has j - i <= D and
 * D <= (2 f + end_bonus) / (penalty - 1).  For a fixed cost s and diagonal k = j - i the best cell is the furthest-reaching
 * one, F_s[k], of the verify kernel's wavefront: so the answer is the maximum of 2 F_s[k] + k - penalty * s over the
 * wavefronts, plus the bonus where F_s[k] = f, ties going first to the smaller s, then to the larger F.  The loop may stop
 * at score s once 2 f + end_bonus - (penalty - 1) (s + 1) <= the best value so far.  A flank that matches to its end is
 * finished at s = 0.
 * penalty = 6, end_bonus = 4 and max_edits = 1023 are the conventions of the layers above, not measured optima. */
typedef struct dcn_extend_params {
    uint32_t penalty;     /* 2 .. 255 */
    uint32_t end_bonus;   /* 0 .. 65535 */
    uint32_t max_edits;   /* 0 .. DCN_VERIFY_MAX_EDITS */
    uint32_t row_stride;  /* as in dcn_verify_params */
    uint32_t reserved[2]; /* must be 0 */
} dcn_extend_params;      /* 24 bytes */

typedef struct dcn_extension {
    uint32_t read_start, read_end;    /* of the read as given */
    uint64_t ref_start, ref_end;
    uint32_t left_edits, right_edits; /* D* of each flank */
} dcn_extension;                      /* 32 bytes */

/*   ctx .. n_rows   as for dcn_verify_batch, with a dcn_extend_params: the same checks of row_offsets and of every placed
 *                   row, in the same order, with the same messages and row numbers
 *   out             n_rows dcn_extension (declared void * for the reason given at dcn_locate_batch)
 * DCN_ERR_ARG, before any device work: what dcn_verify_batch lists, with penalty outside 2 .. 255 and end_bonus above
 * 65535 in place of max_permille, and out is NULL -- which, unlike dcn_verify_batch's edits, is looked at after the rows, so a
 * bad row is named first.  Host pointers, blocking, batch limits as for dcn_place_batch; refused
 * while batches are in flight; the six counters of the context are left unchanged.  The rows are not written: a caller
 * copies the four coordinates of `out` into its rows and hands those to dcn_verify_batch, dcn_align_batch or
 * dcn_pileup_batch.  The batch is staged and packed again (no plan, no scan), so the call may follow any call on the same
 * context.  The host resolves each placed row to two flanks; the kernel runs the wavefront of the verify kernel on each,
 * 16 lanes per flank, and tracks the best candidate.  Device memory, freed with the context: 96 bytes per row of the
 * largest call.  dcn_ctx_set_profiling covers it: pack in its slot, the extend kernel in FINISH; plan, scan and DISTINCT
 * are empty. */
int dcn_extend_batch(dcn_ctx *ctx, const dcn_index *map, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                     const void *params, const uint64_t *row_offsets, const void *rows, uint64_t n_rows, void *out);

/* ---- counters: ProcessingStats (src/local_filter.rs:179-187, merged at :388-396) -------------------------- */

/* Counters accumulated on the device over every dcn_filter_batch* call since the last reset. */
int dcn_ctx_stats(dcn_ctx *ctx, uint64_t counters[DCN_N_STATS]);
int dcn_ctx_reset_stats(dcn_ctx *ctx);

/* Sum of the six counters over n_ctx contexts of THIS process (several devices, or several contexts per device):
 * the merge of the per-worker ProcessingStats at src/local_filter.rs:388-396.  In-process contexts share an address
 * space, so this is a host sum; one-process-per-GPU jobs reduce the same six words with RCCL (bench.py). */
int dcn_stats_allreduce(dcn_ctx *const *ctxs, int n_ctx, uint64_t counters[DCN_N_STATS]);

/* The same merge ACROSS PROCESSES (one process per GPU, reads sharded, index replicated): an RCCL all-reduce(sum) of the
 * six u64 words, the path's only collective -- 48 bytes, once per run.  For a host that is not Python (which reduces them
 * with torch.distributed over RCCL): rank 0 makes an id with dcn_comm_unique_id and hands its 128 bytes to the other ranks
 * by any means of its own (a file, a socket, MPI, the job launcher); every rank then calls dcn_comm_create -- a collective
 * call: it returns when all world_size ranks are in it -- and, at the end of its share of the input,
 * dcn_stats_allreduce_rccl with its contexts (summed on the host first, as dcn_stats_allreduce does).  Every rank gets the
 * job's totals.  RCCL is bound at first use (dlopen librccl.so.1; DCN_RCCL_LIB names another file): dcn_comm_available
 * says whether it can be, without touching a GPU.  The reference's counterpart is the mutex-guarded merge of its
 * worker threads' ProcessingStats (src/local_filter.rs:388-396); it has no multi-process form. */
#define DCN_COMM_ID_BYTES 128
typedef struct dcn_comm dcn_comm;
int dcn_comm_available(void);
int dcn_comm_unique_id(uint8_t id[DCN_COMM_ID_BYTES]);
int dcn_comm_create(const uint8_t id[DCN_COMM_ID_BYTES], int world_size, int rank, int device, dcn_comm **out);
int dcn_stats_allreduce_rccl(dcn_comm *comm, dcn_ctx *const *ctxs, int n_ctx, uint64_t counters[DCN_N_STATS]);
void dcn_comm_destroy(dcn_comm *comm);

/* ---- measurement ------------------------------------------------------------------------------------ */

/* Stages of one batch on the context's stream, timed with HIP events recorded on that stream. */
enum {
    DCN_STAGE_PACK = 0,     /* ASCII -> 2-bit stream + invalid mask */
    DCN_STAGE_PLAN = 1,     /* effective lengths, prefix sum, tile descriptors */
    DCN_STAGE_SCAN = 2,     /* minimizer scan + k-mer hash + index probe + in-wave distinct count (dominant) */
    DCN_STAGE_DISTINCT = 3, /* exact distinct count for units spanning several waves */
    DCN_STAGE_FINISH = 4,   /* decisions of those units + the six counters */
    DCN_N_STAGES = 5
};

/* enable 1: record events around every stage of every following batch (and clear the accumulators); 2: around the
 * scan stage only (two marker packets per batch instead of six: the form a throughput measurement can afford);
 * 0: off. */
int dcn_ctx_set_profiling(dcn_ctx *ctx, int enable);

/* Accumulated device time per stage in milliseconds and the number of batches measured, for batches that
 * have completed (call after dcn_ctx_synchronize). */
int dcn_ctx_profile(dcn_ctx *ctx, double stage_ms[DCN_N_STAGES], uint64_t *n_batches);

#ifdef __cplusplus
}
#endif
#endif /* DEACON_HIP_H */
