"""MI355X-native read-filtering core for Deacon: HIP kernels behind a C ABI (include/deacon_hip.h) plus a thin
host mirror of the reference's filter interface.  The directory name has a hyphen, so import it through the
`deacon_server_amd` shim at the repository root (or importlib.import_module("deacon-server_amd"))."""
from . import _native, client, distributed, server
from ._native import DeaconHipError, build, declared_symbols
from .filter import (DEFAULT_KMER_LENGTH, DEFAULT_WINDOW_SIZE, AnchorMap, Placer, Classifier, DepthTracker, FilterProcessor, Index, IndexBuilder, IndexSet, Locator, PendingBatch, PinnedBuffer,
                     concat_reads, get_minimizer_hashes_and_positions, pack_ascii, paired_should_keep,
                     get_minimizer_variant, set_minimizer_variant, stats_allreduce, unpaired_should_keep, VERIFY_OVER, VERIFY_UNPLACED, cigar_string,
                     PILEUP_A, PILEUP_C, PILEUP_G, PILEUP_T, PILEUP_N, PILEUP_DEL, PILEUP_INS, PILEUP_REV, PILEUP_COLUMNS, PILEUP_SITE_SUB, PILEUP_SITE_DEL, PILEUP_SITE_INS, PILEUP_NO_CODE,
                     EXTENSION_DTYPE, INSERTION_DTYPE, INSERTION_ALLELE_DTYPE, INSERTION_FRONT, INSERTION_REVERSE,
                     GENOTYPE_SITE_DTYPE, GENOTYPE_NONE, GENOTYPES, DELETION_DTYPE, INDEL_SITE_DTYPE, LEFT_ALIGN_INFO_DTYPE, DELETION_REVERSE,
                     INDEL_DELETION, INDEL_FRONT, STRAND_QUERY_DTYPE, STRAND_SITE_DTYPE, STRAND_BIAS, STRAND_ONE_SIDED,
                     REFERENCE_BLOCK_DTYPE, BLOCK_NO_COVERAGE, BLOCK_UNCALLED, BLOCK_REF, BLOCK_VARIANT, merge_blocks,
                     PHASE_SITE_DTYPE, PHASE_RESULT_DTYPE, PHASE_HEAD, PHASE_JOINED)

__all__ = ["DeaconHipError", "build", "declared_symbols", "Index", "IndexBuilder", "IndexSet", "Classifier", "Locator", "DepthTracker", "AnchorMap", "Placer", "FilterProcessor", "PinnedBuffer", "PendingBatch", "concat_reads",
           "pack_ascii", "stats_allreduce", "set_minimizer_variant", "get_minimizer_variant",
           "get_minimizer_hashes_and_positions", "unpaired_should_keep", "paired_should_keep",
           "DEFAULT_KMER_LENGTH", "DEFAULT_WINDOW_SIZE", "VERIFY_OVER", "VERIFY_UNPLACED", "cigar_string",
           "PILEUP_A", "PILEUP_C", "PILEUP_G", "PILEUP_T", "PILEUP_N", "PILEUP_DEL", "PILEUP_INS", "PILEUP_REV", "PILEUP_COLUMNS", "PILEUP_SITE_SUB", "PILEUP_SITE_DEL", "PILEUP_SITE_INS", "PILEUP_NO_CODE",
           "EXTENSION_DTYPE", "INSERTION_DTYPE", "INSERTION_ALLELE_DTYPE", "INSERTION_FRONT", "INSERTION_REVERSE",
           "GENOTYPE_SITE_DTYPE", "GENOTYPE_NONE", "GENOTYPES", "DELETION_DTYPE", "INDEL_SITE_DTYPE", "LEFT_ALIGN_INFO_DTYPE", "DELETION_REVERSE",
           "INDEL_DELETION", "INDEL_FRONT", "STRAND_QUERY_DTYPE", "STRAND_SITE_DTYPE", "STRAND_BIAS", "STRAND_ONE_SIDED",
           "REFERENCE_BLOCK_DTYPE", "BLOCK_NO_COVERAGE", "BLOCK_UNCALLED", "BLOCK_REF", "BLOCK_VARIANT", "merge_blocks",
           "PHASE_SITE_DTYPE", "PHASE_RESULT_DTYPE", "PHASE_HEAD", "PHASE_JOINED"]
