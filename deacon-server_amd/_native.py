"""ctypes binding of lib/libdeacon_hip.so (the C ABI declared in include/deacon_hip.h).

There is NO fallback: if the HIP library is missing or fails to load, importing this module raises.
"""
import ctypes as C
import os
import re
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DCN_LIB_PATH") or os.path.join(_PKG, "lib", "libdeacon_hip.so")  # env: experiment builds
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "deacon_hip.h")

DCN_OK = 0
DCN_ERR_ARG = -1
DCN_ERR_HIP = -2
DCN_ERR_NOMEM = -3
DCN_ERR_IO = -4
DCN_ERR_FORMAT = -5
DCN_ERR_CAPACITY = -6
DCN_ERR_INTERNAL = -7
N_STATS = 6
N_STAGES = 5
STAGE_NAMES = ("pack", "plan", "scan", "distinct", "finish")
STAT_NAMES = ("total_seqs", "filtered_seqs", "total_bp", "output_bp", "filtered_bp", "output_seq_counter")


class DeaconHipError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"deacon_hip error {code}: {message}")
        self.code = code
        self.message = message


class Params(C.Structure):
    _fields_ = [
        ("abs_threshold", C.c_uint64),
        ("rel_threshold", C.c_double),
        ("prefix_length", C.c_uint64),
        ("deplete", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class LocateParams(C.Structure):
    _fields_ = [
        ("max_gap", C.c_uint32),
        ("min_hits", C.c_uint32),
        ("member_mask", C.c_uint32),
        ("reserved", C.c_uint32),
        ("prefix_length", C.c_uint64),
    ]


class TrackParams(C.Structure):
    _fields_ = [
        ("bin_bases", C.c_uint32),
        ("member_mask", C.c_uint32),
        ("depth_cap", C.c_uint32),
        ("reserved", C.c_uint32),
        ("prefix_length", C.c_uint64),
    ]


class TrackBin(C.Structure):
    _fields_ = [
        ("n_positions", C.c_uint32),
        ("n_keys", C.c_uint32),
        ("n_observed", C.c_uint32),
        ("max_depth", C.c_uint32),
        ("sum_depth", C.c_uint64),
    ]


class PlaceParams(C.Structure):
    _fields_ = [
        ("band_bases", C.c_uint32),
        ("min_votes", C.c_uint32),
        ("prefix_length", C.c_uint64),
        ("reserved", C.c_uint32 * 2),
    ]


class Placement(C.Structure):
    _fields_ = [
        ("record", C.c_uint32),
        ("reverse", C.c_uint32),
        ("votes", C.c_uint32),
        ("n_anchors", C.c_uint32),
        ("n_positions", C.c_uint32),
        ("read_start", C.c_uint32),
        ("read_end", C.c_uint32),
        ("reserved", C.c_uint32),
        ("ref_start", C.c_uint64),
        ("ref_end", C.c_uint64),
    ]


class PlaceSplitParams(C.Structure):
    _fields_ = [
        ("band_bases", C.c_uint32),
        ("min_votes", C.c_uint32),
        ("prefix_length", C.c_uint64),
        ("max_placements", C.c_uint32),
        ("reserved", C.c_uint32 * 3),
    ]


class SplitPlacement(C.Structure):
    _fields_ = Placement._fields_ + [
        ("rank", C.c_uint32),
        ("n_placed", C.c_uint32),
        ("rival_votes", C.c_uint32),
        ("mapq", C.c_uint32),
    ]


PLACE_SPLIT_MAX = 8  # DCN_PLACE_SPLIT_MAX


class PlacePairParams(C.Structure):
    _fields_ = [
        ("band_bases", C.c_uint32),
        ("min_votes", C.c_uint32),
        ("prefix_length", C.c_uint64),
        ("max_placements", C.c_uint32),
        ("max_insert", C.c_uint32),
        ("hist_bin_bases", C.c_uint32),
        ("reserved", C.c_uint32 * 3),
    ]


class PairPlacement(C.Structure):
    _fields_ = SplitPlacement._fields_ + [
        ("flags", C.c_uint32),
        ("pair_votes", C.c_uint32),
        ("tlen", C.c_int64),
    ]


PAIR_HIST_BINS = 256  # DCN_PAIR_HIST_BINS


class VerifyParams(C.Structure):
    _fields_ = [
        ("max_edits", C.c_uint32),
        ("max_permille", C.c_uint32),
        ("row_stride", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


VERIFY_MAX_EDITS = 1023  # DCN_VERIFY_MAX_EDITS
VERIFY_OVER = 0xFFFFFFFE  # DCN_VERIFY_OVER
VERIFY_UNPLACED = 0xFFFFFFFF  # DCN_VERIFY_UNPLACED
CIGAR_INS, CIGAR_DEL, CIGAR_EQUAL, CIGAR_DIFF = 1, 2, 7, 8  # DCN_CIGAR_*: BAM's codes of the ops of dcn_align_batch


class PileupCallParams(C.Structure):
    _fields_ = [
        ("min_depth", C.c_uint32),
        ("min_permille", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


# DCN_PILEUP_*: the columns of a pileup, the flags of a site and the code of no call
PILEUP_A, PILEUP_C, PILEUP_G, PILEUP_T, PILEUP_N, PILEUP_DEL, PILEUP_INS, PILEUP_REV = range(8)
PILEUP_COLUMNS = 8
PILEUP_SITE_SUB, PILEUP_SITE_DEL, PILEUP_SITE_INS = 1, 2, 4
PILEUP_NO_CODE = 7


class Insertion(C.Structure):
    _fields_ = [
        ("pos", C.c_uint64),
        ("bases_offset", C.c_uint64),
        ("len", C.c_uint32),
        ("flags", C.c_uint32),
    ]


class InsertionAllele(C.Structure):
    _fields_ = [
        ("pos", C.c_uint64),
        ("bases_offset", C.c_uint64),
        ("len", C.c_uint32),
        ("count", C.c_uint32),
        ("events", C.c_uint32),
        ("flags", C.c_uint32),
    ]


INSERTION_FRONT, INSERTION_REVERSE = 1, 2  # DCN_INSERTION_*: the flags of an event; an allele has FRONT only


class PileupQualParams(C.Structure):
    _fields_ = [
        ("qual_offset", C.c_uint32),
        ("min_base_qual", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


class GenotypeParams(C.Structure):
    _fields_ = [
        ("ploidy", C.c_uint32),
        ("min_depth", C.c_uint32),
        ("min_gq", C.c_uint32),
        ("min_qual", C.c_uint32),
        ("err_centi", C.c_uint32),
        ("het_centi", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


class GenotypeSite(C.Structure):
    _fields_ = [
        ("pos", C.c_uint64),
        ("qual", C.c_uint32),
        ("depth", C.c_uint32),
        ("ad", C.c_uint32 * 4),
        ("gt", C.c_uint8),
        ("gq", C.c_uint8),
        ("ref_code", C.c_uint8),
        ("reserved0", C.c_uint8),
        ("pl", C.c_uint8 * 10),
        ("reserved1", C.c_uint8 * 2),
    ]


GENOTYPE_NONE = 255  # DCN_GENOTYPE_NONE: the gt byte of a position that is not called
GENOTYPES = ("AA", "AC", "CC", "AG", "CG", "GG", "AT", "CT", "GT", "TT")  # rule G3's order at ploidy 2; ploidy 1: A C G T


class DuplicateParams(C.Structure):
    _fields_ = [
        ("row_stride", C.c_uint32),
        ("paired", C.c_uint32),
        ("both_ends", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class Deletion(C.Structure):
    _fields_ = [
        ("pos", C.c_uint64),
        ("len", C.c_uint32),
        ("flags", C.c_uint32),
    ]


DELETION_REVERSE = 1  # DCN_DELETION_REVERSE: the flag of an event of a deletion ledger
INDEL_DELETION, INDEL_FRONT = 1, 2  # DCN_INDEL_*: the flags of an indel site


class IndelParams(C.Structure):
    _fields_ = [
        ("ploidy", C.c_uint32),
        ("min_depth", C.c_uint32),
        ("min_gq", C.c_uint32),
        ("min_qual", C.c_uint32),
        ("min_count", C.c_uint32),
        ("indel_centi", C.c_uint32),
        ("het_centi", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class IndelSite(C.Structure):
    _fields_ = [
        ("pos", C.c_uint64),
        ("bases_offset", C.c_uint64),
        ("len", C.c_uint32),
        ("flags", C.c_uint32),
        ("qual", C.c_uint32),
        ("depth", C.c_uint32),
        ("count", C.c_uint32),
        ("events", C.c_uint32),
        ("gt", C.c_uint8),
        ("gq", C.c_uint8),
        ("pl", C.c_uint8 * 3),
        ("reserved", C.c_uint8 * 3),
    ]


class LeftAlignInfo(C.Structure):
    _fields_ = [
        ("rows_aligned", C.c_uint64),
        ("rows_changed", C.c_uint64),
        ("gaps_shifted", C.c_uint64),
        ("columns_passed", C.c_uint64),
        ("gaps_merged", C.c_uint64),
    ]


class StrandParams(C.Structure):
    _fields_ = [
        ("max_sb_centi", C.c_uint32),
        ("min_alt_strand", C.c_uint32),
        ("min_strand_depth", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class StrandQuery(C.Structure):
    _fields_ = [
        ("pos", C.c_uint64),
        ("kind", C.c_uint32),
        ("ref_code", C.c_uint32),
        ("alt_mask", C.c_uint32),
        ("count", C.c_uint32),
        ("count_reverse", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class StrandSite(C.Structure):
    _fields_ = [
        ("fwd", C.c_uint32 * 4),
        ("rev", C.c_uint32 * 4),
        ("table", C.c_uint32 * 4),
        ("sb_centi", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


STRAND_BIAS, STRAND_ONE_SIDED = 1, 2  # DCN_STRAND_*: the flags of rule S6


class BlockParams(C.Structure):  # dcn_block_params of include/deacon_hip_blocks.h, 48 bytes
    _fields_ = [
        ("ploidy", C.c_uint32),
        ("min_depth", C.c_uint32),
        ("min_gq", C.c_uint32),
        ("min_qual", C.c_uint32),
        ("err_centi", C.c_uint32),
        ("het_centi", C.c_uint32),
        ("n_edges", C.c_uint32),
        ("reserved", C.c_uint32),
        ("edges", C.c_uint8 * 16),
    ]


class ReferenceBlock(C.Structure):  # dcn_reference_block, 40 bytes
    _fields_ = [
        ("pos", C.c_uint64),
        ("sum_depth", C.c_uint64),
        ("len", C.c_uint32),
        ("min_depth", C.c_uint32),
        ("max_depth", C.c_uint32),
        ("min_gq", C.c_uint32),
        ("cls", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


BLOCK_NO_COVERAGE, BLOCK_UNCALLED, BLOCK_REF, BLOCK_VARIANT = 0, 1, 2, 255  # DCN_BLOCK_*: the classes of rule B2


class ExtendParams(C.Structure):
    _fields_ = [
        ("penalty", C.c_uint32),
        ("end_bonus", C.c_uint32),
        ("max_edits", C.c_uint32),
        ("row_stride", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


class Extension(C.Structure):
    _fields_ = [
        ("read_start", C.c_uint32),
        ("read_end", C.c_uint32),
        ("ref_start", C.c_uint64),
        ("ref_end", C.c_uint64),
        ("left_edits", C.c_uint32),
        ("right_edits", C.c_uint32),
    ]


def build(force=False, jobs=6):
    """Compile every HIP source for gfx950 into lib/libdeacon_hip.so (hipcc cross-compiles without a GPU)."""
    csrc = os.path.join(_PKG, "csrc")
    cmd = ["make", "-C", csrc, f"-j{jobs}"]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return LIB_PATH


def declared_symbols():
    """Names of every function declared in include/deacon_hip.h."""
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dcn_[a-z0-9_]+)\s*\(", text)))


_u8p, _u32p, _u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
_vp = C.c_void_p

_SIGNATURES = {
    "dcn_abi_version": (C.c_int, [_u32p, _u32p]),
    "dcn_version": (C.c_char_p, []),
    "dcn_last_error": (C.c_char_p, []),
    "dcn_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "dcn_set_minimizer_variant": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "dcn_get_minimizer_variant": (C.c_int, [_u32p, _u32p, _u32p]),
    "dcn_index_from_keys": (C.c_int, [_vp, C.c_uint64, C.c_uint8, C.c_uint8, C.c_int, C.POINTER(_vp)]),
    "dcn_index_from_file": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(_vp)]),
    "dcn_index_build": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint8, C.c_uint8, C.c_float, C.c_uint64, C.c_int,
                                  C.POINTER(_vp)]),
    "dcn_index_keys": (C.c_int, [_vp, _vp, C.c_uint64, _u64p]),
    "dcn_index_union": (C.c_int, [C.POINTER(_vp), C.c_uint32, C.POINTER(_vp)]),
    "dcn_index_diff": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "dcn_index_intersect": (C.c_int, [C.POINTER(_vp), C.c_uint32, C.POINTER(_vp)]),
    "dcn_index_write_file": (C.c_int, [_vp, C.c_char_p]),
    "dcn_index_header": (C.c_int, [_vp, _u8p, _u8p, _u64p]),
    "dcn_index_contains": (C.c_int, [_vp, _vp, C.c_uint64, _vp]),
    "dcn_index_contains_device": (C.c_int, [_vp, _vp, C.c_uint64, _vp, _vp]),
    "dcn_index_probe_ceiling": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)]),
    "dcn_index_destroy": (None, [_vp]),
    "dcn_ctx_create": (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.POINTER(_vp)]),
    "dcn_ctx_destroy": (None, [_vp]),
    "dcn_filter_batch": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, C.POINTER(Params), _vp, _vp, _vp]),
    "dcn_filter_batch_submit": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, C.POINTER(Params), _vp, _vp, _vp, _u64p]),
    "dcn_filter_batch_wait": (C.c_int, [_vp, C.c_uint64]),
    "dcn_filter_batch_packed": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint32, C.POINTER(Params), _vp, _vp, _vp]),
    "dcn_filter_batch_packed_submit": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint32, C.POINTER(Params), _vp, _vp, _vp,
                                                 _u64p]),
    "dcn_pack_ascii": (C.c_int, [_vp, C.c_uint64, _vp, _vp, _u32p]),
    "dcn_stats_allreduce": (C.c_int, [C.POINTER(_vp), C.c_int, _u64p]),
    "dcn_comm_available": (C.c_int, []),
    "dcn_comm_unique_id": (C.c_int, [_vp]),
    "dcn_comm_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "dcn_stats_allreduce_rccl": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, _u64p]),
    "dcn_comm_destroy": (None, [_vp]),
    "dcn_index_device": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "dcn_index_memory": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "dcn_index_clone": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "dcn_filter_batch_device": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64, C.c_uint32,
                                          C.POINTER(Params), _vp, _vp, _vp]),
    "dcn_ctx_synchronize": (C.c_int, [_vp]),
    "dcn_ctx_last_batch_short": (C.c_int, [_vp, _u32p]),
    "dcn_ctx_reserve_records": (C.c_int, [_vp, C.c_uint64]),
    "dcn_ctx_stream": (_vp, [_vp]),
    "dcn_host_alloc": (C.c_int, [C.c_uint64, C.POINTER(_vp)]),
    "dcn_host_free": (None, [_vp]),
    "dcn_minimizer_hashes_batch": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_uint64, _vp, _vp, _vp, C.c_uint64]),
    "dcn_should_keep_hashes": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.POINTER(Params), _vp, _vp, _vp]),
    "dcn_ctx_stats": (C.c_int, [_vp, _u64p]),
    "dcn_ctx_reset_stats": (C.c_int, [_vp]),
    "dcn_ctx_set_profiling": (C.c_int, [_vp, C.c_int]),
    "dcn_ctx_profile": (C.c_int, [_vp, C.POINTER(C.c_double), _u64p]),
    "dcn_index_set_create": (C.c_int, [C.POINTER(_vp), C.c_uint32, C.POINTER(_vp)]),
    "dcn_index_set_destroy": (None, [_vp]),
    "dcn_index_set_info": (C.c_int, [_vp, _u32p, _u8p, _u8p, _u64p, _u64p]),
    "dcn_classify_batch": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint32, C.POINTER(Params), _vp, _vp, _vp]),
    "dcn_classify_batch_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64, C.c_uint32,
                                            C.POINTER(Params), _vp, _vp, _vp]),
    "dcn_index_set_coverage_enable": (C.c_int, [_vp, C.c_int]),
    "dcn_index_set_coverage_reset": (C.c_int, [_vp]),
    "dcn_index_set_coverage": (C.c_int, [_vp, _vp, _vp]),
    "dcn_index_set_coverage_keys": (C.c_int, [_vp, C.c_uint32, _vp, C.c_uint64, _u64p]),
    "dcn_index_set_depth_enable": (C.c_int, [_vp, C.c_int]),
    "dcn_index_set_depth_reset": (C.c_int, [_vp]),
    "dcn_index_set_depth_stats": (C.c_int, [_vp, _vp, _vp, _vp]),
    "dcn_index_set_depth_hist": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp]),
    "dcn_index_set_depth_keys": (C.c_int, [_vp, C.c_uint32, _vp, _vp, C.c_uint64, _u64p]),
    "dcn_index_set_select": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _u64p,
                                       C.POINTER(_vp)]),
    "dcn_index_set_overlap": (C.c_int, [_vp, _vp, _vp, _vp]),
    "dcn_index_builder_create": (C.c_int, [C.c_uint8, C.c_uint8, C.c_float, C.c_uint64, C.c_int, C.POINTER(_vp)]),
    "dcn_index_builder_add": (C.c_int, [_vp, _vp, _vp, C.c_uint32]),
    "dcn_index_builder_info": (C.c_int, [_vp, _u64p, _u64p, _u64p, _u64p]),
    "dcn_index_builder_hist": (C.c_int, [_vp, C.c_uint32, _vp]),
    "dcn_index_builder_counts": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _u64p]),
    "dcn_index_builder_finish": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _u64p, C.POINTER(_vp)]),
    "dcn_index_builder_destroy": (None, [_vp]),
    "dcn_locate_batch": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, C.c_uint64]),
    "dcn_depth_track_batch": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, C.c_uint64]),
    "dcn_anchor_map_create": (C.c_int, [_vp, C.POINTER(_vp)]),
    "dcn_anchor_map_add": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _u32p]),
    "dcn_anchor_map_info": (C.c_int, [_vp, _u32p, _u64p, _u64p, _u64p]),
    "dcn_anchor_map_anchors": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, _u64p]),
    "dcn_place_batch": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp]),
    "dcn_place_split_batch": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, C.c_uint64, _vp]),
    "dcn_place_pair_batch": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp]),
    "dcn_anchor_map_keep_bases": (C.c_int, [_vp]),
    "dcn_anchor_map_fetch": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.c_uint64, _vp]),
    "dcn_verify_batch": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, C.c_uint64, _vp]),
    "dcn_align_batch": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, C.c_uint64, _vp, _vp, _vp, C.c_uint64]),
    "dcn_anchor_map_pileup_enable": (C.c_int, [_vp, C.c_int]),
    "dcn_anchor_map_pileup_reset": (C.c_int, [_vp]),
    "dcn_pileup_batch": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, C.c_uint64, _vp, _u64p]),
    "dcn_anchor_map_pileup_fetch": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.c_uint64, _vp]),
    "dcn_anchor_map_pileup_call": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint64, C.c_uint64, _vp, _vp, _vp, C.c_uint64, _u64p]),
    "dcn_extend_batch": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, C.c_uint64, _vp]),
    "dcn_anchor_map_pileup_keep_insertions": (C.c_int, [_vp, C.c_int]),
    "dcn_anchor_map_insertions_info": (C.c_int, [_vp, _u64p, _u64p]),
    "dcn_anchor_map_insertions_fetch": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.c_uint64, _vp, C.c_uint64, _vp, C.c_uint64, _u64p, _u64p]),
    "dcn_anchor_map_insertions_call": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint64, C.c_uint64, _vp, C.c_uint64, _vp, C.c_uint64, _u64p, _u64p]),
    "dcn_anchor_map_pileup_keep_qualities": (C.c_int, [_vp, C.c_int]),
    "dcn_pileup_batch_qual": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, C.c_uint64, _vp, _u64p]),
    "dcn_anchor_map_pileup_fetch_qualities": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.c_uint64, _vp]),
    "dcn_anchor_map_genotype": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint64, C.c_uint64, _vp, _vp, _vp, C.c_uint64, _u64p]),
    "dcn_anchor_map_duplicates_enable": (C.c_int, [_vp, C.c_int]),
    "dcn_anchor_map_duplicates_reset": (C.c_int, [_vp]),
    "dcn_anchor_map_duplicates_info": (C.c_int, [_vp, _u64p, _u64p, _u64p]),
    "dcn_mark_duplicates_batch": (C.c_int, [_vp, _vp, C.c_uint32, _vp, _vp, _vp, C.c_uint64, _vp, _vp, _u64p]),
    "dcn_anchor_map_pileup_keep_deletions": (C.c_int, [_vp, C.c_int]),
    "dcn_anchor_map_deletions_info": (C.c_int, [_vp, _u64p, _u64p]),
    "dcn_anchor_map_deletions_fetch": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.c_uint64, _vp, C.c_uint64, _u64p]),
    "dcn_anchor_map_indels_genotype": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint64, C.c_uint64, _vp, C.c_uint64, _vp, C.c_uint64, _u64p, _u64p]),
    "dcn_left_align_batch": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, C.c_uint64, _vp, _vp, _vp, C.c_uint64, _vp]),
    "dcn_anchor_map_pileup_left_align": (C.c_int, [_vp, C.c_int]),
    "dcn_anchor_map_pileup_left_align_info": (C.c_int, [_vp, _vp]),
    "dcn_anchor_map_pileup_keep_strands": (C.c_int, [_vp, C.c_int]),
    "dcn_anchor_map_pileup_fetch_strands": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.c_uint64, _vp]),
    "dcn_anchor_map_strand_evidence": (C.c_int, [_vp, _vp, C.c_uint32, _vp, C.c_uint64, _vp]),
    "dcn_anchor_map_indels_strand": (C.c_int, [_vp, C.c_uint32, _vp, C.c_uint64, _vp, _vp]),
}

# the functions that include/deacon_hip_blocks.h declares (ABI 1.24): a table of their own, so that _SIGNATURES stays the set
# of include/deacon_hip.h
BLOCKS_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "deacon_hip_blocks.h")
_BLOCK_SIGNATURES = {
    "dcn_anchor_map_reference_blocks": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint64, C.c_uint64, _vp, C.c_uint64, _vp, _vp, C.c_uint64, _u64p]),
    "dcn_reference_blocks_merge": (C.c_int, [_vp, C.c_uint64, _u64p]),
}

# ... and those of include/deacon_hip_phase.h (ABI 1.25), likewise
PHASE_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "deacon_hip_phase.h")
_PHASE_SIGNATURES = {
    "dcn_anchor_map_phase_sites": (C.c_int, [_vp, _vp, C.c_uint64]),
    "dcn_anchor_map_phase_info": (C.c_int, [_vp, _vp]),
    "dcn_phase_batch": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, C.c_uint64, _vp, _u64p]),
    "dcn_anchor_map_phase_links": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _vp]),
    "dcn_anchor_map_phase_solve": (C.c_int, [_vp, _vp, _vp]),
}


class PhaseParams(C.Structure):  # dcn_phase_params of include/deacon_hip_phase.h, 16 bytes
    _fields_ = [("min_reads", C.c_uint32), ("max_minor_permille", C.c_uint32), ("reserved", C.c_uint32 * 2)]


PHASE_HEAD, PHASE_JOINED = 1, 2  # DCN_PHASE_*: the flags of a dcn_phase_result

_lib = None
ABI = (1, 25)  # DCN_ABI_MAJOR, the DCN_ABI_MINOR these signatures need


def lib():
    """Load the shared library (once).  Raises if it has not been built: the product has no CPU path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
            "(make -C deacon-server_amd/csrc). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in list(_SIGNATURES.items()) + list(_BLOCK_SIGNATURES.items()) + list(_PHASE_SIGNATURES.items()):
        f = getattr(L, name)  # AttributeError if the library does not export a declared symbol
        f.restype = res
        f.argtypes = args
    major, minor = C.c_uint32(), C.c_uint32()
    if L.dcn_abi_version(C.byref(major), C.byref(minor)) != 0 or (major.value, minor.value >= ABI[1]) != (ABI[0], True):
        raise ImportError(f"{LIB_PATH} has ABI {major.value}.{minor.value}; these bindings were written against {ABI[0]}.{ABI[1]} "
                          "(include/deacon_hip.h: DCN_ABI_MAJOR / DCN_ABI_MINOR)")
    _lib = L
    return L


def check(rc):
    if rc != DCN_OK:
        msg = lib().dcn_last_error()
        raise DeaconHipError(rc, msg.decode("utf-8", "replace") if msg else "")
    return rc
