"""CPU checks of the quality-aware pileup surface (dcn_anchor_map_pileup_keep_qualities / _fetch_qualities,
dcn_pileup_batch_qual): declared, exported and bound at ABI 1.18, the layout of its struct in ctypes and C99, the definition
stated once, the argument errors that are found before a device is looked at, `deacon-hip call`'s usage errors, its refusal
of FASTA and its --help, the quality walk compiled for the host under the sanitizers, and the model of the GPU tests
(tests/_quality_worker.py) alone on cases whose answers are written out here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _pileup_worker as PW
import _quality_worker as QW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
SYMBOLS = {"dcn_anchor_map_pileup_keep_qualities": 2, "dcn_pileup_batch_qual": 13, "dcn_anchor_map_pileup_fetch_qualities": 5}


def test_symbols_are_declared_exported_and_bound(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    for name, n_args in SYMBOLS.items():
        assert name in N.declared_symbols() and name in N._SIGNATURES and hasattr(L, name), name
        assert len(N._SIGNATURES[name][1]) == n_args
    assert len(N.declared_symbols()) >= 98
    assert tuple(N.ABI) >= (1, 18)
    major, minor = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(major), C.byref(minor)) == 0 and (major.value, minor.value) >= (1, 18)
    header = open(N.HEADER_PATH).read()
    assert len(re.findall(r"1\.18 = dcn_anchor_map_pileup_keep_qualities / _fetch_qualities, dcn_pileup_batch_qual", header)) == 1
    assert int(re.search(r"#define DCN_ABI_MINOR (\d+)", header).group(1)) >= 18
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"pub const DCN_ABI_MINOR: u32 = (\d+); +//", md).group(1)) >= 18
    for name in SYMBOLS:
        assert re.search(r"pub fn %s\(" % name, md), name
    assert "pub struct dcn_pileup_qual_params {" in md
    for method in ("pileup_keep_qualities", "pileup_fetch_qualities"):
        assert hasattr(dcn.AnchorMap, method)
    import inspect
    sig = inspect.signature(dcn.Placer.pileup_batch).parameters
    assert [(k, sig[k].default) for k in ("quals", "min_base_qual", "qual_offset")] == [("quals", None), ("min_base_qual", 0), ("qual_offset", 33)]
    assert list(sig)[:8] == ["self", "bases", "offsets", "rows", "row_offsets", "max_edits", "max_permille", "select"]  # (as it was)


def test_the_definition_is_stated_once(dcn):
    flat = " ".join(open(dcn._native.HEADER_PATH).read().replace(" *", " ").split())
    assert flat.count("THE DEFINITION OF A QUALITY-AWARE PILEUP") == 1
    assert flat.count("THE DEFINITION OF A PILEUP") == 1 and flat.count("THE DEFINITION OF AN INSERTION LEDGER") == 1
    for i in range(1, 7):
        assert len(re.findall(r"\bQ%d\." % i, flat)) == 1, i
        assert len(re.findall(r"\bP%d\." % i, flat)) == 1, i
    for i in range(1, 9):
        assert len(re.findall(r"\bL%d\." % i, flat)) == 1, i
    assert "qualities are not complemented" in flat and "q = byte >= qual_offset ? byte - qual_offset : 0" in flat
    assert "the call never changes what aligns" in flat


def test_struct_layout_agrees(tmp_path, dcn):
    N = dcn._native
    S = N.PileupQualParams
    assert C.sizeof(S) == 16 and [f for f, _ in S._fields_] == ["qual_offset", "min_base_qual", "reserved"]
    assert (S.qual_offset.offset, S.min_base_qual.offset, S.reserved.offset) == (0, 4, 8)
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "deacon_hip.h"\n'
                   "int (*f1)(dcn_index *, int) = dcn_anchor_map_pileup_keep_qualities;\n"
                   "int (*f2)(dcn_ctx *, dcn_index *, const uint8_t *, const uint8_t *, const uint64_t *, uint32_t, const void *, const void *,\n"
                   "          const uint64_t *, const void *, uint64_t, uint32_t *, uint64_t *) = dcn_pileup_batch_qual;\n"
                   "int (*f3)(const dcn_index *, uint32_t, uint64_t, uint64_t, uint32_t *) = dcn_anchor_map_pileup_fetch_qualities;\n"
                   "int main(void){ dcn_pileup_qual_params p = {33, 20, {0, 0}};\n"
                   "  return sizeof p == 16 && offsetof(dcn_pileup_qual_params, qual_offset) == 0 && offsetof(dcn_pileup_qual_params, min_base_qual) == 4 &&\n"
                   "         offsetof(dcn_pileup_qual_params, reserved) == 8 && p.min_base_qual == 20 && DCN_ABI_MINOR >= 18 ? 0 : 1; }\n")
    inc = os.path.dirname(N.HEADER_PATH)
    libdir = os.path.dirname(N.LIB_PATH)  # (the function pointers are initialised and never called)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(tmp_path / "t"), "-L", libdir,
                           "-ldeacon_hip", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"])
    assert subprocess.call([str(tmp_path / "t")]) == 0


def test_argument_errors_that_need_no_device(dcn):
    """dcn_pileup_batch_qual: dcn_pileup_batch's checks first, in its order and word for word, whatever qual_params and quals
    are; the map calls: NULL"""
    N, L = dcn._native, dcn._native.lib()

    def prm(edits=1023, permille=200, stride=48, reserved=0):
        return C.byref(N.VerifyParams(edits, permille, stride, reserved))

    stand_in = (C.c_uint8 * 4096)()
    added = C.c_uint64(77)
    bad_q = C.byref(N.PileupQualParams(999, 999, (C.c_uint32 * 2)(1, 1)))
    for args, word in (((None, None, None), b"params is NULL"),
                       ((None, None, prm(reserved=1)), b"reserved"),
                       ((None, None, prm(edits=1024)), b"max_edits must be 0..1023"),
                       ((None, None, prm(permille=1001)), b"max_permille must be 0..1000"),
                       ((None, None, prm(stride=40)), b"row_stride"),
                       ((None, None, prm(stride=52)), b"row_stride"),
                       ((None, None, prm()), b"ctx is NULL"),
                       ((C.cast(stand_in, C.c_void_p), None, prm(stride=64)), b"map is NULL")):
        assert L.dcn_pileup_batch(args[0], args[1], None, None, 0, args[2], None, None, 0, None, C.byref(added)) == N.DCN_ERR_ARG
        message = L.dcn_last_error()
        assert word in message, (word, message)
        for qp in (None, bad_q):
            assert L.dcn_pileup_batch_qual(args[0], args[1], None, None, None, 0, args[2], qp, None, None, 0, None, C.byref(added)) == N.DCN_ERR_ARG
            assert L.dcn_last_error() == message
    assert added.value == 77  # (nothing is written by a refused call)
    out = (C.c_uint32 * 4)()
    for rc in (L.dcn_anchor_map_pileup_keep_qualities(None, 1), L.dcn_anchor_map_pileup_keep_qualities(None, 0),
               L.dcn_anchor_map_pileup_fetch_qualities(None, 0, 0, 1, out)):
        assert rc == N.DCN_ERR_ARG and b"map is NULL" in L.dcn_last_error()
        message = L.dcn_last_error()
        assert L.dcn_anchor_map_pileup_fetch(None, 0, 0, 1, out) == N.DCN_ERR_ARG and L.dcn_last_error() == message


def test_walk_on_the_host(tmp_path):
    """tests/cpp/pileup_qual_walk_test.cpp: dcn_pileup.h's quality walk in the kernel's shape (chunks of 64 runs, the prefix
    emulated serially, 64 lanes), counters and sums of exactly n positions between guard words, the qualities read from an
    array of exactly the batch's bytes between guards, against a walk step by step, under the address and
    undefined-behaviour sanitizers: 4,000 random run lists, both strands, 63 / 64 / 65 / 129 runs, runs of 63, 64, 65 bases"""
    exe = tmp_path / "pileup_qual_walk_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "deacon-server_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "pileup_qual_walk_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "pileup quality walk ok: 4000 run lists" in out.stdout, out.stderr[-2000:]


CALL_ERRORS = [
    (["call"], "the following required arguments were not provided: <REF>"),
    (["call", "ref.fa", "--min-baseq", "256"], "invalid value for --min-baseq: must be 0..255"),
    (["call", "ref.fa", "--min-baseq", "-1"], "invalid value for --min-baseq: must be 0..255"),
    (["call", "ref.fa", "--qual-offset", "256"], "invalid value for --qual-offset: must be 0..255"),
    (["call", "ref.fa", "--min-baseq"], "missing value for --min-baseq"),
    (["call", "ref.fa", "--min-mapq", "61"], "invalid value for --min-mapq: must be 0..60"),
    (["call", "ref.fa", "--min-frac", "1001"], "invalid value for --min-frac: must be 0..1000"),
    (["call", "ref.fa", "-e", "1024"], "invalid value for --max-edits: must be 0..1023"),
    (["call", "ref.fa", "--penalty", "1"], "invalid value for --penalty: must be 2..255"),
    (["call", "ref.fa", "in1", "in2"], "call takes one input: mates are independent here, run it once per file (unexpected argument 'in2')"),
    (["call", "--nope"], "unexpected argument '--nope'"),
    (["call", "ref.fa", "--verified-only"], "unexpected argument '--verified-only'"),
    (["call", "ref.fa", "--variants"], "missing value for --variants"),
]


@pytest.mark.parametrize("args,message", CALL_ERRORS, ids=[" ".join(e[0]) for e in CALL_ERRORS])
def test_call_error_exit_code_and_text(args, message):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "Error: " + message + "\n")


def test_call_refuses_fasta_and_names_the_record(tmp_path):
    """a record without qualities is a usage error that names the record: found at the first record, before the reference is
    read (a FASTA record behind FASTQ ones is found when its batch is gathered: tests/test_gpu_call_cli.py)"""
    reads = tmp_path / "reads.fa"
    reads.write_text(">read7 some words\nACGTACGT\n")
    message = "Error: call needs base qualities, and record 'read7' has none (FASTA): consensus takes reads without\n"
    p = subprocess.run([CLI, "call", "ref.fa", str(reads)], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", message)
    p = subprocess.run([CLI, "call", "ref.fa"], capture_output=True, text=True, timeout=60, input=reads.read_text())
    assert (p.returncode, p.stdout, p.stderr) == (1, "", message)


def test_call_help_text():
    p = subprocess.run([CLI, "call", "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "call.txt")) as f:
        want = f.read()
    assert (p.returncode, p.stderr, p.stdout) == (0, "", want)
    for word in ("Usage: deacon-hip call [OPTIONS] <REF> [READS]", "--min-baseq <Q>", "[default: 20, a convention]", "--qual-offset <N>", "[default: 33]",
                 "ref_qual alt_qual", "qA qC qG qT", "min_base_qual", "quality_sums", "--variants <FILE>", "--fill-ref", "--min-depth <N>", "--min-frac <N>",
                 "--min-mapq <N>", "--all-ranks", "--pileup <FILE>", "--sites <FILE>", "The thresholds are conventions, not measured optima",
                 "With --min-baseq 0 the FASTA is consensus's", "No quality-weighted calls or likelihoods, no VCF"):
        assert word in want, word
    top = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert (top.stdout + top.stderr).count("\n  call ") == 1 and (top.stdout + top.stderr).count("\n  consensus ") == 1
    # the other modes of the same driver do not know call's options
    for sub in ("map", "verify", "align", "pileup", "extend", "consensus"):
        for opt in ("--min-baseq", "--qual-offset"):
            q = subprocess.run([CLI, sub, "ref.fa", opt, "3"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
            assert (q.returncode, q.stderr) == (1, "Error: unexpected argument '%s'\n" % opt)


# ---- the model alone ---------------------------------------------------------------------------------------------------
def col(**at):
    """{position: {column name: value}} -> a dict to compare a counts or sums array with"""
    return at


def rows_of(a, names):
    """the non-zero entries of counts[n, 8] or sums[n, 4] -> {position: {name: value}}"""
    return {p: {names[c]: int(a[p, c]) for c in range(a.shape[1]) if a[p, c]} for p in range(a.shape[0]) if a[p].any()}


CN = ["A", "C", "G", "T", "N", "DEL", "INS", "REV"]
Q = lambda *qs: bytes(q + 33 for q in qs)  # noqa: E731


def test_model_alone_on_thresholds_written_out():
    """THE TESTS HERE THAT PASS WITHOUT THE FEATURE: this one and the three below run the model only.
    q at the threshold counts, one below it is N; a byte below the offset is quality 0; byte 255; thresholds 0 and 255"""
    S = T = b"ACGT"
    q = [20, 19, 20, 19]
    counts, sums, events, text = QW.pile_pair(S, T, q, 20)
    assert text == "4=" and events == []
    assert rows_of(counts, CN) == {0: {"A": 1}, 1: {"N": 1}, 2: {"G": 1}, 3: {"N": 1}}
    assert rows_of(sums, CN) == {0: {"A": 20}, 2: {"G": 20}}
    assert QW.quality(32) == 0 and QW.quality(0) == 0 and QW.quality(33) == 0 and QW.quality(34) == 1 and QW.quality(255) == 222 and QW.quality(255, 0) == 255
    row = dict(read_start=0, read_end=4, reverse=0)
    assert QW.qualities_of_S(bytes([10, 33, 255, 53]), row) == [0, 0, 222, 20]  # (a byte below the offset is no error)
    # threshold 0: nothing is masked, a base of quality 0 counts and adds 0
    counts, sums, _, _ = QW.pile_pair(S, T, [0, 0, 7, 222], 0)
    assert rows_of(counts, CN) == {0: {"A": 1}, 1: {"C": 1}, 2: {"G": 1}, 3: {"T": 1}} and rows_of(sums, CN) == {2: {"G": 7}, 3: {"T": 222}}
    # threshold 255: only q = 255 counts, which needs offset 0 and byte 255
    qs = QW.qualities_of_S(bytes([255, 254, 255, 0]), row, 0)
    counts, sums, _, _ = QW.pile_pair(S, T, qs, 255)
    assert qs == [255, 254, 255, 0] and rows_of(counts, CN) == {0: {"A": 1}, 1: {"N": 1}, 2: {"G": 1}, 3: {"N": 1}}
    assert rows_of(sums, CN) == {0: {"A": 255}, 2: {"G": 255}}


def test_model_alone_on_edits_written_out():
    """an N of high quality stays N and sums nothing; a low-quality base under X; one right behind a D run; a low-quality
    inserted base leaves the event as it is"""
    counts, sums, _, text = QW.pile_pair(b"ACNTACGT", b"ACGTACGT", [40] * 8, 20)
    assert text == "2=1X5=" and counts[2].tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and sums[2].tolist() == [0, 0, 0, 0] and int(sums.sum()) == 7 * 40
    # X at position 4 (T for A): high quality -> T with its sum, low quality -> N without
    for q4, want_c, want_s in ((30, {"T": 1}, {"T": 30}), (5, {"N": 1}, None)):
        counts, sums, _, text = QW.pile_pair(b"ACGTTCGTAC", b"ACGTACGTAC", [30, 30, 30, 30, q4, 30, 30, 30, 30, 30], 20)
        assert text == "4=1X5=" and rows_of(counts, CN)[4] == want_c and rows_of(sums, CN).get(4) == want_s
    # a D run of two, then a low-quality base: S[4] lands on T[6]
    S, T = b"ACGTCATGCA", b"ACGTGGCATGCA"
    counts, sums, _, text = QW.pile_pair(S, T, [30, 30, 30, 30, 3, 30, 30, 30, 30, 30], 20)
    assert text == "4=2D6=" and rows_of(counts, CN)[4] == {"DEL": 1} and rows_of(counts, CN)[5] == {"DEL": 1}
    assert rows_of(counts, CN)[6] == {"N": 1} and rows_of(counts, CN)[7] == {"A": 1} and 6 not in rows_of(sums, CN) and rows_of(sums, CN)[7] == {"A": 30}
    # an inserted base of quality 0: the event is what it is without qualities, the counters around it too
    S, T = b"ACGTTTACGA", b"ACGTACGA"
    for q in ([30] * 10, [30, 30, 30, 30, 0, 0, 30, 30, 30, 30]):
        counts, sums, events, text = QW.pile_pair(S, T, q, 20, ref_start=1)
        assert events == [(4, 0, 2, b"TT", 0)] and int(counts[4, PW.INS]) == 1 and int(counts[:, PW.N].sum()) == 0 and int(sums.sum()) == 8 * 30, text


def test_model_alone_on_a_reverse_row_written_out():
    """a reverse row with one low-quality base at read position 0: S is the reverse complement, so the base is S's LAST, and
    it lands on the last base of T; the qualities are turned, not complemented"""
    read, quals = b"AACCG", Q(2, 30, 31, 32, 33)
    row = dict(read_start=0, read_end=5, reverse=1)
    S = b"CGGTT"  # revcomp(read)
    q = QW.qualities_of_S(quals, row)
    assert q == [33, 32, 31, 30, 2]
    counts, sums, _, text = QW.pile_pair(S, S, q, 20, reverse=1, ref_start=3)
    assert text == "5="
    assert rows_of(counts, CN) == {3: {"C": 1, "REV": 1}, 4: {"G": 1, "REV": 1}, 5: {"G": 1, "REV": 1}, 6: {"T": 1, "REV": 1}, 7: {"N": 1, "REV": 1}}
    assert rows_of(sums, CN) == {3: {"C": 33}, 4: {"G": 32}, 5: {"G": 31}, 6: {"T": 30}}
    # an interval behind a soft clip: read_start = 2 of a 7-base read; S = revcomp(read[2:7]), its qualities quals[2:7] turned
    row = dict(read_start=2, read_end=7, reverse=1)
    assert QW.qualities_of_S(Q(9, 9, 2, 30, 31, 32, 33), row) == [33, 32, 31, 30, 2]
    assert QW.masked(S, q, 31) == b"CGGNN" and QW.masked(b"CnGTT", q, 0) == b"CnGTT"


def test_model_alone_on_variant_qualities_written_out():
    """`deacon-hip call`'s ref_qual and alt_qual: integer quotients; "." for a count of 0 and for an invalid reference base"""
    c = np.array([3, 0, 5, 0, 2, 0, 0, 0])
    s = np.array([100, 0, 199, 0])
    assert QW.variant_quals(c, s, ord("A"), "G") == ("33", "39")
    assert QW.variant_quals(c, s, ord("a"), "G") == ("33", "39")
    assert QW.variant_quals(c, s, ord("C"), "G") == (".", "39")  # no read shows the reference's base
    assert QW.variant_quals(c, s, ord("N"), "G") == (".", "39")  # the reference base is invalid
    assert QW.variant_quals(c, s, ord("G"), "T") == ("39", ".")
