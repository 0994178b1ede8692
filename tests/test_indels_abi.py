"""CPU checks of the indel surface (dcn_anchor_map_pileup_keep_deletions, dcn_anchor_map_deletions_info / _fetch,
dcn_anchor_map_indels_genotype): declared, exported and bound at ABI 1.21, the layout of the three structs in ctypes, numpy
and C99, the two definitions stated once, the argument errors that are found before a device is looked at, in their order,
`deacon-hip indels`'s usage errors and its --help, the rules of csrc/dcn_indels.h compiled for the host under the
sanitizers, and the model of the GPU tests (tests/_indel_worker.py) alone on cases whose answers are written out here."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _align_worker as AW
import _indel_worker as DW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
NAMES = ["dcn_anchor_map_pileup_keep_deletions", "dcn_anchor_map_deletions_info", "dcn_anchor_map_deletions_fetch", "dcn_anchor_map_indels_genotype"]


def test_symbols_are_declared_exported_and_bound(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    for name, n_args in zip(NAMES, (2, 3, 7, 11)):
        assert name in N.declared_symbols() and name in N._SIGNATURES and hasattr(L, name), name
        assert len(N._SIGNATURES[name][1]) == n_args
    assert len(N.declared_symbols()) >= 107
    assert tuple(N.ABI) >= (1, 21)
    major, minor = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(major), C.byref(minor)) == 0 and (major.value, minor.value) >= (1, 21)
    header = open(N.HEADER_PATH).read()
    assert len(re.findall(r"1\.21 = dcn_anchor_map_pileup_keep_deletions, dcn_anchor_map_deletions_info / _fetch, dcn_anchor_map_indels_genotype\.", header)) == 1
    assert int(re.search(r"#define DCN_ABI_MINOR (\d+)", header).group(1)) >= 21
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"pub const DCN_ABI_MINOR: u32 = (\d+); +//", md).group(1)) >= 21
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, md), name
    for struct in ("dcn_deletion", "dcn_indel_params", "dcn_indel_site"):
        assert "pub struct %s {" % struct in md, struct
    for method in ("pileup_keep_deletions", "deletions_info", "deletions_fetch", "indels_genotype"):
        assert callable(getattr(dcn.AnchorMap, method))
    sig = inspect.signature(dcn.AnchorMap.indels_genotype).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("record", inspect.Parameter.empty), ("start", 0), ("n", None), ("ploidy", 2), ("min_depth", 3),
                                                           ("min_gq", 20), ("min_qual", 20), ("min_count", 2), ("indel_centi", 2000), ("het_centi", 301)]
    assert [(k, v.default) for k, v in inspect.signature(dcn.AnchorMap.deletions_fetch).parameters.items()][1:] == [
        ("record", inspect.Parameter.empty), ("start", 0), ("n", None)]
    assert [(k, v.default) for k, v in inspect.signature(dcn.AnchorMap.pileup_keep_deletions).parameters.items()][1:] == [("keep", True)]
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "DCN_DELETION_LEDGER_EVENTS" in readme and "deacon-hip indels" in readme and "107 entry points, ABI 1.21" in readme


def test_the_definitions_are_stated_once(dcn):
    flat = " ".join(open(dcn._native.HEADER_PATH).read().replace(" *", " ").split())
    assert flat.count("THE DEFINITION OF A DELETION LEDGER") == 1 and flat.count("THE DEFINITION OF AN INDEL GENOTYPE") == 1
    for i in range(1, 7):
        assert len(re.findall(r"\bR%d\." % i, flat)) == 1, i
    for i in range(1, 9):
        assert len(re.findall(r"\bI%d\." % i, flat)) == 1, i
    ledger = flat.split("THE DEFINITION OF A DELETION LEDGER")[1].split("THE DEFINITION OF AN INDEL GENOTYPE")[0]
    for words in ("p = ref_start + j is the position of the run's first D step", "DEL(q) equals the number of events with p <= q < p + len",
                  "the sum of all len is the DEL column's total", "A D run may be the first or the last run of a row",
                  "ascending p; then the shorter len; then reverse 0 before 1", "STARTS(p) is the number of events with that p", "ties go to the shorter",
                  "independent of the insertion ledger and of the quality sums"):
        assert words in ledger, words
    rule = flat.split("THE DEFINITION OF AN INDEL GENOTYPE")[1].split("#define DCN_DELETION_REVERSE")[0]
    for words in ("a = its count and e = INS(p)", "a = its count and e = STARTS(p)", "A candidate with a < max(1, min_count) is dropped",
                  "o = depth >= a ? depth - a : 0", "indel_centi a, het_centi (a + o), indel_centi o", "a gap has no base quality, so it is a constant",
                  "saturated at 2^32 - 1", "depth >= max(1, min_depth) and GQ >= min_gq", "a front insertion (L2), then the deletion, then an insertion behind",
                  "there are no multi-allelic indel records", "at the repeat's far end", "this is not normalised here",
                  "indel_centi = 2000, min_count = 2"):
        assert words in rule, words
    assert "16 bytes per event" in flat and "DCN_DELETION_LEDGER_EVENTS" in flat


DELETION_OFFSETS = dict(pos=0, len=8, flags=12)
PARAM_OFFSETS = dict(ploidy=0, min_depth=4, min_gq=8, min_qual=12, min_count=16, indel_centi=20, het_centi=24, reserved=28)
SITE_OFFSETS = dict(pos=0, bases_offset=8, len=16, flags=20, qual=24, depth=28, count=32, events=36, gt=40, gq=41, pl=42, reserved=45)


def test_struct_layout_agrees(tmp_path, dcn):
    N = dcn._native
    for ctype, dtype, offsets, size in ((N.Deletion, dcn.DELETION_DTYPE, DELETION_OFFSETS, 16), (N.IndelParams, None, PARAM_OFFSETS, 32),
                                        (N.IndelSite, dcn.INDEL_SITE_DTYPE, SITE_OFFSETS, 48)):
        assert C.sizeof(ctype) == size
        assert {f: getattr(ctype, f).offset for f, _ in ctype._fields_} == offsets and [f for f, _ in ctype._fields_] == list(offsets)
        if dtype is not None:
            assert dtype.itemsize == size and {f: dtype.fields[f][1] for f in dtype.names} == offsets and list(dtype.names) == list(offsets)
    assert (N.DELETION_REVERSE, N.INDEL_DELETION, N.INDEL_FRONT) == (1, 1, 2)
    checks = " && ".join(["offsetof(dcn_deletion, %s) == %d" % kv for kv in DELETION_OFFSETS.items()] +
                         ["offsetof(dcn_indel_params, %s) == %d" % kv for kv in PARAM_OFFSETS.items()] +
                         ["offsetof(dcn_indel_site, %s) == %d" % kv for kv in SITE_OFFSETS.items()])
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "deacon_hip.h"\n'
                   "int (*f0)(dcn_index *, int) = dcn_anchor_map_pileup_keep_deletions;\n"
                   "int (*f1)(const dcn_index *, uint64_t *, uint64_t *) = dcn_anchor_map_deletions_info;\n"
                   "int (*f2)(const dcn_index *, uint32_t, uint64_t, uint64_t, void *, uint64_t, uint64_t *) = dcn_anchor_map_deletions_fetch;\n"
                   "int (*f3)(const dcn_index *, const void *, uint32_t, uint64_t, uint64_t, void *, uint64_t, uint8_t *, uint64_t, uint64_t *,\n"
                   "          uint64_t *) = dcn_anchor_map_indels_genotype;\n"
                   "int main(void){ dcn_indel_params p = {2, 3, 20, 20, 2, 2000, 301, 0}; dcn_deletion d = {7, 3, DCN_DELETION_REVERSE};\n"
                   "  return sizeof p == 32 && sizeof d == 16 && sizeof(dcn_indel_site) == 48 && p.indel_centi == 2000 && d.len == 3 &&\n"
                   "         DCN_DELETION_REVERSE == 1u && DCN_INDEL_DELETION == 1u && DCN_INDEL_FRONT == 2u && DCN_ABI_MINOR >= 21 && " + checks + " ? 0 : 1; }\n")
    inc = os.path.dirname(N.HEADER_PATH)
    libdir = os.path.dirname(N.LIB_PATH)  # (the function pointers are initialised and never called)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(tmp_path / "t"), "-L", libdir,
                           "-ldeacon_hip", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"])
    assert subprocess.call([str(tmp_path / "t")]) == 0


def test_argument_errors_that_need_no_device(dcn):
    """in the order of the header: params NULL, reserved, ploidy, min_gq, indel_centi, het_centi, the two counts, then the map"""
    N, L = dcn._native, dcn._native.lib()
    n, m = C.c_uint64(77), C.c_uint64(78)
    for p, word in ((None, b"params is NULL"),
                    (N.IndelParams(3, 0, 100, 0, 0, 100001, 100001, 1), b"params.reserved must be 0"),
                    (N.IndelParams(3, 0, 100, 0, 0, 100001, 100001, 0), b"params.ploidy must be 1 or 2"),
                    (N.IndelParams(0, 0, 100, 0, 0, 100001, 100001, 0), b"params.ploidy must be 1 or 2"),
                    (N.IndelParams(2, 0, 100, 0, 0, 100001, 100001, 0), b"params.min_gq must be 0..99"),
                    (N.IndelParams(2, 0, 99, 0, 0, 100001, 100001, 0), b"params.indel_centi must be 0..100000"),
                    (N.IndelParams(2, 0, 99, 0, 0, 100000, 100001, 0), b"params.het_centi must be 0..100000"),
                    (N.IndelParams(2, 0xFFFFFFFF, 99, 0xFFFFFFFF, 0xFFFFFFFF, 100000, 100000, 0), b"map is NULL")):
        assert L.dcn_anchor_map_indels_genotype(None, None if p is None else C.byref(p), 0, 0, 1, None, 0, None, 0, C.byref(n), C.byref(m)) == N.DCN_ERR_ARG
        assert word in L.dcn_last_error(), (word, L.dcn_last_error())
    ok = N.IndelParams(2, 3, 20, 20, 2, 2000, 301, 0)
    assert L.dcn_anchor_map_indels_genotype(None, C.byref(ok), 0, 0, 1, None, 0, None, 0, None, C.byref(m)) == N.DCN_ERR_ARG
    assert b"n_sites/n_inserted is NULL" in L.dcn_last_error()
    assert (n.value, m.value) == (77, 78)  # (nothing is written by a refused call)
    assert L.dcn_anchor_map_deletions_fetch(None, 0, 0, 1, None, 0, None) == N.DCN_ERR_ARG and b"n_events is NULL" in L.dcn_last_error()
    for call in (lambda: L.dcn_anchor_map_pileup_keep_deletions(None, 1), lambda: L.dcn_anchor_map_pileup_keep_deletions(None, 0),
                 lambda: L.dcn_anchor_map_deletions_info(None, None, None), lambda: L.dcn_anchor_map_deletions_fetch(None, 0, 0, 1, None, 0, C.byref(n))):
        assert call() == N.DCN_ERR_ARG and b"map is NULL" in L.dcn_last_error()


def test_rules_on_the_host(tmp_path):
    """tests/cpp/indel_rule_test.cpp: dcn_indels.h's events, winner and decision under the address and undefined-behaviour
    sanitizers, as a program of its own"""
    exe = tmp_path / "indel_rule_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "deacon-server_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "indel_rule_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and re.search(r"indel rule ok: \d{6,} checks", out.stdout) and out.stderr == "", (out.stdout[-2000:], out.stderr[-2000:])


def test_the_shared_header_has_no_floating_point_and_no_device_only_code():
    src = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "dcn_indels.h")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\b(float|double)\b", code) and "hip/" not in code and "atomic" not in code and "__shfl" not in code


INDELS_ERRORS = [
    (["indels"], "the following required arguments were not provided: <REF>"),
    (["indels", "ref.fa"], "nothing to write: give at least one of -o <OUTPUT>, --variants <FILE>, --pileup <FILE>, --sites <FILE>, --vcf <FILE>, "
                           "--duplicates <FILE>, -s <SUMMARY>"),
    (["indels", "ref.fa", "--indel-qual", "30", "--min-indel-count", "1"],
     "nothing to write: give at least one of -o <OUTPUT>, --variants <FILE>, --pileup <FILE>, --sites <FILE>, --vcf <FILE>, --duplicates <FILE>, -s <SUMMARY>"),
    (["indels", "ref.fa", "--indel-qual"], "missing value for --indel-qual"),
    (["indels", "ref.fa", "--indel-qual", "1001"], "invalid value for --indel-qual: must be 0..1000"),
    (["indels", "ref.fa", "--indel-qual", "-1"], "invalid value for --indel-qual: must be 0..1000"),
    (["indels", "ref.fa", "--min-indel-count", "x"], "invalid value for --min-indel-count: must be 0..4294967295"),
    (["indels", "ref.fa", "--duplicates"], "missing value for --duplicates"),
    (["indels", "ref.fa", "--ploidy", "3"], "invalid value for --ploidy: must be 1..2"),
    (["indels", "ref.fa", "--min-gq", "100"], "invalid value for --min-gq: must be 0..99"),
    (["indels", "ref.fa", "--min-baseq", "256"], "invalid value for --min-baseq: must be 0..255"),
    (["indels", "ref.fa", "in1", "in2"], "indels takes one input: mates are independent here, run it once per file (unexpected argument 'in2')"),
    (["indels", "--nope"], "unexpected argument '--nope'"),
    (["indels", "ref.fa", "--paired"], "unexpected argument '--paired'"),
    (["indels", "ref.fa", "--verified-only"], "unexpected argument '--verified-only'"),
]


@pytest.mark.parametrize("args,message", INDELS_ERRORS, ids=[" ".join(e[0]) for e in INDELS_ERRORS])
def test_indels_error_exit_code_and_text(args, message):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "Error: " + message + "\n")


def test_indels_refuses_fasta_and_names_the_record(tmp_path):
    reads = tmp_path / "reads.fa"
    reads.write_text(">read7 some words\nACGTACGT\n")
    message = "Error: indels needs base qualities, and record 'read7' has none (FASTA): consensus takes reads without\n"
    p = subprocess.run([CLI, "indels", "ref.fa", str(reads), "--vcf", str(tmp_path / "v.vcf")], capture_output=True, text=True, timeout=60,
                       stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", message)


def test_indels_help_text():
    p = subprocess.run([CLI, "indels", "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "indels.txt")) as f:
        want = f.read()
    assert (p.returncode, p.stderr, p.stdout) == (0, "", want)
    for word in ("Usage: deacon-hip indels [OPTIONS] <REF> [READS]", "--indel-qual <Q>", "--min-indel-count <N>", "(0..1000) [default: 20, a convention]",
                 "[default: 2, a convention]", "INDEL;DP=depth;IDV=a;IEV=e GT:GQ:DP:AD:PL gt:gq:dp:o,a:pl", "FORMAT DP = o + a", "INFO INDEL, IDV and IEV",
                 "indel_qual, min_indel_count, deletion_events, deleted_bases,", "indel_sites, insertion_sites, deletion_sites, het_indel_sites and hom_indel_sites",
                 "no multi-allelic indel lines", "not\nleft-normalised", "the SNV line of a POS first", "are markdup's, byte for byte"):
        assert word in want, word
    # every option line of markdup's help is in it
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "markdup.txt")) as f:
        lines = [line for line in f.read().split("Options:\n")[1].split("\n\n")[0].split("\n") if re.match(r"^  (-\w,|   ) --?[\w-]+", line) and "--summary" not in line]
    assert len(lines) >= 30
    for line in lines:
        assert line in want, line
    top = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert (top.stdout + top.stderr).count("\n  indels ") == 1 and (top.stdout + top.stderr).count("\n  markdup ") == 1
    for sub in ("map", "verify", "align", "pileup", "extend", "consensus", "call", "genotype", "markdup"):  # the other modes do not know the two options
        for opt in ("--indel-qual", "--min-indel-count"):
            q = subprocess.run([CLI, sub, "ref.fa", opt, "1"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
            assert (q.returncode, q.stderr) == (1, "Error: unexpected argument '%s'\n" % opt)
        h = subprocess.run([CLI, sub, "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
        with open(os.path.join(ROOT, "tests", "golden", "cli_help", sub + ".txt")) as f:
            assert h.stdout == f.read(), sub  # their help texts do not change


# ---- the model alone: THE TESTS HERE THAT PASS WITHOUT THE FEATURE ---------------------------------------------------------
def runs(text):
    return AW.parse_cigar(text)


def test_model_alone_finds_what_the_differential_test_plants():
    """the seed of tests/test_gpu_indels_differential.py, checked here on the CPU: at least 8 deletion sites, 8 insertion sites
    and 3 sites each of gt 1 and gt 2 in the model's own output"""
    import test_gpu_indels_differential as DT
    DT.assert_planted(DT.piled_by_the_model())


def test_model_alone_on_events_written_out():
    """R2, R4, R5"""
    assert DW.deletion_events_of_runs(1000, 1, runs("3D10=2I1X4D5=1D")) == [(1000, 3, 1), (1014, 4, 1), (1023, 1, 1)]  # a D run first and last
    assert DW.deletion_events_of_runs(5, 0, runs("20=")) == [] and DW.deletion_events_of_runs(5, 0, runs("4I")) == []
    assert DW.deletion_events_of_runs(0, 0, runs("2I3=1D")) == [(3, 1, 0)]  # an I run does not move on T
    events = [(9, 2, 1), (7, 3, 0), (9, 2, 0), (9, 1, 1), (30, 1, 0)]
    assert DW.fetch_range(events, 0, 100) == [(7, 3, 0), (9, 1, 1), (9, 2, 0), (9, 2, 1), (30, 1, 0)]
    assert DW.fetch_range(events, 8, 2) == [(9, 1, 1), (9, 2, 0), (9, 2, 1)] and DW.fetch_range(events, 8, 1) == []  # by p alone: (7, 3) covers 8
    assert DW.deletion_winner([(9, 2, 0)] * 3 + [(9, 3, 0)] * 3) == (2, 3)  # a tie goes to the shorter
    assert DW.deletion_winner([(9, 2, 0)] * 3 + [(9, 3, 1)] * 4) == (3, 4)
    # the issue's own example: the DEL column cannot tell these apart, the ledger can
    a = [(100, 2, 0)] * 3
    b = [(100, 3, 0)] + [(101, 1, 0)] * 2
    column = lambda ev: [sum(p <= q < p + ln for p, ln, _ in ev) for q in range(99, 104)]  # noqa: E731
    assert column(a) == [0, 3, 3, 0, 0] and column(b) == [0, 1, 3, 1, 0] and DW.deletion_winner(a) == (2, 3)
    counts = np.zeros((110, 8), np.int64)
    counts[100:102, 5] = 3
    DW.assert_r2(counts, a, 110)
    with pytest.raises(AssertionError):
        DW.assert_r2(counts, b, 110)


def test_model_alone_on_decisions_written_out():
    """I2 - I5 at the defaults: costs in hundredths of a phred"""
    assert DW.costs(3, 3) == [6000, 1806, 6000] and DW.costs(3, 3, ploidy=1) == [6000, 6000]
    d = DW.decide(3, 6)
    assert (d["gt"], d["gq"], d["qual"], d["site"], d["pl"]) == (1, 41, 41, True, [41, 0, 41])
    d = DW.decide(7, 7)  # 14000, 2107, 0
    assert (d["gt"], d["gq"], d["qual"], d["site"], d["pl"]) == (2, 21, 140, True, [140, 21, 0])
    d = DW.decide(6, 6)  # 1806 / 100 = 18: under min_gq
    assert (d["gt"], d["gq"], d["site"]) == (2, 18, False) and DW.decide(6, 6, min_gq=18)["site"]
    assert DW.decide(2, 2, min_depth=3)["site"] is False and DW.decide(2, 2, min_depth=2, min_gq=6)["site"] is True
    assert DW.decide(1, 2, min_depth=1, min_gq=0, min_qual=0, indel_centi=100, het_centi=100)["gt"] == 0  # 100, 200, 100: the first in order
    assert DW.decide(1, 1, min_depth=1, min_gq=0, min_qual=0, indel_centi=100, het_centi=100)["gt"] == 2   # 100, 100, 0
    assert DW.decide(255, 255, ploidy=1, indel_centi=100)["pl"] == [255, 0, 0] and DW.decide(256, 256, ploidy=1, indel_centi=100)["pl"] == [255, 0, 0]
    assert DW.decide(254, 254, ploidy=1, indel_centi=100)["pl"] == [254, 0, 0]
    assert [DW.decide(a, a, ploidy=1, indel_centi=100)["gq"] for a in (98, 99, 100)] == [98, 99, 99]
    assert DW.decide(2 ** 32 - 1, 2 ** 32 - 1, ploidy=1, indel_centi=100000)["qual"] == 2 ** 32 - 1
    assert DW.decide(9, 4)["gt"] == 2  # a > depth: o is 0


def test_model_alone_on_sites_and_vcf_written_out():
    """I1, I6 and the tool's alleles on a 12-base record"""
    record = b"ACGTnACGTACG"
    counts = np.zeros((12, 8), np.int64)
    counts[:, 0] = 8
    counts[0, 6], counts[5, 6] = 8, 9
    ins = [(0, 1, 2, b"TT", 0)] * 8 + [(5, 0, 1, b"G", 0)] * 8 + [(5, 1, 3, b"CCC", 1)]
    dels = [(0, 2, 0)] * 8 + [(5, 1, 0)] * 3 + [(5, 4, 1)] * 4 + [(9, 3, 0)]
    sites = DW.sites_range(counts, ins, dels, 0, 12)
    assert [(s[0], s[1], s[2], s[3], s[6], s[7], s[8]) for s in sites] == [
        (0, DW.INDEL_FRONT, 2, b"TT", 8, 8, 2), (0, DW.INDEL_DELETION, 2, b"", 8, 8, 2),
        (5, DW.INDEL_DELETION, 4, b"", 4, 7, 1), (5, 0, 1, b"G", 8, 9, 2)]  # (9, 3) is one read: under min_count
    assert [s[0] for s in DW.sites_range(counts, ins, dels, 0, 12, min_count=1, min_depth=1, min_gq=0, min_qual=0, indel_centi=3000)] == [0, 0, 5, 5, 9]
    assert [s[1] for s in DW.sites_range(counts, None, dels, 0, 12)] == [DW.INDEL_DELETION] * 2 and len(DW.sites_range(counts, ins, None, 0, 12)) == 2
    assert DW.sites_range(counts, ins, dels, 1, 4) == [] and len(DW.sites_range(counts, ins, dels, 5, 1)) == 2
    ref = b"ACGTNACGTACG"
    assert [DW.indel_alleles(ref, s) for s in sites] == [(1, "A", "TTA"), (1, "ACG", "G"), (5, "NACGT", "N"), (6, "A", "AG")]
    assert DW.indel_alleles(ref, (5, DW.INDEL_FRONT, 3, b"CCC")) == (5, "N", "NCCC") and DW.indel_alleles(ref, (11, 0, 1, b"T")) == (12, "G", "GT")
    assert DW.indel_alleles(ref, (9, DW.INDEL_DELETION, 3, b"")) == (9, "TACG", "T")
    text = DW.vcf_text("0.0.0", ["r"], [record], [[(0, 50, 8, (0, 0, 8, 0), 5, 30, 0, (50, 30, 0, 0, 0, 0, 0, 0, 0, 0)), (5, 50, 8, (0, 0, 8, 0), 5, 30, 0, (50,) + (0,) * 9)]],
                       [sites])
    lines = text.split("\n")
    at = next(i for i, x in enumerate(lines) if x.startswith("##INFO=<ID=DP,"))
    assert lines[at + 1:at + 4] == DW.VCF_INDEL_HEADER and lines[at + 4].startswith("##FORMAT=<ID=GT,")
    body = [x.split("\t") for x in lines if x and not x.startswith("#")]
    assert [(x[1], x[3], x[4], x[7].split(";")[0]) for x in body] == [("1", "A", "G", "DP=8"), ("1", "A", "TTA", "INDEL"), ("1", "ACG", "G", "INDEL"),
                                                                     ("5", "NACGT", "N", "INDEL"), ("6", "A", "G", "DP=8"), ("6", "A", "AG", "INDEL")]
    assert body[1][7:] == ["INDEL;DP=8;IDV=8;IEV=8", "GT:GQ:DP:AD:PL", "1/1:24:8:0,8:160,24,0"]
    assert body[3][7:] == ["INDEL;DP=8;IDV=4;IEV=7", "GT:GQ:DP:AD:PL", "0/1:55:8:4,4:55,0,55"]
    one = DW.vcf_text("0.0.0", ["r"], [record], [[]], [DW.sites_range(counts, ins, dels, 0, 12, ploidy=1)], ploidy=1)
    assert [x.split("\t")[9] for x in one.split("\n") if x.startswith("r\t")][0] == "1:99:8:0,8:160,0"
