"""CPU checks of the strand surface (dcn_anchor_map_pileup_keep_strands / _fetch_strands, dcn_anchor_map_strand_evidence,
dcn_anchor_map_indels_strand): declared, exported and bound at ABI 1.23, the layout of the three structs in ctypes, numpy and
C99, the definition stated once, the argument errors that are found before a device is looked at and the order of the others
as the source spells it (tests/test_gpu_strand_seams.py provokes those on a map), `deacon-hip strand`'s --help and usage errors,
the rules of csrc/dcn_strand.h and rule S2's walk compiled for the host under the sanitizers, and the model of the GPU tests
(tests/_strand_worker.py) against the host program's rows and on cases whose answers are written out here.

The tests of the model alone, at the end, pass without the feature; every other test here needs it."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _align_worker as AW
import _strand_worker as SW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
NAMES = ["dcn_anchor_map_pileup_keep_strands", "dcn_anchor_map_pileup_fetch_strands", "dcn_anchor_map_strand_evidence", "dcn_anchor_map_indels_strand"]
PARAM_OFFSETS = dict(max_sb_centi=0, min_alt_strand=4, min_strand_depth=8, reserved=12)
QUERY_OFFSETS = dict(pos=0, kind=8, ref_code=12, alt_mask=16, count=20, count_reverse=24, reserved=28)
SITE_OFFSETS = dict(fwd=0, rev=16, table=32, sb_centi=48, flags=52, reserved=56)


def test_symbols_are_declared_exported_and_bound(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    for name, n_args in zip(NAMES, (2, 5, 6, 6)):
        assert name in N.declared_symbols() and name in N._SIGNATURES and hasattr(L, name), name
        assert len(N._SIGNATURES[name][1]) == n_args
    assert N._SIGNATURES[NAMES[0]] == N._SIGNATURES["dcn_anchor_map_pileup_keep_deletions"]          # the twins
    assert N._SIGNATURES[NAMES[1]] == N._SIGNATURES["dcn_anchor_map_pileup_fetch_qualities"]
    assert len(N.declared_symbols()) == 114
    assert tuple(N.ABI) >= (1, 23)
    major, minor = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(major), C.byref(minor)) == 0 and (major.value, minor.value) >= (1, 23)
    header = open(N.HEADER_PATH).read()
    assert len(re.findall(r"1\.23 = dcn_anchor_map_pileup_keep_strands / _fetch_strands, dcn_anchor_map_strand_evidence, dcn_anchor_map_indels_strand\.", header)) == 1
    assert int(re.search(r"#define DCN_ABI_MINOR (\d+)", header).group(1)) >= 23
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"pub const DCN_ABI_MINOR: u32 = (\d+); +//", md).group(1)) >= 23
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, md), name
    for struct in ("dcn_strand_params", "dcn_strand_query", "dcn_strand_site"):
        assert "pub struct %s {" % struct in md, struct
    assert "**1.23** `dcn_anchor_map_pileup_keep_strands`" in md and "### 3.15 Strand evidence" in md
    for method in ("pileup_keep_strands", "pileup_fetch_strands", "strand_evidence", "indels_strand", "genotype_strand", "indels_genotype_strand"):
        assert callable(getattr(dcn.AnchorMap, method))
    sig = inspect.signature(dcn.AnchorMap.strand_evidence).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("record", inspect.Parameter.empty), ("queries", inspect.Parameter.empty), ("max_sb_centi", 1083),
                                                           ("min_alt_strand", 1), ("min_strand_depth", 3)]
    assert [(k, v.default) for k, v in inspect.signature(dcn.AnchorMap.pileup_keep_strands).parameters.items()][1:] == [("keep", True)]
    assert [(k, v.default) for k, v in inspect.signature(dcn.AnchorMap.pileup_fetch_strands).parameters.items()][1:] == [
        ("record", inspect.Parameter.empty), ("start", 0), ("n", None)]
    geno = [(k, v.default) for k, v in inspect.signature(dcn.AnchorMap.genotype).parameters.items()]
    assert [(k, v.default) for k, v in inspect.signature(dcn.AnchorMap.genotype_strand).parameters.items()] == geno + [
        ("max_sb_centi", 1083), ("min_alt_strand", 1), ("min_strand_depth", 3)]
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "deacon-hip strand" in readme and "114 entry points, ABI 1.23" in readme and "strand.hip" in readme and "profiles/strand_rate.txt" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Strand evidence (ABI 1.23)" in design and "four reverse planes and not eight" in design
    makefile = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "Makefile")).read()
    assert " strand.hip " in makefile and " strand_api.hip " in makefile and " dcn_strand.h " in makefile


def test_the_definition_is_stated_once(dcn):
    flat = " ".join(open(dcn._native.HEADER_PATH).read().replace(" *", " ").split())
    assert flat.count("THE DEFINITION OF STRAND EVIDENCE") == 1
    for i in range(1, 9):
        assert len(re.findall(r"\bS%d\." % i, flat)) == 1, i
    rule = flat.split("THE DEFINITION OF STRAND EVIDENCE")[1].split("#define DCN_STRAND_BIAS")[0]
    for words in ("Rules P1-P6, Q1-Q6, L1-L8, R1-R6, G1-G8 and I1-I8 stand", "four more uint32_t counters per kept base, RA RC RG RT", "They cost 16 bytes per base",
                  "-DDCN_PILEUP_POSITION_MAJOR", "once a row has added since the pileup was enabled or last reset (L1's rule)", "dcn_index_memory does not count them",
                  "every '=' or X step of a row with reverse = 1 also adds 1 to R[c] at that position", "P3's, or with qualities Q3's",
                  "a base that counts as N (an invalid base, a base under min_base_qual) adds to no plane", "neither do D and I runs",
                  "R[c] <= n[c] everywhere, F[c] = n[c] - R[c] is the forward count", "RA + RC + RG + RT <= REV", "The adds commute (P5)",
                  "Left alignment (N8) applies first", "a = F[ref], b = R[ref], c = the sum of F[x] over x in ALT, d = the same sum of R[x]",
                  "d = a_rev; c = a_all - a_rev; b = REV(p) >= d ? REV(p) - d : 0", "every read there that does not carry the allele",
                  "in hundredths of a chi-square with one degree of freedom", "s = 0 when m < 1024 and (the bit length of m) - 10 otherwise",
                  "GATK shrinks large tables the same way", "If r1 r2 c1 c2 = 0 the score is 0", "sb_centi = min(65535, 100 N (ad - bc)^2 / (r1 r2 c1 c2))",
                  "so the numerator stays below", "2^40 = 2^59, and the denominator below 2^44", "DCN_STRAND_BIAS when max_sb_centi > 0 and sb_centi >= max_sb_centi",
                  "min(c, d) < min_alt_strand and both a + c and b + d are at least min_strand_depth", "This flag uses the unshifted table", "A site with no flag passes",
                  "A hom-alt site has an empty reference row and scores 0", "There is no Yates correction and no exact test", "Only the winner of each indel kind is counted",
                  "max_sb_centi = 1083 is a convention, not a measured optimum", "chi-square 10.83, p = 0.001", "min_alt_strand = 1 and min_strand_depth = 3 are conventions",
                  "The result is unique while no counter has wrapped"):
        assert words in rule, words
    assert "not one memory operation more on a forward row" in flat and "exactly the launches and copies it issued before" in flat


def test_struct_layout_agrees(tmp_path, dcn):
    N = dcn._native
    for ctype, dtype, offsets, size in ((N.StrandParams, None, PARAM_OFFSETS, 16), (N.StrandQuery, dcn.STRAND_QUERY_DTYPE, QUERY_OFFSETS, 32),
                                        (N.StrandSite, dcn.STRAND_SITE_DTYPE, SITE_OFFSETS, 64)):
        assert C.sizeof(ctype) == size
        assert {f: getattr(ctype, f).offset for f, _ in ctype._fields_} == offsets and [f for f, _ in ctype._fields_] == list(offsets)
        if dtype is not None:
            assert dtype.itemsize == size and {f: dtype.fields[f][1] for f in dtype.names} == offsets and list(dtype.names) == list(offsets)
    assert (N.STRAND_BIAS, N.STRAND_ONE_SIDED) == (1, 2) == (dcn.STRAND_BIAS, dcn.STRAND_ONE_SIDED) == (SW.STRAND_BIAS, SW.STRAND_ONE_SIDED)
    checks = " && ".join(["offsetof(dcn_strand_params, %s) == %d" % kv for kv in PARAM_OFFSETS.items()] +
                         ["offsetof(dcn_strand_query, %s) == %d" % kv for kv in QUERY_OFFSETS.items()] +
                         ["offsetof(dcn_strand_site, %s) == %d" % kv for kv in SITE_OFFSETS.items()])
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "deacon_hip.h"\n'
                   "int (*f0)(dcn_index *, int) = dcn_anchor_map_pileup_keep_strands;\n"
                   "int (*f1)(const dcn_index *, uint32_t, uint64_t, uint64_t, uint32_t *) = dcn_anchor_map_pileup_fetch_strands;\n"
                   "int (*f2)(const dcn_index *, const void *, uint32_t, const void *, uint64_t, void *) = dcn_anchor_map_strand_evidence;\n"
                   "int (*f3)(const dcn_index *, uint32_t, const void *, uint64_t, const uint8_t *, uint32_t *) = dcn_anchor_map_indels_strand;\n"
                   "int main(void){ dcn_strand_params p = {1083, 1, 3, 0}; dcn_strand_query q = {7, 1, 0, 0, 5, 2, 0};\n"
                   "  return sizeof p == 16 && sizeof q == 32 && sizeof(dcn_strand_site) == 64 && p.max_sb_centi == 1083 && q.count_reverse == 2 &&\n"
                   "         DCN_STRAND_BIAS == 1u && DCN_STRAND_ONE_SIDED == 2u && DCN_ABI_MINOR >= 23 && " + checks + " ? 0 : 1; }\n")
    inc = os.path.dirname(N.HEADER_PATH)
    libdir = os.path.dirname(N.LIB_PATH)  # (the function pointers are initialised and never called)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(tmp_path / "t"), "-L", libdir,
                           "-ldeacon_hip", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"])
    assert subprocess.call([str(tmp_path / "t")]) == 0


def test_argument_errors_that_need_no_device(dcn):
    """params NULL, then reserved, then the map"""
    N, L = dcn._native, dcn._native.lib()
    out = N.StrandSite()
    q = N.StrandQuery(0, 2, 4, 0, 1, 2, 0)
    for p, word in ((None, b"params is NULL"), (N.StrandParams(1083, 1, 3, 1), b"params.reserved must be 0"),
                    (N.StrandParams(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0), b"map is NULL")):
        assert L.dcn_anchor_map_strand_evidence(None, None if p is None else C.byref(p), 0, C.byref(q), 1, C.byref(out)) == N.DCN_ERR_ARG
        assert word in L.dcn_last_error(), (word, L.dcn_last_error())
    assert list(out.table) == [0] * 4 and out.flags == 0  # (nothing is written by a refused call)
    for call in (lambda: L.dcn_anchor_map_pileup_keep_strands(None, 1), lambda: L.dcn_anchor_map_pileup_keep_strands(None, 0),
                 lambda: L.dcn_anchor_map_pileup_fetch_strands(None, 0, 0, 1, None), lambda: L.dcn_anchor_map_indels_strand(None, 0, None, 1, None, None)):
        assert call() == N.DCN_ERR_ARG and b"map is NULL" in L.dcn_last_error()


def test_the_order_of_the_other_errors_and_the_switch_off_from_the_source():
    """the checks of dcn_anchor_map_strand_evidence in the header's order; rule S1's refusal as the source spells it; and the
    promise that a map without planes launches what it launched: the strand launchers are behind `map->d_pileup_strands` alone"""
    api = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "strand_api.hip")).read()
    body = api.split('extern "C" int dcn_anchor_map_strand_evidence(')[1].split("\n}\n")[0]
    order = ['"params is NULL"', '"params.reserved must be 0"', "check_strands(map)", 'check_record(map, "strand evidence"', "if (n_queries == 0) return DCN_OK;",
             '"queries/out is NULL"', "is past the record's", '"kind must be 0 or 1"', '"ref_code must be 0..3"', '"alt_mask is empty"', '"alt_mask holds ref_code"',
             "is above count", "hipSetDevice", "dcn_launch_strand_evidence"]
    at = [body.index(x) for x in order]
    assert at == sorted(at)
    body = api.split('extern "C" int dcn_anchor_map_indels_strand(')[1].split("\n}\n")[0]
    assert "check_strands" not in body and "check_pileup(map)" in body  # it needs no planes
    pile = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "pileup_api.hip")).read()
    body = pile.split('extern "C" int dcn_anchor_map_pileup_keep_strands(dcn_index *map, int keep) {')[1].split("\n}\n")[0]
    assert "map->pileup_rows != 0" in body and "rows have added to the pileup since it was enabled or reset" in body
    assert "(dcn_anchor_map_pileup_reset first)" in body and "DCN_ERR_ARG" in body
    run = pile.split("int pileup_run(")[1].split("\n} // namespace")[0]
    assert run.count("d_pileup_strands") == 4 and run.count("if (map->d_pileup_strands)") == 2
    assert "else DCN_TRY(dcn_launch_pileup_qual(qa, st));" in run and "DCN_TRY(dcn_launch_pileup(pa, st));" in run
    kernels = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "pileup.hip")).read()
    assert "pileup_kernel<false, false>" in kernels and "pileup_kernel<true, false>" in kernels and "pileup_kernel<false, true>" in kernels and "pileup_kernel<true, true>" in kernels
    shared = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "dcn_pileup.h")).read()
    assert shared.count("if (column <= DCN_PILE_T) add_strand(column, j + q);") == 2
    for block in shared.split("if (reverse) {")[1:]:  # rule S2's add is inside the branch a forward row does not take
        assert "add_strand" in block.split("}")[0]


def host_program(tmp_path):
    exe = tmp_path / "strand_rule_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "deacon-server_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "strand_rule_test.cpp"), "-o", str(exe)])
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)


def test_rules_on_the_host_and_the_model_against_their_rows(tmp_path):
    """tests/cpp/strand_rule_test.cpp: dcn_strand.h against a 128-bit brute force and hand-written rows, and rule S2's walk,
    under the address and undefined-behaviour sanitizers, as a program of its own; then every table it printed through the
    Python model, which shares nothing with either"""
    out = host_program(tmp_path)
    assert out.returncode == 0 and out.stderr == "", (out.stdout[-2000:], out.stderr[-2000:])
    m = re.search(r"strand rule ok: (\d+) tables, (\d+) run lists, (\d+) plane adds", out.stdout)
    assert m and int(m.group(1)) >= 8000 and int(m.group(2)) >= 3000 and int(m.group(3)) >= 100_000
    assert SW.check_rule_rows(out.stdout.splitlines()) == int(m.group(1))


def test_the_shared_header_has_no_floating_point_no_device_only_code_and_no_runtime_index():
    src = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "dcn_strand.h")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\b(float|double)\b", code) and "hip/" not in code and "atomic" not in code and "__shfl" not in code
    assert "[" not in code  # nothing is indexed at all: the four columns are four scalars
    assert "2^59" in src


STRAND_ERRORS = [
    (["strand"], "the following required arguments were not provided: <REF>"),
    (["strand", "ref.fa"], "nothing to write: give at least one of -o <OUTPUT>, --variants <FILE>, --pileup <FILE>, --sites <FILE>, --vcf <FILE>, "
                           "--duplicates <FILE>, -s <SUMMARY>"),
    (["strand", "ref.fa", "--max-sb"], "missing value for --max-sb"),
    (["strand", "ref.fa", "--max-sb", "65536"], "invalid value for --max-sb: must be 0..65535"),
    (["strand", "ref.fa", "--max-sb", "-1"], "invalid value for --max-sb: must be 0..65535"),
    (["strand", "ref.fa", "--min-alt-strand", "x"], "invalid value for --min-alt-strand: must be 0..4294967295"),
    (["strand", "ref.fa", "--min-strand-depth", "4294967296"], "invalid value for --min-strand-depth: must be 0..4294967295"),
    (["strand", "ref.fa", "--indel-qual", "1001"], "invalid value for --indel-qual: must be 0..1000"),
    (["strand", "ref.fa", "in1", "in2"], "strand takes one input: mates are independent here, run it once per file (unexpected argument 'in2')"),
    (["strand", "ref.fa", "--strand"], "unexpected argument '--strand'"),
]


@pytest.mark.parametrize("args,message", STRAND_ERRORS, ids=[" ".join(e[0]) for e in STRAND_ERRORS])
def test_strand_error_exit_code_and_text(args, message):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "Error: " + message + "\n")


def test_strand_refuses_fasta_and_names_the_record(tmp_path):
    reads = tmp_path / "reads.fa"
    reads.write_text(">read7 some words\nACGTACGT\n")
    message = "Error: strand needs base qualities, and record 'read7' has none (FASTA): consensus takes reads without\n"
    p = subprocess.run([CLI, "strand", "ref.fa", str(reads), "--vcf", str(tmp_path / "v.vcf")], capture_output=True, text=True, timeout=60,
                       stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", message)


def test_strand_help_text():
    p = subprocess.run([CLI, "strand", "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "strand.txt")) as f:
        want = f.read()
    assert (p.returncode, p.stderr, p.stdout) == (0, "", want)
    for word in ("Usage: deacon-hip strand [OPTIONS] <REF> [READS]", "\nStrand evidence: ", "--max-sb <N>", "--min-alt-strand <N>", "--min-strand-depth <N>",
                 "[default: 1083, a convention: chi-square 10.83, p = 0.001]", "rA rC rG rT", "strand_bias;one_strand", "Filtered lines are written, not dropped",
                 "ADF + ADR = AD field by field", "strand_bias_sites, one_strand_sites and filtered_sites", "the outputs are normalize's, byte for byte"):
        assert word in want, word
    # every line of normalize's help from its usage on is in it, in order, but for the three options: every option keeps its text
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "normalize.txt")) as f:
        normalize = f.read()
    tail = normalize[normalize.index("\nArguments:\n"):]
    mine = "\n".join(line for line in want.split("\n") if not re.match(r"^      (--max-sb|--min-alt-strand|--min-strand-depth) |^ {33}(the flag off|the site, gets FILTER)", line))
    assert tail in mine and mine.index("\nStrand evidence: ") == mine.index(tail) + len(tail)
    top = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert (top.stdout + top.stderr).count("\n  strand ") == 1 and (top.stdout + top.stderr).count("\n  normalize ") == 1
    for sub in ("map", "verify", "align", "pileup", "extend", "consensus", "call", "genotype", "markdup", "indels", "normalize", "map-pairs", "place", "mask",
                "classify"):
        if sub in ("map", "verify", "align", "pileup", "extend", "consensus", "call", "genotype", "markdup", "indels", "normalize"):
            for opt in ("--max-sb", "--min-alt-strand", "--min-strand-depth"):  # the other modes do not know the three options
                q = subprocess.run([CLI, sub, "ref.fa", opt, "1"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
                assert (q.returncode, q.stderr) == (1, "Error: unexpected argument '%s'\n" % opt)
        h = subprocess.run([CLI, sub, "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
        with open(os.path.join(ROOT, "tests", "golden", "cli_help", sub + ".txt")) as f:
            assert h.stdout == f.read(), sub  # the help texts of the older modes do not change


# ---- the model alone: THE TESTS HERE THAT PASS WITHOUT THE FEATURE ---------------------------------------------------------
def test_model_alone_on_tables_written_out():
    """S3 - S6; the same hand-written rows as tests/cpp/strand_rule_test.cpp gives the header"""
    assert SW.base_table([10, 20, 30, 40], [1, 2, 30, 0], 1, 0b1101) == (18, 2, 9 + 0 + 40, 1 + 30 + 0)
    assert SW.base_table([10, 20, 30, 40], [1, 2, 30, 0], 3, 0b0001) == (40, 0, 9, 1)
    assert SW.indel_table(20, 8, 6, 2) == (8, 6, 4, 2) and SW.indel_table(20, 1, 6, 2) == (15, 0, 4, 2)
    assert SW.indel_table(5, 2, 6, 1) == (0, 1, 5, 1) and SW.indel_table(2, 5, 1, 1) == (0, 4, 0, 1)
    for table, sb in (((0, 0, 7, 9), 0), ((5, 0, 5, 0), 0), ((5, 5, 5, 5), 0), ((10, 0, 0, 10), 2000), ((3, 3, 3, 0), 225), ((6, 6, 6, 1), 242),
                      ((1023, 0, 0, 1023), 65535), ((1024, 1024, 1, 1), 0), ((327, 0, 0, 328), 65500), ((328, 0, 0, 328), 65535),
                      ((2 ** 32 - 1,) * 4, 0), ((2 ** 32 - 1, 0, 0, 2 ** 32 - 1), 65535), ((30, 1030, 10, 30), 2703), ((0, 1060, 40, 0), 55000),
                      ((4, 3, 2, 0), 128), ((4, 3, 2, 1), 7)):
        assert SW.score(table) == sb, table
    assert SW.flags((6, 6, 6, 1), 242, 243) == 0 and SW.flags((6, 6, 6, 1), 242, 242) == SW.STRAND_BIAS and SW.flags((6, 6, 6, 1), 242, 0) == 0
    assert SW.flags((4, 3, 2, 0), 128, 0, 1, 3) == SW.STRAND_ONE_SIDED and SW.flags((4, 3, 2, 1), 7, 0, 1, 3) == 0 and SW.flags((4, 3, 2, 1), 7, 0, 2, 3) == SW.STRAND_ONE_SIDED
    assert SW.flags((4, 2, 2, 0), 88, 0, 1, 3) == 0 and SW.flags((0, 3, 2, 0), 500, 0, 1, 3) == 0 and SW.flags((1, 3, 2, 0), 300, 0, 1, 3) == SW.STRAND_ONE_SIDED
    assert SW.flags((10, 0, 0, 10), 2000) == SW.STRAND_BIAS | SW.STRAND_ONE_SIDED and SW.flags((7, 9, 0, 0), 0) == SW.STRAND_ONE_SIDED


def test_model_alone_piles_planes_by_rule_s2():
    """every run kind on both strands, an N and (through the masked copy) a low base"""
    runs = AW.parse_cigar("3=1X2D2=2I3=")
    S = b"ACGTNCAAGTN"  # (3 '=', 1 X, then N and C under '=', AA inserted, GTN)
    planes = np.zeros((20, 4), np.int64)
    assert SW.add_planes(planes, S, 5, 0, runs) == (11, 11) and not planes.any()          # a forward row adds nothing
    assert SW.add_planes(planes, S, 5, 1, runs) == (11, 11)
    want = np.zeros((20, 4), np.int64)
    for p, col in ((5, 0), (6, 1), (7, 2), (8, 3), (12, 1), (13, 2), (14, 3)):              # 9, 10: the D run; 11: N; 15: N; the I run: nothing
        want[p, col] = 1
    assert np.array_equal(planes, want)
    ins = [(7, 0, 2, b"AA", 1), (7, 0, 2, b"AA", 0), (7, 0, 2, b"AC", 1), (7, 1, 2, b"AA", 1), (8, 0, 2, b"AA", 1)]
    dels = [(7, 2, 1), (7, 2, 1), (7, 3, 1), (7, 2, 0)]
    assert SW.count_reverse(ins, dels, (7, 0, 2, b"AA")) == 1 and SW.count_reverse(ins, dels, (7, 2, 2, b"AA")) == 1  # (flags 2: in front)
    assert SW.count_reverse(ins, dels, (7, 1, 2, b"")) == 2 and SW.count_reverse(ins, dels, (7, 1, 3, b"")) == 1 and SW.count_reverse(ins, dels, (9, 1, 2, b"")) == 0
    assert SW.genotype_queries([(5, 1, 0), (6, 2, 0), (7, 7, 1), (8, 4, 3)]) == [(5, 0, 0, 2, 0, 0), (6, 0, 0, 2, 0, 0), (7, 0, 1, 8, 0, 0), (8, 0, 3, 6, 0, 0)]
    assert SW.genotype_queries([(5, 2, 0)], ploidy=1) == [(5, 0, 0, 4, 0, 0)]
