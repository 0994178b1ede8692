"""CPU checks of the left-alignment surface (dcn_left_align_batch, dcn_anchor_map_pileup_left_align / _left_align_info):
declared, exported and bound at ABI 1.22, the layout of the info struct in ctypes, numpy and C99, the definition stated
once, the argument errors that are found before a device is looked at, in their order, rule N8's refusal as the source
spells it, `deacon-hip normalize`'s --help and usage errors, the procedure of csrc/dcn_left_align.h compiled for the host
under the sanitizers, and the model of the GPU tests (tests/_left_align_worker.py) alone: its own properties on seeded
random pairs, and cases whose answers are written out here.

The tests of the model alone, at the end, pass without the feature; every other test here needs it."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _align_worker as AW
import _left_align_worker as LW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
NAMES = ["dcn_left_align_batch", "dcn_anchor_map_pileup_left_align", "dcn_anchor_map_pileup_left_align_info"]
INFO_OFFSETS = dict(rows_aligned=0, rows_changed=8, gaps_shifted=16, columns_passed=24, gaps_merged=32)


def test_symbols_are_declared_exported_and_bound(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    for name, n_args in zip(NAMES, (14, 2, 2)):
        assert name in N.declared_symbols() and name in N._SIGNATURES and hasattr(L, name), name
        assert len(N._SIGNATURES[name][1]) == n_args
    assert N._SIGNATURES["dcn_left_align_batch"][1][:13] == N._SIGNATURES["dcn_align_batch"][1]  # its signature plus the info
    assert len(N.declared_symbols()) >= 110
    assert tuple(N.ABI) >= (1, 22)
    major, minor = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(major), C.byref(minor)) == 0 and (major.value, minor.value) >= (1, 22)
    header = open(N.HEADER_PATH).read()
    assert len(re.findall(r"1\.22 = dcn_left_align_batch, dcn_anchor_map_pileup_left_align / _left_align_info\.", header)) == 1
    assert int(re.search(r"#define DCN_ABI_MINOR (\d+)", header).group(1)) >= 22
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"pub const DCN_ABI_MINOR: u32 = (\d+); +//", md).group(1)) >= 22
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, md), name
    assert "pub struct dcn_left_align_info {" in md and "**1.22** `dcn_left_align_batch`" in md and "### 3.14 Left-aligned indels" in md
    assert callable(dcn.Placer.left_align_batch) and callable(dcn.AnchorMap.pileup_left_align) and callable(dcn.AnchorMap.pileup_left_align_info)
    assert [(k, v.default) for k, v in inspect.signature(dcn.Placer.left_align_batch).parameters.items()] == \
        [(k, v.default) for k, v in inspect.signature(dcn.Placer.align_batch).parameters.items()]
    assert [(k, v.default) for k, v in inspect.signature(dcn.AnchorMap.pileup_left_align).parameters.items()][1:] == [("on", True)]
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "deacon-hip normalize" in readme and "110 entry points, ABI 1.22" in readme and "left_align.hip" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Left-aligned indels (ABI 1.22)" in design
    makefile = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "Makefile")).read()
    assert " left_align.hip " in makefile and " dcn_left_align.h " in makefile


def test_the_definition_is_stated_once(dcn):
    flat = " ".join(open(dcn._native.HEADER_PATH).read().replace(" *", " ").split())
    assert flat.count("THE DEFINITION OF A LEFT-ALIGNED PLACEMENT") == 1
    for i in range(1, 9):
        assert len(re.findall(r"\bN%d\." % i, flat)) == 1, i
    rule = flat.split("THE DEFINITION OF A LEFT-ALIGNED PLACEMENT")[1].split("typedef struct dcn_left_align_info")[0]
    for words in ("A GAP is a maximal run of I or of D", "A gap is final before the next one is looked at",
                  "the step is allowed if T[j-1] EQUAL T[j+len-1] by rule 2", "an invalid base equals nothing, so such a column is never passed",
                  "not if that column is the row's first column", "After the step the gap covers T[j-1, j+len-1)", "keeps its op",
                  "allowed if S[i-1] EQUAL S[i+len-1] and the column is not the row's first", "After the step the gap covers S[i-1, i+len-1)",
                  "the comparison is on S as aligned", "A gap takes steps until none is allowed", "the two become one gap, which goes on taking steps with its new length",
                  "A gap directly behind a gap of the other kind stops", "A gap that A3 put first in the row stays first", "no step makes a gap first",
                  "the same multiset of column ops", "the same d, so it is still an optimal alignment", "n_ops <= 2 d + 1 still holds",
                  "n_ops may be larger or smaller than before", "A row without a gap is unchanged", "The procedure is idempotent and its result unique",
                  "not on lanes, chunking, trace groups or how a batch is cut", "Integers only",
                  "A row that begins inside a repeat cannot carry its gap past its own first column", "is stopped by the read's base, not by the record's",
                  "changes the switch only while no row has added since the pileup was enabled or reset"):
        assert words in rule, words
    assert "the message names dcn_anchor_map_pileup_reset" in flat and "40 bytes" in flat


def test_struct_layout_agrees(tmp_path, dcn):
    N = dcn._native
    assert C.sizeof(N.LeftAlignInfo) == 40
    assert {f: getattr(N.LeftAlignInfo, f).offset for f, _ in N.LeftAlignInfo._fields_} == INFO_OFFSETS and [f for f, _ in N.LeftAlignInfo._fields_] == list(INFO_OFFSETS)
    dt = dcn.LEFT_ALIGN_INFO_DTYPE
    assert dt.itemsize == 40 and {f: dt.fields[f][1] for f in dt.names} == INFO_OFFSETS and list(dt.names) == list(INFO_OFFSETS) == list(LW.INFO_FIELDS)
    checks = " && ".join("offsetof(dcn_left_align_info, %s) == %d" % kv for kv in INFO_OFFSETS.items())
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "deacon_hip.h"\n'
                   "int (*f0)(dcn_ctx *, const dcn_index *, const uint8_t *, const uint64_t *, uint32_t, const void *, const uint64_t *, const void *,\n"
                   "          uint64_t, uint32_t *, uint64_t *, uint32_t *, uint64_t, void *) = dcn_left_align_batch;\n"
                   "int (*f1)(dcn_index *, int) = dcn_anchor_map_pileup_left_align;\n"
                   "int (*f2)(const dcn_index *, void *) = dcn_anchor_map_pileup_left_align_info;\n"
                   "int main(void){ dcn_left_align_info i = {5, 4, 3, 2, 1};\n"
                   "  return sizeof i == 40 && i.rows_aligned == 5 && i.gaps_merged == 1 && DCN_ABI_MINOR >= 22 && " + checks + " ? 0 : 1; }\n")
    inc = os.path.dirname(N.HEADER_PATH)
    libdir = os.path.dirname(N.LIB_PATH)  # (the function pointers are initialised and never called)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(tmp_path / "t"), "-L", libdir,
                           "-ldeacon_hip", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"])
    assert subprocess.call([str(tmp_path / "t")]) == 0


def test_argument_errors_that_need_no_device(dcn):
    """dcn_align_batch's, in its order and with its messages; the info is zeroed by a refused call"""
    N, L = dcn._native, dcn._native.lib()
    offsets = (C.c_uint64 * 2)(0, 0)
    for p, word in ((None, None), (N.VerifyParams(1024, 0, 48, 0), None), (N.VerifyParams(10, 1001, 48, 0), None), (N.VerifyParams(10, 200, 47, 0), None),
                    (N.VerifyParams(10, 200, 48, 0), None)):
        info = N.LeftAlignInfo(9, 9, 9, 9, 9)
        args = (None, None, None, offsets, 1, None if p is None else C.byref(p), None, None, 1, None, None, None, 0)
        assert L.dcn_align_batch(*args) == N.DCN_ERR_ARG
        want = L.dcn_last_error()
        assert L.dcn_left_align_batch(*args, C.byref(info)) == N.DCN_ERR_ARG and L.dcn_last_error() == want and want
        assert [getattr(info, f) for f in INFO_OFFSETS] == [0] * 5
        assert L.dcn_left_align_batch(*args, None) == N.DCN_ERR_ARG and L.dcn_last_error() == want
    for call in (lambda: L.dcn_anchor_map_pileup_left_align(None, 1), lambda: L.dcn_anchor_map_pileup_left_align(None, 0),
                 lambda: L.dcn_anchor_map_pileup_left_align_info(None, None)):
        assert call() == N.DCN_ERR_ARG and b"map is NULL" in L.dcn_last_error()


def test_rule_n8_names_the_reset_and_off_adds_nothing():
    """the refusal's text, and the promise that a map without the switch issues no launch and no copy more, from the source"""
    api = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "pileup_api.hip")).read()
    body = api.split('extern "C" int dcn_anchor_map_pileup_left_align(dcn_index *map, int on) {')[1].split("\n}\n")[0]
    assert "map->pileup_rows != 0" in body and "rows have added to the pileup since it was enabled or reset" in body
    assert "(dcn_anchor_map_pileup_reset first)" in body and "DCN_ERR_ARG" in body
    assert "map->pileup_left_align ? &left : nullptr" in api
    runs = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "align_api.hip")).read()
    inside = runs.split("int dcn_align_runs(")[1].split("\nint dcn_align_gather_runs")[0]
    # every line that the pass adds to dcn_align_runs is under `if (left)`
    block = inside.split("    if (left) {")[1].split("\n    }\n")[0]
    assert "dcn_launch_left_align" in block and "d_aln_scratch" in block and "hipMemsetAsync" in block
    rest = inside.replace(block, "")
    assert "dcn_launch_left_align" not in rest and "d_aln_scratch" not in rest and rest.count("if (left)") == 2
    assert rest.index("dcn_launch_align(aa, st)") < rest.index("if (left) {") < rest.index("dcn_launch_offsets_scan")


def test_procedure_on_the_host(tmp_path):
    """tests/cpp/left_align_test.cpp: dcn_left_align.h's procedure against rules N1 - N5 taken literally, under the address
    and undefined-behaviour sanitizers, as a program of its own"""
    exe = tmp_path / "left_align_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "deacon-server_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "left_align_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and re.search(r"left align ok: \d{4,} rows, \d{4,} changed", out.stdout) and out.stderr == "", (out.stdout[-2000:], out.stderr[-2000:])


def test_the_shared_header_has_no_floating_point_and_no_device_only_code():
    src = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "dcn_left_align.h")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\b(float|double)\b", code) and "hip/" not in code and "atomic" not in code and "__shfl" not in code and "__ballot" not in code


NORMALIZE_ERRORS = [
    (["normalize"], "the following required arguments were not provided: <REF>"),
    (["normalize", "ref.fa"], "nothing to write: give at least one of -o <OUTPUT>, --variants <FILE>, --pileup <FILE>, --sites <FILE>, --vcf <FILE>, "
                              "--duplicates <FILE>, -s <SUMMARY>"),
    (["normalize", "ref.fa", "--indel-qual", "1001"], "invalid value for --indel-qual: must be 0..1000"),
    (["normalize", "ref.fa", "--min-indel-count", "x"], "invalid value for --min-indel-count: must be 0..4294967295"),
    (["normalize", "ref.fa", "in1", "in2"], "normalize takes one input: mates are independent here, run it once per file (unexpected argument 'in2')"),
    (["normalize", "ref.fa", "--left-align"], "unexpected argument '--left-align'"),
]


@pytest.mark.parametrize("args,message", NORMALIZE_ERRORS, ids=[" ".join(e[0]) for e in NORMALIZE_ERRORS])
def test_normalize_error_exit_code_and_text(args, message):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "Error: " + message + "\n")


def test_normalize_refuses_fasta_and_names_the_record(tmp_path):
    reads = tmp_path / "reads.fa"
    reads.write_text(">read7 some words\nACGTACGT\n")
    message = "Error: normalize needs base qualities, and record 'read7' has none (FASTA): consensus takes reads without\n"
    p = subprocess.run([CLI, "normalize", "ref.fa", str(reads), "--vcf", str(tmp_path / "v.vcf")], capture_output=True, text=True, timeout=60,
                       stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", message)


def test_normalize_help_text():
    p = subprocess.run([CLI, "normalize", "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "normalize.txt")) as f:
        want = f.read()
    assert (p.returncode, p.stderr, p.stdout) == (0, "", want)
    for word in ("Usage: deacon-hip normalize [OPTIONS] <REF> [READS]", "\nLeft alignment: ", "a deleted stretch moves one base while the base in front of it equals\nits last base",
                 "gaps of one kind\nthat meet become one", "##left_aligned", "left_aligned_rows", "left_aligned_gaps, left_align_columns", "left_align_merged_gaps",
                 "a read that begins inside a repeat cannot carry its gap in front of its own\nfirst base", "is stopped by the read's base there, not by the reference's",
                 "The text of a line is indels'"):
        assert word in want, word
    # every line of indels' help from its usage on is in it, in order: every option keeps its text
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "indels.txt")) as f:
        indels = f.read()
    tail = indels[indels.index("\nArguments:\n"):]
    assert tail in want and want.index("\nLeft alignment: ") == want.index(tail) + len(tail) - 1
    options = [line for line in indels.split("Options:\n")[1].split("\n\n")[0].split("\n") if re.match(r"^  (-\w,|   ) --?[\w-]+", line)]
    assert len(options) >= 35 and all(line in want for line in options)
    top = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert (top.stdout + top.stderr).count("\n  normalize ") == 1 and (top.stdout + top.stderr).count("\n  indels ") == 1
    for sub in ("map", "verify", "align", "pileup", "extend", "consensus", "call", "genotype", "markdup", "indels", "map-pairs", "place", "mask", "classify"):
        h = subprocess.run([CLI, sub, "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
        with open(os.path.join(ROOT, "tests", "golden", "cli_help", sub + ".txt")) as f:
            assert h.stdout == f.read(), sub  # the help texts of the older modes do not change


# ---- the model alone: THE TESTS HERE THAT PASS WITHOUT THE FEATURE ---------------------------------------------------------
def la(S, T, cigar):
    new, totals = LW.left_align(S, T, AW.parse_cigar(cigar))
    return AW.cigar_text(new), totals


def test_model_alone_on_cases_written_out():
    """one case per rule; the same pairs as tests/cpp/left_align_test.cpp gives the header's procedure"""
    assert la(b"GTCAAAGTTCAG", b"GTCAAAAGTTCAG", "6=1D6=") == ("3=1D9=", (1, 3, 0))          # N2: three steps, then C differs
    assert la(b"GTCAAAAAGTT", b"GTCAAAAGTT", "7=1I3=") == ("3=1I7=", (1, 4, 0))               # N3
    assert la(b"GGACACACTT", b"GGACACACACTT", "8=2D2=") == ("2=2D8=", (1, 6, 0))              # a unit of a period-2 repeat
    assert la(b"GGACTACTACTACTGA", b"GGACTACTACTGA", "11=3I2=") == ("2=3I11=", (1, 9, 0))     # ... of a period-3 repeat, inserted
    assert la(b"TCANAAG", b"TCANAAAG", "3=1X2=1D1=") == ("3=1X1D3=", (1, 2, 0))               # an invalid base of the record stops a D
    assert la(b"CANAAAG", b"CACAAG", "2=1X2=1I1=") == ("2=1X1I3=", (1, 2, 0))                 # ... of the read an I
    assert la(b"AAAC", b"AAAAC", "3=1D1=") == ("1=1D3=", (1, 2, 0))                           # the row's first column is not passed
    assert la(b"AAC", b"AAAC", "1D3=") == ("1D3=", (0, 0, 0))                                 # a gap that is first stays first
    assert la(b"GTCAAAG", b"GTAAAAAG", "2=1X3=1D1=") == ("2=1D1X4=", (1, 4, 0))               # an X column keeps its op
    assert la(b"GCATAAG", b"GCAAAAAC", "3=1X2=1D1X") == ("2=1D1=1X2=1X", (1, 4, 0))           # one run more
    assert la(b"GCAAATTG", b"GCAAAAATG", "5=1D1X2=") == ("2=1D3=1X2=", (1, 3, 0))
    assert la(b"CAAAAT", b"CGAAT", "1=1X2=1I1=") == ("1=1I1X3=", (1, 3, 0))                   # an I passes an X whose read base equals its last
    assert la(b"CGAGAAAT", b"CGTGAAT", "2=1X3=1I1=") == ("2=1X1=1I3=", (1, 2, 0))
    assert la(b"GCAAAT", b"GCAAAAAT", "2=1D2=1D2=") == ("2=2D4=", (1, 2, 1))                  # N4: two gaps become one
    assert la(b"GCAAAAAT", b"GCAAAT", "2=1I2=1I2=") == ("2=2I4=", (1, 2, 1))
    assert la(b"AAAT", b"AAAAAT", "1D2=1D2=") == ("2D4=", (1, 2, 1))                          # ... into a leading gap
    assert la(b"GCCCT", b"GACCT", "1=1D2=1I1=") == ("1=1D1I3=", (1, 2, 0))                    # behind the other kind: stops
    assert la(b"ACGT", b"ACGT", "4=") == ("4=", (0, 0, 0)) and la(b"", b"", "") == ("", (0, 0, 0))
    for steps in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129):  # a homopolymer: rule A3 leaves the gap at its far end (I7)
        T = b"GTC" + b"A" * (steps + 1) + b"GTTCAG"
        S = T[:3] + T[4:]
        d, runs = AW.align_pair(S, T)
        assert d == 1 and AW.cigar_text(runs) == "%d=1D6=" % (3 + steps)
        assert la(S, T, AW.cigar_text(runs)) == ("3=1D%d=" % (steps + 6), (1, steps, 0))


@pytest.mark.parametrize("letters", [b"A", b"AC", b"ACGT", b"ACN"])
def test_model_alone_keeps_its_promises_on_random_pairs(letters):
    """N4 - N6 on seeded random pairs with up to three planted edits: the columns match S and T, the cost is D[m][n], the op
    multiset is kept, I and D are never adjacent, no gap becomes first, a second application changes nothing"""
    rng = np.random.default_rng(2222 + len(letters))
    changed = 0
    for _ in range(1000):
        T = bytes(rng.choice(np.frombuffer(letters, np.uint8), int(rng.integers(1, 30))))
        S = bytearray(T)
        for _ in range(int(rng.integers(0, 4))):
            at, kind, ln = int(rng.integers(0, len(S) + 1)), int(rng.integers(0, 3)), int(rng.integers(1, 4))
            if kind == 0 and at < len(S):
                S[at] = int(rng.choice(np.frombuffer(letters, np.uint8)))
            elif kind == 1:
                del S[at:at + ln]
            else:
                S[at:at] = bytes(rng.choice(np.frombuffer(letters, np.uint8), ln))
        S = bytes(S)
        d, runs = AW.align_pair(S, T)
        new, totals = LW.left_align(S, T, runs)
        LW.check_properties(S, T, d, [int(x) for x in runs], new)
        assert (new != [int(x) for x in runs]) == (totals[1] > 0) and (totals[0] > 0) == (totals[1] > 0) and totals[1] >= totals[0]
        changed += totals[1] > 0
    assert changed >= (0 if letters == b"ACN" else 150), changed


def test_model_alone_finds_what_the_differential_test_plants():
    """the seed of tests/test_gpu_left_align_differential.py, checked here on the CPU"""
    import test_gpu_left_align_differential as DT
    DT.assert_planted(DT.piled_by_the_model())
