"""CPU checks of the genotype surface (dcn_anchor_map_genotype): declared, exported and bound at ABI 1.19, the layout of its two
structs in ctypes and C99, the definition stated once, the argument errors that are found before a device is looked at, in
their order, `deacon-hip genotype`'s usage errors, its refusal of FASTA and its --help, the rule compiled for the host under
the sanitizers against a second formulation, and the model of the GPU tests (tests/_genotype_worker.py) alone on cases whose
answers are written out here."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

import _genotype_worker as GW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")


def test_symbol_is_declared_exported_and_bound(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    name = "dcn_anchor_map_genotype"
    assert name in N.declared_symbols() and name in N._SIGNATURES and hasattr(L, name)
    assert len(N._SIGNATURES[name][1]) == 10
    assert len(N.declared_symbols()) >= 99
    assert tuple(N.ABI) >= (1, 19)
    major, minor = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(major), C.byref(minor)) == 0 and (major.value, minor.value) >= (1, 19)
    header = open(N.HEADER_PATH).read()
    assert len(re.findall(r"1\.19 = dcn_anchor_map_genotype\.", header)) == 1
    assert int(re.search(r"#define DCN_ABI_MINOR (\d+)", header).group(1)) >= 19
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"pub const DCN_ABI_MINOR: u32 = (\d+); +//", md).group(1)) >= 19
    assert re.search(r"pub fn %s\(" % name, md)
    assert "pub struct dcn_genotype_params {" in md and "pub struct dcn_genotype_site {" in md
    sig = inspect.signature(dcn.AnchorMap.genotype).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("record", inspect.Parameter.empty), ("start", 0), ("n", None), ("ploidy", 2), ("min_depth", 3),
                                                           ("min_gq", 20), ("min_qual", 20), ("err_centi", 477), ("het_centi", 301)]
    assert dcn.GENOTYPE_NONE == N.GENOTYPE_NONE == 255 and list(dcn.GENOTYPES) == GW.names(2)
    for x in ("GENOTYPE_SITE_DTYPE", "GENOTYPE_NONE", "GENOTYPES"):
        assert getattr(dcn, x) is getattr(dcn.filter, x) and x in dcn.__all__


def test_the_definition_is_stated_once(dcn):
    flat = " ".join(open(dcn._native.HEADER_PATH).read().replace(" *", " ").split())
    assert flat.count("THE DEFINITION OF A GENOTYPE") == 1
    for i in range(1, 9):
        assert len(re.findall(r"\bG%d\." % i, flat)) == 1, i
        assert len(re.findall(r"\bL%d\." % i, flat)) == 1, i
    for i in range(1, 7):
        assert len(re.findall(r"\bQ%d\." % i, flat)) == 1, i
        assert len(re.findall(r"\bP%d\." % i, flat)) == 1, i
    assert flat.count("THE DEFINITION OF A QUALITY-AWARE PILEUP") == 1 and flat.count("THE DEFINITION OF A PILEUP") == 1
    assert flat.count("THE DEFINITION OF AN INSERTION LEDGER") == 1
    assert "AA, AC, CC, AG, CG, GG, AT, CT, GT, TT" in flat and "not measured optima" in flat.split("THE DEFINITION OF A GENOTYPE")[1].split("#define")[0]


SITE_OFFSETS = dict(pos=0, qual=8, depth=12, ad=16, gt=32, gq=33, ref_code=34, reserved0=35, pl=36, reserved1=46)
PARAM_OFFSETS = dict(ploidy=0, min_depth=4, min_gq=8, min_qual=12, err_centi=16, het_centi=20, reserved=24)


def test_struct_layouts_agree(tmp_path, dcn):
    N = dcn._native
    P, S = N.GenotypeParams, N.GenotypeSite
    assert C.sizeof(P) == 32 and C.sizeof(S) == 48
    assert {f: getattr(P, f).offset for f, _ in P._fields_} == PARAM_OFFSETS and [f for f, _ in P._fields_] == list(PARAM_OFFSETS)
    assert {f: getattr(S, f).offset for f, _ in S._fields_} == SITE_OFFSETS and [f for f, _ in S._fields_] == list(SITE_OFFSETS)
    dt = dcn.GENOTYPE_SITE_DTYPE
    assert dt.itemsize == 48 and {f: dt.fields[f][1] for f in dt.names} == SITE_OFFSETS
    checks = " && ".join(["offsetof(dcn_genotype_params, %s) == %d" % kv for kv in PARAM_OFFSETS.items()] +
                         ["offsetof(dcn_genotype_site, %s) == %d" % kv for kv in SITE_OFFSETS.items()])
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "deacon_hip.h"\n'
                   "int (*f)(const dcn_index *, const void *, uint32_t, uint64_t, uint64_t, uint8_t *, uint8_t *, void *, uint64_t, uint64_t *) =\n"
                   "    dcn_anchor_map_genotype;\n"
                   "int main(void){ dcn_genotype_params p = {2, 3, 20, 20, 477, 301, {0, 0}}; dcn_genotype_site s; s.pl[9] = 1;\n"
                   "  return sizeof p == 32 && sizeof s == 48 && sizeof s.pl == 10 && sizeof s.ad == 16 && p.het_centi == 301 && s.pl[9] == 1 &&\n"
                   "         DCN_GENOTYPE_NONE == 255 && DCN_ABI_MINOR >= 19 && " + checks + " ? 0 : 1; }\n")
    inc = os.path.dirname(N.HEADER_PATH)
    libdir = os.path.dirname(N.LIB_PATH)  # (the function pointer is initialised and never called)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(tmp_path / "t"), "-L", libdir,
                           "-ldeacon_hip", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"])
    assert subprocess.call([str(tmp_path / "t")]) == 0


def test_argument_errors_that_need_no_device(dcn):
    """in the order of the header: params NULL, reserved, ploidy, min_gq, err_centi, het_centi, then the map"""
    N, L = dcn._native, dcn._native.lib()

    def prm(ploidy=2, min_depth=3, min_gq=20, min_qual=20, err=477, het=301, reserved=(0, 0)):
        return C.byref(N.GenotypeParams(ploidy, min_depth, min_gq, min_qual, err, het, (C.c_uint32 * 2)(*reserved)))

    n_sites = C.c_uint64(77)
    for p, word in ((None, b"params is NULL"),
                    (prm(ploidy=3, min_gq=100, err=100001, het=100001, reserved=(0, 1)), b"params.reserved must be 0"),
                    (prm(reserved=(1, 0)), b"params.reserved must be 0"),
                    (prm(ploidy=0, min_gq=100, err=100001, het=100001), b"params.ploidy must be 1 or 2"),
                    (prm(ploidy=3), b"params.ploidy must be 1 or 2"),
                    (prm(min_gq=100, err=100001, het=100001), b"params.min_gq must be 0..99"),
                    (prm(err=100001, het=100001), b"params.err_centi must be 0..100000"),
                    (prm(het=100001), b"params.het_centi must be 0..100000"),
                    (prm(ploidy=1, min_depth=2 ** 32 - 1, min_gq=99, min_qual=2 ** 32 - 1, err=100000, het=100000), b"map is NULL"),
                    (prm(), b"map is NULL")):
        assert L.dcn_anchor_map_genotype(None, p, 0, 0, 1, None, None, None, 0, C.byref(n_sites)) == N.DCN_ERR_ARG
        assert word in L.dcn_last_error(), (word, L.dcn_last_error())
    assert n_sites.value == 77  # (nothing is written by a refused call)
    message = L.dcn_last_error()
    calls = (C.c_uint8 * 4)()
    assert L.dcn_anchor_map_pileup_call(None, C.byref(N.PileupCallParams(3, 500, (C.c_uint32 * 2)(0, 0))), 0, 0, 1, calls, None, None, 0,
                                        C.byref(n_sites)) == N.DCN_ERR_ARG and L.dcn_last_error() == message


def test_rule_on_the_host(tmp_path):
    """tests/cpp/genotype_rule_test.cpp: dcn_genotype.h's function against every count vector with D <= 6 expanded into
    observations with costs of their own, and 100,000 random vectors up to 2^32 - 1 in 128 bits, under the address and
    undefined-behaviour sanitizers, pl between guard bytes"""
    exe = tmp_path / "genotype_rule_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "deacon-server_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "genotype_rule_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "genotype rule ok: 210 count vectors, 50400 small cases, 100002 large cases, QUAL saturated" in out.stdout, \
        (out.stdout[-2000:], out.stderr[-2000:])


def test_the_shared_header_has_no_floating_point_and_divides_by_100_only(dcn):
    src = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "dcn_genotype.h")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\b(float|double)\b", code)
    assert set(re.findall(r"/\s*([^\s;)]+)", code)) == {"100u"} and "%" not in code


GENOTYPE_ERRORS = [
    (["genotype"], "the following required arguments were not provided: <REF>"),
    (["genotype", "ref.fa"], "nothing to write: give at least one of -o <OUTPUT>, --variants <FILE>, --pileup <FILE>, --sites <FILE>, --vcf <FILE>, -s <SUMMARY>"),
    (["genotype", "ref.fa", "--ploidy", "0"], "invalid value for --ploidy: must be 1..2"),
    (["genotype", "ref.fa", "--ploidy", "3"], "invalid value for --ploidy: must be 1..2"),
    (["genotype", "ref.fa", "--min-gq", "100"], "invalid value for --min-gq: must be 0..99"),
    (["genotype", "ref.fa", "--min-qual", "-1"], "invalid value for --min-qual: must be 0..4294967295"),
    (["genotype", "ref.fa", "--vcf"], "missing value for --vcf"),
    (["genotype", "ref.fa", "--sample"], "missing value for --sample"),
    (["genotype", "ref.fa", "--min-baseq", "256"], "invalid value for --min-baseq: must be 0..255"),
    (["genotype", "ref.fa", "--min-frac", "1001"], "invalid value for --min-frac: must be 0..1000"),
    (["genotype", "ref.fa", "in1", "in2"], "genotype takes one input: mates are independent here, run it once per file (unexpected argument 'in2')"),
    (["genotype", "--nope"], "unexpected argument '--nope'"),
    (["genotype", "ref.fa", "--verified-only"], "unexpected argument '--verified-only'"),
]


@pytest.mark.parametrize("args,message", GENOTYPE_ERRORS, ids=[" ".join(e[0]) for e in GENOTYPE_ERRORS])
def test_genotype_error_exit_code_and_text(args, message):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "Error: " + message + "\n")


def test_genotype_refuses_fasta_and_names_the_record(tmp_path):
    reads = tmp_path / "reads.fa"
    reads.write_text(">read7 some words\nACGTACGT\n")
    message = "Error: genotype needs base qualities, and record 'read7' has none (FASTA): consensus takes reads without\n"
    p = subprocess.run([CLI, "genotype", "ref.fa", str(reads), "--vcf", "-"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", message)
    p = subprocess.run([CLI, "genotype", "ref.fa", "--vcf", "-"], capture_output=True, text=True, timeout=60, input=reads.read_text())
    assert (p.returncode, p.stdout, p.stderr) == (1, "", message)


def test_genotype_help_text():
    p = subprocess.run([CLI, "genotype", "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "genotype.txt")) as f:
        want = f.read()
    assert (p.returncode, p.stderr, p.stdout) == (0, "", want)
    for word in ("Usage: deacon-hip genotype [OPTIONS] <REF> [READS]", "--vcf <FILE>", "--ploidy <1|2>", "--min-gq <N>", "--min-qual <N>", "--sample <NAME>",
                 "[default: 20, a convention]", "[default: sample]", "SNVs only", "insertions and deletions stay", "in --variants", "not measured optima",
                 "genotyped_positions, vcf_sites, het_sites and hom_alt_sites", "--min-baseq <Q>", "--variants <FILE>", "--pileup <FILE>", "--sites <FILE>"):
        assert word in want, word
    top = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert (top.stdout + top.stderr).count("\n  genotype ") == 1 and (top.stdout + top.stderr).count("\n  call ") == 1
    for sub in ("map", "verify", "align", "pileup", "extend", "consensus", "call"):  # the other modes do not know genotype's options
        for opt in ("--vcf", "--ploidy", "--min-gq", "--min-qual", "--sample"):
            q = subprocess.run([CLI, sub, "ref.fa", opt, "1"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
            assert (q.returncode, q.stderr) == (1, "Error: unexpected argument '%s'\n" % opt)


# ---- the model alone: THE TESTS HERE THAT PASS WITHOUT THE FEATURE ---------------------------------------------------------
def test_model_alone_on_cases_written_out():
    """defaults and reference A unless said"""
    names = GW.names(2)
    d = GW.decide([10, 0, 0, 0], [300, 0, 0, 0], 0)
    assert names[d["best"]] == "AA" and d["gq"] == 30 and d["gt"] == 0 and not d["site"] and d["qual"] == 0
    assert [d["pl"][names.index(g)] for g in ("AC", "AG", "AT")] == [30, 30, 30]
    assert all(d["pl"][g] == 255 for g, nm in enumerate(names) if "A" not in nm) and d["pl"][0] == 0
    d = GW.decide([5, 5, 0, 0], [150, 150, 0, 0], 0)
    assert names[d["best"]] == "AC" and d["costs"][names.index("AC")] == 3010 and d["costs"][names.index("AA")] == d["costs"][names.index("CC")] == 17385
    assert d["gq"] == 99 and d["qual"] == 143 and d["site"] and d["gt"] == 1
    d = GW.decide([9, 1, 0, 0], [270, 30, 0, 0], 0)
    assert names[d["best"]] == "AC" and d["costs"][1] == 3010 and d["costs"][0] == 3477 and d["gq"] == 4 and d["gt"] == GW.NONE
    assert GW.decide([9, 1, 0, 0], [270, 30, 0, 0], 0, min_gq=4)["gt"] == 1 and GW.decide([9, 1, 0, 0], [270, 30, 0, 0], 0, min_gq=5)["gt"] == GW.NONE
    d = GW.decide([19, 1, 0, 0], [570, 30, 0, 0], 0)
    assert names[d["best"]] == "AA" and d["costs"][0] == 3477 and d["costs"][1] == 6020 and d["gq"] == 25 and d["gt"] == 0 and not d["site"]
    d = GW.decide([0, 0, 0, 0], [0, 0, 0, 0], 0)
    assert d["gt"] == GW.NONE and d["gq"] == 0 and not d["site"] and d["pl"] == [0] * 10
    assert GW.decide([0, 0, 0, 0], [0, 0, 0, 0], 0, min_depth=0)["gt"] == GW.NONE  # D >= max(1, min_depth)
    d = GW.decide([3, 0, 0, 0], [0, 0, 0, 0], 0, err_centi=0)
    # the four homozygotes tie at cost 0 (and with them the heterozygotes without A, which explain nothing and pay nothing)
    assert [names[g] for g, c in enumerate(d["costs"]) if c == 0] == ["AA", "CC", "CG", "GG", "CT", "GT", "TT"] and d["costs"][1] == 903
    assert d["best"] == 0 and d["gq"] == 0
    # an invalid reference base: the genotype is reported, QUAL is 0, never a site
    d = GW.decide([0, 10, 0, 0], [0, 300, 0, 0], 4, min_qual=0)
    assert names[d["best"]] == "CC" and d["gt"] == 2 and d["gq"] == 30 and d["qual"] == 0 and not d["site"]
    assert GW.decide([0, 10, 0, 0], [0, 300, 0, 0], 0)["site"] and GW.decide([0, 10, 0, 0], [0, 300, 0, 0], 0)["qual"] == 347


def test_model_alone_at_ploidy_one_written_out():
    names = GW.names(1)
    assert names == ["A", "C", "G", "T"]
    d = GW.decide([10, 0, 0, 0], [300, 0, 0, 0], 0, ploidy=1)
    assert d["best"] == 0 and d["costs"] == [0, 34770, 34770, 34770] and d["gq"] == 99 and d["pl"] == [0, 255, 255, 255, 0, 0, 0, 0, 0, 0] and not d["site"]
    d = GW.decide([5, 5, 0, 0], [150, 150, 0, 0], 0, ploidy=1)
    assert d["costs"][:2] == [17385, 17385] and d["best"] == 0 and d["gq"] == 0 and d["gt"] == GW.NONE and not d["site"]  # a tie: A first
    d = GW.decide([9, 1, 0, 0], [270, 30, 0, 0], 0, ploidy=1)
    assert d["best"] == 0 and d["costs"][:2] == [3477, 31293] and d["gq"] == 99 and d["gt"] == 0
    d = GW.decide([1, 19, 0, 0], [30, 570, 0, 0], 0, ploidy=1)
    assert d["best"] == 1 and d["qual"] == (66063 - 3477) // 100 == 625 and d["site"] and d["gt"] == 1
    d = GW.decide([0, 0, 0, 0], [0, 0, 0, 0], 0, ploidy=1)
    assert d["gt"] == GW.NONE and d["gq"] == 0
    d = GW.decide([3, 0, 0, 0], [0, 0, 0, 0], 0, ploidy=1, err_centi=0)
    assert d["costs"] == [0, 0, 0, 0] and d["best"] == 0 and d["gq"] == 0
    d = GW.decide([0, 10, 0, 0], [0, 300, 0, 0], 4, ploidy=1, min_qual=0)
    assert d["best"] == 1 and d["qual"] == 0 and not d["site"]


def test_model_alone_on_vcf_lines_written_out():
    """(pos, qual, depth, ad, gt, gq, ref_code, pl) -> the line"""
    het = (41, 143, 12, (5, 5, 0, 0), 1, 99, 0, (143, 0, 143, 158, 158, 255, 158, 158, 255, 255))
    assert GW.vcf_line("chr1", het, 2) == "chr1\t42\t.\tA\tC\t143\tPASS\tDP=12\tGT:GQ:DP:AD:PL\t0/1:99:10:5,5:143,0,143"
    hom = (0, 347, 10, (0, 10, 0, 0), 2, 30, 0, (255, 30, 0, 255, 30, 255, 255, 30, 255, 255))
    assert GW.vcf_line("r", hom, 2) == "r\t1\t.\tA\tC\t347\tPASS\tDP=10\tGT:GQ:DP:AD:PL\t1/1:30:10:0,10:255,30,0"
    both = (9, 200, 10, (0, 5, 5, 0), 4, 99, 0, (255, 200, 150, 200, 0, 150, 255, 255, 255, 255))  # C/G on a reference A
    assert GW.vcf_line("r", both, 2) == "r\t10\t.\tA\tC,G\t200\tPASS\tDP=10\tGT:GQ:DP:AD:PL\t1/2:99:10:0,5,5:255,200,150,200,0,150"
    ref_t = (9, 200, 10, (5, 0, 0, 5), 6, 99, 3, (150, 255, 255, 255, 255, 255, 0, 255, 255, 150))  # A/T on a reference T: ALT A
    assert GW.vcf_line("r", ref_t, 2) == "r\t10\t.\tT\tA\t200\tPASS\tDP=10\tGT:GQ:DP:AD:PL\t0/1:99:10:5,5:150,0,150"
    hap = (9, 625, 20, (1, 19, 0, 0), 1, 99, 0, (255, 0, 255, 255, 0, 0, 0, 0, 0, 0))
    assert GW.vcf_line("r", hap, 1) == "r\t10\t.\tA\tC\t625\tPASS\tDP=20\tGT:GQ:DP:AD:PL\t1:99:20:1,19:255,0"
    text = GW.vcf_text("0.0.0", ["a", "b"], [b"ACGT", b"AC"], [[], [hom]], ploidy=2, sample="s1")
    lines = text.split("\n")
    assert lines[0] == "##fileformat=VCFv4.2" and lines[1] == "##source=deacon-hip 0.0.0"
    assert lines[2:4] == ["##contig=<ID=a,length=4>", "##contig=<ID=b,length=2>"] and lines[4].startswith("##INFO=<ID=DP,")
    assert [x[:16] for x in lines[5:10]] == ["##FORMAT=<ID=GT,", "##FORMAT=<ID=GQ,", "##FORMAT=<ID=DP,", "##FORMAT=<ID=AD,", "##FORMAT=<ID=PL,"]
    assert lines[10] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1" and lines[11].startswith("b\t1\t.\tA\tC\t") and lines[12:] == [""]
