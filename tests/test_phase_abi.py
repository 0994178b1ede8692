"""CPU checks of the phase surface (dcn_anchor_map_phase_sites / _info / _links / _solve, dcn_phase_batch): declared in
include/deacon_hip_phase.h and not in deacon_hip.h, exported unmangled and bound in a table of their own at ABI 1.25; the
layout of the three structs in ctypes, numpy, C99 and INTEGRATION.md; the definition stated once; the argument errors that
are found before a device is looked at and the order of the others as the source spells it; the documents' pins; the rule
of csrc/dcn_phase.h compiled for the host under the sanitizers; and the model of the GPU tests (tests/_phase_worker.py) on
cases written out here.

The tests of the model alone, at the end, pass without the feature; every other test here needs it."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _phase_worker as HW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "deacon_hip_phase.h")
NAMES = sorted(["dcn_anchor_map_phase_sites", "dcn_anchor_map_phase_info", "dcn_phase_batch", "dcn_anchor_map_phase_links", "dcn_anchor_map_phase_solve"])
N_ARGS = dict(dcn_anchor_map_phase_sites=3, dcn_anchor_map_phase_info=2, dcn_phase_batch=13, dcn_anchor_map_phase_links=4, dcn_anchor_map_phase_solve=3)
SITE_OFFSETS = dict(pos=0, record=8, a0=12, a1=13, reserved=14)
PARAM_OFFSETS = dict(min_reads=0, max_minor_permille=4, reserved=8)
RESULT_OFFSETS = dict(set_pos=0, link=8, set_index=24, hap=28, flags=29, reserved=30)


def declared_in(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dcn_[a-z0-9_]+)\s*\(", text)))


def test_symbols_are_declared_exported_and_bound(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    assert declared_in(HEADER) == NAMES and N.PHASE_HEADER_PATH == HEADER
    assert sorted(N._PHASE_SIGNATURES) == NAMES
    assert not set(NAMES) & set(N._SIGNATURES) and not set(NAMES) & set(N._BLOCK_SIGNATURES) and not set(NAMES) & set(N.declared_symbols())
    assert len(N.declared_symbols()) == 114 and len(declared_in(N.BLOCKS_HEADER_PATH)) == 2  # the older headers declare what they declared
    for name in NAMES:
        assert hasattr(L, name) and len(N._PHASE_SIGNATURES[name][1]) == N_ARGS[name]
        assert getattr(N.lib(), name).argtypes == N._PHASE_SIGNATURES[name][1] and getattr(N.lib(), name).restype is C.c_int
    nm = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, timeout=60).stdout
    for name in NAMES:
        assert re.search(r" T %s$" % name, nm, re.M), name  # unmangled
    assert tuple(N.ABI) >= (1, 25)
    major, minor = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(major), C.byref(minor)) == 0 and (major.value, minor.value) >= (1, 25)
    main = open(N.HEADER_PATH).read()
    assert len(re.findall(r"1\.25 = dcn_anchor_map_phase_sites / _info / _links / _solve, dcn_phase_batch: declared in deacon_hip_phase\.h", main)) == 1
    assert int(re.search(r"#define DCN_ABI_MINOR (\d+)", main).group(1)) >= 25
    assert '#include "deacon_hip.h"' in open(HEADER).read()
    assert (dcn.PHASE_HEAD, dcn.PHASE_JOINED) == (N.PHASE_HEAD, N.PHASE_JOINED) == (HW.HEAD, HW.JOINED) == (1, 2)
    sig = lambda f: [(k, v.default) for k, v in inspect.signature(f).parameters.items()][1:]  # noqa: E731
    assert sig(dcn.AnchorMap.phase_sites) == [("sites", inspect.Parameter.empty)] and sig(dcn.AnchorMap.phase_info) == []
    assert sig(dcn.AnchorMap.phase_links) == [("first", 0), ("n", None)]
    assert sig(dcn.AnchorMap.phase_solve) == [("min_reads", 2), ("max_minor_permille", 200)]
    assert sig(dcn.Placer.phase_batch) == [("bases", inspect.Parameter.empty), ("offsets", inspect.Parameter.empty), ("rows", inspect.Parameter.empty),
                                           ("row_offsets", None), ("max_edits", 1023), ("max_permille", 200), ("select", None), ("quals", None),
                                           ("min_base_qual", 0), ("qual_offset", 33)]
    assert sig(dcn.Placer.phase_batch) == sig(dcn.Placer.pileup_batch)  # argument for argument


def test_the_definition_is_stated_once():
    flat = " ".join(open(HEADER).read().replace(" *", " ").split())
    assert flat.count("THE DEFINITION OF A PHASE") == 1
    for i in range(1, 11):
        assert len(re.findall(r"\bH%d\." % i, flat)) == 1, i
    rule = flat.split("THE DEFINITION OF A PHASE")[1].split("#ifndef DEACON_HIP_PHASE_H")[0]
    for words in ("A map holds at most one site list", "strictly ascending in (record, pos)", "a0 != a1 and both in A C G T (columns 0 .. 3)",
                  "Setting a list replaces the old one and zeroes all links; n = 0 frees it", "it has an alignment and n > 0",
                  "is the pileup column that P3 (with Q3, when qualities are given) would have incremented there for that row",
                  "otherwise NONE (another base, N, a base under min_base_qual, DEL)", "Inserted runs do not observe",
                  "the runs are N5's, exactly as for the pileup (N8)", "when both are of one record", "four 32-bit counters n[x][y]",
                  "A site with observation NONE does not bridge its neighbours", "Each row counts on its own", "The adds commute",
                  "c = n00 + n11, t = n01 + n10, N = c + t, minor = min(c, t), all in 64 bits",
                  "N >= max(1, min_reads), c != t and minor * 1000 <= N * max_minor_permille", "r = (t > c)",
                  "when s == 0, when link s - 1 does not exist (record change), or when link s - 1 is not joined",
                  "hap[head] = 0; hap[s] = hap[s - 1] XOR r[s - 1]", "Haplotype 1 carries a[hap], haplotype 2 a[1 - hap]",
                  "A set of one site is unphased", "unique while no counter has wrapped", "it is defined on the whole list",
                  "a false heterozygous site between two true ones splits a set", "No links across mates or across split rows",
                  "SNV sites only", "Per-read haplotype tags are not produced", "conventions, not measured optima"):
        assert " ".join(words.replace(" *", " ").split()) in rule, words  # (the comment's own " *" went with the products')
    for other_header in ("deacon_hip.h", "deacon_hip_blocks.h"):
        assert "THE DEFINITION OF A PHASE" not in " ".join(open(os.path.join(ROOT, "include", other_header)).read().split())


def test_struct_layout_agrees(tmp_path, dcn):
    N = dcn._native
    assert C.sizeof(N.PhaseParams) == 16 and {f: getattr(N.PhaseParams, f).offset for f, _ in N.PhaseParams._fields_} == PARAM_OFFSETS
    for dtype, offsets, size in ((dcn.PHASE_SITE_DTYPE, SITE_OFFSETS, 16), (dcn.PHASE_RESULT_DTYPE, RESULT_OFFSETS, 32)):
        assert dtype.itemsize == size and {f: dtype.fields[f][1] for f in dtype.names} == offsets and list(dtype.names) == list(offsets)
    assert dcn.PHASE_RESULT_DTYPE["link"].shape == (4,) and dcn.PHASE_RESULT_DTYPE["link"].base == np.uint32
    checks = " && ".join(["offsetof(dcn_phase_site, %s) == %d" % kv for kv in SITE_OFFSETS.items()] +
                         ["offsetof(dcn_phase_params, %s) == %d" % kv for kv in PARAM_OFFSETS.items()] +
                         ["offsetof(dcn_phase_result, %s) == %d" % kv for kv in RESULT_OFFSETS.items()])
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "deacon_hip_phase.h"\n'
                   "int (*f0)(dcn_index *, const void *, uint64_t) = dcn_anchor_map_phase_sites;\n"
                   "int (*f1)(const dcn_index *, uint64_t *) = dcn_anchor_map_phase_info;\n"
                   "int (*f2)(dcn_ctx *, dcn_index *, const uint8_t *, const uint8_t *, const uint64_t *, uint32_t, const void *, const void *,\n"
                   "          const uint64_t *, const void *, uint64_t, uint32_t *, uint64_t *) = dcn_phase_batch;\n"
                   "int (*f3)(const dcn_index *, uint64_t, uint64_t, uint32_t *) = dcn_anchor_map_phase_links;\n"
                   "int (*f4)(const dcn_index *, const void *, void *) = dcn_anchor_map_phase_solve;\n"
                   "int main(void){ dcn_phase_site s = {7, 1, 0, 3, {0, 0}}; dcn_phase_params p = {2, 200, {0, 0}};\n"
                   "  dcn_phase_result r = {9, {1, 2, 3, 4}, 5, 1, 3, {0, 0}};\n"
                   "  return sizeof s == 16 && sizeof p == 16 && sizeof r == 32 && s.a1 == 3 && p.max_minor_permille == 200 && r.link[3] == 4 &&\n"
                   "         r.flags == (DCN_PHASE_HEAD | DCN_PHASE_JOINED) && DCN_PHASE_HEAD == 1u && DCN_PHASE_JOINED == 2u &&\n"
                   "         DCN_ABI_MINOR >= 25 && " + checks + " ? 0 : 1; }\n")
    inc, libdir = os.path.dirname(HEADER), os.path.dirname(N.LIB_PATH)  # (the function pointers are initialised and never called)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(tmp_path / "t"), "-L", libdir,
                           "-ldeacon_hip", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"])
    assert subprocess.call([str(tmp_path / "t")]) == 0
    # the Rust structs of INTEGRATION.md: the fields in order, with the types of the C ones
    section = open(os.path.join(ROOT, "INTEGRATION.md")).read().split("### 3.17 Phase (1.25")[1]
    rust_of = {"uint32_t": "u32", "uint64_t": "u64", "uint8_t": "u8"}
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for struct, offsets in (("dcn_phase_site", SITE_OFFSETS), ("dcn_phase_params", PARAM_OFFSETS), ("dcn_phase_result", RESULT_OFFSETS)):
        c_fields = []
        for ctype, names in re.findall(r"(uint\d+_t)\s+([\w\[\], ]+);", header.split("typedef struct %s {" % struct)[1].split("}")[0]):
            for name in names.split(","):
                m = re.match(r"\s*(\w+)(?:\[(\d+)\])?", name)
                c_fields.append((m.group(1), "[%s; %s]" % (rust_of[ctype], m.group(2)) if m.group(2) else rust_of[ctype]))
        assert "#[repr(C)]\npub struct %s {" % struct in section
        body = section.split("pub struct %s {" % struct)[1].split("\n}")[0]
        rust_fields = re.findall(r"pub (\w+): ([\w\[\]; ]+),", body)
        assert [f for f, _ in c_fields] == list(offsets) == [f for f, _ in rust_fields]
        assert [t for _, t in rust_fields] == [t for _, t in c_fields]


def test_the_documents(dcn):
    import test_abi as TA
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert md.count('extern "C" {') == 2  # the new lines go into the second block of a binding: no third block here
    second = md.split('extern "C" {')[2].split("\n}\n")[0]
    assert sorted(re.findall(r"pub fn (dcn_\w+)\(", second)) == ["dcn_anchor_map_reference_blocks", "dcn_reference_blocks_merge"]
    assert "pub const DCN_ABI_MINOR: u32 = 25;  //" in md and "a binding that stops at reference blocks keeps `pub const DCN_ABI_MINOR: u32 = 24;`" in " ".join(md.replace("//", " ").split())
    assert "pub const DCN_ABI_MINOR: u32 = 7;" in md
    section = md.split("### 3.17 Phase (1.25")[1]
    rust = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (dcn_\w+)\(([^)]*)\)\s*->\s*c_int;", section)}
    assert sorted(rust) == NAMES
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        c_args = re.search(r"int %s\(([^)]*)\);" % name, header).group(1)
        c_types = [" ".join(a.split()).replace("info[4]", "*info") for a in c_args.split(",")]
        rust_types = [a.split(":", 1)[1].strip() for a in rust[name].split(",")]
        assert rust_types == [TA._rust_of_c(t) for t in c_types], (name, c_types, rust_types)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "114 entry points, ABI 1.23" in readme and "ABI 1.24" in readme and "ABI 1.25" in readme and "phase.hip" in readme and "deacon_hip_phase.h" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### Phase (ABI 1.25)" in design and "Reference blocks (ABI 1.24)" in design and "profiles/phase_rate.txt" in design
    makefile = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "Makefile")).read()
    assert " phase.hip " in makefile and " phase_api.hip " in makefile and " dcn_phase.h " in makefile and makefile.count("deacon_hip_phase.h") == 2


def test_argument_errors_that_need_no_device(dcn):
    """dcn_phase_batch: dcn_pileup_batch_qual's checks first, in its order and word for word; the solve's parameters in front
    of its map; the map calls: NULL"""
    N, L = dcn._native, dcn._native.lib()

    def prm(edits=1023, permille=200, stride=48, reserved=0):
        return C.byref(N.VerifyParams(edits, permille, stride, reserved))

    stand_in = (C.c_uint8 * 4096)()
    linking = C.c_uint64(77)
    bad_q = C.byref(N.PileupQualParams(999, 999, (C.c_uint32 * 2)(1, 1)))
    for args, word in (((None, None, None), b"params is NULL"), ((None, None, prm(reserved=1)), b"reserved"),
                       ((None, None, prm(edits=1024)), b"max_edits must be 0..1023"), ((None, None, prm(permille=1001)), b"max_permille must be 0..1000"),
                       ((None, None, prm(stride=40)), b"row_stride"), ((None, None, prm()), b"ctx is NULL"),
                       ((C.cast(stand_in, C.c_void_p), None, prm(stride=64)), b"map is NULL")):
        for qp in (None, bad_q):
            assert L.dcn_pileup_batch_qual(args[0], args[1], None, None, None, 0, args[2], qp, None, None, 0, None, C.byref(linking)) == N.DCN_ERR_ARG
            message = L.dcn_last_error()
            assert word in message, (word, message)
            assert L.dcn_phase_batch(args[0], args[1], None, None, None, 0, args[2], qp, None, None, 0, None, C.byref(linking)) == N.DCN_ERR_ARG
            assert L.dcn_last_error() == message
    assert linking.value == 77  # (nothing is written by a refused call)
    out = np.zeros(64, np.uint8)
    ptr = out.ctypes.data_as(C.c_void_p)
    for p, word in ((None, b"params is NULL"), (N.PhaseParams(2, 1001, (C.c_uint32 * 2)(0, 1)), b"params.reserved must be 0"),
                    (N.PhaseParams(2, 1001, (C.c_uint32 * 2)(0, 0)), b"params.max_minor_permille must be 0..1000"),
                    (N.PhaseParams(0, 1000, (C.c_uint32 * 2)(0, 0)), b"map is NULL"), (N.PhaseParams(2, 200, (C.c_uint32 * 2)(0, 0)), b"map is NULL")):
        assert L.dcn_anchor_map_phase_solve(None, None if p is None else C.byref(p), ptr) == N.DCN_ERR_ARG and word in L.dcn_last_error(), word
    for rc in (L.dcn_anchor_map_phase_sites(None, ptr, 1), L.dcn_anchor_map_phase_sites(None, None, 0), L.dcn_anchor_map_phase_info(None, ptr),
               L.dcn_anchor_map_phase_links(None, 0, 1, ptr)):
        assert rc == N.DCN_ERR_ARG and b"map is NULL" in L.dcn_last_error()
    assert not out.any()


def test_the_order_of_the_other_errors_from_the_source():
    api = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "phase_api.hip")).read()

    def body(name):
        return api.split('extern "C" int %s(' % name)[1].split("\n}\n")[0]

    for name, order in (("dcn_phase_batch", ["dcn_verify_walk(", '"the map has no phase sites', "dcn_align_check_rows(plan)", '"qual_params is NULL and quals is not',
                                             '"qual_params.reserved must be 0"', '"qual_params.qual_offset must be 0..255"', '"qual_params.min_base_qual must be 0..255"',
                                             '"quals is NULL and qual_params is not', "*n_linking = 0;", "if (plan.items.empty()) return DCN_OK;", "phase_run("]),
                        ("dcn_anchor_map_phase_sites", ["check_store(map)", "if (n_sites == 0)", '"sites is NULL"', "at most 4294967294 sites", '"reserved must be 0"',
                                                        '"record "', '"pos "', '"a0 and a1 must be 0..3', '"a0 and a1 are the same allele"', "does not lie behind", "dev_alloc(&l->d_base",
                                                        "l->n = n_sites;", "map->phase = l;"]),
                        ("dcn_anchor_map_phase_solve", ['"params is NULL"', '"params.reserved must be 0"', '"params.max_minor_permille must be 0..1000"', "check_list(map)",
                                                        '"results is NULL"', "hipSetDevice", "dcn_launch_phase_solve"]),
                        ("dcn_anchor_map_phase_links", ["check_list(map)", "are past the list's", "if (n == 0) return DCN_OK;", '"links is NULL"', "hipMemcpy"])):
        at = [body(name).index(x) for x in order]
        assert at == sorted(at), name
    pile = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "pileup_api.hip")).read()
    for message in ('"qual_params.reserved must be 0"', '"qual_params.qual_offset must be 0..255"', '"qual_params.min_base_qual must be 0..255"'):
        assert message in pile  # dcn_pileup_batch_qual's messages
    run = api.split("int phase_run(")[1].split("\n}\n")[0]
    assert "d_pileup" not in run and "ledger" not in run and "pileup_rows" not in run and "left_align_info" not in run  # nothing of a pileup is written


def test_the_shared_header_has_no_floating_point_and_no_device_only_code():
    src = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "dcn_phase.h")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\b(float|double)\b", code) and "hip/" not in code and "atomic" not in code and "__shfl" not in code
    kernels = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "phase.hip")).read()
    for reused in ("dcn_pile_column(", "dcn_pile_qual_column(", "dcn_pile_qual_pos(", "dcn_wf_side16<", "dcn_pile_step_s(", "dcn_pile_step_t("):
        assert reused in kernels, reused  # the pileup's own functions, reused and not restated
    for name in ("pileup.hip", "align.hip", "align_api.hip", "left_align.hip", "offsets_scan.hip"):
        assert "phase" not in open(os.path.join(ROOT, "deacon-server_amd", "csrc", name)).read().lower(), name  # the unchanged paths


def test_rules_on_the_host(tmp_path):
    """tests/cpp/phase_rule_test.cpp: dcn_phase.h's observation, its decision at every boundary, the scan operator's
    associativity by brute force and a blocked scan with block sizes 1 .. 9 against the sequential rule H6, under the address
    and undefined-behaviour sanitizers, as a program of its own"""
    exe = tmp_path / "phase_rule_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "deacon-server_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "phase_rule_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", (out.stdout[-2000:], out.stderr[-2000:])
    m = re.search(r"phase rule ok: (\d+) observations, (\d+) decisions, (\d+) bracketings, (\d+) blocked scans", out.stdout)
    assert m and int(m.group(1)) == 96 and int(m.group(2)) >= 600_000 and int(m.group(3)) >= 10_000 and int(m.group(4)) == 3600


# ---- the tool ---------------------------------------------------------------------------------------------------------------
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
PHASE_ERRORS = [
    (["phase"], "the following required arguments were not provided: <REF>"),
    (["phase", "ref.fa", "--vcf", "x.vcf"], "phase reads its input twice (the pile-up, then the links between the sites that were found): give a file, not stdin"),
    (["phase", "ref.fa", "-", "--vcf", "x.vcf"], "phase reads its input twice (the pile-up, then the links between the sites that were found): give a file, not stdin"),
    (["phase", "ref.fa", "reads.fq", "--ploidy", "1"], "phase needs --ploidy 2: a haploid genotype has no heterozygous site to phase"),
    (["phase", "ref.fa", "reads.fq"], "nothing to write: give at least one of -o <OUTPUT>, --variants <FILE>, --pileup <FILE>, --sites <FILE>, --vcf <FILE>, "
                                      "--gvcf <FILE>, --callable <FILE>, --phase-sets <FILE>, --links <FILE>, --duplicates <FILE>, -s <SUMMARY>"),
    (["phase", "ref.fa", "reads.fq", "--max-link-minor", "1001"], "invalid value for --max-link-minor: must be 0..1000"),
    (["phase", "ref.fa", "reads.fq", "--min-link-reads", "x"], "invalid value for --min-link-reads: must be 0..4294967295"),
    (["phase", "ref.fa", "reads.fq", "--links"], "missing value for --links"),
    (["gvcf", "ref.fa", "reads.fq", "--links", "x"], "unexpected argument '--links'"),
    (["strand", "ref.fa", "reads.fq", "--phase-sets", "x"], "unexpected argument '--phase-sets'"),
]


@pytest.mark.parametrize("args,message", PHASE_ERRORS, ids=[" ".join(e[0]) for e in PHASE_ERRORS])
def test_phase_error_exit_code_and_text(args, message):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "Error: " + message + "\n")


def test_phase_help_text_and_the_older_helps():
    p = subprocess.run([CLI, "phase", "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "phase.txt")) as f:
        want = f.read()
    assert (p.returncode, p.stderr, p.stdout) == (0, "", want)
    for word in ("Usage: deacon-hip phase [OPTIONS] <REF> [READS]", "\nPhase: ", "--min-link-reads <N>", "--max-link-minor <N>", "--phase-sets <FILE>", "--links <FILE>",
                 "[default: 2, a convention]", "[default: 200, a convention]", "GT g1|g2", "##FORMAT PS", "READS is read twice, so it cannot be stdin",
                 "phase_set_n50", "every other line is gvcf's, byte for byte"):
        assert word in want, word
    # every line of gvcf's help from its arguments on is in it, in order, but for the four options and the last paragraph
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "gvcf.txt")) as f:
        gvcf = f.read()
    tail = gvcf[gvcf.index("\nArguments:\n"):]
    mine = want.split("\n")
    first = next(i for i, x in enumerate(mine) if x.startswith("      --min-link-reads "))
    del mine[first:first + 8]
    mine = "\n".join(mine)
    assert tail in mine and mine.index("\nPhase: ") == mine.index(tail) + len(tail)
    top = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert (top.stdout + top.stderr).count("\n  phase ") == 1 and (top.stdout + top.stderr).count("\n  gvcf ") == 1
    for sub in ("map", "verify", "align", "pileup", "extend", "consensus", "call", "genotype", "markdup", "indels", "normalize", "strand", "gvcf",
                "map-pairs", "place", "mask", "classify"):
        h = subprocess.run([CLI, sub, "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
        with open(os.path.join(ROOT, "tests", "golden", "cli_help", sub + ".txt")) as f:
            assert h.stdout == f.read(), sub  # the help texts of the older modes do not change


# ---- the model alone: THE TESTS HERE THAT PASS WITHOUT THE FEATURE ---------------------------------------------------------
def test_model_alone_decisions_written_out():
    assert HW.decide([1, 0, 0, 0]) == (False, 0) and HW.decide([1, 0, 0, 1]) == (True, 0) and HW.decide([0, 1, 1, 0]) == (True, 1)
    assert HW.decide([8, 2, 0, 0]) == (True, 0) and HW.decide([7, 3, 0, 0]) == (False, 0) and HW.decide([8, 2, 0, 0], max_minor_permille=199) == (False, 0)
    assert HW.decide([3, 2, 1, 0], max_minor_permille=1000) == (False, 0) and HW.decide([1, 0, 0, 0], min_reads=0, max_minor_permille=0) == (True, 0)
    assert HW.decide([0, 0, 0, 0], min_reads=0, max_minor_permille=1000) == (False, 0) and HW.decide([2, 8, 0, 0]) == (True, 1)


def test_model_alone_observe_and_solve_written_out():
    sites = np.zeros(5, [("pos", np.uint64), ("record", np.uint32), ("a0", np.uint8), ("a1", np.uint8)])
    sites["pos"], sites["record"] = [10, 20, 30, 5, 9], [0, 0, 0, 1, 1]
    links = np.array([[4, 0, 0, 3], [0, 5, 1, 0], [9, 9, 9, 9], [1, 1, 0, 0], [0, 0, 0, 0]])
    assert HW.solve(sites, links) == [(10, 0, 0, HW.HEAD | HW.JOINED), (10, 0, 0, HW.JOINED), (10, 0, 1, 0), (5, 1, 0, HW.HEAD), (9, 2, 0, HW.HEAD)]
    assert [x[1] for x in HW.solve(sites, links, min_reads=8)] == [0, 1, 2, 3, 4]  # link 0 holds 7 rows, link 1 six
    S = b"ACGTACGT"
    runs = [(2 << 4) | 7, (1 << 4) | 2, (1 << 4) | 1, (2 << 4) | 8, (3 << 4) | 7]  # 2= 1D 1I 2X 3=
    seen = HW.observe(S, 100, runs, {100, 102, 103, 104, 107, 108})
    assert seen == {100: 0, 102: 5, 103: 3, 104: 0, 107: 3}  # A; DEL; the inserted G is skipped: T, A; the last T; 108 lies behind the row
