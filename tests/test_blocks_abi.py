"""CPU checks of the reference-block surface (dcn_anchor_map_reference_blocks, dcn_reference_blocks_merge): declared in
include/deacon_hip_blocks.h and not in deacon_hip.h, exported unmangled and bound in a table of their own at ABI 1.24; the
layout of the two structs in ctypes, numpy, C99 and INTEGRATION.md's second extern block; the definition stated once; the
argument errors that are found before a device is looked at and the order of the others as the source spells it;
dcn_reference_blocks_merge, which needs no device, in full; `deacon-hip gvcf`'s --help and usage errors; the rule of
csrc/dcn_blocks.h compiled for the host under the sanitizers; and the model of the GPU tests (tests/_blocks_worker.py) on
cases written out here.

The tests of the model alone, at the end, pass without the feature; every other test here needs it."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _blocks_worker as BW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
HEADER = os.path.join(ROOT, "include", "deacon_hip_blocks.h")
NAMES = ["dcn_anchor_map_reference_blocks", "dcn_reference_blocks_merge"]
PARAM_OFFSETS = dict(ploidy=0, min_depth=4, min_gq=8, min_qual=12, err_centi=16, het_centi=20, n_edges=24, reserved=28, edges=32)
BLOCK_OFFSETS = dict(pos=0, sum_depth=8, len=16, min_depth=20, max_depth=24, min_gq=28, cls=32, reserved=36)
OLDER = ("map", "verify", "align", "pileup", "extend", "consensus", "call", "genotype", "markdup", "indels", "normalize", "strand")


def declared_in(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dcn_[a-z0-9_]+)\s*\(", text)))


def test_symbols_are_declared_exported_and_bound(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    assert declared_in(HEADER) == NAMES and N.BLOCKS_HEADER_PATH == HEADER
    assert sorted(N._BLOCK_SIGNATURES) == NAMES and not set(NAMES) & set(N._SIGNATURES) and not set(NAMES) & set(N.declared_symbols())
    assert len(N.declared_symbols()) == 114  # deacon_hip.h still declares what it declared
    for name, n_args in zip(NAMES, (11, 3)):
        assert hasattr(L, name) and len(N._BLOCK_SIGNATURES[name][1]) == n_args
        assert getattr(N.lib(), name).argtypes == N._BLOCK_SIGNATURES[name][1] and getattr(N.lib(), name).restype is C.c_int
    nm = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, timeout=60).stdout
    for name in NAMES:
        assert re.search(r" T %s$" % name, nm, re.M), name  # unmangled
    assert tuple(N.ABI) >= (1, 24)
    major, minor = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(major), C.byref(minor)) == 0 and (major.value, minor.value) >= (1, 24)
    main = open(N.HEADER_PATH).read()
    assert len(re.findall(r"1\.24 = dcn_anchor_map_reference_blocks, dcn_reference_blocks_merge: declared in deacon_hip_blocks\.h", main)) == 1
    assert int(re.search(r"#define DCN_ABI_MINOR (\d+)", main).group(1)) >= 24
    assert '#include "deacon_hip.h"' in open(HEADER).read()
    for const in ("BLOCK_NO_COVERAGE", "BLOCK_UNCALLED", "BLOCK_REF", "BLOCK_VARIANT"):
        assert getattr(dcn, const) == getattr(N, const) == getattr(BW, const[6:])
    assert (dcn.BLOCK_NO_COVERAGE, dcn.BLOCK_UNCALLED, dcn.BLOCK_REF, dcn.BLOCK_VARIANT) == (0, 1, 2, 255)
    sig = [(k, v.default) for k, v in inspect.signature(dcn.AnchorMap.reference_blocks).parameters.items()][1:]
    assert sig == [("record", inspect.Parameter.empty), ("start", 0), ("n", None), ("breaks", None), ("gq_edges", (20, 40, 60, 80, 99)), ("ploidy", 2),
                   ("min_depth", 3), ("min_gq", 20), ("min_qual", 20), ("err_centi", 477), ("het_centi", 301)]
    assert callable(dcn.merge_blocks)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "114 entry points, ABI 1.23" in readme and "ABI 1.24" in readme and "deacon-hip gvcf" in readme and "blocks.hip" in readme
    assert "profiles/blocks_rate.txt" in readme
    assert "Reference blocks (ABI 1.24)" in open(os.path.join(ROOT, "DESIGN.md")).read()
    makefile = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "Makefile")).read()
    assert " blocks.hip " in makefile and " blocks_api.hip " in makefile and " dcn_blocks.h " in makefile and "deacon_hip_blocks.h" in makefile


def test_the_definition_is_stated_once():
    flat = " ".join(open(HEADER).read().replace(" *", " ").split())
    assert flat.count("THE DEFINITION OF A REFERENCE BLOCK") == 1
    for i in range(1, 10):
        assert len(re.findall(r"\bB%d\." % i, flat)) == 1, i
    rule = flat.split("THE DEFINITION OF A REFERENCE BLOCK")[1].split("#ifndef DEACON_HIP_BLOCKS_H")[0]
    for words in ("Rules P1-P6, Q1-Q6 and G1-G8 stand", "n_edges (0 .. 15) GQ edges e[0] < e[1] < ..., each in 1 .. 99", "in any order, duplicates allowed",
                  "when p is a break or g is a site (G7)", "otherwise, when depth == 0", "b is the number of edges <= GQ, 0 <= b <= n_edges",
                  "a called non-reference genotype with QUAL below min_qual", "a covered position whose reference base is invalid",
                  "covered only by N or DEL", "VARIANT positions belong to no block", "two runs of one class with a VARIANT position between them are two blocks",
                  "min_gq, the minimum of G4's GQ, called or not", "min_depth, max_depth and sum_depth over D, the last in 64 bits",
                  "Blocks come in ascending pos; the count is always reported", "Two blocks TOUCH when a.pos + a.len == b.pos",
                  "len and sum_depth add, the minima and the maximum combine", "for every m", "It does not depend on grid, lanes or order",
                  "they show as UNCALLED and are not excluded", "except through the breaks the caller passes", "a convention, not a measured optimum"):
        assert words in rule, words
    main = " ".join(open(os.path.join(ROOT, "include", "deacon_hip.h")).read().split())
    assert "THE DEFINITION OF A REFERENCE BLOCK" not in main


def rust_block(md):
    """INTEGRATION.md's second extern block and the text in front of it back to its section's heading"""
    parts = md.split('extern "C" {')
    assert len(parts) == 3  # two blocks
    return parts[1].split("### 3.16 Reference blocks (1.24")[1], parts[2].split("\n}\n")[0]


def test_struct_layout_agrees(tmp_path, dcn):
    N = dcn._native
    for ctype, dtype, offsets, size in ((N.BlockParams, None, PARAM_OFFSETS, 48), (N.ReferenceBlock, dcn.REFERENCE_BLOCK_DTYPE, BLOCK_OFFSETS, 40)):
        assert C.sizeof(ctype) == size
        assert {f: getattr(ctype, f).offset for f, _ in ctype._fields_} == offsets and [f for f, _ in ctype._fields_] == list(offsets)
        if dtype is not None:
            assert dtype.itemsize == size and {f: dtype.fields[f][1] for f in dtype.names} == offsets and list(dtype.names) == list(offsets)
    checks = " && ".join(["offsetof(dcn_block_params, %s) == %d" % kv for kv in PARAM_OFFSETS.items()] +
                         ["offsetof(dcn_reference_block, %s) == %d" % kv for kv in BLOCK_OFFSETS.items()])
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "deacon_hip_blocks.h"\n'
                   "int (*f0)(const dcn_index *, const void *, uint32_t, uint64_t, uint64_t, const uint64_t *, uint64_t, uint8_t *, void *, uint64_t,\n"
                   "          uint64_t *) = dcn_anchor_map_reference_blocks;\n"
                   "int (*f1)(void *, uint64_t, uint64_t *) = dcn_reference_blocks_merge;\n"
                   "int main(void){ dcn_block_params p = {2, 3, 20, 20, 477, 301, 2, 0, {20, 40}}; dcn_reference_block b = {7, 90, 3, 1, 50, 12, 4, 0};\n"
                   "  return sizeof p == 48 && sizeof b == 40 && p.edges[1] == 40 && p.edges[15] == 0 && b.sum_depth == 90 && b.cls == 4 &&\n"
                   "         DCN_BLOCK_NO_COVERAGE == 0u && DCN_BLOCK_UNCALLED == 1u && DCN_BLOCK_REF == 2u && DCN_BLOCK_VARIANT == 255u &&\n"
                   "         DCN_ABI_MINOR >= 24 && " + checks + " ? 0 : 1; }\n")
    inc, libdir = os.path.dirname(HEADER), os.path.dirname(N.LIB_PATH)  # (the function pointers are initialised and never called)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(tmp_path / "t"), "-L", libdir,
                           "-ldeacon_hip", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"])
    assert subprocess.call([str(tmp_path / "t")]) == 0
    # the Rust structs: the fields in order, with the types of the C ones
    section, _ = rust_block(open(os.path.join(ROOT, "INTEGRATION.md")).read())
    rust_of = {"uint32_t": "u32", "uint64_t": "u64", "uint8_t": "u8"}
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for struct, offsets in (("dcn_block_params", PARAM_OFFSETS), ("dcn_reference_block", BLOCK_OFFSETS)):
        c_fields = re.findall(r"(uint\d+_t)\s+(\w+)(\[16\])?;", header.split("typedef struct %s {" % struct)[1].split("}")[0])
        body = section.split("pub struct %s {" % struct)[1].split("\n}")[0]
        assert "#[repr(C)]\npub struct %s {" % struct in section
        rust_fields = re.findall(r"pub (\w+): ([\w\[\]; ]+),", body)
        assert [f for _, f, _ in c_fields] == list(offsets) == [f for f, _ in rust_fields]
        assert [t for _, t in rust_fields] == ["[%s; 16]" % rust_of[t] if arr else rust_of[t] for t, _, arr in c_fields]


def test_the_second_extern_block_is_the_new_header(dcn):
    import test_abi as TA
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    _, block = rust_block(md)
    rust = {m.group(1): m.group(2) for m in re.finditer(r"pub fn (dcn_\w+)\(([^)]*)\)\s*->\s*c_int;", block)}
    assert sorted(rust) == NAMES
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        c_args = re.search(r"int %s\(([^)]*)\);" % name, header).group(1)
        c_types = [" ".join(a.split()) for a in c_args.split(",")]
        rust_types = [a.split(":", 1)[1].strip() for a in rust[name].split(",")]
        assert rust_types == [TA._rust_of_c(t) for t in c_types], (name, c_types, rust_types)
    assert "pub const DCN_ABI_MINOR: u32 = 24;" in md and "**1.24** `dcn_anchor_map_reference_blocks`, `dcn_reference_blocks_merge`" in md


def test_argument_errors_that_need_no_device(dcn):
    """params NULL, its fields in the genotype's order with the genotype's messages, the edges, then the map"""
    N, L = dcn._native, dcn._native.lib()
    count = C.c_uint64(12345)

    def params(*fields, edges=()):
        return N.BlockParams(*fields, (C.c_uint8 * 16)(*edges))

    def call(p):
        return L.dcn_anchor_map_reference_blocks(None, None if p is None else C.byref(p), 0, 0, 1, None, 0, None, None, 0, C.byref(count))

    for p, word in ((None, b"params is NULL"), (params(3, 3, 100, 20, 100001, 100001, 16, 1), b"params.reserved must be 0"),
                    (params(3, 3, 100, 20, 100001, 100001, 16, 0), b"params.ploidy must be 1 or 2"),
                    (params(2, 3, 100, 20, 100001, 100001, 16, 0), b"params.min_gq must be 0..99"),
                    (params(2, 3, 99, 20, 100001, 100001, 16, 0), b"params.err_centi must be 0..100000"),
                    (params(2, 3, 99, 20, 100000, 100001, 16, 0), b"params.het_centi must be 0..100000"),
                    (params(2, 3, 99, 20, 100000, 100000, 16, 0), b"params.n_edges must be 0..15"),
                    (params(2, 3, 20, 20, 477, 301, 2, 0, edges=(0, 5)), b"params.edges[0] must be 1..99"),
                    (params(2, 3, 20, 20, 477, 301, 2, 0, edges=(5, 100)), b"params.edges[1] must be 1..99"),
                    (params(2, 3, 20, 20, 477, 301, 3, 0, edges=(5, 9, 9)), b"params.edges[2] is not above the edge in front of it"),
                    (params(2, 3, 20, 20, 477, 301, 3, 0, edges=(5, 9, 8)), b"params.edges[2] is not above the edge in front of it"),
                    (params(2, 3, 20, 20, 477, 301, 2, 0, edges=(5, 9, 0, 0, 7)), b"params.edges[4] must be 0: it is not one of the n_edges"),
                    (params(2, 3, 20, 20, 477, 301, 0, 0, edges=(5,)), b"params.edges[0] must be 0: it is not one of the n_edges"),
                    (params(1, 0, 0, 0, 0, 0, 15, 0, edges=tuple(range(85, 100))), b"map is NULL"),
                    (params(2, 3, 20, 20, 477, 301, 0, 0), b"map is NULL")):
        assert call(p) == N.DCN_ERR_ARG and word in L.dcn_last_error(), (word, L.dcn_last_error())
    assert count.value == 12345  # (nothing is written by a refused call)


def test_the_order_of_the_other_errors_from_the_source():
    api = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "blocks_api.hip")).read()
    body = api.split('extern "C" int dcn_anchor_map_reference_blocks(')[1].split("\n}\n")[0]
    order = ['"params is NULL"', '"params.reserved must be 0"', '"params.ploidy must be 1 or 2"', '"params.min_gq must be 0..99"', '"params.err_centi must be 0..100000"',
             '"params.het_centi must be 0..100000"', '"params.n_edges must be 0..15"', "check_qsums(map)", 'check_range(map, "reference blocks"',
             '"n_blocks is NULL"', '"breaks["', "*n_blocks = 0;", "if (n_bases == 0) return DCN_OK;", "hipSetDevice", "dcn_launch_blocks_classify",
             "dcn_launch_blocks_breaks", "dcn_launch_blocks_heads(ba, false", "dcn_launch_offsets_scan", "if (cls) ", "DCN_ERR_CAPACITY", '"blocks is NULL"',
             "dcn_launch_blocks_fill", "dcn_launch_blocks_heads(ba, true"]
    at = [body.index(x) for x in order]
    assert at == sorted(at)
    geno = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "genotype_api.hip")).read()
    for message in order[:6]:
        assert message in geno  # the genotype's messages
    merge = api.split('extern "C" int dcn_reference_blocks_merge(')[1]
    assert "hip" not in merge.replace("dcn_fail", "")  # host only: no device call


def test_the_shared_header_has_no_floating_point_no_device_only_code_and_no_runtime_index():
    src = open(os.path.join(ROOT, "deacon-server_amd", "csrc", "dcn_blocks.h")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\b(float|double)\b", code) and "hip/" not in code and "atomic" not in code and "__shfl" not in code
    device = code.split("dcn_blocks_pack_edges")[1].split("\n}\n", 1)[1]  # behind the host's packing loop nothing is indexed at all
    assert "[" not in device.replace("pl[DCN_GENO_GENOTYPES]", "").replace("n[0]", "").replace("n[1]", "").replace("n[2]", "").replace("n[3]", "")


# ---- dcn_reference_blocks_merge: host only, tested in full here ----------------------------------------------------------
def blocks(dcn, rows):
    return BW.to_array(dcn.REFERENCE_BLOCK_DTYPE, rows)


def test_merge_touching_and_not(dcn):
    # (pos, len, cls, min_gq, min_depth, max_depth, sum_depth)
    rows = [(0, 5, 3, 30, 4, 9, 30), (5, 4, 3, 12, 6, 11, 40), (9, 2, 1, 9, 1, 1, 2), (12, 3, 1, 0, 0, 2, 3), (15, 1, 1, 5, 7, 7, 7), (16, 4, 0, 0, 0, 0, 0),
            (20, 1, 2, 40, 9, 9, 9), (21, 1, 3, 41, 9, 9, 9), (22, 1, 3, 42, 8, 8, 8)]
    want = [(0, 9, 3, 12, 4, 11, 70), (9, 2, 1, 9, 1, 1, 2), (12, 4, 1, 0, 0, 7, 10), (16, 4, 0, 0, 0, 0, 0), (20, 1, 2, 40, 9, 9, 9), (21, 2, 3, 41, 8, 9, 17)]
    assert BW.device_blocks(dcn.merge_blocks(blocks(dcn, rows))) == want == BW.merge(rows)
    before = blocks(dcn, rows)
    copy = before.copy()
    dcn.merge_blocks(before)
    assert np.array_equal(before, copy)  # merge_blocks returns a new array
    assert len(dcn.merge_blocks(blocks(dcn, []))) == 0 and BW.device_blocks(dcn.merge_blocks(blocks(dcn, rows[:1]))) == rows[:1]
    assert BW.device_blocks(dcn.merge_blocks(blocks(dcn, want))) == want  # nothing left to merge


def test_merge_a_chain_of_thousands(dcn):
    rng = np.random.default_rng(2402)
    rows, pos = [], 0
    for i in range(5000):
        ln = int(rng.integers(1, 50))
        depth = int(rng.integers(0, 1000))
        rows.append((pos, ln, 7, int(rng.integers(0, 100)), depth, depth + int(rng.integers(0, 9)), depth * ln + int(rng.integers(0, 5))))
        pos += ln
    got = BW.device_blocks(dcn.merge_blocks(blocks(dcn, rows)))
    assert got == [(0, pos, 7, min(r[3] for r in rows), min(r[4] for r in rows), max(r[5] for r in rows), sum(r[6] for r in rows))]
    rows[2500] = rows[2500][:2] + (8,) + rows[2500][3:]
    assert [g[2] for g in BW.device_blocks(dcn.merge_blocks(blocks(dcn, rows)))] == [7, 8, 7]
    big = [(i * 2 ** 31, 2 ** 31, 2, 1, 1, 1, 2 ** 40) for i in range(2)]
    big[1] = (big[1][0], 2 ** 31 - 1) + big[1][2:]
    assert BW.device_blocks(dcn.merge_blocks(blocks(dcn, big))) == [(0, 2 ** 32 - 1, 2, 1, 1, 1, 2 ** 41)]  # the longest block there is


def test_merge_errors(dcn):
    N, L = dcn._native, dcn._native.lib()
    kept = C.c_uint64(777)
    one = blocks(dcn, [(0, 5, 3, 30, 4, 9, 30)])
    assert L.dcn_reference_blocks_merge(one.ctypes.data_as(C.c_void_p), 1, None) == N.DCN_ERR_ARG and b"n_merged is NULL" in L.dcn_last_error()
    assert L.dcn_reference_blocks_merge(None, 1, C.byref(kept)) == N.DCN_ERR_ARG and b"blocks is NULL" in L.dcn_last_error() and kept.value == 777
    assert L.dcn_reference_blocks_merge(None, 0, C.byref(kept)) == N.DCN_OK and kept.value == 0
    for rows, word in (([(0, 5, 3, 1, 1, 1, 5), (4, 2, 3, 1, 1, 1, 2)], b"blocks[1] at 4 does not lie behind blocks[0], which ends at 5"),          # overlapping
                       ([(0, 5, 3, 1, 1, 1, 5), (5, 2, 3, 1, 1, 1, 2), (9, 1, 1, 1, 1, 1, 1), (8, 1, 1, 1, 1, 1, 1)], b"blocks[3] at 8 does not lie behind"),  # descending
                       ([(7, 1, 3, 1, 1, 1, 5), (7, 1, 4, 1, 1, 1, 2)], b"blocks[1] at 7"),                                                             # one position twice
                       ([(0, 2 ** 31, 2, 1, 1, 1, 1), (2 ** 31, 2 ** 31, 2, 1, 1, 1, 1)], b"gives a len above 4294967295"),
                       ([(0, 9, 5, 1, 1, 1, 1), (9, 2 ** 32 - 1, 2, 1, 1, 1, 1), (2 ** 32 + 8, 1, 2, 1, 1, 1, 1)], b"merging into blocks[2] gives a len above 4294967295")):
        arr = blocks(dcn, rows)
        copy, kept.value = arr.copy(), 777
        assert L.dcn_reference_blocks_merge(arr.ctypes.data_as(C.c_void_p), len(arr), C.byref(kept)) == N.DCN_ERR_ARG
        assert word in L.dcn_last_error() and np.array_equal(arr, copy) and kept.value == 777  # the array is as it was
        with pytest.raises(dcn.DeaconHipError):
            dcn.merge_blocks(arr)
    ok = blocks(dcn, [(0, 2 ** 31, 2, 1, 1, 1, 1), (2 ** 31, 2 ** 31, 3, 1, 1, 1, 1)])  # (other classes: nothing merges, nothing overflows)
    assert len(dcn.merge_blocks(ok)) == 2


# ---- the host program and the tool --------------------------------------------------------------------------------------
def test_rules_on_the_host_and_the_model_against_their_rows(tmp_path):
    """tests/cpp/blocks_rule_test.cpp: dcn_blocks.h against a brute force, hand-written rows and rule B7 at every cut, under the
    address and undefined-behaviour sanitizers, as a program of its own; then every row it printed through the Python model"""
    exe = tmp_path / "blocks_rule_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "deacon-server_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "blocks_rule_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", (out.stdout[-2000:], out.stderr[-2000:])
    m = re.search(r"blocks rule ok: (\d+) positions, (\d+) blocks, (\d+) cuts", out.stdout)
    assert m and int(m.group(1)) >= 20_000 and int(m.group(2)) >= 4000 and int(m.group(3)) >= 20_000
    assert BW.check_rule_rows(out.stdout.splitlines()) == 25


GVCF_ERRORS = [
    (["gvcf"], "the following required arguments were not provided: <REF>"),
    (["gvcf", "ref.fa"], "nothing to write: give at least one of -o <OUTPUT>, --variants <FILE>, --pileup <FILE>, --sites <FILE>, --vcf <FILE>, "
                         "--gvcf <FILE>, --callable <FILE>, --duplicates <FILE>, -s <SUMMARY>"),
    (["gvcf", "ref.fa", "--gvcf"], "missing value for --gvcf"),
    (["gvcf", "ref.fa", "--gq-bands", "20,x"], "invalid value for --gq-bands: must be 0..255"),
    (["gvcf", "ref.fa", "--gq-bands", "20,,40"], "invalid value for --gq-bands: must be 0..255"),
    (["gvcf", "ref.fa", "--max-sb", "65536"], "invalid value for --max-sb: must be 0..65535"),
    (["gvcf", "ref.fa", "in1", "in2"], "gvcf takes one input: mates are independent here, run it once per file (unexpected argument 'in2')"),
    (["gvcf", "ref.fa", "--blocks"], "unexpected argument '--blocks'"),
]


@pytest.mark.parametrize("args,message", GVCF_ERRORS, ids=[" ".join(e[0]) for e in GVCF_ERRORS])
def test_gvcf_error_exit_code_and_text(args, message):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "Error: " + message + "\n")


def test_gvcf_refuses_fasta_and_names_the_mode(tmp_path):
    reads = tmp_path / "reads.fa"
    reads.write_text(">read7 some words\nACGTACGT\n")
    p = subprocess.run([CLI, "gvcf", "ref.fa", str(reads), "--gvcf", str(tmp_path / "v.vcf")], capture_output=True, text=True, timeout=60,
                       stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "Error: gvcf needs base qualities, and record 'read7' has none (FASTA): consensus takes reads without\n")


def test_gvcf_help_text_and_the_older_helps():
    p = subprocess.run([CLI, "gvcf", "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "gvcf.txt")) as f:
        want = f.read()
    assert (p.returncode, p.stderr, p.stdout) == (0, "", want)
    for word in ("Usage: deacon-hip gvcf [OPTIONS] <REF> [READS]", "\nReference blocks: ", "--gvcf <FILE>", "--gq-bands <LIST>", "--callable <FILE>",
                 "[default: 20,40,60,80,99, a convention]", "NO_COVERAGE, LOW_CONFIDENCE or CALLABLE", "Variant lines do not gain <NON_REF>: a limit",
                 "##GVCFBlock", "GT:GQ:DP:MIN_DP", "ref_bases_by_band and gq_bands", "every output\nis strand's, byte for byte"):
        assert word in want, word
    # every line of strand's help from its arguments on is in it, in order, but for the three options
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "strand.txt")) as f:
        strand = f.read()
    tail = strand[strand.index("\nArguments:\n"):]
    mine = "\n".join(line for line in want.split("\n") if not re.match(
        r"^      (--gvcf|--gq-bands|--callable) |^ {33}(positions of one class, with END|\(\.gz as BGZF, \.zst and \.xz by extension, as --vcf\)|15, each 1\.\.99\)|the intervals tile every record)", line))
    assert tail in mine and mine.index("\nReference blocks: ") == mine.index(tail) + len(tail)
    top = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert (top.stdout + top.stderr).count("\n  gvcf ") == 1 and (top.stdout + top.stderr).count("\n  strand ") == 1
    for sub in OLDER + ("map-pairs", "place", "mask", "classify"):
        if sub in OLDER:
            for opt in ("--gvcf", "--gq-bands", "--callable"):  # the other modes do not know the three options
                q = subprocess.run([CLI, sub, "ref.fa", opt, "1"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
                assert (q.returncode, q.stderr) == (1, "Error: unexpected argument '%s'\n" % opt), (sub, opt)
        h = subprocess.run([CLI, sub, "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
        with open(os.path.join(ROOT, "tests", "golden", "cli_help", sub + ".txt")) as f:
            assert h.stdout == f.read(), sub  # the help texts of the older modes do not change


# ---- the model alone: THE TESTS HERE THAT PASS WITHOUT THE FEATURE ---------------------------------------------------------
def test_model_alone_on_positions_written_out():
    D = dict(ploidy=2, min_depth=3, min_gq=20, min_qual=20, err_centi=477, het_centi=301)
    ref = lambda k: ([k, 0, 0, 0, 0, 0, 0, 0], [30 * k, 0, 0, 0])  # noqa: E731
    assert BW.classify([0] * 8, [0] * 4, 0, **D) == (BW.NO_COVERAGE, 0, 0)
    assert BW.classify([0, 0, 0, 0, 4, 0, 0, 0], [0] * 4, 0, **D) == (BW.UNCALLED, 0, 0) == BW.classify([0, 0, 0, 0, 0, 4, 0, 0], [0] * 4, 0, **D)
    assert BW.classify([0] * 8, [0] * 4, 4, **D) == (BW.NO_COVERAGE, 0, 0) and BW.classify(*ref(8), 4, **D) == (BW.UNCALLED, 24, 8)
    assert BW.classify([0, 0, 0, 0, 0, 0, 9, 9], [0] * 4, 0, **D) == (BW.NO_COVERAGE, 0, 0)  # INS and REV are no coverage
    assert [BW.classify(*ref(k), 0, **D)[:2] for k in (2, 3, 6, 7, 13, 14)] == [(1, 6), (1, 9), (1, 18), (3, 21), (3, 39), (4, 42)]
    assert [BW.classify(*ref(10), 0, False, e, **D)[0] for e in ((29,), (30,), (31,), ())] == [3, 3, 2, 2]
    assert BW.classify(*ref(40), 0, False, (99,), **D)[:2] == (3, 99) and BW.classify(*ref(40), 0, False, tuple(range(1, 15)) + (99,), **D)[0] == 17
    assert BW.classify(*ref(3), 0, **dict(D, ploidy=1))[:2] == (BW.REF + 5, 99)
    het = ([5, 5, 0, 0, 0, 0, 0, 0], [150, 150, 0, 0])
    assert BW.classify(*het, 0, **dict(D, min_qual=143))[0] == BW.VARIANT and BW.classify(*het, 0, **dict(D, min_qual=144))[0] == BW.UNCALLED
    assert BW.classify(*ref(8), 0, True, **D)[0] == BW.VARIANT and BW.classify([0] * 8, [0] * 4, 0, True, **D)[0] == BW.VARIANT  # a break, whatever is there


def test_model_alone_blocks_and_merge_written_out():
    cls = [0, 0, 3, 3, 255, 3, 1, 255, 255, 1]
    gq = [0, 0, 30, 25, 99, 21, 5, 0, 0, 7]
    depth = [0, 0, 9, 8, 10, 7, 2, 0, 0, 1]
    want = [(100, 2, 0, 0, 0, 0, 0), (102, 2, 3, 25, 8, 9, 17), (105, 1, 3, 21, 7, 7, 7), (106, 1, 1, 5, 2, 2, 2), (109, 1, 1, 7, 1, 1, 1)]
    assert BW.blocks_of(cls, gq, depth, 100) == want and BW.merge(want) == want  # a VARIANT between two runs of one class: two blocks
    for m in range(len(cls) + 1):
        halves = BW.blocks_of(cls[:m], gq[:m], depth[:m], 100) + BW.blocks_of(cls[m:], gq[m:], depth[m:], 100 + m)
        assert BW.merge(halves) == want, m  # rule B7
    assert BW.blocks_of([255, 255], [0, 0], [0, 0]) == [] and BW.blocks_of([], [], []) == [] and BW.merge([]) == []
    with pytest.raises(AssertionError):
        BW.merge([(0, 5, 1, 0, 0, 0, 0), (4, 1, 1, 0, 0, 0, 0)])
