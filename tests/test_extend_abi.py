"""CPU checks of the extend surface (dcn_extend_batch): declared, exported and bound at ABI 1.16, the layout of its two
structs, the argument errors that are found before a device is looked at, the kernel's flank routine compiled for the host
under the sanitizers, and the model of the GPU tests (tests/_extend_worker.py) alone on flanks whose answer is written out
here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _extend_worker as XW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM_FIELDS = (("penalty", 0, 4), ("end_bonus", 4, 4), ("max_edits", 8, 4), ("row_stride", 12, 4), ("reserved", 16, 8))
ROW_FIELDS = (("read_start", 0, 4), ("read_end", 4, 4), ("ref_start", 8, 8), ("ref_end", 16, 8), ("left_edits", 24, 4), ("right_edits", 28, 4))


def test_symbol_is_declared_exported_and_bound(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    assert "dcn_extend_batch" in N.declared_symbols() and hasattr(L, "dcn_extend_batch")
    assert len(N._SIGNATURES["dcn_extend_batch"][1]) == 10
    assert tuple(N.ABI) >= (1, 16)
    major, minor = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(major), C.byref(minor)) == 0 and (major.value, minor.value) >= (1, 16)
    header = open(N.HEADER_PATH).read()
    assert len(re.findall(r"1\.16 = dcn_extend_batch", header)) == 1
    assert int(re.search(r"#define DCN_ABI_MINOR (\d+)", header).group(1)) >= 16
    flat = " ".join(header.replace(" *", " ").split())
    assert flat.count("THE DEFINITION OF AN EXTENDED PLACEMENT") == 1
    for rule in ("X1.", "X2.", "X3.", "X4.", "X5.", "X6.", "X7.", "X8."):
        assert flat.count(" " + rule + " ") == 1, rule
    assert "penalty = 6, end_bonus = 4 and max_edits = 1023 are the conventions of the layers above, not measured optima" in flat
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"pub const DCN_ABI_MINOR: u32 = (\d+); +//", md).group(1)) >= 16
    assert re.search(r"pub fn dcn_extend_batch\(", md) and "dcn_extend_params" in md and "dcn_extension" in md
    assert hasattr(dcn.Placer, "extend_batch")
    for name in ("EXTENSION_DTYPE",):
        assert getattr(dcn, name) is getattr(dcn.filter, name) and name in dcn.__all__
    assert (XW.PENALTY, XW.END_BONUS, XW.MAX_EDITS) == (6, 4, N.VERIFY_MAX_EDITS)
    import inspect
    defaults = {k: v.default for k, v in inspect.signature(dcn.Placer.extend_batch).parameters.items()}
    assert (defaults["penalty"], defaults["end_bonus"], defaults["max_edits"], defaults["row_offsets"]) == (6, 4, 1023, None)


def test_struct_layouts_in_ctypes_and_numpy(dcn):
    N = dcn._native
    assert C.sizeof(N.ExtendParams) == 24 and C.sizeof(N.Extension) == 32
    for name, offset, size in PARAM_FIELDS:
        field = getattr(N.ExtendParams, name)
        assert (field.offset, field.size) == (offset, size), name
    dt = dcn.EXTENSION_DTYPE
    assert dt.itemsize == 32 and list(dt.names) == [f for f, _ in N.Extension._fields_] == [f for f, _, _ in ROW_FIELDS]
    for name, offset, size in ROW_FIELDS:
        field = getattr(N.Extension, name)
        assert (field.offset, field.size) == (offset, size) and (dt.fields[name][1], dt.fields[name][0].itemsize) == (offset, size), name
    assert np.dtype(XW.EXTENSION_FIELDS) == dt


def test_header_compiles_as_c_with_these_layouts(tmp_path, dcn):
    checks = ["sizeof(dcn_extend_params) == 24", "sizeof(dcn_extension) == 32", "DCN_ABI_MINOR >= 16"]
    checks += ["offsetof(dcn_extend_params, %s) == %d" % (n, o) for n, o, _ in PARAM_FIELDS]
    checks += ["offsetof(dcn_extension, %s) == %d" % (n, o) for n, o, _ in ROW_FIELDS]
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "deacon_hip.h"\n'
                   "int (*f1)(dcn_ctx *, const dcn_index *, const uint8_t *, const uint64_t *, uint32_t, const void *, const uint64_t *,\n"
                   "          const void *, uint64_t, void *) = dcn_extend_batch;\n"
                   "int main(void){ dcn_extend_params p = {6, 4, DCN_VERIFY_MAX_EDITS, 64, {0, 0}};\n"
                   "  return p.penalty == 6 && " + " && ".join(checks) + " ? 0 : 1; }\n")
    inc = os.path.dirname(dcn._native.HEADER_PATH)
    exe = tmp_path / "t"
    # (only the layout is run: the function pointer is initialised, never called, so the program links against the library)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(exe),
                           "-L", os.path.dirname(dcn._native.LIB_PATH), "-ldeacon_hip", "-Wl,-rpath," + os.path.dirname(dcn._native.LIB_PATH),
                           "-Wl,--allow-shlib-undefined"])
    assert subprocess.run([str(exe)], timeout=60).returncode == 0


def test_argument_errors_that_need_no_device(dcn):
    """the parameters, in dcn_verify_batch's order: the new ones are penalty, end_bonus and max_edits; the rest carry
    dcn_verify_batch's messages word for word"""
    N, L = dcn._native, dcn._native.lib()

    def prm(penalty=6, bonus=4, edits=1023, stride=48, reserved=(0, 0)):
        return C.byref(N.ExtendParams(penalty, bonus, edits, stride, (C.c_uint32 * 2)(*reserved)))

    def vprm(edits=1023, stride=48):
        return C.byref(N.VerifyParams(edits, 200, stride, 0))

    stand_in = (C.c_uint8 * 4096)()
    out = (C.c_uint8 * 64)(*([7] * 64))
    for args, word, verify in (((None, None, None), b"params is NULL", None),
                               ((None, None, prm(reserved=(1, 0))), b"params.reserved must be 0", None),
                               ((None, None, prm(reserved=(0, 1))), b"params.reserved must be 0", None),
                               ((None, None, prm(penalty=1)), b"params.penalty must be 2..255", None),
                               ((None, None, prm(penalty=0)), b"params.penalty must be 2..255", None),
                               ((None, None, prm(penalty=256)), b"params.penalty must be 2..255", None),
                               ((None, None, prm(bonus=65536)), b"params.end_bonus must be 0..65535", None),
                               ((None, None, prm(edits=1024)), b"params.max_edits must be 0..1023", vprm(edits=1024)),
                               ((None, None, prm(stride=40)), b"row_stride", vprm(stride=40)),
                               ((None, None, prm(stride=52)), b"row_stride", vprm(stride=52)),
                               ((None, None, prm(penalty=2, bonus=65535, edits=0)), b"ctx is NULL", vprm()),
                               ((None, None, prm(penalty=255)), b"ctx is NULL", vprm()),
                               ((C.cast(stand_in, C.c_void_p), None, prm(stride=64)), b"map is NULL", vprm(stride=64))):
        assert L.dcn_extend_batch(args[0], args[1], None, None, 0, args[2], None, None, 0, out) == N.DCN_ERR_ARG
        message = L.dcn_last_error()
        assert word in message, (word, message)
        if verify is not None:
            assert L.dcn_verify_batch(args[0], args[1], None, None, 0, verify, None, None, 0, None) == N.DCN_ERR_ARG
            assert L.dcn_last_error() == message
    assert bytes(out) == bytes([7] * 64)  # (nothing is written by a refused call)


def test_flank_routine_on_the_host(tmp_path):
    """tests/cpp/extend_flank_test.cpp: dcn_extend.h's flank routine on streams of exactly the words the real ones have, the
    store with no word in front of base 0, under the address and undefined-behaviour sanitizers as a program of its own:
    all four strand and side combinations, left flanks from store bases 0 .. 33, right flanks to the last base, neighbours
    that continue the match, against a full table on three thousand random flanks"""
    exe = tmp_path / "extend_flank_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "deacon-server_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "extend_flank_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "extend flank ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])


V12 = b"ACGTTGCATCAG"


def sub(s, at):
    s = bytearray(s)
    s[at] = ord("C") if s[at] == ord("A") else ord("A")
    return bytes(s)


HAND = [
    # (U, V, penalty, end_bonus, max_edits, (i*, j*, D*), why)
    (V12, V12, 6, 4, 1023, (12, 12, 0), "an error-free flank: to its end"),
    (V12, V12 + b"TTTT", 6, 4, 1023, (12, 12, 0), "... and no further on the record"),
    (sub(V12, 11), V12, 6, 4, 1023, (11, 11, 0), "a mismatch at f - 1, bonus 4: 24 - 6 + 4 ties with the 22 of (11, 11), and the smaller D wins: clipped"),
    (sub(V12, 11), V12, 6, 5, 1023, (12, 12, 1), "... bonus 5: 24 - 6 + 5 = 23 > 22: extended"),
    (sub(V12, 10), V12, 6, 4, 1023, (12, 12, 1), "a mismatch at f - 2: 24 - 6 + 4 = 22 > 20"),
    (V12[:5] + b"A" + V12[5:], V12, 6, 4, 1023, (13, 12, 1), "a base of the read alone"),
    (V12[:5] + V12[6:], V12, 6, 4, 1023, (11, 12, 1), "a base of the record alone"),
    (b"ACGTA", b"", 6, 4, 1023, (0, 0, 0), "g = 0: nothing to extend over"),
    (b"A", b"", 2, 3, 1023, (1, 0, 1), "... unless the bonus pays for the read's bases alone: 1 - 2 + 3 > 0"),
    (b"", b"ACGTA", 6, 4, 1023, (0, 0, 0), "f = 0: every (0, j) has the bonus, j = 0 has no edits"),
    (b"", b"", 6, 4, 1023, (0, 0, 0), "f = g = 0"),
    (V12, V12[:6], 6, 4, 1023, (6, 6, 0), "f > g: the record ends first; 18 - 36 + 4 < 12"),
    (b"AAAAAGGGTGG", b"AAAAGGGTGG", 6, 4, 1023, (11, 10, 1), "a homopolymer one base longer in the read: one cell whichever A is alone"),
    (b"AAAAGGGTGG", b"AAAAAGGGTGG", 6, 4, 1023, (10, 11, 1), "... and in the record"),
    (b"AC", b"CA", 2, 0, 1023, (2, 1, 1), "(1, 2) and (2, 1) both cost 1 and are worth 1: the larger i"),
    (b"ACA", b"CAC", 3, 0, 1023, (3, 2, 1), "a repeat shifted by one base: (2, 3) and (3, 2), worth 2 at cost 1: the larger i"),
    (V12[:4] + b"N" + V12[5:], V12, 6, 4, 1023, (12, 12, 1), "N in U: a mismatch"),
    (V12, V12[:4] + b"N" + V12[5:], 6, 4, 1023, (12, 12, 1), "N in V: a mismatch"),
    (V12[:4] + b"N" + V12[5:], V12[:4] + b"N" + V12[5:], 6, 4, 1023, (12, 12, 1), "N against N: a mismatch too"),
    (V12.lower(), V12, 6, 4, 1023, (12, 12, 0), "case does not matter"),
    (sub(V12, 2), V12, 6, 4, 1023, (12, 12, 1), "one mismatch at base 2"),
    (sub(V12, 2), V12, 6, 4, 0, (2, 2, 0), "... max_edits 0 excludes the better cell"),
    (sub(sub(V12, 2), 6), V12, 6, 4, 1023, (12, 12, 2), "two mismatches: 24 - 12 + 4 = 16 > 6"),
    (sub(sub(V12, 2), 6), V12, 6, 4, 1, (6, 6, 1), "... max_edits 1: 12 - 6 = 6 > 4"),
    (sub(sub(V12, 2), 6), V12, 6, 4, 0, (2, 2, 0), "... max_edits 0"),
]


@pytest.mark.parametrize("U,V,penalty,end_bonus,max_edits,want,why", HAND, ids=[h[-1][:48] for h in HAND])
def test_model_alone_on_flanks_written_out(U, V, penalty, end_bonus, max_edits, want, why):
    """THE TESTS HERE THAT PASS WITHOUT THE FEATURE: they run the model only.  (No short flank of one repeated letter makes the
    rule on i decide: test_no_flank_of_one_letter_ties_on_i searches two letters, up to four bases a side, and finds such ties only where a flank has both letters, as between (i, i + 1)
    and (i + 1, i) of sequences shifted against each other.)"""
    assert XW.flank_best(U, V, penalty, end_bonus, max_edits) == want, why


def test_model_rows_on_both_strands():
    """rule X6 on one hand-written row per strand: the same R' gives the same extension, mapped back to the read as given"""
    from conftest import revcomp
    record = b"TTGACCA" + V12 + b"GGATCCTAGGCTA" + V12[::-1] + b"CATTAG"
    a0 = 7 + len(V12)                       # T = record[a0 : a0 + 13]
    oriented = b"GG" + sub(V12, 9)[2:] + b"GGATCCTAGGCTA" + V12[::-1][:8] + b"AAAA"  # 2 clipped, 10 of the left flank, S, 8 + 4 clipped
    for rev, read in ((0, oriented), (1, revcomp(oriented))):
        row = np.zeros(1, [("record", np.uint32), ("reverse", np.uint32), ("read_start", np.uint32), ("read_end", np.uint32),
                           ("ref_start", np.uint64), ("ref_end", np.uint64)])
        L = len(oriented)
        a, b = 12, 25
        row["reverse"], row["ref_start"], row["ref_end"] = rev, a0, a0 + 13
        row["read_start"], row["read_end"] = (L - b, L - a) if rev else (a, b)
        out, ext = XW.extend_rows([read], [record], row)
        # left: 10 bases with one mismatch at the third, then GG against CA: 20 - 6 = 14 > 4; right: 8 bases, then AAAA
        # against TGCA: clipped
        assert (int(ext["ref_start"][0]), int(ext["ref_end"][0]), int(ext["left_edits"][0]), int(ext["right_edits"][0])) == (a0 - 10, a0 + 21, 1, 0)
        assert (int(out["read_start"][0]), int(out["read_end"][0])) == ((L - 33, L - 2) if rev else (2, 33))
        assert XW.clips(L, out[0]) == (2, 4) and XW.clips(L, row[0]) == (12, 12)
    unplaced = row.copy()
    unplaced["record"] = XW.UNPLACED
    out, ext = XW.extend_rows([read], [record], unplaced)
    assert out.tolist() == unplaced.tolist() and int(ext["left_edits"][0]) == 0 == int(ext["right_edits"][0])  # rule X7


CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
EXTEND_ERRORS = [
    (["extend"], "the following required arguments were not provided: <REF>"),
    (["extend", "ref.fa", "--penalty", "1"], "invalid value for --penalty: must be 2..255"),
    (["extend", "ref.fa", "--penalty", "256"], "invalid value for --penalty: must be 2..255"),
    (["extend", "ref.fa", "--end-bonus", "65536"], "invalid value for --end-bonus: must be 0..65535"),
    (["extend", "ref.fa", "--ext-max-edits", "1024"], "invalid value for --ext-max-edits: must be 0..1023"),
    (["extend", "ref.fa", "-e", "1024"], "invalid value for --max-edits: must be 0..1023"),
    (["extend", "ref.fa", "--max-div", "1001"], "invalid value for --max-div: must be 0..1000"),
    (["extend", "ref.fa", "--min-mapq", "61"], "invalid value for --min-mapq: must be 0..60"),
    (["extend", "ref.fa", "--min-frac", "1001"], "invalid value for --min-frac: must be 0..1000"),
    (["extend", "ref.fa", "in1", "in2"], "extend takes one input: mates are independent here, run it once per file (unexpected argument 'in2')"),
    (["extend", "--nope"], "unexpected argument '--nope'"),
    (["extend", "ref.fa", "--verified-only"], "unexpected argument '--verified-only'"),
    (["extend", "ref.fa", "--pileup"], "missing value for --pileup"),
    (["extend", "ref.fa", "--penalty"], "missing value for --penalty"),
]


@pytest.mark.parametrize("args,message", EXTEND_ERRORS, ids=[" ".join(e[0]) for e in EXTEND_ERRORS])
def test_extend_error_exit_code_and_text(args, message):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "Error: " + message + "\n")


def test_extend_help_text():
    p = subprocess.run([CLI, "extend", "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "extend.txt")) as f:
        want = f.read()
    assert (p.returncode, p.stderr, p.stdout) == (0, "", want)
    for word in ("Usage: deacon-hip extend [OPTIONS] <REF> [READS]", "--penalty <N>", "[default: 6, a convention]", "--end-bonus <N>",
                 "[default: 4, a convention]", "--ext-max-edits <N>", "--pileup <FILE>", "--sites <FILE>", "xl:i:", "xr:i:", "cl:i:", "cr:i:",
                 "--min-mapq <N>", "--all-ranks", "--all-positions", "--min-depth <N>", "--min-frac <N>", "-e, --max-edits <N>", "--max-div <N>",
                 "conventions, not measured optima", "rows_extended", "bases_gained", "bases_clipped", "full_length_rows", "no affine gaps, no SAM"):
        assert word in want, word
    top = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert (top.stdout + top.stderr).count("\n  extend ") == 1 and (top.stdout + top.stderr).count("\n  pileup ") == 1


def test_no_flank_of_one_letter_ties_on_i():
    """the search behind the HAND cases: over the letters A and C, flanks of up to four bases a side, penalty 2, 3 and 6, bonus
    0, 1 and 4, from a plain table: wherever rule X5 comes down to the larger i, one of the two flanks has both letters"""
    import itertools
    ties = 0
    for f, g in itertools.product(range(1, 5), repeat=2):
        for U in itertools.product("AC", repeat=f):
            for V in itertools.product("AC", repeat=g):
                D = [[max(i, j) if 0 in (i, j) else 0 for j in range(g + 1)] for i in range(f + 1)]
                for i in range(1, f + 1):
                    for j in range(1, g + 1):
                        D[i][j] = min(D[i - 1][j - 1] + (U[i - 1] != V[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
                for penalty, bonus in itertools.product((2, 3, 6), (0, 1, 4)):
                    cells = [(i + j - penalty * D[i][j] + (bonus if i == f else 0), -D[i][j], i, j) for i in range(f + 1) for j in range(g + 1)]
                    top = [c for c in cells if c[:2] == max(cells)[:2]]
                    if len(top) > 1:
                        ties += 1
                        assert len(set(U)) == 2 or len(set(V)) == 2, (U, V, penalty, bonus)
    assert ties > 20
