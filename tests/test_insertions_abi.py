"""CPU checks of the insertion-ledger surface (dcn_anchor_map_pileup_keep_insertions, dcn_anchor_map_insertions_info / _fetch /
_call): declared, exported and bound at ABI 1.17, the layout of its two structs in ctypes, numpy and C99, the argument errors
that are found before a device is looked at, `deacon-hip consensus`'s usage errors and --help, the ledger's walk and winner
rule compiled for the host under the sanitizers, and the model of the GPU tests (tests/_insertion_worker.py) alone on cases
whose answers are written out here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _align_worker as AW
import _insertion_worker as IW
import _pileup_worker as PW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
SYMBOLS = {"dcn_anchor_map_pileup_keep_insertions": 2, "dcn_anchor_map_insertions_info": 3, "dcn_anchor_map_insertions_fetch": 10,
           "dcn_anchor_map_insertions_call": 11}


def test_symbols_are_declared_exported_and_bound(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    for name, n_args in SYMBOLS.items():
        assert name in N.declared_symbols() and name in N._SIGNATURES and hasattr(L, name), name
        assert len(N._SIGNATURES[name][1]) == n_args
    assert len(N.declared_symbols()) >= 95
    assert tuple(N.ABI) >= (1, 17)
    major, minor = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(major), C.byref(minor)) == 0 and (major.value, minor.value) >= (1, 17)
    header = open(N.HEADER_PATH).read()
    assert len(re.findall(r"1\.17 = dcn_anchor_map_pileup_keep_insertions, dcn_anchor_map_insertions_info / _fetch / _call", header)) == 1
    assert int(re.search(r"#define DCN_ABI_MINOR (\d+)", header).group(1)) >= 17
    for name, value in (("FRONT", 1), ("REVERSE", 2)):
        assert re.search(r"#define DCN_INSERTION_%s %du\b" % (name, value), header)
        assert getattr(N, "INSERTION_" + name) == getattr(dcn, "INSERTION_" + name) == value and "INSERTION_" + name in dcn.__all__
    assert (IW.FRONT, IW.REVERSE) == (N.INSERTION_FRONT, N.INSERTION_REVERSE)
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"pub const DCN_ABI_MINOR: u32 = (\d+); +//", md).group(1)) >= 17
    for name in SYMBOLS:
        assert re.search(r"pub fn %s\(" % name, md), name
    assert "pub struct dcn_insertion {" in md and "pub struct dcn_insertion_allele {" in md
    for method in ("pileup_keep_insertions", "insertions_info", "insertions_fetch", "insertions_call", "consensus"):
        assert hasattr(dcn.AnchorMap, method)
    for name in ("INSERTION_DTYPE", "INSERTION_ALLELE_DTYPE"):
        assert getattr(dcn, name) is getattr(dcn.filter, name) and name in dcn.__all__


def test_the_definition_is_stated_once(dcn):
    flat = " ".join(open(dcn._native.HEADER_PATH).read().replace(" *", " ").split())
    assert flat.count("THE DEFINITION OF AN INSERTION LEDGER") == 1
    assert flat.count("THE DEFINITION OF A PILEUP") == 1 and flat.count("THE DEFINITION OF AN EXTENDED PLACEMENT") == 1
    for i in range(1, 9):
        assert len(re.findall(r"\bL%d\." % i, flat)) == 1, i
        assert len(re.findall(r"\bX%d\." % i, flat)) == 1, i
    assert "quadratic in the events of ONE position" in flat and "DCN_INSERTION_LEDGER_EVENTS" in flat


def test_struct_layouts_agree(tmp_path, dcn):
    N = dcn._native
    for S, dt, size, offsets in ((N.Insertion, dcn.INSERTION_DTYPE, 24, (0, 8, 16, 20)), (N.InsertionAllele, dcn.INSERTION_ALLELE_DTYPE, 32, (0, 8, 16, 20, 24, 28))):
        assert C.sizeof(S) == dt.itemsize == size
        assert tuple(getattr(S, f).offset for f, _ in S._fields_) == offsets == tuple(dt.fields[f][1] for f in dt.names)
        assert [f for f, _ in S._fields_] == list(dt.names)
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "deacon_hip.h"\n'
                   "int (*f1)(dcn_index *, int) = dcn_anchor_map_pileup_keep_insertions;\n"
                   "int (*f2)(const dcn_index *, uint64_t *, uint64_t *) = dcn_anchor_map_insertions_info;\n"
                   "int (*f3)(const dcn_index *, uint32_t, uint64_t, uint64_t, void *, uint64_t, uint8_t *, uint64_t, uint64_t *,\n"
                   "          uint64_t *) = dcn_anchor_map_insertions_fetch;\n"
                   "int (*f4)(const dcn_index *, const void *, uint32_t, uint64_t, uint64_t, void *, uint64_t, uint8_t *, uint64_t, uint64_t *,\n"
                   "          uint64_t *) = dcn_anchor_map_insertions_call;\n"
                   "int main(void){ dcn_insertion e = {7, 0, 3, DCN_INSERTION_FRONT | DCN_INSERTION_REVERSE}; dcn_insertion_allele a = {7, 0, 3, 2, 5, 0};\n"
                   "  return sizeof e == 24 && sizeof a == 32 && offsetof(dcn_insertion, pos) == 0 && offsetof(dcn_insertion, bases_offset) == 8 &&\n"
                   "         offsetof(dcn_insertion, len) == 16 && offsetof(dcn_insertion, flags) == 20 && offsetof(dcn_insertion_allele, pos) == 0 &&\n"
                   "         offsetof(dcn_insertion_allele, bases_offset) == 8 && offsetof(dcn_insertion_allele, len) == 16 &&\n"
                   "         offsetof(dcn_insertion_allele, count) == 20 && offsetof(dcn_insertion_allele, events) == 24 &&\n"
                   "         offsetof(dcn_insertion_allele, flags) == 28 && e.flags == 3u && a.events == 5 && DCN_ABI_MINOR >= 17 ? 0 : 1; }\n")
    inc = os.path.dirname(N.HEADER_PATH)
    libdir = os.path.dirname(N.LIB_PATH)  # (the function pointers are initialised and never called)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(tmp_path / "t"), "-L", libdir,
                           "-ldeacon_hip", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"])
    assert subprocess.call([str(tmp_path / "t")]) == 0


def test_argument_errors_that_need_no_device(dcn):
    """NULL map; the parameters of a call before the map is looked at, word for word as dcn_anchor_map_pileup_call reports
    them; NULL count pointers"""
    N, L = dcn._native, dcn._native.lib()
    n, m = C.c_uint64(77), C.c_uint64(78)
    good = C.byref(N.PileupCallParams(3, 500, (C.c_uint32 * 2)(0, 0)))
    for rc in (L.dcn_anchor_map_pileup_keep_insertions(None, 1), L.dcn_anchor_map_pileup_keep_insertions(None, 0),
               L.dcn_anchor_map_insertions_info(None, C.byref(n), C.byref(m)),
               L.dcn_anchor_map_insertions_fetch(None, 0, 0, 1, None, 0, None, 0, C.byref(n), C.byref(m)),
               L.dcn_anchor_map_insertions_call(None, good, 0, 0, 1, None, 0, None, 0, C.byref(n), C.byref(m))):
        assert rc == N.DCN_ERR_ARG and b"map is NULL" in L.dcn_last_error()
    for params in (None, C.byref(N.PileupCallParams(3, 1001, (C.c_uint32 * 2)(0, 0))), C.byref(N.PileupCallParams(3, 500, (C.c_uint32 * 2)(1, 0))),
                   C.byref(N.PileupCallParams(3, 500, (C.c_uint32 * 2)(0, 9)))):
        assert L.dcn_anchor_map_pileup_call(None, params, 0, 0, 1, None, None, None, 0, C.byref(n)) == N.DCN_ERR_ARG
        message = L.dcn_last_error()
        assert L.dcn_anchor_map_insertions_call(None, params, 0, 0, 1, None, 0, None, 0, C.byref(n), C.byref(m)) == N.DCN_ERR_ARG
        assert L.dcn_last_error() == message and message
    for a, b in ((None, C.byref(m)), (C.byref(n), None)):
        assert L.dcn_anchor_map_insertions_fetch(None, 0, 0, 1, None, 0, None, 0, a, b) == N.DCN_ERR_ARG
        assert b"n_events/n_inserted is NULL" in L.dcn_last_error()
        assert L.dcn_anchor_map_insertions_call(None, good, 0, 0, 1, None, 0, None, 0, a, b) == N.DCN_ERR_ARG
        assert b"n_alleles/n_inserted is NULL" in L.dcn_last_error()
    assert (n.value, m.value) == (77, 78)  # (nothing is written by a refused call)


def test_walk_and_winner_on_the_host(tmp_path):
    """tests/cpp/insertion_walk_test.cpp: dcn_insertions.h's counting and writing walk in the kernel's shape (chunks of 64
    runs, the prefix emulated serially, 64 lanes) into event and base arrays of exactly the counted size between guards,
    against a walk step by step, and the winner rule against a sort and count, under the address and undefined-behaviour
    sanitizers: 4,000 random run lists, I first and last, 63 / 64 / 65 / 129 runs, I runs of 1, 63, 64, 65 bases, an I run
    as the 64th and as the 65th run"""
    exe = tmp_path / "insertion_walk_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-I", os.path.join(ROOT, "deacon-server_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "insertion_walk_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "insertion walk ok: 4000 run lists" in out.stdout, out.stderr[-2000:]


CONSENSUS_ERRORS = [
    (["consensus"], "the following required arguments were not provided: <REF>"),
    (["consensus", "ref.fa", "--min-mapq", "61"], "invalid value for --min-mapq: must be 0..60"),
    (["consensus", "ref.fa", "--min-frac", "1001"], "invalid value for --min-frac: must be 0..1000"),
    (["consensus", "ref.fa", "-e", "1024"], "invalid value for --max-edits: must be 0..1023"),
    (["consensus", "ref.fa", "--penalty", "1"], "invalid value for --penalty: must be 2..255"),
    (["consensus", "ref.fa", "in1", "in2"], "consensus takes one input: mates are independent here, run it once per file (unexpected argument 'in2')"),
    (["consensus", "--nope"], "unexpected argument '--nope'"),
    (["consensus", "ref.fa", "--verified-only"], "unexpected argument '--verified-only'"),
    (["consensus", "ref.fa", "--variants"], "missing value for --variants"),
    (["consensus", "ref.fa", "--fill-ref", "-o"], "missing value for -o"),
]


@pytest.mark.parametrize("args,message", CONSENSUS_ERRORS, ids=[" ".join(e[0]) for e in CONSENSUS_ERRORS])
def test_consensus_error_exit_code_and_text(args, message):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "Error: " + message + "\n")


def test_consensus_help_text():
    p = subprocess.run([CLI, "consensus", "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "consensus.txt")) as f:
        want = f.read()
    assert (p.returncode, p.stderr, p.stdout) == (0, "", want)
    for word in ("Usage: deacon-hip consensus [OPTIONS] <REF> [READS]", "record pos type ref alt depth count events", "--variants <FILE>", "--fill-ref",
                 "--min-depth <N>", "--min-frac <N>", "--min-mapq <N>", "--all-ranks", "--penalty <N>", "--end-bonus <N>", "--ext-max-edits <N>",
                 "--max-div <N>", "--pileup <FILE>", "--sites <FILE>", "The thresholds are conventions, not measured optima",
                 "VCF, base qualities and affine gaps are not built", "insertion_events", "uncalled_positions"):
        assert word in want, word
    top = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert (top.stdout + top.stderr).count("\n  consensus ") == 1 and "\n  extend " in top.stdout + top.stderr
    # the other modes of the same driver do not know consensus's options
    for sub in ("map", "verify", "align", "pileup", "extend"):
        for opt in ("--variants", "--fill-ref"):
            q = subprocess.run([CLI, sub, "ref.fa", opt, "x"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
            assert (q.returncode, q.stderr) == (1, "Error: unexpected argument '%s'\n" % opt)


# ---- the model alone ---------------------------------------------------------------------------------------------------
HAND = [
    # (S, T, reverse, the runs, the events with ref_start = 1, why)
    (b"ACCGT", b"AGT", 0, "1=2I2=", [(1, 0, 2, b"CC", 0)], "an I run of two behind base 0 of T"),
    (b"CCAGT", b"AGT", 0, "2I3=", [(1, 1, 2, b"CC", 0)], "an I run first: in front of ref_start"),
    (b"AGTCC", b"AGT", 0, "3=2I", [(3, 0, 2, b"CC", 0)], "an I run last: behind the last base"),
    (b"ACCGT", b"AGT", 1, "1=2I2=", [(1, 0, 2, b"CC", 1)], "a reverse row: S is already turned, the bases are the record's direction"),
    (b"AnxGT", b"AGT", 0, "1=2I2=", [(1, 0, 2, b"NN", 0)], "invalid bases are N"),
    (b"ActGT", b"AGT", 0, "1=2I2=", [(1, 0, 2, b"CT", 0)], "lower case is kept as upper case"),
]


@pytest.mark.parametrize("S,T,reverse,text,want,why", HAND, ids=["%s/%s/%d" % (h[0].decode(), h[1].decode(), h[2]) for h in HAND])
def test_model_alone_on_rows_written_out(S, T, reverse, text, want, why):
    """THE TESTS HERE THAT PASS WITHOUT THE FEATURE: this one and the four below run the model only"""
    d, runs = AW.align_pair(S, T)
    assert AW.cigar_text(runs) == text, why
    assert IW.events_of_runs(S, 1, reverse, runs) == want, why
    counts = np.zeros((len(T) + 2, 8), np.int64)
    PW.add_runs(counts, S, 1, reverse, runs)
    assert counts[:, PW.INS].sum() == len(want) and counts[want[0][0], PW.INS] == 1  # rule L2: #events = INS, at p


def ev(p, front, bases, reverse=0):
    return (p, front, len(bases), bases, reverse)


WINNERS = [
    ([ev(5, 0, b"AC")] * 3 + [ev(5, 0, b"AG")] * 2, (0, 2, b"AC"), 3, "two alleles 3:2"),
    ([ev(5, 0, b"AG")] * 2 + [ev(5, 0, b"AC")] * 3, (0, 2, b"AC"), 3, "... in any order"),
    ([ev(5, 0, b"ACG")] * 2 + [ev(5, 0, b"TT")] * 2, (0, 2, b"TT"), 2, "a 2:2 tie: the shorter"),
    ([ev(5, 1, b"A")] * 2 + [ev(5, 0, b"TTT")] * 2, (0, 3, b"TTT"), 2, "a 2:2 tie: front 0 before front 1, whatever the length"),
    ([ev(5, 0, b"ATA")] * 2 + [ev(5, 0, b"ANA")] * 2, (0, 3, b"ANA"), 2, "a 2:2 tie by bytes: N before T"),
    ([ev(5, 0, b"AC", 0), ev(5, 0, b"AC", 1), ev(5, 0, b"G", 0)], (0, 2, b"AC"), 2, "the strand is not part of an allele"),
]


@pytest.mark.parametrize("events,allele,count,why", WINNERS, ids=[w[-1] for w in WINNERS])
def test_model_alone_on_winners_written_out(events, allele, count, why):
    """... rule L5"""
    assert IW.winner(events) == (allele, count), why
    assert IW.fetch_range(events[::-1], 5, 1) == sorted(events) and IW.fetch_range(events, 6, 3) == [] and IW.fetch_range(events, 0, 5) == []


def test_model_alone_on_the_order_of_events():
    """... rule L4: p, front 0 before 1, the shorter, the bytes (A < C < G < N < T), reverse 0 before 1"""
    want = [ev(2, 1, b"T"), ev(3, 0, b"C"), ev(3, 0, b"AA"), ev(3, 0, b"AC"), ev(3, 0, b"AG"), ev(3, 0, b"AN"), ev(3, 0, b"AT", 0), ev(3, 0, b"AT", 1),
            ev(3, 1, b"A"), ev(4, 0, b"A")]
    assert IW.fetch_range(want[::-1], 0, 10) == want and IW.fetch_range(want[3:] + want[:3], 3, 1) == want[1:9]


def counts_of(n, **at):
    """n positions of depth 4 in column A, with the columns of `at` = {position: {column: count}} put in"""
    c = np.zeros((n, 8), np.int64)
    c[:, PW.A] = 4
    for p, cols in at.items():
        for name, v in cols.items():
            c[int(p[1:]), getattr(PW, name)] = v
    return c


def test_model_alone_on_calls_and_consensus_written_out():
    """... rules L6 and L7: the threshold met exactly and missed by one event, min_permille = 0 at a position without events,
    an insertion behind a deleted position and behind an uncalled one, a front insertion, with and without fill"""
    rec = b"AAAAAAAA"
    # position 2: INS * 1000 = depth * permille (2 of 4 at 500); position 4: one event fewer
    counts = counts_of(8, p2=dict(INS=2), p4=dict(INS=1))
    events = [ev(2, 0, b"GG")] * 2 + [ev(4, 0, b"C")]
    assert IW.call_range(counts, events, rec) == [(2, 0, 2, b"GG", 2, 2)]
    assert IW.consensus(counts, events, rec) == b"AAAGGAAAAA"
    # min_permille = 0 flags every deep position (P6): only those with INS > 0 have a called insertion
    assert IW.call_range(counts, events, rec, min_permille=0) == [(2, 0, 2, b"GG", 2, 2), (4, 0, 1, b"C", 1, 1)]
    assert IW.consensus(counts, events, rec, min_permille=0) == b"AAAGGAACAAA"
    assert IW.call_range(counts, events, rec, 3, 4) == [] and IW.call_range(counts, events, rec, 2, 1) == [(2, 0, 2, b"GG", 2, 2)]
    assert IW.call_range(counts, events, rec, 3, 4, min_permille=0) == [(4, 0, 1, b"C", 1, 1)]
    # behind a deleted position (3: DEL wins), behind an uncalled one (5: deep, four bases 1:1:1:1), at one that is not deep (6),
    # in front of base 0
    counts = counts_of(8, p3=dict(A=1, DEL=3, INS=2), p5=dict(A=1, C=1, G=1, T=1, INS=2), p6=dict(A=1, C=1, INS=2), p0=dict(INS=3))
    events = [ev(3, 0, b"TT")] * 2 + [ev(5, 0, b"G")] * 2 + [ev(6, 0, b"G")] * 2 + [ev(0, 1, b"CC")] * 2 + [ev(0, 0, b"T")]
    rec = b"AAAAAAcn"
    assert IW.call_range(counts, events, rec) == [(0, 1, 2, b"CC", 2, 3), (3, 0, 2, b"TT", 2, 2), (5, 0, 1, b"G", 2, 2)]  # (6: depth 2 < 3)
    assert IW.consensus(counts, events, rec) == b"CCAAATTANGNA"
    assert IW.consensus(counts, events, rec, fill_ref=True) == b"CCAAATTAAGCA"
    assert IW.call_range(counts, events, rec, min_depth=2)[3:] == [(6, 0, 1, b"G", 2, 2)]
    assert IW.consensus(counts, events, rec, min_depth=2) == b"CCAAATTANGAGA"  # (6 is now called: A before C)
    counts[7] = 0  # depth 0: never called, filled, and the record's n is an N
    assert IW.consensus(counts, events, rec, fill_ref=True) == b"CCAAATTAAGCN" and IW.consensus(counts, events, rec) == b"CCAAATTANGNN"

def test_model_alone_end_to_end():
    """... a 600-base record, a truth with one substitution, a 2-base deletion and a 3-base insertion, error-free 100-base
    reads from the truth every 5 bases on alternating strands, rows from the model's own alignment: the model's consensus
    with fill from the reference is the truth, exactly (tests/_insertion_worker.py fixes the seed so that this holds)"""
    record, truth, reads, rows = IW.truth_case()
    assert len(record) == 600 and len(truth) == 601 and len(reads) == 101 and sorted(set(rows["reverse"].tolist())) == [0, 1]
    counts, ledger = PW.new_counts([record]), IW.new_ledger([record])
    edits, n_added = IW.pile_rows(counts, ledger, reads, [record], rows)
    assert n_added == len(reads) and int(edits.max()) <= 6
    assert IW.consensus(counts[0], ledger[0], record, fill_ref=True) == truth
    plain = IW.consensus(counts[0], ledger[0], record)
    assert plain[:2] == b"NN" and plain[-2:] == b"NN" and plain.strip(b"N") in truth  # (the ends are below min_depth)
    (p, front, ln, bases, count, events), = IW.call_range(counts[0], ledger[0], record)
    assert (p, front, ln, bases) == (449, 0, 3, truth[448:451])  # (two bases are deleted in front of it) and count <= events == int(counts[0][449, PW.INS])
