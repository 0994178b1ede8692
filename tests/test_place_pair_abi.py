"""CPU checks of dcn_place_pair_batch's boundary: declared, exported and bound at ABI 1.11, the two structs' layout, the
argument errors that are found before a device is looked at, `deacon-hip map-pairs`'s usage errors and --help, and one
test of the model of the GPU tests (tests/_place_pair_worker.py) alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _place_pair_worker as PPW
import _place_worker as PW
from conftest import random_reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
NAME = "dcn_place_pair_batch"


def test_symbol_is_declared_exported_and_bound(dcn):
    N = dcn._native
    L = C.CDLL(N.LIB_PATH)
    assert NAME in N.declared_symbols() and NAME in N._SIGNATURES and hasattr(L, NAME)
    assert tuple(N.ABI) >= (1, 11)
    major, minor = C.c_uint32(), C.c_uint32()
    assert N.lib().dcn_abi_version(C.byref(major), C.byref(minor)) == 0 and (major.value, minor.value) >= (1, 11)
    header = open(N.HEADER_PATH).read()
    assert re.search(r"1\.11 = dcn_place_pair_batch", header)
    assert int(re.search(r"#define DCN_ABI_MINOR (\d+)", header).group(1)) >= 11
    assert re.search(r"#define DCN_PAIR_HIST_BINS 256\b", header) and N.PAIR_HIST_BINS == 256
    flat = " ".join(header.replace(" *", " ").split())
    assert "THE DEFINITION OF A PAIRED PLACEMENT" in flat and flat.count("NOT a calibrated probability") >= 2
    for name, bit in (("PROPER", 1), ("RESCUED", 2), ("MATE_PLACED", 4)):
        assert re.search(r"#define DCN_PAIR_%s %du\b" % (name, bit), header) and getattr(dcn.filter, "PAIR_" + name) == bit
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"pub const DCN_ABI_MINOR: u32 = (\d+); +//", md).group(1)) >= 11
    assert re.search(r"pub fn %s\(" % NAME, md)
    assert hasattr(dcn.Placer, "place_pair_batch") and hasattr(dcn.Placer, "place_pairs")


def test_struct_layouts(dcn):
    N = dcn._native
    P, B, S = N.PlacePairParams, N.PairPlacement, N.SplitPlacement
    assert C.sizeof(P) == 40 and C.sizeof(B) == 80
    assert (P.band_bases.offset, P.min_votes.offset, P.prefix_length.offset, P.max_placements.offset, P.max_insert.offset,
            P.hist_bin_bases.offset, P.reserved.offset) == (0, 4, 8, 16, 20, 24, 28)
    assert [getattr(B, f).offset for f, _ in B._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 52, 56, 60, 64, 68, 72]
    dt, split = dcn.filter.PAIR_PLACEMENT_DTYPE, dcn.filter.SPLIT_PLACEMENT_DTYPE
    assert dt.itemsize == 80 and list(dt.names) == [f for f, _ in B._fields_]
    assert [dt.fields[f][1] for f in dt.names] == [getattr(B, f).offset for f in dt.names]
    # the first 64 bytes are dcn_split_placement's, field for field
    assert [f for f, _ in B._fields_[:len(S._fields_)]] == [f for f, _ in S._fields_]
    assert list(dt.names[:len(split.names)]) == list(split.names)
    assert all(dt.fields[f] == split.fields[f] for f in split.names)
    assert list(dt.names[len(split.names):]) == ["flags", "pair_votes", "tlen"] and dt.fields["tlen"][0] == np.int64
    header = open(N.HEADER_PATH).read()
    assert re.search(r"\}\s*dcn_place_pair_params;\s*/\* 40 bytes \*/", header)
    assert re.search(r"\}\s*dcn_pair_placement;\s*/\* 80 bytes \*/", header)


def test_header_structs_in_c(tmp_path, dcn):
    src = tmp_path / "t.c"
    src.write_text('#include "deacon_hip.h"\n#include <stddef.h>\n'
                   "int main(void){ return sizeof(dcn_place_pair_params) == 40 && sizeof(dcn_pair_placement) == 80 && "
                   "offsetof(dcn_place_pair_params, max_placements) == 16 && offsetof(dcn_place_pair_params, max_insert) == 20 && "
                   "offsetof(dcn_place_pair_params, hist_bin_bases) == 24 && offsetof(dcn_place_pair_params, reserved) == 28 && "
                   "offsetof(dcn_pair_placement, read_start) == offsetof(dcn_split_placement, read_start) && "
                   "offsetof(dcn_pair_placement, ref_end) == offsetof(dcn_split_placement, ref_end) && "
                   "offsetof(dcn_pair_placement, mapq) == offsetof(dcn_split_placement, mapq) && "
                   "offsetof(dcn_pair_placement, flags) == sizeof(dcn_split_placement) && offsetof(dcn_pair_placement, pair_votes) == 68 && "
                   "offsetof(dcn_pair_placement, tlen) == 72 && (DCN_PAIR_PROPER | DCN_PAIR_RESCUED | DCN_PAIR_MATE_PLACED) == 7 "
                   "? 0 : 1; }\n")
    inc = os.path.dirname(dcn._native.HEADER_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(tmp_path / "t")])
    assert subprocess.call([str(tmp_path / "t")]) == 0


def test_argument_errors_that_need_no_device(dcn):
    """params and the read count are judged first, then the pointers: nothing here is dereferenced"""
    N, L = dcn._native, dcn._native.lib()

    def prm(band=256, votes=2, n=4, insert=1000, hbin=8, r=(0, 0, 0)):
        return C.byref(N.PlacePairParams(band, votes, 0, n, insert, hbin, (C.c_uint32 * 3)(*r)))

    stand_in = (C.c_uint8 * 4096)()

    def call(ctx, map_, params, n_reads=0):
        return L.dcn_place_pair_batch(ctx, map_, None, None, n_reads, params, None, None)

    for args, word in (((None, None, None), b"params is NULL"),
                       ((None, None, prm(r=(1, 0, 0))), b"reserved"),
                       ((None, None, prm(r=(0, 1, 0))), b"reserved"),
                       ((None, None, prm(r=(0, 0, 1))), b"reserved"),
                       ((None, None, prm(band=0)), b"band_bases"),
                       ((None, None, prm(votes=0)), b"min_votes"),
                       ((None, None, prm(n=0)), b"max_placements must be 1..8"),
                       ((None, None, prm(n=9)), b"max_placements must be 1..8"),
                       ((None, None, prm(insert=0)), b"max_insert"),
                       ((None, None, prm(hbin=0)), b"hist_bin_bases"),
                       ((None, None, prm(), 1), b"n_reads must be even"),
                       ((None, None, prm(), 7), b"n_reads must be even"),
                       ((None, None, prm()), b"ctx is NULL"),
                       ((None, None, prm(), 2), b"ctx is NULL"),
                       ((C.cast(stand_in, C.c_void_p), None, prm()), b"map is NULL")):
        assert call(*args) == N.DCN_ERR_ARG
        assert word in L.dcn_last_error(), (word, L.dcn_last_error())


PAIR_ERRORS = [
    (["map-pairs"], "the following required arguments were not provided: <REF>"),
    (["map-pairs", "ref.fa"], "the following required arguments were not provided: <READS1>"),
    (["map-pairs", "ref.fa", "-N", "0"], "invalid value for -N: must be 1..8"),
    (["map-pairs", "ref.fa", "-N", "9"], "invalid value for -N: must be 1..8"),
    (["map-pairs", "ref.fa", "--band", "0"], "invalid value for --band: must be 1..4294967295"),
    (["map-pairs", "ref.fa", "-a", "0"], "invalid value for --min-votes: must be 1..4294967295"),
    (["map-pairs", "ref.fa", "-I", "0"], "invalid value for --max-insert: must be 1..4294967295"),
    (["map-pairs", "ref.fa", "--max-insert", "x"], "invalid value for --max-insert: must be 1..4294967295"),
    (["map-pairs", "ref.fa", "--insert-bin", "0"], "invalid value for --insert-bin: must be 1..4294967295"),
    (["map-pairs", "ref.fa", "--insert-hist"], "missing value for --insert-hist"),
    (["map-pairs", "ref.fa", "in1", "in2", "in3"], "unexpected argument 'in3'"),
    (["map-pairs", "--nope"], "unexpected argument '--nope'"),
]


@pytest.mark.parametrize("args,message", PAIR_ERRORS, ids=[" ".join(e[0]) for e in PAIR_ERRORS])
def test_map_pairs_error_exit_code_and_text(args, message):
    p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", "Error: " + message + "\n")


def test_map_pairs_help_text():
    p = subprocess.run([CLI, "map-pairs", "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "map-pairs.txt")) as f:
        want = f.read()
    assert (p.returncode, p.stderr, p.stdout) == (0, "", want)
    for word in ("Usage: deacon-hip map-pairs [OPTIONS] <REF> <READS1> [READS2]", "-I, --max-insert <N>", "[default: 1000, a convention]",
                 "--insert-hist <FILE>", "--insert-bin <N>", "The quality and -I are conventions, not a calibrated probability", "mt mate",
                 "tl template length", "\nConcordant: ", "\nProper: ", "\nPaired votes of a placement: ", "\nQuality: "):
        assert word in want, word
    top = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "\n  map-pairs " in top.stdout + top.stderr and "\n  map " in top.stdout + top.stderr


def test_model_alone_on_error_free_pairs(oracle):
    """THE ONE TEST HERE THAT PASSES WITHOUT THE FEATURE: it runs the model only.  Random genomes with no repeated k-mer at
    w = 1 (every k-mer an anchor), error-free pairs cut from fragments of 200 .. I bases, as given on either strand: all
    proper, T = the fragment length (the first and the last k-mer of the fragment are hits), tlen = +T on the mate that
    lies first and -T on the other, pair_votes equal on both rows and the sum of the two votes.  Fragments of I + 1
    bases are never proper."""
    O, k, w, I = oracle, 31, 1, 1000
    F = PPW.F
    genomes = random_reads(np.random.default_rng(981), 3, 20_000, 20_000)
    model = PW.AnchorModel(O, k, w, O.Index.build(genomes, k=k, w=w).keys()).add(genomes)
    assert model.info()["repeats"] == 0
    rng = np.random.default_rng(982)
    for i in range(120):
        ln = I + 1 if i % 4 == 3 else (I if i % 4 == 2 else int(rng.integers(200, I + 1)))
        R, at, frag = PPW.fragment(rng, genomes, ln, ln)
        L1, L2 = int(rng.integers(60, 151)), int(rng.integers(60, 151))
        flip = bool(i % 2)
        m1, m2 = PPW.mates_of(frag, L1, L2, flip=flip)
        for n in (1, 4):
            a, b, T = PPW.place_pair(model, m1, m2, max_placements=n, max_insert=I)
            if ln > I:
                assert T is None and not (a[F["flags"]] | b[F["flags"]]) & PPW.PROPER and a[F["tlen"]] == b[F["tlen"]] == 0
                assert a[F["flags"]] == b[F["flags"]] == PPW.MATE_PLACED and a[F["pair_votes"]] == a[F["votes"]]
                continue
            assert T == ln and a[F["flags"]] == b[F["flags"]] == PPW.PROPER | PPW.MATE_PLACED, (i, n, a, b)
            first, second = (b, a) if flip else (a, b)  # (the forward mate lies first: L1, L2 < 200 <= ln)
            assert first[F["tlen"]] == T and second[F["tlen"]] == -T
            assert first[F["ref_start"]] == at and second[F["ref_end"]] == at + ln and first[F["reverse"]] == 0 and second[F["reverse"]] == 1
            assert a[F["pair_votes"]] == b[F["pair_votes"]] == a[F["votes"]] + b[F["votes"]]
            assert a[F["votes"]] == (L2 if flip else L1) - k + 1 and a[F["rival_votes"]] == 0 and a[F["mapq"]] == 60
            assert a[F["record"]] == b[F["record"]] == R and a[F["rank"]] == b[F["rank"]] == 0
    rows, hist = PPW.place_pair_all(model, list(PPW.mates_of(genomes[0][100:400], 100, 100)) * 3, max_insert=I, hist_bin_bases=8)
    assert hist[300 // 8] == 3 and sum(hist) == 3 and len(rows) == 6
