"""`deacon-hip gvcf` end to end, file to file, on a reference of two records (2,400 and 600 bases) under error-free 150-base
reads on alternating strands that leave 300 bases of the first record uncovered and the 300 behind them covered by one or two
reads, and carry a homozygous and a heterozygous SNV, a 2-base insertion and a 2-base deletion; the second record has one SNV.

Without the mode's three options every output is `deacon-hip strand`'s, byte for byte.  --gvcf, less its block lines and its
added header lines, is --vcf.  The block lines are what AnchorMap.reference_blocks and merge_blocks give, whole and cut in
stretches, on a map that the test piles up from the same reads with the tool's defaults (its counters are first compared with
the tool's --pileup table, position by position); they ascend, do not overlap, and no two neighbours could have merged.  The
BED tiles every record.  All files are the same at DCN_CLI_STRETCH_BASES = 1, 7, 1000 and the default.  Exact throughout."""
import gzip
import json
import subprocess

import numpy as np
import pytest

import _blocks_worker as BW
import _quality_worker as QW
import _verify_worker as VW
from conftest import random_reads, revcomp
from test_gpu_pileup_cli import CLI, run

pytestmark = pytest.mark.gpu

LEN_A, LEN_B, READ = 2400, 600, 150
HOM_SNV, HET_SNV, INSERTION, DELETION, SNV_B = 402, 1602, 1900, 2100, 300
SUMMARY = ("blocks", "block_bases", "variant_positions", "no_coverage_bases", "uncalled_bases", "ref_bases", "ref_bases_by_band", "gq_bands")
OUTS = ["-o", "--variants", "--pileup", "--sites", "--duplicates", "--vcf"]
ADDED_HEADER = ("##ALT=<ID=NON_REF,", "##INFO=<ID=END,", "##FORMAT=<ID=MIN_DP,", "##GVCFBlock")
BANDS = (20, 40, 60, 80, 99)


def other(base):
    return next(x for x in b"ACGT" if x != base)


def make_input(d):
    rng = np.random.default_rng(2411)
    a, b = random_reads(rng, 1, LEN_A, LEN_A)[0], random_reads(rng, 1, LEN_B, LEN_B)[0]
    # the gaps where left alignment cannot move them: the base in front of the deletion differs from its last base, and the
    # inserted stretch ends in a base that is not the one in front of it
    dele = next(p for p in range(DELETION, DELETION + 100) if a[p - 1] != a[p + 1] and a[p] != a[p + 2] and a[p] != a[p + 1])
    ins = bytes([other(a[INSERTION + 1]), other(a[INSERTION])])
    starts_a = list(range(0, 551, 5)) + [1000, 1075, 1150] + list(range(1300, LEN_A - READ + 1, 5))  # [700, 1000) bare, [1000, 1300) thin
    reads = []
    for i, s in enumerate(starts_a):
        rev = i % 2
        S = bytearray(a[s:s + READ + 2])
        if s <= HOM_SNV < s + READ:
            S[HOM_SNV - s] = other(a[HOM_SNV])
        if (i // 2) % 2 == 0 and s <= HET_SNV < s + READ:
            S[HET_SNV - s] = other(a[HET_SNV])
        if s + 20 <= dele < s + READ - 20:
            del S[dele - s:dele - s + 2]
        if s + 20 <= INSERTION < s + READ - 20:
            S[INSERTION - s + 1:INSERTION - s + 1] = ins
        S = bytes(S[:READ])
        reads.append(revcomp(S) if rev else S)
    for i, s in enumerate(range(0, LEN_B - READ + 1, 10)):
        S = bytearray(b[s:s + READ])
        if s <= SNV_B < s + READ:
            S[SNV_B - s] = other(b[SNV_B])
        reads.append(revcomp(bytes(S)) if i % 2 else bytes(S))
    quals = [b"I" * len(r) for r in reads]
    with open(d / "ref.fa", "wb") as f:
        f.write(b">chrA\n" + a + b"\n>chrB\n" + b + b"\n")
    with open(d / "reads.fq", "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@read%d\n" % i + r + b"\n+\n" + quals[i] + b"\n")
    return [a, b], reads, quals, dele


def gvcf_files(d, tag, env=None):
    files = [d / ("%s.%s" % (tag, x)) for x in ("g.vcf", "bed", "vcf", "json")]
    run(["gvcf", d / "ref.fa", d / "reads.fq", "-q", "--gvcf", files[0], "--callable", files[1], "--vcf", files[2], "-s", files[3]], env=env)
    summary = json.load(open(files[3]))
    summary.pop("time")
    return [f.read_bytes() for f in files[:3]] + [summary]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("gvcf")
    records, reads, quals, dele = make_input(d)
    got = {}
    for sub in ("strand", "gvcf"):
        files = [d / ("%s_%s" % (sub, o.strip("-") or "fa")) for o in OUTS]
        args = [sub, d / "ref.fa", d / "reads.fq", "-q", "--all-positions", "-s", d / (sub + ".json")]
        for o, f in zip(OUTS, files):
            args += [o, f]
        run(args)
        got[sub] = [f.read_bytes() for f in files]
    return d, records, reads, quals, dele, got, gvcf_files(d, "default")


def body(text):
    return [line.split("\t") for line in text.decode().splitlines() if not line.startswith("#")]


def test_without_the_three_options_the_outputs_are_strands(data):
    d, records, reads, quals, dele, got, files = data
    assert got["gvcf"] == got["strand"] and all(len(x) > 30 for x in got["gvcf"][:4] + got["gvcf"][5:])
    a, b = (json.load(open(d / (sub + ".json"))) for sub in ("strand", "gvcf"))
    assert {k: b[k] for k in a if k != "time"} == {k: a[k] for k in a if k != "time"} and set(b) - set(a) == set(SUMMARY)
    assert files[2] == got["strand"][5]  # --vcf beside --gvcf as well


def test_the_gvcf_less_its_blocks_is_the_vcf(data):
    d, records, reads, quals, dele, got, (gvcf, bed, vcf, summary) = data
    lines = gvcf.decode().splitlines()
    kept = [x for x in lines if not x.startswith(ADDED_HEADER) and not (not x.startswith("#") and x.split("\t")[4] == "<NON_REF>")]
    assert ("\n".join(kept) + "\n").encode() == vcf
    added = [x for x in lines if x.startswith(ADDED_HEADER)]
    assert len(added) == 3 + len(BANDS) + 1 and lines.index(added[-1]) + 1 == next(i for i, x in enumerate(lines) if x.startswith("#CHROM"))
    assert [x for x in added if x.startswith("##GVCFBlock")] == ["##GVCFBlock%d-%d=minGQ=%d(inclusive),maxGQ=%d(exclusive)" % (lo, hi, lo, hi)
                                                                 for lo, hi in zip((0,) + BANDS, BANDS + (100,))]
    variants = {(x[0], int(x[1])): x for x in body(vcf)}
    assert len(variants) == 5 and sum("INDEL" in x[7] for x in variants.values()) == 2
    assert ("chrA", HOM_SNV + 1) in variants and ("chrA", HET_SNV + 1) in variants and ("chrB", SNV_B + 1) in variants
    # in position order, a block's line in front of a variant line of its POS
    order = [(x[0], int(x[1]), x[4] != "<NON_REF>") for x in body(gvcf)]
    assert order == sorted(order)


def test_blocks_ascend_tile_with_the_variants_and_add_up(data):
    d, records, reads, quals, dele, got, (gvcf, bed, vcf, summary) = data
    total = 0
    for name, record in zip(("chrA", "chrB"), records):
        blocks = [(int(x[1]) - 1, int(x[7][4:])) for x in body(gvcf) if x[0] == name and x[4] == "<NON_REF>"]
        assert all(a < b for a, b in blocks) and all(blocks[i][1] <= blocks[i + 1][0] for i in range(len(blocks) - 1))
        assert blocks[0][0] == 0 and blocks[-1][1] == len(record)
        for x in body(gvcf):
            if x[0] == name and x[4] == "<NON_REF>":
                assert x[3] == chr(record[int(x[1]) - 1]) and x[5:7] == [".", "."] and x[7].startswith("END=") and x[8] == "GT:GQ:DP:MIN_DP"
        total += sum(b - a for a, b in blocks)
    assert summary["block_bases"] == total and summary["block_bases"] + summary["variant_positions"] == LEN_A + LEN_B
    assert summary["variant_positions"] == 5 and summary["gq_bands"] == list(BANDS)
    assert summary["no_coverage_bases"] == 300 and summary["uncalled_bases"] >= 200  # [700, 1000) of chrA; most of the thin stretch
    assert summary["ref_bases"] == sum(summary["ref_bases_by_band"]) == total - summary["no_coverage_bases"] - summary["uncalled_bases"]
    assert summary["blocks"] == sum(1 for x in body(gvcf) if x[4] == "<NON_REF>")


def test_the_bed_tiles_every_record(data):
    d, records, reads, quals, dele, got, (gvcf, bed, vcf, summary) = data
    rows = [x.split("\t") for x in bed.decode().splitlines()]
    for name, record in zip(("chrA", "chrB"), records):
        mine = [(int(x[1]), int(x[2]), x[3]) for x in rows if x[0] == name]
        assert mine[0][0] == 0 and mine[-1][1] == len(record) and all(a < b for a, b, _ in mine)
        assert all(mine[i][1] == mine[i + 1][0] and mine[i][2] != mine[i + 1][2] for i in range(len(mine) - 1))
        assert {x[2] for x in mine} <= {"NO_COVERAGE", "LOW_CONFIDENCE", "CALLABLE"}
    assert ("chrA", "700", "1000", "NO_COVERAGE") in {tuple(x) for x in rows}
    callable_bases = sum(int(x[2]) - int(x[1]) for x in rows if x[3] == "CALLABLE")
    assert callable_bases == summary["ref_bases"] + summary["variant_positions"]


def test_block_lines_are_what_the_library_gives_on_the_same_rows(data, dcn, oracle):
    d, records, reads, quals, dele, got, (gvcf, bed, vcf, summary) = data
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    amap.pileup_keep_qualities()
    amap.pileup_keep_deletions()
    amap.pileup_left_align()
    placer = dcn.Placer(amap, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
    try:
        b, o, q = QW.concat(oracle, reads, quals)
        po, srows, _ = placer.place_split_batch(b, o, max_placements=4)
        xrows, _ = placer.extend_batch(b, o, srows, row_offsets=po)
        xrows = xrows.copy()
        xrows["record"][(xrows["mapq"] < 1) | (xrows["rank"] != 0)] = dcn.filter.UNPLACED  # the tool's --min-mapq 1, rank 0 only
        edits, n_added = placer.pileup_batch(b, o, xrows, row_offsets=po, quals=q, min_base_qual=20)
        assert n_added == len(reads)
        # the same rows: the tool's --pileup table, position by position
        table = [x.split("\t") for x in got["gvcf"][2].decode().splitlines()[1:]]
        for R, name in enumerate(("chrA", "chrB")):
            mine = np.array([[int(v) for v in x[3:15]] for x in table if x[0] == name], np.uint32)
            assert np.array_equal(mine[:, :8], amap.pileup_fetch(R)) and np.array_equal(mine[:, 8:], amap.pileup_fetch_qualities(R))
        for R, name in enumerate(("chrA", "chrB")):
            breaks = []
            for x in body(vcf):
                if x[0] == name and "INDEL" in x[7]:
                    breaks.append(int(x[1]) if len(x[3]) > len(x[4]) else int(x[1]) - 1)  # where the event is counted
            assert (R == 0) == (sorted(breaks) == [INSERTION, dele])
            cls, whole = amap.reference_blocks(R, breaks=breaks)
            whole = dcn.merge_blocks(whole)
            assert BW.device_blocks(whole) == BW.merge(BW.device_blocks(whole))  # no two neighbours could have merged
            parts = []
            for lo in range(0, len(records[R]), 333):
                n = min(333, len(records[R]) - lo)
                parts.append(amap.reference_blocks(R, lo, n, breaks=[p for p in breaks if lo <= p < lo + n])[1])
            assert BW.device_blocks(dcn.merge_blocks(np.concatenate(parts))) == BW.device_blocks(whole)
            want = []
            for pos, ln, c, min_gq, min_depth, max_depth, sum_depth in BW.device_blocks(whole):
                gt = "0/0" if c >= BW.REF else "./."
                want.append([name, str(pos + 1), ".", chr(records[R][pos]), "<NON_REF>", ".", ".", "END=%d" % (pos + ln), "GT:GQ:DP:MIN_DP",
                             "%s:%d:%d:%d" % (gt, min_gq, sum_depth // ln, min_depth)])
            assert [x for x in body(gvcf) if x[0] == name and x[4] == "<NON_REF>"] == want
            assert {int(c) for c in cls} >= ({BW.NO_COVERAGE, BW.UNCALLED, BW.VARIANT} if R == 0 else {BW.VARIANT}) and max(w[2] for w in BW.device_blocks(whole)) > BW.REF
    finally:
        placer.close()
        amap.close()


@pytest.mark.parametrize("stretch", ["1", "7", "1000"])
def test_no_output_depends_on_the_stretch(data, stretch):
    d, records, reads, quals, dele, got, files = data
    assert gvcf_files(d, "s" + stretch, env={"DCN_CLI_STRETCH_BASES": stretch}) == files


def test_other_bands_ploidy_and_gz(data):
    d, records, reads, quals, dele, got, (gvcf, bed, vcf, summary) = data
    run(["gvcf", d / "ref.fa", d / "reads.fq", "-q", "--gvcf", d / "z.g.vcf.gz"])
    assert gzip.decompress((d / "z.g.vcf.gz").read_bytes()) == gvcf and (d / "z.g.vcf.gz").read_bytes()[:2] == b"\x1f\x8b"
    one = run(["gvcf", d / "ref.fa", d / "reads.fq", "-q", "--gvcf", "-", "--gq-bands", "50", "--ploidy", "1", "-s", d / "one.json"]).stdout
    lines = [x for x in body(one) if x[4] == "<NON_REF>"]
    assert {x[9].split(":")[0] for x in lines} == {"0", "."} and json.load(open(d / "one.json"))["gq_bands"] == [50]
    assert sum(x.startswith("##GVCFBlock") for x in one.decode().splitlines()) == 2
    for bands, word in (("40,20", b"params.edges[1] is not above the edge in front of it"), ("0", b"params.edges[0] must be 1..99"),
                        (",".join(str(i) for i in range(1, 17)), b"params.n_edges must be 0..15")):
        p = subprocess.run([CLI, "gvcf", str(d / "ref.fa"), str(d / "reads.fq"), "-q", "--gvcf", str(d / "bad.vcf"), "--gq-bands", bands],
                           capture_output=True, timeout=300)
        assert p.returncode == 1 and word in p.stderr, p.stderr
