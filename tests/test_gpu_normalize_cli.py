"""`deacon-hip normalize` end to end, file to file, on the reference and the reads of
tests/test_gpu_left_align_differential.py (planted indels, most of them inside homopolymers and tandem repeats).  The
placements are those `deacon-hip extend` prints for the same input; the model of tests/_left_align_worker.py left-aligns
the runs of each line and piles them up with the reads' quality lines and both ledgers, the models of
tests/_genotype_worker.py and tests/_indel_worker.py genotype them, and the VCF (header and every line, at two settings,
in many batches, in stretches down to one position, as .vcf.gz) and the summary's four fields are compared with them.  Each
planted repeat indel's line stands at the left-most POS, where `deacon-hip indels` puts it further right; on an input
without a gap in a repeat the two modes write the same bytes, apart from the header line and the summary fields.  Every
comparison is exact."""
import gzip
import json

import pytest

import _align_worker as AW
import _genotype_worker as GW
import _indel_worker as DW
import _insertion_worker as IW
import _left_align_worker as LW
import _pileup_worker as PW
import _quality_worker as QW
import _verify_worker as VW
import test_gpu_left_align_differential as DT
from conftest import revcomp
from test_gpu_genotype_cli import version
from test_gpu_pileup_cli import run

pytestmark = pytest.mark.gpu

NAMES = ("chrA", "chrB")
HEADER_LINE = "##left_aligned=The positions of insertions and deletions are left-aligned per read"
SUMMARY = ("left_aligned_rows", "left_aligned_gaps", "left_align_columns", "left_align_merged_gaps")
SMALL = {"DCN_CLI_ALIGN_BATCH_BASES": "9000"}  # many batches
MIN_BASE_QUAL = 20  # (the tool's default)


def write_input(d, records, reads, quals):
    with open(d / "ref.fa", "wb") as f:
        for name, g in zip(NAMES, records):
            f.write(b">" + name.encode() + b"\n" + g + b"\n")
    with open(d / "reads.fq", "wb") as f:
        for i, (r, q) in enumerate(zip(reads, quals)):
            f.write(b"@read%d\n" % i + r + b"\n+\n" + q + b"\n")


def model(paf, genomes, reads, quals, left, changed=None):
    """extend's verified lines of mapq >= 1 and rank 0, their runs left-aligned when `left` -> (counts, sums, insertions,
    deletions, info); changed: a set that receives the numbers of the reads in whose rows a gap moves"""
    counts, sums, ins, dels = PW.new_counts(genomes), QW.new_sums(genomes), IW.new_ledger(genomes), DW.new_ledger(genomes)
    info = dict.fromkeys(LW.INFO_FIELDS, 0)
    for line in paf.decode().splitlines():
        c = line.split("\t")
        tags = dict(t.split(":", 2)[::2] for t in c[12:])
        if int(c[11]) < 1 or tags["rk"] != "0" or tags["ve"] != "1":
            continue
        n, rev, R, a, b = int(c[0][4:]), c[4] == "-", NAMES.index(c[5]), int(c[7]), int(c[8])
        row = dict(read_start=int(c[2]), read_end=int(c[3]), reverse=int(rev))
        S = reads[n][row["read_start"]:row["read_end"]]
        S = revcomp(S) if rev else S
        T = genomes[R][a:b]
        d, runs = AW.align_pair(S, T)
        assert AW.cigar_text(runs) == tags["cg"]
        if left:
            new, (shifted, passed, merges) = LW.left_align(S, T, runs)
            LW.check_properties(S, T, d, [int(x) for x in runs], new)
            LW.add_info(info, dict(rows_aligned=1, rows_changed=int(passed > 0), gaps_shifted=shifted, columns_passed=passed, gaps_merged=merges))
            runs = new
            if passed > 0 and changed is not None:
                changed.add(n)
        if a == b:
            continue
        q = QW.qualities_of_S(quals[n], row, 33)
        PW.add_runs(counts[R], QW.masked(S, q, MIN_BASE_QUAL), a, rev, runs)
        QW.add_sums(sums[R], S, q, a, runs, MIN_BASE_QUAL)
        ins[R] += IW.events_of_runs(S, a, rev, runs)
        dels[R] += DW.deletion_events_of_runs(a, int(rev), runs)
    return counts, sums, ins, dels, info


def vcf_of(piled, genomes, left, ploidy=2, **shared):
    counts, sums, ins, dels, info = piled
    snvs = [GW.genotype_range(counts[R], sums[R], g, **dict(GW.DEFAULTS, ploidy=ploidy, **shared))[2] for R, g in enumerate(genomes)]
    indels = [DW.sites_range(counts[R], ins[R], dels[R], 0, len(g), ploidy=ploidy, **shared) for R, g in enumerate(genomes)]
    lines = DW.vcf_text(version(), NAMES, genomes, snvs, indels, ploidy).splitlines()
    if left:
        at = lines.index(DW.VCF_INDEL_HEADER[-1]) + 1
        lines[at:at] = [HEADER_LINE]
    return ("\n".join(lines) + "\n").encode(), indels


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("normalize")
    records, events, reads, quals, rows = DT.planted()
    write_input(d, records, reads, quals)
    paf = run(["extend", d / "ref.fa", d / "reads.fq", "-q", "-o", "-"]).stdout
    return d, records, events, reads, quals, model(paf, records, reads, quals, True), model(paf, records, reads, quals, False)


ARGS = ["-q", "--keep-duplicates"]


def test_vcf_and_summary_against_the_model(data):
    d, records, events, reads, quals, piled, plain = data
    want, _ = vcf_of(piled, records, True)
    info = piled[4]
    assert info["rows_changed"] >= 50 and HEADER_LINE.encode() in want and want != vcf_of(plain, records, False)[0]
    args = ["normalize", d / "ref.fa", d / "reads.fq"] + ARGS
    p = run(args + ["--vcf", d / "n.vcf", "-s", d / "n.json"])
    assert (d / "n.vcf").read_bytes() == want and p.stdout == b""
    s = json.load(open(d / "n.json"))
    assert [s[k] for k in SUMMARY] == [info["rows_changed"], info["gaps_shifted"], info["columns_passed"], info["gaps_merged"]]
    # many batches, short stretches down to one position, .gz
    run(args + ["--vcf", d / "small.vcf", "-s", d / "small.json"], env=SMALL)
    assert (d / "small.vcf").read_bytes() == want and [json.load(open(d / "small.json"))[k] for k in SUMMARY] == [s[k] for k in SUMMARY]
    for stretch in ("64", "1"):
        assert run(args + ["--vcf", "-"], env={"DCN_CLI_STRETCH_BASES": stretch}).stdout == want, stretch
    run(args + ["--vcf", d / "n.vcf.gz"], env=SMALL)
    assert gzip.decompress((d / "n.vcf.gz").read_bytes()) == want and (d / "n.vcf.gz").read_bytes()[:2] == b"\x1f\x8b"


def test_another_setting_against_the_model(data):
    d, records, events, reads, quals, piled, plain = data
    want, _ = vcf_of(piled, records, True, ploidy=1, min_gq=0, min_qual=0, min_depth=1)
    p = run(["normalize", d / "ref.fa", d / "reads.fq", "--vcf", "-", "--ploidy", "1", "--min-gq", "0", "--min-qual", "0", "--min-depth", "1"] + ARGS, env=SMALL)
    assert p.stdout == want


def test_planted_repeat_indels_stand_at_the_leftmost_pos(data):
    """each planted indel's line at the left-most POS, with REF and ALT that do not end in the same base; `indels` on the same
    input has the repeat indels further right (and is the model's own on rule A3's runs)"""
    d, records, events, reads, quals, piled, plain = data
    loose = ["--min-gq", "0", "--min-qual", "0"]
    got = run(["normalize", d / "ref.fa", d / "reads.fq", "--vcf", "-"] + ARGS + loose).stdout
    assert got == vcf_of(piled, records, True, min_gq=0, min_qual=0)[0]
    old = run(["indels", d / "ref.fa", d / "reads.fq", "--vcf", "-"] + ARGS + loose).stdout
    assert old == vcf_of(plain, records, False, min_gq=0, min_qual=0)[0]

    def indel_lines(text):
        return {(x[0], int(x[1]), x[3], x[4]) for x in (y.split("\t") for y in text.decode().splitlines() if "\tINDEL;" in y)}
    new_lines, old_lines = indel_lines(got), indel_lines(old)
    moved = 0
    for (R, pos, flags, ln, bases), e in zip(DT.expected_sites(records, events), events):
        ref = VW.fetched_text(records[R]).decode()
        site = (pos, flags, ln, bases)
        vpos, ref_allele, alt = DW.indel_alleles(VW.fetched_text(records[R]), site)
        assert (NAMES[R], vpos, ref_allele, alt) in new_lines, (NAMES[R], vpos, ref_allele, alt)
        in_repeat = pos != (e[1] if flags else e[1] - 1)
        if in_repeat:
            assert ref_allele[-1] != alt[-1] and (NAMES[R], vpos, ref_allele, alt) not in old_lines
            # (further right, and of the same kind; not always of the same length: where the bases behind a repeat begin like its
            # unit, rule A3 splits a gap of three bases into one of one and one of two, which N4 merges again)
            assert any(x[0] == NAMES[R] and vpos < x[1] <= vpos + 40 and (len(x[2]) > len(x[3])) == (len(ref_allele) > len(alt)) for x in old_lines), \
                (vpos, ref[vpos - 1:vpos + 20])
            moved += 1
    assert moved >= len(DT.REPEATS)  # (every indel planted in a repeat, and a plain deletion that happens to repeat the base in front of it)


def test_an_input_without_gaps_in_repeats_gives_the_bytes_of_indels(tmp_path):
    records, events, reads, quals, rows = DT.planted(seed=2224, n_reads=250, repeats=False)
    write_input(tmp_path, records, reads, quals)
    # the few reads in whose placements, as the tool extends them, a gap can move all the same (by a base, at a read's end) go
    moving = set()
    model(run(["extend", tmp_path / "ref.fa", tmp_path / "reads.fq", "-q", "-o", "-"]).stdout, records, reads, quals, True, moving)
    reads, quals = ([x for n, x in enumerate(xs) if n not in moving] for xs in (reads, quals))
    assert len(reads) >= 240
    write_input(tmp_path, records, reads, quals)
    piled = model(run(["extend", tmp_path / "ref.fa", tmp_path / "reads.fq", "-q", "-o", "-"]).stdout, records, reads, quals, True)
    assert piled[4]["rows_changed"] == 0 and piled[4]["rows_aligned"] >= 240 and sum(len(x) for x in piled[2]) > 10 and sum(len(x) for x in piled[3]) > 10
    outs = ["-o", "--variants", "--pileup", "--sites", "--duplicates", "--vcf"]
    got = {}
    for sub in ("indels", "normalize"):
        files = [tmp_path / ("%s_%s" % (sub, o.strip("-") or "fa")) for o in outs]
        args = [sub, tmp_path / "ref.fa", tmp_path / "reads.fq", "-q", "-s", tmp_path / (sub + ".json")]
        for o, f in zip(outs, files):
            args += [o, f]
        run(args)
        got[sub] = [f.read_bytes() for f in files]
    a, b = (json.load(open(tmp_path / (sub + ".json"))) for sub in ("indels", "normalize"))
    assert [b[k] for k in SUMMARY] == [0, 0, 0, 0] and b["deletion_events"] > 10 and b["insertion_events"] > 10  # gaps, none of which can move
    assert got["normalize"][:5] == got["indels"][:5] and all(len(x) > 30 for x in got["indels"][:4])
    assert got["normalize"][5].decode().replace(HEADER_LINE + "\n", "", 1).encode() == got["indels"][5] and HEADER_LINE.encode() in got["normalize"][5]
    assert {k: b[k] for k in a if k != "time"} == {k: a[k] for k in a if k != "time"} and set(b) - set(a) == set(SUMMARY)
