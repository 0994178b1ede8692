"""`deacon-hip indels` end to end, file to file, on tests/test_gpu_call_cli.py's reference, reads and qualities (two planted
indels under every read, and random ones in a fifth of the reads).  The placements are those `deacon-hip extend` prints for
the same input; the models of tests/_quality_worker.py and tests/_indel_worker.py pile those lines up with the reads'
quality lines and both ledgers, those of tests/_genotype_worker.py and tests/_indel_worker.py genotype them, and the VCF
(header and every line, at ploidy 2 and 1, small batches, .vcf.gz) and the summary's new fields are compared with them.
-o, --variants, --pileup, --sites and --duplicates are `deacon-hip markdup`'s for the same input, byte for byte, and so is the
VCF with its INDEL lines and the three header lines removed.  A second reference has a record shorter than the reads, with
indels at and next to its first and last base.  Every comparison is exact."""
import gzip
import json
import re

import numpy as np
import pytest

import _align_worker as AW
import _genotype_worker as GW
import _indel_worker as DW
import _insertion_worker as IW
import _pileup_worker as PW
import _quality_worker as QW
import _verify_worker as VW
from conftest import random_reads, revcomp
from test_gpu_call_cli import _ALIGNED, data, model  # noqa: F401 (data is a fixture)
from test_gpu_consensus_cli import DEL_AT, NAMES, other
from test_gpu_genotype_cli import version
from test_gpu_pileup_cli import run

pytestmark = pytest.mark.gpu

SMALL = {"DCN_CLI_ALIGN_BATCH_BASES": "9000"}  # many batches


def deletions_of(paf, genomes):
    """rule R2 over the lines tests/test_gpu_call_cli.py's model piles up, with the runs it has aligned"""
    dels = DW.new_ledger(genomes)
    for line in paf.decode().splitlines():
        c = line.split("\t")
        tags = dict(t.split(":", 2)[::2] for t in c[12:])
        if int(c[11]) < 1 or tags["rk"] != "0" or tags["ve"] != "1" or int(c[8]) == int(c[7]):
            continue
        dels[NAMES.index(c[5])] += DW.deletion_events_of_runs(int(c[7]), int(c[4] == "-"), _ALIGNED[line])
    return dels


@pytest.fixture(scope="module")
def piled(data):  # noqa: F811
    d, genomes, truths, reads, quals = data
    paf = run(["extend", d / "ref.fa", d / "reads.fq", "-q", "-o", "-"]).stdout
    counts, sums, ins, added = model(paf, genomes, reads, quals)
    assert added > 300
    return counts, sums, ins, deletions_of(paf, genomes)


def expected(piled, genomes, ploidy=2, indel_qual=20, min_indel_count=2, **shared):
    """-> (the VCF's text, the summary's new fields); shared: min_depth, min_gq, min_qual"""
    counts, sums, ins, dels = piled
    snvs = [GW.genotype_range(counts[R], sums[R], g, **dict(GW.DEFAULTS, ploidy=ploidy, **shared))[2] for R, g in enumerate(genomes)]
    indels = [DW.sites_range(counts[R], ins[R], dels[R], 0, len(g), ploidy=ploidy, indel_centi=100 * indel_qual, min_count=min_indel_count, **shared)
              for R, g in enumerate(genomes)]
    flat = [s for sites in indels for s in sites]
    n_del = sum(1 for s in flat if s[1] & DW.INDEL_DELETION)
    hom = sum(1 for s in flat if s[8] == ploidy)
    fields = dict(indel_qual=indel_qual, min_indel_count=min_indel_count, deletion_events=sum(len(x) for x in dels),
                  deleted_bases=sum(e[1] for x in dels for e in x), indel_sites=len(flat), insertion_sites=len(flat) - n_del, deletion_sites=n_del,
                  het_indel_sites=len(flat) - hom, hom_indel_sites=hom)
    return DW.vcf_text(version(), NAMES, genomes, snvs, indels, ploidy).encode(), fields


def test_vcf_and_summary_against_the_model(data, piled):  # noqa: F811
    d, genomes, truths, reads, quals = data
    want, fields = expected(piled, genomes)
    body = [x.split("\t") for x in want.decode().splitlines() if not x.startswith("#")]
    indel = [x for x in body if x[7].startswith("INDEL;")]
    # the model alone: INDEL lines beside SNV lines (the planted ones: test_other_settings_against_the_model)
    assert fields["indel_sites"] == len(indel) >= 1 and len(body) - len(indel) >= 3 and fields["deletion_events"] > 50
    assert [int(x[1]) for x in body if x[0] == "chrA"] == sorted(int(x[1]) for x in body if x[0] == "chrA")  # non-descending POS
    args = ["indels", d / "ref.fa", d / "reads.fq", "-q", "--keep-duplicates"]
    p = run(args + ["--vcf", d / "i.vcf", "-s", d / "i.json"])
    assert (d / "i.vcf").read_bytes() == want and p.stdout == b""
    s = json.load(open(d / "i.json"))
    assert {k: s[k] for k in fields} == fields and s["ploidy"] == 2 and s["keep_duplicates"] is True
    assert run(args + ["--vcf", "-"]).stdout == want
    # many batches, .gz
    run(args + ["--vcf", d / "small.vcf", "-s", d / "small.json"], env=SMALL)
    assert (d / "small.vcf").read_bytes() == want and {k: json.load(open(d / "small.json"))[k] for k in fields} == fields
    run(args + ["--vcf", d / "i.vcf.gz"], env=SMALL)
    assert gzip.decompress((d / "i.vcf.gz").read_bytes()) == want and (d / "i.vcf.gz").read_bytes()[:2] == b"\x1f\x8b"


@pytest.mark.parametrize("args,params", [(["--ploidy", "1"], dict(ploidy=1)),
                                         (["--min-gq", "0"], dict(min_gq=0)),
                                         (["--indel-qual", "100", "--min-indel-count", "1", "--min-depth", "1", "--min-gq", "0", "--min-qual", "0"],
                                          dict(indel_qual=100, min_indel_count=1, min_depth=1, min_gq=0, min_qual=0)),
                                         (["--indel-qual", "1000", "--min-indel-count", "5", "--min-depth", "8", "--min-gq", "60", "--min-qual", "150"],
                                          dict(indel_qual=1000, min_indel_count=5, min_depth=8, min_gq=60, min_qual=150)),
                                         (["--indel-qual", "0"], dict(indel_qual=0))],
                         ids=["ploidy1", "gq0", "loose", "strict", "free"])
def test_other_settings_against_the_model(data, piled, args, params):  # noqa: F811
    d, genomes, truths, reads, quals = data
    want, fields = expected(piled, genomes, **params)
    p = run(["indels", d / "ref.fa", d / "reads.fq", "-q", "--keep-duplicates", "--vcf", "-", "-s", d / "o.json"] + args, env=SMALL)
    assert p.stdout == want
    s = json.load(open(d / "o.json"))
    assert {k: s[k] for k in fields} == fields
    if params.get("min_indel_count") == 1:  # the random indels of single reads, each against the other reads there
        assert fields["het_indel_sites"] >= 3 and fields["insertion_sites"] >= 3 and fields["deletion_sites"] >= 3
    if args == ["--min-gq", "0"]:  # the two planted indels, under every read: a deletion of two bases and an insertion of three
        at = {(x[0], int(x[1]), len(x[3]) > len(x[4])): x for x in (y.split("\t") for y in want.decode().splitlines() if "\tINDEL;" in y)}
        deletion, insertion = at[("chrA", DEL_AT, True)], at[("chrA", 3000, False)]
        assert len(deletion[3]) == 3 and len(deletion[4]) == 1 and deletion[3][0] == deletion[4] and deletion[9][:4] in ("1/1:", "0/1:")
        assert len(insertion[3]) == 1 and len(insertion[4]) == 4 and insertion[4][0] == insertion[3] and insertion[9][:4] in ("1/1:", "0/1:")
        # stretches that begin at the deletion (the base in front lies in the stretch before), that end inside it (REF reaches
        # into the next) and that end with the insertion's position: the reference bases beyond a stretch are fetched
        for stretch in (DEL_AT, DEL_AT + 1, 3000, 997):
            q = run(["indels", d / "ref.fa", d / "reads.fq", "-q", "--keep-duplicates", "--vcf", "-"] + args, env={"DCN_CLI_STRETCH_BASES": str(stretch)})
            assert q.stdout == want, stretch


def test_the_relations_to_markdup(data):  # noqa: F811
    """one input through both modes: -o, --variants, --pileup, --sites and --duplicates byte for byte, and the VCF without its
    INDEL lines and the three header lines"""
    d, genomes, truths, reads, quals = data
    outs = ["-o", "--variants", "--pileup", "--sites", "--duplicates", "--vcf"]
    for tag, extra in (("plain", []), ("other", ["--both-ends", "--fill-ref", "--min-baseq", "25", "--ploidy", "1", "--all-positions"])):
        got = {}
        for sub in ("markdup", "indels"):
            files = [d / ("%s_%s_%s" % (tag, sub, o.strip("-") or "fa")) for o in outs]
            args = [sub, d / "ref.fa", d / "reads.fq", "-q", "-s", d / ("%s_%s.json" % (tag, sub))] + extra
            for o, f in zip(outs, files):
                args += [o, f]
            run(args, env=SMALL if sub == "indels" else None)
            got[sub] = [f.read_bytes() for f in files]
        assert got["indels"][:5] == got["markdup"][:5] and all(len(x) > 30 for x in got["markdup"])
        lines = got["indels"][5].decode().splitlines(keepends=True)
        extra_header = [x for x in lines if x.startswith(("##INFO=<ID=INDEL,", "##INFO=<ID=IDV,", "##INFO=<ID=IEV,"))]
        indel_lines = [x for x in lines if not x.startswith("#") and x.split("\t")[7].startswith("INDEL;")]
        assert [x.rstrip("\n") for x in extra_header] == DW.VCF_INDEL_HEADER and len(indel_lines) >= 1
        assert "".join(x for x in lines if x not in extra_header and x not in indel_lines).encode() == got["markdup"][5]
        # an older mode does not depend on DCN_CLI_STRETCH_BASES either: markdup in stretches of 997 positions
        files = [d / ("%s_stretch_%s" % (tag, o.strip("-") or "fa")) for o in outs]
        args = ["markdup", d / "ref.fa", d / "reads.fq", "-q"] + extra
        for o, f in zip(outs, files):
            args += [o, f]
        run(args, env={"DCN_CLI_STRETCH_BASES": "997"})
        assert [f.read_bytes() for f in files] == got["markdup"]
        a, b = (json.load(open(d / ("%s_%s.json" % (tag, sub)))) for sub in ("markdup", "indels"))
        assert {k: b[k] for k in a if k != "time"} == {k: a[k] for k in a if k != "time"}  # the summary only gains fields
        assert b["indel_sites"] == len(indel_lines) and set(b) - set(a) == {"indel_qual", "min_indel_count", "deletion_events", "deleted_bases", "indel_sites",
                                                                              "insertion_sites", "deletion_sites", "het_indel_sites", "hom_indel_sites"}


# ---- a record shorter than the reads: indels at and next to its first and last base ---------------------------------------
SHORT_NAMES = ("tiny", "chrA")
SHORT_ARGS = ["--end-bonus", "60", "--min-depth", "1", "--min-gq", "0", "--min-qual", "0"]  # (the bonus pays for an overhang of 5 bases as an I run)


@pytest.fixture(scope="module")
def short(tmp_path_factory):
    """A record of 100 bases in front of one of 2,000; ten copies each, on alternating strands, of reads that overhang its
    start (105 bases) and its end, that lack its first three bases behind three foreign ones, that lack bases 2 - 3 and 96 - 97,
    that carry two bases behind base 0, and of the record itself."""
    d = tmp_path_factory.mktemp("indels_short")
    rng = np.random.default_rng(1921)
    tiny, long_ = random_reads(rng, 1, 100, 100)[0], random_reads(rng, 1, 2000, 2000)[0]
    genomes = [tiny, long_]
    with open(d / "ref.fa", "wb") as f:
        for name, g in zip(SHORT_NAMES, genomes):
            f.write(b">" + name.encode() + b"\n" + g + b"\n")
    x, y, z = other(tiny[:1]), other(tiny[-1:]), other(other(tiny[:1]) if other(tiny[:1]) != tiny[1:2] else tiny[:1])
    kinds = [x * 5 + tiny, tiny + y * 4, other(tiny[2:3]) * 3 + tiny[3:], tiny[:2] + tiny[4:], tiny[:1] + z * 2 + tiny[1:], tiny[:96] + tiny[98:], tiny,
             long_[500:700]]
    reads, quals = [], []
    for k, s in enumerate(kinds):
        for q in range(10):
            reads.append(revcomp(s) if q % 2 else s)
            quals.append(b"?" * len(s))
    with open(d / "reads.fq", "wb") as f:
        for i, (r, q) in enumerate(zip(reads, quals)):
            f.write(b"@read%d\n" % i + r + b"\n+\n" + q + b"\n")
    return d, genomes, reads, quals, len(kinds)


def short_model(paf, genomes, reads, quals, min_base_qual=20):
    """tests/test_gpu_call_cli.py's model over SHORT_NAMES, with the deletion events beside: extend's verified lines of mapq >= 1
    and rank 0 -> (counts, sums, insertions, deletions, {read number: cg})"""
    counts, sums, ins, dels, cigars = PW.new_counts(genomes), QW.new_sums(genomes), IW.new_ledger(genomes), DW.new_ledger(genomes), {}
    for line in paf.decode().splitlines():
        c = line.split("\t")
        tags = dict(t.split(":", 2)[::2] for t in c[12:])
        if int(c[11]) < 1 or tags["rk"] != "0" or tags["ve"] != "1":
            continue
        n, rev, R, a, b = int(c[0][4:]), c[4] == "-", SHORT_NAMES.index(c[5]), int(c[7]), int(c[8])
        row = dict(read_start=int(c[2]), read_end=int(c[3]), reverse=int(rev))
        S = reads[n][row["read_start"]:row["read_end"]]
        S = revcomp(S) if rev else S
        runs = AW.align_pair(S, genomes[R][a:b])[1]
        assert AW.cigar_text(runs) == tags["cg"]
        cigars[n] = tags["cg"]
        if a == b:
            continue
        q = QW.qualities_of_S(quals[n], row, 33)
        PW.add_runs(counts[R], QW.masked(S, q, min_base_qual), a, rev, runs)
        QW.add_sums(sums[R], S, q, a, runs, min_base_qual)
        ins[R] += IW.events_of_runs(S, a, rev, runs)
        dels[R] += DW.deletion_events_of_runs(a, int(rev), runs)
    return counts, sums, ins, dels, cigars


@pytest.mark.parametrize("indel_qual", [20, 40])
def test_a_record_shorter_than_the_reads(short, indel_qual):
    """The VCF against the model, in one stretch, in stretches of 64 positions and of one, and in small batches.  What a run
    of the tool reaches at the ends of a record, and what it does not:
      a read that overhangs the record's start is, under an end bonus that pays for it, an I run in front of base 0: the line
        with ALT = bases + ref[0] at POS 1; one that overhangs its end an I run behind the last base (at --indel-qual 40, where
        ten reads of seventy make a site); deletions two bases from the end take their REF from the record's last bases;
      a read that lacks the record's first bases, with or without foreign bases in their place, does NOT become a D run at
        position 0: an extension grows a row outwards from its anchors and ends where the score is best, and record bases
        without read bases beside them only cost, so the row begins behind them or substitutes (the CIGARs below).  No CIGAR
        of the tool's begins or ends with a D run, so its line for a deletion at position 0 (REF = ref[0 .. len], ALT =
        ref[len]) and its error for a deletion of a whole record stay without a run of the tool; the library reaches such a
        site with rows written by hand (tests/test_gpu_indels_seams.py), and tests/test_indels_abi.py has the line's text."""
    d, genomes, reads, quals, n_kinds = short
    tiny = VW.fetched_text(genomes[0]).decode()
    paf = run(["extend", d / "ref.fa", d / "reads.fq", "-q", "-o", "-", "--end-bonus", "60"]).stdout
    counts, sums, ins, dels, cigars = short_model(paf, genomes, reads, quals)
    assert len(cigars) == len(reads)  # every read is placed, verified and counted
    per_kind = [cigars[10 * k] for k in range(n_kinds)]
    assert all(cigars[10 * k + q] == per_kind[k] for k in range(n_kinds) for q in range(10))  # both strands alike
    assert per_kind[0] == "5I100=" and per_kind[1] == "100=4I" and per_kind[6] == "100="
    assert "D" not in per_kind[2] and "D" not in per_kind[3] and per_kind[5].count("D") >= 1  # the first bases: no D run; bases 96 - 97: D runs
    assert not any(re.match(r"^\d+D", cg) or cg.endswith("D") for cg in cigars.values())
    shared = dict(min_depth=1, min_gq=0, min_qual=0)
    snvs = [GW.genotype_range(counts[R], sums[R], g, **dict(GW.DEFAULTS, **shared))[2] for R, g in enumerate(genomes)]
    indels = [DW.sites_range(counts[R], ins[R], dels[R], 0, len(g), indel_centi=100 * indel_qual, **shared) for R, g in enumerate(genomes)]
    want = DW.vcf_text(version(), SHORT_NAMES, genomes, snvs, indels).encode()
    lines = [x.split("\t") for x in want.decode().splitlines() if "\tINDEL;" in x]
    x = reads[0][:1].decode()
    assert ["tiny", "1", ".", tiny[0], x * 5 + tiny[0]] in [y[:5] for y in lines]  # the front insertion at position 0
    if indel_qual == 40:
        y = reads[10][-1:].decode()
        assert ["tiny", "100", ".", tiny[99], tiny[99] + y * 4] in [z[:5] for z in lines]  # behind the last base
        assert any(z[0] == "tiny" and len(z[3]) > len(z[4]) and int(z[1]) + len(z[3]) - 1 >= 97 for z in lines)  # a deletion at the end
    args = ["indels", d / "ref.fa", d / "reads.fq", "-q", "--keep-duplicates", "--vcf", "-", "--indel-qual", str(indel_qual)] + SHORT_ARGS
    for env in (None, {"DCN_CLI_STRETCH_BASES": "64"}, {"DCN_CLI_STRETCH_BASES": "1"}, {"DCN_CLI_ALIGN_BATCH_BASES": "700"}):
        assert run(args, env=env).stdout == want, env
