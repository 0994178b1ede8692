"""`deacon-hip genotype` end to end on tests/test_gpu_call_cli.py's reference, reads and qualities.  The placements are those
`deacon-hip extend` prints for the same arguments; the model of tests/_quality_worker.py piles those lines up with the reads'
quality lines, the model of tests/_genotype_worker.py genotypes the counts and sums, and the VCF (header and every line) and
the summary's new fields are compared with it: --ploidy 1, other thresholds, --sample, small batches, .vcf.gz, stdin, --vcf -.
-o, --variants, --pileup and --sites are `deacon-hip call`'s files for the same arguments, byte for byte.  A planted site
that one read in five does not show appears as 0/1; one that only quality-5 bases support is absent at the default --min-baseq
and present at --min-baseq 0; the planted indels are in --variants and not in the VCF.  Every comparison is exact."""
import gzip
import json
import subprocess

import pytest

import _genotype_worker as GW
from test_gpu_call_cli import LOW_AT, MIXED_AT, data, model  # noqa: F401 (data is a fixture)
from test_gpu_consensus_cli import DEL_AT, NAMES
from test_gpu_pileup_cli import CLI, run

pytestmark = pytest.mark.gpu


def version():
    return subprocess.run([CLI, "--version"], capture_output=True, text=True, timeout=60).stdout.split()[1]


def expected(counts, sums, genomes, sample="sample", **params):
    """-> (the VCF's text, the summary's new fields)"""
    prm = dict(GW.DEFAULTS, **params)
    per_record, called = [], 0
    for R, g in enumerate(genomes):
        gt, gq, sites = GW.genotype_range(counts[R], sums[R], g, **prm)
        per_record.append(sites)
        called += int((gt != GW.NONE).sum())
    flat = [s for sites in per_record for s in sites]
    het = sum(1 for s in flat if len(set(GW.genotypes(prm["ploidy"])[s[4]])) == 2)
    fields = dict(ploidy=prm["ploidy"], min_gq=prm["min_gq"], min_qual=prm["min_qual"], genotyped_positions=called, vcf_sites=len(flat), het_sites=het,
                  hom_alt_sites=len(flat) - het)
    return GW.vcf_text(version(), NAMES, genomes, per_record, prm["ploidy"], sample).encode(), fields


@pytest.fixture(scope="module")
def piled(data):  # noqa: F811
    d, genomes, truths, reads, quals = data
    paf = run(["extend", d / "ref.fa", d / "reads.fq", "-q", "-o", "-"]).stdout
    counts, sums, ledger, added = model(paf, genomes, reads, quals)
    assert added > 300
    return paf, counts, sums


def test_vcf_and_summary_against_the_model(data, piled):  # noqa: F811
    d, genomes, truths, reads, quals = data
    paf, counts, sums = piled
    want, fields = expected(counts, sums, genomes)
    lines = want.decode().splitlines()
    body = [x.split("\t") for x in lines if not x.startswith("#")]
    # the model alone: what was planted is there, and the indels are not
    assert fields["vcf_sites"] == len(body) >= 3 and fields["het_sites"] >= 1 and fields["hom_alt_sites"] >= 2 and fields["genotyped_positions"] > 5000
    at = {(x[0], int(x[1])): x for x in body}
    assert at[("chrA", 1001)][9].startswith("1/1:") and at[("chrB", 501)][9].startswith("1/1:")
    assert at[("chrB", MIXED_AT + 1)][9].startswith("0/1:")  # one read in five shows the reference's base
    assert ("chrA", LOW_AT + 1) not in at  # only quality-5 bases support it
    assert not any((("chrA", p + 1) in at) for p in (DEL_AT, DEL_AT + 1, 2999, 3000))
    assert all(len(x[3]) == 1 and all(len(y) == 1 for y in x[4].split(",")) for x in body)  # SNVs only
    p = run(["genotype", d / "ref.fa", d / "reads.fq", "-q", "--vcf", d / "g.vcf", "-s", d / "g.json"])
    assert (d / "g.vcf").read_bytes() == want and p.stdout == b""
    s = json.load(open(d / "g.json"))
    assert {k: s[k] for k in fields} == fields
    assert run(["genotype", d / "ref.fa", d / "reads.fq", "-q", "--vcf", "-"]).stdout == want
    # small batches, .gz, stdin
    run(["genotype", d / "ref.fa", d / "reads.fq", "-q", "--vcf", d / "small.vcf"], env={"DCN_CLI_ALIGN_BATCH_BASES": "20000"})
    assert (d / "small.vcf").read_bytes() == want
    run(["genotype", d / "ref.fa", d / "reads.fq.gz", "-q", "--vcf", d / "g.vcf.gz"])
    assert gzip.decompress((d / "g.vcf.gz").read_bytes()) == want and (d / "g.vcf.gz").read_bytes()[:2] == b"\x1f\x8b"
    with open(d / "reads.fq", "rb") as f:
        assert run(["genotype", d / "ref.fa", "-q", "--vcf", "-"], stdin=f).stdout == want


@pytest.mark.parametrize("args,params", [(["--ploidy", "1"], dict(ploidy=1)),
                                         (["--min-depth", "8", "--min-gq", "60", "--min-qual", "150"], dict(min_depth=8, min_gq=60, min_qual=150)),
                                         (["--min-depth", "0", "--min-gq", "0", "--min-qual", "0", "--sample", "NA 1"], dict(min_depth=0, min_gq=0, min_qual=0))],
                         ids=["ploidy1", "strict", "loose"])
def test_other_settings_against_the_model(data, piled, args, params):  # noqa: F811
    d, genomes, truths, reads, quals = data
    paf, counts, sums = piled
    want, fields = expected(counts, sums, genomes, sample="NA 1" if "--sample" in args else "sample", **params)
    p = run(["genotype", d / "ref.fa", d / "reads.fq", "-q", "--vcf", "-", "-s", d / "o.json"] + args)
    assert p.stdout == want
    s = json.load(open(d / "o.json"))
    assert {k: s[k] for k in fields} == fields and s["min_depth"] == params.get("min_depth", 3)


def test_the_other_outputs_are_calls(data):  # noqa: F811
    d, genomes, truths, reads, quals = data
    outs = ["--variants", "v.tsv", "--pileup", "pile.tsv", "--sites", "sites.tsv"]
    for extra in ([], ["--fill-ref", "--min-baseq", "25", "--min-frac", "700", "--all-positions"]):
        got = {}
        for sub in ("call", "genotype"):
            files = [str(d / (sub + "_" + x)) if not x.startswith("--") else x for x in outs]
            p = run([sub, d / "ref.fa", d / "reads.fq", "-q", "-o", "-"] + files + extra + (["--vcf", d / "unused.vcf", "--min-gq", "7"] if sub == "genotype" else []))
            got[sub] = [p.stdout] + [(d / (sub + "_" + x)).read_bytes() for x in outs[1::2]]
        assert got["call"] == got["genotype"] and all(len(x) > 100 for x in got["call"])


def test_a_site_of_low_quality_bases_only(data, piled):  # noqa: F811
    d, genomes, truths, reads, quals = data
    paf, counts, sums = piled
    loose = run(["genotype", d / "ref.fa", d / "reads.fq", "-q", "--vcf", "-", "--min-baseq", "0", "--variants", d / "lv.tsv"]).stdout
    counts0, sums0, _, _ = model(paf, genomes, reads, quals, min_base_qual=0)
    assert loose == expected(counts0, sums0, genomes)[0]
    key = "chrA\t%d\t.\t" % (LOW_AT + 1)
    line = next(x for x in loose.decode().splitlines() if x.startswith(key)).split("\t")
    assert line[9].startswith("1/1:") and int(line[9].split(":")[2]) >= 3
    strict = run(["genotype", d / "ref.fa", d / "reads.fq", "-q", "--vcf", "-"]).stdout
    assert key not in strict.decode() and strict == expected(counts, sums, genomes)[0]
    variants = (d / "lv.tsv").read_text()
    assert "\nchrA\t%d\tDEL\t" % DEL_AT in variants and "\nchrA\t2999\tINS\t" in variants  # the indels stay in --variants


def test_a_fasta_record_behind_fastq_ones_is_refused(data, tmp_path):  # noqa: F811
    d, genomes, truths, reads, quals = data
    mixed = tmp_path / "mixed.fq"
    mixed.write_bytes(b"@first\n" + reads[0] + b"\n+\n" + quals[0] + b"\n>second words\n" + reads[1] + b"\n")
    p = subprocess.run([CLI, "genotype", str(d / "ref.fa"), str(mixed), "-q", "--vcf", str(tmp_path / "x.vcf")], capture_output=True, text=True, timeout=300)
    assert (p.returncode, p.stdout) == (1, "")
    assert p.stderr == "Error: genotype needs base qualities, and record 'second' has none (FASTA): consensus takes reads without\n"
