"""`deacon-hip markdup` end to end on tests/test_gpu_call_cli.py's reference and 240 of its reads, some of them repeated
exactly (one before its original, one three times), one repeated with the first bases of the read replaced so that the
extension soft-clips them, on either strand.  The placements are those `deacon-hip extend` prints for the same input; the
dict model of tests/_duplicates_worker.py marks the rows that --min-mapq and the rank leave.  `markdup` must equal `genotype`
run on the input with the model's duplicates deleted, byte for byte, in -o, --variants, --vcf, --pileup and --sites;
`markdup --keep-duplicates` must equal `genotype` on the whole input; --duplicates and the summary's new fields are exact; so
is everything with small batches and with --both-ends."""
import json

import pytest

import _duplicates_worker as DW
from test_gpu_call_cli import data  # noqa: F401 (a fixture)
from test_gpu_consensus_cli import NAMES, other
from test_gpu_pileup_cli import run

pytestmark = pytest.mark.gpu

OUTS = ["-o", "--variants", "--vcf", "--pileup", "--sites"]


def plain(i):
    """reads of the fixture that are neither mutated nor random"""
    return i % 5 != 1 and i % 19 != 4


def junk_front(read, n=9):
    """the first n bases as given replaced by bases they are not: the 5' end of the read, whichever strand it lies on"""
    return b"".join(other(read[j:j + 1]) for j in range(n)) + read[n:]


@pytest.fixture(scope="module")
def sample(data):  # noqa: F811
    d, genomes, truths, reads, quals = data
    fwd = next(i for i in range(20, 240) if plain(i) and i % 2 == 0 and len(reads[i]) > 150)
    rev = next(i for i in range(40, 240) if plain(i) and i % 2 == 1 and len(reads[i]) > 150)
    recs = [("orig%d" % i, reads[i], quals[i]) for i in range(240)]
    late = ("orig300", reads[300], quals[300])
    recs.insert(5, ("early300", reads[300], quals[300]))  # a copy in front of its original: the original is the duplicate
    recs.insert(100, ("copy3", reads[3], quals[3]))
    recs.insert(150, ("copy10a", reads[10], quals[10]))
    recs += [late, ("copy10b", reads[10], quals[10]), ("copy10c", reads[10], quals[10][::-1]), ("copy77", reads[77], quals[77]),
             ("clipfwd", junk_front(reads[fwd]), quals[fwd]), ("cliprev", junk_front(reads[rev]), quals[rev]), ("copy239", reads[239], quals[239])]
    with open(d / "dups.fq", "wb") as f:
        for name, r, q in recs:
            f.write(b"@" + name.encode() + b" words\n" + r + b"\n+\n" + q + b"\n")
    paf = run(["extend", d / "ref.fa", d / "dups.fq", "-q", "-o", "-"]).stdout.decode()
    rows = {name: [] for name, _, _ in recs}
    for line in paf.splitlines():  # the rows that --min-mapq 1 and rank 0 leave, verified or not
        c = line.split("\t")
        tags = dict(t.split(":", 2)[::2] for t in c[12:])
        if int(c[11]) >= 1 and tags["rk"] == "0":
            rows[c[0]].append((NAMES.index(c[5]), int(c[4] == "-"), int(c[2]), int(c[3]), int(c[7]), int(c[8])))
    return d, recs, rows, (fwd, rev)


def expected(d, recs, rows, both_ends, tag):
    """-> (dup flags, the --duplicates TSV, the summary's fields, the path of the input without the duplicates)"""
    model = DW.Model()
    lengths, reads_rows = [len(r) for _, r, _ in recs], [rows[name] for name, _, _ in recs]
    dup, first = model.mark(lengths, reads_rows, both_ends=both_ends)
    tsv = "read\tordinal\tfirst\trecord\tstrand\tpos5\n"
    for u, (name, r, _) in enumerate(recs):
        if dup[u]:
            end = DW.read_end_of(reads_rows[u], len(r), False)
            tsv += "%s\t%d\t%d\t%s\t%s\t%d\n" % (name, u, first[u], NAMES[end[0]], "-" if end[2] else "+", end[1])
    seen, keyed, keys = model.info()
    fields = dict(duplicates_both_ends=both_ends, reads_keyed=keyed, duplicate_reads=sum(dup), distinct_fragments=keys)
    path = d / ("dedup_%s.fq" % tag)
    with open(path, "wb") as f:
        for u, (name, r, q) in enumerate(recs):
            if not dup[u]:
                f.write(b"@" + name.encode() + b" words\n" + r + b"\n+\n" + q + b"\n")
    return dup, tsv, fields, path


def outputs(d, sub, reads, tag, extra=(), env=None):
    files = [d / ("%s_%s%s" % (tag, sub, o.strip("-") or "fa")) for o in OUTS]
    args = [sub, d / "ref.fa", reads, "-q", "-s", d / ("%s_%s.json" % (tag, sub))]
    for o, f in zip(OUTS, files):
        args += [o, f]
    run(args + list(extra), env=env)
    return [f.read_bytes() for f in files], json.load(open(d / ("%s_%s.json" % (tag, sub))))


def test_the_model_alone_finds_what_was_planted(sample):
    d, recs, rows, (fwd, rev) = sample
    names = [name for name, _, _ in recs]
    dup, _, fields, _ = expected(d, recs, rows, False, "alone")
    flagged = {names[u] for u, x in enumerate(dup) if x}
    assert {"orig300", "copy3", "copy10a", "copy10b", "copy10c", "copy77", "copy239", "clipfwd", "cliprev"} <= flagged and "early300" not in flagged
    # the clipped copies are clipped: their first rows begin behind the read's start, and their originals' do not
    assert rows["clipfwd"][0][2] >= 5 and rows["orig%d" % fwd][0][2] == 0 and rows["cliprev"][0][2] >= 5 and rows["orig%d" % rev][0][2] == 0
    assert rows["clipfwd"][0][1] == 0 and rows["cliprev"][0][1] == 1
    assert fields["duplicate_reads"] == len(flagged) < 20 and fields["reads_keyed"] > 200
    assert any(not r for r in rows.values())  # a read without a selected row: no key


@pytest.mark.parametrize("both_ends", [False, True], ids=["pos5", "both_ends"])
def test_markdup_equals_genotype_without_the_models_duplicates(sample, both_ends):
    d, recs, rows, _ = sample
    tag = "be" if both_ends else "p5"
    dup, tsv, fields, dedup = expected(d, recs, rows, both_ends, tag)
    extra = ["--both-ends"] if both_ends else []
    want, _ = outputs(d, "genotype", dedup, tag)
    got, summary = outputs(d, "markdup", d / "dups.fq", tag, ["--duplicates", d / (tag + ".tsv")] + extra)
    for o, a, b in zip(OUTS, got, want):
        assert a == b and len(a) > 100, o
    assert (d / (tag + ".tsv")).read_text() == tsv
    assert {k: summary[k] for k in fields} == fields and summary["keep_duplicates"] is False and summary["reads"] == len(recs)
    whole, _ = outputs(d, "genotype", d / "dups.fq", tag + "_whole")
    assert whole[3] != want[3]  # the duplicates do add to the pile-up when nobody leaves them out
    # several batches: the same files
    small, summary_small = outputs(d, "markdup", d / "dups.fq", tag + "_small", ["--duplicates", d / (tag + "_small.tsv")] + extra,
                                   env={"DCN_CLI_ALIGN_BATCH_BASES": "9000"})
    assert small == got and (d / (tag + "_small.tsv")).read_text() == tsv and {k: summary_small[k] for k in fields} == fields


def test_keep_duplicates_equals_genotype_on_the_whole_input(sample):
    d, recs, rows, _ = sample
    dup, tsv, fields, _ = expected(d, recs, rows, False, "keep")
    want, want_summary = outputs(d, "genotype", d / "dups.fq", "keep")
    got, summary = outputs(d, "markdup", d / "dups.fq", "keep", ["--keep-duplicates", "--duplicates", d / "keep.tsv"])
    assert got == want and (d / "keep.tsv").read_text() == tsv
    assert {k: summary[k] for k in fields} == fields and summary["keep_duplicates"] is True
    for k in ("rows_selected", "rows_added", "positions_covered", "vcf_sites", "genotyped_positions"):
        assert summary[k] == want_summary[k], k
    # --duplicates alone is an output
    run(["markdup", d / "ref.fa", d / "dups.fq", "-q", "--duplicates", d / "only.tsv"])
    assert (d / "only.tsv").read_text() == tsv
