"""`deacon-hip consensus` end to end on a reference with planted edits: reads are cut from a truth that differs from the
reference by substitutions, a deletion and insertions.  The placements are those `deacon-hip extend` prints for the same
arguments (its PAF is pinned by tests/test_gpu_extend_cli.py); the model of tests/_insertion_worker.py piles those lines up,
and the FASTA, the variants TSV and the summary are compared with it: --fill-ref, --all-ranks, --min-mapq, small batches
under DCN_CLI_ALIGN_BATCH_BASES, .gz and stdin inputs.  Every comparison is exact."""
import gzip
import json

import numpy as np
import pytest

import _align_worker as AW
import _insertion_worker as IW
import _pileup_worker as PW
import _verify_worker as VW
from conftest import random_reads, revcomp
from test_gpu_pileup_cli import run

pytestmark = pytest.mark.gpu

NAMES = ("chrA", "chrB")
DEL_AT = 2010
_ALIGNED = {}  # PAF line -> the model's runs (every test here walks the same lines)


def other(base):
    return b"ACGT"[(b"ACGT".find(base.upper()) + 1) % 4:][:1]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("consensus_cli")
    rng = np.random.default_rng(1731)
    genomes = random_reads(rng, 1, 6000, 6000) + random_reads(rng, 1, 3000, 3000)
    a, b = genomes
    # the truth: chrA with a substitution at 1000, two bases deleted at DEL_AT and three inserted behind base 2999; chrB with a
    # substitution at 500 and two bases inserted behind base 1499.  No edit can move: the neighbours differ
    assert a[DEL_AT - 1] != a[DEL_AT + 1] and a[DEL_AT] != a[DEL_AT + 2]
    ins_a = other(a[2999:3000]) if other(a[2999:3000]) != a[3000:3001] else other(other(a[2999:3000]))
    truth_a = a[:1000] + other(a[1000:1001]) + a[1001:DEL_AT] + a[DEL_AT + 2:3000] + ins_a * 3 + a[3000:]
    ins_b = other(b[1499:1500]) if other(b[1499:1500]) != b[1500:1501] else other(other(b[1499:1500]))
    truth_b = b[:500] + other(b[500:501]) + b[501:1500] + ins_b * 2 + b[1500:]
    truths = [truth_a, truth_b]
    with open(d / "ref.fa", "wb") as f:
        for name, g in zip(NAMES, genomes):
            f.write(b">" + name.encode() + b" synthetic record\n")
            f.write(b"\n".join(g[i:i + 60] for i in range(0, len(g), 60)) + b"\n")
    reads = []
    for i in range(600):
        R, ln = int(rng.integers(0, 2)), int(rng.integers(120, 300))
        at = int(rng.integers(0, len(truths[R]) - ln))
        s = truths[R][at:at + ln]
        if i % 5 == 1:
            s = VW.mutate_mixed(rng, s, 0.03)
        if i % 17 == 3:
            s = s + revcomp(truths[1 - R][100:250])  # a chimera: a second placement
        if i % 19 == 4:
            s = random_reads(rng, 1, ln, ln)[0]
        reads.append(revcomp(s) if i % 2 else s)
    with open(d / "reads.fq", "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@read%d some text\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n")
    with gzip.open(d / "reads.fq.gz", "wb") as f:
        f.write((d / "reads.fq").read_bytes())
    return d, genomes, truths, reads


def model(paf, genomes, reads, min_mapq=1, all_ranks=False):
    """extend's PAF lines piled up: the verified ones of at least min_mapq, rank 0 only unless all_ranks
    -> (counts per record, ledger per record, rows added)"""
    counts, ledger, added = PW.new_counts(genomes), IW.new_ledger(genomes), 0
    for line in paf.decode().splitlines():
        c = line.split("\t")
        tags = dict(t.split(":", 2)[::2] for t in c[12:])
        if int(c[11]) < min_mapq or (not all_ranks and tags["rk"] != "0") or tags["ve"] != "1":
            continue
        S = reads[int(c[0][4:])][int(c[2]):int(c[3])]
        S = revcomp(S) if c[4] == "-" else S
        R = NAMES.index(c[5])
        if line not in _ALIGNED:
            _ALIGNED[line] = AW.align_pair(S, genomes[R][int(c[7]):int(c[8])])[1]
        runs = _ALIGNED[line]
        assert AW.cigar_text(runs) == tags["cg"]
        if int(c[8]) == int(c[7]):
            continue
        PW.add_runs(counts[R], S, int(c[7]), c[4] == "-", runs)
        ledger[R] += IW.events_of_runs(S, int(c[7]), c[4] == "-", runs)
        added += 1
    return counts, ledger, added


def expected(counts, ledger, genomes, min_depth=3, min_permille=500, fill_ref=False):
    """-> (the FASTA, the variants TSV, the summary's seven numbers)"""
    fasta, rows = [], ["record\tpos\ttype\tref\talt\tdepth\tcount\tevents"]
    n = dict(insertion_events=sum(len(x) for x in ledger), inserted_bases=sum(e[2] for x in ledger for e in x), insertion_alleles=0, substitutions=0,
             deleted_positions=0, consensus_bases=0, uncalled_positions=0)
    for name, g, k, led in zip(NAMES, genomes, counts, ledger):
        ref = VW.fetched_text(g).decode()
        seq = IW.consensus(k, led, g, 0, None, min_depth, min_permille, fill_ref)
        fasta.append(">" + name + "\n" + seq.decode() + "\n")
        n["consensus_bases"] += len(seq)
        called = {x[0]: x for x in IW.call_range(k, led, g, 0, None, min_depth, min_permille)}
        n["insertion_alleles"] += len(called)
        for p in range(len(g)):
            ch, _ = PW.call_position(k[p], g[p], min_depth, min_permille)
            depth = int(k[p, :6].sum())
            x = called.get(p)
            line = lambda kind, r, alt, count, events: rows.append("\t".join([name, str(p), kind, r, alt, str(depth), str(count), str(events)]))  # noqa: E731
            if x and x[1]:
                line("INS_FRONT", ".", x[3].decode(), x[4], x[5])
            if ch == "N":
                n["uncalled_positions"] += 1
            elif ch == "-":
                n["deleted_positions"] += 1
                line("DEL", ref[p], "-", int(k[p, PW.DEL]), 0)
            elif ch != ref[p]:
                n["substitutions"] += 1
                line("SUB", ref[p], ch, int(k[p, "ACGT".index(ch)]), 0)
            if x and not x[1]:
                line("INS", ".", x[3].decode(), x[4], x[5])
    return "".join(fasta).encode(), ("\n".join(rows) + "\n").encode(), n


def test_fasta_variants_and_summary_against_the_model(data):
    d, genomes, truths, reads = data
    paf = run(["extend", d / "ref.fa", d / "reads.fq", "-q", "-o", "-"]).stdout
    counts, ledger, added = model(paf, genomes, reads)
    assert added > 300
    want_fasta, want_variants, want_n = expected(counts, ledger, genomes)
    p = run(["consensus", d / "ref.fa", d / "reads.fq", "-q", "-o", "-", "--variants", d / "v.tsv", "-s", d / "c.json", "--pileup", d / "pile.tsv"])
    assert p.stdout == want_fasta and (d / "v.tsv").read_bytes() == want_variants
    s = json.load(open(d / "c.json"))
    assert {key: s[key] for key in want_n} == want_n and s["fill_ref"] is False and s["rows_added"] == added
    assert want_n["insertion_alleles"] >= 2 and want_n["substitutions"] >= 2 and want_n["deleted_positions"] >= 2 and want_n["insertion_events"] > 20
    text = want_variants.decode()
    for line in ("chrA\t1000\tSUB\t", "chrA\t%d\tDEL\t" % DEL_AT, "chrA\t%d\tDEL\t" % (DEL_AT + 1), "chrA\t2999\tINS\t.\t", "chrB\t1499\tINS\t.\t", "chrB\t500\tSUB\t"):
        assert "\n" + line in text, line
    # where the depth reaches, the consensus is the truth the reads were cut from
    seq = {name: want_fasta.decode().split(">" + name + "\n")[1].split("\n")[0] for name in NAMES}
    for name, truth, spots in (("chrA", truths[0], (1000, DEL_AT, 2999)), ("chrB", truths[1], (500, 1500))):
        for at in spots:  # (in the truth's coordinates: the substitution, the bases around the deletion, the inserted bases)
            assert truth[at - 12:at + 12].decode() in seq[name], (name, at)
    # the counters are extend's for the same arguments
    run(["extend", d / "ref.fa", d / "reads.fq", "-q", "--pileup", d / "pile2.tsv"])
    assert (d / "pile.tsv").read_bytes() == (d / "pile2.tsv").read_bytes()
    # --fill-ref, and thresholds
    filled = run(["consensus", d / "ref.fa", d / "reads.fq", "-q", "-o", d / "f.fa", "--fill-ref", "-s", d / "f.json"])
    want = expected(counts, ledger, genomes, fill_ref=True)
    assert filled.stdout == b"" and (d / "f.fa").read_bytes() == want[0] and b"N" not in want[0].split(b"\n")[1]
    assert json.load(open(d / "f.json"))["fill_ref"] is True and json.load(open(d / "f.json"))["consensus_bases"] == want[2]["consensus_bases"]
    loose = run(["consensus", d / "ref.fa", d / "reads.fq", "-q", "-o", "-", "--variants", d / "l.tsv", "--min-depth", "1", "--min-frac", "200"])
    want = expected(counts, ledger, genomes, min_depth=1, min_permille=200)
    assert loose.stdout == want[0] and (d / "l.tsv").read_bytes() == want[1] and want[1] != want_variants
    # the same bytes in small batches, from .gz and from stdin
    small = run(["consensus", d / "ref.fa", d / "reads.fq", "-q", "-o", "-", "--variants", d / "s.tsv"], env={"DCN_CLI_ALIGN_BATCH_BASES": "20000"})
    assert small.stdout == want_fasta and (d / "s.tsv").read_bytes() == want_variants
    assert run(["consensus", d / "ref.fa", d / "reads.fq.gz", "-q", "-o", "-"]).stdout == want_fasta
    with open(d / "reads.fq", "rb") as f:
        assert run(["consensus", d / "ref.fa", "-q", "-o", "-"], stdin=f).stdout == want_fasta
    # without -q the tool says what it wrote; without -o there is no FASTA
    loud = run(["consensus", d / "ref.fa", d / "reads.fq"])
    assert loud.stdout == b"" and ("Consensus of %d bases: %d substitutions" % (want_n["consensus_bases"], want_n["substitutions"])).encode() in loud.stderr


def test_selection(data):
    d, genomes, truths, reads = data
    paf = run(["extend", d / "ref.fa", d / "reads.fq", "-q", "-o", "-"]).stdout
    base = model(paf, genomes, reads)[2]
    seen = set()
    for opts, kw in ((["--min-mapq", "0", "--all-ranks"], dict(min_mapq=0, all_ranks=True)), (["--min-mapq", "60"], dict(min_mapq=60)),
                     (["--all-ranks"], dict(all_ranks=True))):
        counts, ledger, added = model(paf, genomes, reads, **kw)
        seen.add(added)
        want_fasta, want_variants, want_n = expected(counts, ledger, genomes)
        p = run(["consensus", d / "ref.fa", d / "reads.fq", "-q", "-o", "-", "--variants", d / "sel.tsv", "-s", d / "sel.json"] + opts)
        assert p.stdout == want_fasta and (d / "sel.tsv").read_bytes() == want_variants
        s = json.load(open(d / "sel.json"))
        assert s["rows_added"] == added and {key: s[key] for key in want_n} == want_n
    assert len(seen | {base}) >= 3  # (the options are not without effect on this input)
