"""`deacon-hip call` end to end on tests/test_gpu_consensus_cli.py's kind of reference with planted edits, with FASTQ reads of
random base qualities.  The placements are those `deacon-hip extend` prints for the same arguments (its PAF is pinned by
tests/test_gpu_extend_cli.py); the model of tests/_quality_worker.py piles those lines up with the reads' quality lines,
and the FASTA, the variants TSV with its two quality columns, --pileup with its four sums, --sites and the summary are
compared with it.  A planted substitution that only low-quality bases support is not called at the default --min-baseq and
is called at --min-baseq 0, where the FASTA is `consensus`'s.  Small batches, .gz, stdin, and the refusal of a FASTA record
behind FASTQ ones.  Every comparison is exact."""
import gzip
import json
import subprocess

import numpy as np
import pytest

import _align_worker as AW
import _insertion_worker as IW
import _pileup_worker as PW
import _quality_worker as QW
import _verify_worker as VW
from conftest import random_reads, revcomp
from test_gpu_consensus_cli import DEL_AT, NAMES, expected, other
from test_gpu_pileup_cli import CLI, run

pytestmark = pytest.mark.gpu

LOW_AT = 4000  # chrA: a substitution that every read shows with quality 5
MIXED_AT = 2000  # chrB: a substitution that four reads of five show
_ALIGNED = {}


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("call_cli")
    rng = np.random.default_rng(1835)  # (a seed whose record meets the assertion below)
    genomes = random_reads(rng, 1, 6000, 6000) + random_reads(rng, 1, 3000, 3000)
    a, b = genomes
    assert a[DEL_AT - 1] != a[DEL_AT + 1] and a[DEL_AT] != a[DEL_AT + 2]
    ins_a = other(a[2999:3000]) if other(a[2999:3000]) != a[3000:3001] else other(other(a[2999:3000]))
    # chrA: substitutions at 1000 and LOW_AT, two bases deleted at DEL_AT, three inserted behind base 2999 (one base longer in all)
    truth_a = a[:1000] + other(a[1000:1001]) + a[1001:DEL_AT] + a[DEL_AT + 2:3000] + ins_a * 3 + a[3000:LOW_AT] + other(a[LOW_AT:LOW_AT + 1]) + a[LOW_AT + 1:]
    minority_b = b[:500] + other(b[500:501]) + b[501:]
    truth_b = minority_b[:MIXED_AT] + other(b[MIXED_AT:MIXED_AT + 1]) + minority_b[MIXED_AT + 1:]
    truths = [truth_a, truth_b]
    low_in_truth = LOW_AT + 1
    assert truth_a[low_in_truth:low_in_truth + 1] == other(a[LOW_AT:LOW_AT + 1])
    with open(d / "ref.fa", "wb") as f:
        for name, g in zip(NAMES, genomes):
            f.write(b">" + name.encode() + b" synthetic record\n")
            f.write(b"\n".join(g[i:i + 60] for i in range(0, len(g), 60)) + b"\n")
    reads, quals = [], []
    for i in range(600):
        R, ln = int(rng.integers(0, 2)), int(rng.integers(120, 300))
        at = int(rng.integers(0, len(truths[R]) - ln))
        s = (minority_b if R == 1 and i % 5 == 2 else truths[R])[at:at + ln]
        q = rng.integers(14, 42, ln)
        covers = R == 0 and at <= low_in_truth < at + ln
        for planted in ((1000,) if R == 0 else (500, MIXED_AT)):  # the other planted substitutions: every read shows them with quality 30
            if at <= planted < at + ln:
                q[planted - at] = 30
        if covers:
            q[low_in_truth - at] = 5
        elif i % 5 == 1:
            s = VW.mutate_mixed(rng, s, 0.03)
            q = rng.integers(14, 42, len(s))
        elif i % 19 == 4:
            s = random_reads(rng, 1, ln, ln)[0]
        q = bytes((q + 33).astype(np.uint8))
        reads.append(revcomp(s) if i % 2 else s)
        quals.append(q[::-1] if i % 2 else q)
    with open(d / "reads.fq", "wb") as f:
        for i, (r, q) in enumerate(zip(reads, quals)):
            f.write(b"@read%d some text\n" % i + r + b"\n+\n" + q + b"\n")
    with gzip.open(d / "reads.fq.gz", "wb") as f:
        f.write((d / "reads.fq").read_bytes())
    return d, genomes, truths, reads, quals


def model(paf, genomes, reads, quals, min_base_qual=20, qual_offset=33):
    """extend's PAF lines piled up with the reads' qualities: the verified ones of mapq >= 1 and rank 0
    -> (counts, sums, ledger per record, rows added)"""
    counts, sums, ledger, added = PW.new_counts(genomes), QW.new_sums(genomes), IW.new_ledger(genomes), 0
    for line in paf.decode().splitlines():
        c = line.split("\t")
        tags = dict(t.split(":", 2)[::2] for t in c[12:])
        if int(c[11]) < 1 or tags["rk"] != "0" or tags["ve"] != "1":
            continue
        n, rev, R = int(c[0][4:]), c[4] == "-", NAMES.index(c[5])
        row = dict(read_start=int(c[2]), read_end=int(c[3]), reverse=int(rev))
        S = reads[n][row["read_start"]:row["read_end"]]
        S = revcomp(S) if rev else S
        q = QW.qualities_of_S(quals[n], row, qual_offset)
        if line not in _ALIGNED:
            _ALIGNED[line] = AW.align_pair(S, genomes[R][int(c[7]):int(c[8])])[1]
        runs = _ALIGNED[line]
        assert AW.cigar_text(runs) == tags["cg"]
        if int(c[8]) == int(c[7]):
            continue
        PW.add_runs(counts[R], QW.masked(S, q, min_base_qual), int(c[7]), rev, runs)
        QW.add_sums(sums[R], S, q, int(c[7]), runs, min_base_qual)
        ledger[R] += IW.events_of_runs(S, int(c[7]), rev, runs)
        added += 1
    return counts, sums, ledger, added


def with_quality_columns(variants, counts, sums, genomes):
    """consensus's variants TSV -> call's: ref_qual and alt_qual on SUB lines, "." on the others"""
    lines = variants.decode().splitlines()
    out = [lines[0] + "\tref_qual\talt_qual"]
    for line in lines[1:]:
        c = line.split("\t")
        R, p = NAMES.index(c[0]), int(c[1])
        out.append(line + "\t" + ("\t".join(QW.variant_quals(counts[R][p], sums[R][p], genomes[R][p], c[4])) if c[2] == "SUB" else ".\t."))
    return ("\n".join(out) + "\n").encode()


def pileup_text(counts, sums, genomes):
    out = ["record\tpos\tref\tA\tC\tG\tT\tN\tdel\tins\trev\tqA\tqC\tqG\tqT"]
    for name, g, k, s in zip(NAMES, genomes, counts, sums):
        ref = VW.fetched_text(g).decode()
        for p in range(len(g)):
            if k[p, :6].sum() > 0 or k[p, PW.INS] > 0:
                out.append("\t".join([name, str(p), ref[p]] + [str(int(x)) for x in k[p]] + [str(int(x)) for x in s[p]]))
    return ("\n".join(out) + "\n").encode()


def sites_text(counts, genomes, min_depth=3, min_permille=500):
    out = ["record\tpos\tref\tcall\tdepth\tflags"]
    for name, g, k in zip(NAMES, genomes, counts):
        ref = VW.fetched_text(g).decode()
        calls, pos, info = PW.call_range(k, g, 0, len(g), min_depth, min_permille)
        for p, x in zip(pos.tolist(), info.tolist()):
            out.append("\t".join([name, str(p), ref[p], chr(calls[p]), str(int(k[p, :6].sum())), str(x & 0xFF)]))
    return ("\n".join(out) + "\n").encode()


def test_outputs_against_the_model(data):
    d, genomes, truths, reads, quals = data
    paf = run(["extend", d / "ref.fa", d / "reads.fq", "-q", "-o", "-"]).stdout
    counts, sums, ledger, added = model(paf, genomes, reads, quals)
    assert added > 300
    want_fasta, plain_variants, want_n = expected(counts, ledger, genomes)
    want_variants = with_quality_columns(plain_variants, counts, sums, genomes)
    p = run(["call", d / "ref.fa", d / "reads.fq", "-q", "-o", "-", "--variants", d / "v.tsv", "-s", d / "c.json", "--pileup", d / "pile.tsv",
             "--sites", d / "sites.tsv"])
    assert p.stdout == want_fasta
    assert (d / "v.tsv").read_bytes() == want_variants
    assert (d / "pile.tsv").read_bytes() == pileup_text(counts, sums, genomes)
    assert (d / "sites.tsv").read_bytes() == sites_text(counts, genomes)
    s = json.load(open(d / "c.json"))
    assert {key: s[key] for key in want_n} == want_n and s["rows_added"] == added
    assert (s["min_base_qual"], s["qual_offset"]) == (20, 33)
    total = sum(x.sum(axis=0) for x in sums)
    assert s["quality_sums"] == {name: int(total[i]) for i, name in enumerate("ACGT")} and all(v > 20 * 1000 for v in s["quality_sums"].values())
    assert s["columns"]["N"] > 1000  # (about a fifth of the bases are below 20)
    # both kinds of quality column: a number, and "." (on a SUB line where no counted read shows the reference's base, and on every other line)
    rows = [x.split("\t") for x in want_variants.decode().splitlines()[1:]]
    subs = [x for x in rows if x[2] == "SUB"]
    assert len(subs) >= 3 and all(x[9] != "." for x in subs), subs[:12]  # (a SUB line always has counted bases that show alt)
    assert all(x[8:] == [".", "."] for x in rows if x[2] != "SUB") and {x[2] for x in rows} >= {"SUB", "DEL", "INS"}
    for line in ("chrA\t1000\tSUB\t", "chrA\t%d\tDEL\t" % DEL_AT, "chrA\t2999\tINS\t.\t", "chrB\t500\tSUB\t", "chrB\t%d\tSUB\t" % MIXED_AT):
        assert "\n" + line in want_variants.decode(), line
    mixed = next(x for x in rows if x[:3] == ["chrB", str(MIXED_AT), "SUB"])
    assert 14 <= int(mixed[8]) <= 41 and 14 <= int(mixed[9]) <= 41 and int(mixed[6]) < int(mixed[5])  # (both alleles were seen with good bases)
    # ("." for a reference base that no counted read shows is tests/test_pileup_qual_abi.py's and the next test's)
    # the same bytes in small batches, from .gz and from stdin
    small = run(["call", d / "ref.fa", d / "reads.fq", "-q", "-o", "-", "--variants", d / "s.tsv", "--pileup", d / "s_pile.tsv"],
                env={"DCN_CLI_ALIGN_BATCH_BASES": "20000"})
    assert small.stdout == want_fasta and (d / "s.tsv").read_bytes() == want_variants and (d / "s_pile.tsv").read_bytes() == (d / "pile.tsv").read_bytes()
    assert run(["call", d / "ref.fa", d / "reads.fq.gz", "-q", "-o", "-"]).stdout == want_fasta
    with open(d / "reads.fq", "rb") as f:
        assert run(["call", d / "ref.fa", "-q", "-o", "-"], stdin=f).stdout == want_fasta
    # another threshold and another offset, against the model again
    counts2, sums2, ledger2, _ = model(paf, genomes, reads, quals, min_base_qual=25, qual_offset=40)
    want2 = expected(counts2, ledger2, genomes, fill_ref=True)
    p = run(["call", d / "ref.fa", d / "reads.fq", "-q", "-o", "-", "--variants", d / "v2.tsv", "--min-baseq", "25", "--qual-offset", "40", "--fill-ref"])
    assert p.stdout == want2[0] and (d / "v2.tsv").read_bytes() == with_quality_columns(want2[1], counts2, sums2, genomes) and want2[0] != want_fasta


def test_a_substitution_of_low_quality_bases_only(data):
    """every read shows chrA's base LOW_AT substituted, each with quality 5: not called under the default --min-baseq (the
    bases count as N, which never wins), called with --min-baseq 0, where the FASTA is consensus's"""
    d, genomes, truths, reads, quals = data
    strict = run(["call", d / "ref.fa", d / "reads.fq", "-q", "-o", "-", "--variants", d / "strict.tsv", "--pileup", d / "strict_pile.tsv"])
    loose = run(["call", d / "ref.fa", d / "reads.fq", "-q", "-o", "-", "--variants", d / "loose.tsv", "--min-baseq", "0"])
    key = "\nchrA\t%d\tSUB\t" % LOW_AT
    assert key not in (d / "strict.tsv").read_text() and key in (d / "loose.tsv").read_text()
    line = next(x for x in (d / "loose.tsv").read_text().splitlines() if x.startswith(key[1:])).split("\t")
    assert line[4] == other(genomes[0][LOW_AT:LOW_AT + 1]).decode() and int(line[5]) >= 3 and line[6] == line[5] and line[8:] == [".", "5"]
    pile = next(x for x in (d / "strict_pile.tsv").read_text().splitlines() if x.startswith("chrA\t%d\t" % LOW_AT)).split("\t")
    assert pile[3:7] == ["0"] * 4 and int(pile[7]) == int(line[5]) and pile[11:] == ["0"] * 4  # all in N, no sums
    assert loose.stdout == run(["consensus", d / "ref.fa", d / "reads.fq", "-q", "-o", "-"]).stdout != strict.stdout
    # where the depth reaches, the loose consensus is the truth around the position
    seq = loose.stdout.decode().split(">chrA\n")[1].split("\n")[0]
    assert truths[0][LOW_AT + 1 - 12:LOW_AT + 1 + 12].decode() in seq


def test_a_fasta_record_behind_fastq_ones_is_refused(data, tmp_path):
    d, genomes, truths, reads, quals = data
    mixed = tmp_path / "mixed.fq"
    mixed.write_bytes(b"@first\n" + reads[0] + b"\n+\n" + quals[0] + b"\n>second words\n" + reads[1] + b"\n")
    p = subprocess.run([CLI, "call", str(d / "ref.fa"), str(mixed), "-q", "-o", "-"], capture_output=True, text=True, timeout=300)
    assert (p.returncode, p.stdout) == (1, "")
    assert p.stderr == "Error: call needs base qualities, and record 'second' has none (FASTA): consensus takes reads without\n"
