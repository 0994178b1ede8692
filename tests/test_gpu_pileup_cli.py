"""`deacon-hip pileup` end to end on the input of tests/test_gpu_align_cli.py: the placements are those `deacon-hip align`
prints for the same arguments (its PAF is pinned by that file), and both TSVs and the summary are compared with the model
of tests/_pileup_worker.py over those lines: --min-mapq, --all-ranks, --all-positions, --min-depth / --min-frac, small
batches under DCN_CLI_ALIGN_BATCH_BASES, .gz and stdin inputs.  Every comparison is exact."""
import json
import os
import subprocess

import numpy as np
import pytest

import _align_worker as AW
import _pileup_worker as PW
import _verify_worker as VW
from conftest import revcomp
from test_gpu_align_cli import NAMES, data  # noqa: F401  (the fixture: three 20 kbp records, 200 reads)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
COLUMN_NAMES = ("A", "C", "G", "T", "N", "del", "ins", "rev")


def run(args, env=None, stdin=None):
    p = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})),
                       stdin=stdin)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p


def model(paf, genomes, reads, min_mapq=1, all_ranks=False):
    """the pileup of align's PAF lines: the verified ones of at least min_mapq, rank 0 only unless all_ranks
    -> (counts per record, rows selected, rows added)"""
    counts = PW.new_counts(genomes)
    selected = added = 0
    for line in paf.decode().splitlines():
        c = line.split("\t")
        tags = dict(t.split(":", 2)[::2] for t in c[12:])
        if int(c[11]) < min_mapq or (not all_ranks and tags["rk"] != "0"):
            continue
        selected += 1
        if tags["ve"] != "1":
            continue
        S = reads[int(c[0][4:])][int(c[2]):int(c[3])]
        R = NAMES.index(c[5])
        d, runs = AW.align_pair(revcomp(S) if c[4] == "-" else S, genomes[R][int(c[7]):int(c[8])])
        assert AW.cigar_text(runs) == tags["cg"]
        PW.add_runs(counts[R], revcomp(S) if c[4] == "-" else S, int(c[7]), c[4] == "-", runs)
        added += 1
    return counts, selected, added


def pileup_text(counts, genomes, every=False):
    out = ["record\tpos\tref\tA\tC\tG\tT\tN\tdel\tins\trev"]
    for name, g, k in zip(NAMES, genomes, counts):
        ref = VW.fetched_text(g).decode()
        for p in range(len(g)):
            if every or k[p, :6].sum() > 0 or k[p, PW.INS] > 0:
                out.append("\t".join([name, str(p), ref[p]] + [str(int(x)) for x in k[p]]))
    return ("\n".join(out) + "\n").encode()


def sites_text(counts, genomes, min_depth=3, min_permille=500):
    out, n = ["record\tpos\tref\tcall\tdepth\tflags"], 0
    for name, g, k in zip(NAMES, genomes, counts):
        ref = VW.fetched_text(g).decode()
        calls, pos, info = PW.call_range(k, g, 0, len(g), min_depth, min_permille)
        for p, x in zip(pos.tolist(), info.tolist()):
            out.append("\t".join([name, str(p), ref[p], chr(calls[p]), str(int(k[p, :6].sum())), str(x & 0xFF)]))
            n += 1
    return ("\n".join(out) + "\n").encode(), n


def test_tsvs_and_summary_against_the_model(data):  # noqa: F811
    d, genomes, reads = data
    paf = run(["align", d / "ref.fa", d / "reads.fq", "-q"]).stdout
    counts, selected, added = model(paf, genomes, reads)
    assert added > 100 and selected > added
    p = run(["pileup", d / "ref.fa", d / "reads.fq", "-q", "--sites", d / "sites.tsv", "-s", d / "pileup.json", "--min-depth", "1"])
    assert p.stdout == pileup_text(counts, genomes)
    want_sites, n_sites = sites_text(counts, genomes, min_depth=1)
    assert (d / "sites.tsv").read_bytes() == want_sites and n_sites > 50
    s = json.load(open(d / "pileup.json"))
    total = sum(k.sum(axis=0) for k in counts)
    assert s["columns"] == {name: int(total[i]) for i, name in enumerate(COLUMN_NAMES)} and all(x > 0 for x in s["columns"].values())
    assert (s["rows_selected"], s["rows_added"], s["sites"]) == (selected, added, n_sites)
    assert s["positions_covered"] == sum(int((k[:, :6].sum(axis=1) > 0).sum()) for k in counts)
    assert (s["min_mapq"], s["all_ranks"], s["min_depth"], s["min_permille"]) == (1, False, 1, 500)
    # the same bytes in small batches, from .gz and from stdin
    small = run(["pileup", d / "ref.fa", d / "reads.fq", "-q"], env={"DCN_CLI_ALIGN_BATCH_BASES": "20000"})
    assert small.stdout == p.stdout
    assert run(["pileup", d / "ref.fa", d / "reads.fq.gz", "-q"]).stdout == p.stdout
    with open(d / "reads.fq", "rb") as f:
        assert run(["pileup", d / "ref.fa", "-q"], stdin=f).stdout == p.stdout
    # without -q the tool says what it added; -o takes the TSV
    loud = run(["pileup", d / "ref.fa", d / "reads.fq", "-o", d / "out.tsv"])
    assert f"Piled up {added} of ".encode() in loud.stderr and (d / "out.tsv").read_bytes() == p.stdout and loud.stdout == b""


def test_selection_and_all_positions(data):  # noqa: F811
    d, genomes, reads = data
    paf = run(["align", d / "ref.fa", d / "reads.fq", "-q"]).stdout
    base = model(paf, genomes, reads)
    for opts, kw in ((["--min-mapq", "0", "--all-ranks"], dict(min_mapq=0, all_ranks=True)), (["--min-mapq", "60"], dict(min_mapq=60)),
                     (["--all-ranks"], dict(all_ranks=True))):
        counts, selected, added = model(paf, genomes, reads, **kw)
        assert (selected, added) != base[1:] or not kw.get("all_ranks")  # (the chimeras have a second placement)
        p = run(["pileup", d / "ref.fa", d / "reads.fq", "-q", "-s", d / "sel.json", "--sites", d / "sel.tsv"] + opts)
        assert p.stdout == pileup_text(counts, genomes)
        s = json.load(open(d / "sel.json"))
        want_sites, n_sites = sites_text(counts, genomes)
        assert (s["rows_selected"], s["rows_added"], s["sites"]) == (selected, added, n_sites) and (d / "sel.tsv").read_bytes() == want_sites
    every = run(["pileup", d / "ref.fa", d / "reads.fq", "-q", "--all-positions", "--min-depth", "2", "--min-frac", "1000", "--sites", d / "strict.tsv"])
    assert every.stdout == pileup_text(base[0], genomes, every=True) and every.stdout.count(b"\n") == 60_001
    assert (d / "strict.tsv").read_bytes() == sites_text(base[0], genomes, 2, 1000)[0]


def test_min_mapq_on_a_repeat(tmp_path):
    """a reference whose second record repeats a stretch of the first with 3 % substitutions: reads from the stretch have
    rival votes, so their placements have qualities between 0 and 60 and --min-mapq decides which of them add"""
    from conftest import mutate, random_reads
    rng = np.random.default_rng(1541)
    a = random_reads(rng, 1, 6000, 6000)[0]
    genomes = [a, mutate(rng, a[1000:4000], 0.04), random_reads(rng, 1, 500, 500)[0]]
    with open(tmp_path / "ref.fa", "wb") as f:
        for name, g in zip(NAMES, genomes):
            f.write(b">" + name.encode() + b"\n" + g + b"\n")
    reads = []
    for i in range(120):
        R = i % 2
        at = int(rng.integers(1000, 3400)) - 1000 * R
        s = VW.mutate_mixed(rng, genomes[R][at:at + 600], 0.02 * (i % 3))
        reads.append(revcomp(s) if i % 4 == 3 else s)
    with open(tmp_path / "reads.fa", "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">read%d\n" % i + r + b"\n")
    paf = run(["align", tmp_path / "ref.fa", tmp_path / "reads.fa", "-q"]).stdout
    quals = sorted({int(line.split("\t")[11]) for line in paf.decode().splitlines()})
    assert len(quals) >= 4 and quals[-1] == 60, quals
    seen = set()
    for q in (0, 1, quals[len(quals) // 2], 60):
        counts, selected, added = model(paf, genomes, reads, min_mapq=q)
        p = run(["pileup", tmp_path / "ref.fa", tmp_path / "reads.fa", "-q", "--min-mapq", q, "-s", tmp_path / "q.json"])
        assert p.stdout == pileup_text(counts, genomes)
        s = json.load(open(tmp_path / "q.json"))
        assert (s["min_mapq"], s["rows_selected"], s["rows_added"]) == (q, selected, added)
        seen.add((selected, added))
    assert len(seen) >= 3, seen
