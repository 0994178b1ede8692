"""`deacon-hip place` end to end against the model of tests/_place_worker.py: every line of the table, the summary's
counts, many batches and a record that re-creates the context, a restricted key set through -x, .gz input and stdin."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import _place_worker as PW
from conftest import mutate, random_reads, revcomp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
K, WIN = 31, 15
NAMES = ("chrA", "chrB", "chrC")


def run(args, env=None, stdin=None):
    p = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})),
                       stdin=stdin)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p


@pytest.fixture(scope="module")
def data(tmp_path_factory, oracle):
    """a FASTA of three records (60 bases a line, a description behind each name), a FASTQ of 3,000 reads, the model over
    the reference's own keys and the table it expects"""
    d = tmp_path_factory.mktemp("place_cli")
    rng = np.random.default_rng(941)
    genomes = random_reads(rng, 3, 20_000, 20_000)
    with open(d / "ref.fa", "wb") as f:
        for name, g in zip(NAMES, genomes):
            f.write(b">" + name.encode() + b" synthetic record\n")
            f.write(b"\n".join(g[i:i + 60] for i in range(0, len(g), 60)) + b"\n")
    reads = []
    for i in range(3000):
        s = PW.cut(rng, genomes, 30, 300)
        if i % 5 == 1:
            s = mutate(rng, s, 0.04)
        if i % 7 == 2:
            s = random_reads(rng, 1, len(s), len(s))[0]
        reads.append(revcomp(s) if i % 2 else s)
    reads.append(genomes[1][1000:9000])  # a read of the workgroup path
    reads.append(genomes[0][300:1300] + revcomp(genomes[2][5000:5600]))
    with open(d / "reads.fq", "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@read%d some text\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n")
    keys = oracle.Index.build(genomes, k=K, w=WIN).keys()
    model = PW.AnchorModel(oracle, K, WIN, keys).add(genomes)
    return d, genomes, reads, model


def table(model, reads, **kw):
    lines = []
    for i, r in enumerate(reads):
        rec, rev, votes, n_anchors, n_pos, q0, q1, p0, p1 = model.place(r, **kw)
        placed = rec != PW.UNPLACED
        lines.append("\t".join(str(x) for x in (
            f"read{i}", len(r), q0, q1, ("-" if rev else "+") if placed else "*", NAMES[rec] if placed else "*",
            len(model.records[rec]) if placed else 0, p0, p1, votes, n_anchors, n_pos)))
    return "\n".join(lines) + "\n"


@pytest.mark.gpu
def test_table_summary_and_small_batches(data):
    d, genomes, reads, model = data
    run(["place", d / "ref.fa", d / "reads.fq", "-o", d / "out.tsv", "-s", d / "sum.json", "-q"])
    got = open(d / "out.tsv").read()
    want = table(model, reads)
    assert got == want
    s = json.load(open(d / "sum.json"))
    rows = [ln.split("\t") for ln in got.splitlines()]
    info = model.info()
    assert (s["records"], s["keys"], s["anchors"], s["repeats"]) == (3, info["keys"], info["anchors"], info["repeats"])
    assert s["reads"] == len(rows) == len(reads) and s["placed"] == sum(r[4] != "*" for r in rows) > 2000
    assert s["placed_by_strand"] == {"+": sum(r[4] == "+" for r in rows), "-": sum(r[4] == "-" for r in rows)}
    assert [(x["name"], x["length"], x["placed"]) for x in s["placed_by_record"]] == \
        [(n, 20_000, sum(r[5] == n for r in rows)) for n in NAMES]
    assert (s["k"], s["w"], s["band_bases"], s["min_votes"]) == (K, WIN, 256, 2)
    # batches of 5,000 bases in a context of 10,000: many batches, and every record re-creates the context
    run(["place", d / "ref.fa", d / "reads.fq", "-o", d / "small.tsv", "-q"], env={"DCN_CLI_PLACE_BATCH_BASES": "5000"})
    assert open(d / "small.tsv").read() == got


@pytest.mark.gpu
def test_options_gz_and_stdin(data):
    d, genomes, reads, model = data
    with gzip.open(d / "reads.fq.gz", "wb") as f:
        f.write(open(d / "reads.fq", "rb").read())
    p = run(["place", d / "ref.fa", d / "reads.fq.gz", "--band", 31, "-a", 3, "-p", 100, "-q"])
    want = table(model, reads, W=31, min_votes=3, prefix=100)
    assert p.stdout.decode() == want
    with open(d / "reads.fq", "rb") as f:
        p = run(["place", d / "ref.fa", "--band", 31, "-a", 3, "-p", 100, "-q"], stdin=f)
    assert p.stdout.decode() == want


@pytest.mark.gpu
def test_an_index_restricts_the_anchors(data, oracle, dcn):
    """-x: the reference's index minus the keys of chrB (dcn_index_diff), at w = 1 so that the file's k and w are seen to
    be used, not the defaults: chrB places nothing, and the lines equal the model's on that key set"""
    d, genomes, reads, _ = data
    full = dcn.Index.from_keys(oracle.Index.build(genomes, k=K, w=1).keys(), K, 1)
    host = dcn.Index.from_keys(oracle.Index.build([genomes[1]], k=K, w=1).keys(), K, 1)
    part = full.diff(host)
    part.write(str(d / "part.idx"))
    model = PW.AnchorModel(oracle, K, 1, part.keys()).add(genomes)
    for i in (full, host, part):
        i.close()
    some = reads[:600]
    with open(d / "some.fa", "wb") as f:
        for i, r in enumerate(some):
            f.write(b">read%d\n" % i + r + b"\n")
    p = run(["place", d / "ref.fa", d / "some.fa", "-x", d / "part.idx", "-s", d / "part.json"])
    got = p.stdout.decode()
    assert got == table(model, some)
    assert "\tchrB\t" not in got and "\tchrA\t" in got and "\tchrC\t" in got
    s = json.load(open(d / "part.json"))
    assert (s["k"], s["w"], s["keys"], s["anchors"]) == (K, 1, len(model.keys), model.info()["anchors"])
    assert b"Anchor map: 3 records" in p.stderr


def test_help_and_argument_errors():
    p = subprocess.run([CLI, "place", "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0
    for word in ("Usage: deacon-hip place [OPTIONS] <REF> [READS]", "-x, --index <INDEX>", "--band <N>", "-a, --min-votes <N>",
                 "-p, --prefix-length <N>", "-s, --summary <SUMMARY>", "-o, --output <OUTPUT>"):
        assert word in p.stdout, word
    top = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "place" in top.stdout + top.stderr
    for args, word in ((["place"], "<REF>"), (["place", "ref.fa", "--band", "0"], "--band"),
                       (["place", "ref.fa", "-a", "0"], "--min-votes"), (["place", "ref.fa", "-p", "-1"], "--prefix-length"),
                       (["place", "ref.fa", "-p", "12x"], "--prefix-length"), (["place", "a", "b", "c"], "one input")):
        p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and word in p.stderr, (args, p.stderr)
