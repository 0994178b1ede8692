"""`deacon-hip map` end to end against the model of tests/_place_split_worker.py: every PAF line and the summary's counts,
many batches, -x, .gz input, stdin and -N 1; and `deacon-hip place` on the same inputs against its own model, since the
two subcommands load the reference through one helper."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import _place_split_worker as SW
import _place_worker as PW
from conftest import mutate, random_reads, revcomp
from test_gpu_place_cli import table as place_table

pytestmark = pytest.mark.gpu

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
    """a FASTA of three records, a FASTQ of 1,200 reads (cuts, mutated cuts, random reads, chimeras of two and three
    parts, a part inside another's stretch, reads of the workgroup path) and the model over the reference's own keys"""
    d = tmp_path_factory.mktemp("map_cli")
    rng = np.random.default_rng(971)
    genomes = random_reads(rng, 3, 20_000, 20_000)
    with open(d / "ref.fa", "wb") as f:
        for name, g in zip(NAMES, genomes):
            f.write(b">" + name.encode() + b" synthetic record\n")
            f.write(b"\n".join(g[i:i + 60] for i in range(0, len(g), 60)) + b"\n")
    reads = []
    for i in range(1200):
        s = PW.cut(rng, genomes, 30, 300)
        if i % 5 == 1:
            s = mutate(rng, s, 0.04)
        if i % 7 == 2:
            s = random_reads(rng, 1, len(s), len(s))[0]
        if i % 4 == 3:
            s = s + revcomp(PW.cut(rng, genomes, 60, 200))
        if i % 12 == 5:
            s = PW.cut(rng, genomes, 60, 200) + s + PW.cut(rng, genomes, 60, 200)
        if i % 20 == 9:
            at = int(rng.integers(0, 19000))
            s = genomes[i % 3][at:at + 150] + s + genomes[i % 3][at + 150 + len(s):at + 300 + len(s)]
        reads.append(revcomp(s) if i % 2 else s)
    reads.append(genomes[1][1000:9000])  # reads of the workgroup path
    reads.append(genomes[0][300:1300] + revcomp(genomes[2][5000:5600]) + genomes[1][100:400])
    with open(d / "reads.fq", "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@read%d some text\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n")
    keys = oracle.Index.build(genomes, k=K, w=WIN).keys()
    model = PW.AnchorModel(oracle, K, WIN, keys).add(genomes)
    return d, genomes, reads, model


def paf(model, reads, **kw):
    """the lines `deacon-hip map` is to write"""
    k = model.k
    lines = []
    for i, r in enumerate(reads):
        for (rec, rev, votes, n_anchors, n_pos, q0, q1, p0, p1, rank, n_placed, rival, mapq) in SW.place_split(model, r, **kw)[0]:
            cols = [f"read{i}", len(r), q0, q1, "-" if rev else "+", NAMES[rec], len(model.records[rec]), p0, p1,
                    min(votes * k, q1 - q0), max(q1 - q0, p1 - p0), mapq,
                    f"cm:i:{votes}", f"rk:i:{rank}", f"np:i:{n_placed}", f"rv:i:{rival}", f"na:i:{n_anchors}", f"ns:i:{n_pos}"]
            lines.append("\t".join(str(c) for c in cols))
    return "".join(ln + "\n" for ln in lines)


def check_lines(text):
    """column 10 <= column 11, and both coordinate pairs within their sequence's length"""
    rows = [ln.split("\t") for ln in text.splitlines()]
    for c in rows:
        assert len(c) == 18 and int(c[9]) <= int(c[10])
        assert 0 <= int(c[2]) < int(c[3]) <= int(c[1]) and 0 <= int(c[7]) < int(c[8]) <= int(c[6])
        assert 0 <= int(c[11]) <= 60 and c[4] in "+-"
    return rows


def test_paf_summary_small_batches_and_place_unchanged(data):
    d, genomes, reads, model = data
    run(["map", d / "ref.fa", d / "reads.fq", "-o", d / "out.paf", "-s", d / "sum.json", "-q"])
    got = open(d / "out.paf").read()
    assert got == paf(model, reads)
    rows = check_lines(got)
    s = json.load(open(d / "sum.json"))
    info = model.info()
    per_read = {}
    for c in rows:
        per_read[c[0]] = per_read.get(c[0], 0) + 1
    assert (s["records"], s["keys"], s["anchors"], s["repeats"]) == (3, info["keys"], info["anchors"], info["repeats"])
    assert (s["k"], s["w"], s["band_bases"], s["min_votes"], s["prefix_length"], s["max_placements"]) == (K, WIN, 256, 2, 0, 4)
    assert s["reads"] == len(reads) and s["placed"] == len(per_read) > 900 and s["placements"] == len(rows)
    assert s["split_reads"] == sum(v >= 2 for v in per_read.values()) > 250
    assert s["mapq60"] == sum(c[11] == "60" for c in rows) > 900 and s["mapq0"] == sum(c[11] == "0" for c in rows) > 10
    assert [(x["name"], x["length"], x["placements"]) for x in s["placements_by_record"]] == \
        [(n, 20_000, sum(c[5] == n for c in rows)) for n in NAMES]
    # batches of 5,000 bases in a context of 10,000: many batches, and every record re-creates the context
    run(["map", d / "ref.fa", d / "reads.fq", "-o", d / "small.paf", "-q"], env={"DCN_CLI_MAP_BATCH_BASES": "5000"})
    assert open(d / "small.paf").read() == got
    # `place` on the same inputs, through the same loading of the reference: its table and its messages
    p = run(["place", d / "ref.fa", d / "reads.fq", "-s", d / "place.json"])
    assert p.stdout.decode() == place_table(model, reads)
    err = p.stderr.decode()
    assert err.startswith(f"Anchor map: 3 records, {info['keys']} keys, {info['anchors']} anchors, {info['repeats']} repeats "
                          f"(k={K}, w={WIN})\nPlaced ") and err.count("\n") == 2
    ps = json.load(open(d / "place.json"))
    assert (ps["records"], ps["keys"], ps["anchors"], ps["reads"]) == (3, info["keys"], info["anchors"], len(reads))
    assert ps["placed"] == s["placed"]


def test_options_gz_stdin_and_one_placement(data):
    d, genomes, reads, model = data
    with gzip.open(d / "reads.fq.gz", "wb") as f:
        f.write(open(d / "reads.fq", "rb").read())
    p = run(["map", d / "ref.fa", d / "reads.fq.gz", "--band", 31, "-a", 3, "-p", 200, "-N", 8, "-q"])
    want = paf(model, reads, W=31, min_votes=3, prefix=200, max_placements=8)
    assert p.stdout.decode() == want
    check_lines(want)
    with open(d / "reads.fq", "rb") as f:
        p = run(["map", d / "ref.fa", "--band", 31, "-a", 3, "-p", 200, "--max-placements", 8, "-q"], stdin=f)
    assert p.stdout.decode() == want
    p = run(["map", d / "ref.fa", d / "reads.fq", "-N", 1])
    one = p.stdout.decode()
    assert one == paf(model, reads, max_placements=1)
    rows = check_lines(one)
    assert all(c[13] == "rk:i:0" and c[14] == "np:i:1" for c in rows) and any(c[15] != "rv:i:0" for c in rows)
    assert b"Anchor map: 3 records" in p.stderr and b"Mapped " in p.stderr


def test_an_index_restricts_the_anchors(data, oracle, dcn):
    """-x at w = 1: the file's k and w are used, chrB's keys are gone and nothing lands there"""
    d, genomes, reads, _ = data
    full = dcn.Index.from_keys(oracle.Index.build(genomes, k=K, w=1).keys(), K, 1)
    host = dcn.Index.from_keys(oracle.Index.build([genomes[1]], k=K, w=1).keys(), K, 1)
    part = full.diff(host)
    part.write(str(d / "part.idx"))
    model = PW.AnchorModel(oracle, K, 1, part.keys()).add(genomes)
    for i in (full, host, part):
        i.close()
    some = reads[:300]
    with open(d / "some.fa", "wb") as f:
        for i, r in enumerate(some):
            f.write(b">read%d\n" % i + r + b"\n")
    p = run(["map", d / "ref.fa", d / "some.fa", "-x", d / "part.idx", "-s", d / "part.json", "-q"])
    got = p.stdout.decode()
    assert got == paf(model, some)
    check_lines(got)
    assert "\tchrB\t" not in got and "\tchrA\t" in got and "\tchrC\t" in got
    s = json.load(open(d / "part.json"))
    assert (s["k"], s["w"], s["keys"], s["anchors"]) == (K, 1, len(model.keys), model.info()["anchors"])
