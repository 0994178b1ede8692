"""`deacon-hip map-pairs` end to end against the model of tests/_place_pair_worker.py: every PAF line, the summary's
counts and the insert histogram; two files, one interleaved file and stdin byte-identical; many batches through the test
hook; -x, .gz and -N 1; the errors of odd and unequal inputs; and `deacon-hip map` on the same reads against its own
model, since the two subcommands share the loading of the reference and the PAF columns."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import _place_pair_worker as PPW
import _place_worker as PW
from _place_pair_worker import F
from conftest import mutate, random_reads
from test_gpu_place_split_cli import paf as map_paf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
K, WIN = 31, 15
NAMES = ("chrA", "chrB", "chrC")


def run(args, env=None, stdin=None, code=0):
    p = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})),
                       stdin=stdin if stdin is not None else subprocess.DEVNULL)
    assert p.returncode == code, p.stderr.decode()[-2000:]
    return p


def fastq(path, reads, first=0, step=1, opener=open):
    with opener(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@read%d/%d some text\n" % ((first + i * step) // 2, (first + i * step) % 2 + 1) + r + b"\n+\n" + b"I" * len(r) + b"\n")


@pytest.fixture(scope="module")
def data(tmp_path_factory, oracle):
    """a FASTA of three records; 600 pairs as two FASTQ files and as one interleaved file: fragments of 200 .. 700 bases
    on either strand, some mutated, long fragments, mates of one window, random mates, mates on different records"""
    d = tmp_path_factory.mktemp("map_pairs_cli")
    rng = np.random.default_rng(991)
    genomes = random_reads(rng, 3, 20_000, 20_000)
    with open(d / "ref.fa", "wb") as f:
        for name, g in zip(NAMES, genomes):
            f.write(b">" + name.encode() + b" synthetic record\n")
            f.write(b"\n".join(g[i:i + 60] for i in range(0, len(g), 60)) + b"\n")
    m1s, m2s = [], []
    for i in range(600):
        lo, hi = (1001, 1500) if i % 10 == 3 else (200, 700)
        _, _, frag = PPW.fragment(rng, genomes, lo, hi)
        L1, L2 = int(rng.integers(60, 151)), int(rng.integers(60, 151))
        if i % 9 == 4:
            L2 = K + WIN - 1
        a, b = PPW.mates_of(frag, L1, L2, flip=bool(i % 2))
        if i % 5 == 1:
            a, b = mutate(rng, a, 0.04), mutate(rng, b, 0.04)
        if i % 13 == 6:
            b = random_reads(rng, 1, 100, 150)[0]
        if i % 17 == 8:
            a = PPW.fragment(rng, genomes, 100, 150)[2]
        if i % 29 == 11:
            a = PW.cut(rng, genomes, 140, 140) + a  # a chimeric mate
        m1s.append(a)
        m2s.append(b)
    inter = [m for pair in zip(m1s, m2s) for m in pair]
    fastq(d / "r1.fq", m1s, 0, 2)
    fastq(d / "r2.fq", m2s, 1, 2)
    fastq(d / "inter.fq", inter)
    keys = oracle.Index.build(genomes, k=K, w=WIN).keys()
    model = PW.AnchorModel(oracle, K, WIN, keys).add(genomes)
    return d, genomes, inter, model


def paf(model, reads, hist_bin_bases=8, **kw):
    """(the lines `deacon-hip map-pairs` is to write, the model's rows, the histogram)"""
    k = model.k
    rows, hist = PPW.place_pair_all(model, reads, hist_bin_bases=hist_bin_bases, **kw)
    lines = []
    for i, (r, row) in enumerate(zip(reads, rows)):
        (rec, rev, votes, n_anchors, n_pos, q0, q1, p0, p1, rank, n_placed, rival, mapq, flags, pv, tlen) = row
        if rec == PPW.UNPLACED:
            continue
        cols = [f"read{i // 2}/{i % 2 + 1}", len(r), q0, q1, "-" if rev else "+", NAMES[rec], len(model.records[rec]), p0, p1,
                min(votes * k, q1 - q0), max(q1 - q0, p1 - p0), mapq,
                f"cm:i:{votes}", f"rk:i:{rank}", f"np:i:{n_placed}", f"rv:i:{rival}", f"na:i:{n_anchors}", f"ns:i:{n_pos}",
                f"mt:i:{i % 2 + 1}", f"pr:i:{flags & 1}", f"rs:i:{flags >> 1 & 1}", f"pv:i:{pv}", f"tl:i:{tlen}"]
        lines.append("\t".join(str(c) for c in cols))
    return "".join(ln + "\n" for ln in lines), rows, hist


def hist_tsv(hist, hbin):
    out = "bin_start\tbin_end\tpairs\n"
    for i, n in enumerate(hist):
        if n:
            out += f"{i * hbin}\t{'inf' if i == 255 else (i + 1) * hbin}\t{n}\n"
    return out


def test_paf_summary_histogram_and_every_form_of_input(data):
    d, genomes, reads, model = data
    run(["map-pairs", d / "ref.fa", d / "r1.fq", d / "r2.fq", "-o", d / "out.paf", "-s", d / "sum.json", "--insert-hist", d / "hist.tsv", "-q"])
    got = open(d / "out.paf").read()
    want, rows, hist = paf(model, reads)
    assert got == want
    lines = [ln.split("\t") for ln in got.splitlines()]
    assert all(len(c) == 23 and int(c[9]) <= int(c[10]) and 0 <= int(c[11]) <= 60 for c in lines)
    assert open(d / "hist.tsv").read() == hist_tsv(hist, 8)
    s = json.load(open(d / "sum.json"))
    info = model.info()
    pairs = [(rows[2 * u], rows[2 * u + 1]) for u in range(len(rows) // 2)]
    placed = lambda r: r[F["record"]] != PPW.UNPLACED  # noqa: E731
    proper = sum(1 for a, _ in pairs if a[F["flags"]] & 1)
    assert (s["records"], s["keys"], s["anchors"], s["repeats"]) == (3, info["keys"], info["anchors"], info["repeats"])
    assert (s["k"], s["w"], s["band_bases"], s["min_votes"], s["prefix_length"], s["max_placements"], s["max_insert"]) == \
        (K, WIN, 256, 2, 0, 4, 1000)
    assert s["reads"] == len(reads) and s["pairs"] == len(pairs) == 600 and s["placed"] == len(lines)
    assert s["proper"] == proper == sum(hist) > 350
    assert s["rescued_mates"] == sum(1 for r in rows if r[F["flags"]] & 2) > 20
    assert s["both_placed_not_proper"] == sum(1 for a, b in pairs if not a[F["flags"]] & 1 and placed(a) and placed(b)) > 40
    assert s["one_mate_placed"] == sum(1 for a, b in pairs if placed(a) != placed(b)) > 30
    assert s["neither_placed"] == sum(1 for a, b in pairs if not placed(a) and not placed(b))
    assert s["proper"] + s["both_placed_not_proper"] + s["one_mate_placed"] + s["neither_placed"] == s["pairs"]
    assert s["mapq60"] == sum(c[11] == "60" for c in lines) and s["mapq0"] == sum(c[11] == "0" for c in lines)
    run_, median = 0, None
    for i, n in enumerate(hist):
        run_ += n
        if median is None and run_ * 2 >= proper:
            median = i * 8
    assert s["insert_median_bin_start"] == median and 300 < median < 600
    assert [(x["name"], x["length"], x["placements"]) for x in s["placements_by_record"]] == \
        [(n, 20_000, sum(c[5] == n for c in lines)) for n in NAMES]
    # one interleaved file, and the same from stdin
    p = run(["map-pairs", d / "ref.fa", d / "inter.fq", "-q"])
    assert p.stdout.decode() == got
    with open(d / "inter.fq", "rb") as f:
        p = run(["map-pairs", d / "ref.fa", "-"], stdin=f)
    assert p.stdout.decode() == got and b"Anchor map: 3 records" in p.stderr and b"Mapped 600 pairs" in p.stderr
    # batches of 5,000 bases in a context of 10,000: many batches, none of which cuts a pair; the histogram is summed
    for inputs in ((d / "r1.fq", d / "r2.fq"), (d / "inter.fq",)):
        run(["map-pairs", d / "ref.fa", *inputs, "-o", d / "small.paf", "--insert-hist", d / "small.tsv", "-s", d / "small.json", "-q"],
            env={"DCN_CLI_MAPPAIRS_BATCH_BASES": "5000"})
        assert open(d / "small.paf").read() == got and open(d / "small.tsv").read() == hist_tsv(hist, 8)
        s2 = json.load(open(d / "small.json"))
        assert all(s2[f] == s[f] for f in s if f not in ("time", "input", "input2"))


def test_no_proper_pair_gives_a_null_median(data, tmp_path):
    d, genomes, reads, model = data
    fastq(tmp_path / "a.fq", [genomes[0][100:250], genomes[1][100:250]])
    run(["map-pairs", d / "ref.fa", tmp_path / "a.fq", "-s", tmp_path / "s.json", "--insert-hist", tmp_path / "h.tsv", "-q"])
    s = json.load(open(tmp_path / "s.json"))
    assert s["proper"] == 0 and s["insert_median_bin_start"] is None and s["both_placed_not_proper"] == 1
    assert open(tmp_path / "h.tsv").read() == "bin_start\tbin_end\tpairs\n"


def test_options_gz_and_one_placement(data):
    d, genomes, reads, model = data
    for name in ("r1.fq", "r2.fq"):
        with gzip.open(d / (name + ".gz"), "wb") as f:
            f.write(open(d / name, "rb").read())
    p = run(["map-pairs", d / "ref.fa", d / "r1.fq.gz", d / "r2.fq.gz", "--band", 31, "-a", 3, "-p", 120, "-N", 8, "-I", 450,
             "--insert-bin", 2, "--insert-hist", d / "h2.tsv", "-q"])
    want, _, hist = paf(model, reads, W=31, min_votes=3, prefix=120, max_placements=8, max_insert=450, hist_bin_bases=2)
    assert p.stdout.decode() == want
    assert open(d / "h2.tsv").read() == hist_tsv(hist, 2) and hist[255] == 0 and sum(hist) > 100
    p = run(["map-pairs", d / "ref.fa", d / "inter.fq", "--max-placements", 1, "--max-insert", 2000, "--insert-bin", 4,
             "--insert-hist", d / "h3.tsv", "-q"])
    want, rows, hist = paf(model, reads, max_placements=1, max_insert=2000, hist_bin_bases=4)
    assert p.stdout.decode() == want and all(r[F["rank"]] == 0 for r in rows)
    assert open(d / "h3.tsv").read() == hist_tsv(hist, 4) and hist[255] > 20 and "\tinf\t" in hist_tsv(hist, 4)


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
    some = reads[:200]
    fastq(d / "some.fq", some)
    p = run(["map-pairs", d / "ref.fa", d / "some.fq", "-x", d / "part.idx", "-s", d / "part.json", "-q"])
    got = p.stdout.decode()
    assert got == paf(model, some)[0]
    assert "\tchrB\t" not in got and "\tchrA\t" in got and "\tchrC\t" in got
    s = json.load(open(d / "part.json"))
    assert (s["k"], s["w"], s["keys"], s["anchors"], s["pairs"]) == (K, 1, len(model.keys), model.info()["anchors"], 100)


def test_odd_and_unequal_inputs(data, tmp_path):
    d, genomes, reads, model = data
    fastq(tmp_path / "odd.fq", reads[:7])
    p = run(["map-pairs", d / "ref.fa", tmp_path / "odd.fq", "-q"], code=1)
    assert p.stderr.decode() == "Error: Paired input ended with an unpaired record\n"
    fastq(tmp_path / "three.fq", reads[0:6:2])
    fastq(tmp_path / "two.fq", reads[1:4:2])
    p = run(["map-pairs", d / "ref.fa", tmp_path / "three.fq", tmp_path / "two.fq", "-q"], code=1)
    assert p.stderr.decode() == "Error: the first input has more records than the second\n"
    p = run(["map-pairs", d / "ref.fa", tmp_path / "two.fq", tmp_path / "three.fq", "-q"], code=1)
    assert p.stderr.decode() == "Error: the second input has more records than the first\n"


def test_map_on_the_same_reads_is_unchanged(data):
    """`map` through the shared loading of the reference and the shared PAF columns: its own model, its own lines"""
    d, genomes, reads, model = data
    with open(d / "plain.fq", "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@read%d some text\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n")
    p = run(["map", d / "ref.fa", d / "plain.fq", "-q"])
    assert p.stdout.decode() == map_paf(model, reads)
