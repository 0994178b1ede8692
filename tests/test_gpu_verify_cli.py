"""`deacon-hip verify` end to end: its PAF against `deacon-hip map`'s for the same arguments (columns 1-9, 11 and 12 and map's
tags identical line by line) and the new tags and column 10 against the model of tests/_verify_worker.py; the summary's
fields; --verified-only; small batches under DCN_CLI_VERIFY_BATCH_BASES; -x, .gz and stdin inputs.  map's own output is
pinned by tests/test_gpu_place_split_cli.py: here it is the reference for what verify must leave as it is."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import _verify_worker as VW
from conftest import random_reads, revcomp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
NAMES = ("chrA", "chrB", "chrC")


def run(args, env=None, stdin=None):
    p = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})),
                       stdin=stdin)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("verify_cli")
    rng = np.random.default_rng(1351)
    genomes = random_reads(rng, 3, 20_000, 20_000)
    with open(d / "ref.fa", "wb") as f:
        for name, g in zip(NAMES, genomes):
            f.write(b">" + name.encode() + b" synthetic record\n")
            f.write(b"\n".join(g[i:i + 60] for i in range(0, len(g), 60)) + b"\n")
    reads = []
    for i in range(400):
        R, ln = int(rng.integers(0, 3)), int(rng.integers(80, 500))
        at = int(rng.integers(0, 20_000 - ln))
        s = genomes[R][at:at + ln]
        if i % 3 == 1:
            s = VW.mutate_mixed(rng, s, 0.05)
        if i % 9 == 2:
            s = VW.mutate_mixed(rng, s, 0.25)  # placed by a few hits at best, and then over the threshold
        if i % 10 == 6:  # two exact ends on one diagonal around 300 unrelated bases: placed, and over the threshold of 20 %
            at = int(rng.integers(0, 19_000))
            s = genomes[R][at:at + 100] + random_reads(rng, 1, 300, 300)[0] + genomes[R][at + 400:at + 500]
        if i % 7 == 3:
            s = s + revcomp(genomes[(R + 1) % 3][at:at + 150])
        if i % 11 == 4:
            s = random_reads(rng, 1, ln, ln)[0]
        if i % 13 == 5:
            s = s[:40] + b"N" + s[41:]
        reads.append(revcomp(s) if i % 2 else s)
    with open(d / "reads.fq", "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@read%d some text\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n")
    with gzip.open(d / "reads.fq.gz", "wb") as f:
        f.write((d / "reads.fq").read_bytes())
    return d, genomes, reads


def check_against_map(verify_out, map_out, genomes, reads, max_edits=1023, max_permille=200, verified_only=False):
    """-> (verified, unverified, edits, verified_bases) after checking every line"""
    v_lines, m_lines = verify_out.decode().splitlines(), map_out.decode().splitlines()
    pairs, meta = [], []
    for ln in m_lines:
        c = ln.split("\t")
        read = reads[int(c[0][4:])]
        S = read[int(c[2]):int(c[3])]
        pairs.append((revcomp(S) if c[4] == "-" else S, genomes[NAMES.index(c[5])][int(c[7]):int(c[8])]))
        meta.append(c)
    d = VW.levenshtein_many(pairs)
    want, tally = [], [0, 0, 0, 0]
    for c, (S, T), dist in zip(meta, pairs, d.tolist()):
        assert int(c[10]) == max(len(S), len(T))
        if dist <= VW.threshold(len(S), len(T), max_edits, max_permille):
            want.append("\t".join(c[:9] + [str(int(c[10]) - dist)] + c[10:] + ["ve:i:1", f"NM:i:{dist}"]))
            tally[0] += 1
            tally[2] += dist
            tally[3] += int(c[10])
        else:
            tally[1] += 1
            if not verified_only:
                want.append("\t".join(c + ["ve:i:0"]))  # (map's line, column 10 included, and the tag)
    assert v_lines == want
    return tuple(tally)


def test_paf_against_map_and_the_model(data):
    d, genomes, reads = data
    m = run(["map", d / "ref.fa", d / "reads.fq", "-q", "-s", d / "map.json"])
    v = run(["verify", d / "ref.fa", d / "reads.fq", "-q", "-s", d / "verify.json"])
    verified, unverified, edits, bases = check_against_map(v.stdout, m.stdout, genomes, reads)
    assert verified > 300 and unverified > 20 and edits > 500
    ms, vs = json.load(open(d / "map.json")), json.load(open(d / "verify.json"))
    extra = {"max_edits": 1023, "max_permille": 200, "verified": verified, "unverified": unverified, "edits": edits, "verified_bases": bases}
    for key in extra:
        assert key not in ms
    assert {k: x for k, x in vs.items() if k not in extra and k != "time"} == {k: x for k, x in ms.items() if k != "time"}
    assert {k: vs[k] for k in extra} == extra
    assert vs["verified"] + vs["unverified"] == vs["placements"]
    # the same lines in small batches, byte for byte
    small = run(["verify", d / "ref.fa", d / "reads.fq", "-q"], env={"DCN_CLI_VERIFY_BATCH_BASES": "20000"})
    assert small.stdout == v.stdout
    # without -q the tool says what it verified
    loud = run(["verify", d / "ref.fa", d / "reads.fq", "-o", d / "out.paf"])
    assert f"Verified {verified} of {verified + unverified} placements".encode() in loud.stderr and (d / "out.paf").read_bytes() == v.stdout


def test_thresholds_and_verified_only(data):
    d, genomes, reads = data
    m = run(["map", d / "ref.fa", d / "reads.fq", "-q", "-N", "2", "--band", "128", "-a", "3"])
    args = ["verify", d / "ref.fa", d / "reads.fq", "-q", "-N", "2", "--band", "128", "-a", "3", "-e", "12", "--max-div", "40"]
    v = run(args + ["-s", d / "tight.json"])
    tally = check_against_map(v.stdout, m.stdout, genomes, reads, max_edits=12, max_permille=40)
    only = run(args + ["--verified-only"])
    assert check_against_map(only.stdout, m.stdout, genomes, reads, max_edits=12, max_permille=40, verified_only=True) == tally
    assert tally[1] > 20 and only.stdout.count(b"\n") == tally[0] and b"ve:i:0" not in only.stdout
    s = json.load(open(d / "tight.json"))
    assert (s["max_edits"], s["max_permille"], s["verified"], s["unverified"], s["edits"], s["verified_bases"]) == (12, 40) + tally
    zero = run(["verify", d / "ref.fa", d / "reads.fq", "-q", "-N", "2", "--band", "128", "-a", "3", "-e", "0"])
    check_against_map(zero.stdout, m.stdout, genomes, reads, max_edits=0)


def test_index_gz_and_stdin_inputs(data, dcn):
    d, genomes, reads = data
    v = run(["verify", d / "ref.fa", d / "reads.fq", "-q"])
    idx = dcn.Index.build(genomes, 31, 15)
    idx.write(str(d / "ref.idx"))
    idx.close()
    assert run(["verify", d / "ref.fa", d / "reads.fq", "-x", d / "ref.idx", "-q"]).stdout == v.stdout
    assert run(["verify", d / "ref.fa", d / "reads.fq.gz", "-q"]).stdout == v.stdout
    with open(d / "reads.fq", "rb") as f:
        assert run(["verify", d / "ref.fa", "-q"], stdin=f).stdout == v.stdout
    with open(d / "reads.fq", "rb") as f:
        assert run(["verify", d / "ref.fa", "-", "-q"], stdin=f).stdout == v.stdout
