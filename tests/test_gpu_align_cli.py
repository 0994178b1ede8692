"""`deacon-hip align` end to end: its PAF against `deacon-hip verify`'s for the same arguments (columns 1-9 and 12 and every
tag but cg identical line by line) and columns 10 and 11 and cg:Z: against the model of tests/_align_worker.py; the
summary's totals; --verified-only; small batches under DCN_CLI_ALIGN_BATCH_BASES; .gz and stdin inputs.  verify's own
output is pinned by tests/test_gpu_verify_cli.py: here it is the reference for what align must leave as it is."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import _align_worker as AW
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
    d = tmp_path_factory.mktemp("align_cli")
    rng = np.random.default_rng(1461)
    genomes = random_reads(rng, 3, 20_000, 20_000)
    with open(d / "ref.fa", "wb") as f:
        for name, g in zip(NAMES, genomes):
            f.write(b">" + name.encode() + b" synthetic record\n")
            f.write(b"\n".join(g[i:i + 60] for i in range(0, len(g), 60)) + b"\n")
    reads = []
    for i in range(200):
        R, ln = int(rng.integers(0, 3)), int(rng.integers(80, 400))
        at = int(rng.integers(0, 20_000 - ln))
        s = genomes[R][at:at + ln]
        if i % 3 == 1:
            s = VW.mutate_mixed(rng, s, 0.05)
        if i % 9 == 2:
            s = VW.mutate_mixed(rng, s, 0.25)
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


def check_against_verify(align_out, verify_out, genomes, reads):
    """-> {matches, mismatches, insertions, deletions, cigar_ops} after checking every line"""
    a_lines, v_lines = align_out.decode().splitlines(), verify_out.decode().splitlines()
    assert len(a_lines) == len(v_lines)
    tot = {"matches": 0, "mismatches": 0, "insertions": 0, "deletions": 0, "cigar_ops": 0}
    for al, vl in zip(a_lines, v_lines):
        c = vl.split("\t")
        if "ve:i:0" in c:
            assert al == vl
            continue
        assert c[-2] == "ve:i:1" and c[-1].startswith("NM:i:")
        read = reads[int(c[0][4:])]
        S = read[int(c[2]):int(c[3])]
        d, runs = AW.align_pair(revcomp(S) if c[4] == "-" else S, genomes[NAMES.index(c[5])][int(c[7]):int(c[8])])
        assert d == int(c[-1][5:])
        t = {AW.OP_EQ: 0, AW.OP_X: 0, AW.OP_I: 0, AW.OP_D: 0}
        for x in runs:
            t[x & 15] += x >> 4
        assert al == "\t".join(c[:9] + [str(t[AW.OP_EQ]), str(sum(t.values()))] + c[11:] + ["cg:Z:" + AW.cigar_text(runs)])
        tot["matches"] += t[AW.OP_EQ]
        tot["mismatches"] += t[AW.OP_X]
        tot["insertions"] += t[AW.OP_I]
        tot["deletions"] += t[AW.OP_D]
        tot["cigar_ops"] += len(runs)
    return tot


def test_paf_against_verify_and_the_model(data):
    d, genomes, reads = data
    v = run(["verify", d / "ref.fa", d / "reads.fq", "-q", "-s", d / "verify.json"])
    a = run(["align", d / "ref.fa", d / "reads.fq", "-q", "-s", d / "align.json"])
    tot = check_against_verify(a.stdout, v.stdout, genomes, reads)
    assert tot["matches"] > 20_000 and min(tot["mismatches"], tot["insertions"], tot["deletions"]) > 50
    assert a.stdout.count(b"ve:i:0") > 5 and a.stdout.count(b"cg:Z:") > 150
    vs, as_ = json.load(open(d / "verify.json")), json.load(open(d / "align.json"))
    for key in tot:
        assert key not in vs
    assert {k: x for k, x in as_.items() if k not in tot and k != "time"} == {k: x for k, x in vs.items() if k != "time"}
    assert {k: as_[k] for k in tot} == tot
    assert tot["mismatches"] + tot["insertions"] + tot["deletions"] == as_["edits"]
    # the same lines in small batches, byte for byte
    small = run(["align", d / "ref.fa", d / "reads.fq", "-q"], env={"DCN_CLI_ALIGN_BATCH_BASES": "20000"})
    assert small.stdout == a.stdout
    # without -q the tool says what it aligned
    loud = run(["align", d / "ref.fa", d / "reads.fq", "-o", d / "out.paf"])
    assert f"Aligned {as_['verified']} placements in {tot['cigar_ops']} runs".encode() in loud.stderr
    assert f"Verified {as_['verified']} of {as_['placements']} placements".encode() in loud.stderr
    assert (d / "out.paf").read_bytes() == a.stdout


def test_thresholds_and_verified_only(data):
    d, genomes, reads = data
    opts = ["-q", "-N", "2", "--band", "128", "-a", "3", "-e", "12", "--max-div", "40"]
    v = run(["verify", d / "ref.fa", d / "reads.fq"] + opts)
    a = run(["align", d / "ref.fa", d / "reads.fq"] + opts + ["-s", d / "tight.json"])
    tot = check_against_verify(a.stdout, v.stdout, genomes, reads)
    vo = run(["verify", d / "ref.fa", d / "reads.fq", "--verified-only"] + opts)
    ao = run(["align", d / "ref.fa", d / "reads.fq", "--verified-only"] + opts)
    assert check_against_verify(ao.stdout, vo.stdout, genomes, reads) == tot
    assert b"ve:i:0" not in ao.stdout and b"ve:i:0" in a.stdout and ao.stdout.count(b"\n") == ao.stdout.count(b"cg:Z:")
    s = json.load(open(d / "tight.json"))
    assert (s["max_edits"], s["max_permille"]) == (12, 40) and {k: s[k] for k in tot} == tot


def test_gz_and_stdin_inputs(data):
    d, genomes, reads = data
    a = run(["align", d / "ref.fa", d / "reads.fq", "-q"])
    assert run(["align", d / "ref.fa", d / "reads.fq.gz", "-q"]).stdout == a.stdout
    with open(d / "reads.fq", "rb") as f:
        assert run(["align", d / "ref.fa", "-q"], stdin=f).stdout == a.stdout
    with open(d / "reads.fq", "rb") as f:
        assert run(["align", d / "ref.fa", "-", "-q"], stdin=f).stdout == a.stdout
