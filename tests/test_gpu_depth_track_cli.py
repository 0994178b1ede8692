"""`deacon-hip classify --track`: after the last read batch the records of a reference are tracked against the counters the
reads left, one block of lines per index.  The lines are compared with the model of tests/_depth_track_worker.py, the
summary's track block with the sums of the lines, and the run without --track with the same run with it."""
import json
import os
import subprocess

import numpy as np
import pytest

import _depth_worker as W
from _depth_track_worker import Model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
K, WIN = 31, 15
HOOK = 6000  # bases per batch; the first context takes twice that


def _lines(model, names, stems, bin_bases, cap):
    out = []
    for j, stem in enumerate(stems):
        out.append(f"# {stem}\trecord\tstart\tend\tn_positions\tn_keys\tn_observed\tsum_depth\tmax_depth\tmean")
        bo, b = model.bins(bin_bases, 1 << j, cap)
        for r, name in enumerate(names):
            ln = int(model.lens[r])
            for q in range(int(bo[r]), int(bo[r + 1])):
                start = (q - int(bo[r])) * bin_bases
                end = min(start + bin_bases, ln) if bin_bases else ln
                nk, sd = int(b["n_keys"][q]), int(b["sum_depth"][q])
                mean = f"{sd / nk:.4f}" if nk else "0"
                out.append("\t".join([name, str(start), str(end)] + [str(int(b[f][q])) for f in
                                     ("n_positions", "n_keys", "n_observed", "sum_depth", "max_depth")] + [mean]))
    return out


def test_classify_track(oracle, dcn, tmp_path):
    genomes = W.make_genomes()
    idx, mkeys, stems = [], [], []
    for j, seqs in enumerate(W.member_seqs(genomes)):
        o = oracle.Index.build(seqs, k=K, w=WIN)
        mkeys.append(set(o.keys().tolist()))
        path = tmp_path / f"ref{j}.idx"
        g = dcn.Index.from_keys(o.keys(), K, WIN)
        g.write(str(path))
        g.close()
        idx.append(str(path))
        stems.append(f"ref{j}")
    reads = [r for r in W.mixed_batch(genomes) if len(r)]
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads)))
    # the reference: a record longer than the first context (it is made again, larger), short ones over several batches
    records = [genomes[0]] + [genomes[1][a:a + 2500] for a in range(0, 20_000, 2500)] + [genomes[2][:HOOK + 1], genomes[2][7000:7040]]
    names = [f"rec{i}" for i in range(len(records))]
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b"".join(b">%s some description\n%s\n" % (n.encode(), s) for n, s in zip(names, records)))
    assert len(records[0]) > 2 * HOOK and sum(len(r) for r in records) > 4 * HOOK
    model = Model(oracle, records, K, WIN, mkeys, W.occurrences(oracle, reads, K, WIN))
    env = dict(os.environ, DCN_CLI_CLASSIFY_BATCH_BASES=str(HOOK))
    x = sum((["-x", p] for p in idx), [])
    runs = {}
    for name, extra, bin_bases, cap in (("plain", [], None, None), ("track", ["--track", str(fa)], 1000, 0),
                                        ("fine", ["--track", str(fa), "--track-bin", "333", "--track-cap", "2"], 333, 2),
                                        ("whole", ["--track", str(fa), "--track-bin", "0"], 0, 0)):
        tsv, summ, out = tmp_path / f"{name}.tsv", tmp_path / f"{name}.json", tmp_path / f"{name}.track"
        cmd = [CLI, "classify", *x, str(fq), "--depth", "--per-read", str(tsv), "-s", str(summ), "-q", *extra]
        if name != "track":
            cmd += ["--track-out", str(out)] if extra else []
        p = subprocess.run(cmd, check=True, capture_output=True, timeout=300, env=env)
        js = json.load(open(summ))
        runs[name] = (open(tsv, "rb").read(), js)
        if not extra:
            assert p.stdout == b"" and "track" not in js
            continue
        got = (p.stdout.decode() if name == "track" else open(out).read()).splitlines()  # (stdout is the default)
        want = _lines(model, names, stems, bin_bases, cap)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g == w
        t = js["track"]
        assert t["reference"] == str(fa) and t["bin_bases"] == bin_bases and t["depth_cap"] == cap
        assert [e["name"] for e in t["indexes"]] == stems
        for j, e in enumerate(t["indexes"]):
            rows = [ln.split("\t") for ln in got if not ln.startswith("#")]
            per = len(rows) // 3
            mine = rows[j * per:(j + 1) * per]
            assert e["bins"] == per and e["bins_observed"] == sum(1 for r in mine if int(r[5]) > 0) > 0
            assert e["sum_depth"] == sum(int(r[6]) for r in mine) > 0 and e["n_keys"] == sum(int(r[4]) for r in mine)
    # without --track nothing changes: the same rows per read, the same summary but for the block (and the clock)
    for name in ("track", "fine", "whole"):
        assert runs[name][0] == runs["plain"][0]
        a, b = dict(runs[name][1]), dict(runs["plain"][1])
        a.pop("track")
        a.pop("time"), b.pop("time")
        assert a == b


def test_track_implies_depth_and_checks_its_flags(tmp_path, dcn):
    keys = np.arange(1, 50, dtype=np.uint64)
    g = dcn.Index.from_keys(keys, K, WIN)
    path = tmp_path / "a.idx"
    g.write(str(path))
    g.close()
    fa = tmp_path / "ref.fa"
    fa.write_text(">r\n" + "ACGT" * 30 + "\n")
    fq = tmp_path / "reads.fq"
    fq.write_text("@a\n" + "ACGT" * 30 + "\n+\n" + "I" * 120 + "\n")
    summ = tmp_path / "s.json"
    p = subprocess.run([CLI, "classify", "-x", str(path), str(fq), "--track", str(fa), "--track-bin", "50", "-s", str(summ), "-q"],
                       check=True, capture_output=True, timeout=300)
    rows = p.stdout.decode().splitlines()
    assert rows[0].startswith("# a\trecord\tstart") and [r.split("\t")[1:3] for r in rows[1:]] == [["0", "50"], ["50", "100"], ["100", "120"]]
    js = json.load(open(summ))
    assert "depth" in js["indexes"][0] and js["track"]["indexes"][0]["bins"] == 3
    for bad in (["--track-cap", "65536"], ["--track-bin", "-1"]):
        q = subprocess.run([CLI, "classify", "-x", str(path), str(fq), "--track", str(fa), *bad], capture_output=True, timeout=300)
        assert q.returncode != 0 and b"invalid value" in q.stderr
