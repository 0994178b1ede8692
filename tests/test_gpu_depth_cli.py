"""`deacon-hip classify --depth --depth-hist`: the depth block of every index in the summary JSON and the histogram TSV
equal the model of tests/_depth_worker.py, over many batches and a context recreated for a long record."""
import json
import os
import subprocess

import numpy as np
import pytest

import _depth_worker as W

pytestmark = pytest.mark.gpu

CLI = os.path.join(W.ROOT, "deacon-server_amd", "bin", "deacon-hip")


def test_cli_classify_depth(oracle, tmp_path):
    genomes = W.make_genomes()
    paths = []
    for j, seqs in enumerate(W.member_seqs(genomes)):
        fa, out = tmp_path / f"m{j}.fa", tmp_path / f"m{j}.idx"
        fa.write_text("".join(f">s{i}\n{s.decode()}\n" for i, s in enumerate(seqs)))
        subprocess.run([CLI, "index", "build", str(fa), "-o", str(out), "-q"], check=True, capture_output=True, timeout=300)
        paths.append(str(out))
    rng = np.random.default_rng(616)
    long_record = genomes[0] + genomes[1][:8000]  # 28 kbp: longer than the context below, which is made anew for it
    reads = W.sample(rng, genomes, 700, 60, 250) + [long_record] + W.sample(rng, genomes, 100, 60, 250)
    fq = tmp_path / "r.fq"
    with open(fq, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@r{i} extra\n{r.decode()}\n+\n{'I' * len(r)}\n")
    x = [a for p in paths for a in ("-x", p)]
    mkeys = [set(oracle.Index.read(p).keys().tolist()) for p in paths]
    model = W.occurrences(oracle, reads, 31, 15)
    env = dict(os.environ, DCN_CLI_CLASSIFY_BATCH_BASES="10000")  # a dozen batches of 10 kbp, a context of 20 kbp
    summ, hist = tmp_path / "depth.json", tmp_path / "h.tsv"
    p = subprocess.run([CLI, "classify", *x, str(fq), "--depth", "--depth-hist", str(hist), "-s", str(summ), "--coverage",
                        "--per-read", str(tmp_path / "per_read.tsv")], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr
    js = json.load(open(summ))
    rows = [line.split("\t") for line in open(hist).read().splitlines()]
    assert rows[0] == ["index", "depth", "keys"]
    want_rows = []
    for j, entry in enumerate(js["indexes"]):
        d = np.array(sorted(W.expected(model, mkeys, j).values()), dtype=np.int64)
        assert len(d) > 100 and d.max() > 2
        assert entry["depth"] == {"observed": len(d), "sum": int(d.sum()), "mean": pytest.approx(d.sum() / len(d), rel=1e-15),
                                  "median": float(np.median(d)), "saturated": 0}, j
        assert entry["keys_observed"] == len(d)  # --coverage beside it
        counts = np.bincount(np.minimum(d, 255), minlength=256)
        counts[0] = len(mkeys[j]) - len(d)
        want_rows += [[f"m{j}", ">=255" if b == 255 else str(b), str(int(c))] for b, c in enumerate(counts) if c]
        assert f"m{j}: depth mean " in p.stderr
    assert rows[1:] == want_rows
    assert len(open(tmp_path / "per_read.tsv").read().splitlines()) == len(reads) + 1
    plain = tmp_path / "plain.json"
    p = subprocess.run([CLI, "classify", *x, str(fq), "-s", str(plain)], capture_output=True, text=True, timeout=300,
                       env=env, check=True)
    assert all("depth" not in entry for entry in json.load(open(plain))["indexes"])
    assert "depth" not in p.stderr
