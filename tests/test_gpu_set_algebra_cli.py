"""`deacon-hip index intersect / compare / select` on the GPU: index files written from Python, the tool's outputs loaded
back (or parsed) and compared with numpy set algebra over the same keys."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, mix64

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
K, W = 31, 15


def ids(lo, hi):
    return mix64(np.arange(lo, hi, dtype=np.uint64))


@pytest.fixture(scope="module")
def files(dcn, tmp_path_factory):
    """three index files with exclusive, pairwise and triple overlaps; key 0 in the first two; and an empty one"""
    d = tmp_path_factory.mktemp("set_algebra_cli")
    zero = np.zeros(1, np.uint64)
    members = [np.concatenate([ids(1, 301), ids(901, 1001), ids(1001, 1051), ids(1201, 1301), zero]),
               np.concatenate([ids(301, 601), ids(901, 1001), ids(1051, 1201), ids(1201, 1301), zero]),
               np.concatenate([ids(601, 901), ids(1001, 1051), ids(1051, 1201), ids(1201, 1301)]),
               np.zeros(0, np.uint64)]
    paths = []
    for j, m in enumerate(members):
        paths.append(str(d / f"m{j}.idx"))
        dcn.Index.from_keys(m, K, W).write(paths[-1])
    return d, paths, members


def run(*args):
    p = subprocess.run([CLI, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (args, p.stderr)
    return p


def load_keys(dcn, path):
    idx = dcn.Index.from_file(path)
    assert (idx.kmer_length, idx.window_size) == (K, W)
    return np.sort(idx.keys())


def test_index_intersect(dcn, files):
    d, paths, members = files
    out = d / "ab.idx"
    p = run("index", "intersect", paths[0], paths[1], "-o", out)
    want = np.intersect1d(members[0], members[1])
    assert 0 in want and len(want) == 201
    assert np.array_equal(load_keys(dcn, out), want)
    assert f"Index 1: {len(members[0])} minimizers" in p.stderr and f"Index 2: {len(members[1])} minimizers" in p.stderr
    assert f"Intersection: {len(want)} minimizers from 2 indexes" in p.stderr and "Completed intersect operation in" in p.stderr
    run("index", "intersect", paths[0], paths[1], paths[2], "-o", out)
    assert np.array_equal(load_keys(dcn, out), np.sort(ids(1201, 1301)))
    p = run("index", "intersect", paths[0], paths[3], "-o", out)  # an empty result is written as a valid index file
    assert "Intersection: 0 minimizers from 2 indexes" in p.stderr and len(load_keys(dcn, out)) == 0


@pytest.mark.parametrize("opts, pick", [
    (["--all", "0", "--max-members", "1"], lambda c, b: (b[:, 0] == 1) & (c == 1)),          # member-specific
    (["--min-members", "2"], lambda c, b: c >= 2),                                            # core
    (["--all", "0,1", "--none", "2"], lambda c, b: (b[:, 0] == 1) & (b[:, 1] == 1) & (b[:, 2] == 0)),
    (["--any", "1,2", "--min-members", "1", "--max-members", "2"], lambda c, b: ((b[:, 1] == 1) | (b[:, 2] == 1)) & (c <= 2)),
    (["--all", "2", "--none", "2"], lambda c, b: c < 0),                                      # nothing: an empty index
])
def test_index_select(dcn, files, opts, pick):
    d, paths, members = files
    keys = np.unique(np.concatenate(members[:3]))
    b = np.stack([np.isin(keys, m) for m in members[:3]], axis=1).astype(np.int64)
    want = keys[pick(b.sum(1), b)]
    out = d / "sel.idx"
    p = run("index", "select", "-x", paths[0], "-x", paths[1], "-x", paths[2], *opts, "-o", out)
    assert f"Selected {len(want)} of {len(keys)} minimizers" in p.stderr
    assert np.array_equal(load_keys(dcn, out), want)


def test_index_compare(dcn, files):
    d, paths, members = files
    js = d / "cmp.json"
    p = run("index", "compare", *paths, "-s", js)  # the empty index takes part: its ratios are 0, not a division by zero
    n = len(paths)
    shared = np.array([[len(np.intersect1d(a, b)) for b in members] for a in members], dtype=np.int64)
    keys = np.diag(shared)
    union = np.unique(np.concatenate(members))
    masks = np.stack([np.isin(union, m) for m in members], axis=1)
    exclusive = [int((masks[:, j] & (masks.sum(1) == 1)).sum()) for j in range(n)]
    by_count = np.bincount(masks.sum(1), minlength=n + 1)[1:].tolist()

    blocks = p.stdout.split("\n\n")
    assert len(blocks) == 2
    for which, block in enumerate(blocks):
        rows = [line.split("\t") for line in block.strip("\n").split("\n")]
        assert rows[0] == ["index", "keys", "exclusive", *paths] and len(rows) == n + 1
        for i, row in enumerate(rows[1:]):
            assert row[0] == paths[i] and int(row[1]) == keys[i] and int(row[2]) == exclusive[i]
            for j in range(n):
                if which == 0:
                    assert int(row[3 + j]) == shared[i, j]
                else:
                    assert abs(float(row[3 + j]) - (shared[i, j] / keys[i] if keys[i] else 0.0)) <= 1e-6
                    if not keys[i]:
                        assert row[3 + j] == "0"
    s = json.loads(open(js).read())
    assert (s["k"], s["w"], s["union"]) == (K, W, len(union))
    assert s["members"] == [{"path": paths[i], "keys": int(keys[i]), "exclusive": exclusive[i]} for i in range(n)]
    assert s["shared"] == shared.tolist() and s["by_count"] == by_count and sum(s["by_count"]) == s["union"]
    for i in range(n):
        for j in range(n):
            denom = keys[i] + keys[j] - shared[i, j]
            assert abs(s["jaccard"][i][j] - (shared[i, j] / denom if denom else 0.0)) <= 1e-6
    assert s["jaccard"][3][3] == 0 and s["jaccard"][0][0] == 1
