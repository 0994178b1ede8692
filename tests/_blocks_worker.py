"""The model of tests/test_blocks_abi.py and tests/test_gpu_blocks*.py, tests/test_gpu_gvcf_cli.py.

THE DEFINITION OF A REFERENCE BLOCK (include/deacon_hip_blocks.h), written as it reads: the class of a position from
tests/_genotype_worker.decide, the blocks by a plain loop over the positions, the merge by a plain loop over the blocks.
Python integers; nothing here is shared with csrc/dcn_blocks.h.  The counts and sums it is given come from the CPU pile-up of
tests/_pileup_worker.py and tests/_quality_worker.py, never from the device."""
import numpy as np

import _genotype_worker as GW
import _pileup_worker as PW

NO_COVERAGE, UNCALLED, REF, VARIANT = 0, 1, 2, 255
DEFAULT_EDGES = (20, 40, 60, 80, 99)


def classify(counts8, sums4, ref_column, is_break=False, edges=DEFAULT_EDGES, **params):
    """rule B2 at one position -> (cls, gq, D)"""
    d = GW.decide(counts8[:4], sums4, ref_column, **params)
    D = sum(int(x) for x in counts8[:4])
    depth = sum(int(x) for x in counts8[:6])
    ploidy = params.get("ploidy", 2)
    if is_break or d["site"]:
        cls = VARIANT
    elif depth == 0:
        cls = NO_COVERAGE
    elif d["gt"] != GW.NONE and ref_column <= 3 and GW.genotypes(ploidy)[d["best"]] == (ref_column,) * ploidy:
        cls = REF + sum(1 for e in edges if e <= d["gq"])
    else:
        cls = UNCALLED
    return cls, d["gq"], D


def blocks_of(cls, gq, D, start=0):
    """rules B3 - B5 over per-position lists -> [(pos, len, cls, min_gq, min_depth, max_depth, sum_depth)]"""
    out, q, n = [], 0, len(cls)
    while q < n:
        if cls[q] == VARIANT:
            q += 1
            continue
        e = q
        while e + 1 < n and cls[e + 1] == cls[q]:
            e += 1
        out.append((start + q, e - q + 1, int(cls[q]), min(gq[q:e + 1]), min(D[q:e + 1]), max(D[q:e + 1]), sum(D[q:e + 1])))
        q = e + 1
    return out


def blocks_range(counts, sums, record, start=0, n=None, breaks=(), edges=DEFAULT_EDGES, **params):
    """counts[len(record), 8] and sums[len(record), 4] of one record -> (cls uint8[n], [block tuples])"""
    n = len(record) - start if n is None else n
    brk = set(int(b) for b in breaks)
    assert all(start <= b < start + n for b in brk)
    cls, gq, D = [], [], []
    for p in range(start, start + n):
        c, g, d = classify(counts[p], sums[p], PW.column(record[p]), p in brk, edges, **params)
        cls.append(c), gq.append(g), D.append(d)
    return np.array(cls, np.uint8).reshape(-1), blocks_of(cls, gq, D, start)


def merge(blocks):
    """rule B6 over block tuples in ascending position"""
    out = []
    for b in blocks:
        if out and out[-1][0] + out[-1][1] == b[0] and out[-1][2] == b[2]:
            a = out.pop()
            b = (a[0], a[1] + b[1], a[2], min(a[3], b[3]), min(a[4], b[4]), max(a[5], b[5]), a[6] + b[6])
        else:
            assert not out or out[-1][0] + out[-1][1] <= b[0]
        out.append(b)
    return out


def device_blocks(blocks):
    """the structured array of AnchorMap.reference_blocks as block tuples; the reserved word must be 0"""
    assert not blocks["reserved"].any()
    return [(int(b["pos"]), int(b["len"]), int(b["cls"]), int(b["min_gq"]), int(b["min_depth"]), int(b["max_depth"]), int(b["sum_depth"]))
            for b in blocks]


def to_array(dtype, blocks):
    """block tuples as the structured array"""
    out = np.zeros(len(blocks), dtype)
    for i, (pos, ln, cls, min_gq, min_depth, max_depth, sum_depth) in enumerate(blocks):
        out[i] = (pos, sum_depth, ln, min_depth, max_depth, min_gq, cls, 0)
    return out


def assert_range(amap, counts, sums, record_bytes, R, start=0, n=None, breaks=(), edges=DEFAULT_EDGES, **params):
    """AnchorMap.reference_blocks over a range against the model, the first difference named -> the model's (cls, blocks)"""
    want = blocks_range(counts, sums, record_bytes, start, n, breaks, edges, **params)
    cls, blocks = amap.reference_blocks(R, start, n, breaks=list(breaks), gq_edges=edges, **params)
    assert cls.dtype == np.uint8 and len(cls) == len(want[0])
    if not np.array_equal(cls, want[0]):
        q = int(np.flatnonzero(cls != want[0])[0])
        raise AssertionError(("cls", "record", R, "position", start + q, "got", int(cls[q]), "want", int(want[0][q]), params))
    got = device_blocks(blocks)
    if got != want[1]:
        k = next((i for i, (a, b) in enumerate(zip(got, want[1])) if a != b), min(len(got), len(want[1])))
        raise AssertionError(("block", k, "of", len(got), len(want[1]), "got", got[k:k + 1], "want", want[1][k:k + 1], (R, start, n), params))
    return want


def check_rule_rows(lines):
    """the `row` lines of tests/cpp/blocks_rule_test.cpp (counters, sums, N, DEL, the reference column, the parameters, the
    edges -> cls gq D) through this model -> how many there were"""
    n = 0
    for line in lines:
        if not line.startswith("row "):
            continue
        left, right = line[4:].split("->")
        x = [int(v) for v in left.split()]
        counts8 = x[0:4] + [x[8], x[9], 0, 0]
        prm = dict(zip(("ploidy", "min_depth", "min_gq", "min_qual", "err_centi", "het_centi"), x[11:17]))
        edges = x[18:18 + x[17]]
        assert len(edges) == x[17] == len(x) - 18
        assert list(classify(counts8, x[4:8], x[10], False, edges, **prm)) == [int(v) for v in right.split()], line
        n += 1
    return n
