"""The model of tests/test_verify_abi.py and tests/test_gpu_verify*.py, and the worker of their subprocess case.

THE DEFINITION OF A VERIFIED PLACEMENT (include/deacon_hip.h), restated over bytes: S = the read interval, reverse-
complemented when the row says so; T = the record interval; two bases are EQUAL when both are in ACGTacgt and the same
letter whatever the case; d = the Levenshtein distance by the plain row-by-row dynamic programme (no wavefront, no band:
it shares nothing with the kernel); E = min(max_edits, max(m, n) * max_permille // 1000); edits = d when d <= E, else OVER;
UNPLACED for a row with record == UINT32_MAX.

levenshtein() is one pair, one row of the table per base of S.  levenshtein_many() runs the same programme for many pairs
at once, padded to the longest, and reads each pair's cell when its last row is reached: the tests use it for speed, and
tests/test_verify_abi.py checks the two against each other.

As a program (python tests/_verify_worker.py CASE) it runs one case in a process of its own, whose environment the test
has set, and exits non-zero with a traceback when a check fails."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from conftest import random_reads, revcomp  # noqa: E402

OVER, UNPLACED = 0xFFFFFFFE, 0xFFFFFFFF
MAX_EDITS = 1023

_CODE = np.full(256, -1, np.int16)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _CODE[_c | 0x20] = _i


def encode(seq, invalid):
    """bytes -> int16 codes: 0..3 for ACGTacgt, `invalid` (negative, one value per side) for everything else, so that an
    invalid base equals nothing, not even another invalid base"""
    a = _CODE[np.frombuffer(bytes(seq), np.uint8)].copy()
    a[a < 0] = invalid
    return a


def levenshtein(S, T):
    """the distance of two byte strings under rule 2's equality: row i of the table from row i - 1"""
    s, t = encode(S, -1), encode(T, -2)
    n = len(t)
    idx = np.arange(n + 1, dtype=np.int64)
    prev = idx.copy()
    for i in range(len(s)):
        x = np.empty(n + 1, np.int64)
        x[0] = i + 1
        x[1:] = np.minimum(prev[:-1] + (t != s[i]), prev[1:] + 1)  # substitution / match, a base of S alone
        prev = np.minimum.accumulate(x - idx) + idx                # a base of T alone: cur[j] = min(cur[j], cur[j - 1] + 1)
    return int(prev[n])


def levenshtein_many(pairs, chunk=512):
    """[(S, T)] -> int64[len(pairs)]: levenshtein() of every pair, a chunk of pairs per table"""
    out = np.zeros(len(pairs), np.int64)
    order = sorted(range(len(pairs)), key=lambda i: (len(pairs[i][0]), len(pairs[i][1])))
    chunks = [[]]
    for i in order:  # a chunk: at most `chunk` pairs of lengths within a factor of two, a quarter of a million cells per row
        m, n = len(pairs[i][0]), len(pairs[i][1])
        if chunks[-1]:
            m0, n_max = len(pairs[chunks[-1][0]][0]), max(max(len(pairs[j][1]) for j in chunks[-1]), n)
            n_min = min(min(len(pairs[j][1]) for j in chunks[-1]), n)
            if len(chunks[-1]) >= chunk or (len(chunks[-1]) + 1) * (n_max + 1) > 1 << 18 or m > 2 * m0 + 32 or n_max > 2 * n_min + 32:
                chunks.append([])
        chunks[-1].append(i)
    for ids in chunks:
        if not ids:
            continue
        m = np.array([len(pairs[i][0]) for i in ids])
        n = np.array([len(pairs[i][1]) for i in ids])
        M, Nn, B = int(m.max()), int(n.max()), len(ids)
        Sa, Ta = np.full((B, max(M, 1)), -3, np.int16), np.full((B, max(Nn, 1)), -4, np.int16)
        for b, i in enumerate(ids):
            Sa[b, :m[b]] = encode(pairs[i][0], -1)
            Ta[b, :n[b]] = encode(pairs[i][1], -2)
        Ta = Ta[:, :Nn]
        idx = np.arange(Nn + 1, dtype=np.int64)
        prev = np.tile(idx, (B, 1))
        res = np.where(m == 0, n, 0).astype(np.int64)
        rows = np.arange(B)
        for i in range(M):
            x = np.empty((B, Nn + 1), np.int64)
            x[:, 0] = i + 1
            x[:, 1:] = np.minimum(prev[:, :-1] + (Ta != Sa[:, i:i + 1]), prev[:, 1:] + 1)
            prev = np.minimum.accumulate(x - idx, axis=1) + idx
            hit = m == i + 1
            if hit.any():
                res[hit] = prev[rows[hit], n[hit]]
        out[ids] = res
    return out


def threshold(m, n, max_edits=MAX_EDITS, max_permille=200):
    return min(max_edits, max(m, n) * max_permille // 1000)


def intervals(read, record, row):
    """(S, T) of a placed row: the two byte strings rule 1 names"""
    S = bytes(read)[int(row["read_start"]):int(row["read_end"])]
    if int(row["reverse"]):
        S = revcomp(S)  # (conftest's: ACGTacgt are complemented, every other byte stays what it is: invalid)
    return S, bytes(record)[int(row["ref_start"]):int(row["ref_end"])]


def verify_rows(reads, records, rows, row_offsets=None, max_edits=MAX_EDITS, max_permille=200):
    """the model of dcn_verify_batch -> np.uint32[len(rows)]"""
    owner = np.arange(len(rows)) if row_offsets is None else np.repeat(np.arange(len(reads)), np.diff(np.asarray(row_offsets, np.int64)))
    assert len(owner) == len(rows)
    out = np.full(len(rows), UNPLACED, np.uint32)
    placed = [i for i in range(len(rows)) if int(rows["record"][i]) != UNPLACED]
    pairs = [intervals(reads[owner[i]], records[int(rows["record"][i])], rows[i]) for i in placed]
    for i, (S, T), d in zip(placed, pairs, levenshtein_many(pairs)):
        out[i] = d if d <= threshold(len(S), len(T), max_edits, max_permille) else OVER
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------
def edit(rng, seq, n_sub=0, n_ins=0, n_del=0):
    """seq with that many substitutions (each to another letter), inserted and deleted bases at random places"""
    s = bytearray(seq)
    for _ in range(n_sub):
        at = int(rng.integers(0, len(s)))
        s[at] = [x for x in b"ACGT" if x != s[at] & 0xDF][int(rng.integers(0, 3))]
    for _ in range(n_ins):
        s.insert(int(rng.integers(0, len(s) + 1)), b"ACGT"[int(rng.integers(0, 4))])
    for _ in range(n_del):
        if s:
            del s[int(rng.integers(0, len(s)))]
    return bytes(s)


def mutate_mixed(rng, seq, rate):
    """every base is, with probability `rate`, substituted, deleted, or followed by an inserted base (a third each)"""
    out = bytearray()
    for c in bytes(seq):
        if rng.random() < rate:
            kind = int(rng.integers(0, 3))
            if kind == 0:
                out.append(b"ACGT"[(b"ACGT".find(bytes([c & 0xDF])) + int(rng.integers(1, 4))) % 4])
            elif kind == 1:
                out += bytes([c, b"ACGT"[int(rng.integers(0, 4))]])
        else:
            out.append(c)
    return bytes(out)


def make_row(dtype, record, reverse, read_start, read_end, ref_start, ref_end):
    r = np.zeros(1, dtype)
    r["record"], r["reverse"], r["read_start"], r["read_end"], r["ref_start"], r["ref_end"] = record, reverse, read_start, read_end, ref_start, ref_end
    return r


def build_map(O, dcn, records, k=31, w=15, calls=None, keep_bases=True):
    """an AnchorMap over the records' own keys; calls: how many records each add call takes (None: all in one)"""
    idx = dcn.Index.from_keys(O.Index.build([r for r in records if len(r) >= k] or [b"A" * k], k=k, w=w).keys(), k, w)
    amap = dcn.AnchorMap(idx, keep_bases=keep_bases)
    idx.close()
    at = 0
    for n in (calls or [len(records)]):
        amap.add_records(records[at:at + n])
        at += n
    assert at == len(records)
    return amap


def fetched_text(record):
    """what fetch returns for a record: upper case, N for every byte outside ACGTacgt"""
    a = np.frombuffer(bytes(record), np.uint8)
    return np.where(_CODE[a] >= 0, a & 0xDF, ord("N")).astype(np.uint8).tobytes()


# ---- subprocess case -----------------------------------------------------------------------------------------------
def case_growth(O, dcn):
    """DCN_ANCHOR_STORE_BASES = 64: the store starts at 64 bases and grows with the first call and twice more; records
    of lengths that leave every add call's successor mid-word, fetched whole and verified against the model"""
    assert os.environ.get("DCN_ANCHOR_STORE_BASES") == "64"
    rng = np.random.default_rng(77)
    records = random_reads(rng, 1, 50, 50) + random_reads(rng, 1, 131, 131) + random_reads(rng, 2, 45, 77) + random_reads(rng, 1, 900, 900)
    amap = build_map(O, dcn, records, calls=[1, 1, 2, 1])  # 64 bases hold the first call; each later call outgrows the store
    placer = dcn.Placer(amap, max_batch_bases=1 << 16, max_batch_reads=1 << 10)
    for R, rec in enumerate(records):
        assert amap.fetch(R, 0, len(rec)) == fetched_text(rec), R
    reads, rows = [], []
    for R, rec in enumerate(records):
        for rev in (0, 1):
            s = edit(rng, rec, n_sub=2, n_ins=1)
            reads.append(revcomp(s) if rev else s)
            rows.append(make_row(dcn.filter.PLACEMENT_DTYPE, R, rev, 0, len(s), 0, len(rec)))
    rows = np.concatenate(rows)
    b, o = O.concat_reads(reads)
    got = placer.verify_batch(b, o, rows)
    want = verify_rows(reads, records, rows)
    assert got.tolist() == want.tolist() and (want <= 3).all(), (got, want)
    placer.close()
    amap.close()
    print("verify growth ok")


if __name__ == "__main__":
    import deacon_server_amd as dcn
    from oracle import oracle as O
    O.lib()
    {"growth": case_growth}[sys.argv[1]](O, dcn)
