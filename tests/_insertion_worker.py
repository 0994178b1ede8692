"""The model of tests/test_insertions_abi.py and tests/test_gpu_insertions*.py, and the worker of their subprocess cases.

THE DEFINITION OF AN INSERTION LEDGER (include/deacon_hip.h), restated over bytes.  The runs of a row come from
tests/_align_worker.py's table and walk, the counters from tests/_pileup_worker.py's add_runs; events_of_runs() follows the
same runs one at a time and collects rule L2's events into a Python list of tuples (p, front, len, bases, reverse).  L4 is
sorted() over those tuples, L5 a Counter, L6 comes from _pileup_worker's call_position (rule P6), L7 is a plain loop.
Nothing here is shared with csrc/dcn_insertions.h: no buckets, no scans, no lanes.

As a program (python tests/_insertion_worker.py CASE) it runs one case in a process of its own, whose environment the test
has set, and exits non-zero with a traceback when a check fails."""
import os
import sys
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _align_worker as AW  # noqa: E402
import _pileup_worker as PW  # noqa: E402
import _verify_worker as VW  # noqa: E402
from _verify_worker import OVER, UNPLACED, intervals  # noqa: E402
from conftest import random_reads, revcomp  # noqa: E402

FRONT, REVERSE = 1, 2
ROW = np.dtype([("record", np.uint32), ("reverse", np.uint32), ("read_start", np.uint32), ("read_end", np.uint32),
                ("ref_start", np.uint64), ("ref_end", np.uint64)])  # what a row of the model needs (the fields of a placement)


def letter(byte):
    """rule L2: a base of S as the ledger keeps it"""
    col = PW.column(byte)
    return b"ACGT"[col:col + 1] if col < 4 else b"N"


def events_of_runs(S, ref_start, reverse, runs):
    """rule L2: the events of one row's runs, one run at a time"""
    i = j = 0
    out = []
    for x in runs:
        ln, op = int(x) >> 4, int(x) & 15
        if op == AW.OP_I:
            out.append((ref_start + (j - 1 if j > 0 else 0), 1 if j == 0 else 0, ln, b"".join(letter(b) for b in S[i:i + ln]), int(reverse)))
            i += ln
        elif op == AW.OP_D:
            j += ln
        else:
            i += ln
            j += ln
    return out


def new_ledger(records):
    return [[] for _ in records]


def pile_rows(counts, ledger, reads, records, rows, row_offsets=None, max_edits=VW.MAX_EDITS, max_permille=200, select=None):
    """the model of dcn_pileup_batch on a map that keeps a ledger: _pileup_worker.pile_rows with the events beside the
    counters (ledger: one list per record) -> (edits, n_added)"""
    rows = rows.copy()
    if select is not None:
        rows["record"][~np.asarray(select, bool)] = UNPLACED
    owner = np.arange(len(rows)) if row_offsets is None else np.repeat(np.arange(len(reads)), np.diff(np.asarray(row_offsets, np.int64)))
    edits, offs, cigar = AW.align_rows(reads, records, rows, row_offsets, max_edits, max_permille)
    n_added = 0
    for r in range(len(rows)):
        if int(edits[r]) >= OVER:
            continue
        R = int(rows["record"][r])
        S, Tt = intervals(reads[owner[r]], records[R], rows[r])
        if len(Tt) == 0:
            continue  # rule P2: n = 0 adds nothing, to the ledger either
        runs = cigar[int(offs[r]):int(offs[r + 1])]
        assert PW.add_runs(counts[R], S, int(rows["ref_start"][r]), int(rows["reverse"][r]), runs) == (len(S), len(Tt))
        ledger[R] += events_of_runs(S, int(rows["ref_start"][r]), int(rows["reverse"][r]), runs)
        n_added += 1
    return edits, n_added


def fetch_range(events, start, n):
    """the model of dcn_anchor_map_insertions_fetch: rule L4 is the order of the tuples"""
    return sorted(e for e in events if start <= e[0] < start + n)


def winner(events_at_p):
    """rule L5 -> ((front, len, bases), count)"""
    tally = Counter(e[1:4] for e in events_at_p)
    allele = min(tally, key=lambda a: (-tally[a], a))
    return allele, tally[allele]


def call_range(counts, events, record, start=0, n=None, min_depth=3, min_permille=500):
    """the model of dcn_anchor_map_insertions_call -> [(p, front, len, bases, count, events)] in ascending p (rule L6)"""
    n = len(record) - start if n is None else n
    out = []
    for p in range(start, start + n):
        _, info = PW.call_position(counts[p], bytes(record)[p], min_depth, min_permille)
        if info & PW.SITE_INS and int(counts[p][PW.INS]) > 0:
            here = [e for e in events if e[0] == p]
            assert len(here) == int(counts[p][PW.INS])  # rule L2
            (front, ln, bases), count = winner(here)
            out.append((p, front, ln, bases, count, len(here)))
    return out


def consensus(counts, events, record, start=0, n=None, min_depth=3, min_permille=500, fill_ref=False):
    """rule L7, position by position"""
    n = len(record) - start if n is None else n
    called = {a[0]: a for a in call_range(counts, events, record, start, n, min_depth, min_permille)}
    out = []
    for p in range(start, start + n):
        ch, _ = PW.call_position(counts[p], bytes(record)[p], min_depth, min_permille)
        a = called.get(p)
        if a and a[1] == 1:
            out.append(a[3])
        if ch == "N":
            out.append(letter(bytes(record)[p]) if fill_ref else b"N")
        elif ch != "-":
            out.append(ch.encode())
        if a and a[1] == 0:
            out.append(a[3])
    return b"".join(out)


# ---- what the device returns, as the model's tuples ------------------------------------------------------------------
def events_as_tuples(events, bases):
    return [(int(e["pos"]), int(e["flags"]) & FRONT, int(e["len"]), bases[int(e["bases_offset"]):int(e["bases_offset"]) + int(e["len"])],
             (int(e["flags"]) & REVERSE) >> 1) for e in events]


def alleles_as_tuples(alleles, bases):
    return [(int(a["pos"]), int(a["flags"]), int(a["len"]), bases[int(a["bases_offset"]):int(a["bases_offset"]) + int(a["len"])],
             int(a["count"]), int(a["events"])) for a in alleles]


def assert_dense(items, bases):
    """bases_offset ascending and dense, the bases array exactly as long as the lengths say"""
    at = 0
    for x in items:
        assert int(x["bases_offset"]) == at
        at += int(x["len"])
    assert at == len(bases)


def assert_ledger(amap, records, counts, ledger, settings=((3, 500),), fills=(False, True)):
    """the whole ledger of a map against the model: fetch over whole records, info, and call and consensus per setting"""
    total = [0, 0]
    for R, rec in enumerate(records):
        ev, b = amap.insertions_fetch(R)
        assert_dense(ev, b)
        got, want = events_as_tuples(ev, b), fetch_range(ledger[R], 0, len(rec))
        assert got == want, ("fetch", R, [x for x in got if x not in want][:3], [x for x in want if x not in got][:3])
        total[0] += len(want)
        total[1] += sum(e[2] for e in want)
        for min_depth, min_permille in settings:
            al, b = amap.insertions_call(R, min_depth=min_depth, min_permille=min_permille)
            assert_dense(al, b)
            got, want = alleles_as_tuples(al, b), call_range(counts[R], ledger[R], rec, 0, None, min_depth, min_permille)
            assert got == want, ("call", R, min_depth, min_permille, got[:3], want[:3])
            for fill in fills:
                got = amap.consensus(R, min_depth=min_depth, min_permille=min_permille, fill_ref=fill)
                assert got == consensus(counts[R], ledger[R], rec, 0, None, min_depth, min_permille, fill), ("consensus", R, fill)
    assert amap.insertions_info() == tuple(total)
    assert total[0] == sum(int(c[:, PW.INS].sum()) for c in counts)
    return total


def rows_as(dtype, rows):
    """the model's rows in a placement dtype of the package"""
    out = np.zeros(len(rows), dtype)
    for f in ROW.names:
        out[f] = rows[f]
    return out


# ---- the end-to-end case ---------------------------------------------------------------------------------------------
TRUTH_SEED = 12


def truth_case(seed=TRUTH_SEED):
    """A 600-base random record and a truth with one substitution (at 150), a 2-base deletion (at 300) and a 3-base
    insertion (behind base 449), each outside homopolymers and repeats and 100 bases or more from the ends and from each
    other; error-free 100-base reads from the truth start every 5 bases on alternating strands, each with the row of the
    record interval it came from -> (record, truth, reads, rows)"""
    rng = np.random.default_rng(seed)
    record = random_reads(rng, 1, 600, 600)[0]
    sub = b"ACGT"[(b"ACGT".find(record[150:151]) + 1) % 4]
    two = [x for x in b"ACGT" if x not in (record[449], record[450])][:2]  # neither neighbour's letter: the run cannot move
    ins = bytes([two[0], two[1], two[0]])
    assert record[299] != record[301] and record[300] != record[302]  # ... nor can the deletion
    pieces = [(record[:150], 0), (bytes([sub]), 150), (record[151:300], 151), (record[302:450], 302), (ins, None), (record[450:], 450)]
    truth = b"".join(p for p, _ in pieces)
    ref_of = []  # per base of the truth: the record position it stands for (an inserted base: that of the base in front)
    for p, at in pieces:
        ref_of += [ref_of[-1]] * len(p) if at is None else list(range(at, at + len(p)))
    reads, rows = [], []
    for n, s in enumerate(range(0, len(truth) - 100 + 1, 5)):
        piece, rev = truth[s:s + 100], n & 1
        a, b = ref_of[s], ref_of[s + 99] + 1
        if s > 0 and ref_of[s] == ref_of[s - 1]:
            a += 1  # the read begins inside the insertion: its first record base is the next one
        reads.append(revcomp(piece) if rev else piece)
        row = np.zeros(1, ROW)
        row["record"], row["reverse"], row["read_start"], row["read_end"], row["ref_start"], row["ref_end"] = 0, rev, 0, 100, a, b
        rows.append(row)
    return record, truth, reads, np.concatenate(rows)


# ---- random rows for the differential test ---------------------------------------------------------------------------
def random_rows(seed, n_rows=300):
    """three records and n_rows rows on them: intervals of 0 .. 300 bases, edited by 0 - 25 % with insertions favoured, N and
    lower case in reads and records, both strands -> (records, reads, rows)"""
    rng = np.random.default_rng(seed)
    records = [random_reads(rng, 1, ln, ln, p_n=0.002, p_lower=0.1)[0] for ln in (700, 333, 1500)]
    reads, rows = [], []
    for _ in range(n_rows):
        R = int(rng.integers(0, 3))
        n = int(rng.integers(0, 301))
        a = int(rng.integers(0, len(records[R]) - n + 1))
        rate = float(rng.choice([0.0, 0.02, 0.05, 0.1, 0.25]))
        S = bytearray()
        for c in records[R][a:a + n]:
            if rng.random() < rate:
                kind = int(rng.integers(0, 6))  # 0: substituted, 1: deleted, 2 - 5: followed by 1 - 4 inserted bases
                if kind == 0:
                    S.append(b"ACGT"[int(rng.integers(0, 4))])
                elif kind >= 2:
                    S.append(c)
                    S += random_reads(rng, 1, kind - 1, kind - 1, p_n=0.05, p_lower=0.2)[0]
            else:
                S.append(c)
        if rng.random() < 0.1:
            S = bytearray(random_reads(rng, 1, 1, 3)[0]) + S  # an I run first
        rev, pre = int(rng.integers(0, 2)), int(rng.integers(0, 40))
        S = bytes(S)
        reads.append(random_reads(rng, 1, pre, pre)[0] + (revcomp(S) if rev else S) + random_reads(rng, 1, 0, 20)[0])
        row = np.zeros(1, ROW)
        row["record"], row["reverse"], row["read_start"], row["read_end"], row["ref_start"], row["ref_end"] = R, rev, pre, pre + len(S), a, a + n
        rows.append(row)
    return records, reads, np.concatenate(rows)


# ---- the subprocess cases --------------------------------------------------------------------------------------------
def _run_truth(O, dcn, batches):
    record, truth, reads, rows = truth_case()
    amap = VW.build_map(O, dcn, [record])
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    placer = dcn.Placer(amap, max_batch_bases=1 << 16, max_batch_reads=1 << 10)
    rows = rows_as(dcn.filter.PLACEMENT_DTYPE, rows)
    counts, ledger = PW.new_counts([record]), new_ledger([record])
    cuts = np.linspace(0, len(reads), batches + 1).astype(int)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        b, o = O.concat_reads(reads[lo:hi])
        edits, n_added = placer.pileup_batch(b, o, rows[lo:hi])
        want_edits, want_added = pile_rows(counts, ledger, reads[lo:hi], [record], rows[lo:hi])
        assert edits.tolist() == want_edits.tolist() and n_added == want_added
    PW.assert_counts(amap, [record], counts)
    total = assert_ledger(amap, [record], counts, ledger)
    assert amap.consensus(0, fill_ref=True) == truth
    ev, b = amap.insertions_fetch(0)
    placer.close()
    amap.close()
    return total, ev.tobytes().hex() + ":" + b.hex()


def case_grow(O, dcn):
    """DCN_INSERTION_LEDGER_EVENTS = 1: the ledger starts at one event and grows with almost every batch"""
    assert os.environ.get("DCN_INSERTION_LEDGER_EVENTS") == "1"
    total, text = _run_truth(O, dcn, 12)
    print("insertions grow %d %d %s" % (total[0], total[1], text))


def case_groups(O, dcn):
    """DCN_ALIGN_TRACE_BYTES as the test set it: several trace groups per call, the same ledger"""
    total, text = _run_truth(O, dcn, 2)
    print("insertions groups %d %d %s" % (total[0], total[1], text))


if __name__ == "__main__":
    import deacon_server_amd as dcn
    from oracle import oracle as O
    O.lib()
    {"grow": case_grow, "groups": case_groups}[sys.argv[1]](O, dcn)
