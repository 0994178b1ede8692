"""Left-aligned indels on a few hundred reads with planted indels, against the model of tests/_left_align_worker.py: two
haplotypes over the two short records of tests/test_gpu_pileup_seams.py, into which homopolymers and tandem repeats are
written first; twenty-two indels, fourteen of them a unit of such a repeat (planted at the repeat's FAR end, where rule A3
also leaves them), three with a planted SNV two bases behind the repeat; reads of 100 - 150 bases from either haplotype on
both strands with a mismatch in a hundred bases and random qualities, of which those under 15 count as N.

assert_planted() is a statement about the model alone: it reports every planted indel at its left-most position, which is
worked out here on the reference (move the allele while the base in front equals its last base), not taken from the model.
tests/test_left_align_abi.py checks it without a device.  Then device == model: counters, both ledgers and the sites under
three settings, compared exactly."""
import numpy as np
import pytest

import _indel_worker as DW
import _insertion_worker as IW
import _left_align_worker as LW
import _pileup_worker as PW
import _verify_worker as VW
from conftest import revcomp
from test_gpu_pileup_seams import make_records, other

pytestmark = pytest.mark.gpu

SEED = 2223  # (checked with the model alone: assert_planted)
# (record, where the repeat is written, the repeat, kind, units of it that go or come, in both haplotypes, an SNV behind the repeat)
REPEATS = [(0, 300, b"T" * 6, "D", 1, True, False), (0, 520, b"G" * 9, "I", 1, False, False), (0, 760, b"CA" * 5, "D", 1, True, True),
           (0, 1010, b"AG" * 4, "I", 1, True, False), (0, 1700, b"ACT" * 4, "D", 1, False, False), (0, 1950, b"GAT" * 3, "I", 1, True, True),
           (0, 2200, b"C" * 5, "D", 2, True, False), (0, 2450, b"TA" * 6, "I", 2, False, False), (0, 2700, b"A" * 12, "D", 3, True, False),
           (0, 3400, b"TTG" * 5, "I", 1, True, False),
           (1, 420, b"C" * 4, "D", 1, True, True), (1, 700, b"GT" * 3, "D", 1, False, False), (1, 980, b"T" * 7, "I", 2, True, False),
           (1, 1300, b"CAG" * 4, "D", 2, True, False)]
# (record, position, kind, length, in both haplotypes): outside repeats, as tests/test_gpu_indels_differential.py plants them
PLAIN = [(0, 1500, "D", 2, True), (0, 2950, "I", 3, False), (0, 3150, "D", 4, True), (0, 3650, "I", 2, True), (0, 3850, "D", 1, False),
         (1, 560, "I", 3, True), (1, 1150, "D", 3, False), (1, 1550, "I", 1, True)]
SETTINGS = (DW.DEFAULTS, dict(ploidy=1, min_depth=5, min_gq=30, min_qual=30, min_count=3, indel_centi=1500),
            dict(min_depth=1, min_gq=0, min_qual=0, min_count=1, indel_centi=500, het_centi=700))
MIN_BASE_QUAL = 15


def records_with_repeats():
    records = [bytearray(r) for r in make_records()]
    for R, at, rep, *_ in REPEATS:
        rec = records[R]
        rec[at:at + len(rep)] = rep
        unit = unit_of(rep)
        rec[at - 1] = other(rep[:1], unit[-1:])[0]  # the repeat begins and ends here
        rec[at + len(rep)] = other(rep[-1:], unit[:1])[0]
    return [bytes(r) for r in records]


def unit_of(rep):
    return next(rep[:u] for u in (1, 2, 3) if rep[:u] * (len(rep) // u) == rep)


def plan(records):
    """every planted event as (record, p, kind, length, both, inserted bases, SNV position or None): a deletion of
    record[p : p + length], an insertion in front of record[p]; a unit of a repeat goes or comes at the repeat's far end"""
    out = []
    for R, at, rep, kind, units, both, snv in REPEATS:
        u = unit_of(rep)
        ln, end = len(u) * units, at + len(rep)
        out.append((R, end - ln if kind == "D" else end, kind, ln, both, u * units if kind == "I" else b"", end + 2 if snv else None))
    for R, p, kind, ln, both in PLAIN:
        rec = records[R]
        out.append((R, p, kind, ln, both, other(rec[p - 1:p], rec[p:p + 1]) * ln if kind == "I" else b"", None))
    return sorted(out)


def leftmost(record, p, kind, ln, bases):
    """the standard normalisation, on the reference alone -> (the site's pos, its bases): a deletion's pos is its first
    base, an insertion's the base it stands behind"""
    ref = VW.fetched_text(record)
    if kind == "D":
        while p > 1 and ref[p - 1] == ref[p + ln - 1] and ref[p - 1:p] != b"N":
            p -= 1
        return p, b""
    while p > 1 and ref[p - 1] == bases[-1] and ref[p - 1:p] != b"N":
        bases = bases[-1:] + bases[:-1]
        p -= 1
    return p - 1, bases


def haplotype(record, R, events, both_only):
    """-> (bases, per base the record position it stands for: an inserted base stands for the base in front of it)"""
    out, ref_of, at = bytearray(), [], 0
    for rec, p, kind, ln, both, bases, snv in events:
        if rec != R or (both_only and not both):
            continue
        out += record[at:p]
        ref_of += range(at, p)
        at = p
        if kind == "D":
            at = p + ln
        else:
            out += bases
            ref_of += [p - 1] * ln
        if snv is not None:
            out += record[at:snv] + other(record[snv:snv + 1])
            ref_of += range(at, snv + 1)
            at = snv + 1
    out += record[at:]
    ref_of += range(at, len(record))
    return bytes(out), ref_of


def planted(seed=SEED, n_reads=700, repeats=True):
    """repeats=False: the records as they were and the indels outside repeats alone (tests/test_gpu_normalize_cli.py)"""
    rng = np.random.default_rng(seed)
    records = records_with_repeats() if repeats else make_records()
    events = [e for e in plan(records) if repeats or ((e[0], e[1]) in {(x[0], x[1]) for x in PLAIN} and
                                                      leftmost(records[e[0]], e[1], e[2], e[3], e[5])[0] == (e[1] if e[2] == "D" else e[1] - 1))]
    haps = [[haplotype(rec, R, events, both_only) for both_only in (False, True)] for R, rec in enumerate(records)]
    reads, quals, rows = [], [], []
    for i in range(n_reads):
        R = int(rng.random() < 0.3)
        seq, ref_of = haps[R][int(rng.integers(0, 2))]
        ln = int(rng.integers(100, 151))
        s = int(rng.integers(0, len(seq) - ln + 1))
        a, b = ref_of[s], ref_of[s + ln - 1] + 1
        if s > 0 and ref_of[s] == ref_of[s - 1]:
            a += 1  # the read begins inside an insertion: its first record base is the next one
        piece = bytearray(seq[s:s + ln])
        for x in np.flatnonzero(rng.random(ln) < (0.01 if repeats else 0.0)):  # (without repeats: no mismatch beside a gap either)
            piece[x] = other(bytes(piece[x:x + 1]))[0]
        rev, pre = i & 1, int(rng.integers(0, 30))
        flank = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), pre))
        body = revcomp(bytes(piece)) if rev else bytes(piece)
        reads.append(flank + body)
        quals.append(bytes((rng.integers(5, 42, pre + ln) + 33).astype(np.uint8)))
        row = np.zeros(1, IW.ROW)
        row["record"], row["reverse"], row["read_start"], row["read_end"], row["ref_start"], row["ref_end"] = R, rev, pre, pre + ln, a, b
        rows.append(row)
    return records, events, reads, quals, np.concatenate(rows)


def piled_by_the_model(seed=SEED):
    """the planted input through the model alone (no device) -> what the tests compare the device with"""
    records, events, reads, quals, rows = planted(seed)
    counts, ins, dels = PW.new_counts(records), IW.new_ledger(records), DW.new_ledger(records)
    edits, n_added, info = LW.pile_rows(counts, ins, dels, reads, records, rows, quals=quals, min_base_qual=MIN_BASE_QUAL)
    return records, events, reads, quals, rows, counts, ins, dels, edits, n_added, info


def expected_sites(records, events):
    """[(record, pos, flags, len, bases)] of every planted indel at its left-most position"""
    out = []
    for R, p, kind, ln, both, bases, snv in events:
        pos, b = leftmost(records[R], p, kind, ln, bases)
        out.append((R, pos, DW.INDEL_DELETION if kind == "D" else 0, ln, b))
    return out


def assert_planted(truth):
    """The condition on the seed and on the generator, asserted on the model's own output: every planted indel is a site at
    its left-most position, and for the indels in repeats that is not where they were planted."""
    records, events, reads, quals, rows, counts, ins, dels, edits, n_added, info = truth
    assert n_added >= 680 and len(events) == 22
    want = expected_sites(records, events)
    moved = [pos != (e[1] if flags else e[1] - 1) for (R, pos, flags, ln, b), e in zip(want, events)]
    in_repeat = [any(R == e[0] and at <= e[1] <= at + len(rep) for R, at, rep, *_ in REPEATS) for e in events]
    assert sum(in_repeat) == len(REPEATS) >= 11 and all(m for m, r in zip(moved, in_repeat) if r)  # at least half sit in a repeat, and must move
    assert sum(1 for e in events if e[6] is not None) == 3
    for R, rec in enumerate(records):
        # (GQ and QUAL are not asked: a read that begins inside a repeat keeps its gap further right, rule N7, and two or three
        # such reads leave a homozygous deletion's GQ under 20; where the allele stands is what is asserted)
        sites = {(s[0], s[1], s[2], s[3]) for s in DW.sites_range(counts[R], ins[R], dels[R], 0, len(rec), min_gq=0, min_qual=0)}
        for r, pos, flags, ln, b in want:
            if r == R:
                assert (pos, flags, ln, b) in sites, ("planted", r, pos, flags, ln, b, sorted(s for s in sites if abs(s[0] - pos) < 20))
    assert info["rows_changed"] >= 100 and info["gaps_shifted"] >= info["rows_changed"] and info["columns_passed"] > info["gaps_shifted"]


@pytest.fixture(scope="module")
def truth():
    out = piled_by_the_model()
    assert_planted(out)
    return out


def test_ledgers_and_sites_against_the_model(dcn, oracle, truth):
    records, events, reads, quals, rows, counts, ins, dels, edits, n_added, info = truth
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    amap.pileup_keep_deletions()
    amap.pileup_left_align()
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    dev_rows = IW.rows_as(dcn.filter.PLACEMENT_DTYPE, rows)
    cuts = np.linspace(0, len(reads), 3).astype(int)
    got_edits, added = [], 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        b, o = oracle.concat_reads(reads[lo:hi])
        e, n = placer.pileup_batch(b, o, dev_rows[lo:hi], quals=np.frombuffer(b"".join(quals[lo:hi]), np.uint8), min_base_qual=MIN_BASE_QUAL)
        got_edits += e.tolist()
        added += n
    assert got_edits == edits.tolist() and added == n_added
    assert amap.pileup_left_align_info() == info
    PW.assert_counts(amap, records, counts)
    DW.assert_ledgers(amap, records, counts, ins, dels, settings=SETTINGS)
    placer.close()
    amap.close()
