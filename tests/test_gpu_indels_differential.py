"""The deletion ledger and the indel genotype on a few hundred reads with planted indels, against the model of
tests/_indel_worker.py: two haplotypes over the two short records of tests/test_gpu_pileup_seams.py, indels of 1 - 5 bases at
twenty positions, in both haplotypes at some and in one at the others, reads of 100 - 250 bases from either on both
strands with a mismatch in a hundred bases and random qualities, of which those under 15 count as N.  The input is cut into
1, 2 and 7 calls; counters, both ledgers and the sites under three parameter settings are compared exactly."""
import numpy as np
import pytest

import _indel_worker as DW
import _insertion_worker as IW
import _pileup_worker as PW
import _verify_worker as VW
from conftest import revcomp
from test_gpu_pileup_seams import make_records, other

pytestmark = pytest.mark.gpu

SEED = 2121  # (checked with the model alone: test_the_model_alone_finds_what_was_planted)
# (record, position, kind, length, in both haplotypes): apart from each other, from the homopolymer and from the N bases
PLAN = [(0, 400, "D", 2, True), (0, 700, "I", 3, False), (0, 1000, "D", 1, False), (0, 1600, "I", 1, True), (0, 1900, "I", 2, True),
        (0, 2100, "D", 5, True), (0, 2300, "I", 3, False), (0, 2500, "I", 4, False), (0, 2900, "D", 3, False), (0, 3100, "I", 1, True),
        (0, 3300, "I", 2, True), (0, 3600, "D", 4, False), (0, 3800, "I", 2, False),
        (1, 350, "D", 2, False), (1, 600, "I", 5, True), (1, 750, "I", 2, False), (1, 900, "D", 3, True), (1, 1050, "I", 3, True),
        (1, 1200, "I", 2, False), (1, 1400, "D", 1, True)]
SETTINGS = (DW.DEFAULTS, dict(ploidy=1, min_depth=5, min_gq=30, min_qual=30, min_count=3, indel_centi=1500),
            dict(min_depth=1, min_gq=0, min_qual=0, min_count=1, indel_centi=500, het_centi=700))
MIN_BASE_QUAL = 15


def haplotype(record, R, both_only):
    """-> (bases, per base the record position it stands for: an inserted base stands for the base in front of it)"""
    out, ref_of, at = bytearray(), [], 0
    for rec, p, kind, ln, both in sorted(PLAN):
        if rec != R or (both_only and not both):
            continue
        out += record[at:p]
        ref_of += range(at, p)
        at = p
        if kind == "D":
            at = p + ln
        else:  # behind base p - 1
            out += other(record[p - 1:p], record[p:p + 1]) * ln
            ref_of += [p - 1] * ln
    out += record[at:]
    ref_of += range(at, len(record))
    return bytes(out), ref_of


def planted(seed=SEED, n_reads=600):
    rng = np.random.default_rng(seed)
    records = make_records()
    haps = [[haplotype(rec, R, both_only) for both_only in (False, True)] for R, rec in enumerate(records)]
    reads, quals, rows = [], [], []
    for i in range(n_reads):
        R = int(rng.random() < 0.3)
        seq, ref_of = haps[R][int(rng.integers(0, 2))]
        ln = int(rng.integers(100, 251))
        s = int(rng.integers(0, len(seq) - ln + 1))
        a, b = ref_of[s], ref_of[s + ln - 1] + 1
        if s > 0 and ref_of[s] == ref_of[s - 1]:
            a += 1  # the read begins inside an insertion: its first record base is the next one
        piece = bytearray(seq[s:s + ln])
        for x in np.flatnonzero(rng.random(ln) < 0.01):
            piece[x] = other(bytes(piece[x:x + 1]))[0]
        rev, pre = i & 1, int(rng.integers(0, 30))
        flank = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), pre))
        body = revcomp(bytes(piece)) if rev else bytes(piece)
        reads.append(flank + body)
        quals.append(bytes((rng.integers(5, 42, pre + ln) + 33).astype(np.uint8)))
        row = np.zeros(1, IW.ROW)
        row["record"], row["reverse"], row["read_start"], row["read_end"], row["ref_start"], row["ref_end"] = R, rev, pre, pre + ln, a, b
        rows.append(row)
    return records, reads, quals, np.concatenate(rows)


def piled_by_the_model(seed=SEED):
    """the planted input through the model alone (no device) -> what the tests compare the device with"""
    records, reads, quals, rows = planted(seed)
    counts, ins, dels = PW.new_counts(records), IW.new_ledger(records), DW.new_ledger(records)
    edits, n_added = DW.pile_rows(counts, ins, dels, reads, records, rows, quals=quals, min_base_qual=MIN_BASE_QUAL)
    return records, reads, quals, rows, counts, ins, dels, edits, n_added


def assert_planted(truth):
    """The condition on the seed, asserted on the model's own output: tests/test_indels_abi.py checks it without a device, and
    the fixture below before the device is asked, so that it cannot hide a failure."""
    records, reads, quals, rows, counts, ins, dels, edits, n_added = truth
    assert n_added >= 580
    sites = [s for R, rec in enumerate(records) for s in DW.sites_range(counts[R], ins[R], dels[R], 0, len(rec))]
    n_del = sum(1 for s in sites if s[1] & DW.INDEL_DELETION)
    assert n_del >= 8 and len(sites) - n_del >= 8, (n_del, len(sites))
    assert sum(s[8] == 1 for s in sites) >= 3 and sum(s[8] == 2 for s in sites) >= 3
    assert sum(int(c[:, PW.N].sum()) for c in counts) > 1000  # bases of low quality count as N


@pytest.fixture(scope="module")
def truth():
    out = piled_by_the_model()
    assert_planted(out)
    return out


@pytest.mark.parametrize("calls", [1, 2, 7])
def test_ledgers_and_sites_against_the_model(dcn, oracle, truth, calls):
    records, reads, quals, rows, counts, ins, dels, edits, n_added = truth
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    amap.pileup_keep_deletions()
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    dev_rows = IW.rows_as(dcn.filter.PLACEMENT_DTYPE, rows)
    cuts = np.linspace(0, len(reads), calls + 1).astype(int)
    got_edits, added = [], 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        b, o = oracle.concat_reads(reads[lo:hi])
        e, n = placer.pileup_batch(b, o, dev_rows[lo:hi], quals=np.frombuffer(b"".join(quals[lo:hi]), np.uint8), min_base_qual=MIN_BASE_QUAL)
        got_edits += e.tolist()
        added += n
    assert got_edits == edits.tolist() and added == n_added
    PW.assert_counts(amap, records, counts)
    DW.assert_ledgers(amap, records, counts, ins, dels, settings=SETTINGS)
    placer.close()
    amap.close()
