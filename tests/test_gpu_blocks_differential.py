"""Reference blocks against the model of tests/_blocks_worker.py on rows that the placement calls return: the mutated reads
of tests/test_gpu_align.py with random qualities through Placer (place_split_batch, extend_batch, the quality pile-up at
min_base_qual 20 on a map that keeps both ledgers), the counters and sums compared with the CPU pile-up first.  Then whole
records and random cuts of up to 3,000 positions, each with random parameters, random GQ edges and breaks taken from the record's indel sites, cls and
every block; and every cut's halves, merged by dcn_reference_blocks_merge, against the whole.  Every comparison is exact.

What the input is good for is asserted from the model, so that a run cannot pass vacuously: the trials see no coverage,
positions that are not called, breaks, reference blocks of more than one band, blocks of hundreds of positions, and breaks
between two blocks of one class."""
import numpy as np
import pytest

import _blocks_worker as BW
import _insertion_worker as IW
import _pileup_worker as PW
import _quality_worker as QW
import _verify_worker as VW
from test_gpu_align import make_reads, make_records

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def piled(dcn, oracle):
    records = make_records()
    reads = make_reads(records)
    quals = QW.random_quals(np.random.default_rng(2421), reads, lo=10, hi=41)
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    amap.pileup_keep_qualities()
    amap.pileup_keep_deletions()
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    b, o, q = QW.concat(oracle, reads, quals)
    po, srows, _ = placer.place_split_batch(b, o, max_placements=4)
    xrows, _ = placer.extend_batch(b, o, srows, row_offsets=po)
    edits, n_added = placer.pileup_batch(b, o, xrows, row_offsets=po, quals=q, min_base_qual=20)
    counts, sums, ledger = PW.new_counts(records), QW.new_sums(records), IW.new_ledger(records)
    want_edits, want_added = QW.pile_rows(counts, sums, ledger, reads, quals, records, xrows, row_offsets=po, min_base_qual=20)
    assert edits.tolist() == want_edits.tolist() and n_added == want_added > 60
    PW.assert_counts(amap, records, counts)
    QW.assert_sums(amap, records, sums)
    yield dcn, records, amap, counts, sums
    placer.close()
    amap.close()


def random_params(rng):
    edges, e = [], int(rng.integers(1, 30))
    while e <= 99 and len(edges) < 15:
        edges.append(e)
        e += int(rng.integers(1, 30))
    if rng.integers(0, 6) == 0:
        edges = []
    prm = dict(ploidy=int(rng.integers(1, 3)), min_depth=int(rng.integers(0, 5)), min_gq=int(rng.choice([0, 0, 3, 10, 20])),
               min_qual=int(rng.choice([0, 20, 60])), err_centi=int(rng.choice([477, 477, 100, 2000])), het_centi=int(rng.choice([301, 301, 0, 900])))
    return tuple(edges), prm


def test_whole_records_and_random_cuts(piled):
    dcn, records, amap, counts, sums = piled
    rng = np.random.default_rng(2422)
    seen, lengths, split = set(), set(), 0
    for R, record in enumerate(records):
        sites, _ = amap.indels_genotype(R, min_depth=0, min_gq=0, min_qual=0, min_count=1)
        indel_pos = sorted({int(s["pos"]) for s in sites})
        for trial in range(6):
            edges, prm = random_params(rng)
            if trial == 0:  # the whole record, haploid and loose: a single base is a reference call, its GQ its quality and a little
                start, n = 0, len(record)
                edges, prm = BW.DEFAULT_EDGES, dict(ploidy=1, min_depth=1, min_gq=0, min_qual=20, err_centi=477, het_centi=301)
            else:
                start = int(rng.integers(0, len(record)))
                n = int(rng.integers(1, min(3000, len(record) - start) + 1))
            breaks = [p for p in indel_pos if start <= p < start + n]
            breaks = breaks + breaks[:2] if trial % 2 else breaks[::-1]  # duplicated, or descending
            cls, blocks = BW.assert_range(amap, counts[R], sums[R], record, R, start, n, breaks, edges, **prm)
            split += sum(1 for p in set(breaks) if 0 < p - start < n - 1 and cls[p - start - 1] == cls[p - start + 1] != BW.VARIANT)
            seen |= set(cls.tolist())
            lengths |= {b[1] for b in blocks}
            # rule B7 through the library's merge, at a random cut
            m = start + int(rng.integers(0, n + 1))
            halves = []
            for a, b in ((start, m), (m, start + n)):
                halves.append(amap.reference_blocks(R, a, b - a, breaks=[p for p in breaks if a <= p < b], gq_edges=edges, **prm)[1])
            assert BW.device_blocks(dcn.merge_blocks(np.concatenate(halves))) == blocks, (R, start, n, m)
    print("classes seen:", sorted(seen), "longest block:", max(lengths), "breaks that split a block:", split)
    assert {BW.NO_COVERAGE, BW.UNCALLED, BW.VARIANT} <= seen and len([c for c in seen if BW.REF <= c < BW.VARIANT]) >= 2
    assert max(lengths) >= 100 and split >= 1
