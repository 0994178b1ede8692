"""CPU: the batches of tests/test_gpu_short_geometry.py hold every case they are there for, by the oracle alone.  Repeated
keys within a read are established from _place_worker.occurrences, which gives the key at each distinct minimizer position
of a read (_depth_worker.occurrences sums over reads and loses the position)."""
import numpy as np
import pytest

import _place_worker as PW
import _short_geometry_cases as GC

LMAX, W = GC.LMAX, GC.W


@pytest.fixture(scope="module", params=GC.KS)
def case(request, oracle):
    k = request.param
    g, src = GC.world(k)
    oidx = oracle.Index.build(list(src), k=k, w=W)
    reads = GC.k_batch(g, k)
    b, o = oracle.concat_reads(reads)
    by_threshold = {t: oracle.filter_batch(oidx, b, o, abs_threshold=t[0], rel_threshold=t[1], deplete=t[2], threads=4)
                    for t in GC.THRESHOLDS}
    return k, g, oidx, reads, o, by_threshold


def raw_hits(oracle, oidx, read, k):
    """minimizer positions of the read with a key of the index, repeated keys counted each time"""
    return sum(1 for h, _ in PW.occurrences(oracle, read, k, W) if h in oidx)


def test_shape_of_the_batch(oracle, case):
    k, g, oidx, reads, o, _ = case
    # the case can tell: the first read with the bytes in front of the stream, and the last one with those behind it, taken
    # for bases have other minimizers or other hits than the reads alone
    for shift in (9, 15):
        front, back = GC.outside(k, shift)
        for alone, leaked in ((reads[0], front + reads[0]), (reads[-1], reads[-1] + back)):
            a, b = ([h for h, _ in PW.occurrences(oracle, r, k, W)] for r in (alone, leaked))
            assert (len(a), len({h for h in a if h in oidx})) != (len(b), len({h for h in b if h in oidx})), (k, shift)
    assert len(reads) == GC.N_READS and len(reads) % 64 not in (0, 63) and max(len(r) for r in reads) == LMAX
    assert reads[0] == g[GC.front_at(k):GC.front_at(k) + LMAX] and reads[-1] == g[GC.BACK_END - len(reads[-1]):GC.BACK_END]
    front, back = GC.outside(k, 9)
    assert len(front) == 9 and len(back) == 64 and front + reads[0] + b"" == g[GC.front_at(k) - 9:GC.front_at(k) + LMAX]
    assert reads[-1] + back == g[GC.BACK_END - len(reads[-1]):GC.BACK_END + 64]


def test_length_edges_and_their_totals(case):
    k, g, oidx, reads, o, by_threshold = case
    l = GC.ell(k)
    _, hits, total = by_threshold[GC.THRESHOLDS[0]]
    want_bases = {"0": 0, "k-1": k - 1, "k": k, "l-1": l - 1, "l": l, "l+1": l + 1}
    seen = set()
    for pos, name, bases, nl in GC.edge_slots(k):
        r = reads[pos]
        assert r.endswith(b"\n") == nl and len(r) == bases + nl and b"\n" not in r[:-1], (pos, name)
        if name.startswith("LMAX"):
            assert len(r) == LMAX and total[pos] > 0
        else:
            assert bases == want_bases[name.replace("+nl", "")]
            assert total[pos] == max(0, bases - l + 1) and total[pos] == {l: 1, l + 1: 2}.get(bases, 0), (pos, name)
        seen.add((name, pos % 64))
    names = {n for n, _, _ in GC.length_kinds(k)}
    assert names == {"0", "k-1", "k", "l-1", "l", "l+1", "0+nl", "k-1+nl", "k+nl", "l-1+nl", "l+nl", "l+1+nl", "LMAX", "LMAX-1+nl"}
    for name in names:  # every kind at a wave's first and at a wave's last lane
        assert (name, 0) in seen and (name, 63) in seen, name
    assert len({p for p, _, _, _ in GC.edge_slots(k)}) == 2 * GC.N_KINDS


def test_ordinary_reads(case):
    k, g, oidx, reads, o, _ = case
    l = GC.ell(k)
    special = {p for p, _, _, _ in GC.edge_slots(k)} | {GC.POLY_A, GC.AC_REPEAT, GC.COPY, GC.ENDS_IN_HIT, GC.STARTS_WITH_HIT,
                                                      len(reads) - 1}
    if k in GC.LEAK_KS:
        special |= {GC.LEAK_NEIGHBOUR, GC.LEAK_READ}
    rest = [r for i, r in enumerate(reads) if i not in special]
    lens = {len(r) for r in rest}
    assert min(lens) == l + 1 and max(lens) == LMAX and len(rest) > 850
    assert any(r[:1] == b"N" for r in rest) and any(r[-1:] == b"N" for r in rest)
    assert any(r[:2].islower() for r in rest) and any(r[-2:].islower() for r in rest)
    if k == 1:
        assert sum(set(r.upper()) <= set(b"ATN") for r in rest) > 100


def test_decisions_hits_and_flushes(oracle, case):
    k, g, oidx, reads, o, by_threshold = case
    mixed = []
    for t, (keep, hits, total) in by_threshold.items():
        win = total > 0
        mixed.append(bool(keep[win].any() and not keep[win].all()))
    assert any(mixed), "no threshold triple with both decisions"
    _, hits, total = by_threshold[GC.THRESHOLDS[0]]
    # hits range from 0 to total (k = 1: both keys are in the index, so only a read without a minimizer has no hit)
    assert (hits == 0).any() and (hits[total > 0] == total[total > 0]).any()
    assert k == 1 or (hits[total > 0] == 0).any()
    over = total > GC.LCAP_FLUSH
    print(f"k={k}: total mean {total[total > 0].mean():.1f} max {total.max()}, reads past {GC.LCAP_FLUSH} entries: {int(over.sum())},"
          f" waves with one: {len({i // 64 for i in np.flatnonzero(over)})} of {(len(reads) + 63) // 64}, keys {len(oidx)},"
          f" keep fraction {[round(float(v[0][v[2] > 0].mean()), 2) for v in by_threshold.values()]}")
    if k in (1, 3):  # a mid-scan flush in a wave where many lanes carry hits
        assert any(over[w0:w0 + 64].any() and (hits[w0:w0 + 64] > 0).sum() >= 8 for w0 in range(0, len(reads), 64))
    if k == 1:
        assert len(oidx) == 2  # both canonical 1-mers
        long_enough = np.array([len(r) >= 100 for r in reads])
        assert (total[long_enough] > (LMAX >> 2) + 1).all()
        assert (hits == 2).any() and (hits[total > 0] == 1).any()
    if k == 5:
        assert ((hits > 0) & (hits < total)).any()
        occ = [[h for h, _ in PW.occurrences(oracle, r, k, W)] for r in reads]
        assert sum(len(set(h)) < len(h) for h in occ) > len(reads) // 4, "repeated keys within a read are ordinary at k = 5"
        assert any(len([x for x in h if x in oidx]) > len({x for x in h if x in oidx}) for h in occ), "a repeated key that hits"
    # which k need one slot of the record array per window: a read's hits against a run of one slot per four bases
    outgrown = [i for i, r in enumerate(reads) if raw_hits(oracle, oidx, r, k) > GC.run_cap(int(o[i]), len(r))]
    if k == 1:
        assert len(outgrown) > len(reads) // 2
    if k not in GC.ONE_SLOT_PER_WINDOW:
        assert not outgrown, outgrown


def test_special_reads(oracle, case):
    k, g, oidx, reads, o, by_threshold = case
    _, hits, total = by_threshold[GC.THRESHOLDS[0]]
    assert reads[GC.POLY_A] == b"A" * LMAX and reads[GC.AC_REPEAT] == (b"AC" * LMAX)[:LMAX]
    assert total[GC.POLY_A] == LMAX - GC.ell(k) + 1  # a minimizer in every window
    assert reads[GC.COPY] == g[1000:1000 + LMAX] and hits[GC.COPY] > 0
    if k >= 13:
        assert hits[GC.COPY] == total[GC.COPY]
    for pos, last in ((GC.ENDS_IN_HIT, True), (GC.STARTS_WITH_HIT, False)):
        r = reads[pos]
        occ = PW.occurrences(oracle, r, k, W)
        at = len(r) - k if last else 0
        assert [h for h, p in occ if p == at and h in oidx], (pos, at)
        assert r in g and GC.ell(k) < len(r) <= LMAX
    if k in GC.LEAK_KS:
        nb, r = reads[GC.LEAK_NEIGHBOUR], reads[GC.LEAK_READ]
        assert GC.LEAK_READ == GC.LEAK_NEIGHBOUR + 1 and GC.LEAK_READ % 64 != 0  # the same wave: one staged span
        assert total[GC.LEAK_READ] > 0 and hits[GC.LEAK_READ] == 0
        tail = nb[-(W - 1):]
        assert len(tail) == 14 and any(GC.kmer_key(tail[i:i + k]) in oidx for i in range(len(tail) - k + 1))
        assert raw_hits(oracle, oidx, tail + r, k) > 0  # the case can tell: the lead-in scanned as part of r gives r a hit


@pytest.mark.parametrize("k", [GC.SC.K, 5])
def test_full_wave_batches(oracle, k):
    g, src = GC.world(k)
    oidx = oracle.Index.build(list(src), k=k, w=W)
    counts = {}
    for j in range(16):
        reads = GC.full_wave_batch(g, j, k)
        b, o = oracle.concat_reads(reads)
        assert len(reads) == 138 and [len(r) for r in reads[:63]] == [LMAX] * 63 and len(reads[63]) == LMAX - j
        assert [len(r) for r in reads[64:128]] == [LMAX] * 64
        assert int(o[64]) == 64 * LMAX - j and int(o[128]) - int(o[64]) == 64 * LMAX
        occ = PW.occurrences(oracle, reads[127], k, W)
        assert occ[-1][1] == LMAX - k and occ[-1][0] in oidx  # wave 1's last read ends in a hit
        keep, hits, total = oracle.filter_batch(oidx, b, o, threads=4)
        assert keep.any() and not keep.all()
        for shift in (0, 15):
            a16 = shift % 16
            first, _ = GC.short_lane_chunks(int(o[64]), int(o[65]), a16)
            _, last = GC.short_lane_chunks(int(o[127]), int(o[128]), a16)
            counts[(a16 + int(o[64])) % 16] = last - first + 1
        assert GC.short_lane_chunks(0, int(o[1]), 0)[0] == -1  # the batch's first wave: its lead-in lies in front of the stream
    assert sorted(counts) == list(range(16))  # wave 1's first base at every position inside a chunk
    assert max(counts.values()) == 610 <= GC.STAGE_WORDS and min(counts.values()) >= 609


def test_alternate_plan(oracle):
    k = 5
    g, src = GC.world(k)
    oidx = oracle.Index.build(list(src), k=k, w=W)
    plan = GC.alternate_plan(g, k)
    assert [s for _, _, s in plan] == [True, False, True, False, True]
    for reads, uid, short in plan:
        assert (max(len(r) for r in reads) <= LMAX and uid is None) is short
        b, o = oracle.concat_reads(reads)
        keep, hits, total = oracle.filter_batch(oidx, b, o, uid, threads=4)
        assert keep.any() and not keep.all()
        # no run of the record array is outgrown at one slot per four bases: no batch comes back with a capacity error
        assert all(raw_hits(oracle, oidx, r, k) <= GC.run_cap(int(o[i]), len(r)) for i, r in enumerate(reads))
    assert len(plan[4][0]) == 129 and len(plan[3][0]) % 2 == 0
