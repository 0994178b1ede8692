"""The model of tests/test_indels_abi.py and tests/test_gpu_indels*.py, and the worker of their subprocess cases.

THE DEFINITION OF A DELETION LEDGER and THE DEFINITION OF AN INDEL GENOTYPE (include/deacon_hip.h), written as they read.
The runs of a row come from tests/_align_worker.py's table and walk, the counters from tests/_pileup_worker.py's add_runs,
the insertion events from tests/_insertion_worker.py's events_of_runs; deletion_events_of_runs() follows the same runs one at
a time and collects rule R2's events (p, len, reverse) into a Python list: never from the device.  R4 is sorted() over the
tuples, R5 and L5 a Counter each, decide() rules I2 - I5 in Python integers as a loop over the genotypes, sites_range() rules
I1 and I6 position by position, vcf_text() the tool's file on top of tests/_genotype_worker.py's.  Nothing here is shared
with csrc/dcn_indels.h: no buckets, no scans, no lanes.

As a program (python tests/_indel_worker.py CASE) it runs one case in a process of its own, whose environment the test has
set, and exits non-zero with a traceback when a check fails."""
import os
import sys
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _align_worker as AW  # noqa: E402
import _genotype_worker as GW  # noqa: E402
import _insertion_worker as IW  # noqa: E402
import _pileup_worker as PW  # noqa: E402
import _quality_worker as QW  # noqa: E402
import _verify_worker as VW  # noqa: E402
from _verify_worker import OVER, UNPLACED, intervals  # noqa: E402

DELETION_REVERSE = 1
INDEL_DELETION, INDEL_FRONT = 1, 2
DEFAULTS = dict(ploidy=2, min_depth=3, min_gq=20, min_qual=20, min_count=2, indel_centi=2000, het_centi=301)


# ---- the deletion ledger ---------------------------------------------------------------------------------------------
def deletion_events_of_runs(ref_start, reverse, runs):
    """rule R2: the events of one row's runs, one run at a time"""
    j = 0
    out = []
    for x in runs:
        ln, op = int(x) >> 4, int(x) & 15
        if op == AW.OP_D:
            out.append((ref_start + j, ln, int(reverse)))
        if op != AW.OP_I:
            j += ln
    return out


def new_ledger(records):
    return [[] for _ in records]


def pile_rows(counts, insertions, deletions, reads, records, rows, row_offsets=None, max_edits=VW.MAX_EDITS, max_permille=200, select=None,
              quals=None, min_base_qual=0, qual_offset=33):
    """the model of dcn_pileup_batch on a map that keeps both ledgers: the counters, rule L2's events and rule R2's events of
    every row that adds (each ledger: one list per record) -> (edits, n_added).  quals (one bytes per read): the model of
    dcn_pileup_batch_qual, whose counters take a base under min_base_qual as N (rule Q3); the ledgers do not look at them"""
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
            continue  # rule P2: n = 0 adds nothing, to either ledger
        runs = cigar[int(offs[r]):int(offs[r + 1])]
        ref_start, reverse = int(rows["ref_start"][r]), int(rows["reverse"][r])
        counted = S if quals is None else QW.masked(S, QW.qualities_of_S(quals[owner[r]], rows[r], qual_offset), min_base_qual)
        assert PW.add_runs(counts[R], counted, ref_start, reverse, runs) == (len(S), len(Tt))
        insertions[R] += IW.events_of_runs(S, ref_start, reverse, runs)
        deletions[R] += deletion_events_of_runs(ref_start, reverse, runs)
        n_added += 1
    return edits, n_added


def fetch_range(events, start, n):
    """the model of dcn_anchor_map_deletions_fetch: by p alone; rule R4 is the order of the tuples"""
    return sorted(e for e in events if start <= e[0] < start + n)


def deletion_winner(events_at_p):
    """rule R5 -> (len, count)"""
    tally = Counter(e[1] for e in events_at_p)
    ln = min(tally, key=lambda x: (-tally[x], x))
    return ln, tally[ln]


def assert_r2(counts, events, length):
    """rule R2's two invariants against the DEL column of one record"""
    cover = np.zeros(length + 1, np.int64)
    for p, ln, _ in events:
        assert 0 <= p and p + ln <= length and ln >= 1
        cover[p] += 1
        cover[p + ln] -= 1
    assert np.array_equal(np.cumsum(cover)[:length], np.asarray(counts)[:, PW.DEL])
    assert sum(e[1] for e in events) == int(np.asarray(counts)[:, PW.DEL].sum())


def deletions_as_tuples(events):
    return [(int(e["pos"]), int(e["len"]), int(e["flags"]) & DELETION_REVERSE) for e in events if int(e["flags"]) & ~DELETION_REVERSE == 0]


# ---- the indel genotype ----------------------------------------------------------------------------------------------
def genotypes(ploidy):
    """rule I3's order, 0 = R and 1 = V"""
    return [(0,), (1,)] if ploidy == 1 else [(0, 0), (0, 1), (1, 1)]


def costs(a, o, ploidy=2, indel_centi=2000, het_centi=301):
    """rule I3: a read that carries the allele contradicts R, one that does not contradicts V"""
    out = []
    for g in genotypes(ploidy):
        if len(set(g)) == 2:
            out.append(het_centi * (a + o))
        else:
            out.append(indel_centi * (a if g[0] == 0 else o))
    return out


def decide(a, depth, ploidy=2, min_depth=3, min_gq=20, min_qual=20, min_count=2, indel_centi=2000, het_centi=301):
    """rules I2 - I5 for one candidate that rule I1 has kept -> dict(gt, gq, qual, site, pl (three entries), costs)"""
    o = depth - a if depth >= a else 0
    cost = costs(a, o, ploidy, indel_centi, het_centi)
    best = min(range(len(cost)), key=lambda g: (cost[g], g))
    second = min(cost[g] for g in range(len(cost)) if g != best)
    gq = min(99, (second - cost[best]) // 100)
    pl = [min(255, (c - cost[best]) // 100) for c in cost] + [0] * (3 - len(cost))
    qual = min(2 ** 32 - 1, (cost[0] - cost[best]) // 100)
    called = depth >= max(1, min_depth) and gq >= min_gq
    return dict(gt=best, gq=gq, qual=qual, site=bool(called and best != 0 and qual >= min_qual), pl=pl, costs=cost)


def sites_range(counts, insertions, deletions, start, n, **params):
    """Rules I1 - I6 over [start, start + n) of one record: counts[len(record), 8]; insertions / deletions are the record's
    events, or None for a ledger the map does not keep -> [(pos, flags, len, bases, qual, depth, count, events, gt, gq, pl)]"""
    prm = dict(DEFAULTS, **params)
    ins_at, del_at = {}, {}
    for e in insertions or []:
        ins_at.setdefault(e[0], []).append(e)
    for e in deletions or []:
        del_at.setdefault(e[0], []).append(e)
    out = []
    for p in range(start, start + n):
        depth = sum(int(x) for x in counts[p][:6]) & 0xFFFFFFFF
        here = []  # in I6's order: (rank, flags, len, bases, a, e)
        if insertions is not None and int(counts[p][PW.INS]) > 0:
            assert len(ins_at.get(p, [])) == int(counts[p][PW.INS])  # rule L2
            (front, ln, bases), a = IW.winner(ins_at[p])
            here.append((0 if front else 2, INDEL_FRONT if front else 0, ln, bases, a, int(counts[p][PW.INS])))
        if deletions is not None and p in del_at:
            ln, a = deletion_winner(del_at[p])
            here.append((1, INDEL_DELETION, ln, b"", a, len(del_at[p])))
        for _, flags, ln, bases, a, e in sorted(here):
            if a < max(1, prm["min_count"]):
                continue  # rule I1
            d = decide(a, depth, **prm)
            if d["site"]:
                out.append((p, flags, ln, bases, d["qual"], depth, a, e, d["gt"], d["gq"], tuple(d["pl"])))
    return out


def device_sites(sites, bases):
    """the structured array and the bases of AnchorMap.indels_genotype as the model's tuples: bases_offset ascending and
    dense, a deletion site with the offset reached so far, the reserved bytes 0"""
    assert not sites["reserved"].any()
    out, at = [], 0
    for s in sites:
        assert int(s["bases_offset"]) == at
        is_del = bool(int(s["flags"]) & INDEL_DELETION)
        mine = b"" if is_del else bases[at:at + int(s["len"])]
        at += len(mine)
        out.append((int(s["pos"]), int(s["flags"]), int(s["len"]), mine, int(s["qual"]), int(s["depth"]), int(s["count"]), int(s["events"]),
                    int(s["gt"]), int(s["gq"]), tuple(int(x) for x in s["pl"])))
    assert at == len(bases)
    return out


def assert_sites(amap, counts, insertions, deletions, R, start=0, n=None, length=None, **params):
    """AnchorMap.indels_genotype over a range against the model, the first difference named -> the model's sites"""
    n = length - start if n is None else n
    want = sites_range(counts, insertions, deletions, start, n, **params)
    sites, bases = amap.indels_genotype(R, start, n, **params)
    got = device_sites(sites, bases)
    if got != want:
        k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
        raise AssertionError(("site", k, "of", len(got), len(want), "got", got[k:k + 1], "want", want[k:k + 1], (R, start, n), params))
    return want


def assert_ledgers(amap, records, counts, insertions, deletions, settings=(DEFAULTS,)):
    """both ledgers and the sites of a map against the model, over whole records"""
    total = [0, 0]
    for R, rec in enumerate(records):
        got, want = deletions_as_tuples(amap.deletions_fetch(R)), fetch_range(deletions[R], 0, len(rec))
        assert got == want, ("deletions", R, [x for x in got if x not in want][:3], [x for x in want if x not in got][:3])
        assert_r2(counts[R], want, len(rec))
        total[0] += len(want)
        total[1] += sum(e[1] for e in want)
        if insertions is not None:
            ev, b = amap.insertions_fetch(R)
            assert IW.events_as_tuples(ev, b) == IW.fetch_range(insertions[R], 0, len(rec)), ("insertions", R)
        for params in settings:
            assert_sites(amap, counts[R], None if insertions is None else insertions[R], deletions[R], R, length=len(rec), **params)
    assert amap.deletions_info() == tuple(total)
    return total


# ---- VCF -------------------------------------------------------------------------------------------------------------
VCF_INDEL_HEADER = ['##INFO=<ID=INDEL,Number=0,Type=Flag,Description="An insertion or a deletion">',
                    '##INFO=<ID=IDV,Number=1,Type=Integer,Description="Reads that carry the allele">',
                    '##INFO=<ID=IEV,Number=1,Type=Integer,Description="Insertions behind, or deletions that begin at, the position, of any allele">']


def indel_alleles(ref, site):
    """rule of the tool: ref = the record as dcn_anchor_map_fetch gives it -> (POS, REF, ALT)"""
    p, flags, ln, bases = site[:4]
    ref, bases = ref.decode(), bases.decode()
    if flags & INDEL_DELETION:
        if p > 0:
            return p, ref[p - 1:p + ln], ref[p - 1]
        assert ln < len(ref)  # (a deletion of a whole record is not a line)
        return 1, ref[0:ln + 1], ref[ln]
    if flags & INDEL_FRONT:
        if p > 0:
            return p, ref[p - 1], ref[p - 1] + bases
        return 1, ref[0], bases + ref[0]
    return p + 1, ref[p], ref[p] + bases


def indel_line(name, ref, site, ploidy):
    pos, ref_allele, alt = indel_alleles(ref, site)
    _, _, _, _, qual, depth, a, e, gt, gq, pl = site
    o = depth - a if depth >= a else 0
    gt_text = "1" if ploidy == 1 else ("0/1" if gt == 1 else "1/1")
    sample = ":".join([gt_text, str(gq), str(o + a), "%d,%d" % (o, a), ",".join(str(x) for x in pl[:ploidy + 1])])
    return pos, "\t".join([name, str(pos), ".", ref_allele, alt, str(qual), "PASS", "INDEL;DP=%d;IDV=%d;IEV=%d" % (depth, a, e), "GT:GQ:DP:AD:PL", sample])


def vcf_text(version, names_, records, snv_sites_per_record, indel_sites_per_record, ploidy=2, sample="sample"):
    """The whole file of `deacon-hip indels`: tests/_genotype_worker.py's header with the three lines behind INFO DP; per
    record the lines in non-descending POS, at one POS the SNV line first, then the indel lines in I6's order."""
    head = GW.vcf_header(version, [(nm, len(rec)) for nm, rec in zip(names_, records)], sample)
    at = next(i for i, line in enumerate(head) if line.startswith("##INFO=<ID=DP,")) + 1
    lines = head[:at] + VCF_INDEL_HEADER + head[at:]
    for nm, rec, snvs, indels in zip(names_, records, snv_sites_per_record, indel_sites_per_record):
        ref = VW.fetched_text(rec)
        keyed = [((s[0] + 1, 0), GW.vcf_line(nm, s, ploidy)) for s in snvs]
        for s in indels:
            pos, line = indel_line(nm, ref, s, ploidy)
            keyed.append(((pos, 1), line))
        lines += [line for _, line in sorted(keyed, key=lambda kl: kl[0])]  # (stable: I6's order at one POS)
    return "\n".join(lines) + "\n"


# ---- the subprocess cases --------------------------------------------------------------------------------------------
def _run_truth(O, dcn, batches):
    """tests/_insertion_worker.py's end-to-end case (a substitution, a 2-base deletion, a 3-base insertion under error-free
    reads) on a map that keeps both ledgers, cut into `batches` calls"""
    record, truth, reads, rows = IW.truth_case()
    amap = VW.build_map(O, dcn, [record])
    amap.pileup_enable()
    amap.pileup_keep_insertions()
    amap.pileup_keep_deletions()
    placer = dcn.Placer(amap, max_batch_bases=1 << 16, max_batch_reads=1 << 10)
    rows = IW.rows_as(dcn.filter.PLACEMENT_DTYPE, rows)
    counts, ins, dels = PW.new_counts([record]), IW.new_ledger([record]), new_ledger([record])
    cuts = np.linspace(0, len(reads), batches + 1).astype(int)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        b, o = O.concat_reads(reads[lo:hi])
        edits, n_added = placer.pileup_batch(b, o, rows[lo:hi])
        want_edits, want_added = pile_rows(counts, ins, dels, reads[lo:hi], [record], rows[lo:hi])
        assert edits.tolist() == want_edits.tolist() and n_added == want_added
    PW.assert_counts(amap, [record], counts)
    total = assert_ledgers(amap, [record], counts, ins, dels)
    sites = sites_range(counts[0], ins[0], dels[0], 0, len(record))
    assert [(s[0], s[1], s[2], s[8]) for s in sites] == [(300, INDEL_DELETION, 2, 2), (449, 0, 3, 2)]  # both homozygous
    ev = amap.deletions_fetch(0)
    st, b = amap.indels_genotype(0)
    placer.close()
    amap.close()
    return total, ev.tobytes().hex() + ":" + st.tobytes().hex() + ":" + b.hex()


def case_grow(O, dcn):
    """DCN_DELETION_LEDGER_EVENTS = 1: the ledger starts at one event and grows with almost every batch"""
    assert os.environ.get("DCN_DELETION_LEDGER_EVENTS") == "1"
    total, text = _run_truth(O, dcn, 12)
    print("indels grow %d %d %s" % (total[0], total[1], text))


def case_groups(O, dcn):
    """DCN_ALIGN_TRACE_BYTES as the test set it: several trace groups per call, the same ledger"""
    total, text = _run_truth(O, dcn, 2)
    print("indels groups %d %d %s" % (total[0], total[1], text))


def case_trips(O, dcn):
    """DCN_GRID_CUS = 1 as the test set it: a few hundred rows, so that the append's work loop makes a second trip"""
    assert os.environ.get("DCN_GRID_CUS") == "1"
    from test_gpu_pileup_seams import Case, make_records
    records = make_records()
    amap = VW.build_map(O, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_deletions()
    placer = dcn.Placer(amap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
    c = Case(dcn, records, 91)
    for q in range(300):  # (one CU: 32 workgroups of four waves = 128 rows a trip)
        a = (53 * q) % (len(records[1]) - 80)
        T = records[1][a:a + 80]
        c.put(T[:30 + q % 9] + T[30 + q % 9 + 1 + q % 3:] if q % 4 else T, 1, a, a + 80, rev=q % 2)
    rows = np.concatenate(c.rows)
    b, o = O.concat_reads(c.reads)
    edits, n_added = placer.pileup_batch(b, o, rows)
    counts, dels = PW.new_counts(records), new_ledger(records)
    want_edits, want_added = pile_rows(counts, IW.new_ledger(records), dels, c.reads, records, rows)
    assert edits.tolist() == want_edits.tolist() and n_added == want_added == 300
    PW.assert_counts(amap, records, counts)
    total = assert_ledgers(amap, records, counts, None, dels)
    assert total[0] >= 200
    placer.close()
    amap.close()
    print("indels trips %d %d" % tuple(total))


if __name__ == "__main__":
    import deacon_server_amd as dcn
    from oracle import oracle as O
    O.lib()
    {"grow": case_grow, "groups": case_groups, "trips": case_trips}[sys.argv[1]](O, dcn)
