"""The model of tests/test_phase_abi.py and tests/test_gpu_phase*.py, and the worker of their subprocess case.

THE DEFINITION OF A PHASE (include/deacon_hip_phase.h), restated over bytes.  The runs of a row come from
tests/_align_worker.py's table and walk (tests/_left_align_worker.py's when the map's switch is on); observe() follows them one
step at a time and notes, at every base of T that is a listed site, what rule H2 sees there; link_rows() then adds rule H3's
pairs of neighbouring sites; solve() is rules H5-H7 as a loop over the list in Python integers.  Nothing here is shared with
csrc/dcn_phase.h: no prefix sums, no lanes, no search, no scan.

As a program (python tests/_phase_worker.py CASE) it runs one case in a process of its own, whose environment the test has
set, and exits non-zero with a traceback when a check fails."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _align_worker as AW  # noqa: E402
import _insertion_worker as IW  # noqa: E402
import _left_align_worker as LW  # noqa: E402
import _pileup_worker as PW  # noqa: E402
import _quality_worker as QW  # noqa: E402
import _verify_worker as VW  # noqa: E402
from _verify_worker import OVER, UNPLACED, intervals  # noqa: E402

NONE = None
HEAD, JOINED = 1, 2


def make_sites(dtype, entries):
    """[(record, pos, a0, a1)] -> PHASE_SITE_DTYPE[]"""
    out = np.zeros(len(entries), dtype)
    for k, (R, pos, a0, a1) in enumerate(entries):
        out[k] = (pos, R, a0, a1, (0, 0))
    return out


def observe(S, ref_start, runs, wanted):
    """rule H2: {record position: column} at the positions of `wanted` inside the row's interval; DEL under a D run"""
    seen = {}
    i, j = 0, 0
    for x in runs:
        ln, op = int(x) >> 4, int(x) & 15
        if op == AW.OP_I:
            i += ln  # inserted bases observe nothing
            continue
        for _ in range(ln):
            p = ref_start + j
            if p in wanted:
                seen[p] = PW.DEL if op == AW.OP_D else PW.column(S[i])
            if op != AW.OP_D:
                i += 1
            j += 1
    return seen


def link_rows(links, sites, reads, records, rows, row_offsets=None, max_edits=VW.MAX_EDITS, max_permille=200, select=None, quals=None,
              min_base_qual=0, qual_offset=33, left_align=False):
    """the model of dcn_phase_batch: adds to links (int64[len(sites), 4]) -> (edits, n_linking, rows counted, link adds)"""
    rows = rows.copy()
    if select is not None:
        rows["record"][~np.asarray(select, bool)] = UNPLACED
    owner = np.arange(len(rows)) if row_offsets is None else np.repeat(np.arange(len(reads)), np.diff(np.asarray(row_offsets, np.int64)))
    if left_align:
        edits, offs, cigar, _ = LW.left_align_rows(reads, records, rows, row_offsets, max_edits, max_permille)
    else:
        edits, offs, cigar = AW.align_rows(reads, records, rows, row_offsets, max_edits, max_permille)
    index = {(int(s["record"]), int(s["pos"])): k for k, s in enumerate(sites)}
    by_record = {}
    for (R, pos) in index:
        by_record.setdefault(R, set()).add(pos)
    n_linking = counted = adds = 0
    for r in range(len(rows)):
        if int(edits[r]) >= OVER:
            continue
        R = int(rows["record"][r])
        S, Tt = intervals(reads[owner[r]], records[R], rows[r])
        if len(Tt) == 0:
            continue  # rule P2: n = 0 is no counted row
        counted += 1
        if quals is not None:
            S = QW.masked(S, QW.qualities_of_S(quals[owner[r]], rows[r], qual_offset), min_base_qual)
        seen = observe(S, int(rows["ref_start"][r]), cigar[int(offs[r]):int(offs[r + 1])], by_record.get(R, ()))
        mine = 0
        for pos, col in seen.items():
            k = index[(R, pos)]
            if k + 1 >= len(sites) or int(sites["record"][k + 1]) != R:
                continue  # rule H3: no link across records
            nxt = seen.get(int(sites["pos"][k + 1]))
            x = allele(col, sites[k])
            y = NONE if nxt is None else allele(nxt, sites[k + 1])
            if x is not NONE and y is not NONE:
                links[k, 2 * x + y] += 1
                mine += 1
        n_linking += mine > 0
        adds += mine
    return edits, n_linking, counted, adds


def allele(col, site):
    return 0 if col == int(site["a0"]) else 1 if col == int(site["a1"]) else NONE


def decide(n, min_reads=2, max_minor_permille=200):
    """rule H5 -> (joined, r)"""
    c, t = int(n[0]) + int(n[3]), int(n[1]) + int(n[2])
    total, minor = c + t, min(c, t)
    joined = total >= max(1, min_reads) and c != t and minor * 1000 <= total * max_minor_permille
    return joined, int(joined and t > c)


def solve(sites, links, min_reads=2, max_minor_permille=200):
    """rules H5-H7, site after site -> [(set_pos, set_index, hap, flags)]"""
    out = []
    heads = 0
    prev = (False, 0)
    for s in range(len(sites)):
        exists = s + 1 < len(sites) and int(sites["record"][s + 1]) == int(sites["record"][s])
        mine = decide(links[s], min_reads, max_minor_permille) if exists else (False, 0)
        if s == 0 or not prev[0]:
            heads += 1
            set_pos, hap, flags = int(sites["pos"][s]), 0, HEAD
        else:
            set_pos, hap, flags = out[-1][0], out[-1][2] ^ prev[1], 0
        out.append((set_pos, heads - 1, hap, flags | (JOINED if mine[0] else 0)))
        prev = mine
    return out


def assert_links(amap, links):
    got = amap.phase_links()
    want = PW.as_u32(links)
    assert got.shape == want.shape and got.dtype == np.uint32, (got.shape, want.shape)
    if not np.array_equal(got, want):
        s = int(np.argwhere((got != want).any(axis=1))[0][0])
        raise AssertionError(("link", s, "got", got[s].tolist(), "want", want[s].tolist()))


def assert_solve(amap, sites, links, **kw):
    got = amap.phase_solve(**kw)
    want = solve(sites, links, **kw)
    exists = [s + 1 < len(sites) and int(sites["record"][s + 1]) == int(sites["record"][s]) for s in range(len(sites))]
    assert len(got) == len(want)
    have = list(zip(got["set_pos"].tolist(), got["set_index"].tolist(), got["hap"].tolist(), got["flags"].tolist()))
    if have != want:
        s = next(k for k in range(len(want)) if have[k] != want[k])
        raise AssertionError(("site", s, "got", have[s], "want", want[s]))
    assert np.array_equal(got["link"], PW.as_u32(links) * np.array(exists, np.uint32)[:, None]) and not got["reserved"].any()
    return got


# ---- the subprocess case --------------------------------------------------------------------------------------------
def grid_case(dcn):
    """300 rows over record 0 of the pileup seams' records, each with a substitution or two, and a site every 17 bases"""
    from test_gpu_pileup_seams import make_records, other
    records = make_records()
    rng = np.random.default_rng(77)
    sites = []
    for pos in range(100, 3900, 17):
        ref = PW.column(records[0][pos])
        alt = (ref + 1 + pos % 3) % 4
        sites.append((0, pos, min(ref, alt), max(ref, alt)))
    reads, rows = [], []
    dtype = dcn.filter.PLACEMENT_DTYPE
    for q in range(300):
        a = int(rng.integers(0, 3800))
        n = int(rng.integers(40, 180))
        b = min(a + n, len(records[0]))
        S = bytearray(records[0][a:b])
        for at in rng.integers(0, len(S), 3):
            S[at] = other(bytes(S[at:at + 1]))[0]
        rev = q % 2
        reads.append(PW.revcomp(bytes(S)) if rev else bytes(S))
        rows.append(VW.make_row(dtype, 0, rev, 0, len(S), a, b))
    return records, make_sites(dcn.filter.PHASE_SITE_DTYPE, sites), reads, np.concatenate(rows)


def case_grid(O, dcn):
    """DCN_GRID_CUS = 1 with 300 rows: the capped grid of the link kernel takes the second trip of its work loop"""
    assert os.environ.get("DCN_GRID_CUS") == "1"
    records, sites, reads, rows = grid_case(dcn)
    assert int((AW.align_rows(reads, records, rows)[0] < OVER).sum()) > 128  # (one trip of that grid: 32 workgroups of four waves)
    amap = VW.build_map(O, dcn, records)
    amap.phase_sites(sites)
    placer = dcn.Placer(amap, max_batch_bases=1 << 18, max_batch_reads=1 << 10)
    b, o = O.concat_reads(reads)
    edits, n_linking = placer.phase_batch(b, o, rows)
    links = np.zeros((len(sites), 4), np.int64)
    want = link_rows(links, sites, reads, records, rows)
    assert edits.tolist() == want[0].tolist() and n_linking == want[1] and n_linking > 100
    assert_links(amap, links)
    assert amap.phase_info() == (len(sites), want[2], want[1], want[3])
    text = np.ascontiguousarray(amap.phase_links()).tobytes().hex()
    placer.close()
    amap.close()
    print("phase grid " + text)


if __name__ == "__main__":
    import deacon_server_amd as dcn
    from oracle import oracle as O
    O.lib()
    {"grid": case_grid}[sys.argv[1]](O, dcn)
