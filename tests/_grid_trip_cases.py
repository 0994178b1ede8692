"""The cases of tests/test_gpu_grid_trips.py: inputs whose calls make the work loop of a capped-grid kernel run a second and a
third time per wave or workgroup, and what the existing models say of them.  CPU only; tests/test_grid_trip_cases.py checks
that no case is vacuous: that its items exceed the cap, that the items a wave takes one after the other differ in shape, and
that the item after a stateful one would show what the first left behind.

Most kernels behind the row calls, the vote, classify and locate launch a grid capped at a multiple of dcn_cu_count()
(ctx.hip) and stride over the rest of their work.  DCN_GRID_CUS lowers that count at call time (never raises it), so with
DCN_GRID_CUS = 1 a few hundred items loop; the full-grid case needs no hook and has more rows than the caps of an MI355X.
The caps are stated here once, as functions of C = dcn_cu_count()."""
import functools

import numpy as np

import _align_worker as AW
import _extend_worker as XW
import _insertion_worker as IW
import _pileup_worker as PW
import _verify_worker as VW
from conftest import random_reads, revcomp

HOOK_CUS = 1      # what the hooked tests set DCN_GRID_CUS to
FULL_CUS = 256    # an MI355X
OVER, UNPLACED = VW.OVER, VW.UNPLACED


# ---- the caps: how many items a grid takes in one trip ----------------------------------------------------------------
def wave_rows(C):
    """verify_kernel and align_kernel: dcn_verify.h, dcn_wave_grid_for: `resident = dcn_cu_count() * 32`, blocks =
    min(n, resident * 4); a block is one wave and takes one row (verify.hip: `row += gridDim.x`)"""
    return C * 32 * 4


def extend_rows(C):
    """extend_kernel: extend.hip, dcn_launch_extend: dcn_wave_grid_for over (n_items + WAVE_FLANKS - 1) / WAVE_FLANKS blocks of
    WAVE_FLANKS = 4 flanks; extend_api.hip makes two flanks of every row (`items(2 * n_rows)`)"""
    return C * 32 * 4 * 4 // 2


def wave4_items(C):
    """pileup_kernel (pileup.hip, dcn_launch_pileup), align_gather_kernel (align.hip, dcn_launch_align_gather) and the
    wave-strided kernels of insertions.hip (wave_blocks): min(.., dcn_cu_count() * 32) blocks of four waves, an item each"""
    return C * 32 * 4


def winner_positions(C):
    """ins_winner_kernel: insertions.hip, dcn_launch_ins_winner: wave_blocks((n + 63) / 64), a wave per 64 positions"""
    return wave4_items(C) * 64


def list_items(C):
    """place_wg_kernel (place_vote.hip, plc_launch_vote: `min(a.n_reads, dcn_cu_count() * 4)`) and classify_big_kernel
    (classify.hip, dcn_launch_classify_big: `min(a.n_units, dcn_cu_count() * 4)`): a workgroup per listed item"""
    return C * 4


def locate_reads(C):
    """locate_segments_wave_kernel: locate.hip, loc_wave_blocks: min(.., dcn_cu_count() * 8) blocks of DCN_LOC_THREADS / 64 =
    4 waves, a read each"""
    return C * 8 * 4


def sweep_blocks(C):
    """the thread-strided sweeps: place.hip (plc_sweep_blocks), set_algebra.hip (sa_blocks), depth.hip, index_builder.hip,
    classify.hip (cov_blocks) and track.hip (trk_piece_blocks): min(.., dcn_cu_count() * 8) blocks"""
    return C * 8


SWEEP_THREADS = 256  # DCN_PLC_THREADS, SA_THREADS, DCN_COV_THREADS and the builder's and depth's block: one slot per thread


def trips(items, cap):
    """how many times the busiest wave (workgroup, thread) runs its loop's body"""
    return (int(items) + cap - 1) // cap


def stride(items, cap):
    """the grid's stride over `items` items: the grid is min(items, cap) wide (in units of items)"""
    return min(int(items), cap)


# ---- seeing how many rows a call of an existing seam case has ---------------------------------------------------------
ROW_CALLS = ("verify_batch", "align_batch", "pileup_batch", "extend_batch")


class CountingPlacer:
    """a Placer whose row calls note (name, rows, aligned rows or None) and are otherwise the Placer's own"""

    def __init__(self, placer):
        self._placer, self.calls = placer, []

    def __getattr__(self, name):
        f = getattr(self._placer, name)
        if name not in ROW_CALLS:
            return f

        def call(b, o, rows, *args, **kw):
            out = f(b, o, rows, *args, **kw)
            edits = out[0] if name in ("align_batch", "pileup_batch") else None
            self.calls.append((name, len(rows), None if edits is None else int((np.asarray(edits) < OVER).sum())))
            return out
        return call

    def largest(self, name):
        """(rows, aligned rows) of ONE call of that name: the one with the most aligned rows (verify, extend: the most rows)"""
        mine = [c for c in self.calls if c[0] == name]
        best = max(mine, key=lambda c: (c[2] or 0, c[1]))
        return best[1], best[2] or 0


def assert_looped(counting, name, C=HOOK_CUS):
    """one `name` call that the case made had more items than its kernels take in one trip"""
    rows, aligned = counting.largest(name)
    if name == "verify_batch":
        assert trips(rows, wave_rows(C)) >= 2, (name, rows)
    elif name == "extend_batch":
        assert trips(rows, extend_rows(C)) >= 2, (name, rows)
    else:  # align and pileup: verify over the rows, then the aligned rows
        assert trips(rows, wave_rows(C)) >= 2 and trips(aligned, wave4_items(C)) >= 2, (name, rows, aligned)


ALIGN_TRACE_BYTES = 1 << 30  # DCN_ALIGN_TRACE_DEFAULT (align_api.hip): what the traces of one group of rows may take


def trace_bytes(edits):
    """the traces of a call's aligned rows: (d + 1)^2 words each (dcn_align.h, dcn_aln_trace_words).  Within the budget all of
    them are ONE trace group, so align_kernel's grid strides over the whole work list"""
    d = np.asarray(edits)[np.asarray(edits) < OVER].astype(np.int64)
    return int(((d + 1) ** 2).sum()) * 4


def assert_listed(n_listed, C=HOOK_CUS):
    """a call listed more reads than place_wg_kernel's workgroups take in one trip"""
    assert trips(n_listed, list_items(C)) >= 2, n_listed


# ---- the map chain: one call of hand-written rows through extend, verify, align and pileup -----------------------------
LEN0, LEN1 = 12_005, 1_777       # (12,005 % 16 != 0: record 1 starts mid-word of the store and of every plane)
CHAIN_ROWS = 600
CHAIN_KW = dict(max_edits=160, max_permille=1000)  # E = min(160, the longer side): a pure gap aligns, an unrelated 400 does not
N_ROW, N_AT, N_BASES = 300, 9000, 150   # the row of (1=1I) x 150: its number, its interval on record 0
KINDS = ("clean", "large", "unplaced", "ins_many", "n0", "runs", "over", "del", "m0", "long_clean")


def chain_records():
    rng = np.random.default_rng(1911)
    a, b = bytearray(random_reads(rng, 1, LEN0, LEN0)[0]), bytearray(random_reads(rng, 1, LEN1, LEN1)[0])
    a[1300:1370] = b"A" * 70
    b[100:103] = b"NNN"
    b[200:260] = bytes(b[200:260]).lower()
    return [bytes(a), bytes(b)]


def other(base, *avoid):
    return next(bytes([x]) for x in b"ACGT" if all(bytes([x]) != y.upper() for y in (base,) + avoid))


def _row(R, rev, left, S, right, a, b):
    """the read left + S + right as the row's strand reads it, S on records[R][a:b] -> (read, row)"""
    oriented = left + S + right
    L, lo, hi = len(oriented), len(left), len(left) + len(S)
    row = VW.make_row(IW.ROW, R, rev, L - hi if rev else lo, L - lo if rev else hi, a, b)
    return (revcomp(oriented) if rev else oriented), row


def _kind_row(rng, records, kind):
    """one row of a kind.  Rows stay clear of [N_AT - 200, N_AT + N_BASES + 200) of record 0, which belongs to the N row."""
    rec0, rec1 = records

    def at(R, n, margin=40):
        L = len(records[R])
        while True:
            a = int(rng.integers(margin, L - n - margin))
            if R == 1 or a + n + margin < N_AT - 200 or a - margin > N_AT + N_BASES + 200:
                return a
    rev = int(rng.integers(0, 2))
    if kind == "unplaced":
        return random_reads(rng, 1, 50, 50)[0], VW.make_row(IW.ROW, UNPLACED, 0, 0, 0, 0, 0)
    if kind == "clean":    # d = 0, with the record's own bases on both sides: extend carries the row over them
        n, f = int(rng.integers(40, 151)), int(rng.integers(5, 31))
        a = at(0, n)
        return _row(0, rev, rec0[a - f:a], rec0[a:a + n], rec0[a + n:a + n + f], a, a + n)
    if kind == "long_clean":
        a = at(0, 300)
        return _row(0, 0, b"", rec0[a:a + 300], b"", a, a + 300)
    if kind == "large":    # d of about 50 on 200 bases, unrelated bases on both sides
        a = at(0, 200)
        return _row(0, rev, random_reads(rng, 1, 0, 20)[0], VW.mutate_mixed(rng, rec0[a:a + 200], 0.25), random_reads(rng, 1, 0, 20)[0], a, a + 200)
    if kind == "ins_many":  # 12 I runs of 1 - 3 invalid bases (they equal nothing, so each run stays where it is)
        a = at(0, 64)
        T = rec0[a:a + 64]
        S = b"".join(T[p:p + 1] + (b"N" * (1 + p % 3) if p % 5 == 2 and p < 60 else b"") for p in range(64))
        return _row(0, rev, b"", S, b"", a, a + 64)
    if kind == "n0":       # n = 0: all I, aligned under CHAIN_KW, and adds nothing (rule P2)
        a = at(0, 0)
        return _row(0, rev, b"", random_reads(rng, 1, 20, 20)[0], b"", a, a)
    if kind == "m0":       # m = 0: all D
        a = at(1, 20)
        return _row(1, rev, b"", b"", b"", a, a + 20)
    if kind == "runs":     # a substitution at every fourth base of 260: about 130 runs, three chunks of 64
        a = at(0, 260)
        S = bytearray(rec0[a:a + 260])
        for p in range(1, 260, 4):
            S[p] = other(bytes(S[p:p + 1]))[0]
        return _row(0, rev, b"", bytes(S), b"", a, a + 260)
    if kind == "over":     # unrelated: d of about 210 on 400 bases, past max_edits
        a = at(0, 400)
        return _row(0, rev, b"", random_reads(rng, 1, 400, 400)[0], b"", a, a + 400)
    assert kind == "del"   # three deletions of two bases on record 1, reverse, a substitution in the left flank
    a = at(1, 120, margin=30)
    T = rec1[a:a + 120]
    S = T[:30] + T[32:60] + T[62:90] + T[92:]
    left = bytearray(rec1[a - 20:a])
    left[10] = other(bytes(left[10:11]))[0]
    return _row(1, 1, bytes(left), S, rec1[a + 120:a + 135], a, a + 120)


@functools.lru_cache(maxsize=None)
def chain_inputs():
    """(records, reads, rows, kinds): CHAIN_ROWS rows, one per read; row N_ROW is the read that is its reference interval with
    an N behind each of its 150 bases"""
    records = chain_records()
    rng = np.random.default_rng(1912)
    reads, rows, kinds = [], [], []
    for i in range(CHAIN_ROWS):
        kind = KINDS[int(rng.integers(0, len(KINDS)))]
        if i == N_ROW:
            kind = "n_behind_each"
            T = records[0][N_AT:N_AT + N_BASES]
            read, row = _row(0, 0, b"", b"".join(T[p:p + 1] + b"N" for p in range(N_BASES)), b"", N_AT, N_AT + N_BASES)
        else:
            read, row = _kind_row(rng, records, kind)
        reads.append(read)
        rows.append(row)
        kinds.append(kind)
    return records, reads, np.concatenate(rows), kinds


def n_runs_of(offs, cigar, r):
    return int(offs[r + 1]) - int(offs[r])


def i_runs_of(offs, cigar, r):
    return int(((cigar[int(offs[r]):int(offs[r + 1])] & 15) == AW.OP_I).sum())


@functools.lru_cache(maxsize=None)
def chain_model():
    """what the models say of the chain -> dict: ext_rows, ext (extend); edits (verify); offs, cigar (align); counts, ledger,
    n_added (pileup with the ledger); work (the aligned rows in row order: the work list of align, pileup and the walk)"""
    records, reads, rows, _ = chain_inputs()
    ext_rows, ext = XW.extend_rows(reads, records, rows, max_edits=CHAIN_KW["max_edits"])
    edits, offs, cigar = AW.align_rows(reads, records, ext_rows, **CHAIN_KW)
    counts, ledger = PW.new_counts(records), IW.new_ledger(records)
    edits2, n_added = IW.pile_rows(counts, ledger, reads, records, ext_rows, **CHAIN_KW)
    assert edits2.tolist() == edits.tolist()
    return dict(ext_rows=ext_rows, ext=ext, edits=edits, offs=offs, cigar=cigar, counts=counts, ledger=ledger, n_added=n_added,
                work=np.flatnonzero(edits < OVER))


def row_shape(rows, edits, offs, cigar, r, max_edits, max_permille):
    """(m, n, E, strand, number of runs, has an I run) of a row; an unplaced row: None"""
    if int(rows["record"][r]) == UNPLACED:
        return None
    m, n = int(rows["read_end"][r]) - int(rows["read_start"][r]), int(rows["ref_end"][r]) - int(rows["ref_start"][r])
    return (m, n, VW.threshold(m, n, max_edits, max_permille), int(rows["reverse"][r]), n_runs_of(offs, cigar, r), i_runs_of(offs, cigar, r) > 0)


# ---- one call at the full grid ------------------------------------------------------------------------------------------
FULL_UNIQUE = 200
FULL_EXTRA = 517
FULL_KW = dict(max_edits=1023, max_permille=200)


def full_rows(C):
    """n = 256 * C + 517: past extend's cap of 256 * C rows, twice verify's and pileup's of 128 * C"""
    return 256 * C + FULL_EXTRA


@functools.lru_cache(maxsize=None)
def full_unique():
    """(records, reads, rows): about 200 unique (read, row) pairs on the chain's records: intervals of 40 - 150 bases on both
    strands, d = 0 .. 8, every third with I runs (enough of them that record 0 alone receives more events than the range
    kernels of the ledger take in one trip at the full grid), the record's own bases around each (extend carries the row over them)"""
    records = chain_records()
    rng = np.random.default_rng(1913)
    reads, rows = [], []
    for u in range(FULL_UNIQUE):
        R = int(u % 7 == 3)
        n, d, rev = int(rng.integers(40, 151)), u % 9, int(rng.integers(0, 2))
        a = int(rng.integers(40, len(records[R]) - n - 40))
        T = records[R][a:a + n]
        if u % 3 == 0 and d:   # I runs of letters that neither neighbour has: 2 .. 4 runs (d = 3: 3), d bases in all
            S, k = bytearray(), min(d, 2 + (u // 3) % 3)
            where = sorted(int(x) for x in rng.choice(np.arange(5, n - 5), k, replace=False))
            for p in range(n):
                S += T[p:p + 1]
                if p in where:
                    ln = d // k + (1 if where.index(p) < d % k else 0)
                    S += other(T[p:p + 1], T[p + 1:p + 2]) * ln
            S = bytes(S)
        else:
            S = VW.edit(rng, T, n_sub=d - d // 2, n_del=d // 2)
        f = int(rng.integers(0, 21))
        read, row = _row(R, rev, records[R][a - f:a], S, records[R][a + n:a + n + f], a, a + n)
        reads.append(read)
        rows.append(row)
    return records, reads, np.concatenate(rows)


def full_draw(C):
    """which unique pair each of the n rows is: every pair at least once, the rest a seeded draw"""
    rng = np.random.default_rng(1914)
    draw = np.concatenate([np.arange(FULL_UNIQUE), rng.integers(0, FULL_UNIQUE, full_rows(C) - FULL_UNIQUE)])
    rng.shuffle(draw)
    return draw


@functools.lru_cache(maxsize=None)
def full_model(C):
    """the models on the unique pairs only, gathered through the draw -> dict: draw, ext_rows, ext (per row of the call);
    edits, offs, cigar (per row of the call); counts (the unique rows' counters weighted by how often each is drawn); ledger
    (each unique row's events, repeated: rule L4 orders them when they are fetched); n_added; work"""
    records, reads, rows = full_unique()
    draw = full_draw(C)
    weight = np.bincount(draw, minlength=FULL_UNIQUE)
    ext_rows, ext = XW.extend_rows(reads, records, rows, max_edits=FULL_KW["max_edits"])
    edits, offs, cigar = AW.align_rows(reads, records, ext_rows, **FULL_KW)
    counts, ledger = PW.new_counts(records), IW.new_ledger(records)
    n_added = 0
    for u in range(FULL_UNIQUE):
        one, events = PW.new_counts(records), IW.new_ledger(records)
        _, added = IW.pile_rows(one, events, reads[u:u + 1], records, ext_rows[u:u + 1], **FULL_KW)
        n_added += added * int(weight[u])
        for R in range(len(records)):
            counts[R] += one[R] * int(weight[u])
            ledger[R] += events[R] * int(weight[u])
    lens = np.diff(offs.astype(np.int64))
    parts = [cigar[int(offs[u]):int(offs[u + 1])] for u in range(FULL_UNIQUE)]
    all_offs = np.concatenate([[0], np.cumsum(lens[draw])]).astype(np.uint64)
    all_cigar = np.concatenate([parts[u] for u in draw]).astype(np.uint32)
    return dict(draw=draw, weight=weight, ext_rows=ext_rows[draw], ext=ext[draw], edits=edits[draw], offs=all_offs, cigar=all_cigar,
                counts=counts, ledger=ledger, n_added=n_added, unique=(edits, offs, cigar, ext_rows),
                work=np.flatnonzero(edits[draw] < OVER))


# ---- the list kernels: place_wg_kernel, classify_big_kernel, locate_segments_wave_kernel --------------------------------
# Their work lists are written with atomicAdd, so the order of the items is the order in which the atomics land, and it is
# not the read order: classify_units_kernel, for one, lists a unit of more than 64 entries at one point and a unit past the
# hit limit at a later one, so lean units can come in front of a heavy unit with a smaller number.  tests/
# test_grid_trip_cases.py proves the alternation of kinds for the list in read order only; what the GPU runs is some other
# interleaving of the same items.  The cases therefore do not rest on one layout: every workgroup takes ten items and more,
# about a third of the items are stateful and the rest lean, in a pattern whose period is coprime to the stride, so that a
# lean item behind a stateful one on some workgroup is what almost every order gives -- likely, not guaranteed.


def _oracle():
    from oracle import oracle as O
    O.lib()
    return O


PLACE_READS = 48
PLACE_CELLS = 16   # DCN_PLACE_LDS_CELLS of the second run


@functools.lru_cache(maxsize=None)
def place_case():
    """(records, model, reads): the records of the place tests at w = 1; read i is stitched from 60 scattered 40-base cuts
    (i % 3 == 0: some 1,200 cells, 16 partitions and more of a 16-slot set), a clean 60-base cut (1) or a clean 300-base cut
    (2).  With DCN_PLACE_LANE_BASES = 0 every read is listed."""
    import _place_worker as PLW
    O = _oracle()
    records = PLW.make_records(PLW.make_genomes())
    model = PLW.AnchorModel(O, 31, 1, O.Index.build(records, k=31, w=1).keys()).add(records)
    rng = np.random.default_rng(1921)
    reads = []
    for i in range(PLACE_READS):
        if i % 3 == 0:
            reads.append(PLW.stitched(rng, records, 60))
        else:
            r = PLW.cut(rng, records, 60, 60) if i % 3 == 1 else PLW.cut(rng, records, 300, 300)
            reads.append(revcomp(r) if i % 2 else r)
    return records, model, reads


def place_shape(model, read, W, slots):
    """(distinct set keys, partitions) of a listed read: what it leaves in the LDS set and how often it sweeps"""
    import _place_worker as PLW
    cells = model.cells(read, W)[0]
    return len({(c[0], c[2]) for c in cells}), PLW.partitions_of(cells, slots)[0]


CLASSIFY_UNITS = 45
CLS_LANE_ENTRIES, CLS_LANE_HITS, CLS_HALF = 64, 32, 2048  # dcn_classify.h; classify_big_kernel's entries per partition


@functools.lru_cache(maxsize=None)
def classify_case():
    """Units of single-window reads (tests/test_gpu_classify_seams.py's Pool and Units) -> Units.  Unit u has 4,300 and more
    entries of 2,400 distinct hashes (u % 5 in (0, 3): three hash partitions), 65 - 67 entries (1, 4: just past the lane
    kernel's entry limit) or 40 entries of which 33 are distinct hits (2: just past its hit limit); at a stride of four a
    unit of kind k is followed by one of kind (k + 4) % 5.  The units draw on one pool, so a
    hash occurs in many units and the members hold it for all of them."""
    from test_gpu_classify_seams import Pool, Units
    pool = Pool(_oracle(), 31, 4200, 1931)
    es = pool.take(4000)
    U = Units(3)
    for u in range(CLASSIFY_UNITS):
        at = (53 * u) % 1500
        if u % 5 in (0, 3):
            mine = es[at:at + 2400]
            mine = mine + mine[:1900 + 10 * u] + [pool.invalid() for _ in range(u % 4)]
        elif u % 5 in (1, 4):
            mine = es[at:at + 65 + u % 3]
        else:
            mine = es[at:at + 40]
        U.add(mine)
    # member 0: every third hash of the pool; member 1: hashes 3,000 and up (no unit has them) and a few; member 2: the
    # first 33 of each lean unit of kind 2
    U.members[0].update(h for _, h in es[::3])
    U.members[1].update(h for _, h in es[3000:])
    U.members[1].update(h for _, h in es[5:1500:7])
    for u in range(2, CLASSIFY_UNITS, 5):
        at = (53 * u) % 1500
        U.members[2].update(h for _, h in es[at:at + 33])
    return U


LOCATE_READS = 120
LOC_LANE_BASES, LOC_ITER_BASES, LOC_K = 1024, 2048, 31


def locate_plan():
    """[(length, hit positions)] of LOCATE_READS reads, all longer than LOC_LANE_BASES (the wave kernel's list).  Kind i % 5:
    0, 3: hits in the read's last word and before: the segment is open when the read ends; 2, 4: 2,300 bases and more with
    no hit in the first 64 words, then hits; 1: hits in the first words only."""
    plan = []
    for i in range(LOCATE_READS):
        kind = i % 5
        if kind in (0, 3):
            ln = 1100 + 37 * (i % 11)
            last = ln - LOC_K
            plan.append((ln, [last - 40, last - 20 - i % 7, last]))
        elif kind in (2, 4):
            ln = 2300 + 41 * (i % 9)
            plan.append((ln, [2100 + i % 13, 2100 + 31 + i % 13, ln - LOC_K - 5 * (i % 3)]))
        else:
            ln = 1500 + 29 * (i % 5)
            plan.append((ln, [3 + i % 9, 20 + i % 9, 700]))
    return plan


# ---- the existing seam cases that are run again under the hook ---------------------------------------------------------
class ModelPlacer:
    """the row calls of a Placer answered by the models: lets tests/test_grid_trip_cases.py run a seam case of verify, align
    or extend without a GPU, under a CountingPlacer, to see how many rows its calls have"""

    def __init__(self, records):
        self.records = records

    @staticmethod
    def _reads(b, o):
        b = bytes(np.asarray(b, np.uint8).tobytes()) if not isinstance(b, (bytes, bytearray)) else bytes(b)
        return [b[int(o[i]):int(o[i + 1])] for i in range(len(o) - 1)]

    def verify_batch(self, b, o, rows, row_offsets=None, **kw):
        if len(rows) == 0:
            return np.zeros(0, np.uint32)
        return VW.verify_rows(self._reads(b, o), self.records, rows, row_offsets, **kw)

    def align_batch(self, b, o, rows, row_offsets=None, capacity=None, **kw):
        return AW.align_rows(self._reads(b, o), self.records, rows, row_offsets, **kw)

    def extend_batch(self, b, o, rows, row_offsets=None, **kw):
        return XW.extend_rows(self._reads(b, o), self.records, rows, row_offsets, **kw)


# (module, test function, its arguments behind env, the row calls that must loop).  Cases of fewer rows than a cap are not
# taken.  The cases of verify, align and extend are proven on the CPU (ModelPlacer); those of pileup and the insertions need
# the map and are counted when they run, by the same assert_looped.
SEAM_CASES = [
    ("test_gpu_verify_seams", "test_every_offset_mod_32_on_both_strands", (), ("verify_batch",)),
    ("test_gpu_verify_seams", "test_interval_lengths", (), ("verify_batch",)),
    ("test_gpu_verify_seams", "test_one_edit_at_the_seams_of_a_word", (), ("verify_batch",)),
    ("test_gpu_verify_seams", "test_row_counts_and_row_offsets", (), ("verify_batch",)),
    ("test_gpu_align_seams", "test_one_edit_at_the_seams_of_a_word", (), ("align_batch",)),
    ("test_gpu_align_seams", "test_row_order_and_counts", (), ("align_batch",)),
    ("test_gpu_extend_seams", "test_row_counts_and_row_offsets", (), ("extend_batch",)),
    ("test_gpu_pileup_seams", "test_one_edit_at_the_seams_of_a_word", (), ("pileup_batch",)),
    ("test_gpu_pileup_seams", "test_row_counts", (257,), ("pileup_batch",)),
    ("test_gpu_pileup_seams", "test_depth_of_one_identical_read", (1000,), ("pileup_batch",)),
    ("test_gpu_insertions_seams", "test_row_counts", (257,), ("pileup_batch",)),
    ("test_gpu_insertions_seams", "test_events_at_one_position", (1000,), ("pileup_batch",)),
    ("test_gpu_insertions_seams", "test_two_alleles_at_one_position", (500, 500), ("pileup_batch",)),
]
CPU_PROVEN = ("test_gpu_verify_seams", "test_gpu_align_seams", "test_gpu_extend_seams")


def seam_id(case):
    return "%s-%s%s" % (case[0].replace("test_gpu_", "").replace("_seams", ""), case[1].replace("test_", ""),
                        "".join("-%s" % a for a in case[2]))


def run_seam_case(case, env, placer):
    """the case's function with `placer` in the place of env's -> the CountingPlacer around it"""
    import importlib
    module, name, args, _ = case
    counting = CountingPlacer(placer)
    getattr(importlib.import_module(module), name)(tuple(env[:4]) + (counting,), *args)
    return counting
