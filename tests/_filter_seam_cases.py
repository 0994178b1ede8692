"""The cases of tests/test_gpu_filter_seams.py: batches whose hits are placed minimizer by minimizer at the numeric edges of
the filter's scan kernel (scan.hip, scan_body) and of its distinct pass (plan.hip), a model of where the planning kernel puts
every tile of such a batch, and the plain statement of what the filter must return.  CPU only;
tests/test_filter_seam_cases.py proves from this model and the oracle that every case reaches the edge it is built for.

How hits are placed.  The oracle gives, for the final bytes of a read, its emitted minimizers in order and which of them
are valid (`analyse`).  The index holds a chosen subset of those hashes.  A read of k + w - 1 bases has one window and so
one item; a read of a few more bases has a few, and the Source hands out reads by their number of items, every hash new.
A duplicate is the same read a second time in a unit (through unit_id), a mate that is the other's reverse complement, or
a repeat inside a read; whatever the construction, the expected numbers come from the oracle's list of the final bytes.

The layout model.  A batch here has at most 256 reads, so dcn_launch_plan runs plan_kernel<1> with ONE workgroup and the tile
order is fixed: with unit_id, tiles follow the reads in order; without, the tiles of the multi-tile reads come first and
the single-tile reads follow (plan.hip, `two_classes`).  A read has ceil(windows / tile_windows) tiles, tile t is lane
t % 64 of scan wave t // 64, and phase B takes a wave's items in flat order: lane by lane, each lane's list in order."""
import collections
import functools
import os
import re

import numpy as np

from conftest import ROOT, revcomp
from test_classify_replicas import group_of
from test_gpu_classify_seams import Pool, group_slots, required
from test_gpu_classify_seams import W as POOL_W

CSRC = os.path.join(ROOT, "deacon-server_amd", "csrc")


# ---- the constants, read from the sources: a changed constant fails the CPU test instead of moving a seam silently ------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _int(name, pattern):
    m = re.search(pattern, _src(name))
    assert m, (name, pattern)
    return int(m.group(1))


WAVE = _int("dcn_internal.h", r"constexpr int DCN_WAVE = (\d+);")            # lanes (tiles) of a scan wave
LCAP = _int("dcn_internal.h", r"constexpr int DCN_LCAP = (\d+);")            # entries of a lane's list between flushes
RCAP = _int("scan.hip", r"constexpr int DCN_RCAP = (\d+);")                  # slots of the in-wave hit ring
FAST_EXTRA = _int("scan.hip", r"#define DCN_FAST_EXTRA_ROUNDS (\d+)")        # own-list rounds beyond abs_threshold
SHORT_LMAX = _int("scan.hip", r"constexpr int DCN_SHORT_LMAX = (\d+);")      # longest read of the short path
TILE_WINDOWS = _int("dcn_ctx.h", r"uint32_t tile_windows = (\d+);")          # windows of a tile unless DCN_TILE_WINDOWS says so
# 2^shift windows per slot of a run: dcn_ctx_create's assignment, the one in front of `if (index->w <= 7) c->rec_shift = 0;`
REC_SHIFT = _int("ctx.hip", r"\n    c->rec_shift = (\d+);\n(?:\s*//[^\n]*\n)*\s*if \(index->w <= 7\) c->rec_shift = 0;")
NO_EARLY_OUT_ENV = re.search(r'static const bool no_early_out = getenv\("(\w+)"\)', _src("ctx.hip")).group(1)  # read once per process
LDS_SET_SLOTS = 1 << _int("plan.hip", r"#define DCN_LDS_SET_LOG2 (\d+)")
_m = re.search(r"DCN_LDS_SET_MAX = DCN_LDS_SET_SLOTS \* (\d+) / (\d+) - (\d+);", _src("plan.hip"))
LDS_SET_MAX = LDS_SET_SLOTS * int(_m.group(1)) // int(_m.group(2)) - int(_m.group(3))  # hits the LDS set takes
LDS_WALK_MAX_TILES = _int("plan.hip", r"constexpr uint32_t DCN_LDS_WALK_MAX_TILES = (\d+);")
ONE_WORKGROUP_READS = 256    # plan.hip, dcn_launch_plan: plan_kernel<1>, (n_reads + 255) / 256 workgroups of 256 reads
ENOUGH_STRIDE = 256          # plan.hip, unit_distinct_kernel: `j0 += 256`, the stop at `enough` is tested once per pass
LOCAL_ITEMS = RCAP - WAVE    # scan.hip, flush: `sh.items[uslot] <= (uint32_t)(DCN_RCAP - DCN_WAVE)`


def fixed_ws():
    """the window sizes with a kernel of their own (scan.hip, dcn_launch_scan: `case W: return launch_w<W>`)"""
    return sorted(int(a) for a, b in re.findall(r"case (\d+): return launch_w<(\d+)>", _src("scan.hip")) if a == b)


def step_of(w):
    """scan.hip, phase A: `constexpr uint32_t STEP = W > 0 ? (uint32_t)W : 8u`"""
    return w if w in fixed_ws() else 8


def flush_above(w):
    """scan.hip: `if (__any(cnt > DCN_LCAP - STEP)) flush(IntTag<1>{}, false)` after every block: a lane whose tile has
    more entries than this forces a mid-scan flush (the test after the tile's last block sees them all)"""
    return LCAP - step_of(w)


def windows_of(length, k, w):
    """dcn_short_lane.h, dcn_window_count, for a read without a prefix cut or a trailing newline"""
    l = k + w - 1
    return 0 if length < k or length < l else length - l + 1


GEOMETRIES = ((31, 15), (41, 15), (31, 11), (21, 9))
# (31, 15): the fixed-W kernel, k <= 32; (41, 15): K128; (31, 11): the other fixed W; (21, 9): generic w, ring in LDS, STEP 8.
# Every constructed batch carries unit_id, which keeps it off the short path (ctx.hip: `!v.d_unit_id`).


def _oracle():
    from oracle import oracle as O
    O.lib()
    return O


# ---- reads by their items -----------------------------------------------------------------------------------------------
Entry = collections.namedtuple("Entry", "read items")  # items: the read's emitted minimizers in order, a hash or None (invalid)


def analyse(O, read, k, w):
    """the emitted minimizers of a read in order -> tuple of hash | None.  Emitted: canonical_minimizer_positions (consecutive
    equal choices merged); valid: those the oracle keeps.  The valid ones, in order, ARE the oracle's list."""
    pos = O.canonical_minimizer_positions(read, k, w).tolist() if windows_of(len(read), k, w) else []
    h, p = O.minimizer_hashes_and_positions(read, k, w)
    by = dict(zip(p.tolist(), h.tolist()))
    items = tuple(by.get(q) for q in pos)
    assert [x for x in items if x is not None] == h.tolist(), "the emitted list does not contain the oracle's in order"
    return items


class Source:
    """reads with a chosen number of items, every hash handed out once over the Source's life"""

    def __init__(self, O, k, w, seed):
        self.O, self.k, self.w, self.l = O, k, w, k + w - 1
        self.rng = np.random.default_rng(seed)
        self.seen = set()
        self.buckets = collections.defaultdict(list)
        self.pool = Pool(O, k, 1200, seed) if w == POOL_W else None  # (its reads have k + POOL_W - 1 bases)

    def random(self, n):
        return np.frombuffer(b"ACGT", np.uint8)[self.rng.integers(0, 4, n)].tobytes()

    def _new(self, items):
        return None not in items and len(set(items)) == len(items) and not (set(items) & self.seen)

    def single(self):
        """a read of one window: one item"""
        while True:
            if self.pool is not None:
                r, h = self.pool.take(1)[0]
                items = (h,)
            else:
                r = self.random(self.l)
                items = analyse(self.O, r, self.k, self.w)
            if len(items) == 1 and self._new(items):
                self.seen.update(items)
                return Entry(r, items)

    def invalid(self):
        """a read of one window whose middle base is N: one item, emitted and not valid"""
        r = bytearray(self.random(self.l))
        r[self.l // 2] = ord("N")
        e = Entry(bytes(r), analyse(self.O, bytes(r), self.k, self.w))
        assert e.items == (None,)
        return e

    def multi(self, j):
        """a read with exactly j items, all valid, all new"""
        if j == 1:
            return self.single()
        while True:
            while self.buckets[j]:
                e = self.buckets[j].pop()
                if self._new(e.items):
                    self.seen.update(e.items)
                    return e
            r = self.random(self.l + int(self.rng.integers(4 * (j - 1), 10 * (j - 1) + 1)))
            items = analyse(self.O, r, self.k, self.w)
            if self._new(items) and 2 <= len(items) <= flush_above(self.w):
                self.buckets[len(items)].append(Entry(r, items))

    def fill(self, n_items, n_reads):
        """n_reads reads with n_items items between them, as even as they go"""
        base, rem = divmod(n_items, n_reads)
        assert base >= 1 and base + 1 <= flush_above(self.w)
        return [self.multi(base + (1 if i < rem else 0)) for i in range(n_reads)]

    def fill_hits(self, n_items, most=5):
        """reads of `most` items and one smaller one: n_items items in as few reads as that gives"""
        out = [self.multi(most) for _ in range(n_items // most)]
        if n_items % most:
            out.append(self.multi(n_items % most))
        return out

    def same_first(self, m, tail):
        """a read whose list begins with m copies of one hash (a short period repeated) and goes on with `tail` or more
        other hashes, all different -- as the oracle reports it for the final bytes"""
        for _ in range(4000):
            per = self.random(int(self.rng.integers(5, 14)))
            r = (per * 20)[:int(self.rng.integers(45, 75))] + self.random(int(self.rng.integers(70, 110)))
            items = analyse(self.O, r, self.k, self.w)
            rest = items[m:]
            if (len(items) >= m + tail and len(items) <= flush_above(self.w) and None not in items and len(set(items[:m])) == 1
                    and items[0] not in rest and len(set(rest)) == len(rest) and not (set(items) & self.seen)):
                self.seen.update(items)
                return Entry(r, items)
        raise AssertionError("no read with %d equal first items" % m)

    def low_complexity(self, which=0):
        """a read of one tile with more entries than a lane's list takes between two flush tests; which: the first such
        read or the second (another hash)"""
        ok = [r for r in (b"AT" * 70, b"ACGT" * 35, b"GCATGCAT" * 18, b"A" * 150)
              if len(analyse(self.O, r, self.k, self.w)) > flush_above(self.w) and windows_of(len(r), self.k, self.w) <= TILE_WINDOWS]
        assert len(ok) > which, "no low-complexity read"
        return Entry(ok[which], analyse(self.O, ok[which], self.k, self.w))


def valid(entries):
    return [h for e in entries for h in e.items if h is not None]


# ---- a case ---------------------------------------------------------------------------------------------------------------
class Case:
    """units of entries (unit u = reads with unit_id u), the keys the case wants in the index, and what it aims at"""

    def __init__(self, name, k, w, aim, env=None):
        self.name, self.k, self.w, self.aim, self.env = name, k, w, aim, dict(env or {})
        self.units, self.keys, self.mark = [], set(), {}
        self.thresholds = THRESHOLDS

    def add(self, entries, keys=None, mark=None):
        """keys: the hashes of this unit that go into the index (default: every valid one) -> the unit's number"""
        self.units.append(list(entries))
        self.keys.update(valid(entries) if keys is None else keys)
        if mark:
            self.mark[mark] = len(self.units) - 1
        return len(self.units) - 1

    @property
    def n_reads(self):
        return sum(len(u) for u in self.units)

    def pad_to_wave(self, src):
        """single reads without a key, a unit each, up to the next multiple of 64 reads (single-tile reads: 64 tiles)"""
        while self.n_reads % WAVE:
            self.add([src.single()], keys=())

    def batch(self):
        reads = [e.read for u in self.units for e in u]
        uid = np.array([i for i, u in enumerate(self.units) for _ in u], np.uint32)
        assert 0 < len(reads) <= ONE_WORKGROUP_READS, (self.name, len(reads))
        return reads, uid

    def tile_windows(self):
        return int(self.env.get("DCN_TILE_WINDOWS", TILE_WINDOWS))


# ---- the layout model -------------------------------------------------------------------------------------------------------
Tile = collections.namedtuple("Tile", "read unit j items entries")  # entries: what the lane's list takes (items + the carry entry)


def window_choices(O, read, k, w):
    """the minimizer position every window of a read chooses: a window's choice depends on its own k + w - 1 bases only
    (scan.hip, header), so it is the oracle's answer for those bases alone"""
    l = k + w - 1
    return [int(O.canonical_minimizer_positions(read[i:i + l], k, w)[0]) + i for i in range(windows_of(len(read), k, w))]


def read_tiles(O, entry, k, w, tile_windows):
    """the tiles of one read -> [(items, entries)].  Tile j holds windows [j * tile_windows, ..); a window emits an item when
    its choice differs from the previous window's (the first window always does); a tile behind the first recomputes the
    window in front of it as a carry entry, which phase B drops (plan.hip, write_tile; scan.hip, first_pending)"""
    n = windows_of(len(entry.read), k, w)
    nt = (n + tile_windows - 1) // tile_windows
    if nt <= 1:
        return [(entry.items, len(entry.items))] * nt
    choice = window_choices(O, entry.read, k, w)
    first = [i for i in range(n) if i == 0 or choice[i] != choice[i - 1]]
    assert [choice[i] for i in first] == O.canonical_minimizer_positions(entry.read, k, w).tolist(), "the window model is off"
    assert len(first) == len(entry.items)
    out = []
    for j in range(nt):
        mine = tuple(entry.items[x] for x, i in enumerate(first) if j * tile_windows <= i < (j + 1) * tile_windows)
        out.append((mine, len(mine) + (1 if j else 0)))
    return out


class Layout:
    """where plan_kernel<1> puts the tiles of a case's batch, and what the scan kernel's waves make of them"""

    def __init__(self, O, case, with_unit_id=True):
        self.case, self.w = case, case.w
        per_read = []
        r = 0
        for u, es in enumerate(case.units):
            for e in es:
                per_read.append([Tile(r, u if with_unit_id else r, j, it, n)
                                 for j, (it, n) in enumerate(read_tiles(O, e, case.k, case.w, case.tile_windows()))])
                r += 1
        if with_unit_id:
            self.tiles = [t for ts in per_read for t in ts]
        else:  # two classes: the multi-tile reads' tiles, then the single-tile reads
            self.tiles = [t for ts in per_read if len(ts) > 1 for t in ts] + [t for ts in per_read if len(ts) == 1 for t in ts]
        self.n_waves = (len(self.tiles) + WAVE - 1) // WAVE

    def wave(self, i):
        return self.tiles[i * WAVE:(i + 1) * WAVE]

    def where(self, unit):
        """[(tile index, Tile)] of a unit"""
        return [(t, x) for t, x in enumerate(self.tiles) if x.unit == unit]

    def waves_of(self, unit):
        return sorted({t // WAVE for t, _ in self.where(unit)})

    def lanes_of(self, unit):
        return [(t // WAVE, t % WAVE) for t, _ in self.where(unit)]

    def local(self, unit):
        """scan.hip: `first >= wave_first && first + count <= wave_first + DCN_WAVE`"""
        return len(self.waves_of(unit)) == 1

    def flushes(self, wave):
        """some lane of the wave forces a mid-scan flush: then `go_global` takes in-wave resolution from every unit of it"""
        return any(t.entries > flush_above(self.w) for t in self.wave(wave))

    def items(self, unit, wave=None):
        """the unit's items in flat order (of one wave, or of all)"""
        return [h for t, x in self.where(unit) if wave is None or t // WAVE == wave for h in x.items]

    def in_wave(self, unit):
        """the unit is resolved through the hit ring: `sh.local[uslot] && !go_global && sh.items[uslot] <= DCN_RCAP - DCN_WAVE`"""
        return self.local(unit) and not self.flushes(self.waves_of(unit)[0]) and len(self.items(unit)) <= LOCAL_ITEMS

    def hits(self, unit, keys, wave=None):
        """the unit's raw hits in item order"""
        return [h for h in self.items(unit, wave) if h is not None and h in keys]

    def flat(self, wave):
        """[(unit, hash | None)] of a wave's items in flat order: item e is handled by lane e % 64 of round e // 64"""
        return [(x.unit, h) for x in self.wave(wave) for h in x.items]

    def ring(self, wave, keys):
        """[(unit, hash)] of the hits that go through the wave's ring, in order: hit n sits in slot n % DCN_RCAP"""
        ok = {u for u in {x.unit for x in self.wave(wave)} if self.in_wave(u)}
        return [(u, h) for u, h in self.flat(wave) if u in ok and h is not None and h in keys]


def runs_fit(L, keys, shift):
    """scan.hip: a unit that is not resolved in its wave exports its hits of a wave into a run of one slot per 2^shift
    bases of its reads there (`sh.ucap`); more hits raise run_overflow and the host runs the batch again at shift 0.  True
    when no run of the case comes near that (single-tile reads only; one slot is left to the alignment of the run's start)."""
    case = L.case
    assert len(L.tiles) == case.n_reads
    lens = [len(e.read) for u in case.units for e in u]
    for u in range(len(case.units)):
        if L.in_wave(u):
            continue
        for wv in L.waves_of(u):
            bases = sum(lens[x.read] for t, x in L.where(u) if t // WAVE == wv)
            if len(L.hits(u, keys, wv)) > (bases >> shift) - 1:
                return False
    return True


def expected(O, case, keys, abs_t, rel_t, deplete):
    """the plain statement -> (keep, hits, total) per unit"""
    keep, hits, total = [], [], []
    for es in case.units:
        v = valid(es)
        total.append(len(v))
        hits.append(len(set(v) & keys))
        keep.append(O.meets_filtering_criteria(hits[-1], total[-1], abs_t, rel_t, deplete))
    return keep, hits, total


def distances(hit_list):
    """{d: a rank i with hit_list[i] == hit_list[i + d] and no copy between} of a unit's raw hits"""
    last, out = {}, {}
    for i, h in enumerate(hit_list):
        if h in last:
            out.setdefault(i - last[h], last[h])
        last[h] = i
    return out


# ---- the scan kernel's cases, per geometry --------------------------------------------------------------------------------
A2_DISTANCES = (1, 2, 3, 4, 5, 8, 63, 64, 65, 191)
A2_RANKS = {1: 10, 2: 13, 3: 17, 4: 22, 5: 28, 8: 35, 63: 45, 64: 46, 65: 47, 191: 0}  # d -> rank of the first copy
THRESHOLDS = ((2, 0.01, False), (1, 0.5, False), (1, 0.5, True))


def a1_ring_limit(src):
    """A1, scan.hip flush(): `sh.items[uslot] <= (uint32_t)(DCN_RCAP - DCN_WAVE)`.  Units of a whole wave with 191, 192 and
    193 items, and 192 of which five are invalid; every valid item a hit, two reads of each unit a second time."""
    c = Case("A1", src.k, src.w, a1_ring_limit.__doc__)
    for name, n_items, n_reads, bad in (("191", LOCAL_ITEMS - 1, 63, 0), ("192", LOCAL_ITEMS, 64, 0), ("193", LOCAL_ITEMS + 1, 64, 0),
                                        ("192bad", LOCAL_ITEMS, 64, 5)):
        es = src.fill(n_items - bad, n_reads - bad) + [src.invalid() for _ in range(bad)]
        es[7], es[n_reads // 2] = es[3], es[1]      # the same reads again: duplicates (fill gives 3 .. 4 items, the first ones 4)
        if sum(len(e.items) for e in es) != n_items:  # a copy of another size: put the count right with the last read
            es[-1 - bad] = src.multi(len(es[-1 - bad].items) + n_items - sum(len(e.items) for e in es))
        c.add(es, mark=name)
        c.pad_to_wave(src)
    return c


def a1_thresholds(src):
    """Thresholds on A1's shapes, dcn_required_hits' rounding: totals of 191 (in-wave) and 193 (distinct pass), where
    0.5 * total is x.5 exactly, with required - 1 and required distinct hits; raw hits are more (a read twice)."""
    c = Case("A1t", src.k, src.w, a1_thresholds.__doc__)
    for n_items, n_reads in ((LOCAL_ITEMS - 1, 63), (LOCAL_ITEMS + 1, 64)):
        for less in (1, 0):
            es = src.fill(n_items, n_reads)
            distinct = list(dict.fromkeys(valid(es)))
            es[-1] = es[0]  # (its items are keys below: duplicates among the raw hits; the total stays odd)
            if sum(len(e.items) for e in es) != n_items:
                es[-2] = src.multi(len(es[-2].items) + n_items - sum(len(e.items) for e in es))
            total = len(valid(es))
            assert total == n_items and total % 2 == 1
            present = set(valid(es))
            keys = [h for h in distinct if h in present][:required(1, 0.5, total) - less]
            c.add(es, keys=keys, mark="%d-%d" % (n_items, less))
            c.pad_to_wave(src)
    return c


def a2_distances(src):
    """A2, scan.hip ring compare: `for (uint32_t d0 = 0; __any(d0 < run); d0 += 4)` and `sh.hraw` carried over rounds.  One
    in-wave unit of 192 hits that repeats a hash at each distance of A2_DISTANCES in hit rank; its twin without a repeat."""
    c = Case("A2", src.k, src.w, a2_distances.__doc__)
    at = {}
    for d, r in A2_RANKS.items():
        e = src.single()
        at[r], at[r + d] = e, e
    assert len(at) == 2 * len(A2_RANKS) and max(at) == LOCAL_ITEMS - 1
    for twin in (False, True):
        es, rank = [], 0
        for r in sorted(at):
            es += src.fill_hits(r - rank)
            es.append(src.single() if twin else at[r])
            rank = r + 1
        assert len(es) <= WAVE and sum(len(e.items) for e in es) == LOCAL_ITEMS
        c.add(es, mark="control" if twin else "dup")
        c.pad_to_wave(src)
    return c


def a2_thresholds(src):
    """Thresholds on a unit with duplicates at ring distances: 63 items, 0.5 * 63 = 31.5 -> 32 required; 31 and 32 distinct
    hits among 40 raw ones."""
    c = Case("A2t", src.k, src.w, a2_thresholds.__doc__)
    for less in (1, 0):
        es = src.fill(55, 18)
        es += es[:2] + [src.single()]
        while sum(len(e.items) for e in es) < 63:
            es.append(src.single())
        assert sum(len(e.items) for e in es) == 63 and len(es) <= WAVE
        distinct = list(dict.fromkeys(valid(es)))
        c.add(es, keys=distinct[:required(1, 0.5, 63) - less], mark="63-%d" % less)
    c.pad_to_wave(src)
    return c


def a3_neighbours(src):
    """A3, scan.hip ring compare: `d0 + 3 < run` bounds the walk at the unit's own hits, and `x & (DCN_RCAP - 1)` wraps.  Wave
    0: A's last hit is B's first; C's last hit is D's hit of rank 3 and of rank 7.  Wave 1: five units with 320 hits; the
    first hit of the fifth is the hash 256 ring slots earlier (the first unit's first), and it repeats hashes of its own."""
    c = Case("A3", src.k, src.w, a3_neighbours.__doc__)
    x, y = src.single(), src.single()
    c.add(src.fill_hits(11) + [x], mark="A")
    c.add([x] + src.fill_hits(9), mark="B")
    c.add(src.fill_hits(13) + [y], mark="C")
    c.add([src.single(), src.single(), src.single(), y, src.single(), src.single(), src.single(), y] + src.fill_hits(6), mark="D")
    c.pad_to_wave(src)
    z = src.single()
    c.add([z] + src.fill(63, 12), mark="R0")
    c.add(src.fill(64, 13), mark="R1")
    c.add(src.fill(64, 13), mark="R2")
    c.add(src.fill(64, 12), mark="R3")
    own = src.fill(58, 11)
    c.add([z] + own[:5] + [own[1]] + own[5:], mark="R4")
    assert c.n_reads == 2 * WAVE
    return c


def a4_rounds(src):
    """A4, scan.hip ring bookkeeping: `run_head = lok && (below == 0 || prev_us != o_uslot[u])`, `rank_head`, and the update of
    sh.hraw / sh.hits by a run's first lane.  Wave 0 has 192 items: unit boundaries at flat items 63|64 and 127|128; the
    first unit's only hit is lane 0 of round 0, the second's lane 63 of round 1, and round 2 holds three units with hits.
    Wave 1: a unit of 128 items whose second round repeats the first, so every hit lane of that round is a duplicate."""
    c = Case("A4", src.k, src.w, a4_rounds.__doc__)
    es = src.fill(60, 20) + [src.multi(4)]
    c.add(es, keys=valid(es)[:1], mark="lane0")
    es = src.fill(60, 20) + [src.multi(4)]
    c.add(es, keys=valid(es)[-1:], mark="lane63")
    for name, n, r in (("r2a", 21, 7), ("r2b", 21, 7), ("r2c", 22, 8)):
        es = src.fill(n, r)
        c.add(es, keys=valid(es)[::2], mark=name)
    assert c.n_reads == WAVE
    es = src.fill(60, 20) + [src.multi(4)]
    c.add(es + es, mark="echo")
    c.pad_to_wave(src)
    return c


def a6_flush(src, clean, with_it):
    """A6, scan.hip: `if (!final_flush) go_global = true`.  63 clean reads in 22 units: two pairs whose mate 2 is the reverse
    complement of mate 1, nineteen units a, b, a (a read twice) and a pair a, a; every other item of a read is a key, so
    every unit has the same hash as a hit twice and its duplicates must go whether the ring or, after the flush, the
    distinct pass counts it.  `with_it`: a low-complexity read behind the first ten reads (lane 10) forces the wave's
    mid-scan flush."""
    c = Case("A6" if with_it else "A6c", src.k, src.w, a6_flush.__doc__)
    lanes = 0
    for es in clean:
        if with_it and lanes == 10:
            c.add([src.low_complexity()], keys=(), mark="low")
        c.add(es, keys=[h for e in es for h in e.items[::2]])
        lanes += len(es)
    assert lanes == WAVE - 1
    return c


def a6_clean(src):
    """the clean units of A6: 4 + 6 reads in front of lane 10, 53 behind it"""
    def rc(e):
        return Entry(revcomp(e.read), analyse(src.O, revcomp(e.read), src.k, src.w))
    units = []
    for _ in range(2):
        a = src.multi(3)
        units.append([a, rc(a)])
    for _ in range(19):
        a, b = src.multi(3), src.multi(4)
        units.append([a, b, a])
    a = src.multi(3)
    units.append([a, a])
    return units


class World:
    """the default-environment cases of one geometry, over one Source, so that no hash of one case is a key of another:
    one index (the union of the cases' keys) serves them all, and one context can run them in any order (C5)"""

    def __init__(self, k, w):
        O = _oracle()
        self.O, self.k, self.w = O, k, w
        self.src = Source(O, k, w, 7000 + 100 * k + w)
        s = self.src
        clean = a6_clean(s)
        self.cases = [a1_ring_limit(s), a1_thresholds(s), a2_distances(s), a2_thresholds(s), a3_neighbours(s), a4_rounds(s),
                      a6_flush(s, clean, True), a6_flush(s, clean, False)]
        if (k, w) == (31, 15):
            self.cases += [c2_set_edge(s, H) for H in (LDS_SET_MAX - 1, LDS_SET_MAX, LDS_SET_MAX + 1)]
            self.cases += c3_enough(s)
        self.keys = set().union(*(c.keys for c in self.cases))
        self.by_name = {c.name: c for c in self.cases}

    def stale_plan(self):
        """C5 -> ([(case, thresholds)], keys): every case of this world and, at (31, 15), the B batches (each with its own
        abs_threshold, under which the wave of B-n takes the scan's early-out in a decisions-only call), over ONE index: the
        union of their keys and the hash of overflow_case.  The CPU test holds that no hash of one case is a key of another
        and that no run of the plan overflows at DCN_REC_SHIFT = 3."""
        over, keys = self.overflow_case()
        plan = [(c, c.thresholds) for c in self.cases]
        if (self.k, self.w) == (31, 15):
            plan += [(case, thr) for _, case, _, thr in b_plan()]
        for c, _ in plan:
            keys = keys | c.keys
        return plan, keys

    @functools.lru_cache(maxsize=None)
    def overflow_case(self):
        """C5: a unit of a low-complexity read (not A6's: the second such read), whose one hash is a key, and a clean read: at
        DCN_REC_SHIFT = 3 its run does not hold its hits -> (case, the world's keys with that hash)"""
        low = self.src.low_complexity(1)
        c = Case("overflow", self.k, self.w, self.overflow_case.__doc__)
        c.add([low, self.src.single()], keys=[h for h in low.items if h is not None])
        c.add([self.src.single()], keys=())
        return c, self.keys | c.keys

    def key_array(self):
        return np.array(sorted(self.keys), np.uint64)

    @functools.lru_cache(maxsize=None)
    def layout(self, name):
        return Layout(self.O, self.by_name[name])


@functools.lru_cache(maxsize=None)
def world(k, w):
    return World(k, w)


# ---- the distinct pass through the scan -------------------------------------------------------------------------------------
def c2_set_edge(src, H):
    """C2, plan.hip unit_distinct_kernel: `Hset > DCN_LDS_SET_MAX` sends a unit to the global set.  One unit of 90 reads (two
    waves, so nothing of it is resolved in-wave) with exactly H raw hits, sixty-odd of them copies."""
    c = Case("C2-%d" % H, src.k, src.w, c2_set_edge.__doc__)
    es = src.fill(H - 64, 86)
    es += es[:4]                      # four reads twice
    n = sum(len(e.items) for e in es)
    assert n >= H
    keys = list(dict.fromkeys(valid(es)))
    drop = n - H                      # items that must not be hits: hashes of reads that occur once
    once = [h for e in es[4:86] for h in e.items][:drop]
    c.add(es, keys=[h for h in keys if h not in set(once)], mark="unit")
    return c


def c3_enough(src):
    """C3, plan.hip unit_distinct_kernel in decisions-only mode: `if ((uint64_t)H < req)`, `Hset = H < enough ? H : enough`,
    `distinct < enough` tested once per 256 entries.  Units of ten reads and more (never the early-out path of the scan).
    required is 2 (abs 2, rel 0.01 of 200 items: more than the ring serves), 33 (rel 0.165 of 200) and 300 (rel 0.06 of
    5,000).  below: required - 1 distinct hits, repeated to many more raw hits than required: dropped.  last: required
    distinct hits, the last new one the unit's last item.  few: fewer raw hits than required.  exact: as many raw hits
    as required, all different: kept.  early (5,000 items, all different, all keys; 33 required): required is reached
    inside the first 256 entries of the first run, which has 1,280 (64 reads of 20 items; a wave's run cannot hold 5,000)."""
    out = []
    for name, total, n_reads, req, rel in (("C3-2", 200, 20, 2, 0.01), ("C3-33", 200, 20, 33, 0.165),
                                           ("C3-300", 5000, 250, 300, 0.06)):
        assert required(2, rel, total) == req
        per = total // n_reads
        c = Case(name, src.k, src.w, c3_enough.__doc__)
        c.thresholds = ((2, rel, False), (2, rel, True))
        c.req = req
        kinds = [src.multi(per) for _ in range(max(1, (req - 1 + per - 1) // per))]
        es = [kinds[i % len(kinds)] for i in range(n_reads)]
        c.add(es, keys=list(dict.fromkeys(valid(es)))[:req - 1], mark="below")
        if total < 5000:
            tail = src.multi(per)
            es = es[:-1] + [tail]
            c.add(es, keys=list(dict.fromkeys(valid(es[:-1])))[:req - 1] + [tail.items[-1]], mark="last")
            es = [src.multi(per) for _ in range(n_reads)]
            c.add(es, keys=valid(es)[:req - 1], mark="few")
            es = [src.multi(per) for _ in range(n_reads)]
            c.add(es, keys=valid(es)[:req], mark="exact")
        out.append(c)
        if total == 5000:
            c = Case(name + "-early", src.k, src.w, c3_enough.__doc__)
            c.thresholds = ((2, 0.0066, False), (2, 0.0066, True))  # 33 required of 5,000
            c.req = required(2, 0.0066, total)
            c.add([src.multi(per) for _ in range(n_reads)], mark="early")
            out.append(c)
    return out


# ---- decisions-only mode: the early-out block of the scan ------------------------------------------------------------------
def fast_r1(need):
    """scan.hip: `R1 = min(need + (uint32_t)DCN_FAST_EXTRA_ROUNDS, maxc)` with maxc past it"""
    return need + FAST_EXTRA


def early_out_max_items(abs_t, rel_t):
    """ctx.hip, enqueue_batch: the largest total whose required hits still equal abs_threshold"""
    lo, hi = 0, 65535
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if required(abs_t, rel_t, mid) == abs_t:
            lo = mid
        else:
            hi = mid - 1
    return lo


B_SAME = 4      # equal first items of a B1 read
B_FAR_RANK = 9  # own-list rank of the far hit: >= fast_r1(4) = 8


@functools.lru_cache(maxsize=None)
def _b_source():
    """one Source for every B batch: no hash of one is a key of another, so one index can serve them all (C5)"""
    return Source(_oracle(), 31, 15, 9100)


def b_world(need):
    """(case, source) of B-need; the four are built in order, once"""
    return _b_worlds()[need - 1], _b_source()


@functools.lru_cache(maxsize=None)
def _b_worlds():
    return [_b_world(need) for need in (1, 2, 3, 4)]


def _b_world(need):
    """B1 and B2 for abs_threshold = need, (k, w) = (31, 15): every read (B1) or pair (B2) a unit.
    B1, scan.hip note_hit: `(nh > 0 && hash == seen0) | (nh > 1 && hash == seen1) | (nh > 2 && hash == seen2)` and the
    flattened rest behind `R1`.  A read's list is h, h, h, h, d1, d2, ...: its first `need` hits are the same hash.  `none`
    has need - 1 distinct keys (dropped); `near` one more at own-list rank < R1; `far` one more at rank 9 >= R1 instead.
    B2: pairs in adjacent lanes, mate 2 the reverse complement of mate 1, with need - 1 distinct keys (dropped) and with
    need (kept); a pair whose keys are all in mate 2."""
    O = _oracle()
    src = _b_source()
    c = Case("B-%d" % need, 31, 15, b_world.__doc__)
    for rep in range(6):
        for kind in ("none", "near", "far"):
            e = src.same_first(B_SAME, B_FAR_RANK - B_SAME + 2)
            d = list(dict.fromkeys(e.items))          # distinct in order: d[0] at ranks 0..3, d[i] at rank 3 + i
            keys = d[:need - 1]
            if kind == "near":
                keys = d[:need]
            elif kind == "far":
                keys = d[:need - 1] + [e.items[B_FAR_RANK]]
            c.add([e], keys=keys, mark="%s%d" % (kind, rep))
        for kind in ("rc_below", "rc_at", "mate2"):
            m1 = src.multi(6)
            if kind == "mate2":
                m2 = src.multi(6)
                c.add([m1, m2], keys=m2.items[:need], mark="%s%d" % (kind, rep))
            else:
                m2 = Entry(revcomp(m1.read), analyse(O, revcomp(m1.read), 31, 15))
                c.add([m1, m2], keys=m1.items[:need - (1 if kind == "rc_below" else 0)], mark="%s%d" % (kind, rep))
    # 6 * (3 + 6) = 54 lanes; ten more reads with hits in every other item
    for _ in range(WAVE - c.n_reads):
        e = src.multi(7)
        c.add([e], keys=e.items[::2])
    assert c.n_reads == WAVE
    return c


@functools.lru_cache(maxsize=None)
def b3_world():
    """B3, scan.hip: `own = ... && sh.local[uslot] && cnt_unit <= a.early_out_max_items` and `if (__all(own))`.  abs 2, rel
    0.2: 12 items are the most.  A pair cut at lanes 63|64 (its unit is in two waves, so not local): waves 0 and 1 take the
    general path.  Wave 2 ends with a read of 13 items: the general path for its 63 other reads too; in `B3twin` that
    read has 12 and the wave's early-out runs.  -> ([B3, B3twin], 12)"""
    O = _oracle()
    _b_worlds()
    src = _b_source()
    most = early_out_max_items(2, 0.2)
    cases = []
    body = [src.multi(3 + i % 8) for i in range(63 + 63 + 63)]
    m1 = src.multi(5)
    m2 = Entry(revcomp(m1.read), analyse(O, revcomp(m1.read), 31, 15))
    over, at = src.multi(most + 1), src.multi(most)
    for name, last in (("B3", over), ("B3twin", at)):
        c = Case(name, 31, 15, b3_world.__doc__)
        c.thresholds = ((2, 0.2, False), (2, 0.2, True))
        for i, e in enumerate(body):
            if i == 63:
                c.add([m1, m2], keys=m1.items[:2], mark="cut")
            c.add([e], keys=(e.items[1:3], e.items[:1], ())[i % 3])
        c.add([last], keys=last.items[4:6], mark="last")
        assert c.n_reads == 3 * WAVE
        cases.append(c)
    return cases, most


def b_plan():
    """[(name, case, the keys of its index, thresholds)] of the B batches: what test_early_out, the B4 child and C5 run"""
    (b3, twin), _ = b3_world()
    out = [("B-%d" % n, b_world(n)[0], b_world(n)[0].keys, ((n, 0.01, False), (n, 0.01, True))) for n in (1, 2, 3, 4)]
    return out + [("B3", b3, b3.keys | twin.keys, b3.thresholds), ("B3twin", twin, b3.keys | twin.keys, twin.thresholds)]


# ---- tiny tiles: locality (A5) and the tile-count edge (C4) ------------------------------------------------------------------
TINY = 16  # DCN_TILE_WINDOWS of these cases: a tile has at most 17 entries, so no wave flushes mid-scan


def _read_of_tiles(src, n_tiles, repeat=False):
    """a random read of exactly n_tiles tiles of TINY windows; repeat: its second half begins with a copy of its first 200 bases"""
    n = n_tiles * TINY + src.l - 1
    r = src.random(n)
    if repeat:
        r = r[:n // 2] + r[:200] + r[n // 2 + 200:]
    assert len(r) == n
    return Entry(r, analyse(src.O, r, src.k, src.w))


@functools.lru_cache(maxsize=None)
def a5_world(k=31, w=15):
    """A5, scan.hip: `loc = count != 0xFFFFFFFFu && first >= wave_first && first + count <= wave_first + DCN_WAVE`, with
    DCN_TILE_WINDOWS = 16.  Tiles 0..39 and 40..63: two units of wave 0, the second ending at lane 63; 64..93: a unit from
    lane 0 of wave 1; 94..128: a unit that crosses into wave 2 by one tile; 129..190; then a pair of one-tile mates in
    lanes 63 and 64 of the batch's tiles 191 and 192, mate 2 the reverse complement of mate 1: each hash once on either side."""
    O = _oracle()
    src = Source(O, k, w, 9300 + 100 * k + w)
    c = Case("A5", k, w, a5_world.__doc__, env={"DCN_TILE_WINDOWS": str(TINY)})
    for name, n_tiles, rep in (("first", 40, True), ("ends63", 24, False), ("lane0", 30, True), ("crosses", 35, True), ("body", 62, False)):
        e = _read_of_tiles(src, n_tiles, rep)
        v = valid([e])
        c.add([e], keys=v if name == "crosses" else v[::2] + v[-3:], mark=name)
    m1 = _read_of_tiles(src, 1)
    m2 = Entry(revcomp(m1.read), analyse(O, revcomp(m1.read), k, w))
    c.add([m1, m2], mark="pair")
    return c, Layout(O, c)


def _plant(src, r, a, b, n):
    """copy n bases of r from a to b"""
    return r[:b] + r[a:a + n] + r[b + n:]


@functools.lru_cache(maxsize=None)
def c4_world():
    """C4, plan.hip unit_distinct_kernel: `count > DCN_LDS_WALK_MAX_TILES`, with DCN_TILE_WINDOWS = 16: a read of exactly 1024
    tiles (pass A walks its tiles in 16 rounds of 64) and one of 1025 (the global set, 17 work items of pass B).  Each has
    a 60-base segment a second time, far away: the keys are a hash that occurs in both copies and three others, in
    different 64-tile slices."""
    O = _oracle()
    src = Source(O, 31, 15, 9400)
    c = Case("C4", 31, 15, c4_world.__doc__, env={"DCN_TILE_WINDOWS": str(TINY)})
    slice_windows = 64 * TINY
    for n_tiles in (LDS_WALK_MAX_TILES, LDS_WALK_MAX_TILES + 1):
        n = n_tiles * TINY + src.l - 1
        r = _plant(src, src.random(n), 3 * slice_windows + 100, 9 * slice_windows + 300, 60)
        e = Entry(r, analyse(O, r, src.k, src.w))
        v = valid([e])
        twice = [h for h, m in collections.Counter(v).items() if m == 2]
        assert twice, "the planted copy gave no repeated minimizer"
        others = [v[5], v[len(v) // 2], v[-2]]
        c.add([e], keys=twice[:1] + others, mark=str(n_tiles))
    return c, Layout(O, c)


@functools.lru_cache(maxsize=None)
def c4_boundary_world():
    """C4, plan.hip pass A: `for (uint32_t t0 = 0; t0 < count && distinct < enough; t0 += 64)`.  One read of 1024 tiles from
    tile 0, so a 64-tile slice is a scan wave and has a run of its own.  47 bases from elsewhere are planted twice, in the
    last tile of slice 7 and early in slice 8: the hash they share is the last hit of one slice and the first of the next
    (the two other keys lie in other slices)."""
    O = _oracle()
    src = Source(O, 31, 15, 9450)
    slice_windows = 64 * TINY
    n = LDS_WALK_MAX_TILES * TINY + src.l - 1
    for _ in range(50):
        r = src.random(n)
        at = 8 * slice_windows - 10
        r = _plant(src, _plant(src, r, 5000, at, src.l + 2), 5000, at + src.l + 2, src.l + 2)
        e = Entry(r, analyse(O, r, src.k, src.w))
        c = Case("C4b", 31, 15, c4_boundary_world.__doc__, env={"DCN_TILE_WINDOWS": str(TINY)})
        c.add([e], keys=())
        L = Layout(O, c)
        last7 = [h for x in L.tiles[8 * 64 - 1:8 * 64] for h in x.items]
        first8 = [h for x in L.tiles[8 * 64:8 * 64 + 4] for h in x.items]
        both = [h for h in last7 if h is not None and h in first8]
        if both:
            v = valid([e])
            c.keys.update([both[0], v[3], v[len(v) * 12 // 16 + 5]])
            return c, L
    raise AssertionError("no read with a hash on both sides of the slice boundary")


# ---- C1: exact hashes through should_keep_hashes ------------------------------------------------------------------------------
C1_H = (1, 63, 64, 65, 255, 256, 257, 1024, LDS_SET_MAX - 1, LDS_SET_MAX, LDS_SET_MAX + 1, 2900)


def c1_units(seed=9500):
    """C1, plan.hip: unit_distinct_kernel's LDS pass (`j0 += 256`, `old == h[q]`), insert_run of the global set, `g_zero`.
    -> (units: list of u64 arrays, keys: u64 array without 0, names).  Every unit of H hashes has copies of earlier entries
    at its start (entry 1 = entry 0), across the 256-entry boundary (entries 256.. = entries 250..) and at its end."""
    rng = np.random.default_rng(seed)
    units, keys, names = [], [], []

    def fresh(n):
        return (rng.integers(1, 2**62, n, dtype=np.uint64) << np.uint64(1)) | np.uint64(1)

    def with_copies(h):
        h = h.copy()
        H = len(h)
        if H >= 2:
            h[1] = h[0]
        if H > 260:
            h[256:260] = h[250:254]
        if H >= 8:
            h[-1] = h[-5]
            h[-2] = h[2]
        return h
    for H in C1_H:
        a = with_copies(fresh(H))
        units.append(a)
        keys.append(a)
        names.append("all-%d" % H)
        b = with_copies(fresh(H))
        units.append(b)
        keys.append(np.array([x for i, x in enumerate(b.tolist()) if i % 3 != 2], np.uint64))  # a third are not keys
        names.append("third-%d" % H)
    for n_zero in (0, 1, 3):
        z = fresh(40)
        z[[5, 17, 33][:n_zero]] = 0
        units.append(z)
        keys.append(z[z != 0][::2])
        names.append("zero-%d" % n_zero)
    for i in range(300):   # many small units beside the large ones
        s = fresh(int(rng.integers(0, 9)))
        if len(s) >= 2 and i % 3 == 0:
            s[-1] = s[0]
        units.append(s)
        keys.append(s[::2])
        names.append("small-%d" % i)
    keys = np.unique(np.concatenate(keys))
    return units, keys[keys != 0], names


def c1_expected(units, keys, has_zero, abs_t, rel_t, deplete):
    O = _oracle()
    ks = set(keys.tolist()) | ({0} if has_zero else set())
    keep, hits, total = [], [], []
    for u in units:
        total.append(len(u))
        hits.append(len(set(u.tolist()) & ks))
        keep.append(O.meets_filtering_criteria(hits[-1], total[-1], abs_t, rel_t, deplete))
    return keep, hits, total


# ---- A7: the table walk -------------------------------------------------------------------------------------------------------
A7_SLOTS_PER_KEY = 2   # DCN_TABLE_SLOTS_PER_KEY of the case's index
A7_GROUPS = 15


def table_groups(n_keys, slots_per_key):
    """index_table.hip, dcn_table_groups_for with DCN_TABLE_SLOTS_PER_KEY set: `groups = 64; while (groups * DCN_GROUP_SLOTS <
    n_keys * s + 8) groups <<= 1`"""
    groups = _int("index_table.hip", r"uint64_t groups = (\d+);")
    while groups * group_slots() < n_keys * slots_per_key + 8:
        groups <<= 1
    return groups


@functools.lru_cache(maxsize=None)
def a7_world(k=31, w=15):
    """A7, dcn_probe.h through scan.hip: `while (r < 0) { grp[u] = (grp[u] + 1) & a.table.group_mask; ...}` in phase B and in
    probe_item.  Fifteen times four single-window reads whose hashes have one home group among the table's 64: three are
    keys, one more than the group holds, so whichever the build displaced is found one group on (or further), and the
    fourth's walk starts in a full group and must end "absent".  `single`: every read a unit (decisions-only: the
    early-out's probe_item); `fours`: each four a unit (phase B and the ring).  -> (single, fours, groups, quadruples)"""
    O = _oracle()
    src = Source(O, k, w, 9600 + 100 * k + w)
    S = group_slots()
    G = table_groups(3 * A7_GROUPS, A7_SLOTS_PER_KEY)
    by_home, quads, done = collections.defaultdict(list), [], set()
    while len(quads) < A7_GROUPS:
        e = src.single()
        g = int(group_of(np.array(e.items, np.uint64), G)[0])
        if g in done:
            continue
        by_home[g].append(e)
        if len(by_home[g]) == S + 2:  # (one quadruple per home group)
            quads.append(by_home[g])
            done.add(g)
    single = Case("A7", k, w, a7_world.__doc__, env={"DCN_TABLE_SLOTS_PER_KEY": str(A7_SLOTS_PER_KEY)})
    fours = Case("A7u", k, w, a7_world.__doc__, env=single.env)
    for q in quads:
        keys = [h for e in q[:S + 1] for h in e.items]
        for e in q:
            single.add([e], keys=keys)
        fours.add(q + q[:1], keys=keys)
    single.thresholds = fours.thresholds = ((1, 0.0, False), (1, 0.0, True), (2, 0.5, False))
    return single, fours, G, quads


# ---- A8: the short path ---------------------------------------------------------------------------------------------------------
A8_DISTANCES = (1, 2, 3, 4, 5)


@functools.lru_cache(maxsize=None)
def a8_world():
    """A8, scan.hip scan_short / scan_body<SHORT>: the ring compare inside one read, and after a mid-scan flush `if (sh.lok[uslot]
    || (SHORT && !enrol))`: a read without a hit is decided by the scan kernel, a read with hits goes to the work list,
    its run sized by run_cap from the offsets.  No unit_id, no read longer than DCN_SHORT_LMAX; read r is lane r % 64 of
    wave r // 64.  `dups`: 64 reads, a short period repeated, whose lists repeat hashes at hit distances 1 to 5 and
    more (as the oracle reports them), every hash a key.  `flush64` / `flush65`: a periodic read of 140 bases in lane 10
    beside 63 (64) reads: a third of three items without a key, a third with keys, a third periodic reads of `dups` (a
    hash hit several times inside the read, every hash a key).  -> {name: (reads, keys)}"""
    O = _oracle()
    src = Source(O, 31, 15, 9700)
    out = {}
    dups, keys, found = [], set(), set()
    p = 5
    want = set(A8_DISTANCES) | {8}
    while len(dups) < WAVE:
        per = src.random(p)
        r = (per * 40)[:int(src.rng.integers(120, SHORT_LMAX + 1))]
        items = analyse(O, r, 31, 15)
        p = p + 1 if p < 75 else 5
        d = set(distances(list(items)))
        if None in items or len(items) > flush_above(15) or not d or (want - found and not d & (want - found)):
            continue  # (while a wanted distance is missing, only a read that has one is taken)
        dups.append(Entry(r, items))
        keys.update(items)
        found.update(d)
    assert want <= found, sorted(found)
    out["dups"] = (dups, keys)
    clean = src.fill(3 * 64, 64)
    for i in range(1, 64, 3):  # every third a read of `dups`: the same hash as a hit twice and more inside one read
        clean[i] = dups[i]
    low = src.low_complexity()
    assert len(low.read) <= SHORT_LMAX
    ck = {h for i, e in enumerate(clean) if i % 3 for h in (e.items if i % 3 == 1 else e.items[::2])}
    out["flush64"] = (clean[:10] + [low] + clean[10:63], ck)
    out["flush65"] = (clean[:10] + [low] + clean[10:64], ck)
    return out
