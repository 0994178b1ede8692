"""The model of duplicate marking (THE DEFINITION OF A DUPLICATE, rules D1-D7 of include/deacon_hip.h) and what its tests
share: a dict from key tuples to the smallest ordinal, fed unit by unit in input order; rows built by hand, field by field
(no placement is needed to test the library call); and a generator of random units with a seeded rate of duplication.
Nothing here looks at the device or at csrc/dcn_duplicates.h."""
import numpy as np

UNPLACED = 0xFFFFFFFF
NO_FIRST = 2 ** 64 - 1


def end_of(row, read_len, both_ends):
    """D3: row = (record, reverse, read_start, read_end, ref_start, ref_end) -> the end in D4's tuple order
    (record, pos5, reverse[, pos3])"""
    record, reverse, read_start, read_end, ref_start, ref_end = (int(x) for x in row)
    tail = read_len - read_end
    if not reverse:
        pos5, pos3 = ref_start - read_start, ref_end + tail
    else:
        pos5, pos3 = ref_end + read_start, ref_start - tail
    return (record, pos5, reverse, pos3) if both_ends else (record, pos5, reverse)


def read_end_of(rows, read_len, both_ends):
    """the end of a read from its rows in order (each a 6-tuple, or None / record == UNPLACED for an unplaced row), or None"""
    for row in rows:
        if row is not None and int(row[0]) != UNPLACED:
            return end_of(row, read_len, both_ends)
    return None


def key_of(ends, paired, both_ends):
    """D4: ends = the ends of the unit's reads (None for a read without one) -> a hashable key, or None"""
    have = sorted(e for e in ends if e is not None)
    if not have:
        return None
    return (bool(paired), bool(both_ends), len(have), tuple(have))


class Model:
    """D1, D2, D5, D6"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.first, self.seen, self.keyed = {}, 0, 0

    def info(self):
        return self.seen, self.keyed, len(self.first)

    def mark(self, lengths, reads_rows, paired=False, both_ends=False):
        """lengths[r] and reads_rows[r] (the 6-tuples or Nones of read r, in order) -> (dup list, first list) per unit"""
        per = 2 if paired else 1
        assert len(lengths) == len(reads_rows) and len(lengths) % per == 0
        keys = []
        for u in range(len(lengths) // per):
            ends = [read_end_of(reads_rows[r], int(lengths[r]), both_ends) for r in range(per * u, per * u + per)]
            keys.append(key_of(ends, paired, both_ends))
        for u, key in enumerate(keys):  # the call's units go in first (D5) ...
            if key is not None:
                self.keyed += 1
                self.first.setdefault(key, self.seen + u)
        dup, first = [], []
        for u, key in enumerate(keys):  # ... then every unit looks its key up
            f = NO_FIRST if key is None else self.first[key]
            first.append(f)
            dup.append(1 if f < self.seen + u else 0)
        self.seen += len(keys)
        return dup, first


# ---- rows by hand ---------------------------------------------------------------------------------------------------------
def pack(dcn, dtype, lengths, reads_rows, with_row_offsets=None):
    """-> (offsets u64[n + 1], rows dtype[], row_offsets or None).  Without row_offsets every read has exactly one row.  The
    fields behind the 48-byte head, and votes / n_anchors / n_positions in it, are filled with a pattern that no rule reads."""
    offsets = np.zeros(len(lengths) + 1, np.uint64)
    offsets[1:] = np.cumsum(np.asarray(lengths, np.uint64))
    flat = [row for rows in reads_rows for row in rows]
    if with_row_offsets is None:
        with_row_offsets = any(len(rows) != 1 for rows in reads_rows)
    out = np.zeros(len(flat), dtype)
    for name in out.dtype.names:
        if name not in ("record", "reverse", "read_start", "read_end", "reserved", "ref_start", "ref_end"):
            out[name] = (np.arange(len(flat)) * 7 + 3).astype(out.dtype[name])
    for i, row in enumerate(flat):
        if row is None:
            out["record"][i] = UNPLACED
            out["ref_start"][i], out["ref_end"][i], out["read_end"][i] = 2 ** 63, 5, 2 ** 32 - 1  # (an unplaced row's fields are not looked at)
        else:
            for name, v in zip(("record", "reverse", "read_start", "read_end", "ref_start", "ref_end"), row):
                out[name][i] = v
    row_offsets = None
    if with_row_offsets:
        row_offsets = np.zeros(len(lengths) + 1, np.uint64)
        row_offsets[1:] = np.cumsum([len(rows) for rows in reads_rows])
    return offsets, out, row_offsets


def dtypes(dcn):
    """the three row types: strides 48, 64, 80"""
    d = [dcn.filter.PLACEMENT_DTYPE, dcn.filter.SPLIT_PLACEMENT_DTYPE, dcn.filter.PAIR_PLACEMENT_DTYPE]
    assert [x.itemsize for x in d] == [48, 64, 80]
    return d


def mark(dcn, amap, dtype, lengths, reads_rows, paired=False, both_ends=False, with_row_offsets=None):
    offsets, rows, row_offsets = pack(dcn, dtype, lengths, reads_rows, with_row_offsets)
    dup, first = amap.mark_duplicates(offsets, rows, row_offsets, paired=paired, both_ends=both_ends)
    return [int(x) for x in dup], [int(x) for x in first]


def check(dcn, amap, model, dtype, lengths, reads_rows, paired=False, both_ends=False, with_row_offsets=None):
    """one call on the device and on the model: flags, first and info must be equal; -> (dup, first)"""
    got = mark(dcn, amap, dtype, lengths, reads_rows, paired, both_ends, with_row_offsets)
    want = model.mark(lengths, reads_rows, paired, both_ends)
    assert got[0] == want[0], [(u, a, b) for u, (a, b) in enumerate(zip(got[0], want[0])) if a != b][:10]
    assert got[1] == want[1], [(u, a, b) for u, (a, b) in enumerate(zip(got[1], want[1])) if a != b][:10]
    assert amap.duplicates_info() == model.info()
    return got


# ---- random units -----------------------------------------------------------------------------------------------------------
def random_units(rng, n_units, dup_rate, rec_lens, paired=False, read_len=(60, 151), p_unplaced=0.05, p_split=0.2):
    """-> (lengths, reads_rows).  A unit is, with probability dup_rate, a copy of the fragment of an earlier unit (the same
    unclipped ends, clipped anew and, when paired, with its mates swapped half the time), else a fragment of its own: per read
    a record, a strand and an unclipped interval that lies inside the record with room for the clips.  A read is unplaced
    with probability p_unplaced and has, with probability p_split, an unplaced row in front and a second placement behind."""
    per = 2 if paired else 1
    frags, lengths, reads_rows = [], [], []

    def new_read():
        rec = int(rng.integers(0, len(rec_lens)))
        L = int(rng.integers(read_len[0], read_len[1]))
        span = L + int(rng.integers(-3, 4))  # the unclipped interval on the record: a few indels' worth off the read's length
        start = int(rng.integers(0, rec_lens[rec] - span + 1))
        return (rec, int(rng.integers(0, 2)), L, start, start + span)

    def clipped(fr):
        rec, rev, L, lo, hi = fr
        c5, c3 = (int(x) for x in rng.integers(0, 9, 2))
        if not rev:
            return (rec, rev, c5, L - c3, lo + c5, hi - c3)
        return (rec, rev, c5, L - c3, lo + c3, hi - c5)

    for u in range(n_units):
        if frags and rng.random() < dup_rate:  # (of a fragment with an end: copies of nothing would breed)
            fr = list(frags[int(rng.integers(0, len(frags)))])
            if paired and rng.random() < 0.5:
                fr.reverse()
        else:
            fr = [None if rng.random() < p_unplaced else new_read() for _ in range(per)]
        if any(f is not None for f in fr):
            frags.append(tuple(fr))
        for f in fr:
            if f is None:
                lengths.append(int(rng.integers(read_len[0], read_len[1])))
                reads_rows.append([None] if rng.random() < 0.5 else [])
                continue
            rows = [clipped(f)]
            if rng.random() < p_split:
                rows = [None] + rows + [(f[0], 1 - f[1], 0, 1, 0, 1)]
            lengths.append(f[2])
            reads_rows.append(rows)
    return lengths, reads_rows


# ---- a map to hang the set on -----------------------------------------------------------------------------------------------
REC_LENS = [1000, 1200, 700]


def make_map(oracle, dcn, keep_bases=True, rec_lens=REC_LENS, seed=77):
    """an AnchorMap over random records of the given lengths, with or without kept bases: the set needs neither the bases
    nor a pileup, only a map with that many records added"""
    import _verify_worker as VW
    from conftest import random_reads
    rng = np.random.default_rng(seed)
    records = [random_reads(rng, 1, n, n)[0] for n in rec_lens]
    return VW.build_map(oracle, dcn, records, 31, 15, keep_bases=keep_bases)


def split(lengths, reads_rows, cuts, per=1):
    """the batch cut into calls after the given numbers of units"""
    out, at = [], 0
    for c in list(cuts) + [len(lengths) // per]:
        out.append((lengths[at * per:c * per], reads_rows[at * per:c * per]))
        at = c
    return out
