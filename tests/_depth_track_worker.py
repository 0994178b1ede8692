"""The model of tests/test_gpu_depth_track*.py and the worker of their subprocess case.

Model (the statement of include/deacon_hip.h as a short function): per read, the distinct positions of
oracle.minimizer_hashes_and_positions(read, k, w, prefix_length); position p falls into bin p // bin_bases (bin 0 when
bin_bases is 0) of the read's ceil(len / bin_bases) bins (one when bin_bases is 0); a position is a key when its hash is
in a member the mask selects, and then adds d = min(depth, 65,535), capped at depth_cap when that is not 0.  Depths come
from a {key: depth} dict (tests/_depth_worker.py::occurrences), members are key sets.  Integers only.

As a program (python tests/_depth_track_worker.py seams) it runs one case in a process of its own, whose environment the
test has set (DCN_TILE_WINDOWS), and exits non-zero with a traceback when a check fails."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _depth_worker as W  # noqa: E402

SAT = 65535
FIELDS = ("n_positions", "n_keys", "n_observed", "max_depth", "sum_depth")
BIN_BASES = (0, 1, 31, 32, 33, 1000, 1 << 20)


class Model:
    """the positions of `reads` with the label and depth of each one's hash, binned on demand"""

    def __init__(self, O, reads, k, w, mkeys, depth, prefix=0):
        rid, pos, hs = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.uint64)]
        for r, read in enumerate(reads):
            h, p = O.minimizer_hashes_and_positions(read, k, w, prefix)
            if len(p):
                up, first = np.unique(p, return_index=True)  # a position the list repeats counts once
                rid.append(np.full(len(up), r, np.int64))
                pos.append(up.astype(np.int64))
                hs.append(np.asarray(h, np.uint64)[first])
        self.rid, self.pos, hs = np.concatenate(rid), np.concatenate(pos), np.concatenate(hs)
        self.lens = np.array([len(r) for r in reads], np.int64)
        label = {}
        for j, m in enumerate(mkeys):
            for key in (m.tolist() if isinstance(m, np.ndarray) else m):
                label[key] = label.get(key, 0) | (1 << j)
        keys = np.array(sorted(label), np.uint64)
        labels = np.array([label[key] for key in keys.tolist()], np.int64)
        depths = np.array([min(int(depth.get(key, 0)), SAT) for key in keys.tolist()], np.int64)
        if len(keys):
            at = np.minimum(np.searchsorted(keys, hs), len(keys) - 1)
            found = keys[at] == hs
            self.label = np.where(found, labels[at], 0)
            self.depth = np.where(found, depths[at], 0)
        else:
            self.label = self.depth = np.zeros(len(hs), np.int64)

    def bins(self, bin_bases, mask, cap=0):
        """(bin_offsets, {field: int64 array over all bins})"""
        B = int(bin_bases)
        nb = np.ones(len(self.lens), np.int64) if B == 0 else -(-self.lens // B)
        bo = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
        g = bo[self.rid] + (0 if B == 0 else self.pos // B)
        key = (self.label & mask) != 0
        d = np.where(key, self.depth, 0)
        if cap:
            d = np.minimum(d, cap)
        total = int(bo[-1])
        out = {"n_positions": np.bincount(g, minlength=total),
               "n_keys": np.bincount(g[key], minlength=total),
               "n_observed": np.bincount(g[key & (d > 0)], minlength=total),
               "max_depth": np.zeros(total, np.int64), "sum_depth": np.zeros(total, np.int64)}
        np.maximum.at(out["max_depth"], g, d)
        np.add.at(out["sum_depth"], g, d)
        return bo, out


def assert_track(got, want, what=()):
    """(bin_offsets, bins) of DepthTracker.track_batch against Model.bins"""
    (gbo, gbins), (wbo, wbins) = got, want
    assert gbo.dtype == np.uint64 and np.array_equal(gbo.astype(np.int64), wbo), ("bin_offsets",) + tuple(what)
    assert len(gbins) == int(wbo[-1]), ("bins",) + tuple(what)
    for f in FIELDS:
        g = gbins[f].astype(np.int64)
        if not np.array_equal(g, wbins[f]):
            bad = np.flatnonzero(g != wbins[f])
            raise AssertionError((f,) + tuple(what) + (len(bad), bad[:5].tolist(), g[bad[:5]].tolist(), wbins[f][bad[:5]].tolist()))


def tracked_reads(genomes, batch):
    """the three genomes, the batch's own reads, and a read with a trailing newline"""
    return list(genomes) + list(batch) + [genomes[0][500:700] + b"\n", genomes[1][100:131] + b"\n"]


def track(dcn, s, reads, O, **kw):
    b, o = O.concat_reads(reads)
    t = dcn.DepthTracker(s, max_batch_bases=1 << 20, max_batch_reads=1 << 12, **kw)
    try:
        return t.track_batch(b, o)
    finally:
        t.close()


# ---- subprocess case ----------------------------------------------------------------------------------------------
def case_seams(O, dcn):
    """the mixed batch with tiles of 16 windows (every read of 31 bases or more is cut into several tiles, each seam a
    carry window), at w = 15 and at w = 1: a position marked on both sides of a seam is one bit and one value"""
    assert os.environ.get("DCN_TILE_WINDOWS") == "16"
    genomes = W.make_genomes()
    batch = W.mixed_batch(genomes)
    reads = tracked_reads(genomes, batch)
    for w in (15, 1):
        mkeys, gl = W.build_members(O, dcn, genomes, 31, w)
        s = dcn.IndexSet(gl)
        s.enable_depth()
        clf = dcn.Classifier(s, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
        W.classify(O, clf, batch)
        clf.close()
        m = Model(O, reads, 31, w, mkeys, W.occurrences(O, batch, 31, w))
        n = 0
        for B in (0, 33, 1000):
            for mask in (7, 2):
                want = m.bins(B, mask)
                assert_track(track(dcn, s, reads, O, bin_bases=B, member=[j for j in range(3) if mask >> j & 1]), want, (w, B, mask))
                n += int(want[1]["n_keys"].sum())
        assert n > 10_000
        print(f"track seams w={w}: {n} keys in bins")


if __name__ == "__main__":
    import deacon_server_amd as dcn
    from oracle import oracle as O
    O.lib()
    {"seams": case_seams}[sys.argv[1]](O, dcn)
