"""Segments of reads (dcn_locate_batch, Locator, `deacon-hip mask`) against the definition carried as a model over the CPU
oracle: every expected value below comes from locate_model, never from the code under test.  Integers only, no tolerance."""
import ctypes as C
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, mutate, random_reads, revcomp

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
K, W = 31, 15


def locate_model(oracle, seq, k, w, label_of, prefix_length, max_gap, min_hits, member_mask=0xFFFFFFFF):
    hashes, positions = oracle.minimizer_hashes_and_positions(seq, k, w, prefix_length)
    hit = {}
    for h, p in zip(hashes, positions):
        L = label_of(int(h)) & member_mask
        if L:
            hit[int(p)] = L
    segs = []
    for p in sorted(hit):
        if segs and p <= segs[-1][1] + max_gap:
            s = segs[-1]
            segs[-1] = (s[0], p + k, s[2] + 1, s[3] | hit[p])
        else:
            segs.append((p, p + k, 1, hit[p]))
    return [s for s in segs if s[2] >= min_hits]


def plain_label(oidx):
    keys = set(oidx.keys().tolist())
    return lambda h: 1 if h in keys else 0


def set_label(oidx_list):
    ks = [set(o.keys().tolist()) for o in oidx_list]
    return lambda h: sum((h in s) << j for j, s in enumerate(ks))


def model_batch(oracle, reads, k, w, label_of, prefix_length, max_gap, min_hits, member_mask=0xFFFFFFFF):
    return [locate_model(oracle, r, k, w, label_of, prefix_length, max_gap, min_hits, member_mask) for r in reads]


def gpu_batch(oracle, loc, reads):
    b, o = oracle.concat_reads(reads)
    so, segs = loc.locate_batch(b, o)
    assert len(so) == len(reads) + 1 and so[0] == 0 and int(so[-1]) == len(segs)
    return [[tuple(int(x) for x in s) for s in segs[int(so[r]):int(so[r + 1])]] for r in range(len(reads))]


def assert_same(got, want):
    assert len(got) == len(want)
    for r, (g, m) in enumerate(zip(got, want)):
        assert g == m, (r, g[:4], m[:4])


@pytest.fixture(scope="module")
def genomes():
    rng = np.random.default_rng(71)
    return random_reads(rng, 3, 60_000, 60_000)


def _member_seqs(genomes):
    g0, g1, g2 = genomes
    return [[g0, g1[:30_000]], [g1], [g2]]


@pytest.fixture(scope="module")
def members(oracle, dcn, genomes):
    out = []
    for seqs in _member_seqs(genomes):
        o = oracle.Index.build(seqs, k=K, w=W)
        out.append((o, dcn.Index.from_keys(o.keys(), K, W)))
    return out


@pytest.fixture(scope="module")
def plain(oracle, dcn, genomes):
    """an index over the first two genomes: slices of the third never hit"""
    o = oracle.Index.build([genomes[0], genomes[1]], k=K, w=W)
    return o, dcn.Index.from_keys(o.keys(), K, W)


def sample(rng, genomes, n, lo, hi, p_n=0.002):
    reads = []
    for _ in range(n):
        ln = int(rng.integers(lo, hi + 1))
        g = genomes[int(rng.integers(0, len(genomes)))]
        if rng.random() < 0.75 and ln < len(g):
            s = int(rng.integers(0, len(g) - ln))
            r = mutate(rng, g[s:s + ln], 0.01)
            if rng.random() < 0.5:
                r = revcomp(r)
        else:
            r = random_reads(rng, 1, ln, ln)[0]
        a = np.frombuffer(r, dtype=np.uint8).copy()
        if ln:
            a[rng.random(ln) < p_n] = ord("N")
            if rng.random() < 0.1:  # an N run
                s = int(rng.integers(0, ln))
                a[s:s + 40] = ord("N")
        reads.append(a.tobytes())
    return reads


def edge_reads(genomes, k, w):
    l = k + w - 1
    return [b"", b"ACGT", b"A" * (k - 1), b"ACGTN" * 20, b"N" * 200, genomes[0][500:500 + l], genomes[1][77:77 + k],
            genomes[0][900:900 + l + 1]]


def chimeric_reads(rng, genomes, n=22):
    """indexed slice (>= 3,000 unmutated bases) + random (>= 1,000) + slice of another genome, repeated up to the read's
    length: 5 to 200 kbp, every third one reverse-complemented"""
    reads = []
    for i in range(n):
        target = int(np.geomspace(5_000, 200_000, n)[i])
        parts, ln, j = [], 0, i
        while ln < target:
            g = genomes[j % 3] if parts else genomes[i % 2]  # the first part is of an indexed genome
            take = int(rng.integers(3_000, 50_000))
            s = int(rng.integers(0, len(g) - take))
            parts.append(g[s:s + take])
            parts.append(random_reads(rng, 1, 1_000, 4_000)[0])
            ln += len(parts[-1]) + len(parts[-2])
            j += 1
        parts.pop()  # ends with a slice
        if j % 3 == 0:  # ... of an indexed genome
            parts.append(genomes[1][100:3_300])
        r = b"".join(parts)
        reads.append(revcomp(r) if i % 3 == 2 else r)
    return reads


# ---- 1. short reads, plain index ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,w", [(31, 15), (41, 15)])
@pytest.mark.parametrize("max_gap,min_hits,prefix", [(None, 1, 0), (0, 1, 0), (None, 2, 0), (200, 3, 0), (None, 1, 60)])
def test_short_reads_plain_index(oracle, dcn, genomes, k, w, max_gap, min_hits, prefix):
    o = oracle.Index.build([genomes[0], genomes[1]], k=k, w=w)
    g = dcn.Index.from_keys(o.keys(), k, w)
    rng = np.random.default_rng(100 + min_hits * 7 + prefix + k)
    reads = sample(rng, genomes, 2500, 80, 160) + edge_reads(genomes, k, w)
    loc = dcn.Locator(g, max_gap=max_gap, min_hits=min_hits, prefix_length=prefix, max_batch_bases=1 << 21, max_batch_reads=1 << 13)
    gap = 2 * w - 1 if max_gap is None else max_gap
    assert loc.max_gap == gap
    want = model_batch(oracle, reads, k, w, plain_label(o), prefix, gap, min_hits)
    assert sum(1 for s in want if s) > 500
    if prefix == 0 and gap < 200:  # (an N run of 40 bases inside a matching read splits it)
        assert any(len(s) > 1 for s in want)
    assert_same(gpu_batch(oracle, loc, reads), want)
    assert all(m == 1 for segs in want for (_, _, _, m) in segs)


# ---- 2. long chimeric reads --------------------------------------------------------------------------------------------
def test_long_chimeric_reads(oracle, dcn, genomes, plain):
    o, g = plain
    rng = np.random.default_rng(2)
    reads = chimeric_reads(rng, genomes)
    gap = 2 * W - 1
    want = model_batch(oracle, reads, K, W, plain_label(o), 0, gap, 1)
    # conditions on the input, asserted on the model before the GPU is asked
    assert any(len(s) >= 2 for s in want)
    assert any(e - st > 64 * 32 for s in want for (st, e, _, _) in s)
    assert any(len(r) > 256 * 64 for r in reads)
    assert any(s and s[0][0] < W for s in want)
    assert any(s and s[-1][1] > len(r) - W for s, r in zip(want, reads))
    assert 2 * sum(1 for s in want if s) >= len(reads)
    assert min(len(r) for r in reads) >= 5_000 and max(len(r) for r in reads) >= 150_000
    loc = dcn.Locator(g, max_batch_bases=1 << 22, max_batch_reads=1 << 10)
    assert_same(gpu_batch(oracle, loc, reads), want)
    # other parameters on the same reads, mixed with short ones (lane and wave paths side by side)
    mixed = reads[:8] + sample(rng, genomes, 300, 30, 1500) + reads[8:]
    for max_gap, min_hits, prefix in ((0, 1, 0), (gap, 5, 0), (5000, 1, 0), (gap, 1, 7000)):
        loc = dcn.Locator(g, max_gap=max_gap, min_hits=min_hits, prefix_length=prefix, max_batch_bases=1 << 22,
                          max_batch_reads=1 << 10)
        assert_same(gpu_batch(oracle, loc, mixed), model_batch(oracle, mixed, K, W, plain_label(o), prefix, max_gap, min_hits))


def test_small_k_takes_the_bit_walk_for_every_read(oracle, dcn, genomes):
    """k + max_gap < 31: a bitmap word may hold hits of two segments, so long reads are walked by one lane too"""
    k, w = 15, 5
    o = oracle.Index.build([genomes[0][:20_000]], k=k, w=w)
    g = dcn.Index.from_keys(o.keys(), k, w)
    rng = np.random.default_rng(3)
    reads = [mutate(rng, genomes[0][1_000:9_000], 0.05), genomes[0][15_000:25_000], random_reads(rng, 1, 3000, 3000)[0]]
    for max_gap in (0, 9, 15, 16):
        want = model_batch(oracle, reads, k, w, plain_label(o), 0, max_gap, 1)
        assert len(want[0]) > 10
        loc = dcn.Locator(g, max_gap=max_gap, max_batch_bases=1 << 18, max_batch_reads=64)
        assert_same(gpu_batch(oracle, loc, reads), want)


# ---- 3. the derived default -------------------------------------------------------------------------------------------
def test_default_gap_joins_an_isolated_substitution(oracle, dcn, genomes, plain):
    o, g = plain
    rng = np.random.default_rng(4)
    reads = []
    for i in range(40):
        s = int(rng.integers(0, 59_000))
        a = bytearray(genomes[i % 2][s:s + 600])
        a[300] = ord("ACGT"[("ACGT".index(chr(a[300])) + 1 + i % 3) % 4])
        reads.append(revcomp(bytes(a)) if i % 2 else bytes(a))
    gap = 2 * W - 1
    want = model_batch(oracle, reads, K, W, plain_label(o), 0, gap, 1)
    for s in want:
        assert len(s) == 1 and s[0][0] < W and s[0][1] > 600 - W
    loc = dcn.Locator(g, max_batch_bases=1 << 18, max_batch_reads=256)
    assert_same(gpu_batch(oracle, loc, reads), want)


# ---- 4. labelled set ------------------------------------------------------------------------------------------------
def test_labelled_set_members_and_mask(oracle, dcn, genomes, members):
    ol = [o for o, _ in members]
    s = dcn.IndexSet([g for _, g in members])
    rng = np.random.default_rng(5)
    g0, g1, g2 = genomes
    chim = g0[2_000:6_000] + random_reads(rng, 1, 300, 300)[0] + g2[10_000:15_000]
    reads = sample(rng, genomes, 1500, 80, 400) + [chim, revcomp(chim), g1[25_000:35_000] + g2[:3000] + g0[:2000]]
    lab = set_label(ol)
    gap = 2 * W - 1
    want = model_batch(oracle, reads, K, W, lab, 0, gap, 1)
    seen = {m for sg in want for (_, _, _, m) in sg}
    assert {1, 3, 4} <= seen  # keys of one member, of the two overlapping ones, of the disjoint one
    c = want[len(reads) - 3]
    assert len(c) == 2 and c[0][3] == 1 and c[1][3] == 4  # member 0, then member 2
    loc = dcn.Locator(s, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
    assert_same(gpu_batch(oracle, loc, reads), want)
    for j in range(3):
        loc = dcn.Locator(s, member_mask=1 << j, min_hits=2, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
        wj = model_batch(oracle, reads, K, W, lab, 0, gap, 2, member_mask=1 << j)
        assert any(wj) and all(m == 1 << j for sg in wj for (_, _, _, m) in sg)
        assert_same(gpu_batch(oracle, loc, reads), wj)
        # ... which is what a plain index of that member gives, up to the label
        lp = dcn.Locator(members[j][1], min_hits=2, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
        assert_same([[(a, b, n, 1 << j) for (a, b, n, _) in sg] for sg in gpu_batch(oracle, lp, reads)], wj)


# ---- 5. seams ---------------------------------------------------------------------------------------------------------
def test_tile_seams(oracle, dcn, genomes, plain, monkeypatch):
    o, g = plain
    rng = np.random.default_rng(6)
    reads = sample(rng, genomes, 400, 60, 3000, p_n=0.0005) + [genomes[0][5:40_000], genomes[2][:9000] + genomes[1][40_000:]]
    rng.shuffle(reads)
    want = model_batch(oracle, reads, K, W, plain_label(o), 0, 2 * W - 1, 1)
    for tw in ("16", "100", None):
        if tw:
            monkeypatch.setenv("DCN_TILE_WINDOWS", tw)
        else:
            monkeypatch.delenv("DCN_TILE_WINDOWS")
        loc = dcn.Locator(g, max_batch_bases=1 << 21, max_batch_reads=1 << 10)
        assert_same(gpu_batch(oracle, loc, reads), want)


def test_read_boundaries_inside_bitmap_words(oracle, dcn, genomes, plain):
    o, g = plain
    rng = np.random.default_rng(7)
    reads = []
    for i in range(3000):  # many 1..70-base reads in a row, then reads of odd lengths that all hit
        ln = int(rng.integers(1, 71))
        s = int(rng.integers(0, 59_000))
        reads.append(genomes[i % 2][s:s + ln])
    for i in range(500):
        ln = int(rng.integers(45, 200)) | 1
        s = int(rng.integers(0, 59_000))
        reads.append(genomes[i % 2][s:s + ln])
    for max_gap in (0, 2 * W - 1):
        want = model_batch(oracle, reads, K, W, plain_label(o), 0, max_gap, 1)
        assert sum(1 for s in want if s) > 1000
        loc = dcn.Locator(g, max_gap=max_gap, max_batch_bases=1 << 20, max_batch_reads=1 << 12)
        assert_same(gpu_batch(oracle, loc, reads), want)


def test_no_hits_all_hits_and_consecutive_calls(oracle, dcn, genomes, plain):
    o, g = plain
    rng = np.random.default_rng(8)
    none = random_reads(rng, 800, 50, 400) + [genomes[2][:30_000]]
    every = [genomes[i % 2][s:s + ln] for i, (s, ln) in enumerate(zip(rng.integers(0, 50_000, 800), rng.integers(45, 5000, 800)))]
    lab = plain_label(o)
    w_none = model_batch(oracle, none, K, W, lab, 0, 2 * W - 1, 1)
    w_every = model_batch(oracle, every, K, W, lab, 0, 2 * W - 1, 1)
    assert not any(w_none)
    for r, s in zip(every, w_every):  # every window hits: one segment over (nearly) the whole read
        assert len(s) == 1 and s[0][0] < W and s[0][1] > len(r) - W
    loc = dcn.Locator(g, max_batch_bases=1 << 22, max_batch_reads=1 << 10)
    # the bitmap of one call must not leak into the next
    assert_same(gpu_batch(oracle, loc, every), w_every)
    assert_same(gpu_batch(oracle, loc, none), w_none)
    assert_same(gpu_batch(oracle, loc, every), w_every)
    assert_same(gpu_batch(oracle, loc, []), [])
    assert_same(gpu_batch(oracle, loc, [b""]), [[]])


def test_beside_filter_and_classify_on_one_context(oracle, dcn, genomes, members):
    ol = [o for o, _ in members]
    s = dcn.IndexSet([g for _, g in members])
    rng = np.random.default_rng(9)
    reads = sample(rng, genomes, 1500, 80, 600) + [genomes[1][:20_000]]
    b, o = oracle.concat_reads(reads)
    clf = dcn.Classifier(s, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
    N = dcn._native
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def filt():
        keep, hits, total = (np.zeros(len(reads), np.uint8), np.zeros(len(reads), np.uint32), np.zeros(len(reads), np.uint32))
        prm = N.Params(2, 0.01, 0, 0, 0)
        N.check(N.lib().dcn_filter_batch(clf._h, ptr(b), ptr(o), None, len(reads), C.byref(prm), ptr(keep), ptr(hits), ptr(total)))
        return keep.astype(bool).tolist(), hits.tolist(), total.tolist()

    def locate():
        prm = N.LocateParams(2 * W - 1, 1, 0xFFFFFFFF, 0, 0)
        so = np.zeros(len(reads) + 1, np.uint64)
        rc = N.lib().dcn_locate_batch(clf._h, s._h, ptr(b), ptr(o), len(reads), C.byref(prm), ptr(so), None, 0)
        assert rc in (0, N.DCN_ERR_CAPACITY)
        segs = np.zeros(max(int(so[-1]), 1), dcn.filter.SEGMENT_DTYPE)
        N.check(N.lib().dcn_locate_batch(clf._h, s._h, ptr(b), ptr(o), len(reads), C.byref(prm), ptr(so), ptr(segs), len(segs)))
        return [[tuple(int(x) for x in q) for q in segs[int(so[r]):int(so[r + 1])]] for r in range(len(reads))]

    union = oracle.Index(np.unique(np.concatenate([x.keys() for x in ol])), K, W)
    wk, wh, wt = oracle.filter_batch(union, b, o, None, abs_threshold=2, rel_threshold=0.01, deplete=False, threads=4)
    want_f = (wk.tolist(), wh.tolist(), wt.tolist())
    want_l = model_batch(oracle, reads, K, W, set_label(ol), 0, 2 * W - 1, 1)

    def classify_ok():
        match, hits, total = clf.classify_batch(b, o)
        for j, oj in enumerate(ol):
            keep, h, t = oracle.filter_batch(oj, b, o, None, abs_threshold=2, rel_threshold=0.01, deplete=False, threads=4)
            assert hits[:, j].tolist() == h.tolist() and total.tolist() == t.tolist()
            assert ((match >> j) & 1).astype(bool).tolist() == keep.tolist()

    assert filt() == want_f
    classify_ok()
    stats = clf.stats()
    assert_same(locate(), want_l)
    assert clf.stats() == stats
    assert filt() == want_f
    classify_ok()
    assert_same(locate(), want_l)


# ---- 6. capacity protocol ------------------------------------------------------------------------------------------------
def test_capacity_protocol(oracle, dcn, genomes, plain):
    o, g = plain
    rng = np.random.default_rng(10)
    reads = sample(rng, genomes, 1000, 80, 800)
    b, off = oracle.concat_reads(reads)
    want = model_batch(oracle, reads, K, W, plain_label(o), 0, 0, 1)
    want_off = np.concatenate([[0], np.cumsum([len(s) for s in want])]).tolist()
    needed = want_off[-1]
    assert needed > 100
    N = dcn._native
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    loc = dcn.Locator(g, max_gap=0, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
    prm = loc._params()
    GUARD = 0xA5A5A5A5
    for cap, rc_want in ((0, N.DCN_ERR_CAPACITY), (needed - 1, N.DCN_ERR_CAPACITY), (needed, 0)):
        so = np.full(len(reads) + 1, 7, np.uint64)
        buf = np.full((needed + 8) * 4, GUARD, np.uint32)
        rc = N.lib().dcn_locate_batch(loc._h, g._h, ptr(b), ptr(off), len(reads), C.byref(prm), ptr(so),
                                      ptr(buf) if cap else None, cap)
        assert rc == rc_want, (cap, rc, N.lib().dcn_last_error())
        assert so.tolist() == want_off
        assert (buf[cap * 4:] == GUARD).all()
        if rc == 0:
            got = buf[:needed * 4].reshape(-1, 4).tolist()
            assert got == [list(s) for sg in want for s in sg]
        else:
            assert b"capacity" in N.lib().dcn_last_error()
    # argument errors with a live context
    bad = N.LocateParams(0, 0, 0xFFFFFFFF, 0, 0)
    so = np.zeros(len(reads) + 1, np.uint64)
    assert N.lib().dcn_locate_batch(loc._h, g._h, ptr(b), ptr(off), len(reads), C.byref(bad), ptr(so), None, 0) == N.DCN_ERR_ARG
    assert N.lib().dcn_locate_batch(loc._h, None, ptr(b), ptr(off), len(reads), C.byref(prm), ptr(so), None, 0) == N.DCN_ERR_ARG
    g41 = dcn.Index.from_keys(np.arange(1, 100, dtype=np.uint64), 41, 15)
    assert N.lib().dcn_locate_batch(loc._h, g41._h, ptr(b), ptr(off), len(reads), C.byref(prm), ptr(so), None, 0) == N.DCN_ERR_ARG
    assert b"differ" in N.lib().dcn_last_error()
    small = dcn.Locator(g, max_batch_bases=1 << 12, max_batch_reads=16)
    with pytest.raises(dcn.DeaconHipError) as e:
        small.locate_batch(b, off)
    assert e.value.code == N.DCN_ERR_CAPACITY


# ---- 7. counters and profiling --------------------------------------------------------------------------------------------
def test_counters_unchanged_and_profile(oracle, dcn, genomes, plain):
    o, g = plain
    rng = np.random.default_rng(11)
    reads = sample(rng, genomes, 1000, 80, 300)
    b, off = oracle.concat_reads(reads)
    proc = dcn.FilterProcessor(g, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
    proc.filter_batch(b, off)
    s0 = proc.stats()
    assert s0["total_seqs"] == len(reads)
    N = dcn._native
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    prm = N.LocateParams(2 * W - 1, 1, 0xFFFFFFFF, 0, 0)
    so = np.zeros(len(reads) + 1, np.uint64)
    segs = np.zeros(len(reads) * 8, dcn.filter.SEGMENT_DTYPE)
    for _ in range(2):
        N.check(N.lib().dcn_locate_batch(proc._h, g._h, ptr(b), ptr(off), len(reads), C.byref(prm), ptr(so), ptr(segs), len(segs)))
    assert proc.stats() == s0
    loc = dcn.Locator(g, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
    assert all(v == 0 for v in loc.stats().values())
    loc.locate_batch(b, off)  # (its first call asks for the count, then calls again with room for it)
    loc.set_profiling(True)
    for _ in range(3):
        loc.locate_batch(b, off)
    ms, n = loc.profile()
    assert n == 3 and all(ms[st] > 0 for st in ("pack", "plan", "scan", "distinct", "finish"))
    assert all(v == 0 for v in loc.stats().values())


# ---- 8. the command line ------------------------------------------------------------------------------------------------
def _build_indexes(tmp_path, seq_lists):
    idx = []
    for j, seqs in enumerate(seq_lists):
        fa = tmp_path / f"g{j}.fa"
        fa.write_text("".join(f">s{i}\n{s.decode()}\n" for i, s in enumerate(seqs)))
        out = tmp_path / f"ref{j}.idx"
        subprocess.run([CLI, "index", "build", str(fa), "-o", str(out), "-q"], check=True, capture_output=True, timeout=300)
        idx.append(str(out))
    return idx


def _records(text, fastq):
    lines = text.split("\n")
    assert lines[-1] == ""
    step = 4 if fastq else 2
    return [lines[i:i + step] for i in range(0, len(lines) - 1, step)]


def _masked(seq, segs, soft):
    a = bytearray(seq)
    for (s, e, _, _) in segs:
        a[s:e] = (bytes(a[s:e]).lower() if soft else b"N" * (e - s))
    return bytes(a)


def _run_mask(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([CLI, "mask", *args, "-q"], capture_output=True, text=True, timeout=600, env=e)
    assert p.returncode == 0, p.stderr
    return p


def _check_cli(oracle, tmp_path, idx, labels, label_of, names, reads, fastq, gz, soft, max_gap, min_hits, prefix, env=None, tag=""):
    ext = "fq" if fastq else "fa"
    if fastq:
        text = "".join(f"@{nm} extra words\n{r.decode()}\n+\n{'I' * len(r)}\n" for nm, r in zip(names, reads))
    else:
        text = "".join(f">{nm} extra words\n{r.decode()}\n" for nm, r in zip(names, reads))
    inp = tmp_path / f"in{tag}.{ext}{'.gz' if gz else ''}"
    inp.write_bytes(gzip.compress(text.encode()) if gz else text.encode())
    out, bed, summ = tmp_path / f"out{tag}.{ext}", tmp_path / f"hits{tag}.bed", tmp_path / f"sum{tag}.json"
    args = sum((["-x", p] for p in idx), []) + [str(inp), "-o", str(out), "--bed", str(bed), "-s", str(summ)]
    gap = 2 * W - 1 if max_gap is None else max_gap
    if max_gap is not None:
        args += ["-g", str(max_gap)]
    if min_hits is not None:
        args += ["-a", str(min_hits)]
    if prefix:
        args += ["-p", str(prefix)]
    if soft:
        args += ["--soft"]
    _run_mask(args, env)
    mh = 2 if min_hits is None else min_hits
    want = model_batch(oracle, reads, K, W, label_of, prefix, gap, mh)
    # --bed: line for line
    names_of = lambda m: ",".join(labels[j] for j in range(len(labels)) if m >> j & 1)
    want_bed = [f"{nm}\t{s}\t{e}\t{n}\t{names_of(m)}" for nm, sg in zip(names, want) for (s, e, n, m) in sg]
    assert open(bed).read().splitlines() == want_bed
    # -o: every record, in order, exactly the segments replaced
    recs_in, recs_out = _records(text, fastq), _records(open(out).read(), fastq)
    assert len(recs_out) == len(recs_in) == len(reads)
    n_clean = 0
    for ri, ro, r, sg in zip(recs_in, recs_out, reads, want):
        assert ro[0] == ri[0] and ro[2:] == ri[2:]
        assert ro[1].encode() == _masked(r, sg, soft)
        if not sg:
            assert ro == ri
            n_clean += 1
    assert 0 < n_clean < len(reads)
    js = json.load(open(summ))
    assert js["reads"] == len(reads) and js["bases"] == sum(len(r) for r in reads)
    assert js["reads_with_segments"] == sum(1 for sg in want if sg)
    assert js["segments"] == sum(len(sg) for sg in want)
    assert js["masked_bases"] == sum(e - s for sg in want for (s, e, _, _) in sg)
    assert (js["max_gap"], js["min_hits"], js["prefix_length"], js["soft"]) == (gap, mh, prefix, soft)
    assert [x["name"] for x in js["indexes"]] == labels
    for j, x in enumerate(js["indexes"]):
        assert x["segments"] == sum(1 for sg in want for (_, _, _, m) in sg if m >> j & 1)
        assert x["masked_bases"] == sum(e - s for sg in want for (s, e, _, m) in sg if m >> j & 1)
    return open(out, "rb").read(), open(bed, "rb").read()


def test_cli_mask(oracle, genomes, tmp_path):
    rng = np.random.default_rng(12)
    seqs = _member_seqs(genomes)
    idx = _build_indexes(tmp_path, [seqs[0], seqs[2]])
    ol = [oracle.Index.build(seqs[0], k=K, w=W), oracle.Index.build(seqs[2], k=K, w=W)]
    g0, g1, g2 = genomes
    reads = sample(rng, genomes, 700, 60, 900, p_n=0.001) + [g0[1000:4000] + random_reads(rng, 1, 1500, 1500)[0] + g2[500:5000],
                                                            g1[31_000:50_000], b"ACGT", g2[20_000:52_000]]
    # lower-case input bases stay as they are outside segments
    reads[5] = reads[5].lower()
    names = [f"r{i}" for i in range(len(reads))]
    one = plain_label(ol[0])
    # plain index: FASTQ (gzip) hard mask with defaults, FASTA soft mask with options
    _check_cli(oracle, tmp_path, idx[:1], ["ref0"], one, names, reads, True, True, False, None, None, 0, tag="a")
    _check_cli(oracle, tmp_path, idx[:1], ["ref0"], one, names, reads, False, False, True, 0, 1, 0, tag="b")
    # two -x: labels, FASTA (gzip) and FASTQ
    two = set_label(ol)
    _check_cli(oracle, tmp_path, idx, ["ref0", "ref1"], two, names, reads, False, True, False, 100, 3, 0, tag="c")
    whole = _check_cli(oracle, tmp_path, idx, ["ref0", "ref1"], two, names, reads, True, False, True, None, 2, 2000, tag="d")
    # many batches, and records longer than the batch (the context is recreated): identical output
    small = _check_cli(oracle, tmp_path, idx, ["ref0", "ref1"], two, names, reads, True, False, True, None, 2, 2000,
                       env={"DCN_CLI_LOCATE_BATCH_BASES": "6000"}, tag="e")
    assert small == whole
    assert max(len(r) for r in reads) > 2 * 6000
