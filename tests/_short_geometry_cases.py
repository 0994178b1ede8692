"""The batches of tests/test_gpu_short_geometry.py: the short path of the scan kernel (scan.hip, scan_short) and the W = 15
instantiation of scan_body at every kind of k they serve, not only at k = 31.  CPU only: reads, seeds and what each batch must
contain; tests/test_short_geometry_cases.py checks with the oracle alone that they do contain it.

Why each k: 1 has no prologue, 138 windows in a read and a minimizer in most of them (every wave flushes in mid-scan, and a
read's hits outgrow a run of one slot per four bases); 3 has a flush in some waves only; 5 repeats keys within a read; 13 is
the largest k whose k-mers fit the lead-in of w - 1 = 14 bases; 15, 17 and 19 lie on either side of the prologue's first word
reload (k - 1 = 14, 16, 18 bases); 29 has the reload and table rotations next to those of k = 31.

k_batch has 14 full waves and a partial one, not seven: it holds 14 length kinds, and each has to meet lane 0 and lane 63
of some wave, of which a wave has one each."""
import functools

import numpy as np

import _place_worker as PW
import _short_fused_cases as SC
from conftest import random_reads

KS = (1, 3, 5, 13, 15, 17, 19, 29)
W, LMAX = SC.W, SC.LMAX
THRESHOLDS = SC.THRESHOLDS
LCAP_FLUSH = 25            # a lane past this many list entries makes its wave flush in mid-scan (DCN_LCAP - w, scan.hip)
STAGE_WORDS = 612          # DCN_STAGE_WORDS (scan.hip): 16-byte chunks a wave's staging area holds
ONE_SLOT_PER_WINDOW = (1, 3)  # k at which a read's hits outgrow a run of one slot per four bases: DCN_REC_SHIFT=0
LEAK_KS = (5, 13)          # k <= 13: a whole k-mer fits the 14 bases of lead-in
GENOME_BASES = 3000
# bases of the genome the index is built from: fewer at small k, where a few keys already meet most reads
INDEX_BASES = {3: 1000, 5: 100}
BACK_END = 2900  # a batch's last read ends here in the genome (its first read starts at front_at(k))
N_KINDS = 14
N_READS = 64 * N_KINDS + 10
POLY_A, AC_REPEAT, COPY, ENDS_IN_HIT, STARTS_WITH_HIT, LEAK_NEIGHBOUR, LEAK_READ = 100, 101, 102, 200, 201, 300, 301


def ell(k):
    """the shortest read with a window"""
    return k + W - 1


def run_cap(off, ln, shift=2):
    """hits a read's run of the record array holds at one slot per 2^shift bases (scan.hip, run_cap: windows + l - 1 is the
    read's length, less a trailing newline)"""
    return ((off + ln) >> shift) - (off >> shift)


@functools.lru_cache(maxsize=None)
def world(k):
    """(genome, sequences the index is built from)"""
    if k == SC.K:
        g = SC.genome()
        return g, (g,)
    g = random_reads(np.random.default_rng(500 + k), 1, GENOME_BASES, GENOME_BASES)[0]
    src = (g[:INDEX_BASES.get(k, len(g))],)
    if k == 1:
        # two canonical keys, of which the one with the smaller hash is the minimizer of every window it occurs in: the other
        # gets into the index (and into a read's hits) only through a window of 15 bases without the first
        src += (b"AT" * 20, b"CG" * 20)
    return g, src


def _oracle():
    from oracle import oracle as O
    O.lib()
    return O


@functools.lru_cache(maxsize=None)
def index_keys(k):
    g, src = world(k)
    return frozenset(_oracle().Index.build(list(src), k=k, w=W).keys().tolist())


def kmer_key(kmer):
    """the key of one k-mer (k odd): its only minimizer at w = 1"""
    h, _ = _oracle().minimizer_hashes_and_positions(kmer, len(kmer), 1)
    return int(h[0]) if len(h) else None


def hit_positions(read, k):
    """positions of the read's minimizers whose key is in the index of world(k)"""
    keys = index_keys(k)
    return [p for h, p in PW.occurrences(_oracle(), read, k, W) if h in keys]


@functools.lru_cache(maxsize=None)
def read_with_hit_at(k, ln, last):
    """a cut of the genome, ln bases, whose last (first) k-mer is a minimizer with a key of the index"""
    g, _ = world(k)
    want = ln - k if last else 0
    for s in range(300, len(g) - ln - 300):
        if want in hit_positions(g[s:s + ln], k):
            return g[s:s + ln]
    raise AssertionError(f"no cut of {ln} bases with a hit at {want} (k = {k})")


def _profile(read, k):
    """(minimizers, distinct keys of the index among them) of a read"""
    keys = index_keys(k)
    hs = [h for h, _ in PW.occurrences(_oracle(), read, k, W)]
    return len(hs), len({h for h in hs if h in keys})


@functools.lru_cache(maxsize=None)
def front_at(k):
    """where in the genome a batch's first read (LMAX bases) starts: the first place from 200 on at which the read with the 9
    or 15 bases in front of it taken for bases has other minimizers or other hits than the read alone"""
    g, _ = world(k)
    for at in range(200, 1000):
        alone = _profile(g[at:at + LMAX], k)
        if all(_profile(g[at - s:at + LMAX], k) != alone for s in (9, 15)):
            return at
    raise AssertionError(f"no such place (k = {k})")


def length_kinds(k):
    """(name, bases, ends in a newline): the lengths around k and l, each again with a newline behind it, and the longest"""
    l = ell(k)
    plain = [("0", 0), ("k-1", k - 1), ("k", k), ("l-1", l - 1), ("l", l), ("l+1", l + 1)]
    kinds = [("LMAX", LMAX, False)] + [(n, b, False) for n, b in plain] + [(n + "+nl", b, True) for n, b in plain]
    kinds.append(("LMAX-1+nl", LMAX - 1, True))
    assert len(kinds) == N_KINDS
    return kinds


def edge_slots(k):
    """[(read, kind name, bases, newline)]: kind i is read 0 of wave i and read 63 of wave (i + 5) % 14"""
    out = []
    for i, (name, bases, nl) in enumerate(length_kinds(k)):
        out.append((64 * i, name, bases, nl))
        out.append((64 * ((i + 5) % N_KINDS) + 63, name, bases, nl))
    return out


def _pure_stretch(rng, r, alphabet):
    """20 to 40 bases of the read (all of a shorter one) replaced by letters of one canonical 1-mer"""
    n = min(int(rng.integers(20, 41)), len(r))
    s = int(rng.integers(0, len(r) - n + 1))
    return r[:s] + random_reads(rng, 1, n, n, alphabet=alphabet)[0] + r[s + n:]


def _ordinary(rng, g, k, n, lmax=LMAX):
    """reads of l + 1 .. lmax bases, about half cut from the genome (0.5 % mutations, either strand), decorated.  k = 1: one
    read in four has only A and T, and one in four a stretch of one canonical 1-mer, so that reads differ in their hits"""
    out = []
    for i in range(n):
        ln = int(rng.integers(ell(k) + 1, lmax + 1))
        r = SC._read(rng, g, ln, rng.random() < 0.5)
        if k == 1 and i % 4 == 1:
            r = random_reads(rng, 1, ln, ln, alphabet=b"AT")[0]
        elif k == 1 and i % 4 == 2:
            r = _pure_stretch(rng, r, b"AT" if i % 8 == 2 else b"CG")
        out.append(SC._decorate(rng, r))
    return out


def leak_pair(k):
    """(neighbour, r): the neighbour's last 14 bases hold a k-mer of the index; r, directly behind it, has no hit at all, and
    would have one if its lead-in, those 14 bases, were scanned as part of it"""
    assert k in LEAK_KS
    g, src = world(k)
    p = max(hit_positions(src[0], k))  # the index sequence's last minimizer
    end = p + k + 1                    # one base behind the k-mer: it lies in bases -(k + 1) .. -2 of the neighbour
    neighbour = g[max(0, end - 120):end]
    rng = np.random.default_rng(600 + k)
    while True:
        r = random_reads(rng, 1, 120, 120)[0]
        if not hit_positions(r, k) and hit_positions(neighbour[-(W - 1):] + r, k):
            return neighbour, r


def k_batch(g, k):
    assert g is world(k)[0]
    rng = np.random.default_rng(400 + k)
    reads = _ordinary(rng, g, k, N_READS)
    for i, (pos, name, bases, nl) in enumerate(edge_slots(k)):
        at = front_at(k) + 37 * i
        # (l + 1 bases: a cut whose two windows have different minimizers, so that a window too few shows in the total)
        while bases == ell(k) + 1 and len(PW.occurrences(_oracle(), g[at:at + bases], k, W)) != 2:
            at += 1
        reads[pos] = g[at:at + bases] + (b"\n" if nl else b"")
    reads[POLY_A] = b"A" * LMAX
    reads[AC_REPEAT] = (b"AC" * LMAX)[:LMAX]
    reads[COPY] = g[1000:1000 + LMAX]
    reads[ENDS_IN_HIT] = read_with_hit_at(k, 120, True)
    reads[STARTS_WITH_HIT] = read_with_hit_at(k, 120, False)
    if k in LEAK_KS:
        reads[LEAK_NEIGHBOUR], reads[LEAK_READ] = leak_pair(k)
    reads[-1] = g[BACK_END - 120:BACK_END]
    assert reads[0] == g[front_at(k):front_at(k) + LMAX]
    return reads


def outside(k, shift):
    """the genome in front of a batch's first read (`shift` bases) and behind its last one (64 bases): what the bytes around
    the stream hold in the GPU test.  A kernel that took them for bases would find the genome's k-mers there."""
    g, _ = world(k)
    return g[front_at(k) - shift:front_at(k)], g[BACK_END:BACK_END + 64]


def full_wave_batch(g, j, k=SC.K):
    """wave 0: 63 reads of LMAX bases and one of LMAX - j; wave 1: 64 reads of LMAX, the last one ending in a hit; wave 2: 10
    reads.  Wave 1's first base lies at stream offset 64 * LMAX - j."""
    assert g is world(k)[0]
    rng = np.random.default_rng(700 + j)
    reads = [SC._read(rng, g, LMAX, i % 2 == 0) for i in range(128)] + _ordinary(rng, g, k, 10)
    reads[0] = g[front_at(k):front_at(k) + LMAX]
    reads[63] = reads[63][:LMAX - j]
    reads[127] = read_with_hit_at(k, LMAX, True)
    reads[-1] = g[BACK_END - 120:BACK_END]
    return reads


def short_lane_chunks(off, end, a16):
    """dcn_short_lane's two formulas (csrc/dcn_short_lane.h): first and last 16-byte chunk of a lane's span"""
    return (a16 + off - (W - 1)) >> 4, (a16 + end - 1) >> 4


def alternate_plan(g, k=5):
    """[(reads, unit_id or None, short)] in the order they are enqueued: short, long reads, short, paired, short"""
    batch = k_batch(g, k)
    rng = np.random.default_rng(800 + k)
    long_reads = [SC._read(rng, g, int(rng.integers(LMAX + 1, 400)), i % 2 == 0) for i in range(40)]
    paired = batch[320:520]
    uid = (np.arange(len(paired)) // 2).astype(np.uint32)
    return [(batch[:300], None, True), (long_reads, None, False), (batch[576:900], None, True), (paired, uid, False),
            (batch[64:193], None, True)]
