"""The batches of tests/test_gpu_short_offsets.py: short device batches whose reads the scan kernel takes straight from the
offsets (scan.hip, scan_short: read r is lane r % 64 of workgroup r // 64) and whose kept reads and bases it counts itself.
CPU only: reads, seeds and what each batch must contain; tests/test_short_offsets_cases.py checks with the oracle alone that
they do contain it."""
import numpy as np

import _short_fused_cases as SC

K, W, L, LMAX = SC.K, SC.W, SC.L, SC.LMAX
EDGE_SIZES = (64, 65, 128, 129)
# reads without a window: empty, below k, between k and l, and l bytes of which the last is a newline
NO_WINDOW_KINDS = ("empty", "below_k", "below_l", "newline")
POLY_A = b"A" * LMAX


def overflow_genome(g):
    """the genome of test 3: poly-A is in its index, so b"A" * LMAX has a hit in every window"""
    return g + b"A" * 400


def no_window_read(g, kind, at):
    if kind == "empty":
        return b""
    if kind == "below_k":
        return g[at:at + 30]
    if kind == "below_l":
        return g[at:at + L - 1]
    assert kind == "newline"
    return g[at:at + L - 1] + b"\n"


def _ordinary(rng, g, n):
    """reads with windows, about half of them from the genome; one in five ends in a newline"""
    out = []
    for _ in range(n):
        r = SC._read(rng, g, int(rng.integers(L + 1, LMAX)), rng.random() < 0.5)
        out.append(r + b"\n" if rng.random() < 0.2 else r)
    return out


def edge_positions(n):
    return sorted({0, 63, 64, n - 1} & set(range(n)))


def edge_batch(g, n):
    """Test 1: n reads; reads 0, 63, 64 and the last one have no window, the four kinds in turn (which kind comes first
    moves from batch to batch, so that each kind meets lane 0, lane 63 and a wave of one read)"""
    rng = np.random.default_rng(300 + n)
    reads = _ordinary(rng, g, n)
    rot = EDGE_SIZES.index(n)
    for i, p in enumerate(edge_positions(n)):
        reads[p] = no_window_read(g, NO_WINDOW_KINDS[(i + rot) % 4], 1000 * (i + 1))
    return reads


def idle_wave_batch(g):
    """Test 1: reads 64..127, a whole wave, have no window (lengths 0..44), between two ordinary waves"""
    rng = np.random.default_rng(310)
    reads = _ordinary(rng, g, 192)
    for i in range(64):
        reads[64 + i] = g[2000 + i:2000 + i + (i * (L - 1)) // 63]
    return reads


def empty_batch():
    """Test 1: 70 empty reads: a stream of no bases at all"""
    return [b""] * 70


def counters_batch(g, n=1000):
    """Test 2: kept and dropped reads, newline-terminated reads, and reads without a window of every kind"""
    rng = np.random.default_rng(320)
    reads = _ordinary(rng, g, n)
    for i in range(0, n, 9):
        reads[i] = no_window_read(g, NO_WINDOW_KINDS[(i // 9) % 4], int(rng.integers(0, len(g) - LMAX)))
    reads[500] = POLY_A  # more than a lane's list holds between flushes: its wave (448..511) goes through a mid-scan flush
    reads[501] = g[5000:5000 + LMAX]  # ... with hits in it: an exported unit
    return reads


OVERFLOW_WAVE_LANE0, OVERFLOW_WAVE_LANE63, IN_WAVE_POLY_A = 64, 191, 10


def overflow_batch(g):
    """Test 3: poly-A reads of LMAX bases at lane 0 of wave 1 and lane 63 of wave 2: a hit in each of their 108 windows, which
    their runs of the record array do not hold at one slot per four bases.  b"A" * 60 in wave 0 has 16 windows with one key and
    is resolved in its wave."""
    rng = np.random.default_rng(330)
    reads = _ordinary(rng, g, 200)
    reads[OVERFLOW_WAVE_LANE0] = POLY_A
    reads[OVERFLOW_WAVE_LANE63] = POLY_A
    reads[IN_WAVE_POLY_A] = b"A" * 60
    return reads


def stale_plan(g):
    """Test 4: (reads, short) in the order they are enqueued"""
    rng = np.random.default_rng(340)
    first = counters_batch(g)[:900]
    second = _ordinary(rng, g, 100)
    long_reads = [SC._read(rng, g, int(rng.integers(500, 3000)), i % 2 == 0) for i in range(40)]
    last = _ordinary(rng, g, 65)
    last[64] = b""
    return [(first, True), (second, True), (long_reads, False), (last, True)]
