"""The batches of tests/test_gpu_short_fused.py: device batches of short unpaired reads, which the scan kernel packs itself
(scan.hip, scan_short) instead of reading a packed stream.  CPU only: reads, seeds and what each batch must contain;
tests/test_short_fused_cases.py checks with the oracle alone that they do contain it."""
import numpy as np

from conftest import mutate, random_reads, revcomp

K, W = 31, 15
L = K + W - 1     # 45: the shortest read with a window
LMAX = 152        # the longest read of a short batch (include/deacon_hip.h, dcn_ctx_last_batch_short)
PLAN_BLOCK = 256  # reads per planning block of a batch below 2^19 reads (2,048 above)
THRESHOLDS = [(2, 0.01, False), (1, 0.0, True), (5, 0.3, True)]


def genome():
    return random_reads(np.random.default_rng(1), 1, 200_000, 200_000)[0]


def _read(rng, g, ln, host):
    if ln == 0:
        return b""
    if host:
        s = int(rng.integers(0, len(g) - ln))
        r = mutate(rng, g[s:s + ln], 0.005)
        return revcomp(r) if rng.random() < 0.5 else r
    return random_reads(rng, 1, ln, ln)[0]


def _decorate(rng, r):
    """N bases and lower-case letters at a read's start and end"""
    s = bytearray(r)
    if len(s) >= 4:
        what = int(rng.integers(0, 6))
        if what == 0:
            s[0] = ord("N")
        elif what == 1:
            s[-1] = ord("N")
        elif what == 2:
            s[0] |= 0x20
            s[1] |= 0x20
        elif what == 3:
            s[-1] |= 0x20
            s[-2] |= 0x20
    return bytes(s)


def seam_batch(g, seed=101, n=2 * 2048 + 17):
    """Test 1: lengths from {0, 10, 30 (< k), 31..44 (k <= len < l), 45, 46, 100..LMAX}: planning-block ranges are no multiples
    of 64 and the last wave is partial."""
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(n):
        c = rng.random()
        if c < 0.04:
            ln = 0
        elif c < 0.08:
            ln = 10
        elif c < 0.12:
            ln = 30
        elif c < 0.22:
            ln = int(rng.integers(31, 45))
        elif c < 0.26:
            ln = 45
        elif c < 0.30:
            ln = 46
        elif c < 0.34:
            ln = LMAX
        else:
            ln = int(rng.integers(100, LMAX + 1))
        reads.append(_decorate(rng, _read(rng, g, ln, rng.random() < 0.5)))
    # a stretch of reads without a tile (one wave then holds several runs of tiles), and low complexity: a minimizer per
    # window, more than a lane's list holds between flushes
    for i in range(600, 760):
        reads[i] = _read(rng, g, int(rng.integers(31, 45)), True) if i % 8 else _read(rng, g, 120, True)
    reads[1000] = b"A" * LMAX
    reads[1001] = (b"AC" * LMAX)[:LMAX]
    reads[2000] = g[5000:5000 + LMAX]  # an exact copy: every minimizer hits
    return reads


def newline_batch(g, seed=202):
    """Test 2: reads that end in a newline, of every length at which that changes the window count"""
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(300):
        ln = int(rng.integers(60, LMAX))
        r = _read(rng, g, ln, rng.random() < 0.6)
        reads.append(r + b"\n" if i % 2 == 0 else r)
    reads[10] = g[1000:1000 + L] + b"\n"           # l + 1 bytes: one window left
    reads[11] = g[2000:2000 + L - 1] + b"\n"       # l bytes: no window left, though the plan gave it a tile
    reads[12] = g[3000:3000 + K - 1] + b"\n"       # k bytes
    reads[13] = g[4000:4060] + b"\n" + g[4060:4120]  # a newline in the middle: an invalid base
    reads[14] = g[6000:6000 + LMAX - 1] + b"\n"    # LMAX bytes, the last a newline
    reads[15] = _read(rng, g, LMAX - 1, False) + b"\n"
    reads[70] = g[7000:7000 + L - 1] + b"\n"
    reads.append(g[8000:8100] + b"\n")             # the stream's last byte
    return reads


def expected_stats(reads, keep, unit_id=None):
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    keep = np.asarray(keep, dtype=bool)
    if unit_id is not None:
        keep = keep[np.asarray(unit_id)]
    return {"total_seqs": len(reads), "total_bp": int(lens.sum()), "output_bp": int(lens[keep].sum()),
            "filtered_bp": int(lens[~keep].sum()), "filtered_seqs": int((~keep).sum()),
            "output_seq_counter": int(keep.sum())}
