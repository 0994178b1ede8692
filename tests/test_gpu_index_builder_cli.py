"""`deacon-hip index build --min-count / --max-count / --count-hist`: the input goes batch by batch into a counting
builder; the index file and the histogram equal the library's.  Without the options the command is the plain build."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, random_reads, revcomp

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")


def _run(args, **env):
    p = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert p.returncode == 0, (args, p.stderr[-3000:])
    return p


@pytest.fixture(scope="module")
def reads():
    rng = np.random.default_rng(702)
    genome = random_reads(rng, 1, 20_000, 20_000)[0]
    out = []
    for i in range(2000):
        at = int(rng.integers(0, len(genome) - 150))
        r = genome[at:at + 150]
        out.append(revcomp(r) if i % 2 else r)
    return out


def _fastq(reads):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))


@pytest.mark.parametrize("gz", [False, True])
def test_min_count_and_histogram_equal_the_library(dcn, reads, tmp_path, gz):
    b = dcn.IndexBuilder()
    b.add(reads)
    want_keys = sorted(b.finish(2, 0).keys().tolist())
    _, counts = b.counts()
    want_hist = {int(c): int(n) for c, n in zip(*np.unique(counts, return_counts=True))}
    fq = tmp_path / ("reads.fastq.gz" if gz else "reads.fastq")
    fq.write_bytes(gzip.compress(_fastq(reads)) if gz else _fastq(reads))
    out, hist = tmp_path / "out.idx", tmp_path / "hist.tsv"
    # batches of about 20 kbp: fifteen add calls
    p = _run(["index", "build", str(fq), "-o", str(out), "-q", "--min-count", "2", "--count-hist", str(hist)],
             DCN_CLI_BUILD_BATCH_BASES="20000")
    assert sorted(dcn.Index.from_file(str(out)).keys().tolist()) == want_keys
    got_hist = {int(c): int(n) for c, n in (line.split("\t") for line in hist.read_text().splitlines())}
    assert got_hist == want_hist
    info = b.info()
    line = [ln for ln in p.stderr.splitlines() if ln.startswith("Counted ")]
    assert len(line) == 1, p.stderr
    assert (f"Counted {info['n_keys']} minimizers ({info['n_occurrences']} occurrences) from 2000 sequence(s) (300000bp): "
            f"kept {len(want_keys)}, dropped {info['n_keys'] - len(want_keys)} below --min-count, 0 above --max-count") == line[0]


def test_count_hist_alone_keeps_everything_and_max_count_drops_repeats(dcn, reads, tmp_path):
    fq = tmp_path / "reads.fastq"
    fq.write_bytes(_fastq(reads))
    b = dcn.IndexBuilder()
    b.add(reads)
    out = tmp_path / "all.idx"
    p = _run(["index", "build", str(fq), "-o", str(out), "-q", "--count-hist", "-"])
    assert sorted(dcn.Index.from_file(str(out)).keys().tolist()) == sorted(b.finish(1, 0).keys().tolist())
    assert p.stdout.splitlines()[0].split("\t")[0] == "1"
    _run(["index", "build", str(fq), "-o", str(out), "-q", "--min-count", "3", "--max-count", "10"])
    assert sorted(dcn.Index.from_file(str(out)).keys().tolist()) == sorted(b.finish(3, 10).keys().tolist())


def _decode_index_file(raw):
    """(bytes of the header up to and including the key count, keys in file order) of a format-2 index file: version, k,
    w, then the count and every key as bincode varints (< 251: one byte; 0xFB u16; 0xFC u32; 0xFD u64, little endian)"""
    def varint(at):
        b = raw[at]
        if b < 251:
            return b, at + 1
        size = {0xFB: 2, 0xFC: 4, 0xFD: 8}[b]
        return int.from_bytes(raw[at + 1:at + 1 + size], "little"), at + 1 + size
    n, at = varint(3)
    head, keys = raw[:at], []
    for _ in range(n):
        key, at = varint(at)
        keys.append(key)
    assert at == len(raw)
    return head, keys


def test_without_the_options_the_output_is_the_plain_build(dcn, reads, tmp_path):
    """Without the three options the command runs the plain build: its file against the one written from dcn_index_build's
    index of the same sequences with the tool's capacity hint (bases / 4 + 1024).  Everything about the file that is
    determined by the input is compared: the whole header with the key count, the file's length, and the keys as a
    multiset.  The ORDER of the keys in a file is not determined by the input, in this or any earlier version: the file
    lists the table's keys as export_keys_kernel compacts them, each wave taking the next range of the output with an
    atomicAdd on one cursor, so waves land in the order they happen to run (a wave takes 1,024 slots: this table is over a
    hundred such spans), and which of two keys of one group gets the group's first slot is decided by a compare-and-swap race at insert.  Two
    runs of one binary on one input need not give the same bytes, so no byte-for-byte comparison exists to be made."""
    some = reads[:400]
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(some)))
    out, lib_out = tmp_path / "cli.idx", tmp_path / "lib.idx"
    p = _run(["index", "build", str(fa), "-o", str(out), "-q"])
    assert "Counted " not in p.stderr and "Indexed " in p.stderr and "capacity=400M" in p.stderr
    idx = dcn.Index.build(some, capacity_keys=sum(len(r) for r in some) // 4 + 1024)
    idx.write(str(lib_out))
    got, want = out.read_bytes(), lib_out.read_bytes()
    got_head, got_keys = _decode_index_file(got)
    want_head, want_keys = _decode_index_file(want)
    assert got_head == want_head and len(got_head) > 3 and got_head[:3] == bytes([2, 31, 15])
    assert len(got) == len(want)
    assert len(set(got_keys)) == len(got_keys) == idx.n_keys > 1000
    assert sorted(got_keys) == sorted(want_keys) == sorted(idx.keys().tolist())
