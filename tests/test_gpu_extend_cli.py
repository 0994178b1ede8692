"""`deacon-hip extend` end to end on the input of tests/test_gpu_align_cli.py.  The placements are those `deacon-hip map`
prints for the same arguments; the model of tests/_extend_worker.py extends them; the PAF is compared line for line with
align's line for the extended extents (tests/_align_worker.py, tests/_verify_worker.py) followed by the four tags, and
--pileup / --sites with the model of tests/_pileup_worker.py over those lines.  The summary, small batches under
DCN_CLI_ALIGN_BATCH_BASES, .gz and stdin inputs, and align's and pileup's own output.  Every comparison is exact."""
import json
import os
import re

import numpy as np
import pytest

import _align_worker as AW
import _extend_worker as XW
import _verify_worker as VW
from conftest import revcomp
from test_gpu_align_cli import NAMES, data  # noqa: F401  (the fixture: three 20 kbp records, 200 reads)
from test_gpu_pileup_cli import model as pile_model, pileup_text, run, sites_text

pytestmark = pytest.mark.gpu

ROW = [("record", np.uint32), ("reverse", np.uint32), ("read_start", np.uint32), ("read_end", np.uint32), ("ref_start", np.uint64),
       ("ref_end", np.uint64)]
K = 31


def expected_paf(map_paf, genomes, reads, **kw):
    """map's lines -> extend's lines: the model's coordinates, align's columns 10 and 11, ve / NM / cg, then xl xr cl cr
    -> (the text, rows_extended, bases_gained, bases_clipped, full_length_rows, the extension)"""
    lines = [line.split("\t") for line in map_paf.decode().splitlines()]
    rows = np.zeros(len(lines), ROW)
    owner = []
    for t, c in enumerate(lines):
        rows[t] = (NAMES.index(c[5]), c[4] == "-", int(c[2]), int(c[3]), int(c[7]), int(c[8]))
        owner.append(int(c[0][4:]))
    counts = np.bincount(owner, minlength=len(reads))
    assert owner == sorted(owner)  # (map prints the reads in their order: the rows of a read are together)
    xrows, ext = XW.extend_rows(reads, genomes, rows, row_offsets=np.concatenate([[0], np.cumsum(counts)]), **kw)
    out, n_ext, gained, clipped, full = [], 0, 0, 0, 0
    for t, c in enumerate(lines):
        L, rev = int(c[1]), c[4] == "-"
        rs, re_, fs, fe = (int(xrows[name][t]) for name in ("read_start", "read_end", "ref_start", "ref_end"))
        lo, hi = int(c[2]) - rs, re_ - int(c[3])
        n_ext += lo + hi > 0
        gained += lo + hi
        clipped += rs + L - re_
        full += rs == 0 and re_ == L
        S = reads[owner[t]][rs:re_]
        S = revcomp(S) if rev else S
        d, runs = AW.align_pair(S, genomes[int(rows["record"][t])][fs:fe])
        votes = int(dict(x.split(":", 2)[::2] for x in c[12:])["cm"])
        if d <= VW.threshold(re_ - rs, fe - fs):
            text = AW.cigar_text(runs)
            ops = [(int(n), op) for n, op in re.findall(r"(\d+)([=XID])", text)]
            col10, col11 = sum(n for n, op in ops if op == "="), sum(n for n, _ in ops)
            more = ["ve:i:1", "NM:i:%d" % d, "cg:Z:" + (text or "*")]
        else:
            col10, col11, more = min(votes * K, re_ - rs), max(re_ - rs, fe - fs), ["ve:i:0"]
        tags = ["xl:i:%d" % (hi if rev else lo), "xr:i:%d" % (lo if rev else hi), "cl:i:%d" % (L - re_ if rev else rs), "cr:i:%d" % (rs if rev else L - re_)]
        out.append("\t".join(c[:2] + [str(rs), str(re_)] + c[4:7] + [str(fs), str(fe), str(col10), str(col11)] + c[11:] + more + tags))
    return ("\n".join(out) + "\n").encode(), n_ext, gained, clipped, full, ext


def test_paf_pileup_sites_and_summary_against_the_model(data):  # noqa: F811
    d, genomes, reads = data
    map_paf = run(["map", d / "ref.fa", d / "reads.fq", "-q"]).stdout
    want, n_ext, gained, clipped, full, ext = expected_paf(map_paf, genomes, reads)
    assert n_ext > 100 and gained > 1000 and full > 50 and (ext["left_edits"] > 0).any()
    p = run(["extend", d / "ref.fa", d / "reads.fq", "-q", "-o", "-", "--pileup", d / "pile.tsv", "--sites", d / "sites.tsv", "-s", d / "x.json",
             "--min-depth", "1"])
    got, exp = p.stdout.decode().splitlines(), want.decode().splitlines()
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g == e
    assert p.stdout == want
    counts, selected, added = pile_model(p.stdout, genomes, reads)  # (the lines carry the extended extents and their cg)
    assert (d / "pile.tsv").read_bytes() == pileup_text(counts, genomes)
    want_sites, n_sites = sites_text(counts, genomes, min_depth=1)
    assert (d / "sites.tsv").read_bytes() == want_sites
    s = json.load(open(d / "x.json"))
    assert (s["penalty"], s["end_bonus"], s["ext_max_edits"]) == (6, 4, 1023)
    assert (s["rows_extended"], s["bases_gained"], s["bases_clipped"], s["full_length_rows"]) == (n_ext, gained, clipped, full)
    assert (s["rows_selected"], s["rows_added"], s["sites"]) == (selected, added, n_sites)
    assert s["verified"] == sum("ve:i:1" in line for line in got) and s["placements"] == len(got) and s["cigar_ops"] > 0
    # the pileup over the original rows is lower
    plain = run(["pileup", d / "ref.fa", d / "reads.fq", "-q"]).stdout
    assert plain != (d / "pile.tsv").read_bytes() and plain.count(b"\n") < (d / "pile.tsv").read_bytes().count(b"\n")
    # the same bytes in small batches, from .gz and from stdin
    small = run(["extend", d / "ref.fa", d / "reads.fq", "-q", "-o", "-", "--pileup", d / "small.tsv"], env={"DCN_CLI_ALIGN_BATCH_BASES": "20000"})
    assert small.stdout == want and (d / "small.tsv").read_bytes() == pileup_text(pile_model(want, genomes, reads)[0], genomes)
    assert run(["extend", d / "ref.fa", d / "reads.fq.gz", "-q", "-o", "-"]).stdout == want
    with open(d / "reads.fq", "rb") as f:
        assert run(["extend", d / "ref.fa", "-q", "-o", d / "out.paf"], stdin=f).stdout == b"" and (d / "out.paf").read_bytes() == want
    # without -o there is no PAF; without -q the tool says what it did
    loud = run(["extend", d / "ref.fa", d / "reads.fq", "-s", d / "y.json"])
    assert loud.stdout == b"" and f"Extended {n_ext} of {len(got)} placements by {gained} bases".encode() in loud.stderr
    y = json.load(open(d / "y.json"))
    assert (y["rows_extended"], y["verified"]) == (n_ext, s["verified"]) and "cigar_ops" not in y and "rows_added" not in y


def test_options_change_the_extension(data):  # noqa: F811
    d, genomes, reads = data
    map_paf = run(["map", d / "ref.fa", d / "reads.fq", "-q"]).stdout
    base = expected_paf(map_paf, genomes, reads)[0]
    seen = {base}
    for opts, kw in ((["--penalty", "2", "--end-bonus", "0"], dict(penalty=2, end_bonus=0)), (["--ext-max-edits", "0"], dict(max_edits=0)),
                     (["--end-bonus", "40"], dict(end_bonus=40))):
        want = expected_paf(map_paf, genomes, reads, **kw)[0]
        seen.add(want)
        assert run(["extend", d / "ref.fa", d / "reads.fq", "-q", "-o", "-"] + opts).stdout == want
    assert len(seen) >= 3  # (the options are not without effect on this input)


def test_align_and_pileup_are_what_they_were(data):  # noqa: F811
    """align's lines carry none of extend's tags and are map's placements, unextended; both refuse extend's options"""
    d, genomes, reads = data
    map_paf = run(["map", d / "ref.fa", d / "reads.fq", "-q"]).stdout.decode().splitlines()
    align_paf = run(["align", d / "ref.fa", d / "reads.fq", "-q"]).stdout.decode().splitlines()
    assert len(map_paf) == len(align_paf) and not any("xl:i:" in line or "cl:i:" in line for line in align_paf)
    for m, a in zip(map_paf, align_paf):
        m, a = m.split("\t"), a.split("\t")
        assert m[:9] == a[:9] and m[11:18] == a[11:18]
    import subprocess
    from test_gpu_pileup_cli import CLI
    for sub in ("align", "pileup", "verify", "map"):
        for opt in ("--penalty", "--end-bonus", "--ext-max-edits", "--pileup"):
            q = subprocess.run([CLI, sub, "ref.fa", opt, "3"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
            assert (q.returncode, q.stderr) == (1, "Error: unexpected argument '%s'\n" % opt)
