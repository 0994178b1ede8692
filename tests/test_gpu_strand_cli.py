"""`deacon-hip strand` end to end, file to file, on a reference of 3,000 bases under 150-base reads that start every 5 bases on
alternating strands (30-fold, 15 of each strand), error-free but for three planted variants:
  a heterozygous SNV that every forward read carries and no reverse read (an artefact's picture, under two-stranded coverage),
  a heterozygous SNV carried by every other read of each strand,
  a 2-base deletion that the reverse reads carry which have it 20 bases or more from their ends, and no forward read.
The first must be filtered strand_bias;one_strand, the second must PASS, the third is filtered too.  On every line ADF + ADR
is AD field by field, and ADF, ADR, SB and FILTER are what the --pileup columns of the same run and the rule of
tests/_strand_worker.py make of them.  With FILTER put back to PASS and SB, ADF, ADR, the five header lines and the four
pileup columns removed, every output is `deacon-hip normalize`'s, byte for byte.  Every comparison is exact."""
import json
import re

import numpy as np
import pytest

import _strand_worker as SW
from conftest import random_reads, revcomp
from test_gpu_pileup_cli import run

pytestmark = pytest.mark.gpu

LENGTH, READ, STEP = 3000, 150, 5
ONE_STRAND_SNV, BALANCED_SNV, DELETION = 802, 1602, 2300  # (no read begins or ends on an SNV: extend would clip it)
NEW_HEADER = ("##FILTER=<ID=strand_bias,", "##FILTER=<ID=one_strand,", "##INFO=<ID=SB,", "##FORMAT=<ID=ADF,", "##FORMAT=<ID=ADR,")
SUMMARY = ("max_sb", "min_alt_strand", "min_strand_depth", "strand_bias_sites", "one_strand_sites", "filtered_sites")


def other(base):
    return next(x for x in b"ACGT" if x != base)


def make_input(d):
    rng = np.random.default_rng(2341)
    record = random_reads(rng, 1, LENGTH, LENGTH)[0]
    # the deletion where no neighbour lets it move or split: the base in front differs from its last base, its first from the one behind
    at = next(p for p in range(DELETION, DELETION + 200) if record[p - 1] != record[p + 1] and record[p] != record[p + 2] and record[p] != record[p + 1])
    reads = []
    for i, s in enumerate(range(0, LENGTH - READ + 1, STEP)):
        rev = i % 2
        S = bytearray(record[s:s + READ + (2 if rev else 0)])  # (a read with the deletion still has 150 bases)
        if not rev and s <= ONE_STRAND_SNV < s + READ:
            S[ONE_STRAND_SNV - s] = other(record[ONE_STRAND_SNV])
        if (i // 2) % 2 == 0 and s <= BALANCED_SNV < s + READ:
            S[BALANCED_SNV - s] = other(record[BALANCED_SNV])
        if rev and s + 20 <= at < s + READ - 20:
            del S[at - s:at - s + 2]
        S = bytes(S[:READ])
        reads.append(revcomp(S) if rev else S)
    with open(d / "ref.fa", "wb") as f:
        f.write(b">chrA\n" + record + b"\n")
    with open(d / "reads.fq", "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@read%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n")
    return record, at


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("strand")
    record, at = make_input(d)
    outs = ["-o", "--variants", "--pileup", "--sites", "--duplicates", "--vcf"]
    got = {}
    for sub in ("normalize", "strand"):
        files = [d / ("%s_%s" % (sub, o.strip("-") or "fa")) for o in outs]
        args = [sub, d / "ref.fa", d / "reads.fq", "-q", "-s", d / (sub + ".json")]
        for o, f in zip(outs, files):
            args += [o, f]
        run(args)
        got[sub] = [f.read_bytes() for f in files]
    return d, record, at, got


def vcf_lines(text):
    return [line.split("\t") for line in text.decode().splitlines() if not line.startswith("#")]


def test_the_planted_sites_get_their_filters(data):
    d, record, at, got = data
    lines = {(int(x[1]), "INDEL" in x[7]): x for x in vcf_lines(got["strand"][5])}
    assert len(lines) == 3
    one, balanced, deletion = lines[(ONE_STRAND_SNV + 1, False)], lines[(BALANCED_SNV + 1, False)], lines[(at, True)]
    assert one[6] == "strand_bias;one_strand" and balanced[6] == "PASS" and deletion[6] == "strand_bias;one_strand"
    assert one[3] == chr(record[ONE_STRAND_SNV]) and one[4] == chr(other(record[ONE_STRAND_SNV])) and one[9].split(":")[0] == "0/1"
    fmt = dict(zip(one[8].split(":"), one[9].split(":")))
    assert one[8] == "GT:GQ:DP:AD:ADF:ADR:PL" and fmt["ADF"].split(",")[0] == "0" and fmt["ADR"].split(",")[1] == "0" and min(int(v) for v in fmt["AD"].split(",")) >= 12
    fmt = dict(zip(balanced[8].split(":"), balanced[9].split(":")))
    assert all(int(x) >= 6 for x in fmt["ADF"].split(",") + fmt["ADR"].split(","))
    fmt = dict(zip(deletion[8].split(":"), deletion[9].split(":")))
    assert len(deletion[3]) == 3 and len(deletion[4]) == 1 and fmt["GT"] == "0/1" and fmt["ADF"].split(",")[1] == "0" and int(fmt["ADR"].split(",")[1]) >= 8
    assert re.search(r";SB=\d+\.\d\d$", one[7]) and re.search(r"^INDEL;DP=\d+;IDV=\d+;IEV=\d+;SB=\d+\.\d\d$", deletion[7])
    s = json.load(open(d / "strand.json"))
    assert [s[k] for k in SUMMARY] == [1083, 1, 3, 2, 2, 2]
    # the flags off, and thresholds that the balanced site misses: the lines stay, their FILTER changes
    off = vcf_lines(run(["strand", d / "ref.fa", d / "reads.fq", "-q", "--vcf", "-", "--max-sb", "0", "--min-alt-strand", "0"]).stdout)
    assert [x[6] for x in off] == ["PASS"] * 3
    hard = vcf_lines(run(["strand", d / "ref.fa", d / "reads.fq", "-q", "--vcf", "-", "--max-sb", "0", "--min-alt-strand", "9"]).stdout)
    assert [x[6] for x in hard] == ["one_strand"] * 3 and [x[:6] for x in hard] == [x[:6] for x in off]  # (15 ALT reads over two strands: one has 8 at most)


def test_adf_adr_sb_and_filter_are_what_the_pileup_columns_make_of_them(data):
    d, record, at, got = data
    head, *rows = [x.split("\t") for x in got["strand"][2].decode().splitlines()]
    assert head == "record pos ref A C G T N del ins rev qA qC qG qT rA rC rG rT".split()
    pile = {int(x[1]): dict(zip(head[3:], (int(v) for v in x[3:]))) for x in rows}
    assert all(sum(c["r" + b] for b in "ACGT") <= c["rev"] and all(c["r" + b] <= c[b] for b in "ACGT") for c in pile.values())
    assert sum(c["rA"] + c["rC"] + c["rG"] + c["rT"] for c in pile.values()) > 30_000
    for x in vcf_lines(got["strand"][5]):
        fmt = dict(zip(x[8].split(":"), x[9].split(":")))
        ad, adf, adr = ([int(v) for v in fmt[k].split(",")] for k in ("AD", "ADF", "ADR"))
        assert [f + r for f, r in zip(adf, adr)] == ad, x
        if "INDEL" in x[7]:
            table = (adf[0], adr[0], adf[1], adr[1])
            c = pile[int(x[1]) if len(x[3]) > len(x[4]) else int(x[1]) - 1]  # (a deletion's line stands on the base in front of its first position)
            assert adr[0] + adr[1] == c["rev"] and sum(ad) == c["A"] + c["C"] + c["G"] + c["T"] + c["N"] + c["del"]
        else:
            c = pile[int(x[1]) - 1]
            alleles = [x[3]] + x[4].split(",")
            assert adr == [c["r" + b] for b in alleles] and adf == [c[b] - c["r" + b] for b in alleles]
            table = (adf[0], adr[0], sum(adf[1:]), sum(adr[1:]))
        sb = SW.score(table)
        want = {0: "PASS", 1: "strand_bias", 2: "one_strand", 3: "strand_bias;one_strand"}[SW.flags(table, sb)]
        assert x[6] == want and x[7].endswith(";SB=%d.%02d" % (sb // 100, sb % 100)), (x, table, sb)


def test_without_the_strand_fields_the_outputs_are_normalizes(data):
    d, record, at, got = data
    a, b = got["normalize"], got["strand"]
    assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and a[4] == b[4] and all(len(x) > 30 for x in (a[0], a[1], a[2], a[3]))
    stripped = b"".join(b"\t".join(line.split(b"\t")[:-4]) + b"\n" for line in b[2].splitlines())
    assert stripped == a[2] and b[2] != a[2]
    lines = []
    for line in b[5].decode().splitlines():
        if line.startswith(NEW_HEADER):
            continue
        if not line.startswith("#"):
            x = line.split("\t")
            assert x[6] in ("PASS", "strand_bias", "one_strand", "strand_bias;one_strand") and x[8] == "GT:GQ:DP:AD:ADF:ADR:PL"
            x[6] = "PASS"
            x[7] = re.sub(r";SB=\d+\.\d\d$", "", x[7])
            x[8] = "GT:GQ:DP:AD:PL"
            f = x[9].split(":")
            x[9] = ":".join(f[:4] + f[6:])
            line = "\t".join(x)
        lines.append(line)
    assert ("\n".join(lines) + "\n").encode() == a[5]
    assert sum(1 for line in b[5].decode().splitlines() if line.startswith(NEW_HEADER)) == 5
    sa, sb = (json.load(open(d / (sub + ".json"))) for sub in ("normalize", "strand"))
    assert {k: sb[k] for k in sa if k != "time"} == {k: sa[k] for k in sa if k != "time"} and set(sb) - set(sa) == set(SUMMARY)
