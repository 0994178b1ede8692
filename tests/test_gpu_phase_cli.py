"""`deacon-hip phase` end to end, file to file, on a reference of two records (2,400 and 600 bases) under error-free 150-base
reads of two haplotypes on alternating strands.  The haplotypes differ at eight SNVs: three within reach of one read of each
other, one alone, two more together, and two on the second record; a ninth SNV is homozygous.

The VCF is `deacon-hip gvcf`'s except on the phased lines and one header line; a phased line with `|` put back to `/` in
ascending order and PS taken off is gvcf's line.  PS and `|` are what AnchorMap.phase_solve gives on a map that the test piles
up and links from the same reads with the tool's defaults, and agree with the haplotypes the reads were cut from.  All files
are the same at DCN_CLI_STRETCH_BASES = 1, 7, 1000 and the default and with the align batch-bases hook.  --phase-sets and
--links are the solve's sets and counters.  Exact throughout."""
import json
import os
import subprocess

import numpy as np
import pytest

import _phase_worker as HW
import _pileup_worker as PW
import _quality_worker as QW
import _verify_worker as VW
from conftest import random_reads, revcomp
from test_gpu_pileup_cli import CLI, run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEN_A, LEN_B, READ = 2400, 600, 150
# (record, pos, the haplotype that carries the other base)
HETS = [(0, 300, 0), (0, 360, 1), (0, 420, 0), (0, 1200, 0), (0, 1800, 1), (0, 1850, 1), (1, 200, 0), (1, 260, 1)]
HOM = (0, 900)
SETS = [[(0, 300), (0, 360), (0, 420)], [(0, 1800), (0, 1850)], [(1, 200), (1, 260)]]
NAMES = ("chrA", "chrB")
SUMMARY = ("min_link_reads", "max_link_minor", "phase_sites", "phase_sets", "phased_sites", "links_joined", "rows_linking", "phase_set_n50")
PS_HEADER = "##FORMAT=<ID=PS,"


def other(base):
    return next(x for x in b"ACGT" if x != base)


def make_input(d):
    rng = np.random.default_rng(2511)
    records = [random_reads(rng, 1, LEN_A, LEN_A)[0], random_reads(rng, 1, LEN_B, LEN_B)[0]]
    haps = [[bytearray(r) for r in records], [bytearray(r) for r in records]]
    for R, p, h in HETS:
        haps[h][R][p] = other(records[R][p])
    for h in (0, 1):
        haps[h][HOM[0]][HOM[1]] = other(records[HOM[0]][HOM[1]])
    reads = []
    for R, ln in ((0, LEN_A), (1, LEN_B)):
        for i, s in enumerate(range(0, ln - READ + 1, 5)):  # every start once: no read repeats another's end
            S = bytes(haps[(i // 2) % 2][R][s:s + READ])
            reads.append(revcomp(S) if i % 2 else S)
    quals = [b"I" * len(r) for r in reads]
    with open(d / "ref.fa", "wb") as f:
        f.write(b">chrA\n" + records[0] + b"\n>chrB\n" + records[1] + b"\n")
    with open(d / "reads.fq", "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@read%d\n" % i + r + b"\n+\n" + quals[i] + b"\n")
    return records, reads, quals


def phase_files(d, tag, env=None, more=()):
    files = [d / ("%s.%s" % (tag, x)) for x in ("vcf", "g.vcf", "sets.tsv", "links.tsv", "json")]
    run(["phase", d / "ref.fa", d / "reads.fq", "-q", "--vcf", files[0], "--gvcf", files[1], "--phase-sets", files[2], "--links", files[3],
         "-s", files[4]] + list(more), env=env)
    summary = json.load(open(files[4]))
    summary.pop("time")
    return [f.read_bytes() for f in files[:4]] + [summary]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("phase")
    records, reads, quals = make_input(d)
    run(["gvcf", d / "ref.fa", d / "reads.fq", "-q", "--vcf", d / "gvcf.vcf", "--gvcf", d / "gvcf.g.vcf", "--pileup", d / "gvcf.tsv", "--all-positions",
         "-s", d / "gvcf.json"])
    return d, records, reads, quals, phase_files(d, "default")


def body(text):
    return [line.split("\t") for line in text.decode().splitlines() if not line.startswith("#")]


def unphased(x):
    """a phased line as gvcf writes it"""
    assert x[8].endswith(":PS") and "|" in x[9]
    sample = x[9].split(":")
    gt = "/".join(sorted(sample[0].split("|")))
    return x[:8] + [x[8][:-3], ":".join([gt] + sample[1:-1])]


def test_the_vcf_is_gvcfs_but_for_the_phased_lines_and_one_header_line(data):
    d, records, reads, quals, (vcf, gvcf, sets, links, summary) = data
    for mine, theirs in ((vcf, (d / "gvcf.vcf").read_bytes()), (gvcf, (d / "gvcf.g.vcf").read_bytes())):
        mine, theirs = mine.decode().splitlines(), theirs.decode().splitlines()
        assert [x for x in mine if x.startswith("#") and not x.startswith(PS_HEADER)] == [x for x in theirs if x.startswith("#")]
        assert sum(x.startswith(PS_HEADER) for x in mine) == 1 and mine[[x[:12] for x in mine].index("##FORMAT=<ID")].startswith("##FORMAT=<ID=GT")
        a, b = [x.split("\t") for x in mine if not x.startswith("#")], [x.split("\t") for x in theirs if not x.startswith("#")]
        assert len(a) == len(b)
        phased = 0
        for x, y in zip(a, b):
            if "|" in x[9]:
                assert unphased(x) == y and len(x[3]) == len(x[4]) == 1 and "INDEL" not in x[7]
                phased += 1
            else:
                assert x == y  # byte for byte
        assert phased == sum(len(s) for s in SETS) == summary["phased_sites"]
    a, b = json.load(open(d / "gvcf.json")), summary
    assert {k: b[k] for k in a if k != "time"} == {k: a[k] for k in a if k != "time"} and set(b) - set(a) == set(SUMMARY)


def test_the_phased_lines_agree_with_the_haplotypes(data):
    d, records, reads, quals, (vcf, gvcf, sets, links, summary) = data
    lines = {(x[0], int(x[1]) - 1): x for x in body(vcf)}
    carrier = {(R, p): h for R, p, h in HETS}
    for group in SETS:
        ps = {lines[(NAMES[R], p)][9].split(":")[-1] for R, p in group}
        assert ps == {str(group[0][1] + 1)}  # PS: the POS of the set's first site
        # haplotype 1 of the line against haplotype 0 of the truth: the same at every site of the set, or the other at every site
        first = [lines[(NAMES[R], p)][9].split("|")[0] for R, p in group]
        truth = ["1" if carrier[(R, p)] == 0 else "0" for R, p in group]
        assert first == truth or first == ["1" if t == "0" else "0" for t in truth], (group, first, truth)
    alone, hom = lines[("chrA", 1200)], lines[("chrA", HOM[1])]
    assert alone[9].startswith("0/1:") and alone[8].endswith(":PL") and hom[9].startswith("1/1:") and hom[8].endswith(":PL")
    assert summary["phase_sites"] == len(HETS) and summary["phase_sets"] == len(SETS) and summary["links_joined"] == 4
    assert summary["phase_set_n50"] == 121 and summary["min_link_reads"] == 2 and summary["max_link_minor"] == 200 and summary["rows_linking"] > 50


def test_ps_and_gt_are_what_phase_solve_gives_on_the_same_rows(data, dcn, oracle):
    d, records, reads, quals, (vcf, gvcf, sets, links, summary) = data
    amap = VW.build_map(oracle, dcn, records)
    amap.pileup_enable()
    amap.pileup_keep_qualities()
    amap.pileup_left_align()
    placer = dcn.Placer(amap, max_batch_bases=1 << 21, max_batch_reads=1 << 12)
    try:
        b, o, q = QW.concat(oracle, reads, quals)
        po, srows, _ = placer.place_split_batch(b, o, max_placements=4)
        xrows, _ = placer.extend_batch(b, o, srows, row_offsets=po)
        xrows = xrows.copy()
        xrows["record"][(xrows["mapq"] < 1) | (xrows["rank"] != 0)] = dcn.filter.UNPLACED  # the tool's --min-mapq 1, rank 0 only
        _, n_added = placer.pileup_batch(b, o, xrows, row_offsets=po, quals=q, min_base_qual=20)
        assert n_added == len(reads)
        table = [x.split("\t") for x in (d / "gvcf.tsv").read_bytes().decode().splitlines()[1:]]
        for R, name in enumerate(NAMES):  # the same rows: the tool's --pileup table, position by position
            mine = np.array([[int(v) for v in x[3:11]] for x in table if x[0] == name], np.uint32)
            assert np.array_equal(mine, amap.pileup_fetch(R))
        entries = []
        for R in (0, 1):
            for s in amap.genotype(R)[2]:
                x, y = (PW.column(c) for c in dcn.GENOTYPES[int(s["gt"])].encode())
                if x != y:
                    ref = int(s["ref_code"])
                    entries.append((R, int(s["pos"]), ref if ref in (x, y) else x, (x + y - ref) if ref in (x, y) else y))
        assert [(R, p) for R, p, _, _ in entries] == [(R, p) for R, p, _ in HETS]
        sites = HW.make_sites(dcn.PHASE_SITE_DTYPE, entries)
        amap.phase_sites(sites)
        _, n_linking = placer.phase_batch(b, o, xrows, row_offsets=po, quals=q, min_base_qual=20)
        assert n_linking == summary["rows_linking"]
        res = amap.phase_solve()
        lines = {(x[0], int(x[1]) - 1): x for x in body(vcf)}
        for k, (R, p, a0, a1) in enumerate(entries):
            x = lines[(NAMES[R], p)]
            in_set = bool(res["flags"][k] & dcn.PHASE_JOINED) or not res["flags"][k] & dcn.PHASE_HEAD
            assert ("|" in x[9]) == in_set
            if in_set:
                alleles = [PW.column(x[3].encode()[0])] + [PW.column(c) for c in x[4].replace(",", "").encode()]
                al = (a0, a1)
                hap = int(res["hap"][k])
                assert x[9].split(":")[0] == "%d|%d" % (alleles.index(al[hap]), alleles.index(al[1 - hap]))
                assert x[9].split(":")[-1] == str(int(res["set_pos"][k]) + 1)
        # the two TSV files from the same results
        want_links = ["record\tpos\tnext_pos\tn00\tn01\tn10\tn11\tjoined"]
        for k in range(len(entries) - 1):
            if entries[k][0] == entries[k + 1][0]:
                want_links.append("\t".join([NAMES[entries[k][0]], str(entries[k][1]), str(entries[k + 1][1])] + [str(int(v)) for v in res["link"][k]] +
                                            ["1" if res["flags"][k] & dcn.PHASE_JOINED else "0"]))
        assert links.decode().splitlines() == want_links
        want_sets = ["record\tfirst_pos\tlast_pos\tsites"] + ["%s\t%d\t%d\t%d" % (NAMES[g[0][0]], g[0][1], g[-1][1], len(g)) for g in SETS]
        assert sets.decode().splitlines() == want_sets
    finally:
        placer.close()
        amap.close()


@pytest.mark.parametrize("env", [{"DCN_CLI_STRETCH_BASES": "1"}, {"DCN_CLI_STRETCH_BASES": "7"}, {"DCN_CLI_STRETCH_BASES": "1000"},
                                 {"DCN_CLI_ALIGN_BATCH_BASES": "20000"}], ids=["stretch1", "stretch7", "stretch1000", "batch20000"])
def test_no_output_depends_on_the_stretch_or_the_batches(data, env):
    d, records, reads, quals, files = data
    assert phase_files(d, "e" + "".join(env.values()), env=env) == files


def test_other_thresholds_and_the_messages(data):
    d, records, reads, quals, (vcf, gvcf, sets, links, summary) = data
    strict = phase_files(d, "strict", more=["--min-link-reads", "100000"])
    assert strict[4]["phase_sets"] == 0 and strict[4]["phased_sites"] == 0 and strict[4]["links_joined"] == 0 and strict[4]["phase_set_n50"] == 0
    assert b"|" not in strict[0] and strict[2] == b"record\tfirst_pos\tlast_pos\tsites\n" and strict[3].count(b"\t0\n") == 6
    assert [x for x in strict[0].decode().splitlines() if not x.startswith(PS_HEADER)] == (d / "gvcf.vcf").read_bytes().decode().splitlines()
    loud = run(["phase", d / "ref.fa", d / "reads.fq", "--vcf", d / "loud.vcf"])
    assert b"Phased 7 of 8 heterozygous SNV sites in 3 sets (4 links joined, " in loud.stderr and (d / "loud.vcf").read_bytes() == vcf
    for args, message in ((["phase", "ref.fa", "--vcf", "x.vcf"], "phase reads its input twice (the pile-up, then the links between the sites that were found): give a file, not stdin"),
                          (["phase", "ref.fa", "reads.fq", "--ploidy", "1", "--vcf", "x.vcf"], "phase needs --ploidy 2: a haploid genotype has no heterozygous site to phase")):
        p = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
        assert (p.returncode, p.stdout, p.stderr) == (1, "", "Error: " + message + "\n")
    p = subprocess.run([CLI, "phase", "--help"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    with open(os.path.join(ROOT, "tests", "golden", "cli_help", "phase.txt")) as f:
        assert (p.returncode, p.stderr, p.stdout) == (0, "", f.read())
