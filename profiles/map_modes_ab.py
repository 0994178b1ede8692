#!/usr/bin/env python3
"""The map family of `deacon-hip` (map, verify, align, pileup, extend, consensus, call, genotype, markdup, indels, normalize,
strand, gvcf, phase) against a parent tool: every output byte, and the time.

    python3 profiles/map_modes_ab.py PARENT_TOOL [--out FILE] [--reads N] [--runs N] [--no-time] [--no-equality]

PARENT_TOOL is the parent commit's cli/deacon_hip_cli.cpp compiled with the Makefile's g++ line against this tree's library
(the driver is host code; the library is the same for both).  Both tools load deacon-server_amd/lib/libdeacon_hip.so.

Equality: one small generated input (two records; 150-base FASTQ reads of two haplotypes on both strands; heterozygous and
homozygous SNVs; an insertion and a deletion inside a homopolymer; reads that repeat another's end; a stretch without
coverage), every subcommand with every output option it has, at DCN_CLI_STRETCH_BASES unset and 7 and at the batch-bases
hook unset and small, and a few more option sets.  Every file is compared byte for byte, stderr without the duration, the
-s JSON without "time".  Any difference ends the script with status 1.

Time: a larger input, `map`, `align`, `call`, `gvcf` and `phase`, --runs runs of each tool, alternating, one process per run.
Limit: the new median is at most the parent's largest + (the parent's largest - its smallest), for the wall time and for the
JSON's "time".

A run that does not end with status 0 within its time limit ends the script at once: nothing more is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
LIB = os.path.join(ROOT, "deacon-server_amd", "lib")
READ = 150
COMP = bytes.maketrans(b"ACGT", b"TGCA")

PAF = ["-o", "out.paf"]
PILE = ["--pileup", "pile.tsv", "--sites", "sites.tsv"]
CONS = ["-o", "cons.fa", "--variants", "variants.tsv"] + PILE
VCF = CONS + ["--vcf", "calls.vcf"]
DUP = VCF + ["--duplicates", "dups.tsv"]
GVCF = DUP + ["--gvcf", "calls.g.vcf", "--callable", "callable.bed"]
MODES = [("map", PAF), ("verify", PAF), ("align", PAF), ("pileup", ["-o", "pile.tsv", "--sites", "sites.tsv"]), ("extend", PAF + PILE),
         ("consensus", CONS), ("call", CONS), ("genotype", VCF), ("markdup", DUP), ("indels", DUP), ("normalize", DUP), ("strand", DUP),
         ("gvcf", GVCF), ("phase", GVCF + ["--phase-sets", "sets.tsv", "--links", "links.tsv"])]
MORE = [("verify", PAF + ["--verified-only", "--max-edits", "2"]), ("pileup", ["-o", "pile.tsv", "--all-positions", "--all-ranks", "--min-mapq", "0"]),
        ("extend", []), ("extend", ["--sites", "sites.tsv"]), ("consensus", CONS + ["--fill-ref"]), ("genotype", VCF + ["--ploidy", "1"]),
        ("markdup", DUP + ["--keep-duplicates", "--both-ends"]), ("strand", DUP + ["--ploidy", "1", "--max-sb", "100"]),
        ("gvcf", GVCF + ["--gq-bands", "30", "--ploidy", "1"]), ("gvcf", ["--callable", "callable.bed"]), ("phase", ["--vcf", "calls.vcf.gz"]),
        ("phase", GVCF + ["--min-link-reads", "1000"])]
TIMED = [("map", PAF), ("align", PAF), ("call", CONS), ("gvcf", GVCF), ("phase", GVCF + ["--phase-sets", "sets.tsv", "--links", "links.tsv"])]


def hook(mode):
    return "DCN_CLI_MAP_BATCH_BASES" if mode == "map" else "DCN_CLI_VERIFY_BATCH_BASES" if mode == "verify" else "DCN_CLI_ALIGN_BATCH_BASES"


def other(rng, base):
    return int(rng.choice([x for x in b"ACGT" if x != base]))


def make_input(d, rng, lengths, step, hets_per_kb=1.5):
    """records, two haplotypes, reads every `step` bases of each haplotype in turn on alternating strands"""
    records = [bytearray(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes()) for n in lengths]
    for rec in records:  # a homopolymer for the indels to stand in
        rec[700:712] = b"A" * 12
        rec[699], rec[712] = ord("C"), ord("G")
    haps = [[bytearray(r) for r in records], [bytearray(r) for r in records]]
    for R, rec in enumerate(records):
        sites = rng.choice(np.arange(40, len(rec) - 40), max(4, int(len(rec) * hets_per_kb / 1000)), replace=False)
        for i, p in enumerate(sorted(int(x) for x in sites)):
            if 690 <= p < 720:
                continue
            alt = other(rng, rec[p])
            for h in ((0, 1) if i % 4 == 3 else (i % 2,)):  # every fourth site homozygous
                haps[h][R][p] = alt
    for h in (0, 1):  # both haplotypes: an A less in the first record's homopolymer, two more in the second's
        del haps[h][0][705]
        if len(records) > 1:
            haps[h][1][705:705] = b"AA"
    reads = []
    for R in range(len(records)):
        for i, s in enumerate(range(0, len(haps[0][R]) - READ + 1, step)):
            if R == 0 and 1500 <= s < 1900:  # a stretch without coverage
                continue
            S = bytes(haps[(i // 2) % 2][R][s:s + READ])
            reads.append(S.translate(COMP)[::-1] if i % 2 else S)
            if i % 37 == 5:  # a read that repeats another's end
                reads.append(reads[-1])
    with open(os.path.join(d, "ref.fa"), "wb") as f:
        for R, rec in enumerate(records):
            f.write(b">chr%c some words\n" % (65 + R) + bytes(rec) + b"\n")
    with open(os.path.join(d, "reads.fq"), "wb") as f:
        for i, r in enumerate(reads):
            q = bytearray(b"I" * len(r))
            q[i % len(r)] = ord("#")  # one base under --min-baseq
            f.write(b"@read%d/x y\n" % i + r + b"\n+\n" + bytes(q) + b"\n")
    return len(reads)


def run(tool, mode, opts, cwd, env_more, limit):
    env = dict(os.environ, LD_LIBRARY_PATH=LIB + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    for key in ("DCN_CLI_STRETCH_BASES", "DCN_CLI_MAP_BATCH_BASES", "DCN_CLI_VERIFY_BATCH_BASES", "DCN_CLI_ALIGN_BATCH_BASES"):
        env.pop(key, None)
    env.update(env_more)
    t0 = time.perf_counter()
    try:
        p = subprocess.run([tool, mode, "../ref.fa", "../reads.fq", "-s", "summary.json"] + opts, cwd=cwd, env=env, capture_output=True, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit("%s %s: no end within %d s; nothing more is started" % (tool, mode, limit))
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        sys.exit("%s %s %s: status %d; nothing more is started\n%s" % (tool, mode, " ".join(opts), p.returncode, p.stderr.decode()[-2000:]))
    return p, wall


def outputs(cwd, p):
    """every file of the run, the JSON without its time, stdout, and stderr without the duration"""
    got = {}
    for name in sorted(os.listdir(cwd)):
        blob = open(os.path.join(cwd, name), "rb").read()
        if name == "summary.json":
            got["time"] = json.loads(blob)["time"]
            blob = b"".join(x for x in blob.splitlines(True) if not x.startswith(b'  "time": '))  # (the text itself, less one line)
        got[name] = blob
    err = p.stderr.decode().splitlines()
    got["stderr"] = "\n".join(x[:x.rindex(" in ")] if x.startswith("Mapped ") else x for x in err).encode()
    got["stdout"] = p.stdout
    return got


def compare(parent, d, mode, opts, env_more, label, report):
    both = []
    for which, tool in (("parent", parent), ("new", NEW)):
        cwd = tempfile.mkdtemp(prefix=which + "_", dir=d)
        both.append(outputs(cwd, run(tool, mode, opts, cwd, env_more, 120)[0]))
    a, b = both
    a.pop("time"), b.pop("time")
    if a.keys() != b.keys():
        sys.exit("%s %s: files differ: %s against %s" % (mode, label, sorted(a), sorted(b)))
    for name in a:
        if a[name] != b[name]:
            for which, blob in (("parent", a[name]), ("new", b[name])):  # (kept for a diff, in DCN_PROFILE_OUT as the other scripts)
                open(os.path.join(os.environ.get("DCN_PROFILE_OUT", tempfile.gettempdir()), "map_modes_ab_%s_%s" % (which, name)), "wb").write(blob)
            sys.exit("%s %s %s: %s differs (%d against %d bytes)" % (mode, " ".join(opts), label, name, len(a[name]), len(b[name])))
    report.append("%-10s %-44s %2d files %8d bytes equal" % (mode, label, len(a), sum(len(x) for x in a.values())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("--out")
    ap.add_argument("--reads", type=int, default=40000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-time", action="store_true")
    ap.add_argument("--no-equality", action="store_true")
    args = ap.parse_args()
    parent = os.path.abspath(args.parent)
    failed = False

    class Report(list):  # every line is shown as it comes, and kept for --out
        def append(self, line):
            print(line, flush=True)
            list.append(self, line)
    report = Report()
    with tempfile.TemporaryDirectory() as d:
        if args.no_equality:
            MODES.clear(), MORE.clear()
        n = make_input(d, np.random.default_rng(2601), (2400, 1100), 5, hets_per_kb=4)
        report.append("# equality: 2 records (2,400 and 1,100 bases), %d reads; per mode and setting, the files compared (outputs, summary without" % n)
        report.append("# time, stdout, stderr without the duration) and their bytes")
        for mode, opts in MODES:
            for stretch in (None, "7"):
                for batch in (None, "2000"):
                    env_more = dict(([("DCN_CLI_STRETCH_BASES", stretch)] if stretch else []) + ([(hook(mode), batch)] if batch else []))
                    compare(parent, d, mode, opts, env_more, "stretch %s, batch bases %s" % (stretch or "default", batch or "default"), report)
        for mode, opts in MORE:
            compare(parent, d, mode, opts, {"DCN_CLI_STRETCH_BASES": "1000", hook(mode): "5000"}, " ".join(opts[-4:]) or "(no output option)", report)
        if not args.no_equality:
            report.append("every compared byte equal")
    if not args.no_time:
        with tempfile.TemporaryDirectory() as d:
            step = 5
            n = make_input(d, np.random.default_rng(2602), (args.reads * step + READ,), step)
            report.append("")
            report.append("# time: 1 record of %d bases, %d reads; %d runs of each tool, alternating; seconds" % (args.reads * step + READ, n, args.runs))
            for mode, opts in TIMED:
                walls, times = {"parent": [], "new": []}, {"parent": [], "new": []}
                for _ in range(args.runs):
                    for which, tool in (("parent", parent), ("new", NEW)):
                        cwd = tempfile.mkdtemp(prefix=which + "_", dir=d)
                        p, wall = run(tool, mode, opts + ["-q"], cwd, {}, 300)
                        walls[which].append(round(wall, 3))
                        times[which].append(round(json.load(open(os.path.join(cwd, "summary.json")))["time"], 3))
                for what, v in (("wall", walls), ("time", times)):
                    limit = max(v["parent"]) + (max(v["parent"]) - min(v["parent"]))
                    med = statistics.median(v["new"])
                    over = med > limit
                    failed |= over
                    report.append("%-6s %-5s parent %s new %s | parent median %.3f largest %.3f spread %.3f limit %.3f | new median %.3f%s" % (
                        mode, what, v["parent"], v["new"], statistics.median(v["parent"]), max(v["parent"]), max(v["parent"]) - min(v["parent"]), limit, med,
                        "  <-- over" if over else ""))
            report.append("cells over the limit: %s" % ("some" if failed else "none"))
    text = "\n".join(report) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
