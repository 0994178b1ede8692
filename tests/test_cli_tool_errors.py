"""`deacon-hip` argument and usage errors that end before any device call, and the subcommands' --help: exit code and the
exact text, as the tool gave them before its subcommands came to share their batch helpers.  No GPU is needed: none of these
loads an index or opens an output (what those say depends on whether a device is present)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "deacon-server_amd", "bin", "deacon-hip")
HELP = os.path.join(ROOT, "tests", "golden", "cli_help")
X33 = ["-x", "a"] * 33
LIST = "a comma-separated list of 0-based index positions"
ODD = "Constraint violated: k + w - 1 must be odd (k=31, w=16)"
NOTHING = "nothing to write: give at least one of -o <OUTPUT>, --variants <FILE>, --pileup <FILE>, --sites <FILE>, "

# (arguments, the one `Error: ...` line, what stderr holds in front of it)
ERRORS = [
    (["classify"], "the following required arguments were not provided: -x <INDEX>", ""),
    (["classify", "-x"], "missing value for -x", ""),
    (["classify", "-a", "0", "-x", "a"], "invalid value for --abs-threshold: must be 1..65535", ""),
    (["classify", "-x", "a", "--track-cap", "70000"], "invalid value for --track-cap: must be 0..65535", ""),
    (["classify", "--track-bin", "-1", "-x", "a"], "invalid value for --track-bin", ""),
    (["classify", "a", "b", "c"], "unexpected argument 'c'", ""),
    (["classify"] + X33, "classify takes at most 32 indexes", ""),
    (["mask", "-x", "a"], "nothing to write: give at least one of -o <OUTPUT>, --bed <BED>, -s <SUMMARY>", ""),
    (["mask", "-x", "a", "-o", "o", "in1", "in2"],
     "mask takes one input: mates are independent here, run it once per file (unexpected argument 'in2')", ""),
    (["mask", "--nope"], "unexpected argument '--nope'", ""),
    (["mask", "-x", "a", "-g", "-1", "-o", "o"], "invalid value for --max-gap: must be 0..4294967295", ""),
    (["mask", "-x", "a", "-a", "0", "-o", "o"], "invalid value for --min-hits: must be 1..65535", ""),
    (["mask"] + X33, "mask takes at most 32 indexes", ""),
    (["mask"] + X33 + ["-o", "o"], "mask takes at most 32 indexes", ""),
    (["place"], "the following required arguments were not provided: <REF>", ""),
    (["place", "ref.fa", "--band", "0"], "invalid value for --band: must be 1..4294967295", ""),
    (["place", "ref.fa", "-k", "57"], "invalid value for -k: must be 1..56", ""),
    (["index", "compare"], "index compare takes 2 to 32 indexes, not 0", ""),
    (["index", "compare", "a"], "index compare takes 2 to 32 indexes, not 1", ""),
    (["index", "intersect"], "index intersect needs at least one <INDEX>", ""),
    (["index", "diff", "a", "-o", "o"], "index diff needs <FIRST> <SECOND>", ""),
    (["index", "select"], "the following required arguments were not provided: -x <INDEX>", ""),
    (["index", "select", "-x", "a", "--all", "0,"], f"invalid value '0,' for --all: {LIST}", ""),
    (["index", "select", "-x", "a", "--all", ""], f"invalid value '' for --all: {LIST}", ""),
    (["index", "select", "-x", "a", "--any", "5"], "invalid value '5' for --any: position 5, but 1 -x given", ""),
    (["index", "select", "-x", "a", "--min-members", "3", "--max-members", "2"], "--min-members is larger than --max-members", ""),
    (["index", "select"] + X33, "index select takes at most 32 indexes", ""),
    (["index", "build"], "the following required arguments were not provided: <INPUT>", ""),
    (["index", "build", "-k", "0", "x.fa"], "invalid value for -k: 1..=57", ""),
    (["index", "build", "--min-count", "0", "x.fa"], "invalid value '0' for --min-count: 1 to 65535", ""),
    (["index", "build", "--min-count", "3", "--max-count", "2", "x.fa"], "--min-count 3 is above --max-count 2", ""),
    (["index", "build", "-k", "31", "-w", "16", "x.fa"], ODD,
     "Deacon-hip v{v}; mode: build; input: single; options: capacity=400M\n"),
    (["index", "build", "--min-count", "2", "-k", "31", "-w", "16", "x.fa"], ODD,
     "Deacon-hip v{v}; mode: build; input: single; options: capacity=as needed, min_count=2, max_count=0\n"),
    # the map family (one driver, run_map): the texts of the tool as it was before run_map was cut into stages
    (["map"], "the following required arguments were not provided: <REF>", ""),
    (["call"], "the following required arguments were not provided: <REF>", ""),
    (["genotype", "REF"], f"{NOTHING}--vcf <FILE>, -s <SUMMARY>", ""),
    (["markdup", "REF"], f"{NOTHING}--vcf <FILE>, --duplicates <FILE>, -s <SUMMARY>", ""),
    (["gvcf", "REF"], f"{NOTHING}--vcf <FILE>, --gvcf <FILE>, --callable <FILE>, --duplicates <FILE>, -s <SUMMARY>", ""),
    (["phase", "REF", "reads.fq"],
     f"{NOTHING}--vcf <FILE>, --gvcf <FILE>, --callable <FILE>, --phase-sets <FILE>, --links <FILE>, --duplicates <FILE>, -s <SUMMARY>", ""),
    (["phase", "--ploidy", "1", "REF", "reads.fq"], "phase needs --ploidy 2: a haploid genotype has no heterozygous site to phase", ""),
    (["phase", "REF"],
     "phase reads its input twice (the pile-up, then the links between the sites that were found): give a file, not stdin", ""),
    (["map", "--verified-only"], "unexpected argument '--verified-only'", ""),
    (["verify", "REF", "--min-mapq", "3"], "unexpected argument '--min-mapq'", ""),
    (["pileup", "REF", "--pileup", "x"], "unexpected argument '--pileup'", ""),
    (["extend", "REF", "--verified-only"], "unexpected argument '--verified-only'", ""),
    (["call", "REF", "--vcf", "x"], "unexpected argument '--vcf'", ""),
    (["genotype", "--gvcf", "x"], "unexpected argument '--gvcf'", ""),
    (["gvcf", "REF", "--links", "x"], "unexpected argument '--links'", ""),
    (["map", "REF", "-N", "0"], "invalid value for -N: must be 1..8", ""),
    (["verify", "REF", "--max-div", "1001"], "invalid value for --max-div: must be 0..1000", ""),
    (["pileup", "REF", "--min-mapq", "61"], "invalid value for --min-mapq: must be 0..60", ""),
    (["extend", "REF", "--penalty", "1"], "invalid value for --penalty: must be 2..255", ""),
    (["call", "REF", "--min-baseq", "256"], "invalid value for --min-baseq: must be 0..255", ""),
    (["genotype", "REF", "--min-gq", "100"], "invalid value for --min-gq: must be 0..99", ""),
    (["gvcf", "REF", "--gq-bands", "20,x"], "invalid value for --gq-bands: must be 0..255", ""),
    (["phase", "REF", "--max-link-minor", "1001"], "invalid value for --max-link-minor: must be 0..1000", ""),
    (["phase", "REF", "--vcf"], "missing value for --vcf", ""),
    (["map", "a", "b", "c"], "map takes one input: mates are independent here, run it once per file (unexpected argument 'c')", ""),
    (["verify", "REF", "a", "b"], "verify takes one input: mates are independent here, run it once per file (unexpected argument 'b')", ""),
    (["phase", "a", "b", "c"], "phase takes one input: mates are independent here, run it once per file (unexpected argument 'c')", ""),
]

HELPS = ["classify", "mask", "place", "index", "index build", "index info", "index union", "index diff", "index intersect",
         "index compare", "index select"]


def tool(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)


@pytest.fixture(scope="module")
def version():
    p = tool(["--version"])
    assert p.returncode == 0 and p.stdout.startswith("deacon-hip ")
    return p.stdout.split()[1]


@pytest.mark.parametrize("args,message,banner", ERRORS, ids=[" ".join(e[0][:8]) for e in ERRORS])
def test_error_exit_code_and_text(version, args, message, banner):
    p = tool(args)
    assert (p.returncode, p.stdout, p.stderr) == (1, "", banner.format(v=version) + "Error: " + message + "\n")


@pytest.mark.parametrize("sub", HELPS)
def test_help_text(sub):
    p = tool(sub.split() + ["--help"])
    with open(os.path.join(HELP, sub.replace(" ", "_") + ".txt")) as f:
        want = f.read()
    assert (p.returncode, p.stderr, p.stdout) == (0, "", want)
