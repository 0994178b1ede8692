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
