"""The text that the map family of the command-line tool writes (deacon-server_amd/cli/map_text.hpp: PAF lines, the VCF header
and its SNV, INDEL and block lines, the callable BED, phase sets, the by-POS merge, the tables), checked without a GPU:
tests/cpp/map_text_test.cpp holds the expected strings, written by hand from the rules the help texts and include/*.h state.
(no reference counterpart: the reference has no mapper.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_map_text_under_the_sanitizers(tmp_path):
    """a stand-alone program with AddressSanitizer and UBSan (CPU build: the header makes no device call and needs no library)"""
    exe = tmp_path / "map_text_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "deacon-server_amd", "cli"), "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "map_text_test.cpp")], check=True)
    p = subprocess.run([str(exe)], capture_output=True)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"bad 0"), (p.stdout[-3000:], p.stderr[-3000:])
