"""The lattice member's exact-division index (heavydb_amd/csrc/lattice_index.h: what the producers of k_part_scatter MODE 3 / 4
run per record, and the host function that makes its parameters) against a 128-bit division on the CPU:
tests/lattice_index_check.cpp, a stand-alone program built with AddressSanitizer and UBSan, walks 16 strides x 7 cards and
per pair the edges of the range, ~3 000 lattice points with their near misses (off by a remainder, by 2^32 points, by half
a stride, by the stride's odd part, by its power of two) and uniform 64-bit values."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exact_division_index_matches_128_bit_division(tmp_path):
    exe = str(tmp_path / "lattice_index_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "heavydb_amd", "csrc"), os.path.join(ROOT, "tests", "lattice_index_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 mismatches" in r.stdout, r.stdout
