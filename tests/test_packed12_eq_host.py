"""csrc/packed12_eq.hpp under the host sanitizers: tests/c/packed12_eq_test.cpp runs the raw-dword equality of a 12-bit packed
chunk against field-by-field comparison -- all 4096 codes against random chunks, the code in every field alone, in adjacent
pairs (across both dword boundaries) and in all, every one-bit near-miss in every field, codes 0 and 4095 beside all-zero and
all-one neighbours.  A stand-alone program, no device, nothing loaded into Python."""
import subprocess

import qpelib as q


def test_the_raw_dword_equality_under_the_host_sanitizers(tmp_path):
    exe = tmp_path / "packed12_eq_test"
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{q.ROOT / 'parallel-query-processing-system_amd' / 'csrc'}", str(q.ROOT / "tests" / "c" / "packed12_eq_test.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all passed" in r.stdout and "FAIL" not in r.stdout
