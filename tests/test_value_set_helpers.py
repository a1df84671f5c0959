"""The host helpers of value sets under the host sanitizers: tests/c/value_set_helpers_test.c includes engine/hip/hipPredicate.c
and calls hipCompileHaving and hipCompileWherePlanSets alone -- a stand-alone program, no device, nothing loaded into Python."""
import subprocess

import qpelib as q


def test_having_text_and_set_nodes_under_the_host_sanitizers(tmp_path):
    exe = tmp_path / "value_set_helpers_test"
    subprocess.run(["gcc", "-std=c11", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-stringop-truncation", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{q.ROOT / 'include'}", str(q.ROOT / "tests" / "c" / "value_set_helpers_test.c"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all passed" in r.stdout and "FAIL" not in r.stdout
