"""hipCountManyPack under the host sanitizers: tests/c/count_many_helpers_test.c includes engine/hip/hipPredicate.c, packs
compiled predicates and walks every batch row by row -- a stand-alone program, no device, nothing loaded into Python."""
import subprocess

import qpelib as q


def test_the_packer_under_the_host_sanitizers(tmp_path):
    exe = tmp_path / "count_many_helpers_test"
    subprocess.run(["gcc", "-std=c11", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-stringop-truncation", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{q.ROOT / 'include'}", str(q.ROOT / "tests" / "c" / "count_many_helpers_test.c"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all passed" in r.stdout and "FAIL" not in r.stdout
