"""What the engine's writers share on the host -- the rank of a string in a dictionary, the dictionary insert, the cached
range of a column, the codes of a width, the host row store -- checked without a device: tests/c/writer_helpers_test.c
includes the engine's sources and calls those helpers alone, its device calls left unresolved."""
import subprocess

import qpelib as q


def test_writer_helpers_keep_dictionaries_ranges_and_rows_whole(tmp_path):
    exe = tmp_path / "writer_helpers_test"
    # the engine's sources under the warnings their own Makefile builds them with (record fields are filled to the last byte)
    subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-Wextra", "-Werror", "-Wno-stringop-truncation", f"-I{q.ROOT / 'include'}",
                    str(q.ROOT / "tests" / "c" / "writer_helpers_test.c"), "-o", str(exe), "-lpthread",
                    "-Wl,--unresolved-symbols=ignore-all"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout and "FAIL" not in r.stdout
