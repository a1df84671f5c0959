"""The fused filter-and-aggregate kernels (grouped COUNT(*), COUNT / SUM / MIN / MAX, ORDER BY .. LIMIT, COUNT(DISTINCT)) called
at the shim, with inputs the engine never sends, under both load flavours -- each in its own process, because the shim
reads PQPS_NT_LOADS once (tests/fused_driver.py does the work; see its docstring for the inputs).

  * streaming (`nt`) loads: every fused scan kernel exists as NT=false and NT=true, and the default picks NT=true only when
    the predicate columns exceed 256 MiB -- no engine-level test gets there
  * the bin cut-off (bins >= n_bins, values below the base that wrap), empty aggregate bins, byte group / key columns in the
    scans, both sides of every path switch (16 / 17 and 16 384 / 16 385 bins; 2304 / 2305 aggregate bins; the bitmap forms),
    K on the steps of the top-K buffer, top-K without input, list forms with capacity < count and bases at the top of u32
  * rows in the readable padding that WOULD match and change the answer: the trim of the partial last step
  * after every fused call pqps_last_kernel() names the path the case expects and this process's load flavour

Not here, because they read no once-per-process switch: the sort forms pqps_sort_list and pqps_distinct_sort, pqps_distinct_count
and pqps_column_bounds are called at the shim by tests/test_gpu_sort_shim.py (pqps_group_pair_sort by test_gpu_group_pair_shim.py).
"""
import os
import re
import subprocess
import sys

import pytest

import fused_driver
import qpelib as q

pytestmark = pytest.mark.gpu
DRIVER = str(q.ROOT / "tests" / "fused_driver.py")
INSTANCES = {"group": 3, "aggregate": 6, "topk": 2, "distinct": 6}      # fused scan kernels per load flavour
FUSED_FILES = ["test_gpu_group_count.py", "test_gpu_aggregate.py", "test_gpu_order_by.py", "test_gpu_count_distinct.py"]


def run_driver(env, *args, timeout=600):
    p = subprocess.run([sys.executable, DRIVER, *args], capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, **env), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])
    return p.stdout


@pytest.mark.parametrize("nt", ["0", "1"])
@pytest.mark.parametrize("family", list(INSTANCES))
def test_fused_family(family, nt):
    out = run_driver({"PQPS_NT_LOADS": nt}, family)
    flavour = "NT=true" if nt == "1" else "NT=false"
    m = re.search(rf"^{family}: {flavour} cases=(\d+) kernels=(\d+)$", out, re.M)
    assert m, out[-2000:]
    kernels = re.findall(r"^  (\S.*)$", out, re.M)
    # every fused scan instance of the family ran, in this flavour and in no other
    assert len(kernels) == int(m.group(2)) == len(set(kernels)) == INSTANCES[family], kernels
    assert all(flavour in k for k in kernels), kernels
    # ... over every planned case: the number comes from the case lists alone, so it is the same for both flavours
    assert int(m.group(1)) == fused_driver.planned_cases(family) > 0


def test_engine_small_tables_with_streaming_loads():
    """The engine's own small-table sweeps of the four fused files at 65 537 rows with PQPS_NT_LOADS=1: bit-plane group and key
    columns (sudo_used) and every engine-made bin range under streaming loads."""
    p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "--tb=short", "-m", "gpu", "-p", "no:cacheprovider",
                        *[str(q.ROOT / "tests" / f) for f in FUSED_FILES], "-k", "synthetic_small and 65537"],
                       capture_output=True, text=True, timeout=900, env=dict(os.environ, PQPS_NT_LOADS="1"), cwd=str(q.ROOT))
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-2000:])
    assert "4 passed" in p.stdout and "skipped" not in p.stdout and "failed" not in p.stdout, p.stdout[-2000:]

