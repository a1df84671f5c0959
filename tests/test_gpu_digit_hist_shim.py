"""pqps_filter_digit_hist / pqps_digit_hist_list -- one pass of the radix select behind exact percentiles -- called at the
shim with inputs the engine never sends, under both load flavours, each in its own process because the shim reads
PQPS_NT_LOADS once (tests/digit_hist_driver.py does the work; see its docstring for the inputs).

  * key columns of 1, 2, 4 and 8 bytes and the bit plane, i32 keys with INT32_MIN / INT32_MAX under a negative base, u64 keys
    either side of 2^32 and 2^63, keys whose image has a bit at or above key_bits (left out, never an index)
  * digits of 1, 8 and 11 bits at shifts 0 .. 53; 1, 8 and 9 tables of 11 bits and 64 and 65 of 8 bits -- both sides of the
    LDS / global switch -- and 2000 groups x 2 slots; 1, 2 and 16 prefix slots, unused slots, a group hole, a bin window that
    cuts groups off at both ends; a selection whose rows all hit ONE counter
  * rows in the readable padding that WOULD count: the trim of the partial last step; a table at which a wave takes a second step
  * the list form: count below, equal to and above capacity, id_base at the top of u32, ids listed twice counted twice
  * after every call pqps_last_kernel() names the tables' home, the key width and this process's load flavour

The CPU half (`-m "not gpu"`): the driver's references against a row-by-row loop, and that every declared shape is planned."""
import os
import re
import subprocess
import sys

import pytest

import digit_hist_driver
import qpelib as q

DRIVER = str(q.ROOT / "tests" / "digit_hist_driver.py")


def test_references_check_themselves(capsys):
    digit_hist_driver.self_check(sizes=[digit_hist_driver.fd.SLOW_N])
    assert f"digit: n={digit_hist_driver.fd.SLOW_N} ok" in capsys.readouterr().out


@pytest.mark.gpu
@pytest.mark.parametrize("nt", ["0", "1"])
def test_digit_hist(nt):
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, DRIVER, "run"], capture_output=True, text=True,
                       env=dict(os.environ, PQPS_NT_LOADS=nt), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])
    flavour = "NT=true" if nt == "1" else "NT=false"
    m = re.search(rf"^digit: {flavour} cases=(\d+) kernels=(\d+)$", p.stdout, re.M)
    assert m, p.stdout[-2000:]
    kernels = re.findall(r"^  (\S.*)$", p.stdout, re.M)
    # every fused instance ran, in this flavour and in no other, over every planned case
    assert len(kernels) == int(m.group(2)) == len(set(kernels)) == digit_hist_driver.SCAN_KERNELS, kernels
    assert all(flavour in k for k in kernels), kernels
    assert int(m.group(1)) == digit_hist_driver.planned_cases() > 0
