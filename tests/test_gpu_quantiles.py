"""Exact percentiles through the engine (executeQueryQuantilesHIP / HipEngine.quantiles, median): every expected answer is
tests/quantile_model.py's -- the selection's values sorted with numpy and indexed at the rank -- over rows and cells that
tests/column_model.py or HostSynth give, never the engine's.  Equality everywhere.

tests/quantile_driver.py holds the matrix (every WHERE route x the 12 value columns x no group / risk_level / user_name, the
four fraction lists, the cross-checks against aggregate and group_count, an IN SET, more than 4096 groups in batches) and the
writer history; they run here on one shard and, in a child process per layout, over three and five shards.  The batches come
from the environment variable PQPS_QUANTILE_WORDS, which lowers the words one launch may count (2^22 are not reached at these
sizes).  Here besides: the pass counts at the domain edges, a synthetic table, the refusals."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import column_model as cm
import quantile_driver as qd
import quantile_model as qm
import qpelib as q
import shard_matrix as sm
import test_gpu_group_first as gf

pq = q.pq
pytestmark = pytest.mark.gpu
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def test_matrix_on_one_shard():
    assert qd.run("0") > 1500


def test_history_on_one_shard():
    assert qd.history("0") > 800


@pytest.mark.parametrize("what", ["run", "history"])
@pytest.mark.parametrize("k", sm.LAYOUTS)
def test_over_shards(k, what):
    """Quantiles do not decompose per shard, histograms do: the shards' tables are summed before a digit is picked."""
    devices = ",".join("0" * k)
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(q.ROOT / "tests" / "quantile_driver.py"), what, devices],
                       capture_output=True, text=True, env=dict(os.environ, PQPS_DEVICES=devices), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.split()[-1:] == ["OK"], (p.stdout[-3000:], p.stderr[-3000:])


@pytest.mark.parametrize("users", [2047, 2048, 2049])
def test_one_pass_up_to_2048_values(users):
    """A value column of exactly 2047 and 2048 distinct values is ONE counting scan, of 2049 two."""
    n = 20_000
    rng = np.random.default_rng([77, users])
    cols = gf.edge_columns(n, rng, users)
    cols["user_name"][0][:users] = np.arange(users)                  # every value occurs
    model = cm.ColumnModel(cols)
    eng = pq.HipEngine.from_columns(n, cols)
    try:
        for chain in gf.EDGE_CHAINS:
            ids = model.select_ids(chain)
            for group, ppm in ((None, qd.SIX), ("shell_type", [500_000]), ("risk_level", qd.SIXTEEN)):
                got, info = eng.quantiles_result("user_name", ppm, group, chain)
                assert got == qm.column_expected(model, ids, "user_name", ppm, group), (users, chain, group)
                # (no row: pass 0 finds that out, and no later pass has a group to count)
                assert info["total"] == len(ids) and info["passes"] == (1 if users <= 2048 or not ids else 2), (users, group, info)
    finally:
        eng.close()


def test_pass_counts_of_wide_keys():
    """exit_code from INT32_MIN to INT32_MAX: 32 bits, three passes of 11 + 11 + 10; command_id over the whole u64 range: six."""
    cols = sm.table()
    model = cm.ColumnModel(cols)
    eng = pq.HipEngine.from_columns(sm.N, cols)
    try:
        every = list(range(sm.N))
        for value, passes in (("exit_code", 3), ("command_id", 6), ("timestamp", 2), ("risk_level", 1), ("sudo_used", 1), ("raw_command", 0)):
            got, info = eng.quantiles_result(value, [500_000])
            assert got == qm.column_expected(model, every, value, [500_000]) and info["passes"] == passes, (value, info)
        assert eng.median("command_id") == [(None, sm.N, int(np.sort(cols["command_id"])[(sm.N - 1) // 2]))]
        assert eng.median("exit_code", "shell_type") == [(k, n, v[0]) for k, n, v in qm.column_expected(model, every, "exit_code", [500_000], "shell_type")]
        assert eng.quantiles("sudo_used", [0, 1.0]) == [(None, sm.N, [False, True])]
        assert eng.quantiles("exit_code", [0.0, 1_000_000]) == [(None, sm.N, [INT32_MIN, INT32_MAX])]
    finally:
        eng.close()


def test_synthetic_table():
    n = 200_000
    host = q.HostSynth(n, full=True)
    eng = pq.HipEngine.synthetic(n)
    rows = {}
    try:
        for cname, value, group, ppm in (("all", "user_id", None, qd.SIX), ("risk_gt2", "user_id", None, [500_000]), ("all", "command_id", None, qd.SIXTEEN),
                                         ("all", "timestamp", "user_name", [500_000, 950_000, 990_000]), ("all", "risk_level", "host_name", [500_000]),
                                         ("s1", "exit_code", "shell_type", qd.SIX), ("or_tree", "user_name", "sudo_used", qd.SIX),
                                         ("nothing", "command_id", "risk_level", [500_000]), ("risk_gt2", "shell_type", "risk_level", qd.SIXTEEN)):
            chain = gf.grp.SYNTH_CHAINS[cname]
            if cname not in rows:
                rows[cname] = np.asarray(host.oracle_scan(chain or [], nthreads=min(16, os.cpu_count() or 1)), dtype=np.int64)
            got = eng.quantiles(value, ppm, group, chain)
            assert got == qm.synth_expected(host, rows[cname], value, ppm, group), (cname, value, group)
            if group:
                assert [(k, c) for k, c, _ in got] == eng.group_count(group, chain)
    finally:
        eng.close()


def test_refusals():
    eng = pq.HipEngine(q.GOLDEN / "commands_2k.csv", [])
    L = pq.lib()
    try:
        for fractions in ([], [500_000] * 17, [1_000_001], [-1], [0.5000001], [1.5]):
            with pytest.raises(ValueError):
                eng.quantiles("exit_code", fractions)
        for value, group in (("no_such_column", None), ("exit_code", "no_such_column"), ("exit_code", "command_id")):
            with pytest.raises(pq.PqpsError):
                eng.quantiles(value, [500_000], group)
        for ppm in ([], [7] * 17, [1_000_001]):                      # the C entry point's own refusals
            arr = (C.c_uint * max(1, len(ppm)))(*ppm)
            res = L.executeQueryQuantilesHIP(eng.e, b"exit_code", None, arr, len(ppm), None)
            assert res and not res.contents.success and res.contents.numGroups == 0
            L.freeQuantileResultHIP(res)
        assert len(eng.quantiles("exit_code", [500_000])) == 1       # nothing crashed
    finally:
        eng.close()
