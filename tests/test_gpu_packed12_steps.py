"""Two adjacent steps per scan wave for the shapes with a 12-bit packed column: (P) and (P,B) as ID list and COUNT(*).

With two steps per wave a scan tile is 8 steps (8192 rows) instead of 4; a wave's second step reuses the wave's staging
area in LDS, its count and tiny word lie in slot 2 * wave + 1 of the tile's arrays, and the last step of a table can be
a wave's first or second step, or be missing.  Everything is checked at the shim (pqps_filter_scan / pqps_filter_count)
against kernel_model.evaluate on the u16 codes, ID for ID and in order.

The data is constructed: no row carries code 1030 except the rows placed by a PLAN = {step: matches}, so that the form
in which a step leaves its matches is known -- 1..3 a tiny word, 4..104 16-bit entries in the step's slot (from 65 on
its second line), 105 and more a list in the list area, or (option "list16" 0, as from 268 M rows on) a bit mask.  On
(P,B) the predicate is S1's (`sudo_used = FALSE AND user_name = 1030`): the placed rows have sudo_used FALSE, and five
more rows per planned step carry 1030 with sudo_used TRUE, so a plane read from the wrong step shows.

DEFAULT_S2 says which launches take the two-step kernel by default at these sizes (steps_default in pqps_hip.hip)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import kernel_model
import qpelib as q
import test_gpu_bit_plane as bp
from test_gpu_packed12 import P, B, packed_copy, predicate

pq = q.pq
pytestmark = pytest.mark.gpu

STEP, TILE, GROUP = 1024, 8192, 65536
CODE = 1030
DEFAULT_S2 = {"ids": True, "count": True}
SIZES = [1, 1025, 2047, 2048, 2049, 3073, 8191, 8192, 8193, 9217, 65535, 65537, 73729, 4194304 + 1025]
NT_SIZES = [1, 2049, 73729]

# step -> matches, by tile of 8 steps (wave w of a tile: steps 2 w and 2 w + 1 of it)
PLAN = {
    0: 1, 2: 2, 4: 3, 6: 4,                                        # tile 0: the first step of each wave only
    9: 64, 11: 65, 13: 104, 15: 105,                               # tile 1: the second step only
    16: 256, 17: 1, 18: 600, 19: 4, 20: 1024, 21: 3, 22: 2, 23: 1024,   # tile 2: both steps, in different forms
    26: 1, 27: 65, 28: 105, 31: 1024,                              # tile 3: waves 1 - 3 only: wave 0 publishes words it did not produce
                                                                   # tile 4: no match at all
    40: 1, 41: 2, 42: 104, 43: 64, 44: 600, 45: 256, 46: 1024, 47: 1024,   # tile 5: both steps, in the same form
    63: 3, 64: 105, 71: 1024,                                      # the last step of a group, the first of the next, a tile's last
}
CYCLE = [1024, 3, 105, 64, 1, 600, 4, 2, 104, 65, 256]              # plan "cycle": step s has CYCLE[s % 11] matches


def plan_of(kind, steps):
    """{step: matches} for a table of `steps` steps; the LAST step (full or partial) always has matches."""
    if kind == "cycle":
        plan = {s: CYCLE[s % len(CYCLE)] for s in range(min(steps, 96))}
    else:
        shift = {"plan": 0, "shifted": 1}[kind]                     # "shifted": first and second steps swap roles
        plan = {s + shift: k for s, k in PLAN.items() if s + shift < steps}
    if steps > 96:                                                  # the table's tail: its last tile, whatever it consists of
        for s, k in ((steps - 3, 2), (steps - 2, 105)):
            plan.setdefault(s, k)
    plan.setdefault(steps - 1, 700)
    return plan


def table(n, shape, kind, seed):
    """codes, sudo_used of n rows: code 1030 exactly where the plan puts it."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4096, n).astype(np.uint16)
    codes[codes == CODE] = CODE + 1
    sudo = (rng.random(n) < 0.4).astype(np.uint8)
    steps = (n + STEP - 1) // STEP
    for s, k in plan_of(kind, steps).items():
        rows = min(STEP, n - s * STEP)
        decoys = 5 if len(shape) == 2 and k + 5 <= rows else 0
        at = s * STEP + rng.choice(rows, min(k, rows) + decoys, replace=False)
        codes[at] = CODE
        sudo[at] = 0
        if decoys:
            sudo[at[-decoys:]] = 1
    return codes, sudo


def predicates(shape):
    """(P): one comparison (the vector-unit kernel of one leaf) and the same rows as an AND of two leaves (ballots); (P,B): S1."""
    if len(shape) == 1:
        return [predicate([(0, CODE, 0, 0)], "one", 1), predicate([(0, CODE, 0, 0), (0, 0, 1638, 0)], "and", 1)]
    return [predicate([(0, CODE, 0, 0), (1, 0, 0, 0)], "and", 2)]


def kernel():
    return pq.lib().pqps_last_kernel().decode()


def check_table(ctx, n, shape, kind, seed=7, options=(), nt=False):
    """IDs and COUNT under the default and with the option "steps" 0 and 1; `options`: further context options of the run."""
    L = pq.lib()
    codes, sudo = table(n, shape, kind, seed)
    preds = predicates(shape)
    want = np.nonzero(kernel_model.evaluate(preds[0], [codes, sudo][:len(shape)]))[0].astype(np.uint32)
    assert len(want) > 0
    out, dev = bp.Out(ctx, n), bp.Dev(ctx)
    try:
        cols = [(packed_copy(dev, codes, n), pq.WIDTH_P12)] + ([(dev.plane(sudo, n), pq.WIDTH_BITS)] if len(shape) == 2 else [])
        carr = pq.column_array(cols)
        for name, value in options:
            ctx.set_option(name, value)
        lists = {}
        for steps_opt, pred in [(o, p) for p in preds for o in (-1, 0, 1)]:
            ctx.set_option("steps", steps_opt)
            tag = f"n={n} shape={shape} {kind} leaves={pred.n_leaves} steps={steps_opt} {options}"
            pq.check(L.pqps_filter_scan(ctx.h, carr, len(shape), n, 0, C.byref(pred), out.ids, out.cap, out.count, None), tag)
            k_ids = kernel()
            got = out.ids_value()
            assert len(got) == len(want) and np.array_equal(got, want), (tag, k_ids)
            lists[steps_opt] = got
            pq.check(L.pqps_filter_count(ctx.h, carr, len(shape), n, C.byref(pred), out.count, None), tag)
            k_count = kernel()
            assert out.count_value() == len(want), (tag, k_count)
            for mode, k in (("ids", k_ids), ("count", k_count)):
                two = steps_opt == 1 or (steps_opt < 0 and DEFAULT_S2[mode])
                assert "W0=P12" in k and ("S=2" if two else "S=1") in k and ("NT=true" if nt else "NT=false") in k, (tag, mode, k)
        assert np.array_equal(lists[0], lists[1]) and np.array_equal(lists[0], lists[-1])
    finally:
        ctx.set_option("steps", -1)
        for name, _ in options:
            ctx.set_option(name, -1)
        dev.free()
        out.free()


def check_sizes(sizes, kinds=("plan", "shifted", "cycle"), options=(), nt=False):
    ctx = pq.Context(0)
    try:
        for n in sizes:
            for shape in ((P,), (P, B)):
                for kind in kinds:
                    check_table(ctx, n, shape, kind, seed=n % 1000 + len(shape), options=options, nt=nt)
    finally:
        ctx.close()


@pytest.mark.parametrize("n", SIZES)
def test_two_steps_per_wave(n):
    """Sizes at which a wave has no second step or a partial one, a tile has one step, a group or a supergroup has just ended."""
    check_sizes([n], kinds=("plan", "shifted", "cycle") if n < 10**6 else ("plan",))


@pytest.mark.parametrize("options", [(("list_max", 0),), (("tiny_max", 0),), (("list16", 0),), (("list_max", 0), ("tiny_max", 0), ("list16", 0))],
                         ids=["list_max 0", "tiny_max 0", "list16 0", "bit masks only"])
def test_two_steps_per_wave_fallback_forms(options):
    """No entries in the slots (bit masks / the list area instead), no tiny words (slots instead), no list area (bit masks for the
    fuller steps, as from 268 M rows on), and every non-empty step as a bit mask."""
    check_sizes([73729], kinds=("plan", "cycle"), options=options)


def test_two_steps_per_wave_streaming_loads():
    """The `nt` instantiations (the default from 256 MB of columns on), forced at test sizes in a process of their own."""
    code = ("import sys; sys.path.insert(0, %r); import test_gpu_packed12_steps as t; t.check_sizes(%r, nt=True); print('OK')"
            % (str(q.ROOT / "tests"), NT_SIZES))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, PQPS_NT_LOADS="1"), cwd=str(q.ROOT / "tests"))
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), (p.stdout[-2000:], p.stderr[-2000:])


def test_engine_takes_the_two_step_kernels():
    n = 200003
    host = q.HostSynth(n, seed=0x5EED, full=True)
    eng = pq.HipEngine.synthetic(n, seed=0x5EED)
    try:
        for chain in ([("sudo_used", "=", "FALSE"), "AND", ("user_name", "=", "student1030")], [("user_name", "=", "student1030")]):
            want = host.oracle_scan(chain).tolist()
            assert eng.select_ids(chain) == want, chain
            k = kernel()
            assert "W0=P12" in k and ("S=2" if DEFAULT_S2["ids"] else "S=1") in k, (chain, k)
            assert eng.count(chain) == len(want), chain
            k = kernel()
            assert "W0=P12" in k and ("S=2" if DEFAULT_S2["count"] else "S=1") in k, (chain, k)
    finally:
        eng.close()
