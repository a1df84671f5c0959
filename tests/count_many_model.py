"""numpy model of count_many_scan_kernel (csrc/count_many_kernels.hpp): what pqps_filter_count_many computes from a
pqps_count_many -- the hit mask of every shared leaf once, then every query's jump program, run BACKWARDS on those masks as
the kernel runs it.  Test-only, and independent of kernel_model.evaluate (which walks a pqps_predicate forwards)."""
import numpy as np

import qpelib as q

pq = q.pq


def leaf_hits(leaf, v):
    """The window test of pqps_leaf on one column: 64-bit arithmetic for an 8-byte column, 32-bit for everything else."""
    if v.dtype.itemsize == 8:
        return (v.astype(np.uint64) - np.uint64(leaf.lo)) <= np.uint64(leaf.span)
    x = v.astype(np.int64).astype(np.uint32) if v.dtype == np.int32 else v.astype(np.uint32)
    return (x - np.uint32(leaf.lo & 0xFFFFFFFF)) <= np.uint32(leaf.span & 0xFFFFFFFF)


def evaluate(prog, col_arrays, n_rows=None):
    """col_arrays[slot] = numpy array of the batch's column `slot` (a bit plane as its 0 / 1 bytes).  -> one bool mask per
    query.  n_rows: for a batch without columns."""
    n = len(col_arrays[0]) if col_arrays else n_rows
    hits = [leaf_hits(prog.leaf[k], col_arrays[prog.leaf[k].column]) for k in range(prog.n_leaves)]
    out = []
    for i in range(prog.n_queries):
        p = prog.query[i]
        if p.n_steps == 0:
            out.append(np.full(n, bool(p.constant)))
            continue
        val = [None] * p.n_steps

        def target(t, s):
            if t == pq.ACCEPT:
                return np.ones(n, dtype=bool)
            if t == pq.REJECT:
                return np.zeros(n, dtype=bool)
            assert s < t < p.n_steps, "jumps go forward"
            return val[t]
        for s in range(p.n_steps - 1, -1, -1):
            m = hits[p.leaf[s]]
            val[s] = (m & target(p.on_true[s], s)) | (~m & target(p.on_false[s], s))
        out.append(val[0])
    return out


def counts(prog, col_arrays, n_rows=None):
    return [int(m.sum()) for m in evaluate(prog, col_arrays, n_rows)]


def make_prog(leaves, queries, n_columns):
    """leaves = [(column slot, lo, span), ...]; queries = [[(leaf slot, on_true, on_false), ...] | True | False, ...]"""
    prog = pq.CountMany()
    prog.n_queries, prog.n_leaves, prog.n_columns = len(queries), len(leaves), n_columns
    for k, (c, lo, span) in enumerate(leaves[:pq.MAX_LEAVES]):
        prog.leaf[k] = pq.Leaf(c, 0, lo & (2**64 - 1), span & (2**64 - 1))
    for i, steps in enumerate(queries[:pq.COUNT_MANY_MAX]):
        if isinstance(steps, bool):
            prog.query[i].n_steps, prog.query[i].constant = 0, int(steps)
            continue
        prog.query[i].n_steps = len(steps)
        for s, (k, t, f) in enumerate(steps[:pq.TT_LEAVES]):
            prog.query[i].leaf[s], prog.query[i].on_true[s], prog.query[i].on_false[s] = k, t, f
    return prog
