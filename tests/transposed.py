"""The reference of every transposed-product check (y = A^T x, include/smvp_amd.h): the entries with row and column
swapped, the host converter's CSR arrays of them (stable: ascending (new row, new column), ties in input order), and the
oracle's serial loop over those arrays.  Plain functions, no fixtures: test_transposed_host.py pins them against a plain
Python loop, the GPU tests compare bits with them."""
import numpy as np

import oracle_binding as ob
import smvp_toolkit_amd as sm


def swapped(coo):
    """The COO list of A^T: the same entries in the same order, row and column exchanged."""
    coo = np.asarray(coo, dtype=sm.COO_DTYPE)
    return sm.make_coo(coo["col"], coo["row"], coo["val"])


def transposed_csr(coo, cols):
    """(row_ptr, col_ind, val) of the cols x rows matrix A^T as smvp_csr_from_coo builds them from the swapped entries."""
    return sm.csr_from_coo(swapped(coo), cols)


def reference(coo, rows, cols, x):
    """y = A^T x by the oracle's serial loop over transposed_csr; y has `cols` elements."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert x.shape == (rows,)
    rp, ci, v = transposed_csr(coo, cols)
    return ob.csr_spmv(rp, ci, v, x) if cols else np.zeros(0)


def coo_of_csr(row_ptr, col_ind, val):
    """The entries of CSR arrays in storage order."""
    row_ptr = np.asarray(row_ptr)
    return sm.make_coo(np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr)), np.asarray(col_ind)[:row_ptr[-1]],
                       np.asarray(val)[:row_ptr[-1]])


def python_loop(coo, cols, x):
    """The definition itself, in plain Python: per column the entries in ascending (row, input index), acc += val * x[row]."""
    cols_of = [[] for _ in range(cols)]
    for i, (r, c, v) in enumerate(zip(coo["row"].tolist(), coo["col"].tolist(), coo["val"].tolist())):
        cols_of[c].append((r, i, v))
    y = np.zeros(cols, dtype=np.float64)
    xs = [float(t) for t in x]
    for c, entries in enumerate(cols_of):
        acc = 0.0
        for r, i, v in sorted(entries, key=lambda e: (e[0], e[1])):
            acc += v * xs[r]
        y[c] = acc
    return y


def same_bits(a, b):
    """Bit-equal, except that any NaN equals any NaN (the host and the GPU make different NaN payloads)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.shape == b.shape) and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def assert_bits(y, ref, what=""):
    y, ref = np.ascontiguousarray(y, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
    assert y.shape == ref.shape, "%s: shape %s against %s" % (what, y.shape, ref.shape)
    ok = (y.view(np.int64) == ref.view(np.int64)) | (np.isnan(y) & np.isnan(ref))
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError("%s: %d of %d elements differ from the reference's bits; first at %d: %r against %r" % (
            what, (~ok).sum(), ok.size, i, y[i], ref[i]))
