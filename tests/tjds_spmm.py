"""The reference of every check of the forward block product from a TJDS handle (Y = A X, smvp_tjds_spmm, K10): the oracle's
serial TJDS loop (orc_tjds_spmv: y[row_ind[j]] += val[j] * x[perm[j - start_pos[d]]] for the positions j in ascending order, so
a row is summed in ascending TJDS position, each product rounded before the add) run on every column of X.  Plain functions, no
fixtures: test_tjds_spmm_host.py and test_gpu_tjds_spmm.py share them."""
import numpy as np

import oracle_binding as ob
import transposed as tr


def reference_block(t, X):
    """A X column by column over the host TJDS arrays t (sm.tjds_from_coo or ob.tjds_build); (rows, k)."""
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim == 2 and X.shape[0] == t.cols
    if t.rows == 0:
        return np.zeros((0, X.shape[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([ob.tjds_spmv(t, np.ascontiguousarray(X[:, v])) for v in range(X.shape[1])], axis=1)


def assert_block(Y, ref, what):
    """Equality of bits (any NaN equals any NaN) on every column."""
    Y, ref = np.asarray(Y), np.asarray(ref)
    assert Y.shape == ref.shape, "%s: shape %s against %s" % (what, Y.shape, ref.shape)
    for v in range(ref.shape[1]):
        tr.assert_bits(Y[:, v], ref[:, v], "%s, vector %d" % (what, v))
