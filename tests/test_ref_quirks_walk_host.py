"""Host: the two matrices of the ref-quirks walk (ref_quirks_walk.py) are what the GPU test needs them to be."""
import numpy as np
import pytest

import ref_quirks_walk as rq
import smvp_toolkit_amd as sm


@pytest.mark.parametrize("name, single", [("single", 1), ("pair", 0)])
def test_the_two_matrices_are_the_two_regimes_of_the_last_diagonal(name, single):
    m = rq.matrix(name)
    t = m.oracle
    assert 30_000 <= len(m.coo) <= 40_000 and m.rows == m.cols == rq.N
    assert t.last_diag_single == single
    assert t.start_pos[-1] - t.start_pos[-2] == rq.LONGEST_COLUMNS[name]       # entries of the last diagonal
    assert t.num_diag == t.ref_num_tjdiag == rq.LONGEST                        # the ref-quirks loop reaches every diagonal
    ours = sm.tjds_from_coo(m.coo, m.rows, m.cols)                             # (whose flags the handle is given)
    assert (ours.num_diag, ours.ref_num_tjdiag, ours.last_diag_single) == (t.num_diag, t.ref_num_tjdiag, single)
    # the walk proves something only if the two products differ
    assert not np.array_equal(m.y[True], m.y[False])
    for y in m.y.values():                                                     # every sum is an integer a double holds
        assert np.array_equal(y, np.rint(y)) and np.abs(y).max() < 2 ** 53
