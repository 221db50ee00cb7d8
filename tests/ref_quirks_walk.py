"""What test_gpu_replan.py::test_tjds_walk_through_ref_quirks_and_modes multiplies: two square TJDS matrices, one for each
regime of the reference's unwritten start_pos terminator, with their operand and the oracle's products.

Plain functions (no fixtures, no GPU): test_ref_quirks_walk_host.py holds them to their conditions.

N columns of 5 ... 18 entries in distinct random rows, about 35 000 entries: several tiles at 256 and at 2048 entries per tile.
Column 0 has LONGEST entries, more than any of those, so the ref-quirks product (diagonals 0 ... length of column 0) covers
every diagonal and differs from the true product by the operand's index and by the last diagonal alone:
  "single"  column 0 is the only longest column: the last diagonal has one entry, last_diag_single = 1, and the ref-quirks
            product loses that entry;
  "pair"    columns 0 and 1 are both longest: the last diagonal has two entries, last_diag_single = 0.
Values and operand are non-zero integers of magnitude 1 ... 8 (adopted.int_values), so every sum is exact in any order and the
atomic kernel has one answer.
"""
import functools
from types import SimpleNamespace

import numpy as np

import oracle_binding as ob
import smvp_toolkit_amd as sm
from adopted import int_values

N = 3000
LONGEST = 25
LONGEST_COLUMNS = {"single": 1, "pair": 2}


@functools.lru_cache(maxsize=None)
def matrix(name):
    """-> namespace: rows, cols, coo (row-major), x, oracle (ob.tjds_build's arrays and flags), y {ref-quirks on?: the oracle's
    product}; computed once and left unchanged."""
    rng = np.random.default_rng(1013 + LONGEST_COLUMNS[name])
    lens = rng.integers(5, 19, N)
    lens[:LONGEST_COLUMNS[name]] = LONGEST
    col = np.repeat(np.arange(N), lens)
    row = np.concatenate([rng.choice(N, n, replace=False) for n in lens])
    order = np.lexsort((col, row))
    coo = sm.make_coo(row[order], col[order], int_values(rng, len(row), 1, 8))
    x = int_values(rng, N, 1, 8)
    oracle = ob.tjds_build(coo, N, N)
    y = {quirks: ob.tjds_spmv(oracle, x, refquirks=quirks) for quirks in (False, True)}
    for a in (coo, x, y[False], y[True]):
        a.setflags(write=False)
    return SimpleNamespace(rows=N, cols=N, coo=coo, x=x, oracle=oracle, y=y)
