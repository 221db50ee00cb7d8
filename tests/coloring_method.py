"""The multicolour reordering (include/smvp_amd.h: smvp_csr_color / smvp_perm_from_classes / smvp_csr_create_permuted, kernel K23)
restated in numpy and plain Python, and the matrices it is held to.  Plain functions, no fixtures: test_coloring_host.py pins them to
hand-computed values and to the library's own host loop on the CPU, test_gpu_multicolor.py compares the device's results with them.

Why equality everywhere.  key(v) = mix32(v ^ seed) is a bijection, so no two vertices tie; color(v) looks only at neighbours of
larger key: the recurrence has one solution, whatever the order a device evaluates it in.  The permutation is a stable sort, the
permuted arrays are the host converter's of the mapped entries: every integer and every bit has one right answer."""
import functools

import numpy as np

import pcg_tri_method as tri
import smvp_toolkit_amd as sm
import trsv_method as trsv

SEEDS = (0, 1, 0xffffffff)
M32 = 0xffffffff


def mix32(x):
    """The header's five lines on Python ints."""
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def keys(n, seed):
    """key(v) for v < n as uint32, the same lines on numpy words."""
    x = (np.arange(n, dtype=np.uint64) ^ np.uint64(seed & M32)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def neighbours(n, row_ptr, col_ind, t_row_ptr=None, t_col_ind=None):
    """N(v) as a list of sorted lists: the columns u != v of row v, of both patterns where there are two, each once."""
    out = []
    rp, ci = np.asarray(row_ptr).tolist(), np.asarray(col_ind).tolist()
    trp = None if t_row_ptr is None else np.asarray(t_row_ptr).tolist()
    tci = None if t_col_ind is None else np.asarray(t_col_ind).tolist()
    for v in range(n):
        s = set(ci[rp[v]:rp[v + 1]])
        if trp is not None:
            s.update(tci[trp[v]:trp[v + 1]])
        s.discard(v)
        out.append(sorted(s))
    return out


def color(n, row_ptr, col_ind, t_row_ptr=None, t_col_ind=None, seed=0):
    """(color, colors, depth) by the definition: the vertices in descending key order, each the smallest colour no neighbour of
    larger key holds, and 1 + the largest depth among those neighbours."""
    N = neighbours(n, row_ptr, col_ind, t_row_ptr, t_col_ind)
    key = keys(n, seed).tolist()
    assert len(set(key)) == n
    col, dep = [-1] * n, [-1] * n
    for v in sorted(range(n), key=lambda v: -key[v]):
        above = [u for u in N[v] if key[u] > key[v]]
        assert all(col[u] >= 0 for u in above)
        held = {col[u] for u in above}
        c = 0
        while c in held:
            c += 1
        col[v] = c
        dep[v] = 1 + max((dep[u] for u in above), default=-1)
    return np.array(col, dtype=np.int32), (max(col) + 1 if n else 0), (max(dep) + 1 if n else 0)


def max_degree(n, row_ptr, col_ind, t_row_ptr=None, t_col_ind=None):
    return max((len(s) for s in neighbours(n, row_ptr, col_ind, t_row_ptr, t_col_ind)), default=0)


def proper(n, row_ptr, col_ind, col):
    """No stored (i, j), i != j, joins two rows of one colour."""
    r = np.repeat(np.arange(n), np.diff(np.asarray(row_ptr)))
    c = np.asarray(col_ind)[:len(r)]
    col = np.asarray(col)
    return not bool(((col[r] == col[c]) & (r != c)).any())


def transposed_pattern(n, row_ptr, col_ind):
    """(t_row_ptr, t_col_ind): the rows that store each column, ascending."""
    r = np.repeat(np.arange(n), np.diff(np.asarray(row_ptr)))
    c = np.asarray(col_ind)[:len(r)]
    order = np.lexsort((r, c))
    return np.concatenate([[0], np.cumsum(np.bincount(c, minlength=n))]).astype(np.int32), r[order].astype(np.int32)


def symmetric(n, row_ptr, col_ind):
    a = neighbours(n, row_ptr, col_ind)
    b = neighbours(n, *transposed_pattern(n, row_ptr, col_ind))
    return a == b


def perm_from_classes(classes, n_classes):
    """(old_of_new, new_of_old, class_ptr): the new order is by (class, old index) ascending -- a stable argsort."""
    classes = np.asarray(classes, dtype=np.int64)
    old_of_new = np.argsort(classes, kind="stable").astype(np.int32)
    new_of_old = np.empty(len(classes), dtype=np.int32)
    new_of_old[old_of_new] = np.arange(len(classes), dtype=np.int32)
    class_ptr = np.concatenate([[0], np.cumsum(np.bincount(classes, minlength=n_classes))]).astype(np.int32)
    return old_of_new, new_of_old, class_ptr


def mapped_coo(n, row_ptr, col_ind, val, new_of_old):
    """The entries (new_of_old[r], new_of_old[c], val) in storage order."""
    r = np.repeat(np.arange(n), np.diff(np.asarray(row_ptr)))
    p = np.asarray(new_of_old)
    return sm.make_coo(p[r], p[np.asarray(col_ind)[:len(r)]], np.asarray(val)[:len(r)])


def permuted_csr(n, row_ptr, col_ind, val, new_of_old):
    """(row_ptr, col_ind, val) of P A P^T as the host converter smvp_csr_from_coo builds them from the mapped entries."""
    return sm.csr_from_coo(mapped_coo(n, row_ptr, col_ind, val, new_of_old), n)


def levels_after(n, row_ptr, col_ind, col, colors):
    """(levels of LOWER, levels of UPPER) of the pattern renumbered colour by colour, by the library's own host analysis."""
    _, new_of_old, _ = perm_from_classes(col, colors)
    rp, ci, _ = permuted_csr(n, row_ptr, col_ind, np.ones(int(np.asarray(row_ptr)[n])), new_of_old)
    return tuple(sm.trsv_levels(n, rp, ci, uplo)[1] for uplo in (sm.TRSV_LOWER, sm.TRSV_UPPER))


# ---------------------------------------------------------------------------------------------------------------- the matrices
class Pattern:
    """A square pattern with values: n, csr = (row_ptr, col_ind, val), and the references computed once per (at, seed)."""

    def __init__(self, name, n, r, c, v=None, sort=False):
        self.name, self.n = name, int(n)
        r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int32)
        if v is None:
            v = np.random.default_rng(20230 + len(r)).uniform(0.5, 1.5, len(r))
        order = np.lexsort((c, r)) if sort else np.argsort(r, kind="stable")
        row_ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=self.n))]).astype(np.int32)
        self.csr = row_ptr, np.ascontiguousarray(c[order]), np.ascontiguousarray(np.asarray(v, dtype=np.float64)[order])
        self.nnz = len(r)
        self._ref = {}

    def transposed(self):
        return transposed_pattern(self.n, self.csr[0], self.csr[1])

    def reference(self, at, seed):
        """(color, colors, depth) of the restatement, with the transposed pattern where `at`; shared and left unchanged."""
        if (at, seed) not in self._ref:
            t = self.transposed() if at else (None, None)
            col, colors, depth = color(self.n, self.csr[0], self.csr[1], t[0], t[1], seed)
            col.setflags(write=False)
            self._ref[(at, seed)] = (col, colors, depth)
        return self._ref[(at, seed)]


def diagonal(n):
    return Pattern("diagonal(%d)" % n, n, np.arange(n), np.arange(n))


def path(n, ring=False):
    i = np.arange(n)
    r, c = [i], [i]
    if n > 1:
        r += [i[1:], i[:-1]]
        c += [i[:-1], i[1:]]
    if ring and n > 2:
        r += [[0], [n - 1]]
        c += [[n - 1], [0]]
    return Pattern(("ring(%d)" if ring else "path(%d)") % n, n, np.concatenate(r), np.concatenate(c), sort=True)


def complete(k):
    """K_k with its diagonal: k colours, the last of which lies in window (k - 1) // 64 of the mask."""
    r, c = np.divmod(np.arange(k * k), k)
    return Pattern("K%d" % k, k, r, c)


def star(leaves):
    """Vertex 0 joined to `leaves` others: a hub row of leaves + 1 entries, two colours."""
    n = leaves + 1
    i = np.arange(1, n)
    return Pattern("star(%d)" % leaves, n, np.concatenate([np.zeros(n, dtype=np.int64), i, i]), np.concatenate([np.arange(n), np.zeros(leaves, dtype=np.int64), i]))


def banded(n, half):
    """|i - j| <= half stored, diagonal included."""
    rows, cols = [], []
    i = np.arange(n)
    for d in range(-half, half + 1):
        keep = (i + d >= 0) & (i + d < n)
        rows.append(i[keep])
        cols.append(i[keep] + d)
    return Pattern("banded(%d, %d)" % (n, half), n, np.concatenate(rows), np.concatenate(cols), sort=True)


def messy(n=203, seed=20231):
    """Unsorted columns, repeats, explicit self-loops and empty rows; structurally unsymmetric."""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, n, 6 * n)
    r = r[(r % 7) != 3]                                  # rows 3, 10, 17, ... are empty
    c = rng.integers(0, n, len(r))
    r, c = np.concatenate([r, r[:n], r[:50]]), np.concatenate([c, c[:n], r[:50]])   # repeats, then self-loops
    P = Pattern("messy(%d)" % n, n, r, c)
    assert not symmetric(P.n, P.csr[0], P.csr[1]) and (np.diff(P.csr[0]) == 0).any()
    return P


def of_matrix(name, M):
    """A power_iteration.Matrix (cg_method, pcg_tri_method, pbicgstab_method) as a Pattern on its CSR arrays."""
    rp, ci, v = M.csr
    P = Pattern.__new__(Pattern)
    P.name, P.n, P.csr, P.nnz, P._ref = name, M.n, (np.asarray(rp), np.asarray(ci), np.asarray(v)), int(rp[M.n]), {}
    return P


@functools.lru_cache(maxsize=None)
def lap2d(k):
    return of_matrix("lap2d(%d)" % k, tri.lap2d(k))


@functools.lru_cache(maxsize=None)
def sample(name):
    """A golden sample's structure with trsv_method.dominant values."""
    Cs = trsv.sample(name)
    P = Pattern.__new__(Pattern)
    P.name, P.n, P.csr, P.nnz, P._ref = name, Cs.n, Cs.csr, Cs.nnz, {}
    return P


@functools.lru_cache(maxsize=None)
def small_cases():
    """The constructed cases, built once: (Pattern, whether N is symmetric as stored)."""
    return ((diagonal(1), True), (diagonal(40), True), (path(2), True), (path(301), True), (path(300, ring=True), True),
            (complete(65), True), (complete(129), True), (star(1500), True), (lap2d(32), True), (messy(), False))


SAMPLES = ("ibm32", "memplus", "pwt")
