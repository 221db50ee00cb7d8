"""The matrix of the size-ceiling tests (test_gpu_ceiling.py): a closed-form CSR matrix of exactly K_MAX entries, the most
smvp_csr_create and smvp_tjds_create accept, built chunk by chunk with torch on whatever device the caller names.

Rows, in order (layout()):
  banded     rows [0, rb): 8 ... 16 entries in the columns r + 2 ... r + len + 1.  Tiles of them span a few hundred columns
             (16-bit column offsets), every row is near the diagonal at the default band of the binned plan (and short: the
             near-window kernel takes whole blocks of them), but no entry lies within 1 of it (band 1: all far);
  scattered  rows [rb, rb + rs): 1 ... 79 entries, entry j of a row of len in column j * (cols // len) + hash: ascending,
             distinct, spread over all columns (wide tiles, far entries);
  long       row rb + rs: the rest of the entries (LONG_MIN ... LONG_MIN + 55, scattered like the rows before it); it crosses
             the edges of the last tiles and ends on entry K_MAX - 1;
  empty      the rows after it.
Row lengths come in pairs (base + d, base - d), d a hash of the pair, so every region's total is base x rows exactly and
row_ptr[-1] is K_MAX by construction.  Values and operands are non-zero integers of magnitude <= 8: every product and every
partial sum is exact in fp64, so every kernel, in any order of summation, must give the int64 reference bit for bit.

Plain functions of torch tensors: the CPU tests (test_ceiling_helpers.py) run them on small layouts.
"""
import math

K_MAX = 2 ** 31 - 1 - 65536      # kMaxEntries (smvp_common.h)
ROWS = 1 << 27                   # rows = columns of the full-size matrix: about 16 entries per row
EMPTY_TAIL = 1000                # empty rows after the long row (one more when that makes the other regions even)
BAND_BASE, BAND_W = 12, 4
SCAT_BASE, SCAT_W = 40, 39
LONG_MIN = 5120                  # > 2048: the long row crosses tile edges; <= 16384: AUTO keeps the one-launch tile kernel
M32 = (1 << 32) - 1
SALT_SCAT, SALT_COL, SALT_VAL, SALT_X = 0x3C6EF372, 0x1B873593, 0x5BD1E995, 0x27D4EB2F


def layout(rows=ROWS, nnz=K_MAX, empty_tail=EMPTY_TAIL, long_min=LONG_MIN):
    """{rows, nnz, rb, rs, long_row, long_len, first_empty}: rb banded + rs scattered rows (both even), then one long row
    that takes the rest, then empty rows."""
    m = rows - empty_tail - 1
    m -= m & 1
    rest = nnz - BAND_BASE * m
    rs = 2 * ((rest - long_min) // (2 * (SCAT_BASE - BAND_BASE)))
    assert 0 <= rs <= m, "no layout of %d entries in %d rows" % (nnz, rows)
    rb = m - rs
    long_len = nnz - BAND_BASE * rb - SCAT_BASE * rs
    assert long_min <= long_len < long_min + 2 * (SCAT_BASE - BAND_BASE)
    return {"rows": rows, "nnz": nnz, "rb": rb, "rs": rs, "long_row": m, "long_len": long_len, "first_empty": m + 1}


def mix(torch, x):
    """A 32-bit hash of non-negative int64 values (< 2^62), in int64 arithmetic that cannot overflow: the same bits on any
    device."""
    x = (x ^ (x >> 32)) & M32
    x = ((x * 0x45D9F3B) & M32) ^ (x >> 16)
    x = (x * 0x45D9F3B) & M32
    return x ^ (x >> 16)


def row_lengths(torch, L, r0, r1, device="cpu"):
    """int64 lengths of rows [r0, r1)."""
    r = torch.arange(r0, r1, dtype=torch.int64, device=device)
    lens = torch.zeros_like(r)
    rb, rs = L["rb"], L["rs"]
    for lo, hi, base, w, salt in ((0, rb, BAND_BASE, BAND_W, 0), (rb, rb + rs, SCAT_BASE, SCAT_W, SALT_SCAT)):
        sel = (r >= lo) & (r < hi)
        q = r[sel] - lo
        d = mix(torch, (q >> 1) + salt) % (2 * w + 1) - w
        lens[sel] = base + torch.where((q & 1) == 0, d, -d)
    lens[r == L["long_row"]] = L["long_len"]
    return lens


def row_ptr64(torch, L, device="cpu", chunk=1 << 22):
    """int64 row_ptr[rows + 1] of the layout."""
    out = torch.empty(L["rows"] + 1, dtype=torch.int64, device=device)
    out[0] = 0
    run = 0
    for r0 in range(0, L["rows"], chunk):
        r1 = min(L["rows"], r0 + chunk)
        c = torch.cumsum(row_lengths(torch, L, r0, r1, device), 0) + run
        out[r0 + 1:r1 + 1] = c
        run = int(c[-1]) if r1 > r0 else run
    return out


def x_int(torch, cols, device="cpu"):
    """The operand: non-zero integers in [-8, 8], int64."""
    h = mix(torch, torch.arange(cols, dtype=torch.int64, device=device) + SALT_X)
    return (h % 8 + 1) * torch.where((h >> 8) & 1 == 1, 1, -1)


def entries(torch, L, rp64, r0, r1, device="cpu"):
    """(row, col, val) of the entries of rows [r0, r1), int64 tensors: row of each entry, its column, its integer value."""
    lens = rp64[r0 + 1:r1 + 1] - rp64[r0:r1]
    row = torch.repeat_interleave(torch.arange(r0, r1, dtype=torch.int64, device=device), lens)
    e = torch.arange(int(rp64[r0]), int(rp64[r1]), dtype=torch.int64, device=device)
    j = e - rp64[row]
    n = lens[row - r0]
    cols = L["rows"]
    seg = cols // torch.clamp(n, min=1)
    scattered = mix(torch, (row << 7) + j + SALT_COL) % seg + j * seg
    col = torch.where(row < L["rb"], row + 2 + j, scattered)
    h = mix(torch, e + SALT_VAL)
    val = (h % 8 + 1) * torch.where((h >> 8) & 1 == 1, 1, -1)
    return row, col, val


def build(torch, L, device="cpu", spare=1, chunk=1 << 21):
    """(row_ptr int32, col_ind int32, val float64, y_ref float64) on `device`: col_ind and val hold `spare` more elements
    than the matrix (zero; the ceiling's refusal test claims one more entry), y_ref = A x_int summed in int64 row chunks."""
    rp64 = row_ptr64(torch, L, device)
    assert int(rp64[-1]) == L["nnz"]
    nnz = L["nnz"]
    col_ind = torch.zeros(nnz + spare, dtype=torch.int32, device=device)
    val = torch.zeros(nnz + spare, dtype=torch.float64, device=device)
    x = x_int(torch, L["rows"], device)
    y = torch.zeros(L["rows"], dtype=torch.int64, device=device)
    for r0 in range(0, L["first_empty"], chunk):
        r1 = min(L["first_empty"], r0 + chunk)
        row, col, v = entries(torch, L, rp64, r0, r1, device)
        e0, e1 = int(rp64[r0]), int(rp64[r1])
        col_ind[e0:e1] = col.to(torch.int32)
        val[e0:e1] = v.to(torch.float64)
        y.index_add_(0, row, v * x[col])
        del row, col, v
    assert int(y.abs().max()) < 2 ** 53
    return rp64.to(torch.int32), col_ind, val, y.to(torch.float64)


def checksum(torch, a, chunk=1 << 28):
    """An order-sensitive int64 checksum of a tensor's bits (int32 / float64), in chunks."""
    bits = a.view(torch.int32) if a.dtype == torch.float64 else a
    s = 0
    for i in range(0, bits.numel(), chunk):
        b = bits[i:i + chunk].to(torch.int64)
        w = torch.arange(i, i + b.numel(), dtype=torch.int64, device=b.device) % 65521 + 1
        s = (s + int((b * w).sum())) % (1 << 61)
    return s


def coo_permutation(n):
    """(a, b): position p of the shuffled COO holds entry (a p + b) mod n -- a bijection of [0, n) when gcd(a, n) == 1."""
    a = 2654435761 % n
    while math.gcd(a, n) != 1:
        a += 1
    return a, 12345 % n


def build_coo(torch, row_ptr, col_ind, val, nnz, device, chunk=1 << 26):
    """The matrix as a COO (smvp_coo_t: int row, int col, double val; 16 B per entry) in the order of coo_permutation, as a
    uint8 tensor."""
    a, b = coo_permutation(nnz)
    buf = torch.empty(16 * nnz, dtype=torch.uint8, device=device)
    i32 = buf.view(torch.int32).view(nnz, 4)
    f64 = buf.view(torch.float64).view(nnz, 2)
    rp = row_ptr.to(torch.int64)
    for p0 in range(0, nnz, chunk):
        p = torch.arange(p0, min(nnz, p0 + chunk), dtype=torch.int64, device=device)
        e = (p * a + b) % nnz
        i32[p0:p0 + len(p), 0] = (torch.searchsorted(rp, e, right=True) - 1).to(torch.int32)
        i32[p0:p0 + len(p), 1] = col_ind[e]
        f64[p0:p0 + len(p), 1] = val[e]
    return buf


# ------------------------------------------------------------------------------- the binned plan's 32-bit stream guard
def binned_far_count(torch, row_ptr, col_ind, band, row_cap, chunk=1 << 22):
    """What build_binned_plan counts as far (smvp_binned.hip, bin_classify / bin_cap_rows): entries with |column - row| > band,
    except in rows with more than row_cap of them (those stay near)."""
    rows = row_ptr.numel() - 1
    rp = row_ptr.to(torch.int64)
    nf = 0
    for r0 in range(0, rows, chunk):
        r1 = min(rows, r0 + chunk)
        e0, e1 = int(rp[r0]), int(rp[r1])
        if e1 == e0:
            continue
        lens = rp[r0 + 1:r1 + 1] - rp[r0:r1]
        row = torch.repeat_interleave(torch.arange(r0, r1, dtype=torch.int64, device=rp.device), lens)
        far = ((col_ind[e0:e1].to(torch.int64) - row).abs() > band).to(torch.int64)
        per_row = torch.zeros(r1 - r0, dtype=torch.int64, device=rp.device).index_add_(0, row - r0, far)
        nf += int(per_row[per_row <= row_cap].sum())
    return nf
