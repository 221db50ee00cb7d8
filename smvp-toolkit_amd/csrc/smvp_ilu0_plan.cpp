// smvp_ilu0_plan.cpp -- K17, host side: what an ILU(0) on a CSR pattern asks of the pattern (smvp_csr_ilu0_check) and the
// factorisation itself as the serial loop of include/smvp_amd.h (smvp_csr_ilu0_host): the definition every element of the device's
// factor is held to, and the only CPU baseline.  No HIP in this file: it is part of the host-san build.  The schedule is K15's LOWER
// analysis (smvp_trsv_plan.cpp): row i reads exactly the rows k < i for which (i, k) is stored.
#include "smvp_common.h"

namespace smvp {

// The first row that keeps an ILU(0) from being defined on this pattern, or SMVP_OK: row_ptr a non-decreasing sequence from 0 and
// every column inside [0, rows) (else SMVP_ERR_INVALID); every row's columns strictly ascending and (i, i) among them (else
// SMVP_ERR_UNSUPPORTED).  Nothing is written but *bad_row and the error text.
static int ilu0_scan(const char *fn, int rows, const int *row_ptr, const int *col_ind, int *bad_row)
{
    auto bad = [&](int row) {
        if (bad_row)
            *bad_row = row;
    };
    if (rows > 0 && row_ptr[0] != 0) {
        bad(0);
        return fail(SMVP_ERR_INVALID, "%s: row_ptr[0] = %d, not 0", fn, row_ptr[0]);
    }
    for (int i = 0; i < rows; ++i)
        if (row_ptr[i] > row_ptr[i + 1]) {
            bad(i);
            return fail(SMVP_ERR_INVALID, "%s: row_ptr decreases at row %d", fn, i);
        }
    if (rows > 0 && row_ptr[rows] > 0 && !col_ind)
        return fail(SMVP_ERR_INVALID, "%s: null col_ind", fn);
    for (int i = 0; i < rows; ++i) {
        bool diag = false;
        for (int p = row_ptr[i]; p < row_ptr[i + 1]; ++p) {
            const int c = col_ind[p];
            if (c < 0 || c >= rows) {
                bad(i);
                return fail(SMVP_ERR_INVALID, "%s: row %d: col_ind[%d] = %d outside [0, %d)", fn, i, p, c, rows);
            }
            if (p > row_ptr[i] && c <= col_ind[p - 1]) {
                bad(i);
                return fail(SMVP_ERR_UNSUPPORTED, "%s: row %d: column %d at position %d follows column %d (%s): an ILU(0) needs every "
                                                  "row's columns strictly ascending",
                            fn, i, c, p, col_ind[p - 1], c == col_ind[p - 1] ? "a repeated column" : "not sorted");
            }
            diag = diag || c == i;
        }
        if (!diag) {
            bad(i);
            return fail(SMVP_ERR_UNSUPPORTED, "%s: row %d stores no diagonal entry (%d, %d)", fn, i, i, i);
        }
    }
    return SMVP_OK;
}

int ilu0_check(const char *fn, int rows, const int *row_ptr, const int *col_ind, int *diag_pos, int *bad_row)
{
    if (int rc = ilu0_scan(fn, rows, row_ptr, col_ind, bad_row))
        return rc;
    if (diag_pos)
        for (int i = 0; i < rows; ++i) {
            int p = row_ptr[i];
            while (col_ind[p] != i)
                ++p;  // (the scan found it inside the row)
            diag_pos[i] = p;
        }
    if (bad_row)
        *bad_row = -1;
    return SMVP_OK;
}

}  // namespace smvp

extern "C" int smvp_csr_ilu0_check(int rows, const int *row_ptr, const int *col_ind, int *diag_pos, int *bad_row)
{
    if (rows < 0 || (rows > 0 && !row_ptr))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_ilu0_check: %s", rows < 0 ? "rows < 0" : "null row_ptr");
    return smvp::ilu0_check("smvp_csr_ilu0_check", rows, row_ptr, col_ind, diag_pos, bad_row);
}

// The loop of the header, row by row.  where[c] is the position of column c in the row at hand (-1: not stored), so "does row i store
// this column" is one look; every w[t] takes at most one update per pivot and the pivots come in ascending k.  The product is a
// statement of its own: rounded before the difference (this file is compiled without a fused multiply-add, as the whole library).
extern "C" int smvp_csr_ilu0_host(int rows, const int *row_ptr, const int *col_ind, const double *val, double *val_out)
{
    if (rows < 0 || (rows > 0 && !row_ptr))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_ilu0_host: %s", rows < 0 ? "rows < 0" : "null row_ptr");
    std::vector<int> diag_pos((size_t)rows);
    if (int rc = smvp::ilu0_check("smvp_csr_ilu0_host", rows, row_ptr, col_ind, diag_pos.data(), nullptr))
        return rc;
    if (rows > 0 && row_ptr[rows] > 0 && (!val || !val_out))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_ilu0_host: null %s", !val ? "val" : "val_out");
    std::vector<int> where((size_t)rows, -1);
    double *F = val_out;
    for (int i = 0; i < rows; ++i) {
        const int a = row_ptr[i], z = row_ptr[i + 1];
        for (int p = a; p < z; ++p) {
            F[p] = val[p];
            where[(size_t)col_ind[p]] = p;
        }
        for (int p = a; p < diag_pos[(size_t)i]; ++p) {
            const int k = col_ind[p];
            const double l = F[p] / F[diag_pos[(size_t)k]];
            F[p] = l;
            for (int q = diag_pos[(size_t)k] + 1; q < row_ptr[k + 1]; ++q) {
                const int t = where[(size_t)col_ind[q]];
                if (t >= 0) {
                    const volatile double product = l * F[q];
                    F[t] = F[t] - product;
                }
            }
        }
        for (int p = a; p < z; ++p)
            where[(size_t)col_ind[p]] = -1;
    }
    return SMVP_OK;
}
