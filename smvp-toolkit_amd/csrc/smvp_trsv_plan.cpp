// smvp_trsv_plan.cpp -- K15, host side: the structural analysis of a sparse triangular solve (no HIP in this file: it is part of
// the host-san build).  level(i) = 0 where row i has no stored off-diagonal entry inside the triangle, else 1 + the largest level
// of the rows those entries name.  The recurrence is sequential, so it is one O(nnz) pass over the rows in the order the solve
// takes them (ascending for LOWER, descending for UPPER); a counting sort by level then lists the rows by (level, row) ascending.
// Levels are structural: an explicitly stored 0.0 counts, values are never looked at.
#include "smvp_common.h"

namespace smvp {

int trsv_analyse(int rows, const int *row_ptr, const int *col_ind, int uplo, TrsvSchedule *out)
{
    const bool upper = uplo == SMVP_TRSV_UPPER;
    out->level_of_row.assign((size_t)rows, 0);
    out->level_ptr.assign(1, 0);
    out->order.assign((size_t)rows, 0);
    out->levels = out->max_level_width = out->missing_diagonals = 0;
    out->off_entries = out->diag_entries = 0;
    out->max_row_entries = 0;
    if (rows > 0 && row_ptr[0] != 0)
        return fail(SMVP_ERR_INVALID, "smvp_csr_trsv_levels: row_ptr[0] = %d, not 0", row_ptr[0]);
    for (int r = 0; r < rows; ++r)
        if (row_ptr[r] > row_ptr[r + 1])
            return fail(SMVP_ERR_INVALID, "smvp_csr_trsv_levels: row_ptr decreases at row %d", r);
    if (rows > 0 && row_ptr[rows] > 0 && !col_ind)
        return fail(SMVP_ERR_INVALID, "smvp_csr_trsv_levels: null col_ind");
    std::vector<int> &level = out->level_of_row;
    int deepest = -1;
    for (int k = 0; k < rows; ++k) {
        const int i = upper ? rows - 1 - k : k;
        int lv = 0, mine = 0;
        bool diag = false;
        for (int p = row_ptr[i]; p < row_ptr[i + 1]; ++p) {
            const int c = col_ind[p];
            if (c < 0 || c >= rows)
                return fail(SMVP_ERR_INVALID, "smvp_csr_trsv_levels: col_ind[%d] = %d outside [0, %d)", p, c, rows);
            if (c == i) {
                diag = true;
                ++out->diag_entries;
                ++mine;
            } else if (upper ? c > i : c < i) {
                ++out->off_entries;
                ++mine;
                if (level[(size_t)c] + 1 > lv)
                    lv = level[(size_t)c] + 1;
            }
        }
        level[(size_t)i] = lv;
        if (mine > out->max_row_entries)
            out->max_row_entries = mine;
        if (lv > deepest)
            deepest = lv;
        if (!diag)
            ++out->missing_diagonals;
    }
    out->levels = deepest + 1;
    out->level_ptr.assign((size_t)out->levels + 1, 0);
    for (int i = 0; i < rows; ++i)
        ++out->level_ptr[(size_t)level[(size_t)i] + 1];
    for (int l = 0; l < out->levels; ++l) {
        if (out->level_ptr[(size_t)l + 1] > out->max_level_width)
            out->max_level_width = out->level_ptr[(size_t)l + 1];
        out->level_ptr[(size_t)l + 1] += out->level_ptr[(size_t)l];
    }
    std::vector<int> next(out->level_ptr.begin(), out->level_ptr.end() - 1);
    for (int i = 0; i < rows; ++i)  // ascending row index inside every level
        out->order[(size_t)next[(size_t)level[(size_t)i]]++] = i;
    return SMVP_OK;
}

// A maximal run of consecutive levels of at most chain_width rows each is one launch (a chain); every wider level is one.
void trsv_launches(const std::vector<int> &level_ptr, int chain_width, std::vector<TrsvLaunch> *out, int *chains)
{
    out->clear();
    *chains = 0;
    const int levels = (int)level_ptr.size() - 1;
    for (int l = 0; l < levels;) {
        int e = l;
        while (e < levels && level_ptr[(size_t)e + 1] - level_ptr[(size_t)e] <= chain_width)
            ++e;
        if (e > l) {
            out->push_back({l, e, true});
            ++*chains;
            l = e;
        } else {
            out->push_back({l, l + 1, false});
            ++l;
        }
    }
}

// K21: the storage range [begin_i, end_i) of every row -- the smallest that holds all of the row's entries inside the triangle and,
// for DIAG_STORED, on the diagonal; [row_ptr[i], row_ptr[i]) where the row has none.  Everything of the row outside the range is of
// the skipped kind, so a walk of the range alone adds the same values in the same order as a walk of the row.  Rows with ascending
// columns get a tight range (nothing skipped inside it); an unsorted row a loose one, which is still right.  col_ind was checked by
// trsv_analyse.
void trsv_ranges(int rows, const int *row_ptr, const int *col_ind, int uplo, int diag, std::vector<int> *begin, std::vector<int> *end,
                 long long *entries, int *longest)
{
    const bool upper = uplo == SMVP_TRSV_UPPER, unit = diag == SMVP_TRSV_DIAG_UNIT;
    begin->assign((size_t)rows, 0);
    end->assign((size_t)rows, 0);
    *entries = 0;
    *longest = 0;
    for (int i = 0; i < rows; ++i) {
        int a = row_ptr[i], z = row_ptr[i];
        bool any = false;
        for (int p = row_ptr[i]; p < row_ptr[i + 1]; ++p) {
            const int c = col_ind[p];
            if (c == i ? !unit : (upper ? c > i : c < i)) {
                if (!any)
                    a = p;
                any = true;
                z = p + 1;
            }
        }
        (*begin)[(size_t)i] = a;
        (*end)[(size_t)i] = z;
        *entries += z - a;
        if (z - a > *longest)
            *longest = z - a;
    }
}

}  // namespace smvp

extern "C" int smvp_csr_trsv_levels(int rows, const int *row_ptr, const int *col_ind, int uplo, int *level_of_row, int *levels)
{
    if (uplo != SMVP_TRSV_LOWER && uplo != SMVP_TRSV_UPPER)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_trsv_levels: uplo = %d is neither SMVP_TRSV_LOWER nor SMVP_TRSV_UPPER", uplo);
    if (rows < 0 || !levels)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_trsv_levels: %s", rows < 0 ? "rows < 0" : "null levels");
    if (rows > 0 && (!row_ptr || !level_of_row))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_trsv_levels: null %s", !row_ptr ? "row_ptr" : "level_of_row");
    smvp::TrsvSchedule s;
    if (int rc = smvp::trsv_analyse(rows, row_ptr, col_ind, uplo, &s))
        return rc;
    for (int i = 0; i < rows; ++i)
        level_of_row[i] = s.level_of_row[(size_t)i];
    *levels = s.levels;
    return SMVP_OK;
}
