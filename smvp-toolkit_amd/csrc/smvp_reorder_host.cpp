// smvp_reorder_host.cpp -- K23, host side: the multicolour ordering's definition on one core (no HIP in this file: it is part of the
// host-san build), and what smvp_csr_color refuses before any HIP call.
//
// key(v) = mix32(v ^ seed), distinct for distinct v.  color(v) = the smallest integer >= 0 that no neighbour of larger key has;
// depth(v) = 0 without such a neighbour, else 1 + the largest depth among them.  Both recurrences run over the vertices in descending
// key order, so one sort and one O(entries) pass give them.  A neighbour is a stored column u != v of row v, in `row_ptr / col_ind`
// and, where given, in `t_row_ptr / t_col_ind`; repeats count once, values are never looked at.
#include "smvp_common.h"

#include <algorithm>
#include <cstdint>

namespace smvp {

int color_check_opts(const char *fn, const smvp_color_opts_t *opts, const smvp_color_info_t *info)
{
    if (opts && opts->struct_size != sizeof(smvp_color_opts_t))
        return fail(SMVP_ERR_INVALID, "%s: opts->struct_size = %u, this library's smvp_color_opts_t has %zu bytes (call smvp_color_opts_default)", fn,
                    opts->struct_size, sizeof(smvp_color_opts_t));
    if (opts && opts->max_rounds < 1)
        return fail(SMVP_ERR_INVALID, "%s: opts->max_rounds = %d (need max_rounds >= 1)", fn, opts->max_rounds);
    if (info && info->struct_size != sizeof(smvp_color_info_t))
        return fail(SMVP_ERR_INVALID, "%s: info->struct_size = %u, this library's smvp_color_info_t has %zu bytes", fn, info->struct_size,
                    sizeof(smvp_color_info_t));
    return SMVP_OK;
}

namespace {

int check_pattern(const char *which, int rows, const int *row_ptr, const int *col_ind)
{
    if (rows > 0 && row_ptr[0] != 0)
        return fail(SMVP_ERR_INVALID, "smvp_csr_color_host: %srow_ptr[0] = %d, not 0", which, row_ptr[0]);
    for (int r = 0; r < rows; ++r)
        if (row_ptr[r] > row_ptr[r + 1])
            return fail(SMVP_ERR_INVALID, "smvp_csr_color_host: %srow_ptr decreases at row %d", which, r);
    if (rows > 0 && row_ptr[rows] > 0 && !col_ind)
        return fail(SMVP_ERR_INVALID, "smvp_csr_color_host: null %scol_ind", which);
    for (int p = 0; rows > 0 && p < row_ptr[rows]; ++p)
        if (col_ind[p] < 0 || col_ind[p] >= rows)
            return fail(SMVP_ERR_INVALID, "smvp_csr_color_host: %scol_ind[%d] = %d outside [0, %d)", which, p, col_ind[p], rows);
    return SMVP_OK;
}

}  // namespace

}  // namespace smvp

extern "C" void smvp_color_opts_default(smvp_color_opts_t *o)
{
    if (!o)
        return;
    o->struct_size = sizeof(smvp_color_opts_t);
    o->seed = 0;
    o->max_rounds = 4096;
}

extern "C" int smvp_csr_color_host(int rows, const int *row_ptr, const int *col_ind, const int *t_row_ptr, const int *t_col_ind, unsigned seed,
                                   int *color, int *colors, int *depth)
{
    if (rows < 0)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_color_host: rows < 0");
    if (!colors || !depth)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_color_host: null %s", !colors ? "colors" : "depth");
    if (rows > 0 && (!row_ptr || !color))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_color_host: null %s", !row_ptr ? "row_ptr" : "color");
    if (!t_row_ptr != !t_col_ind)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_color_host: t_row_ptr and t_col_ind must both be NULL or both be set");
    if (int rc = smvp::check_pattern("", rows, row_ptr, col_ind))
        return rc;
    const bool both = t_row_ptr != nullptr && rows > 0;
    if (both)
        if (int rc = smvp::check_pattern("t_", rows, t_row_ptr, t_col_ind))
            return rc;
    const size_t n = (size_t)rows;
    std::vector<uint64_t> by_key(n);  // key << 32 | vertex: keys are distinct, the low word only rides along
    for (size_t v = 0; v < n; ++v)
        by_key[v] = (uint64_t)smvp::mix32((uint32_t)v ^ seed) << 32 | v;
    std::sort(by_key.begin(), by_key.end());
    std::vector<int> dep(n, -1);   // -1: not reached yet, i.e. of smaller key than the vertex in hand
    std::vector<int> col(n, -1);
    std::vector<int> taken;        // taken[c] == stamp of the vertex in hand: a neighbour of larger key holds colour c
    int ncolors = 0, deepest = -1;
    for (size_t k = n; k-- > 0;) {
        const int v = (int)(by_key[k] & 0xffffffffu);
        int d = 0, seen = 0;
        for (int side = 0; side < (both ? 2 : 1); ++side) {
            const int *rp = side ? t_row_ptr : row_ptr, *ci = side ? t_col_ind : col_ind;
            for (int p = rp[v]; p < rp[v + 1]; ++p) {
                const int u = ci[p];
                if (u == v || dep[(size_t)u] < 0)
                    continue;
                d = std::max(d, dep[(size_t)u] + 1);
                const size_t c = (size_t)col[(size_t)u];
                if (c >= taken.size())
                    taken.resize(c + 1, -1);
                taken[c] = v;
                ++seen;
            }
        }
        int c = 0;
        while (seen > 0 && (size_t)c < taken.size() && taken[(size_t)c] == v)
            ++c;
        col[(size_t)v] = c;
        dep[(size_t)v] = d;
        ncolors = std::max(ncolors, c + 1);
        deepest = std::max(deepest, d);
    }
    for (size_t v = 0; v < n; ++v)
        color[v] = col[v];
    *colors = ncolors;
    *depth = deepest + 1;
    return SMVP_OK;
}
