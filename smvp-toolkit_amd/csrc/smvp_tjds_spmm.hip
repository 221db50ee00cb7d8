// smvp_tjds_spmm.hip -- K10: Y = A X for a block of k vectors from a TJDS handle (smvp_tjds_spmm; new: the reference multiplies
// by one x, main-cli.c:1013-1020).
//
//   Y(r, v) = sum over the TJDS positions j with row_ind[j] == r, ascending, of  val[j] * X(perm[j - start_pos[d(j)]], v)
//
// X is cols x k and Y rows x k, row-major with leading dimensions ldx / ldy.  K7's walk (smvp_spmm.hip) over the entries
// regrouped by row, with one more indirection: the plan names an entry by its TJDS position and its original column, and the
// value is read from val itself through the position -- no copy of val, so val of adopted arrays changed in place is seen.
//
//   * the plan (built on the device by the first smvp_tjds_spmm of a handle, buffers of its own): ptr[rows + 1]; pos[nnz], the
//     TJDS positions grouped by row and ascending inside a row (smvp_prim.h's stable radix sort on row_ind); col[nnz] =
//     perm[pos - start_pos[d]], the original column; order[rows], K7's row order -- inside blocks of kSpmmBlockRows consecutive
//     rows the longest first, stable (build_spmm_order, shared with K7);
//   * a group of G adjacent lanes (G = 1, 2, 4, 8, 16: the smallest power of two >= the vectors of the pass) takes one row, lane
//     v holds vector v0 + v; a wavefront covers 64 / G rows of the plan's order.  Passes of one vector (G = 1) keep the rows in
//     their own order, as in K7;
//   * per batch of kTjdsSpmmU entries the group first loads the batch's pos and col -- entry u by lane u % G, handed round with
//     __shfl of width G -- then issues val[pos] and the gathers X[(long long)col * ldx + v] together (both depend on the first
//     stage only), then adds the products IN ENTRY ORDER.  The last batch of a row re-reads the row's last entry in its unused
//     slots and leaves them out of the sum with a select (never 0 * X: X may hold NaN or Inf in columns the row does not
//     store); a lane with v >= nv gathers its neighbour's vector and stores nothing;
//   * every offset into X and Y is 64-bit (col * ldx and row * ldy pass 2^31 for ordinary sizes); positions stay 32-bit
//     (nnz <= 2^31 - 1 - 65536);
//   * placement: a workgroup holds 256 / G rows; workgroups are dealt to the XCDs by tile_of_block in groups of
//     kSpmmBlockRows / (256 / G), so that one XCD's turn is one sorted block (K7's placement);
//   * no atomics, no LDS, no barriers.  A row is never split between groups and a (row, vector) sum never between lanes: every
//     Y(r, v) is the serial sum over the row in TJDS position order, each product rounded before it is added
//     (-ffp-contract=off), the same bits on every run.
#include "smvp_common.h"
#include "smvp_kernels.h"

#include <algorithm>
#include <cstdio>
#include <string>

namespace smvp {

namespace {

constexpr int kTjdsSpmmBlock = 256;  // threads per workgroup
#ifndef SMVP_TJDS_SPMM_U
#define SMVP_TJDS_SPMM_U 8
#endif
constexpr int kTjdsSpmmU = SMVP_TJDS_SPMM_U;  // entries per batch

// X and Y point at vector v0 of the pass; nv = vectors of the pass (<= G)
template <int G>
__global__ __launch_bounds__(kTjdsSpmmBlock) void tjds_spmm_rows(const int *__restrict__ ptr, const int *__restrict__ pos,
                                                                 const int *__restrict__ col, const double *__restrict__ val,
                                                                 const int *__restrict__ order, const double *__restrict__ X,
                                                                 long long ldx, double *__restrict__ Y, long long ldy, int rows,
                                                                 int nv, int group)
{
    constexpr int kRowsPerBlock = kTjdsSpmmBlock / G;
    const long long slot = (long long)tile_of_block((int)blockIdx.x, group) * kRowsPerBlock + threadIdx.x / G;
    if (slot >= rows)
        return;  // (the whole group leaves: the shuffles below stay inside a group)
    const int v = threadIdx.x & (G - 1);
    const int r = order ? order[slot] : (int)slot;
    const int a = ptr[r], z = ptr[r + 1];
    const double *__restrict__ xv = X + (v < nv ? v : nv - 1);  // (a lane past the pass's vectors gathers its neighbour's, stores nothing)
    // stage 1: entry u of the batch is loaded by lane u % G of the group into its slot u / G and handed to the others by a
    // shuffle inside the group; stage 2: every lane reads val[pos] (G lanes at one address) and its own column of X
    constexpr int L = (kTjdsSpmmU + G - 1) / G;
    double acc = 0.0;
    for (int j = a; j < z; j += kTjdsSpmmU) {
        int p[kTjdsSpmmU], c[kTjdsSpmmU], pl[L], cl[L];
        double w[kTjdsSpmmU], g[kTjdsSpmmU];
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const int u = (v % kTjdsSpmmU) + i * G;
            const int jj = j + u < z ? j + u : z - 1;  // (a slot past the row's end re-reads its last entry)
            pl[i] = pos[jj];
            cl[i] = col[jj];
        }
#pragma unroll
        for (int u = 0; u < kTjdsSpmmU; ++u) {
            if constexpr (G == 1) {
                p[u] = pl[u];
                c[u] = cl[u];
            } else {
                p[u] = __shfl(pl[u / G], u % G, G);
                c[u] = __shfl(cl[u / G], u % G, G);
            }
        }
#pragma unroll
        for (int u = 0; u < kTjdsSpmmU; ++u) {
            w[u] = val[p[u]];
            g[u] = xv[(long long)c[u] * ldx];
        }
#pragma unroll
        for (int u = 0; u < kTjdsSpmmU; ++u)
            acc = j + u < z ? acc + w[u] * g[u] : acc;  // (a select, never 0 * X)
    }
    if (v < nv)
        Y[(long long)r * ldy + v] = acc;
}

// col[e] = perm[col[e]]: the permuted column of a stream entry (build_row_gather_plan's kcol) -> the original column
__global__ __launch_bounds__(256) void tjds_spmm_original_columns(const int *__restrict__ perm, int nnz, int *__restrict__ col)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < nnz)
        col[e] = perm[col[e]];
}

// *longest = the most entries a row holds (the sort key's width in build_spmm_order); *longest is 0 on entry
__global__ __launch_bounds__(256) void tjds_spmm_longest_row(const int *__restrict__ ptr, int rows, int *__restrict__ longest)
{
    const long long stride = (long long)gridDim.x * 256;
    int m = 0;
    for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < rows; r += stride)
        m = max(m, ptr[r + 1] - ptr[r]);
    if (m > 0)
        atomicMax(longest, m);
}

int lanes_for(int nv)
{
    int g = 1;
    while (g < nv)
        g <<= 1;
    return g;
}

template <int G>
hipError_t launch_pass(const int *ptr, const int *pos, const int *col, const double *val, const int *order, const double *X,
                       long long ldx, double *Y, long long ldy, int rows, int nv, hipStream_t st)
{
    constexpr int kRowsPerBlock = kTjdsSpmmBlock / G;
    const long long nwg = ((long long)rows + kRowsPerBlock - 1) / kRowsPerBlock;
    // one XCD turn = one sorted block of rows; fewer for a small matrix, so that the grid is not mostly empty workgroups.  The
    // grid is a whole number of rounds of 8 * group workgroups: tile_of_block permutes each round, and a slot >= rows leaves
    const long long group = std::max<long long>(1, std::min<long long>(kSpmmBlockRows / kRowsPerBlock, (nwg + 7) / 8));
    const long long grid = (nwg + 8 * group - 1) / (8 * group) * 8 * group;  // (<= 2^27 + 2048 for G = 16)
    hipLaunchKernelGGL(tjds_spmm_rows<G>, dim3((unsigned)grid), dim3(kTjdsSpmmBlock), 0, st, ptr, pos, col, val, order, X, ldx, Y, ldy,
                       rows, nv, (int)group);
    return hipGetLastError();
}

}  // namespace

int build_tjds_spmm_plan(const int *row_ind, const int *start_pos, const int *perm, int num_diag, int nnz, int rows, int *ptr,
                         int *pos, int *col, int *order, hipStream_t st)
{
    // ptr, pos and the permuted column of every entry: the row-gather plan's builder (a stable sort on row_ind)
    if (int rc = build_row_gather_plan(row_ind, start_pos, num_diag, nnz, rows, ptr, pos, col, st))
        return rc;
    if (rows <= 0)
        return SMVP_OK;
    int *d_longest = nullptr, longest = 0;
    if (hipMalloc((void **)&d_longest, sizeof(int)) != hipSuccess)
        return smvp::fail(SMVP_ERR_ALLOC, "smvp_tjds_spmm: cannot allocate the plan's scratch");
    hipError_t e = hipMemsetAsync(d_longest, 0, sizeof(int), st);
    if (e == hipSuccess && nnz > 0) {
        hipLaunchKernelGGL(tjds_spmm_original_columns, dim3((unsigned)(((long long)nnz + 255) / 256)), dim3(256), 0, st, perm, nnz, col);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        const long long blocks = std::min<long long>(((long long)rows + 255) / 256, 2048);
        hipLaunchKernelGGL(tjds_spmm_longest_row, dim3((unsigned)blocks), dim3(256), 0, st, ptr, rows, d_longest);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(&longest, d_longest, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    (void)hipFree(d_longest);
    if (e != hipSuccess)
        return smvp::fail(SMVP_ERR_HIP, "smvp_tjds_spmm: building the plan failed: %s", hipGetErrorString(e));
    return build_spmm_order(ptr, rows, longest, order, st);
}

hipError_t launch_tjds_spmm(const int *ptr, const int *pos, const int *col, const double *val, const int *order, const double *X,
                            long long ldx, double *Y, long long ldy, int rows, int k, hipStream_t st)
{
    if (rows <= 0)
        return hipSuccess;
    for (long long v0 = 0; v0 < k; v0 += kSpmmMaxVectors) {  // (64-bit: k may be close to INT_MAX)
        const int nv = (int)std::min<long long>(k - v0, kSpmmMaxVectors);
        const double *Xp = X ? X + v0 : nullptr;  // (X may be null when there are no entries: every row is empty, nothing is gathered)
        hipError_t e;
        switch (lanes_for(nv)) {
        case 1: e = launch_pass<1>(ptr, pos, col, val, nullptr, Xp, ldx, Y + v0, ldy, rows, nv, st); break;
        case 2: e = launch_pass<2>(ptr, pos, col, val, order, Xp, ldx, Y + v0, ldy, rows, nv, st); break;
        case 4: e = launch_pass<4>(ptr, pos, col, val, order, Xp, ldx, Y + v0, ldy, rows, nv, st); break;
        case 8: e = launch_pass<8>(ptr, pos, col, val, order, Xp, ldx, Y + v0, ldy, rows, nv, st); break;
        default: e = launch_pass<16>(ptr, pos, col, val, order, Xp, ldx, Y + v0, ldy, rows, nv, st); break;
        }
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

void tjds_spmm_kernel_name(int k, char *name, size_t cap)
{
    if (!name || cap == 0)
        return;
    std::string s;  // (stops once it no longer fits `cap`: a k of millions does not build millions of names)
    for (long long v0 = 0; v0 < k && s.size() < cap; v0 += kSpmmMaxVectors) {
        if (!s.empty())
            s += " + ";
        s += "tjds_spmm_rows<" + std::to_string(lanes_for((int)std::min<long long>(k - v0, kSpmmMaxVectors))) + ">";
    }
    snprintf(name, cap, "%s", s.c_str());
}

}  // namespace smvp
