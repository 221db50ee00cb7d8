// smvp_spmm.hip -- K7: k products that share one read of the matrix (smvp_csr_spmm; new: the reference multiplies by one
// x, main-cli.c:410-416).
//
//   Y(r, v) = sum_{j in row r} val[j] * X(col_ind[j], v)     X: cols x k, Y: rows x k, row-major, leading dimensions ldx / ldy
//
// Every Y(r, v) is the serial loop on column v, bit for bit: ONE lane sums a row for one vector, left to right, each product
// rounded before it is added (-ffp-contract=off).  A row's sum is never shared between lanes, so the balance comes from the
// order in which the rows are handed out:
//
//   * a group of G adjacent lanes (G = 1, 2, 4, 8, 16: the smallest power of two >= the vectors of the pass) takes one row,
//     lane v holds vector v0 + v.  The group loads the row's next kSpmmU (col_ind, val) pairs together -- entry u by lane
//     u % G -- and hands them round with __shfl (one load per lane and entry instead, measured: memplus x944 k = 8 2.38 against
//     1.58 ms); every lane then gathers from its own column of X, so the group reads G consecutive doubles (G = 16: one
//     128-byte line).  Vectors go kSpmmMaxVectors at a time: k <= 16 reads the matrix once, a
//     larger k takes ceil(k / 16) passes;
//   * a lane issues the loads and gathers of kSpmmU entries before it adds them in entry order (the tile kernel's pattern:
//     a lane's gathers are in flight together).  The last batch of a row re-reads the row's last entry in its unused slots
//     and leaves their products out of the sum;
//   * the plan: inside blocks of kSpmmBlockRows consecutive rows the rows are ordered by length, longest first (stable: equal
//     lengths keep ascending row order), so that the 64 / G rows of a wavefront are about equally long.  Passes of one vector
//     (G = 1) keep the rows in their own order: a lane then reads its own row's indices, and 64 neighbouring rows share their
//     lines (memplus x944, k = 1: 0.757 ms unsorted against 1.469 sorted; k = 8: 1.761 against 1.580).  Never across blocks:
//     a block's gathers stay inside the block's window of X, which one XCD's L2 holds (kron(I, memplus) at k = 8: 1.1 MB per
//     copy of memplus);
//   * placement: a workgroup holds 256 / G rows; workgroups are dealt to the XCDs by tile_of_block in groups of
//     kSpmmBlockRows / (256 / G), so that one XCD's turn is one sorted block.
// The plan is one int per row (block b is order[b * kSpmmBlockRows ...]), built on the device with smvp_prim.h's stable radix
// sort by the first smvp_csr_spmm of a handle.  It depends on row_ptr only.  No atomics, no LDS, no barriers.
#include "smvp_common.h"
#include "smvp_kernels.h"
#include "smvp_prim.h"

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return smvp::fail(SMVP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace smvp {

namespace {

constexpr int kSpmmBlock = 256;  // threads per workgroup
#ifndef SMVP_SPMM_U
#define SMVP_SPMM_U 8
#endif
constexpr int kSpmmU = SMVP_SPMM_U;  // entries per batch
#ifndef SMVP_SPMM_SORT
#define SMVP_SPMM_SORT 1  // 0: rows in their own order for every G (the A/B build of DESIGN section 4)
#endif

// X and Y point at vector v0 of the pass; nv = vectors of the pass (<= G)
template <int G>
__global__ __launch_bounds__(kSpmmBlock) void csr_spmm_rows(const int *__restrict__ row_ptr, const int *__restrict__ col_ind,
                                                            const double *__restrict__ val, const int *__restrict__ order,
                                                            const double *__restrict__ X, long long ldx, double *__restrict__ Y,
                                                            long long ldy, int rows, int nv, int group)
{
    constexpr int kRowsPerBlock = kSpmmBlock / G;
    const long long slot = (long long)tile_of_block((int)blockIdx.x, group) * kRowsPerBlock + threadIdx.x / G;
    if (slot >= rows)
        return;
    const int v = threadIdx.x & (G - 1);
    const int r = order ? order[slot] : (int)slot;
    const int a = row_ptr[r], z = row_ptr[r + 1];
    const double *__restrict__ xv = X + (v < nv ? v : nv - 1);  // (a lane past the pass's vectors gathers its neighbour's, stores nothing)
    // the group loads a batch together: entry u of the batch is loaded by lane u % G of the group into its slot u / G and
    // handed to the others by a shuffle inside the group (one request per row for the batch instead of one per entry and lane)
    constexpr int L = (kSpmmU + G - 1) / G;
    double acc = 0.0;
    for (int j = a; j < z; j += kSpmmU) {
        int c[kSpmmU], cl[L];
        double w[kSpmmU], wl[L], g[kSpmmU];
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const int u = (v % kSpmmU) + i * G;
            const int jj = j + u < z ? j + u : z - 1;
            cl[i] = col_ind[jj];
            wl[i] = val[jj];
        }
#pragma unroll
        for (int u = 0; u < kSpmmU; ++u) {
            if constexpr (G == 1) {
                c[u] = cl[u];
                w[u] = wl[u];
            } else {
                c[u] = __shfl(cl[u / G], u % G, G);
                w[u] = __shfl(wl[u / G], u % G, G);
            }
        }
#pragma unroll
        for (int u = 0; u < kSpmmU; ++u)
            g[u] = xv[(long long)c[u] * ldx];
#pragma unroll
        for (int u = 0; u < kSpmmU; ++u)
            if (j + u < z)
                acc += w[u] * g[u];
    }
    if (v < nv)
        Y[(long long)r * ldy + v] = acc;
}

// sort key of row r: (block, longest - length) -- ascending = the block's rows longest first
__global__ __launch_bounds__(256) void spmm_order_keys(const int *__restrict__ row_ptr, int rows, unsigned len_bits, int longest,
                                                       unsigned long long *__restrict__ key, unsigned *__restrict__ id)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows)
        return;
    const int len = row_ptr[r + 1] - row_ptr[r];
    key[r] = ((unsigned long long)(r / kSpmmBlockRows) << len_bits) | (len_bits ? (unsigned long long)(unsigned)(longest - len) : 0ull);
    id[r] = (unsigned)r;
}

int lanes_for(int nv)
{
    int g = 1;
    while (g < nv)
        g <<= 1;
    return g;
}

template <int G>
hipError_t launch_pass(const int *row_ptr, const int *col_ind, const double *val, const int *order, const double *X, long long ldx,
                       double *Y, long long ldy, int rows, int nv, hipStream_t st)
{
    constexpr int kRowsPerBlock = kSpmmBlock / G;
    const long long nwg = ((long long)rows + kRowsPerBlock - 1) / kRowsPerBlock;
    // one XCD turn = one sorted block of rows; fewer for a small matrix, so that the grid is not mostly empty workgroups
    const long long group = std::max<long long>(1, std::min<long long>(kSpmmBlockRows / kRowsPerBlock, (nwg + 7) / 8));
    const long long grid = (nwg + 8 * group - 1) / (8 * group) * 8 * group;
    hipLaunchKernelGGL(csr_spmm_rows<G>, dim3((unsigned)grid), dim3(kSpmmBlock), 0, st, row_ptr, col_ind, val, order, X, ldx, Y, ldy,
                       rows, nv, (int)group);
    return hipGetLastError();
}

}  // namespace

int build_spmm_order(const int *row_ptr, int rows, int longest_row, int *order, hipStream_t st)
{
    if (rows <= 0)
        return SMVP_OK;
    unsigned len_bits = 0;  // longest - length lies in [0, longest]
    while (SMVP_SPMM_SORT && len_bits < 31 && (1ull << len_bits) <= (unsigned long long)longest_row)
        ++len_bits;
    const long long nblocks = ((long long)rows + kSpmmBlockRows - 1) / kSpmmBlockRows;
    unsigned blk_bits = 0;
    while ((1ll << blk_bits) < nblocks)
        ++blk_bits;
    struct Scratch {
        std::vector<void *> p;
        ~Scratch()
        {
            for (void *q : p)
                (void)hipFree(q);
        }
        hipError_t get(void **out, size_t bytes)
        {
            *out = nullptr;
            const hipError_t e = hipMalloc(out, std::max<size_t>(bytes, 256));
            if (e == hipSuccess)
                p.push_back(*out);
            return e;
        }
    } sc;
    void *k0, *k1, *ids, *tmp;
    HIP_TRY(sc.get(&k0, sizeof(unsigned long long) * (size_t)rows));
    HIP_TRY(sc.get(&k1, sizeof(unsigned long long) * (size_t)rows));
    HIP_TRY(sc.get(&ids, sizeof(unsigned) * (size_t)rows));
    hipLaunchKernelGGL(spmm_order_keys, dim3((unsigned)(((long long)rows + 255) / 256)), dim3(256), 0, st, row_ptr, rows, len_bits,
                       longest_row, (unsigned long long *)k0, (unsigned *)ids);
    HIP_TRY(hipGetLastError());
    size_t bytes = 0;
    HIP_TRY(prim::radix_sort_pairs(nullptr, bytes, (const unsigned long long *)k0, (unsigned long long *)k1, (const unsigned *)ids,
                                   (unsigned *)order, (size_t)rows, 0u, len_bits + blk_bits, st));
    HIP_TRY(sc.get(&tmp, bytes));
    HIP_TRY(prim::radix_sort_pairs(tmp, bytes, (const unsigned long long *)k0, (unsigned long long *)k1, (const unsigned *)ids,
                                   (unsigned *)order, (size_t)rows, 0u, len_bits + blk_bits, st));
    HIP_TRY(hipStreamSynchronize(st));  // (before the scratch goes)
    return SMVP_OK;
}

hipError_t launch_csr_spmm(const int *row_ptr, const int *col_ind, const double *val, const int *order, const double *X,
                           long long ldx, double *Y, long long ldy, int rows, int k, hipStream_t st)
{
    if (rows <= 0)
        return hipSuccess;
    for (long long v0 = 0; v0 < k; v0 += kSpmmMaxVectors) {  // (64-bit: k may be close to INT_MAX)
        const int nv = (int)std::min<long long>(k - v0, kSpmmMaxVectors);
        const double *Xp = X ? X + v0 : nullptr;  // (X may be null when there are no entries)
        hipError_t e;
        switch (lanes_for(nv)) {
        case 1: e = launch_pass<1>(row_ptr, col_ind, val, nullptr, Xp, ldx, Y + v0, ldy, rows, nv, st); break;
        case 2: e = launch_pass<2>(row_ptr, col_ind, val, order, Xp, ldx, Y + v0, ldy, rows, nv, st); break;
        case 4: e = launch_pass<4>(row_ptr, col_ind, val, order, Xp, ldx, Y + v0, ldy, rows, nv, st); break;
        case 8: e = launch_pass<8>(row_ptr, col_ind, val, order, Xp, ldx, Y + v0, ldy, rows, nv, st); break;
        default: e = launch_pass<16>(row_ptr, col_ind, val, order, Xp, ldx, Y + v0, ldy, rows, nv, st); break;
        }
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

void spmm_kernel_name(int k, char *name, size_t cap)
{
    if (!name || cap == 0)
        return;
    std::string s;  // (stops once it no longer fits `cap`: a k of millions does not build millions of names)
    for (long long v0 = 0; v0 < k && s.size() < cap; v0 += kSpmmMaxVectors) {
        if (!s.empty())
            s += " + ";
        s += "csr_spmm_rows<" + std::to_string(lanes_for((int)std::min<long long>(k - v0, kSpmmMaxVectors))) + ">";
    }
    snprintf(name, cap, "%s", s.c_str());
}

}  // namespace smvp
