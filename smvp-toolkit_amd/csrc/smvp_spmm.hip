// smvp_spmm.hip -- the block products: k vectors share one read of the matrix (new: the reference multiplies by one x and by A
// only, main-cli.c:410-416, 1013-1020).  X and Y are row-major with leading dimensions ldx / ldy.
//
//   K7  csr_spmm_rows<G>                 smvp_csr_spmm              Y(r, v) = sum_{j in row r} val[j] * X(col_ind[j], v)
//   K10 tjds_spmm_rows<G>                smvp_tjds_spmm             Y(r, v) = sum over the TJDS positions j with row_ind[j] == r,
//                                                                   ascending, of val[j] * X(perm[j - start_pos[d(j)]], v)
//   K8  tjds_transposed_columns          smvp_tjds_spmv_transposed  y[perm[c]] = sum over the diagonals d that reach permuted column c
//                                                                   of val[start_pos[d] + c] * x[row_ind[start_pos[d] + c]]
//   K9  tjds_spmm_transposed_columns<G>  smvp_tjds_spmm_transposed  Y(perm[c], v) = the same sum with X(row_ind[...], v)
//
// The lane-group scheme, common to all four.  A group of G adjacent lanes (G = 1, 2, 4, 8, 16: the smallest power of two >= the
// vectors of the pass) takes one row (K7, K10) or one permuted column (K8 with G = 1, K9); lane v of the group holds vector
// v0 + v, so a wavefront covers 64 / G rows or columns.  Vectors go kSpmmMaxVectors at a time: k <= 16 reads the matrix once, a
// larger k takes ceil(k / 16) passes.
//   * the sum: ONE lane sums a row or column for one vector in entry order, each product rounded before it is added
//     (-ffp-contract=off).  A row or column is never split between groups and a sum never between lanes: every Y(r, v) is the
//     serial loop on column v of X, bit for bit, the same bits on every run.  No atomics, no LDS, no barriers;
//   * the batch: a lane issues the index and value loads of a batch of entries, then the batch's gathers -- every lane from
//     its own column of X, so the group reads G consecutive doubles (G = 16: one 128-byte line) -- and only then adds the
//     products IN ENTRY ORDER (the tile kernel's pattern: a lane's gathers are in flight together).  Every lane of a group
//     needs the same index / value pair: the group loads the batch together -- entry u by lane u % G into its slot u / G --
//     and hands the pairs round with __shfl of width G: one request per row and batch instead of one per entry and lane
//     (measured on K7: memplus x944 k = 8 2.38 against 1.58 ms);
//   * the tail: a slot past the end re-reads an entry that exists (a row's last; entry 0 for a column that has ended) and is
//     left out of the sum by a select, never 0 * X: X may hold NaN or Inf in rows the row or column does not touch.  No branch
//     stands between the loads of a batch;
//   * a lane with v >= nv gathers its neighbour's vector and stores nothing;
//   * a whole group leaves before the shuffles, never part of one: the shuffles stay inside a group;
//   * every offset into X and Y is 64-bit (index * ldx and row * ldy pass 2^31 for ordinary sizes); positions into the
//     matrix's arrays stay 32-bit (nnz <= 2^31 - 1 - 65536).
//
// The row walk (K7, K10), batches of kSpmmU entries.  The balance comes from the order in which the rows are handed out:
//   * the plan (build_spmm_order): inside blocks of kSpmmBlockRows consecutive rows the rows are ordered by length, longest
//     first (stable: equal lengths keep ascending row order), so that the 64 / G rows of a wavefront are about equally long.
//     Passes of one vector (G = 1) keep the rows in their own order: a lane then reads its own row's indices, and 64
//     neighbouring rows share their lines (memplus x944, k = 1: 0.757 ms unsorted against 1.469 sorted; k = 8: 1.761 against
//     1.580).  Never across blocks: a block's gathers stay inside the block's window of X, which one XCD's L2 holds
//     (kron(I, memplus) at k = 8: 1.1 MB per copy of memplus).  One int per row (block b is order[b * kSpmmBlockRows ...]),
//     built on the device with smvp_prim.h's stable radix sort by the first product of a handle; it depends on row_ptr only;
//   * placement: a workgroup holds 256 / G rows; workgroups are dealt to the XCDs by tile_of_block in groups of
//     kSpmmBlockRows / (256 / G), so that one XCD's turn is one sorted block;
//   * K7 reads (col_ind, val) in the first stage;
//   * K10 walks the entries of a TJDS handle regrouped by row, with one more indirection: its plan (build_tjds_spmm_plan,
//     buffers of its own) is ptr[rows + 1]; pos[nnz], the TJDS positions grouped by row and ascending inside a row (a stable
//     radix sort on row_ind); col[nnz] = perm[pos - start_pos[d]], the original column; order[rows] as for K7.  The first
//     stage hands round (pos, col); val[pos] (G lanes at one address) and the gathers are issued together, both depend on
//     the first stage only.  No copy of val, so val of adopted arrays changed in place is seen.
//
// The column walk (K8, K9), batches of kTjdsSpmmTBatch jagged diagonals.  TJDS stores A by columns, so what is a scatter for
// A x is a gather for A^T x: permuted column c is a row of A^T, and at every step a wavefront reads one contiguous run of
// val / row_ind (the traversal of tjds_colmajor_products).  No plan: the kernels read the handle's own arrays.
//   * start_pos[d] and the diagonal's width start_pos[d + 1] - start_pos[d] are wave-uniform (scalar loads).  A column is
//     active at diagonal d while c < width(d); widths never grow with d (smvp_tjds_create checks it) and a wavefront's first
//     column is its longest, so the wavefront leaves the loop at the first batch whose first width does not reach its first
//     column: a wave runs as long as its longest column, and neighbouring columns have (nearly) equal lengths because the
//     format sorts them.  Workgroups run in index order, so the longest columns start first;
//   * columns are counted unsigned, so that the last workgroup of a matrix of 2^31 - 1 columns does not wrap; start_pos[d] + c
//     < nnz for an active lane;
//   * K8 is the walk with G = 1 and unit strides: x[row] and y[perm[c]] without the multiplications by ldx and ldy.  Batch depth
//     8 is a measured choice (profiles/transposed_measured.txt; memplus x944 / memplus alone, where one column of 574 entries
//     binds): 8 0.620 / 0.052 ms, 16 0.706 / 0.048; a two-batch pipeline (the next batch's loads issued ahead of the current
//     batch's gathers) 0.621 / 0.048 at depth 8 with twice the registers, 0.604 / 0.060 at depth 4: nothing that pays on
//     both, so the plain loop stays;
//   * K9: one gathered row of X is k consecutive doubles -- the line K8 fetches for 8 useful bytes carries 8 k of them here.
//     SMVP_TJDS_SPMM_T_SHFL = 1: diagonal i of the batch is loaded by lane i % G of the group and handed round with __shfl;
//     0: every lane loads the pair itself, G lanes at one address.  The choice and both figures are in DESIGN section 4, K9.
//     Batch depth 8 is a measured choice (profiles/spmm_transposed_k_sweep.txt; memplus x944 / config 4, ms at k = 8 and 16):
//     depth 4 1.712, 2.942 / 6.711, 8.090; depth 8 1.767, 3.193 / 6.511, 7.630; depth 16 2.290, 3.892 / 6.723, 7.686 -- a depth
//     that shrinks as G grows pays on the first matrix and costs on the second, so one depth stays.  For k = 1 and
//     ldx = ldy = 1 the bits are K8's, whose launch that case is handed to (launch_tjds_spmm_transposed below).
#include "smvp_common.h"
#include "smvp_kernels.h"
#include "smvp_prim.h"

#include <algorithm>
#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return smvp::fail(SMVP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace smvp {

namespace {

constexpr int kSpmmBlock = 256;  // threads per workgroup, the row walk (the column walk: kTjdsBlock)
#ifndef SMVP_SPMM_U
#define SMVP_SPMM_U 8
#endif
constexpr int kSpmmU = SMVP_SPMM_U;  // entries per batch, the row walk
#ifndef SMVP_SPMM_SORT
#define SMVP_SPMM_SORT 1  // 0: rows in their own order for every G (the A/B build of DESIGN section 4)
#endif
#ifndef SMVP_TJDS_SPMM_T_BATCH
#define SMVP_TJDS_SPMM_T_BATCH 8
#endif
constexpr int kTjdsSpmmTBatch = SMVP_TJDS_SPMM_T_BATCH;  // jagged diagonals whose loads a lane keeps in flight together (K8 and K9)
#ifndef SMVP_TJDS_SPMM_T_SHFL
#define SMVP_TJDS_SPMM_T_SHFL 1  // 1: one (row_ind, val) load per group and diagonal, handed round by __shfl; 0: one per lane
#endif

// ---- the kernels ----

// Each of the four keeps a body of its own.  K10's differs from K7's in the first stage only, and K8's is K9's G = 1 branch with
// unit strides, but a body shared through a __forceinline__ function does not compile to the same kernels: the callee is
// optimised before it is inlined and the kernel once more afterwards, and 13 of the 16 instantiations change their registers
// (tjds_spmm_rows<1> 68 -> 73 VGPRs, 7 -> 6 waves per SIMD; the parent's own bodies wrapped unchanged give the same figures as
// the shared ones: profiles/spmm_refactor_measured.txt).  A fix to the walk is made in both kernels of a pair.

// K7.  X and Y point at vector v0 of the pass; nv = vectors of the pass (<= G)
template <int G>
__global__ __launch_bounds__(kSpmmBlock) void csr_spmm_rows(const int *__restrict__ row_ptr, const int *__restrict__ col_ind,
                                                            const double *__restrict__ val, const int *__restrict__ order,
                                                            const double *__restrict__ X, long long ldx, double *__restrict__ Y,
                                                            long long ldy, int rows, int nv, int group)
{
    constexpr int kRowsPerBlock = kSpmmBlock / G;
    const long long slot = (long long)tile_of_block((int)blockIdx.x, group) * kRowsPerBlock + threadIdx.x / G;
    if (slot >= rows)
        return;  // (the whole group leaves: the shuffles below stay inside a group)
    const int v = threadIdx.x & (G - 1);
    const int r = order ? order[slot] : (int)slot;
    const int a = row_ptr[r], z = row_ptr[r + 1];
    const double *__restrict__ xv = X + (v < nv ? v : nv - 1);  // (a lane past the pass's vectors gathers its neighbour's, stores nothing)
    // entry u of the batch is loaded by lane u % G of the group into its slot u / G and handed to the others by a shuffle
    // inside the group
    constexpr int L = (kSpmmU + G - 1) / G;
    double acc = 0.0;
    for (int j = a; j < z; j += kSpmmU) {
        int c[kSpmmU], cl[L];
        double w[kSpmmU], wl[L], g[kSpmmU];
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const int u = (v % kSpmmU) + i * G;
            const int jj = j + u < z ? j + u : z - 1;  // (a slot past the row's end re-reads its last entry)
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
            acc = j + u < z ? acc + w[u] * g[u] : acc;  // (a select, never 0 * X)
    }
    if (v < nv)
        Y[(long long)r * ldy + v] = acc;
}

// K10: K7 with (pos, col) in the first stage and val[pos] (G lanes at one address) beside the gathers in the second
template <int G>
__global__ __launch_bounds__(kSpmmBlock) void tjds_spmm_rows(const int *__restrict__ ptr, const int *__restrict__ pos,
                                                             const int *__restrict__ col, const double *__restrict__ val,
                                                             const int *__restrict__ order, const double *__restrict__ X,
                                                             long long ldx, double *__restrict__ Y, long long ldy, int rows, int nv,
                                                             int group)
{
    constexpr int kRowsPerBlock = kSpmmBlock / G;
    const long long slot = (long long)tile_of_block((int)blockIdx.x, group) * kRowsPerBlock + threadIdx.x / G;
    if (slot >= rows)
        return;  // (the whole group leaves: the shuffles below stay inside a group)
    const int v = threadIdx.x & (G - 1);
    const int r = order ? order[slot] : (int)slot;
    const int a = ptr[r], z = ptr[r + 1];
    const double *__restrict__ xv = X + (v < nv ? v : nv - 1);  // (a lane past the pass's vectors gathers its neighbour's, stores nothing)
    constexpr int L = (kSpmmU + G - 1) / G;
    double acc = 0.0;
    for (int j = a; j < z; j += kSpmmU) {
        int p[kSpmmU], c[kSpmmU], pl[L], cl[L];
        double w[kSpmmU], g[kSpmmU];
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const int u = (v % kSpmmU) + i * G;
            const int jj = j + u < z ? j + u : z - 1;  // (a slot past the row's end re-reads its last entry)
            pl[i] = pos[jj];
            cl[i] = col[jj];
        }
#pragma unroll
        for (int u = 0; u < kSpmmU; ++u) {
            if constexpr (G == 1) {
                p[u] = pl[u];
                c[u] = cl[u];
            } else {
                p[u] = __shfl(pl[u / G], u % G, G);
                c[u] = __shfl(cl[u / G], u % G, G);
            }
        }
#pragma unroll
        for (int u = 0; u < kSpmmU; ++u) {
            w[u] = val[p[u]];
            g[u] = xv[(long long)c[u] * ldx];
        }
#pragma unroll
        for (int u = 0; u < kSpmmU; ++u)
            acc = j + u < z ? acc + w[u] * g[u] : acc;  // (a select, never 0 * X)
    }
    if (v < nv)
        Y[(long long)r * ldy + v] = acc;
}

// K9.  X and Y point at vector v0 of the pass; nv = vectors of the pass (<= G)
template <int G>
__global__ __launch_bounds__(kTjdsBlock) void tjds_spmm_transposed_columns(
    const int *__restrict__ start_pos, const int *__restrict__ row_ind, const double *__restrict__ val,
    const int *__restrict__ perm, const double *__restrict__ X, long long ldx, double *__restrict__ Y, long long ldy,
    unsigned cols, int num_diag, int nv)
{
    constexpr unsigned kColsPerBlock = kTjdsBlock / G;
    constexpr unsigned kColsPerWave = 64 / G;
    const unsigned c = blockIdx.x * kColsPerBlock + threadIdx.x / G;  // the group's permuted column
    const int v = threadIdx.x & (G - 1);
    // the wavefront's first column: the longest of its 64 / G, so its length is the wave's trip count
    const unsigned c_wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(c & ~(kColsPerWave - 1)));
    const int out = c < cols ? perm[c] : 0;  // (loaded ahead of the walk: one round trip less at the end of a short column)
    const double *__restrict__ xv = X + (v < nv ? v : nv - 1);  // (a lane past the pass's vectors gathers its neighbour's, stores nothing)
    double acc = 0.0;
    for (int d = 0; d < num_diag; d += kTjdsSpmmTBatch) {
        int base[kTjdsSpmmTBatch + 1];
#pragma unroll
        for (int i = 0; i <= kTjdsSpmmTBatch; ++i)
            base[i] = start_pos[d + i < num_diag ? d + i : num_diag];  // (uniform index: scalar loads)
        if ((unsigned)(base[1] - base[0]) <= c_wave)
            break;  // no column of this wavefront reaches diagonal d, nor any later one
        bool on[kTjdsSpmmTBatch];
        int r[kTjdsSpmmTBatch];
        double w[kTjdsSpmmTBatch], g[kTjdsSpmmTBatch];
#pragma unroll
        for (int i = 0; i < kTjdsSpmmTBatch; ++i)
            on[i] = c < (unsigned)(base[i + 1] - base[i]);  // (a diagonal past the last has width 0; the same in every lane of a group)
        // a group whose column has ended reads entry 0 and leaves its product out: no branch around a load, so the batch's
        // loads are in flight together (the loop runs: nnz > 0, entry 0 exists)
        if constexpr (G == 1 || !SMVP_TJDS_SPMM_T_SHFL) {
#pragma unroll
            for (int i = 0; i < kTjdsSpmmTBatch; ++i) {
                const int j = on[i] ? base[i] + (int)c : 0;
                r[i] = row_ind[j];
                w[i] = val[j];
            }
        } else {
            // diagonal i of the batch is loaded by lane i % G of the group into its slot i / G (base[] lives in scalar
            // registers, so a lane picks its diagonal's start and width by selects, not by an index)
            constexpr int L = (kTjdsSpmmTBatch + G - 1) / G;
            const int vsel = v % (G < kTjdsSpmmTBatch ? G : kTjdsSpmmTBatch);
            int rl[L];
            double wl[L];
#pragma unroll
            for (int s = 0; s < L; ++s) {
                int lo = 0;
                unsigned width = 0;  // (a slot past the batch keeps width 0 and re-reads entry 0)
#pragma unroll
                for (int i = s * G; i < kTjdsSpmmTBatch && i < (s + 1) * G; ++i)
                    if (i - s * G == vsel) {
                        lo = base[i];
                        width = (unsigned)(base[i + 1] - base[i]);
                    }
                const int j = c < width ? lo + (int)c : 0;
                rl[s] = row_ind[j];
                wl[s] = val[j];
            }
#pragma unroll
            for (int i = 0; i < kTjdsSpmmTBatch; ++i) {
                r[i] = __shfl(rl[i / G], i % G, G);
                w[i] = __shfl(wl[i / G], i % G, G);
            }
        }
#pragma unroll
        for (int i = 0; i < kTjdsSpmmTBatch; ++i)
            g[i] = xv[(long long)r[i] * ldx];
#pragma unroll
        for (int i = 0; i < kTjdsSpmmTBatch; ++i)
            acc = on[i] ? acc + w[i] * g[i] : acc;  // (a select, never 0 * X)
    }
    if (c < cols && v < nv)
        Y[(long long)out * ldy + v] = acc;
}

// K8: K9's G = 1 branch with x[row] for xv[row * ldx] and y[perm[k]] for Y[perm[c] * ldy + v]
__global__ __launch_bounds__(kTjdsBlock) void tjds_transposed_columns(
    const int *__restrict__ start_pos, const int *__restrict__ row_ind, const double *__restrict__ val,
    const int *__restrict__ perm, const double *__restrict__ x, double *__restrict__ y, unsigned cols, int num_diag)
{
    const unsigned k = blockIdx.x * (unsigned)kTjdsBlock + threadIdx.x;
    const unsigned k_wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(k & ~63u));
    const int c = k < cols ? perm[k] : 0;
    double acc = 0.0;
    for (int d = 0; d < num_diag; d += kTjdsSpmmTBatch) {
        int base[kTjdsSpmmTBatch + 1];
#pragma unroll
        for (int i = 0; i <= kTjdsSpmmTBatch; ++i)
            base[i] = start_pos[d + i < num_diag ? d + i : num_diag];
        if ((unsigned)(base[1] - base[0]) <= k_wave)
            break;
        bool on[kTjdsSpmmTBatch];
        int r[kTjdsSpmmTBatch];
        double v[kTjdsSpmmTBatch], g[kTjdsSpmmTBatch];
#pragma unroll
        for (int i = 0; i < kTjdsSpmmTBatch; ++i) {
            on[i] = k < (unsigned)(base[i + 1] - base[i]);
            const int j = on[i] ? base[i] + (int)k : 0;
            r[i] = row_ind[j];
            v[i] = val[j];
        }
#pragma unroll
        for (int i = 0; i < kTjdsSpmmTBatch; ++i)
            g[i] = x[r[i]];
#pragma unroll
        for (int i = 0; i < kTjdsSpmmTBatch; ++i)
            acc = on[i] ? acc + v[i] * g[i] : acc;  // (a select, never 0 * x)
    }
    if (k < cols)
        y[c] = acc;
}

// ---- passes ----

int lanes_for(int nv)
{
    int g = 1;
    while (g < nv)
        g <<= 1;
    return g;
}

// launch(G, X, Y, nv) once per pass of at most kSpmmMaxVectors vectors, G = lanes_for(nv) as a compile-time constant
template <typename Launch>
hipError_t for_each_pass(int k, const double *X, double *Y, Launch launch)
{
    for (long long v0 = 0; v0 < k; v0 += kSpmmMaxVectors) {  // (64-bit: k may be close to INT_MAX)
        const int nv = (int)std::min<long long>(k - v0, kSpmmMaxVectors);
        const double *Xp = X ? X + v0 : nullptr;  // (X may be null when there are no entries: nothing is gathered)
        hipError_t e;
        switch (lanes_for(nv)) {
        case 1: e = launch(std::integral_constant<int, 1>(), Xp, Y + v0, nv); break;
        case 2: e = launch(std::integral_constant<int, 2>(), Xp, Y + v0, nv); break;
        case 4: e = launch(std::integral_constant<int, 4>(), Xp, Y + v0, nv); break;
        case 8: e = launch(std::integral_constant<int, 8>(), Xp, Y + v0, nv); break;
        default: e = launch(std::integral_constant<int, 16>(), Xp, Y + v0, nv); break;
        }
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

// "stem<G> + stem<G> + ...", one term per pass
void pass_names(const char *stem, int k, char *name, size_t cap)
{
    if (!name || cap == 0)
        return;
    std::string s;  // (stops once it no longer fits `cap`: a k of millions does not build millions of names)
    for (long long v0 = 0; v0 < k && s.size() < cap; v0 += kSpmmMaxVectors) {
        if (!s.empty())
            s += " + ";
        s += stem + ("<" + std::to_string(lanes_for((int)std::min<long long>(k - v0, kSpmmMaxVectors))) + ">");
    }
    snprintf(name, cap, "%s", s.c_str());
}

// one pass of K7 or, by position, K10; a pass of one vector keeps the rows in their own order
template <int G, bool kByPosition>
hipError_t launch_rows(const int *ptr, const int *pos, const int *col, const double *val, const int *order, const double *X,
                       long long ldx, double *Y, long long ldy, int rows, int nv, hipStream_t st)
{
    constexpr int kRowsPerBlock = kSpmmBlock / G;
    const long long nwg = ((long long)rows + kRowsPerBlock - 1) / kRowsPerBlock;
    // one XCD turn = one sorted block of rows; fewer for a small matrix, so that the grid is not mostly empty workgroups.  The
    // grid is a whole number of rounds of 8 * group workgroups: tile_of_block permutes each round, and a slot >= rows leaves
    const long long group = std::max<long long>(1, std::min<long long>(kSpmmBlockRows / kRowsPerBlock, (nwg + 7) / 8));
    const long long grid = (nwg + 8 * group - 1) / (8 * group) * 8 * group;  // (<= 2^27 + 2048 for G = 16)
    if (G == 1)
        order = nullptr;
    if constexpr (kByPosition)
        hipLaunchKernelGGL(tjds_spmm_rows<G>, dim3((unsigned)grid), dim3(kSpmmBlock), 0, st, ptr, pos, col, val, order, X, ldx, Y, ldy,
                           rows, nv, (int)group);
    else
        hipLaunchKernelGGL(csr_spmm_rows<G>, dim3((unsigned)grid), dim3(kSpmmBlock), 0, st, ptr, col, val, order, X, ldx, Y, ldy, rows,
                           nv, (int)group);
    return hipGetLastError();
}

// one pass of K9
template <int G>
hipError_t launch_columns(const int *start_pos, const int *row_ind, const double *val, const int *perm, const double *X,
                          long long ldx, double *Y, long long ldy, int cols, int num_diag, int nv, hipStream_t st)
{
    constexpr int kColsPerBlock = kTjdsBlock / G;
    const unsigned grid = (unsigned)(((long long)cols + kColsPerBlock - 1) / kColsPerBlock);  // (<= 2^27 for G = 16)
    hipLaunchKernelGGL(tjds_spmm_transposed_columns<G>, dim3(grid), dim3(kTjdsBlock), 0, st, start_pos, row_ind, val, perm, X, ldx, Y,
                       ldy, (unsigned)cols, num_diag, nv);
    return hipGetLastError();
}

// ---- plans ----

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

// ---- the products ----

hipError_t launch_csr_spmm(const int *row_ptr, const int *col_ind, const double *val, const int *order, const double *X,
                           long long ldx, double *Y, long long ldy, int rows, int k, hipStream_t st)
{
    if (rows <= 0)
        return hipSuccess;
    return for_each_pass(k, X, Y, [&](auto G, const double *Xp, double *Yp, int nv) {
        return launch_rows<decltype(G)::value, false>(row_ptr, nullptr, col_ind, val, order, Xp, ldx, Yp, ldy, rows, nv, st);
    });
}

hipError_t launch_tjds_spmm(const int *ptr, const int *pos, const int *col, const double *val, const int *order, const double *X,
                            long long ldx, double *Y, long long ldy, int rows, int k, hipStream_t st)
{
    if (rows <= 0)
        return hipSuccess;
    return for_each_pass(k, X, Y, [&](auto G, const double *Xp, double *Yp, int nv) {
        return launch_rows<decltype(G)::value, true>(ptr, pos, col, val, order, Xp, ldx, Yp, ldy, rows, nv, st);
    });
}

hipError_t launch_tjds_transposed(const int *start_pos, const int *row_ind, const double *val, const int *perm, const double *x,
                                  double *y, int cols, int num_diag, hipStream_t st)
{
    if (cols <= 0)
        return hipSuccess;
    const unsigned grid = (unsigned)(((long long)cols + kTjdsBlock - 1) / kTjdsBlock);
    hipLaunchKernelGGL(tjds_transposed_columns, dim3(grid), dim3(kTjdsBlock), 0, st, start_pos, row_ind, val, perm, x, y,
                       (unsigned)cols, num_diag);
    return hipGetLastError();
}

hipError_t launch_tjds_spmm_transposed(const int *start_pos, const int *row_ind, const double *val, const int *perm, const double *X,
                                       long long ldx, double *Y, long long ldy, int cols, int num_diag, int k, hipStream_t st)
{
    if (cols <= 0)
        return hipSuccess;
    // one contiguous vector is K8's product: its kernel gathers x[row] without the multiplication by ldx and is 2.2 % faster on
    // memplus x944 (0.587 against 0.601 ms, window spread 0.5 %; equal on pwt x459 and config 4).  Same walk, same bits.
    if (k == 1 && ldx == 1 && ldy == 1)
        return launch_tjds_transposed(start_pos, row_ind, val, perm, X, Y, cols, num_diag, st);
    return for_each_pass(k, X, Y, [&](auto G, const double *Xp, double *Yp, int nv) {
        return launch_columns<decltype(G)::value>(start_pos, row_ind, val, perm, Xp, ldx, Yp, ldy, cols, num_diag, nv, st);
    });
}

void spmm_kernel_name(int k, char *name, size_t cap) { pass_names("csr_spmm_rows", k, name, cap); }
void tjds_spmm_kernel_name(int k, char *name, size_t cap) { pass_names("tjds_spmm_rows", k, name, cap); }
void tjds_spmm_transposed_kernel_name(int k, char *name, size_t cap) { pass_names("tjds_spmm_transposed_columns", k, name, cap); }
const char *tjds_transposed_kernel_name() { return "tjds_transposed_columns"; }

}  // namespace smvp
