// smvp_tjds_transposed.hip -- K8: y = A^T x from the TJDS arrays themselves (smvp_tjds_spmv_transposed; new: the reference
// multiplies by A only, main-cli.c:1013-1020).
//
//   y[perm[k]] = sum over the diagonals d that reach permuted column k of  val[start_pos[d] + k] * x[row_ind[start_pos[d] + k]]
//
// TJDS stores A by columns, so what is a scatter for A x is a gather for A^T x: permuted column k is a row of A^T.  Lane k of
// a workgroup of kTjdsBlock columns walks down its column, one jagged diagonal per step -- at every step a wavefront reads one
// contiguous run of val / row_ind, the traversal of tjds_colmajor_products -- keeps the sum in a register and stores it once.
// A column is never split between lanes: every y is the serial sum over the column in TJDS position order (ascending row,
// ties in storage order), each product rounded before it is added (-ffp-contract=off), the same bits on every run.
//
//   * start_pos[d] and the diagonal's width start_pos[d + 1] - start_pos[d] are wave-uniform (scalar loads).  Lane k is
//     active at diagonal d while k < width(d); widths never grow with d (smvp_tjds_create checks it), so a wavefront leaves
//     the loop at the first batch whose first width does not reach its first column: a wave runs as long as its longest
//     column, and neighbouring columns have (nearly) equal lengths because the format sorts them;
//   * the chain per entry is row_ind -> x[row]: the row_ind / val loads of a batch of kTjdsTBatch diagonals are issued
//     together, then the batch's gathers, then the products are added IN DIAGONAL ORDER.  A lane whose column has ended
//     reads entry 0 and leaves its product out of the sum (a select): no branch stands between the loads of a batch.
//     Batch depth 8 is a measured choice (profiles/transposed_measured.txt; memplus x944 / memplus alone, where one column
//     of 574 entries binds): 8 0.620 / 0.052 ms, 16 0.706 / 0.048; a two-batch pipeline (the next batch's loads issued
//     ahead of the current batch's gathers) 0.621 / 0.048 at depth 8 with twice the registers, 0.604 / 0.060 at depth 4:
//     nothing that pays on both, so the plain loop stays;
//   * workgroups run in index order, so the longest columns start first;
//   * no atomics, no LDS, no barriers, no plan: the kernel reads the handle's own arrays and the caller's x.
// 32-bit positions: start_pos[d] + k < nnz <= 2^31 - 1 - 65536 for an active lane; columns are counted unsigned, so that the
// last workgroup of a matrix of 2^31 - 1 columns does not wrap.
#include "smvp_common.h"
#include "smvp_kernels.h"

namespace smvp {

namespace {

#ifndef SMVP_TJDS_T_BATCH
#define SMVP_TJDS_T_BATCH 8
#endif
constexpr int kTjdsTBatch = SMVP_TJDS_T_BATCH;  // jagged diagonals whose loads a lane keeps in flight together

__global__ __launch_bounds__(kTjdsBlock) void tjds_transposed_columns(
    const int *__restrict__ start_pos, const int *__restrict__ row_ind, const double *__restrict__ val,
    const int *__restrict__ perm, const double *__restrict__ x, double *__restrict__ y, unsigned cols, int num_diag)
{
    const unsigned k = blockIdx.x * (unsigned)kTjdsBlock + threadIdx.x;
    // the wavefront's first column: the longest of its 64, so its length is the wave's trip count
    const unsigned k_wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(k & ~63u));
    const int c = k < cols ? perm[k] : 0;  // (loaded ahead of the walk: one round trip less at the end of a short column)
    double acc = 0.0;
    for (int d = 0; d < num_diag; d += kTjdsTBatch) {
        int base[kTjdsTBatch + 1];
#pragma unroll
        for (int i = 0; i <= kTjdsTBatch; ++i)
            base[i] = start_pos[d + i < num_diag ? d + i : num_diag];  // (uniform index: scalar loads)
        if ((unsigned)(base[1] - base[0]) <= k_wave)
            break;  // no column of this wavefront reaches diagonal d, nor any later one
        bool on[kTjdsTBatch];
        int r[kTjdsTBatch];
        double v[kTjdsTBatch], g[kTjdsTBatch];
#pragma unroll
        for (int i = 0; i < kTjdsTBatch; ++i) {
            on[i] = k < (unsigned)(base[i + 1] - base[i]);  // (a diagonal past the last has width 0)
            // a lane whose column has ended reads entry 0 and leaves its product out: no branch around a load, so the
            // batch's loads are in flight together (the loop runs: nnz > 0, entry 0 exists)
            const int j = on[i] ? base[i] + (int)k : 0;
            r[i] = row_ind[j];
            v[i] = val[j];
        }
#pragma unroll
        for (int i = 0; i < kTjdsTBatch; ++i)
            g[i] = x[r[i]];
#pragma unroll
        for (int i = 0; i < kTjdsTBatch; ++i)
            acc = on[i] ? acc + v[i] * g[i] : acc;  // (a select, never 0 * x: x may hold NaN or Inf in rows the column does not touch)
    }
    if (k < cols)
        y[c] = acc;
}

}  // namespace

hipError_t launch_tjds_transposed(const int *start_pos, const int *row_ind, const double *val, const int *perm, const double *x,
                                  double *y, int cols, int num_diag, hipStream_t stream)
{
    if (cols <= 0)
        return hipSuccess;
    const unsigned grid = (unsigned)(((long long)cols + kTjdsBlock - 1) / kTjdsBlock);
    hipLaunchKernelGGL(tjds_transposed_columns, dim3(grid), dim3(kTjdsBlock), 0, stream, start_pos, row_ind, val, perm, x, y,
                       (unsigned)cols, num_diag);
    return hipGetLastError();
}

const char *tjds_transposed_kernel_name() { return "tjds_transposed_columns"; }

}  // namespace smvp
