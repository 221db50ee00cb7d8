// smvp_tjds_spmm_transposed.hip -- K9: Y = A^T X for a block of k vectors from the TJDS arrays themselves
// (smvp_tjds_spmm_transposed; new: the reference multiplies by A only and by one x, main-cli.c:1013-1020).
//
//   Y(perm[c], v) = sum over the diagonals d that reach permuted column c of  val[start_pos[d] + c] * X(row_ind[start_pos[d] + c], v)
//
// K8's walk (smvp_tjds_transposed.hip) crossed with K7's lane groups (smvp_spmm.hip): X is rows x k and Y cols x k, row-major
// with leading dimensions ldx / ldy, so one gathered row of X is k consecutive doubles -- the line K8 fetches for 8 useful
// bytes carries 8 k of them here -- and val / row_ind are read once for up to kSpmmMaxVectors vectors.
//
//   * a group of G adjacent lanes (G = 1, 2, 4, 8, 16: the smallest power of two >= the vectors of the pass) takes one permuted
//     column, lane v of the group holds vector v0 + v: a wavefront covers 64 / G consecutive permuted columns.  Its first
//     column is its longest and widths never grow with d (smvp_tjds_create checks it), so K8's wave-uniform early exit holds;
//   * per batch of kTjdsSpmmTBatch jagged diagonals the row_ind / val loads are issued together, then the gathers
//     X[(long long)row * ldx + v] -- the group reads G consecutive doubles -- then the products are added IN DIAGONAL ORDER.
//     A lane whose column has ended reads entry 0 and leaves its product out of the sum with a select (never 0 * X: X may hold
//     NaN or Inf in rows the column does not touch); a lane with v >= nv gathers its neighbour's vector and stores nothing;
//   * every lane of a group needs the same (row_ind, val) pair.  SMVP_TJDS_SPMM_T_SHFL = 1: diagonal i of the batch is loaded
//     by lane i % G of the group and handed round with __shfl (K7's form); 0: every lane loads the pair itself, G lanes at one
//     address.  The choice and both figures are in DESIGN section 4, K9;
//   * the store is Y[(long long)perm[c] * ldy + v].  Every offset into X and Y is 64-bit (row * ldx and perm * ldy pass 2^31
//     for ordinary sizes); positions into val / row_ind stay 32-bit (start_pos[d] + c < nnz <= 2^31 - 1 - 65536 for an active
//     lane) and columns are counted unsigned, as in K8;
//   * no atomics, no LDS, no barriers, no plan.  A column is never split between groups and a (column, vector) sum never
//     between lanes: every Y(c, v) is the serial sum over the column in TJDS position order, each product rounded before it
//     is added (-ffp-contract=off), the same bits on every run -- for G = 1 and ldx = ldy = 1 the bits of K8, whose launch
//     that case is handed to (launch_tjds_spmm_transposed below).
// Batch depth 8 is a measured choice (profiles/spmm_transposed_k_sweep.txt; memplus x944 / config 4, ms at k = 8 and 16):
// depth 4 1.712, 2.942 / 6.711, 8.090; depth 8 1.767, 3.193 / 6.511, 7.630; depth 16 2.290, 3.892 / 6.723, 7.686 -- a depth that
// shrinks as G grows pays on the first matrix and costs on the second, so one depth stays.
#include "smvp_common.h"
#include "smvp_kernels.h"

#include <algorithm>
#include <cstdio>
#include <string>

namespace smvp {

namespace {

#ifndef SMVP_TJDS_SPMM_T_BATCH
#define SMVP_TJDS_SPMM_T_BATCH 8
#endif
constexpr int kTjdsSpmmTBatch = SMVP_TJDS_SPMM_T_BATCH;  // jagged diagonals whose loads a lane keeps in flight together
#ifndef SMVP_TJDS_SPMM_T_SHFL
#define SMVP_TJDS_SPMM_T_SHFL 1  // 1: one (row_ind, val) load per group and diagonal, handed round by __shfl; 0: one per lane
#endif

// X and Y point at vector v0 of the pass; nv = vectors of the pass (<= G)
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
    const int out = c < cols ? perm[c] : 0;  // (loaded ahead of the walk, as in K8)
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

int lanes_for(int nv)
{
    int g = 1;
    while (g < nv)
        g <<= 1;
    return g;
}

template <int G>
hipError_t launch_pass(const int *start_pos, const int *row_ind, const double *val, const int *perm, const double *X, long long ldx,
                       double *Y, long long ldy, int cols, int num_diag, int nv, hipStream_t st)
{
    constexpr int kColsPerBlock = kTjdsBlock / G;
    const unsigned grid = (unsigned)(((long long)cols + kColsPerBlock - 1) / kColsPerBlock);  // (<= 2^27 for G = 16)
    hipLaunchKernelGGL(tjds_spmm_transposed_columns<G>, dim3(grid), dim3(kTjdsBlock), 0, st, start_pos, row_ind, val, perm, X, ldx,
                       Y, ldy, (unsigned)cols, num_diag, nv);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_tjds_spmm_transposed(const int *start_pos, const int *row_ind, const double *val, const int *perm, const double *X,
                                       long long ldx, double *Y, long long ldy, int cols, int num_diag, int k, hipStream_t st)
{
    if (cols <= 0)
        return hipSuccess;
    // one contiguous vector is K8's product: its kernel gathers x[row] without the multiplication by ldx and is 2.2 % faster on
    // memplus x944 (0.587 against 0.601 ms, window spread 0.5 %; equal on pwt x459 and config 4).  Same walk, same bits.
    if (k == 1 && ldx == 1 && ldy == 1)
        return launch_tjds_transposed(start_pos, row_ind, val, perm, X, Y, cols, num_diag, st);
    for (long long v0 = 0; v0 < k; v0 += kSpmmMaxVectors) {  // (64-bit: k may be close to INT_MAX)
        const int nv = (int)std::min<long long>(k - v0, kSpmmMaxVectors);
        const double *Xp = X ? X + v0 : nullptr;  // (X may be null when there are no entries: num_diag = 0, nothing is gathered)
        hipError_t e;
        switch (lanes_for(nv)) {
        case 1: e = launch_pass<1>(start_pos, row_ind, val, perm, Xp, ldx, Y + v0, ldy, cols, num_diag, nv, st); break;
        case 2: e = launch_pass<2>(start_pos, row_ind, val, perm, Xp, ldx, Y + v0, ldy, cols, num_diag, nv, st); break;
        case 4: e = launch_pass<4>(start_pos, row_ind, val, perm, Xp, ldx, Y + v0, ldy, cols, num_diag, nv, st); break;
        case 8: e = launch_pass<8>(start_pos, row_ind, val, perm, Xp, ldx, Y + v0, ldy, cols, num_diag, nv, st); break;
        default: e = launch_pass<16>(start_pos, row_ind, val, perm, Xp, ldx, Y + v0, ldy, cols, num_diag, nv, st); break;
        }
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

void tjds_spmm_transposed_kernel_name(int k, char *name, size_t cap)
{
    if (!name || cap == 0)
        return;
    std::string s;  // (stops once it no longer fits `cap`: a k of millions does not build millions of names)
    for (long long v0 = 0; v0 < k && s.size() < cap; v0 += kSpmmMaxVectors) {
        if (!s.empty())
            s += " + ";
        s += "tjds_spmm_transposed_columns<" + std::to_string(lanes_for((int)std::min<long long>(k - v0, kSpmmMaxVectors))) + ">";
    }
    snprintf(name, cap, "%s", s.c_str());
}

}  // namespace smvp
