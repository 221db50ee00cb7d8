// smvp_cg_multi.hip -- K20: conjugate gradients for k right-hand sides on a handle (smvp_csr_cg_multi, smvp_tjds_cg_multi), to the
// bits include/smvp_amd.h defines.  k independent runs of K12 (d_m == NULL) or K14 (d_m given) that share every read of the matrix
// and every launch: the product of a step is one block product (K7 / K10, smvp_spmm.hip) on all k directions, and a pass over the
// vectors handles up to kCgmMaxColumns columns at a time.  It is not block CG: the columns share no Krylov space, and column v of
// every output is the one-vector run on column v of the operands.
//
// Layout.  R, P and Q are n x k row-major with ld = k; B, X0 and X are the caller's, with leading dimensions of their own.  A pass
// takes a group of nv <= 16 columns, templated on the group width W = 1, 2, 4, 8, 16 (the smallest power of two >= nv, as the block
// products do).  The grid is the one-vector dot's: G = min(ceil(n / 256), 2048) workgroups of 256 lanes, and workgroup g owns the
// dot's slots 256 g .. 256 g + 255 of every column of the group: the rows s, s + 256 G, ... of slot s.  Inside the workgroup a slot's
// accumulators are NOT the lane of that number's: a trip's tile -- 256 rows of W columns -- is dealt to the lanes element by
// element, lane t taking column t % W of the rows t / W + (256 / W) j, so that a wavefront's load reads W consecutive doubles of
// 64 / W consecutive rows (whole lines when ld = k = W).  A lane so keeps, for ONE column, the accumulators of W slots; each adds
// exactly the header's terms in the header's order, and before the fold they go through LDS into the dot's own arrangement -- column
// v's slot l in lane l -- where cg_fold256 per column gives the workgroup's partial of that column (cgm_fold_columns).  Both this
// mapping and the one it replaced (a lane takes a whole row of the group) are measured in profiles/cg_multi_measured.txt.  Trips in
// flight shrink as W grows (kCgmDotTrips, kCgmPassTrips): loads in flight x columns stay in registers.
//
// Idle lanes.  A lane whose column is >= nv (a group of 3, 5 .. 7 or 9 .. 15 columns) re-reads column nv - 1 and stores nothing, so
// that no branch stands between a tile's loads.  In cgm_residual (R) and cgm_direction (P, X) that element is one the lane of column
// nv - 1 of the same workgroup writes in the same launch, through the same pointer: the one place where a launch reads a word that
// another lane of it writes.  The idle lane may see the old or the new value; it uses neither -- `c < nv` gates its stores and its
// accumulators' way into LDS -- so no result depends on which.  (cgm_start's idle lanes read B, Q, X0 and m only, which it never
// writes.)
//
// A step k, beside the block product q = A p (one launch per 16 columns):
//
//   cgm_dot<W>            the partials of sigma_v = dot(p_v, q_v), per column                      (P, Q read)          per group
//   cgm_sigma_finish      one workgroup per column: folds them, forms sigma_v, rule A and alpha_v = rho_v / sigma_v, and leaves
//                         them in the column's words                                                                    one launch
//   cgm_residual<W, D>    r_v -= alpha_v q_v with the partials of rr_v (D: and of rho_v = dot(r_v, r_v ./ m))
//                                                                                                 (Q, R, m read, R written) per group
//   cgm_rho_finish<D>     one workgroup per column: folds them, forms rule B and beta_v, writes the column's status block of the
//                         step, its history elements and what the last pass is to do with the column                   one launch
//   cgm_direction<W, D>   x_v += alpha_v p_v; p_v = z_v + beta_v p_v unless the column stops here (X, P, R, m read, X, P written)
//                                                                                                                       per group
//
// The two finish launches replace every workgroup folding k x 2048 partials itself; the bits are the same either way.  The launch
// discipline is smvp_cg_common.h's: no atomics, no flags, every hand-off between workgroups is a launch boundary, no kernel waits
// on a value another workgroup writes, a scalar reaches the later launches through a word of its own written with a plain store,
// and the status blocks (2 x k) are ping-ponged by step parity.  Each column has its own status: once its rule has fired, no later
// launch writes that column of X, of R or P, or its histories; the block product still multiplies it (in vain), which cannot disturb
// the others because the block product's columns are independent.  The host reads the k status blocks at looked steps only, and only
// to leave the loop, which ends when all columns have stopped.
#include "smvp_cg_common.h"
#include "smvp_engine.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

namespace smvp {

namespace {

constexpr int kCgmMaxColumns = 16;  // columns of one pass (the block products': kSpmmMaxVectors)

// trips in flight per lane: of the dot's pass, which only reads, and of a pass that also writes -- K12's 8 and 4 for one column
template <int W>
constexpr int kCgmDotTrips = W >= kCgDotTrips ? 1 : kCgDotTrips / W;
template <int W>
constexpr int kCgmPassTrips = W >= 8 ? 1 : W == 4 ? 2 : kCgTrips;

// a column's status: K12's / K14's block (without a preconditioner rho and rr hold the same number)
struct CgmStatus {
    double rho;   // rho_updates = dot(r, z) of the last update
    double rr;    // dot(r, r) of the last update: what the stop rule looks at
    double bb;    // dot(b, b)
    double thr;   // (tol * tol) * bb
    int stopped;  // a rule has fired: reason, steps and updates are final
    int reason;   // SMVP_CG_*
    int steps;    // products done
    int updates;  // updates of x done
};

// what a column's finish workgroups leave for the passes of the step
struct CgmWords {
    double sigma;   // sigma_k                                  (cgm_sigma_finish)
    double alpha;   // rho_{k-1} / sigma_k                      (cgm_sigma_finish)
    double beta;    // rho_k / rho_{k-1}                        (cgm_rho_finish)
    int residual;   // cgm_residual updates the column          (cgm_sigma_finish: not stopped, and rule A does not hold)
    int direction;  // cgm_direction: 0 nothing, 1 x only (the column stops at this step), 2 x and p   (cgm_rho_finish)
};

// ------------------------------------------------------------------------------------------------------------------ the passes
// Every pass gets its vectors at the group's first column.  A workgroup's tile is 256 consecutive rows of the group's W columns; lane
// t of the workgroup takes column t % W of the rows t / W + (256 / W) j, j = 0 .. W - 1, so that the lanes of a wavefront read W
// consecutive doubles of 64 / W consecutive rows at every load.  Lane t so holds, for its one column, the accumulators of the W
// slots 256 g + t / W + (256 / W) j.  A lane whose column is >= nv reads the group's last column and stores nothing; a row >= n
// (the matrix's last tile) re-reads row n - 1 and is left out of the sums by a select.

// the workgroup's partial of every column of the group: the accumulators go through LDS into the dot's own order -- column v's 256
// slots in lanes 0 .. 255 -- and cg_fold256 folds them.  `words`: only the columns whose word says so are written.
template <int W>
__device__ inline void cgm_fold_columns(const double (&acc)[W], int nv, const CgmWords *__restrict__ words, double *__restrict__ parts,
                                        int cap)
{
    __shared__ double s_acc[W][kCgBlock + 1];  // (+ 1: the W columns of a row fall into different banks)
    const int c = threadIdx.x & (W - 1), r0 = threadIdx.x / W;
    __syncthreads();  // (the last call's readers are done with s_acc)
    if (c < nv) {
#pragma unroll
        for (int j = 0; j < W; ++j)
            s_acc[c][r0 + (kCgBlock / W) * j] = acc[j];
    }
    __syncthreads();
    for (int v = 0; v < nv; ++v) {  // (nv is the same in every lane: the barriers of the fold stay uniform)
        const double f = cg_fold256(s_acc[v][threadIdx.x]);
        if (threadIdx.x == 0 && (!words || words[v].residual != 0))
            parts[(size_t)v * cap + blockIdx.x] = f;
    }
}

// step 0: r_0 = b - q (q = A x_0), or b itself without a q; p_0 = z_0 = r_0 (kDiag: r_0 ./ m); x = x_0 or zeros where X is not X0
// itself; the partials of bb, rr_0 and (kDiag) rho_0
template <int W, bool kDiag>
__global__ __launch_bounds__(kCgBlock) void cgm_start(const double *__restrict__ B, long long ldb, const double *__restrict__ Q,
                                                      const double *X0, long long ldx0, double *X, long long ldx, int write_x,
                                                      const double *__restrict__ m, double *__restrict__ R, double *__restrict__ P,
                                                      long long ld, int n, int nv, int cap, double *__restrict__ parts_bb,
                                                      double *__restrict__ parts_rr, double *__restrict__ parts_rz)
{
    constexpr int RW = kCgBlock / W;
    const int c = threadIdx.x & (W - 1), col = c < nv ? c : nv - 1;
    const long long stride = (long long)gridDim.x * kCgBlock, r0 = threadIdx.x / W;
    double abb[W], arr[W], arz[W];
#pragma unroll
    for (int j = 0; j < W; ++j)
        abb[j] = arr[j] = arz[j] = 0.0;
    for (long long b = (long long)blockIdx.x * kCgBlock; b < n; b += stride) {
        double bv[W], qv[W], xv[W], mv[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const long long i = b + r0 + RW * j < n ? b + r0 + RW * j : n - 1;
            bv[j] = B[i * ldb + col];
            qv[j] = Q ? Q[i * ld + col] : 0.0;
            xv[j] = write_x && X0 ? X0[i * ldx0 + col] : 0.0;
            mv[j] = kDiag ? m[i] : 1.0;
        }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const long long i = b + r0 + RW * j;
            const bool in = i < n;
            const double v = Q ? bv[j] - qv[j] : bv[j];
            const double z = kDiag ? v / mv[j] : v;
            if (in && c < nv) {
                R[i * ld + c] = v;
                P[i * ld + c] = z;
                if (write_x)
                    X[i * ldx + c] = xv[j];
            }
            const double tb = bv[j] * bv[j], tr = v * v;
            abb[j] = in ? abb[j] + tb : abb[j];
            arr[j] = in ? arr[j] + tr : arr[j];
            if (kDiag) {
                const double s = v * z;
                arz[j] = in ? arz[j] + s : arz[j];
            }
        }
    }
    cgm_fold_columns<W>(abb, nv, nullptr, parts_bb, cap);
    cgm_fold_columns<W>(arr, nv, nullptr, parts_rr, cap);
    if (kDiag)
        cgm_fold_columns<W>(arz, nv, nullptr, parts_rz, cap);
}

// the partials of dot(p_v, q_v) for every column of the group, stopped or not (a stopped column's are never folded)
template <int W>
__global__ __launch_bounds__(kCgBlock) void cgm_dot(const double *__restrict__ P, const double *__restrict__ Q, long long ld, int n, int nv,
                                                    int cap, double *__restrict__ parts)
{
    constexpr int T = kCgmDotTrips<W>, RW = kCgBlock / W;
    const int c = threadIdx.x & (W - 1), col = c < nv ? c : nv - 1;
    const long long stride = (long long)gridDim.x * kCgBlock, r0 = threadIdx.x / W;
    long long b = (long long)blockIdx.x * kCgBlock;  // the tile's first row
    double acc[W];
#pragma unroll
    for (int j = 0; j < W; ++j)
        acc[j] = 0.0;
    for (; b + (T - 1) * stride + kCgBlock <= n; b += T * stride) {  // T whole tiles
        double t[T][W];
#pragma unroll
        for (int u = 0; u < T; ++u)
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const long long at = (b + u * stride + r0 + RW * j) * ld + col;
                t[u][j] = P[at] * Q[at];
            }
#pragma unroll
        for (int u = 0; u < T; ++u)
#pragma unroll
            for (int j = 0; j < W; ++j)
                acc[j] = acc[j] + t[u][j];
    }
    for (; b < n; b += stride) {
        double t[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const long long i = b + r0 + RW * j < n ? b + r0 + RW * j : n - 1;
            t[j] = P[i * ld + col] * Q[i * ld + col];
        }
#pragma unroll
        for (int j = 0; j < W; ++j)
            acc[j] = b + r0 + RW * j < n ? acc[j] + t[j] : acc[j];
    }
    cgm_fold_columns<W>(acc, nv, nullptr, parts, cap);
}

// r_v -= alpha_v q_v for the columns whose word says so, with the partials of dot(r, r); kDiag: and of dot(r, r ./ m), a second
// accumulator per slot in the dot's own order
template <int W, bool kDiag>
__global__ __launch_bounds__(kCgBlock) void cgm_residual(const double *__restrict__ Q, double *__restrict__ R, long long ld,
                                                         const double *__restrict__ m, int n, int nv, int cap,
                                                         const CgmWords *__restrict__ words, double *__restrict__ parts_rr,
                                                         double *__restrict__ parts_rz)
{
    constexpr int T = kCgmPassTrips<W>, RW = kCgBlock / W;
    bool any = false;
    for (int v = 0; v < nv; ++v)
        any = any || words[v].residual != 0;
    if (!any)
        return;  // (the same in every lane)
    const int c = threadIdx.x & (W - 1), col = c < nv ? c : nv - 1;
    const bool mine = c < nv && words[col].residual != 0;
    const double alpha = words[col].alpha;
    const long long stride = (long long)gridDim.x * kCgBlock, r0 = threadIdx.x / W;
    long long b = (long long)blockIdx.x * kCgBlock;
    double arr[W], arz[W];
#pragma unroll
    for (int j = 0; j < W; ++j)
        arr[j] = arz[j] = 0.0;
    for (; b + (T - 1) * stride + kCgBlock <= n; b += T * stride) {  // T whole tiles
        double aq[T][W], v[T][W], mv[T][W];
#pragma unroll
        for (int u = 0; u < T; ++u)
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const long long i = b + u * stride + r0 + RW * j;
                aq[u][j] = alpha * Q[i * ld + col];  // rounded, then the difference is rounded
                v[u][j] = R[i * ld + col];
                mv[u][j] = kDiag ? m[i] : 1.0;
            }
#pragma unroll
        for (int u = 0; u < T; ++u)
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const double w = v[u][j] - aq[u][j];
                if (mine)
                    R[(b + u * stride + r0 + RW * j) * ld + c] = w;
                const double t = w * w;
                arr[j] = arr[j] + t;
                if (kDiag) {
                    const double z = w / mv[u][j];
                    const double s = w * z;
                    arz[j] = arz[j] + s;
                }
            }
    }
    for (; b < n; b += stride) {
        double aq[W], v[W], mv[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const long long i = b + r0 + RW * j < n ? b + r0 + RW * j : n - 1;
            aq[j] = alpha * Q[i * ld + col];
            v[j] = R[i * ld + col];
            mv[j] = kDiag ? m[i] : 1.0;
        }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const long long i = b + r0 + RW * j;
            const bool in = i < n;
            const double w = v[j] - aq[j];
            if (mine && in)
                R[i * ld + c] = w;
            const double t = w * w;
            arr[j] = in ? arr[j] + t : arr[j];
            if (kDiag) {
                const double z = w / mv[j];
                const double s = w * z;
                arz[j] = in ? arz[j] + s : arz[j];
            }
        }
    }
    cgm_fold_columns<W>(arr, nv, words, parts_rr, cap);
    if (kDiag)
        cgm_fold_columns<W>(arz, nv, words, parts_rz, cap);
}

// x_v += alpha_v p_v for the columns that update at this step; p_v = z_v + beta_v p_v for those that go on (z = r, kDiag: r ./ m)
template <int W, bool kDiag>
__global__ __launch_bounds__(kCgBlock) void cgm_direction(double *__restrict__ X, long long ldx, double *__restrict__ P,
                                                          const double *__restrict__ R, long long ld, const double *__restrict__ m, int n,
                                                          int nv, const CgmWords *__restrict__ words)
{
    constexpr int T = kCgmPassTrips<W>, RW = kCgBlock / W;
    int any = 0;
    for (int v = 0; v < nv; ++v)
        any |= words[v].direction;
    if (!any)
        return;  // (every column of the group has stopped, or stops at this step without an update)
    const int c = threadIdx.x & (W - 1), col = c < nv ? c : nv - 1;
    const int todo = c < nv ? words[col].direction : 0;
    const double alpha = words[col].alpha, beta = words[col].beta;
    const long long stride = (long long)gridDim.x * kCgBlock, r0 = threadIdx.x / W;
    long long b = (long long)blockIdx.x * kCgBlock;
    for (; b + (T - 1) * stride + kCgBlock <= n; b += T * stride) {  // T whole tiles
        double pv[T][W], xv[T][W], zv[T][W], mv[T][W];
#pragma unroll
        for (int u = 0; u < T; ++u)
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const long long i = b + u * stride + r0 + RW * j;
                pv[u][j] = P[i * ld + col];
                xv[u][j] = X[i * ldx + col];
                zv[u][j] = R[i * ld + col];
                mv[u][j] = kDiag ? m[i] : 1.0;
            }
#pragma unroll
        for (int u = 0; u < T; ++u)
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const long long i = b + u * stride + r0 + RW * j;
                const double ap = alpha * pv[u][j], bp = beta * pv[u][j];
                const double z = kDiag ? zv[u][j] / mv[u][j] : zv[u][j];
                if (todo >= 1)
                    X[i * ldx + c] = xv[u][j] + ap;
                if (todo == 2)
                    P[i * ld + c] = z + bp;
            }
    }
    for (; b < n; b += stride) {
        double pv[W], xv[W], zv[W], mv[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const long long i = b + r0 + RW * j < n ? b + r0 + RW * j : n - 1;
            pv[j] = P[i * ld + col];
            xv[j] = X[i * ldx + col];
            zv[j] = R[i * ld + col];
            mv[j] = kDiag ? m[i] : 1.0;
        }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const long long i = b + r0 + RW * j;
            const double ap = alpha * pv[j], bp = beta * pv[j];
            const double z = kDiag ? zv[j] / mv[j] : zv[j];
            if (todo >= 1 && i < n)
                X[i * ldx + c] = xv[j] + ap;
            if (todo == 2 && i < n)
                P[i * ld + c] = z + bp;
        }
    }
}

// ------------------------------------------------------------------------------------------- the scalars: one workgroup per column
// bb, rr_0, rho_0, the threshold and step 0's rule into the column's status block 0, rr_0 and rho_0 into its histories.  OwnRho: rho
// has partials and a history of its own, and "not (rho_0 > 0)" is a breakdown; without, rho_0 is rr_0.
template <bool OwnRho>
__global__ __launch_bounds__(kCgBlock) void cgm_start_finish(const double *__restrict__ parts_bb, const double *__restrict__ parts_rr,
                                                             const double *__restrict__ parts_rz, int cap, int nparts, double tol2,
                                                             int max_steps, CgmStatus *__restrict__ st, double *__restrict__ hist_rr,
                                                             double *__restrict__ hist_rz)
{
    const size_t v = blockIdx.x;
    const double bb = cg_fold_parts(parts_bb + v * cap, nparts);
    const double rr = cg_fold_parts(parts_rr + v * cap, nparts);
    const double rho = OwnRho ? cg_fold_parts(parts_rz + v * cap, nparts) : rr;
    if (threadIdx.x != 0)
        return;
    CgmStatus s;
    s.rho = rho;
    s.rr = rr;
    s.bb = bb;
    s.thr = tol2 * bb;
    const bool bad = !cg_finite(bb) || !cg_finite(rr) || !cg_finite(rho);
    const bool down = OwnRho && !(rho > 0.0);
    s.stopped = bad || rr <= s.thr || down;
    s.reason = bad ? SMVP_CG_NONFINITE : rr <= s.thr || !OwnRho ? SMVP_CG_CONVERGED : SMVP_CG_BREAKDOWN;
    s.steps = 0;
    s.updates = 0;
    st[v] = s;
    hist_rr[v * ((size_t)max_steps + 1)] = rr;
    if (OwnRho)
        hist_rz[v * ((size_t)max_steps + 1)] = rho;
}

// step k: sigma_k, rule A and alpha_k of the column into its words
__global__ __launch_bounds__(kCgBlock) void cgm_sigma_finish(const double *__restrict__ parts_pq, int cap, int nparts,
                                                             const CgmStatus *__restrict__ prev, CgmWords *__restrict__ words)
{
    const size_t v = blockIdx.x;
    const CgmStatus s = prev[v];
    if (s.stopped) {
        if (threadIdx.x == 0)
            words[v].residual = 0;
        return;
    }
    const double sigma = cg_fold_parts(parts_pq + v * cap, nparts);
    if (threadIdx.x != 0)
        return;
    words[v].sigma = sigma;
    words[v].alpha = s.rho / sigma;
    words[v].residual = cg_finite(sigma) && sigma > 0.0;  // else rule A: cgm_rho_finish reports it
}

// step k: rule A's report, or rr_k, rho_k, rule B and beta_k; the column's status block k, its history elements and what
// cgm_direction is to do with it.  A column that had stopped is carried over.
template <bool OwnRho>
__global__ __launch_bounds__(kCgBlock) void cgm_rho_finish(const double *__restrict__ parts_rr, const double *__restrict__ parts_rz, int cap,
                                                           int nparts, const CgmStatus *__restrict__ prev, CgmStatus *__restrict__ cur,
                                                           CgmWords *__restrict__ words, int step, int max_steps,
                                                           double *__restrict__ hist_rr, double *__restrict__ hist_rz,
                                                           double *__restrict__ hist_sigma)
{
    const size_t v = blockIdx.x;
    const bool first = threadIdx.x == 0;
    CgmStatus s = prev[v];
    if (s.stopped) {
        if (first) {
            cur[v] = s;
            words[v].direction = 0;
        }
        return;
    }
    const double sigma = words[v].sigma;
    s.steps = step;
    if (!cg_finite(sigma) || !(sigma > 0.0)) {  // rule A: x stays x_{k-1}
        if (first) {
            s.stopped = 1;
            s.reason = cg_finite(sigma) ? SMVP_CG_BREAKDOWN : SMVP_CG_NONFINITE;
            cur[v] = s;
            words[v].direction = 0;
            hist_sigma[v * (size_t)max_steps + step - 1] = sigma;
        }
        return;
    }
    const double rr = cg_fold_parts(parts_rr + v * cap, nparts);
    const double rho = OwnRho ? cg_fold_parts(parts_rz + v * cap, nparts) : rr;
    if (!first)
        return;
    const bool bad = !cg_finite(rr) || !cg_finite(rho);
    const bool down = OwnRho && !(rho > 0.0);  // K12's rule B has no such rule
    const bool stop = bad || rr <= s.thr || down || step == max_steps;
    words[v].beta = rho / s.rho;
    words[v].direction = stop ? 1 : 2;
    s.rho = rho;
    s.rr = rr;
    s.updates = step;
    s.stopped = stop;
    s.reason = bad ? SMVP_CG_NONFINITE : rr <= s.thr ? SMVP_CG_CONVERGED : down ? SMVP_CG_BREAKDOWN : SMVP_CG_MAX_STEPS;
    cur[v] = s;
    hist_sigma[v * (size_t)max_steps + step - 1] = sigma;
    hist_rr[v * ((size_t)max_steps + 1) + step] = rr;
    if (OwnRho)
        hist_rz[v * ((size_t)max_steps + 1) + step] = rho;
}

// ------------------------------------------------------------------------------------------------------------------ the host side
// launch(W, v0, nv) once per group of at most kCgmMaxColumns columns, W = the group's width as a compile-time constant
template <typename Launch>
void for_each_group(int k, Launch launch)
{
    for (long long v0 = 0; v0 < k; v0 += kCgmMaxColumns) {
        const int nv = (int)std::min<long long>(k - v0, kCgmMaxColumns);
        if (nv == 1)
            launch(std::integral_constant<int, 1>(), v0, nv);
        else if (nv == 2)
            launch(std::integral_constant<int, 2>(), v0, nv);
        else if (nv <= 4)
            launch(std::integral_constant<int, 4>(), v0, nv);
        else if (nv <= 8)
            launch(std::integral_constant<int, 8>(), v0, nv);
        else
            launch(std::integral_constant<int, 16>(), v0, nv);
    }
}

using CgmWork = KrylovWork<CgmStatus>;  // R, P, Q; the partials of three dots per column, the columns' words, the histories; 2 x k blocks

inline size_t round32(size_t doubles) { return (doubles + 31) / 32 * 32; }

// a looked step: the k status blocks, nothing else, and only to leave the loop -> have all columns stopped?
int cgm_look(CgmWork &w, const char *fn, const CgmStatus *blocks, int k, int step, int max_steps, bool *all_stopped)
{
    HIP_TRY(hipMemcpyAsync(w.seen, blocks, sizeof(CgmStatus) * (size_t)k, hipMemcpyDeviceToHost, w.stream));
    HIP_TRY(hipStreamSynchronize(w.stream));
    *all_stopped = true;
    for (int v = 0; v < k; ++v)
        *all_stopped = *all_stopped && w.seen[v].stopped;
    if (step == max_steps && !*all_stopped)
        return smvp::fail(SMVP_ERR_HIP, "%s: the device did not stop every column at max_steps = %d", fn, max_steps);
    return SMVP_OK;
}

// the workspace and the loop; the caller has checked everything and made the device current
template <bool kDiag>
int cgm_steps(const char *fn, int n, const smvp_cg_opts_t *o, int k, const double *d_B, long long ldb, const double *d_X0, long long ldx0,
              double *d_X, long long ldx, const double *d_m, smvp_pcg_result_t *results, double *rr_each, double *rz_each,
              double *sigma_each, hipStream_t st, const BlockProduct &product)
{
    CgmWork w;
    w.stream = st;
    const int max_steps = o->max_steps, grid = cg_grid(n), cap = kCgGridCap;
    const size_t kk = (size_t)k, pitch = round32((size_t)n * kk), parts = kk * cap, hist = kk * ((size_t)max_steps + 1);
    const size_t words_doubles = kk * (sizeof(CgmWords) / sizeof(double));
    static_assert(sizeof(CgmWords) % sizeof(double) == 0, "the words live among doubles");
    if (hipMalloc((void **)&w.vec, sizeof(double) * 3 * pitch) != hipSuccess ||
        hipMalloc((void **)&w.small, sizeof(double) * (3 * parts + words_doubles + 2 * hist + kk * (size_t)max_steps)) != hipSuccess ||
        hipMalloc((void **)&w.st, 2 * kk * sizeof(CgmStatus)) != hipSuccess ||
        hipHostMalloc((void **)&w.seen, kk * sizeof(CgmStatus)) != hipSuccess) {
        (void)hipGetLastError();
        return smvp::fail(SMVP_ERR_ALLOC, "%s: cannot allocate the workspace (%d elements, %d columns, %d steps)", fn, n, k, max_steps);
    }
    double *R = w.vec, *P = R + pitch, *Q = P + pitch;
    double *parts_a = w.small, *parts_b = parts_a + parts, *parts_c = parts_b + parts;
    CgmWords *words = (CgmWords *)(parts_c + parts);
    double *hist_rr = parts_c + parts + words_doubles, *hist_rz = hist_rr + hist, *hist_sigma = hist_rz + hist;
    const long long ld = k;
    const double tol2 = o->tol * o->tol;
    const dim3 g(grid), cols((unsigned)k), blk(kCgBlock);

    // step 0: q = A x_0 (none without an x_0: r_0 is b itself); x_0 into d_X, r_0, p_0 and the partials of bb, rr_0, rho_0 in one
    // pass; the first status blocks
    if (d_X0)
        if (int rc = product(d_X0, ldx0, Q, ld))
            return rc;
    for_each_group(k, [&](auto W, long long v0, int nv) {
        hipLaunchKernelGGL((cgm_start<decltype(W)::value, kDiag>), g, blk, 0, st, d_B + v0, ldb, d_X0 ? Q + v0 : nullptr,
                           d_X0 ? d_X0 + v0 : nullptr, ldx0, d_X + v0, ldx, (int)(d_X != d_X0), d_m, R + v0, P + v0, ld, n, nv, cap,
                           parts_a + v0 * cap, parts_b + v0 * cap, parts_c + v0 * cap);
    });
    hipLaunchKernelGGL(cgm_start_finish<kDiag>, cols, blk, 0, st, parts_a, parts_b, parts_c, cap, grid, tol2, max_steps, w.st, hist_rr, hist_rz);
    HIP_TRY(hipGetLastError());
    bool done = false;
    if (int rc = cgm_look(w, fn, w.st, k, 0, max_steps, &done))
        return rc;

    for (int step = 1; !done; ++step) {
        const CgmStatus *prev = w.st + (size_t)((step - 1) & 1) * kk;
        CgmStatus *cur = w.st + (size_t)(step & 1) * kk;
        if (int rc = product(P, ld, Q, ld))
            return rc;
        if (k == 1)  // (one contiguous column: the one-vector dot's own pass)
            hipLaunchKernelGGL(krylov_dot_parts, g, blk, 0, st, P, Q, n, parts_a);
        else
            for_each_group(k, [&](auto W, long long v0, int nv) {
                hipLaunchKernelGGL(cgm_dot<decltype(W)::value>, g, blk, 0, st, P + v0, Q + v0, ld, n, nv, cap, parts_a + v0 * cap);
            });
        hipLaunchKernelGGL(cgm_sigma_finish, cols, blk, 0, st, parts_a, cap, grid, prev, words);
        for_each_group(k, [&](auto W, long long v0, int nv) {
            hipLaunchKernelGGL((cgm_residual<decltype(W)::value, kDiag>), g, blk, 0, st, Q + v0, R + v0, ld, d_m, n, nv, cap, words + v0,
                               parts_b + v0 * cap, parts_c + v0 * cap);
        });
        hipLaunchKernelGGL(cgm_rho_finish<kDiag>, cols, blk, 0, st, parts_b, parts_c, cap, grid, prev, cur, words, step, max_steps, hist_rr,
                           hist_rz, hist_sigma);
        for_each_group(k, [&](auto W, long long v0, int nv) {
            hipLaunchKernelGGL((cgm_direction<decltype(W)::value, kDiag>), g, blk, 0, st, d_X + v0, ldx, P + v0, R + v0, ld, d_m, n, nv,
                               words + v0);
        });
        HIP_TRY(hipGetLastError());
        if (step % o->check_every == 0 || step == max_steps)
            if (int rc = cgm_look(w, fn, cur, k, step, max_steps, &done))
                return rc;
    }

    // w.seen holds every column's final block.  The histories come back once, whole; the caller's get the filled elements.
    std::vector<double> host;
    const auto history = [&](double *each, const double *dev, size_t per_column, auto filled) -> int {
        if (!each)
            return SMVP_OK;
        try {
            host.resize(kk * per_column);
        } catch (const std::bad_alloc &) {
            return smvp::fail(SMVP_ERR_ALLOC, "%s: cannot allocate the host copy of a history", fn);
        }
        HIP_TRY(hipMemcpy(host.data(), dev, sizeof(double) * kk * per_column, hipMemcpyDeviceToHost));
        for (size_t v = 0; v < kk; ++v)
            memcpy(each + v * per_column, host.data() + v * per_column, sizeof(double) * (size_t)filled(w.seen[v]));
        return SMVP_OK;
    };
    if (int rc = history(rr_each, hist_rr, (size_t)max_steps + 1, [](const CgmStatus &s) { return s.updates + 1; }))
        return rc;
    if (kDiag)
        if (int rc = history(rz_each, hist_rz, (size_t)max_steps + 1, [](const CgmStatus &s) { return s.updates + 1; }))
            return rc;
    if (int rc = history(sigma_each, hist_sigma, (size_t)max_steps, [](const CgmStatus &s) { return s.steps; }))
        return rc;
    for (size_t v = 0; v < kk; ++v) {
        const CgmStatus &s = w.seen[v];
        memset(&results[v], 0, sizeof results[v]);
        results[v].steps = s.steps;
        results[v].updates = s.updates;
        results[v].reason = s.reason;
        results[v].rr = s.rr;
        results[v].rz = s.rho;
        results[v].bb = s.bb;
    }
    return SMVP_OK;
}

}  // namespace

int cg_multi_check_args(const char *fn, const void *h, const smvp_cg_opts_t *o, const void *results, const double *d_B)
{
    if (!h || !o || !results || !d_B)
        return smvp::fail(SMVP_ERR_INVALID, "%s: null %s", fn, !h ? "handle" : !o ? "opts" : !results ? "results" : "d_B");
    return krylov_check_args(fn, "cg", h, o, results, d_B);  // the options
}

int cg_multi_run(const char *fn, int device, int rows, int cols, const smvp_cg_opts_t *o, int k, const double *d_B, long long ldb,
                 const double *d_X0, long long ldx0, double *d_X, long long ldx, const double *d_m, smvp_pcg_result_t *results,
                 double *rr_each, double *rz_each, double *sigma_each, void *stream, const BlockProduct &product)
{
    if (k < 1 || ldb < k || ldx < k || (d_X0 && ldx0 < k))
        return smvp::fail(SMVP_ERR_INVALID, "%s: k = %d, ldb = %lld, ldx0 = %lld, ldx = %lld (need k >= 1 and every leading dimension >= k)",
                          fn, k, ldb, ldx0, ldx);
    if (rows != cols)
        return smvp::fail(SMVP_ERR_INVALID, "%s: conjugate gradients need a square matrix (%d x %d given)", fn, rows, cols);
    const int n = rows;
    if (n > 0 && !d_X)
        return smvp::fail(SMVP_ERR_INVALID, "%s: null d_X", fn);
    if (!(d_X0 == d_X && ldx0 == ldx) && operands_overlap(d_X0, ldx0, n, d_X, ldx, n, k))
        return smvp::fail(SMVP_ERR_INVALID, "%s: d_X0 and d_X overlap without being the same block", fn);
    if (operands_overlap(d_B, ldb, n, d_X, ldx, n, k))
        return smvp::fail(SMVP_ERR_INVALID, "%s: d_B and d_X overlap", fn);
    if (operands_overlap(d_m, 1, n, d_X, ldx, n, 1, k))
        return smvp::fail(SMVP_ERR_INVALID, "%s: d_m and d_X overlap", fn);
    DeviceScope on(device);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = refuse_capture(st, "conjugate gradients for k right-hand sides allocate and synchronise, so they cannot be captured (the "
                                    "stream is capturing)"))
        return rc;
    if (n > 0)  // (the blocks are written last, after everything else has succeeded)
        return d_m ? cgm_steps<true>(fn, n, o, k, d_B, ldb, d_X0, ldx0, d_X, ldx, d_m, results, rr_each, rz_each, sigma_each, st, product)
                   : cgm_steps<false>(fn, n, o, k, d_B, ldb, d_X0, ldx0, d_X, ldx, d_m, results, rr_each, rz_each, sigma_each, st, product);
    for (int v = 0; v < k; ++v) {
        memset(&results[v], 0, sizeof results[v]);
        results[v].reason = SMVP_CG_CONVERGED;
    }
    return SMVP_OK;
}

}  // namespace smvp
