// smvp_lsqr.hip -- K22: LSQR on a handle's own pair of products, min |A x - b| for any M x N matrix, to the bits include/smvp_amd.h
// defines (smvp_csr_lsqr with the caller's handle of A^T, smvp_tjds_lsqr with K8's transposed product of the one handle).  New: the
// reference only multiplies.  The dot's folds, the grid rule, the workspace holder, the look and the launch discipline are
// smvp_cg_common.h's.
//
// The bidiagonalisation's vectors are stored unnormalised (uh = beta u over M elements, vh = alpha v over N) and every scaling rides
// in the next pass that reads the vector.  Beside the two products a step k is two launches and eleven passes over a vector:
//
//   ls_pass_u   after q = A vh_k.  Every workgroup folds the partials of dot(vh_k, vh_k) to alpha_k and, with beta_k from pass V's
//               word, closes step k - 1: its rotation, its estimates and its rules, from status block k - 2; workgroup 0 writes
//               status block k - 1 and the history elements.  Then step k - 1's x += tx w and w = vh / alpha_k - tw w
//               (vh, w, x read, w, x written: 5 passes over N) and uh_{k+1} = q / alpha_k - alpha_k (uh_k / beta_k) with the
//               partials of its dot (q, uh read, uh written: 3 passes over M).  The grid covers max(M, N): workgroup g takes part in
//               a vector's loop where g is below that vector's own grid, so each dot keeps its own slot map.
//   ls_pass_v   after p = A^T uh_{k+1}.  Every workgroup folds the partials of dot(uh_{k+1}, uh_{k+1}) to beta_{k+1} (workgroup 0
//               leaves it in the word) and writes vh_{k+1} = p / beta_{k+1} - beta_{k+1} (vh_k / alpha_k) with the partials of its
//               dot (p, vh read, vh written: 3 passes over N).
//
// So the close of a step rides in the next step's pass U, where alpha_{k+1} is first known.  The host can only look at a step that
// is closed: at a looked step it launches the close on its own (ls_pass_u without the uh half, kClose alone) and tells the next
// step's pass U that nothing is left to close (kPlain: alpha_k and beta_k come from the status block).  The arithmetic is the same
// either way, so nothing depends on check_every.  Step 1's pass U has no step to close and writes w_1 = vh_1 / alpha_1 (kFirst).
// A rule that has fired is known to every workgroup of the launch that finds it (each evaluates the close itself) and to every
// later launch from the status block: the step that fires completes its update of x (rule N excepted), and nothing is written to
// x, w, uh, vh or the histories after it; the products enqueued in vain write the workspace's q and p only.
#include "smvp_cg_common.h"
#include "smvp_engine.h"

#include <cmath>
#include <cstring>

namespace smvp {

namespace {

// status block j: what the close of step j leaves behind (block 0: step 0's rules)
struct LsStatus {
    double alpha, beta;     // alpha_{j+1}, beta_{j+1}: the norms of the stored vh and uh
    double phibar, rhobar;  // phibar_{j+1}, rhobar_{j+1}
    double a2;              // the running square of anorm
    double bnorm, thr;      // sqrt(dot(b, b)), tol * bnorm
    double rnorm, arnorm, anorm;  // of step `updates`
    int stopped;            // a rule has fired: everything here is final
    int reason;             // SMVP_LSQR_*
    int steps;              // the step the run stopped in (else j)
    int updates;            // updates of x done
};

enum { kFirst = 1, kClose = 2, kPlain = 4, kWriteU = 8 };  // ls_pass_u's modes: one of the first three, with or without the uh half

// a norm that divides: the root of a dot, or +0.0 where the vector was not formed (its scaling was zero or not finite)
__device__ inline double ls_norm_after(double scaling, double dd) { return cg_finite(scaling) && scaling != 0.0 ? sqrt(dd) : 0.0; }

// uh_1 = b - q (q = A x_0), or b itself without a q, with the partials of dot(uh_1, uh_1)
__global__ __launch_bounds__(kCgBlock) void ls_start(const double *__restrict__ b, const double *__restrict__ q, double *__restrict__ uh,
                                                     int m, double *__restrict__ parts)
{
    const long long stride = (long long)gridDim.x * kCgBlock;
    double c = 0.0;
    for (long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x; i < m; i += stride) {
        const double v = q ? b[i] - q[i] : b[i];
        uh[i] = v;
        const double t = v * v;
        c = c + t;
    }
    c = cg_fold256(c);
    if (threadIdx.x == 0)
        parts[blockIdx.x] = c;
}

// step k (First: k = 0, no status block yet and no vh_0): beta_{k+1} from the partials of dot(uh, uh), vh over itself, the partials
// of dot(vh, vh).  A beta that cannot divide forms no vector; the close takes alpha as +0.0 then.
template <bool First>
__global__ __launch_bounds__(kCgBlock) void ls_pass_v(const double *__restrict__ p, double *vh, int n, int mparts,
                                                      const double *__restrict__ parts_u, const LsStatus *__restrict__ prev,
                                                      double *__restrict__ word, double *__restrict__ parts_v)
{
    if (!First && prev->stopped)
        return;
    const double beta = sqrt(cg_fold_parts(parts_u, mparts));
    if (blockIdx.x == 0 && threadIdx.x == 0)
        *word = beta;
    if (!cg_finite(beta) || beta == 0.0)
        return;
    const double alpha = First ? 1.0 : prev->alpha;
    const long long stride = (long long)gridDim.x * kCgBlock;
    long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x;
    double c = 0.0;
    for (; i + (kCgTrips - 1) * stride < n; i += kCgTrips * stride) {
        double pv[kCgTrips], vv[kCgTrips];
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            pv[u] = p[i + u * stride];
            if (!First)
                vv[u] = vh[i + u * stride];
        }
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            double vn = pv[u] / beta;
            if (!First) {
                const double d = vv[u] / alpha;
                const double e = beta * d;
                vn = vn - e;
            }
            vh[i + u * stride] = vn;
            const double t = vn * vn;
            c = c + t;
        }
    }
    for (; i < n; i += stride) {
        double vn = p[i] / beta;
        if (!First) {
            const double d = vh[i] / alpha;
            const double e = beta * d;
            vn = vn - e;
        }
        vh[i] = vn;
        const double t = vn * vn;
        c = c + t;
    }
    c = cg_fold256(c);
    if (threadIdx.x == 0)
        parts_v[blockIdx.x] = c;
}

// one workgroup: bnorm, beta_1, alpha_1, the estimates and step 0's rules into status block 0, history element 0
__global__ __launch_bounds__(kCgBlock) void ls_open(const double *__restrict__ parts_b, const double *__restrict__ parts_u, int mparts,
                                                    const double *__restrict__ parts_v, int nparts, double tol, LsStatus *__restrict__ st,
                                                    double *__restrict__ hist_r, double *__restrict__ hist_ar)
{
    const double bb = cg_fold_parts(parts_b, mparts);
    const double uu = cg_fold_parts(parts_u, mparts);
    const double vv = cg_fold_parts(parts_v, nparts);  // (not written where beta_1 cannot divide: not used then)
    if (threadIdx.x != 0)
        return;
    LsStatus s;
    s.bnorm = sqrt(bb);
    s.thr = tol * s.bnorm;
    s.beta = sqrt(uu);
    s.alpha = ls_norm_after(s.beta, vv);
    s.phibar = s.beta;
    s.rhobar = s.alpha;
    s.a2 = s.alpha * s.alpha;
    s.anorm = sqrt(s.a2);
    s.rnorm = s.beta;
    s.arnorm = s.beta * s.alpha;
    const bool bad = !cg_finite(s.bnorm) || !cg_finite(s.beta) || !cg_finite(s.alpha) || !cg_finite(s.anorm) || !cg_finite(s.arnorm);
    const bool done = s.beta <= s.thr;
    s.stopped = bad || done || s.alpha == 0.0;
    s.reason = bad ? SMVP_LSQR_NONFINITE : done ? SMVP_LSQR_CONVERGED : SMVP_LSQR_LEAST_SQUARES;
    s.steps = 0;
    s.updates = 0;
    st[0] = s;
    hist_r[0] = s.rnorm;
    hist_ar[0] = s.arnorm;
}

// the close of step `step` from the block before it, beta_{step+1} and alpha_{step+1}: the block after it and the two factors of
// the updates.  false: rule N, nothing of the step is applied.
__device__ inline bool ls_close(const LsStatus &before, double beta, double alpha, int step, int max_steps, double atol, LsStatus *after,
                                double *tx, double *tw)
{
    LsStatus s = before;
    const double bb = beta * beta, rr = s.rhobar * s.rhobar;
    const double rho = sqrt(rr + bb);
    const double c = s.rhobar / rho, sn = beta / rho;
    const double theta = sn * alpha;
    const double ca = c * alpha;
    const double phi = c * s.phibar, phibar = sn * s.phibar;
    *tx = phi / rho;
    *tw = theta / rho;
    const double aa = alpha * alpha;
    const double a2 = (s.a2 + bb) + aa;
    const double anorm = sqrt(a2);
    const double ac = alpha * fabs(c);
    const double arnorm = phibar * ac;
    s.steps = step;
    if (!cg_finite(beta) || !cg_finite(alpha) || !cg_finite(rho) || !cg_finite(*tx) || !cg_finite(*tw) || !cg_finite(anorm) ||
        !cg_finite(phibar) || !cg_finite(arnorm)) {
        s.stopped = 1;
        s.reason = SMVP_LSQR_NONFINITE;
        *after = s;
        return false;
    }
    s.alpha = alpha;
    s.beta = beta;
    s.phibar = phibar;
    s.rhobar = -ca;
    s.a2 = a2;
    s.rnorm = phibar;
    s.arnorm = arnorm;
    s.anorm = anorm;
    s.updates = step;
    const double bound = atol * anorm;
    const int reason = phibar <= s.thr ? SMVP_LSQR_CONVERGED : ac <= bound ? SMVP_LSQR_LEAST_SQUARES : step == max_steps ? SMVP_LSQR_MAX_STEPS : -1;
    s.stopped = reason >= 0;
    if (reason >= 0)
        s.reason = reason;
    *after = s;
    return true;
}

// step k's pass U (the header of this file).  from: kFirst, kPlain: status block k - 1; kClose: block k - 2, and `to` is block k - 1.
__global__ __launch_bounds__(kCgBlock) void ls_pass_u(int mode, const double *__restrict__ q, double *uh, int m, int mgrid,
                                                      const double *__restrict__ vh, double *w, double *x, int n, int ngrid,
                                                      const double *__restrict__ parts_v, const double *__restrict__ word,
                                                      const LsStatus *__restrict__ from, LsStatus *__restrict__ to, int k, int max_steps,
                                                      double atol, double *__restrict__ hist_r, double *__restrict__ hist_ar,
                                                      double *__restrict__ parts_u)
{
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    LsStatus s = *from;
    if (s.stopped) {
        if ((mode & kClose) && first)
            *to = s;
        return;
    }
    const long long lane = (long long)blockIdx.x * kCgBlock + threadIdx.x;
    if (mode & kClose) {
        const double beta = *word;
        const double alpha = ls_norm_after(beta, cg_fold_parts(parts_v, ngrid));
        double tx, tw;
        const bool applied = ls_close(s, beta, alpha, k - 1, max_steps, atol, &s, &tx, &tw);
        if (first) {
            *to = s;
            if (applied) {
                hist_r[k - 1] = s.rnorm;
                hist_ar[k - 1] = s.arnorm;
            }
        }
        if (!applied)
            return;
        if ((int)blockIdx.x < ngrid) {
            const long long stride = (long long)ngrid * kCgBlock;
            long long i = lane;
            if (s.stopped) {  // the last update of x; no w_{k}: alpha may be zero
                for (; i < n; i += stride) {
                    const double t = tx * w[i];
                    x[i] = x[i] + t;
                }
            } else {
                for (; i + (kCgTrips - 1) * stride < n; i += kCgTrips * stride) {
                    double xv[kCgTrips], wv[kCgTrips], vv[kCgTrips];
#pragma unroll
                    for (int u = 0; u < kCgTrips; ++u) {
                        xv[u] = x[i + u * stride];
                        wv[u] = w[i + u * stride];
                        vv[u] = vh[i + u * stride];
                    }
#pragma unroll
                    for (int u = 0; u < kCgTrips; ++u) {
                        const double t = tx * wv[u];
                        x[i + u * stride] = xv[u] + t;
                        const double d = vv[u] / alpha, e = tw * wv[u];
                        w[i + u * stride] = d - e;
                    }
                }
                for (; i < n; i += stride) {
                    const double wv = w[i];
                    const double t = tx * wv;
                    x[i] = x[i] + t;
                    const double d = vh[i] / alpha, e = tw * wv;
                    w[i] = d - e;
                }
            }
        }
        if (s.stopped)
            return;
    } else if ((mode & kFirst) && (int)blockIdx.x < ngrid) {
        const long long stride = (long long)ngrid * kCgBlock;
        for (long long i = lane; i < n; i += stride)
            w[i] = vh[i] / s.alpha;
    }
    if (!(mode & kWriteU) || (int)blockIdx.x >= mgrid)
        return;
    const double alpha = s.alpha, beta = s.beta;  // alpha_k, beta_k
    const long long stride = (long long)mgrid * kCgBlock;
    long long i = lane;
    double c = 0.0;
    for (; i + (kCgTrips - 1) * stride < m; i += kCgTrips * stride) {
        double qv[kCgTrips], uv[kCgTrips];
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            qv[u] = q[i + u * stride];
            uv[u] = uh[i + u * stride];
        }
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            const double a = qv[u] / alpha, d = uv[u] / beta;
            const double e = alpha * d;
            const double un = a - e;
            uh[i + u * stride] = un;
            const double t = un * un;
            c = c + t;
        }
    }
    for (; i < m; i += stride) {
        const double a = q[i] / alpha, d = uh[i] / beta;
        const double e = alpha * d;
        const double un = a - e;
        uh[i] = un;
        const double t = un * un;
        c = c + t;
    }
    c = cg_fold256(c);
    if (threadIdx.x == 0)
        parts_u[blockIdx.x] = c;
}

using LsWork = KrylovWork<LsStatus>;  // uh, q (M each), vh, p, w (N each); the partials of three dots, pass V's word, the histories

}  // namespace

int lsqr_run(const char *fn, int device, int rows, int cols, const smvp_lsqr_opts_t *o, const double *d_b, const double *d_x0, double *d_x,
             smvp_lsqr_result_t *result, double *rnorm_each, double *arnorm_each, void *stream, const HandleProduct &forward,
             const HandleProduct &transposed)
{
    const int m = rows, n = cols;
    if (n > 0 && !d_x)
        return smvp::fail(SMVP_ERR_INVALID, "%s: null d_x", fn);
    if (d_x0 != d_x && operands_overlap(d_x0, 1, n, d_x, 1, n, 1))
        return smvp::fail(SMVP_ERR_INVALID, "%s: d_x0 and d_x overlap without being the same vector", fn);
    if (operands_overlap(d_b, 1, m, d_x, 1, n, 1))
        return smvp::fail(SMVP_ERR_INVALID, "%s: d_b and d_x overlap", fn);
    DeviceScope on(device);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = refuse_capture(st, "LSQR allocates and synchronises, so it cannot be captured (the stream is capturing)"))
        return rc;
    smvp_lsqr_result_t res;
    memset(&res, 0, sizeof res);
    res.reason = SMVP_LSQR_CONVERGED;
    if (m == 0 || n == 0) {
        if (n > 0) {  // no equation: x_0 stands
            if (!d_x0)
                HIP_TRY(hipMemsetAsync(d_x, 0, sizeof(double) * (size_t)n, st));
            else if (d_x0 != d_x)
                HIP_TRY(hipMemcpyAsync(d_x, d_x0, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        for (double *each : {rnorm_each, arnorm_each})
            if (each)
                each[0] = 0.0;  // updates = 0: element 0 is filled
        *result = res;
        return SMVP_OK;
    }

    LsWork w;
    w.stream = st;
    const int max_steps = o->max_steps, mgrid = cg_grid(m), ngrid = cg_grid(n);
    const size_t mpitch = krylov_pitch(m), npitch = krylov_pitch(n);
    if (int rc = krylov_alloc(w, fn, m > n ? m : n, max_steps, 2 * mpitch + 3 * npitch, 3 * (size_t)kCgGridCap + 1 + 2 * ((size_t)max_steps + 1)))
        return rc;
    double *uh = w.vec, *q = uh + mpitch, *vh = q + mpitch, *p = vh + npitch, *wv = p + npitch;
    double *parts_b = w.small, *parts_u = parts_b + kCgGridCap, *parts_v = parts_u + kCgGridCap;
    double *word = parts_v + kCgGridCap, *hist_r = word + 1, *hist_ar = hist_r + max_steps + 1;
    const dim3 gm(mgrid), gn(ngrid), gu(mgrid > ngrid ? mgrid : ngrid), blk(kCgBlock);

    // step 0: x_0 into d_x, bnorm, uh_1 = b - A x_0 (b itself without an x_0: no product), beta_1, vh_1, alpha_1, the first block
    hipLaunchKernelGGL(krylov_dot_parts, gm, blk, 0, st, d_b, d_b, m, parts_b);
    if (int rc = krylov_first_x(forward, d_x0, d_x, q, n, st))
        return rc;
    hipLaunchKernelGGL(ls_start, gm, blk, 0, st, d_b, d_x0 ? q : nullptr, uh, m, parts_u);
    if (int rc = transposed(uh, p))
        return rc;
    hipLaunchKernelGGL(ls_pass_v<true>, gn, blk, 0, st, p, vh, n, mgrid, parts_u, nullptr, word, parts_v);
    hipLaunchKernelGGL(ls_open, dim3(1), blk, 0, st, parts_b, parts_u, mgrid, parts_v, ngrid, o->tol, w.st, hist_r, hist_ar);
    HIP_TRY(hipGetLastError());
    LsStatus hs;
    if (int rc = krylov_look(w, fn, w.st, 0, max_steps, &hs))
        return rc;

    int closed = 0;  // the last step whose status block has been written
    for (int k = 1; !hs.stopped; ++k) {
        if (int rc = forward(vh, q))
            return rc;
        const int mode = (k == 1 ? kFirst : closed == k - 1 ? kPlain : kClose) | kWriteU;
        // kClose reads block k - 2 and writes block k - 1; the others read block k - 1
        hipLaunchKernelGGL(ls_pass_u, gu, blk, 0, st, mode, q, uh, m, mgrid, vh, wv, d_x, n, ngrid, parts_v, word,
                           w.st + ((mode & kClose ? k - 2 : k - 1) & 1), w.st + ((k - 1) & 1), k, max_steps, o->atol, hist_r, hist_ar, parts_u);
        closed = k - 1;
        if (int rc = transposed(uh, p))
            return rc;
        hipLaunchKernelGGL(ls_pass_v<false>, gn, blk, 0, st, p, vh, n, mgrid, parts_u, w.st + ((k - 1) & 1), word, parts_v);
        if (k % o->check_every == 0 || k == max_steps) {
            hipLaunchKernelGGL(ls_pass_u, gn, blk, 0, st, (int)kClose, q, uh, m, mgrid, vh, wv, d_x, n, ngrid, parts_v, word,
                               w.st + ((k - 1) & 1), w.st + (k & 1), k + 1, max_steps, o->atol, hist_r, hist_ar, parts_u);
            closed = k;
            HIP_TRY(hipGetLastError());
            if (int rc = krylov_look(w, fn, w.st + (k & 1), k, max_steps, &hs))
                return rc;
        } else
            HIP_TRY(hipGetLastError());
    }
    if (int rc = krylov_history(rnorm_each, hist_r, hs.updates + 1))
        return rc;
    if (int rc = krylov_history(arnorm_each, hist_ar, hs.updates + 1))
        return rc;
    res.steps = hs.steps;
    res.updates = hs.updates;
    res.reason = hs.reason;
    res.rnorm = hs.rnorm;
    res.arnorm = hs.arnorm;
    res.anorm = hs.anorm;
    res.bnorm = hs.bnorm;
    *result = res;
    return SMVP_OK;
}

}  // namespace smvp
