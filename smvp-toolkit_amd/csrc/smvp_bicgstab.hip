// smvp_bicgstab.hip -- BiCGSTAB on a handle's own product, A x = b for a general square matrix, to the bits include/smvp_amd.h
// defines: K13 without a preconditioner (smvp_csr_bicgstab, smvp_tjds_bicgstab) and K18, right-preconditioned with K16's
// M = T1 diag(m)^-1 T2, each of the three parts optional (smvp_csr_pbicgstab, smvp_tjds_pbicgstab).  New: the reference only ever
// multiplies.  The dot, its folds, the grid rule, the workspace holder, krylov_apply and the launch discipline are
// smvp_cg_common.h's; the solves are K15's kernels, enqueued through smvp::trsv_enqueue.
//
// One set of kernels and one host loop.  A step k has x_{k-1} in the caller's d_x, r_{k-1}, p_{k-1}, the shadow residual rhat = r_0
// and rho_{k-1} = dot(rhat, r_{k-1}) in the status block.  K18: phat = M^-1 p_{k-1} comes first, then v = A phat (the handle's own
// launch, whatever its plan); shat = M^-1 s and t = A shat sit between the second and the third launch below.  K13 is the same
// loop with no M^-1: v = A p, t = A s, five vectors and not seven, and the plain bi_full.  Beside the two products and the solves'
// own launches a step is five launches of the dot's grid; K13: eighteen vector passes, K18: nineteen.
//
//   bi_sigma_parts  the partials of sigma = dot(rhat, v)                                             (rhat, v read: 2 passes)
//   bi_half         every workgroup folds those partials itself: sigma, alpha = rho_{k-1} / sigma, rule A.  s = r - alpha v over r
//                   with the partials of ss = dot(s, s)                                     (v, r read, r written: 3 passes)
//   bi_t_parts      the partials of ts = dot(t, s) and tt = dot(t, t) in one pass: two accumulators per lane, each in the dot's
//                   order                                                                            (t, s read: 2 passes)
//   bi_full         every workgroup folds ss, ts and tt and evaluates rules H and T.  x = (x + alpha phat) + omega shat and
//                   r = s - omega t with the partials of rr = dot(r, r) and rho = dot(rhat, r)
//                   (x, phat, shat, s, t, rhat read, x, r written: 8 passes; bi_full<false>, K13's, reads p for phat and s once for
//                   both of its uses: 7 passes); where rule H converges or rule T breaks down, only x = x + alpha phat
//   bi_direction    every workgroup folds rr and rho and evaluates rule B; p = r + beta (p - omega v) unless the run stops here
//                   (r, p, v read, p written: 4 passes).  Workgroup 0 writes the step's status block and the history elements.
//
// Without a `first` the multiplication by m needs no launch of its own: the kernel that produces y writes m_i * y_i beside it in the
// same pass (Scaled: bi_start and bi_direction write phat, bi_half writes shat: Jacobi is five launches a step and 23 passes, not
// seven and 25), and `second` solves in place on that.  With a `first` it is krylov_scale between the solves.  With neither a `first`
// nor an m, `second` solves straight from p or s.  The bits are the same either way.
//
// sigma (from bi_half's workgroup 0) and ss, ts, tt (from bi_full's) reach the later launches of the step through words of their own.
// Rule A is known to every launch from bi_half on, rules H and T from bi_full on; once a rule has fired, every later launch sees it
// (in the step's words, then as `stopped` in the status block) and writes nothing to x, r, p, phat, shat or the histories; the
// products, the solves and krylov_scale enqueued in vain write the workspace's v, t, phat and shat only.
#include "smvp_cg_common.h"
#include "smvp_engine.h"
#include "smvp_kernels.h"

#include <cmath>
#include <cstring>

namespace smvp {

namespace {

// what a step leaves behind for the next step's lanes and, at a looked step, for the host
struct BiStatus {
    double rho;   // rho_full = dot(rhat, r_full)
    double rr;    // the squared norm of the residual that belongs to d_x: ss of the last step after a half update, else rr_full
    double bb;    // dot(b, b)
    double thr;   // (tol * tol) * bb
    int stopped;  // a rule has fired: everything below is final
    int reason;   // SMVP_BICGSTAB_*
    int steps;    // the step the run stopped in
    int full;     // complete updates of x
    int half;     // d_x holds the alpha * phat half update on top of them
    int nss;      // elements of the ss history: the steps that reached rule H
};

// the words a step's launches hand on
enum { kBiSigma = 0, kBiSs = 1, kBiTs = 2, kBiTt = 3, kBiWords = 4 };

__device__ inline bool bi_rule_a(double sigma) { return !cg_finite(sigma) || sigma == 0.0; }

// step k's sigma: as krylov_dot_parts, and nothing once the run has stopped
__global__ __launch_bounds__(kCgBlock) void bi_sigma_parts(const double *__restrict__ rhat, const double *__restrict__ v, int n,
                                                           const BiStatus *__restrict__ prev, double *__restrict__ parts)
{
    if (prev->stopped)
        return;
    const double c = cg_fold256(cg_lane_dot(rhat, v, n));
    if (threadIdx.x == 0)
        parts[blockIdx.x] = c;
}

// r_0 = b - q (q = A x_0), or b itself without a q; rhat = p_0 = r_0; the partials of rr_0 = dot(r_0, r_0).  Scaled: phat_i =
// m_i * p_i in the same pass.
template <bool Scaled>
__global__ __launch_bounds__(kCgBlock) void bi_start(const double *__restrict__ b, const double *__restrict__ q, double *__restrict__ r,
                                                     double *__restrict__ rhat, double *__restrict__ p, const double *__restrict__ m,
                                                     double *__restrict__ phat, int n, double *__restrict__ parts)
{
    const long long stride = (long long)gridDim.x * kCgBlock;
    double c = 0.0;
    for (long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x; i < n; i += stride) {
        const double v = q ? b[i] - q[i] : b[i];
        r[i] = v;
        rhat[i] = v;
        p[i] = v;
        if (Scaled)
            phat[i] = m[i] * v;
        const double t = v * v;
        c = c + t;
    }
    c = cg_fold256(c);
    if (threadIdx.x == 0)
        parts[blockIdx.x] = c;
}

// one workgroup: bb, rr_0 = rho_0, the threshold and step 0's rule into status block 0, rr_0 into the history
__global__ __launch_bounds__(kCgBlock) void bi_start_finish(const double *__restrict__ parts_bb, const double *__restrict__ parts_rr, int nparts,
                                                            double tol2, BiStatus *__restrict__ st, double *__restrict__ hist_rr)
{
    const double bb = cg_fold_parts(parts_bb, nparts);
    const double rr = cg_fold_parts(parts_rr, nparts);
    if (threadIdx.x != 0)
        return;
    BiStatus s;
    s.rho = rr;
    s.rr = rr;
    s.bb = bb;
    s.thr = tol2 * bb;
    const bool bad = !cg_finite(bb) || !cg_finite(rr);
    s.stopped = bad || rr <= s.thr;
    s.reason = bad ? SMVP_BICGSTAB_NONFINITE : SMVP_BICGSTAB_CONVERGED;
    s.steps = 0;
    s.full = 0;
    s.half = 0;
    s.nss = 0;
    st[0] = s;
    hist_rr[0] = rr;
}

// step k: prev = the status of step k - 1, parts_sigma = the partials of dot(rhat, v).  s = r - alpha v over r, the partials of ss.
// Scaled: shat_i = m_i * s_i in the same pass.
template <bool Scaled>
__global__ __launch_bounds__(kCgBlock) void bi_half(const double *__restrict__ v, double *__restrict__ r, const double *__restrict__ m,
                                                    double *__restrict__ shat, int n, int nparts, const double *__restrict__ parts_sigma,
                                                    const BiStatus *__restrict__ prev, double *__restrict__ words,
                                                    double *__restrict__ parts_ss)
{
    if (prev->stopped)
        return;
    const double sigma = cg_fold_parts(parts_sigma, nparts);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        words[kBiSigma] = sigma;
    if (bi_rule_a(sigma))
        return;  // rule A: bi_direction reports it
    const double alpha = prev->rho / sigma;
    const long long stride = (long long)gridDim.x * kCgBlock;
    long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x;
    double c = 0.0;
    for (; i + (kCgTrips - 1) * stride < n; i += kCgTrips * stride) {
        double s[kCgTrips], av[kCgTrips], mv[kCgTrips];
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            av[u] = alpha * v[i + u * stride];  // rounded, then the difference is rounded
            s[u] = r[i + u * stride];
            if (Scaled)
                mv[u] = m[i + u * stride];
        }
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            s[u] = s[u] - av[u];
            r[i + u * stride] = s[u];
            if (Scaled)
                shat[i + u * stride] = mv[u] * s[u];
            const double t = s[u] * s[u];
            c = c + t;
        }
    }
    for (; i < n; i += stride) {
        const double av = alpha * v[i];
        const double s = r[i] - av;
        r[i] = s;
        if (Scaled)
            shat[i] = m[i] * s;
        const double t = s * s;
        c = c + t;
    }
    c = cg_fold256(c);
    if (threadIdx.x == 0)
        parts_ss[blockIdx.x] = c;
}

// step k: the partials of ts = dot(t, s) and tt = dot(t, t), each lane's two accumulators in the dot's order
__global__ __launch_bounds__(kCgBlock) void bi_t_parts(const double *__restrict__ t, const double *__restrict__ s, int n,
                                                       const BiStatus *__restrict__ prev, const double *__restrict__ words,
                                                       double *__restrict__ parts_ts, double *__restrict__ parts_tt)
{
    if (prev->stopped || bi_rule_a(words[kBiSigma]))
        return;
    const long long stride = (long long)gridDim.x * kCgBlock;
    long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x;
    double cs = 0.0, ct = 0.0;
    for (; i + (kCgDotTrips - 1) * stride < n; i += kCgDotTrips * stride) {
        double a[kCgDotTrips], b[kCgDotTrips];
#pragma unroll
        for (int u = 0; u < kCgDotTrips; ++u) {
            const double tv = t[i + u * stride];
            a[u] = tv * s[i + u * stride];
            b[u] = tv * tv;
        }
#pragma unroll
        for (int u = 0; u < kCgDotTrips; ++u) {
            cs = cs + a[u];
            ct = ct + b[u];
        }
    }
    for (; i < n; i += stride) {
        const double tv = t[i];
        const double a = tv * s[i], b = tv * tv;
        cs = cs + a;
        ct = ct + b;
    }
    cs = cg_fold256(cs);
    ct = cg_fold256(ct);
    if (threadIdx.x == 0) {
        parts_ts[blockIdx.x] = cs;
        parts_tt[blockIdx.x] = ct;
    }
}

// step k: rules H and T; x = (x + alpha phat) + omega shat, r = s - omega t (over s) with the partials of rr and rho, or the half
// update x = x + alpha phat.  Hat = false (K13, no M^-1): phat is p itself, s is read once from r for both of its uses, and shat
// is not touched.
template <bool Hat>
__global__ __launch_bounds__(kCgBlock) void bi_full(double *__restrict__ x, const double *__restrict__ phat, const double *__restrict__ shat,
                                                    double *__restrict__ r, const double *__restrict__ t, const double *__restrict__ rhat,
                                                    int n, int nparts, const double *__restrict__ parts_ss,
                                                    const double *__restrict__ parts_ts, const double *__restrict__ parts_tt,
                                                    const BiStatus *__restrict__ prev, double *__restrict__ words,
                                                    double *__restrict__ parts_rr, double *__restrict__ parts_rho)
{
    if (prev->stopped)
        return;
    const double sigma = words[kBiSigma];
    if (bi_rule_a(sigma))
        return;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    const double alpha = prev->rho / sigma;
    const double ss = cg_fold_parts(parts_ss, nparts);
    if (first)
        words[kBiSs] = ss;
    if (!cg_finite(ss))
        return;  // rule H, NONFINITE: x stays
    const long long stride = (long long)gridDim.x * kCgBlock;
    long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x;
    bool half = ss <= prev->thr;  // rule H, CONVERGED
    double omega = 0.0;
    if (!half) {
        const double ts = cg_fold_parts(parts_ts, nparts);
        const double tt = cg_fold_parts(parts_tt, nparts);
        if (first) {
            words[kBiTs] = ts;
            words[kBiTt] = tt;
        }
        if (!cg_finite(ts) || !cg_finite(tt))
            return;  // rule T, NONFINITE: x stays
        half = !(tt > 0.0);  // rule T, BREAKDOWN
        omega = ts / tt;
    }
    if (half) {
        for (; i < n; i += stride) {
            const double ap = alpha * phat[i];
            x[i] = x[i] + ap;
        }
        return;
    }
    double crr = 0.0, crho = 0.0;
    for (; i + (kCgTrips - 1) * stride < n; i += kCgTrips * stride) {
        double xv[kCgTrips], pv[kCgTrips], qv[kCgTrips], sv[kCgTrips], tv[kCgTrips], hv[kCgTrips];
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            xv[u] = x[i + u * stride];
            pv[u] = phat[i + u * stride];
            sv[u] = r[i + u * stride];
            qv[u] = Hat ? shat[i + u * stride] : sv[u];
            tv[u] = t[i + u * stride];
            hv[u] = rhat[i + u * stride];
        }
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            const double ap = alpha * pv[u], os = omega * qv[u], ot = omega * tv[u];
            const double xh = xv[u] + ap;
            x[i + u * stride] = xh + os;
            const double rv = sv[u] - ot;
            r[i + u * stride] = rv;
            const double a = rv * rv, b = hv[u] * rv;
            crr = crr + a;
            crho = crho + b;
        }
    }
    for (; i < n; i += stride) {
        const double sv = r[i];
        const double ap = alpha * phat[i], os = omega * (Hat ? shat[i] : sv), ot = omega * t[i];
        const double xh = x[i] + ap;
        x[i] = xh + os;
        const double rv = sv - ot;
        r[i] = rv;
        const double a = rv * rv, b = rhat[i] * rv;
        crr = crr + a;
        crho = crho + b;
    }
    crr = cg_fold256(crr);
    crho = cg_fold256(crho);
    if (threadIdx.x == 0) {
        parts_rr[blockIdx.x] = crr;
        parts_rho[blockIdx.x] = crho;
    }
}

// step k: the rules once more, in their order, for the status block; rule B; p = r + beta (p - omega v) unless the run stops here
// (Scaled: phat_i = m_i * p_i in the same pass).  Workgroup 0 writes status block k and the histories.
template <bool Scaled>
__global__ __launch_bounds__(kCgBlock) void bi_direction(double *__restrict__ p, const double *__restrict__ r, const double *__restrict__ v,
                                                         const double *__restrict__ m, double *__restrict__ phat, int n, int nparts,
                                                         const double *__restrict__ parts_rr, const double *__restrict__ parts_rho,
                                                         const double *__restrict__ words, const BiStatus *__restrict__ prev,
                                                         BiStatus *__restrict__ cur, int step, int max_steps, double *__restrict__ hist_rr,
                                                         double *__restrict__ hist_ss)
{
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    BiStatus s = *prev;
    if (s.stopped) {
        if (first)
            *cur = s;
        return;
    }
    s.steps = step;
    s.stopped = 1;
    const double sigma = words[kBiSigma];
    if (bi_rule_a(sigma)) {  // rule A: x stays x_{k-1}
        if (first) {
            s.reason = cg_finite(sigma) ? SMVP_BICGSTAB_BREAKDOWN : SMVP_BICGSTAB_NONFINITE;
            *cur = s;
        }
        return;
    }
    const double alpha = s.rho / sigma;
    const double ss = words[kBiSs];
    s.nss = step;
    if (!cg_finite(ss) || ss <= s.thr) {  // rule H
        if (first) {
            s.reason = cg_finite(ss) ? SMVP_BICGSTAB_CONVERGED : SMVP_BICGSTAB_NONFINITE;
            if (cg_finite(ss)) {
                s.half = 1;
                s.rr = ss;
            }
            *cur = s;
            hist_ss[step - 1] = ss;
        }
        return;
    }
    const double ts = words[kBiTs], tt = words[kBiTt];
    const bool bad_t = !cg_finite(ts) || !cg_finite(tt);
    if (bad_t || !(tt > 0.0)) {  // rule T
        if (first) {
            s.reason = bad_t ? SMVP_BICGSTAB_NONFINITE : SMVP_BICGSTAB_BREAKDOWN;
            if (!bad_t) {
                s.half = 1;
                s.rr = ss;
            }
            *cur = s;
            hist_ss[step - 1] = ss;
        }
        return;
    }
    const double omega = ts / tt;
    const double rr = cg_fold_parts(parts_rr, nparts);
    const double rho = cg_fold_parts(parts_rho, nparts);
    const bool bad = !cg_finite(rr) || !cg_finite(rho);
    int reason = -1;  // rule B, the first that holds
    if (bad)
        reason = SMVP_BICGSTAB_NONFINITE;
    else if (rr <= s.thr)
        reason = SMVP_BICGSTAB_CONVERGED;
    else if (step == max_steps)
        reason = SMVP_BICGSTAB_MAX_STEPS;
    else if (omega == 0.0 || rho == 0.0)
        reason = SMVP_BICGSTAB_BREAKDOWN;
    const double qr = rho / s.rho, qa = alpha / omega;  // two quotients rounded, then their product
    const double beta = qr * qa;
    if (first) {
        s.stopped = reason >= 0;
        if (reason >= 0)
            s.reason = reason;
        s.full = step;
        s.rr = rr;
        s.rho = rho;
        *cur = s;
        hist_ss[step - 1] = ss;
        hist_rr[step] = rr;
    }
    if (reason >= 0)
        return;
    const long long stride = (long long)gridDim.x * kCgBlock;
    long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x;
    for (; i + (kCgTrips - 1) * stride < n; i += kCgTrips * stride) {
        double pv[kCgTrips], rv[kCgTrips], ov[kCgTrips], mv[kCgTrips];
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            ov[u] = omega * v[i + u * stride];
            pv[u] = p[i + u * stride];
            rv[u] = r[i + u * stride];
            if (Scaled)
                mv[u] = m[i + u * stride];
        }
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            const double d = pv[u] - ov[u];
            const double bd = beta * d;
            const double pn = rv[u] + bd;
            p[i + u * stride] = pn;
            if (Scaled)
                phat[i + u * stride] = mv[u] * pn;
        }
    }
    for (; i < n; i += stride) {
        const double ov = omega * v[i];
        const double d = p[i] - ov;
        const double bd = beta * d;
        const double pn = r[i] + bd;
        p[i] = pn;
        if (Scaled)
            phat[i] = m[i] * pn;
    }
}

using BiWork = KrylovWork<BiStatus>;  // r, p, v, t, rhat (K18: and phat, shat); the partials of six dots, the step's words, the histories

}  // namespace

int bicgstab_check_args(const char *fn, const void *h, const smvp_bicgstab_opts_t *o, const smvp_bicgstab_result_t *result, const double *d_b)
{
    return krylov_check_args(fn, "bicgstab", h, o, result, d_b);
}

int pbicgstab_check_args(const char *fn, const void *h, const smvp_bicgstab_opts_t *o, const smvp_bicgstab_result_t *result,
                         const double *d_b, const KrylovPrecond &M)
{
    if (int rc = bicgstab_check_args(fn, h, o, result, d_b))
        return rc;
    if (!M.first && !M.d_m && !M.second)
        return smvp::fail(SMVP_ERR_INVALID, "%s: first, d_m and second are all NULL: there is no preconditioner (smvp_csr_bicgstab / "
                                            "smvp_tjds_bicgstab run BiCGSTAB without one)", fn);
    return SMVP_OK;
}

int bicgstab_run(const char *fn, int device, int rows, int cols, const smvp_bicgstab_opts_t *o, const double *d_b, const double *d_x0,
                 double *d_x, const KrylovPrecond *precond, smvp_bicgstab_result_t *result, double *rr_each, double *ss_each, void *stream,
                 const HandleProduct &product)
{
    const KrylovPrecond M = precond ? *precond : KrylovPrecond{};
    if (int rc = krylov_check_operands(fn, "BiCGSTAB needs", device, rows, cols, M, d_b, d_x0, d_x))
        return rc;
    const int n = rows;
    DeviceScope on(device);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = refuse_capture(st, precond ? "preconditioned BiCGSTAB allocates and synchronises, so it cannot be captured (the stream is "
                                              "capturing)"
                                            : "BiCGSTAB allocates and synchronises, so it cannot be captured (the stream is capturing)"))
        return rc;
    smvp_bicgstab_result_t res;
    memset(&res, 0, sizeof res);
    res.reason = SMVP_BICGSTAB_CONVERGED;
    if (n == 0) {
        *result = res;
        return SMVP_OK;
    }

    BiWork w;
    w.stream = st;
    const int max_steps = o->max_steps, grid = cg_grid(n);
    const size_t pitch = krylov_pitch(n);
    if (int rc = krylov_alloc(w, fn, n, max_steps, (precond ? 7 : 5) * pitch, 6 * (size_t)kCgGridCap + kBiWords + 2 * (size_t)max_steps + 1))
        return rc;
    double *r = w.vec, *p = r + pitch, *v = p + pitch, *t = v + pitch, *rhat = t + pitch;
    double *phat = precond ? rhat + pitch : p, *shat = precond ? phat + pitch : r;  // K13: the products read p and s themselves
    double *parts_sigma = w.small, *parts_ss = parts_sigma + kCgGridCap, *parts_ts = parts_ss + kCgGridCap;
    double *parts_tt = parts_ts + kCgGridCap, *parts_rr = parts_tt + kCgGridCap, *parts_rho = parts_rr + kCgGridCap;
    double *words = parts_rho + kCgGridCap, *hist_rr = words + kBiWords, *hist_ss = hist_rr + max_steps + 1;
    const double tol2 = o->tol * o->tol;
    const dim3 g(grid), blk(kCgBlock);
    const bool fused = !M.first && M.d_m;  // the kernel that writes y writes m .* y beside it

    // step 0: x_0 into d_x, bb, r_0 = b - A x_0 (b itself without an x_0: no product), rhat = p_0 = r_0, rr_0, the first status block
    hipLaunchKernelGGL(krylov_dot_parts, g, blk, 0, st, d_b, d_b, n, parts_sigma);
    if (int rc = krylov_first_x(product, d_x0, d_x, v, n, st))
        return rc;
    if (fused)
        hipLaunchKernelGGL(bi_start<true>, g, blk, 0, st, d_b, d_x0 ? v : nullptr, r, rhat, p, M.d_m, phat, n, parts_ss);
    else
        hipLaunchKernelGGL(bi_start<false>, g, blk, 0, st, d_b, d_x0 ? v : nullptr, r, rhat, p, nullptr, nullptr, n, parts_ss);
    hipLaunchKernelGGL(bi_start_finish, dim3(1), blk, 0, st, parts_sigma, parts_ss, grid, tol2, w.st, hist_rr);
    HIP_TRY(hipGetLastError());
    BiStatus hs;
    if (int rc = krylov_look(w, fn, w.st, 0, max_steps, &hs))
        return rc;

    for (int k = 1; !hs.stopped; ++k) {
        const BiStatus *prev = w.st + ((k - 1) & 1);
        BiStatus *cur = w.st + (k & 1);
        if (int rc = krylov_apply(fn, M, p, phat, n, st))
            return rc;
        if (int rc = product(phat, v))
            return rc;
        hipLaunchKernelGGL(bi_sigma_parts, g, blk, 0, st, rhat, v, n, prev, parts_sigma);
        if (fused)
            hipLaunchKernelGGL(bi_half<true>, g, blk, 0, st, v, r, M.d_m, shat, n, grid, parts_sigma, prev, words, parts_ss);
        else
            hipLaunchKernelGGL(bi_half<false>, g, blk, 0, st, v, r, nullptr, nullptr, n, grid, parts_sigma, prev, words, parts_ss);
        if (int rc = krylov_apply(fn, M, r, shat, n, st))  // r holds s
            return rc;
        if (int rc = product(shat, t))
            return rc;
        hipLaunchKernelGGL(bi_t_parts, g, blk, 0, st, t, r, n, prev, words, parts_ts, parts_tt);
        if (precond)
            hipLaunchKernelGGL(bi_full<true>, g, blk, 0, st, d_x, phat, shat, r, t, rhat, n, grid, parts_ss, parts_ts, parts_tt, prev, words,
                               parts_rr, parts_rho);
        else
            hipLaunchKernelGGL(bi_full<false>, g, blk, 0, st, d_x, p, nullptr, r, t, rhat, n, grid, parts_ss, parts_ts, parts_tt, prev, words,
                               parts_rr, parts_rho);
        if (fused)
            hipLaunchKernelGGL(bi_direction<true>, g, blk, 0, st, p, r, v, M.d_m, phat, n, grid, parts_rr, parts_rho, words, prev, cur, k,
                               max_steps, hist_rr, hist_ss);
        else
            hipLaunchKernelGGL(bi_direction<false>, g, blk, 0, st, p, r, v, nullptr, nullptr, n, grid, parts_rr, parts_rho, words, prev, cur,
                               k, max_steps, hist_rr, hist_ss);
        HIP_TRY(hipGetLastError());
        if (k % o->check_every == 0 || k == max_steps)
            if (int rc = krylov_look(w, fn, cur, k, max_steps, &hs))
                return rc;
    }
    if (int rc = krylov_history(rr_each, hist_rr, hs.full + 1))
        return rc;
    if (int rc = krylov_history(ss_each, hist_ss, hs.nss))
        return rc;
    res.steps = hs.steps;
    res.full = hs.full;
    res.half = hs.half;
    res.reason = hs.reason;
    res.rr = hs.rr;
    res.bb = hs.bb;
    *result = res;
    return SMVP_OK;
}

}  // namespace smvp

extern "C" void smvp_bicgstab_opts_default(smvp_bicgstab_opts_t *o)
{
    if (!o)
        return;
    memset(o, 0, sizeof *o);
    o->struct_size = (unsigned)sizeof *o;
    o->max_steps = 100;
    o->check_every = 10;
    o->tol = 1e-10;
}
