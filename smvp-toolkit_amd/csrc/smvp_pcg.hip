// smvp_pcg.hip -- K14: conjugate gradients with a diagonal preconditioner M on a handle's own product (smvp_csr_pcg,
// smvp_tjds_pcg), to the bits include/smvp_amd.h defines.  New: the reference only ever multiplies.  The dot, its folds, the grid
// rule and the workspace holder are K12's (smvp_cg_common.h); the launch discipline is K12's too.
//
// A step k has the direction p_{k-1}, the residual r_{k-1}, x_{k-1} in the caller's d_x, rho_{k-1} = dot(r_{k-1}, z_{k-1}) in the
// status block and q_k = A p_{k-1} (the handle's own launch, whatever its plan).  z = r ./ m is never stored: a launch that needs
// z_i divides r_i by m_i again -- an IEEE division, the same bits -- which costs one read of m where a stored z would cost a write
// and a read.  Beside the product a step is three launches of the dot's grid over the vectors, twelve vector passes:
//
//   pcg_dot_parts   the partials of sigma_k = dot(p, q)                                                      (p, q read)
//   pcg_residual    every workgroup folds those partials itself and so holds the same sigma_k and alpha_k = rho_{k-1} / sigma_k;
//                   r -= alpha q, and the partials of rr_k = dot(r, r) and rho_k = dot(r, r ./ m) in the same pass: two
//                   accumulators per lane, each in the dot's own order (q, r, m read, r written).  Workgroup 0 leaves sigma_k in
//                   a word of its own for the next launch;
//   pcg_direction   every workgroup folds the partials of rr_k and rho_k, forms beta_k and the stop rules itself; x += alpha p and,
//                   unless the run stops here, p = r ./ m + beta p (x, p, r, m read, x, p written).  Workgroup 0 writes the step's
//                   status block and the three history elements.
//
// No launch reads a word that another lane of the same launch writes, and every hand-off between workgroups is a launch boundary:
// the partials, sigma's word and the status block are written by one launch and read by later ones; the status block is
// ping-ponged by step parity because pcg_direction reads step k - 1's while its workgroup 0 writes step k's.  No atomics.  The
// device evaluates the stop rules at every step.  Once one has fired, pcg_residual and pcg_direction of every later step see
// `stopped` in the status block, write nothing to x, r, p or the histories, and carry the block over; the host reads the block at
// looked steps only, and only to leave the loop.  Every operation on an element is one rounded IEEE operation
// (-ffp-contract=off, as everywhere; r_i / m_i is a division, no reciprocal is taken).
#include "smvp_cg_common.h"
#include "smvp_engine.h"
#include "smvp_kernels.h"

#include <cmath>
#include <cstring>
#include <limits>

namespace smvp {

namespace {

// what a step leaves behind for the next step's lanes and, at a looked step, for the host
struct PcgStatus {
    double rho;   // rho_updates = dot(r, z) of the last update
    double rr;    // dot(r, r) of the last update: what the stop rule looks at
    double bb;    // dot(b, b)
    double thr;   // (tol * tol) * bb
    int stopped;  // a rule has fired: reason, steps and updates are final
    int reason;   // SMVP_CG_*
    int steps;    // products done
    int updates;  // updates of x done
};

__global__ __launch_bounds__(kCgBlock) void pcg_dot_parts(const double *__restrict__ a, const double *__restrict__ b, int n,
                                                          double *__restrict__ parts)
{
    const double c = cg_fold256(cg_lane_dot(a, b, n));
    if (threadIdx.x == 0)
        parts[blockIdx.x] = c;
}

// r_0 = b - q (q = A x_0), or b itself without a q; p_0 = z_0 = r_0 ./ m; the partials of rr_0 = dot(r_0, r_0) and rho_0 = dot(r_0, z_0)
__global__ __launch_bounds__(kCgBlock) void pcg_start(const double *__restrict__ b, const double *__restrict__ q, const double *__restrict__ m,
                                                      double *__restrict__ r, double *__restrict__ p, int n, double *__restrict__ parts_rr,
                                                      double *__restrict__ parts_rz)
{
    const long long stride = (long long)gridDim.x * kCgBlock;
    double c = 0.0, e = 0.0;
    for (long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x; i < n; i += stride) {
        const double v = q ? b[i] - q[i] : b[i];
        const double z = v / m[i];
        r[i] = v;
        p[i] = z;
        const double t = v * v, s = v * z;
        c = c + t;
        e = e + s;
    }
    c = cg_fold256(c);
    e = cg_fold256(e);
    if (threadIdx.x == 0) {
        parts_rr[blockIdx.x] = c;
        parts_rz[blockIdx.x] = e;
    }
}

// one workgroup: bb, rr_0, rho_0, the threshold and step 0's rule into status block 0, rr_0 and rho_0 into the histories
__global__ __launch_bounds__(kCgBlock) void pcg_start_finish(const double *__restrict__ parts_bb, const double *__restrict__ parts_rr,
                                                             const double *__restrict__ parts_rz, int nparts, double tol2,
                                                             PcgStatus *__restrict__ st, double *__restrict__ hist_rr,
                                                             double *__restrict__ hist_rz)
{
    const double bb = cg_fold_parts(parts_bb, nparts);
    const double rr = cg_fold_parts(parts_rr, nparts);
    const double rho = cg_fold_parts(parts_rz, nparts);
    if (threadIdx.x != 0)
        return;
    PcgStatus s;
    s.rho = rho;
    s.rr = rr;
    s.bb = bb;
    s.thr = tol2 * bb;
    const bool bad = !cg_finite(bb) || !cg_finite(rr) || !cg_finite(rho);
    s.stopped = bad || rr <= s.thr || !(rho > 0.0);
    s.reason = bad ? SMVP_CG_NONFINITE : rr <= s.thr ? SMVP_CG_CONVERGED : SMVP_CG_BREAKDOWN;
    s.steps = 0;
    s.updates = 0;
    st[0] = s;
    hist_rr[0] = rr;
    hist_rz[0] = rho;
}

// step k: prev = the status of step k - 1, parts_pq = the partials of dot(p, q).  r -= alpha q with the partials of dot(r, r) and
// dot(r, r ./ m).
__global__ __launch_bounds__(kCgBlock) void pcg_residual(const double *__restrict__ q, const double *__restrict__ m, double *__restrict__ r,
                                                         int n, int nparts, const double *__restrict__ parts_pq,
                                                         const PcgStatus *__restrict__ prev, double *__restrict__ sigma_out,
                                                         double *__restrict__ parts_rr, double *__restrict__ parts_rz)
{
    if (prev->stopped)
        return;
    const double sigma = cg_fold_parts(parts_pq, nparts);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        *sigma_out = sigma;
    if (!cg_finite(sigma) || !(sigma > 0.0))
        return;  // rule A: pcg_direction reports it
    const double alpha = prev->rho / sigma;
    const long long stride = (long long)gridDim.x * kCgBlock;
    long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x;
    double c = 0.0, e = 0.0;
    for (; i + (kCgTrips - 1) * stride < n; i += kCgTrips * stride) {
        double v[kCgTrips], aq[kCgTrips], mv[kCgTrips];
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            aq[u] = alpha * q[i + u * stride];  // rounded, then the difference is rounded
            v[u] = r[i + u * stride];
            mv[u] = m[i + u * stride];
        }
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            v[u] = v[u] - aq[u];
            r[i + u * stride] = v[u];
            const double z = v[u] / mv[u];
            const double t = v[u] * v[u], s = v[u] * z;
            c = c + t;
            e = e + s;
        }
    }
    for (; i < n; i += stride) {
        const double aq = alpha * q[i];
        const double v = r[i] - aq;
        r[i] = v;
        const double z = v / m[i];
        const double t = v * v, s = v * z;
        c = c + t;
        e = e + s;
    }
    c = cg_fold256(c);
    e = cg_fold256(e);
    if (threadIdx.x == 0) {
        parts_rr[blockIdx.x] = c;
        parts_rz[blockIdx.x] = e;
    }
}

// step k: x += alpha p; rule B; p = r ./ m + beta p unless the run stops here.  Workgroup 0 writes status block k and the histories.
__global__ __launch_bounds__(kCgBlock) void pcg_direction(double *__restrict__ x, double *__restrict__ p, const double *__restrict__ r,
                                                          const double *__restrict__ m, int n, int nparts,
                                                          const double *__restrict__ parts_rr, const double *__restrict__ parts_rz,
                                                          const double *__restrict__ sigma_in, const PcgStatus *__restrict__ prev,
                                                          PcgStatus *__restrict__ cur, int step, int max_steps, double *__restrict__ hist_rr,
                                                          double *__restrict__ hist_rz, double *__restrict__ hist_sigma)
{
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    PcgStatus s = *prev;
    if (s.stopped) {
        if (first)
            *cur = s;
        return;
    }
    const double sigma = *sigma_in;
    s.steps = step;
    if (!cg_finite(sigma) || !(sigma > 0.0)) {  // rule A: x stays x_{k-1}
        if (first) {
            s.stopped = 1;
            s.reason = cg_finite(sigma) ? SMVP_CG_BREAKDOWN : SMVP_CG_NONFINITE;
            *cur = s;
            hist_sigma[step - 1] = sigma;
        }
        return;
    }
    const double alpha = s.rho / sigma;
    const double rr = cg_fold_parts(parts_rr, nparts);
    const double rho = cg_fold_parts(parts_rz, nparts);
    const bool bad = !cg_finite(rr) || !cg_finite(rho);
    const bool stop = bad || rr <= s.thr || !(rho > 0.0) || step == max_steps;
    const double beta = rho / s.rho;
    const long long stride = (long long)gridDim.x * kCgBlock;
    long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x;
    if (stop) {
        for (; i < n; i += stride) {
            const double ap = alpha * p[i];
            x[i] = x[i] + ap;
        }
    } else {
        for (; i + (kCgTrips - 1) * stride < n; i += kCgTrips * stride) {
            double pv[kCgTrips], xv[kCgTrips], rv[kCgTrips], mv[kCgTrips];
#pragma unroll
            for (int u = 0; u < kCgTrips; ++u) {
                pv[u] = p[i + u * stride];
                xv[u] = x[i + u * stride];
                rv[u] = r[i + u * stride];
                mv[u] = m[i + u * stride];
            }
#pragma unroll
            for (int u = 0; u < kCgTrips; ++u) {
                const double ap = alpha * pv[u], bp = beta * pv[u];
                const double z = rv[u] / mv[u];
                x[i + u * stride] = xv[u] + ap;
                p[i + u * stride] = z + bp;
            }
        }
        for (; i < n; i += stride) {
            const double pv = p[i];
            const double ap = alpha * pv, bp = beta * pv;
            const double z = r[i] / m[i];
            x[i] = x[i] + ap;
            p[i] = z + bp;
        }
    }
    if (first) {
        s.rho = rho;
        s.rr = rr;
        s.updates = step;
        s.stopped = stop;
        s.reason = bad ? SMVP_CG_NONFINITE : rr <= s.thr ? SMVP_CG_CONVERGED : !(rho > 0.0) ? SMVP_CG_BREAKDOWN : SMVP_CG_MAX_STEPS;
        *cur = s;
        hist_sigma[step - 1] = sigma;
        hist_rr[step] = rr;
        hist_rz[step] = rho;
    }
}

using PcgWork = KrylovWork<PcgStatus>;  // r, p, q; the partials of three dots, sigma's word, the histories

}  // namespace

int pcg_check_args(const char *fn, const void *h, const smvp_cg_opts_t *o, const smvp_pcg_result_t *result, const double *d_b,
                   const double *d_m)
{
    if (!h || !o || !result || !d_b || !d_m)
        return smvp::fail(SMVP_ERR_INVALID, "%s: null %s", fn, !h ? "handle" : !o ? "opts" : !result ? "result" : !d_b ? "d_b" : "d_m");
    if (o->struct_size != (unsigned)sizeof(smvp_cg_opts_t))
        return smvp::fail(SMVP_ERR_INVALID, "%s: smvp_cg_opts_t of %u bytes, this library's has %u: initialise it with "
                                            "smvp_cg_opts_default and build against this library's header",
                          fn, o->struct_size, (unsigned)sizeof(smvp_cg_opts_t));
    if (o->max_steps < 1 || o->check_every < 1 || !(o->tol >= 0.0) || !(o->tol <= std::numeric_limits<double>::max()))
        return smvp::fail(SMVP_ERR_INVALID, "%s: max_steps = %d, check_every = %d, tol = %g (need max_steps >= 1, check_every >= 1, "
                                            "tol >= 0 and finite)", fn, o->max_steps, o->check_every, o->tol);
    return SMVP_OK;
}

int pcg_run(const char *fn, int device, int rows, int cols, const smvp_cg_opts_t *o, const double *d_b, const double *d_x0, double *d_x,
            const double *d_m, smvp_pcg_result_t *result, double *rr_each, double *rz_each, double *sigma_each, void *stream,
            const HandleProduct &product)
{
    if (rows != cols)
        return smvp::fail(SMVP_ERR_INVALID, "%s: conjugate gradients need a square matrix (%d x %d given)", fn, rows, cols);
    const int n = rows;
    if (n > 0 && !d_x)
        return smvp::fail(SMVP_ERR_INVALID, "%s: null d_x", fn);
    if (d_x0 != d_x && operands_overlap(d_x0, 1, n, d_x, 1, n, 1))
        return smvp::fail(SMVP_ERR_INVALID, "%s: d_x0 and d_x overlap without being the same vector", fn);
    if (operands_overlap(d_b, 1, n, d_x, 1, n, 1))
        return smvp::fail(SMVP_ERR_INVALID, "%s: d_b and d_x overlap", fn);
    if (operands_overlap(d_m, 1, n, d_x, 1, n, 1))
        return smvp::fail(SMVP_ERR_INVALID, "%s: d_m and d_x overlap", fn);
    DeviceScope on(device);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = refuse_capture(st, "preconditioned conjugate gradients allocate and synchronise, so they cannot be captured (the stream is "
                                    "capturing)"))
        return rc;
    smvp_pcg_result_t res;
    memset(&res, 0, sizeof res);
    res.reason = SMVP_CG_CONVERGED;
    if (n == 0) {
        *result = res;
        return SMVP_OK;
    }

    PcgWork w;
    w.stream = st;
    const int max_steps = o->max_steps, grid = cg_grid(n);
    const size_t small_doubles = 3 * (size_t)kCgGridCap + 1 + 3 * (size_t)max_steps + 2;
    const size_t pitch = ((size_t)n + 31) / 32 * 32;  // every vector on a 256-byte boundary, as vectors of their own would be
    if (hipMalloc((void **)&w.vec, sizeof(double) * 3 * pitch) != hipSuccess ||
        hipMalloc((void **)&w.small, sizeof(double) * small_doubles) != hipSuccess ||
        hipMalloc((void **)&w.st, 2 * sizeof(PcgStatus)) != hipSuccess || hipHostMalloc((void **)&w.seen, sizeof(PcgStatus)) != hipSuccess) {
        (void)hipGetLastError();
        return smvp::fail(SMVP_ERR_ALLOC, "%s: cannot allocate the workspace (%d elements, %d steps)", fn, n, max_steps);
    }
    double *r = w.vec, *p = r + pitch, *q = p + pitch;
    double *parts_a = w.small, *parts_b = parts_a + kCgGridCap, *parts_c = parts_b + kCgGridCap, *sigma = parts_c + kCgGridCap;
    double *hist_rr = sigma + 1, *hist_rz = hist_rr + max_steps + 1, *hist_sigma = hist_rz + max_steps + 1;
    const double tol2 = o->tol * o->tol;

    // step 0: x_0 into d_x, bb, r_0 = b - A x_0 (b itself without an x_0: no product), p_0 = z_0 = r_0 ./ m, rr_0, rho_0, the first
    // status block
    hipLaunchKernelGGL(pcg_dot_parts, dim3(grid), dim3(kCgBlock), 0, st, d_b, d_b, n, parts_a);
    if (d_x0) {
        if (d_x0 != d_x)
            HIP_TRY(hipMemcpyAsync(d_x, d_x0, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
        if (int rc = product(d_x, q))
            return rc;
    } else {
        HIP_TRY(hipMemsetAsync(d_x, 0, sizeof(double) * (size_t)n, st));
    }
    hipLaunchKernelGGL(pcg_start, dim3(grid), dim3(kCgBlock), 0, st, d_b, d_x0 ? q : nullptr, d_m, r, p, n, parts_b, parts_c);
    hipLaunchKernelGGL(pcg_start_finish, dim3(1), dim3(kCgBlock), 0, st, parts_a, parts_b, parts_c, grid, tol2, w.st, hist_rr, hist_rz);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(w.seen, w.st, sizeof(PcgStatus), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    PcgStatus hs = *w.seen;

    for (int k = 1; !hs.stopped; ++k) {
        const PcgStatus *prev = w.st + ((k - 1) & 1);
        PcgStatus *cur = w.st + (k & 1);
        if (int rc = product(p, q))
            return rc;
        hipLaunchKernelGGL(pcg_dot_parts, dim3(grid), dim3(kCgBlock), 0, st, p, q, n, parts_a);
        hipLaunchKernelGGL(pcg_residual, dim3(grid), dim3(kCgBlock), 0, st, q, d_m, r, n, grid, parts_a, prev, sigma, parts_b, parts_c);
        hipLaunchKernelGGL(pcg_direction, dim3(grid), dim3(kCgBlock), 0, st, d_x, p, r, d_m, n, grid, parts_b, parts_c, sigma, prev, cur, k,
                           max_steps, hist_rr, hist_rz, hist_sigma);
        HIP_TRY(hipGetLastError());
        if (k % o->check_every == 0 || k == max_steps) {  // a looked step: the status block, nothing else, and only to leave the loop
            HIP_TRY(hipMemcpyAsync(w.seen, cur, sizeof(PcgStatus), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            hs = *w.seen;
            if (k == max_steps && !hs.stopped)
                return smvp::fail(SMVP_ERR_HIP, "%s: the device did not stop at max_steps = %d", fn, max_steps);
        }
    }
    if (rr_each)
        HIP_TRY(hipMemcpy(rr_each, hist_rr, sizeof(double) * ((size_t)hs.updates + 1), hipMemcpyDeviceToHost));
    if (rz_each)
        HIP_TRY(hipMemcpy(rz_each, hist_rz, sizeof(double) * ((size_t)hs.updates + 1), hipMemcpyDeviceToHost));
    if (sigma_each && hs.steps > 0)
        HIP_TRY(hipMemcpy(sigma_each, hist_sigma, sizeof(double) * (size_t)hs.steps, hipMemcpyDeviceToHost));
    res.steps = hs.steps;
    res.updates = hs.updates;
    res.reason = hs.reason;
    res.rr = hs.rr;
    res.rz = hs.rho;
    res.bb = hs.bb;
    *result = res;
    return SMVP_OK;
}

}  // namespace smvp
