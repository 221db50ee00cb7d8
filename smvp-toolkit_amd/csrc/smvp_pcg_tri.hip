// smvp_pcg_tri.hip -- K16: conjugate gradients on a handle's own product, preconditioned with M = T1 diag(m)^-1 T2 where T1 and T2
// are two of K15's triangular-solve plans the caller brings (smvp_csr_pcg_tri, smvp_tjds_pcg_tri), to the bits include/smvp_amd.h
// defines.  New: the reference only ever multiplies.  The dot, its folds, the grid rule and the workspace holder are K12's
// (smvp_cg_common.h); the rules, their order and the launch discipline are K14's (smvp_pcg.hip); the solves are K15's kernels,
// enqueued through smvp::trsv_enqueue, the entry smvp_trsv_solve itself goes through.
//
// z = M^-1 r is  w = T1^-1 r;  v_i = m_i * w_i (skipped without an m);  z = T2^-1 v, the second solve in place.  It cannot be
// re-derived element by element the way K14 divides r_i by m_i again, so it is stored: four vectors r, p, q, z.  A step k has
// p_{k-1}, r_{k-1}, x_{k-1} in the caller's d_x, rho_{k-1} in the status block and q_k = A p_{k-1} (the handle's own launch).  Beside
// the product and the two solves' launches a step is five launches of the dot's grid (four without an m), fifteen vector passes:
//
//   tri_dot_parts   the partials of sigma_k = dot(p, q)                                                       (p, q read)
//   tri_residual    every workgroup folds those partials itself and so holds the same sigma_k and alpha_k = rho_{k-1} / sigma_k;
//                   r -= alpha q and the partials of rr_k = dot(r, r) in the same pass (q, r read, r written).  Workgroup 0 leaves
//                   sigma_k in a word of its own for tri_direction;
//   (first's solve: r -> z)
//   tri_scale       z_i = m_i * z_i                                                                         (z, m read, z written)
//   (second's solve: z -> z)
//   tri_dot_parts   the partials of rho_k = dot(r, z)                                                         (r, z read)
//   tri_direction   every workgroup folds the partials of rr_k and rho_k, forms beta_k and the stop rules itself; x += alpha p and,
//                   unless the run stops here, p = z + beta p (x, p, z read, x, p written).  Workgroup 0 writes the step's status
//                   block and the three history elements.
//
// No launch reads a word that another lane of the same launch writes, and every hand-off between workgroups is a launch boundary
// (K15's kernels keep that rule for themselves: a chain's levels meet at __syncthreads() of its one workgroup).  NO KERNEL WAITS ON
// A VALUE ANOTHER WORKGROUP WRITES.  The status block is ping-ponged by step parity because tri_direction reads step k - 1's while
// its workgroup 0 writes step k's.  No atomics.  The device evaluates the stop rules at every step.  Once one has fired,
// tri_residual and tri_direction of every later step see `stopped`, write nothing to x, r, p or the histories, and carry the block
// over; the solves and tri_scale of such a step only rewrite z from an r that no longer changes.  Every operation on an element is
// one rounded IEEE operation (-ffp-contract=off, as everywhere).
#include "smvp_cg_common.h"
#include "smvp_engine.h"
#include "smvp_kernels.h"

#include <cmath>
#include <cstring>
#include <limits>

namespace smvp {

namespace {

// what a step leaves behind for the next step's lanes and, at a looked step, for the host (K14's block)
struct TriStatus {
    double rho;   // rho_updates = dot(r, z) of the last update
    double rr;    // dot(r, r) of the last update: what the stop rule looks at
    double bb;    // dot(b, b)
    double thr;   // (tol * tol) * bb
    int stopped;  // a rule has fired: reason, steps and updates are final
    int reason;   // SMVP_CG_*
    int steps;    // products done
    int updates;  // updates of x done
};

__global__ __launch_bounds__(kCgBlock) void tri_dot_parts(const double *__restrict__ a, const double *__restrict__ b, int n,
                                                          double *__restrict__ parts)
{
    const double c = cg_fold256(cg_lane_dot(a, b, n));
    if (threadIdx.x == 0)
        parts[blockIdx.x] = c;
}

// r_0 = b - q (q = A x_0), or b itself without a q; the partials of rr_0 = dot(r_0, r_0)
__global__ __launch_bounds__(kCgBlock) void tri_start(const double *__restrict__ b, const double *__restrict__ q, double *__restrict__ r, int n,
                                                      double *__restrict__ parts_rr)
{
    const long long stride = (long long)gridDim.x * kCgBlock;
    double c = 0.0;
    for (long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x; i < n; i += stride) {
        const double v = q ? b[i] - q[i] : b[i];
        r[i] = v;
        const double t = v * v;
        c = c + t;
    }
    c = cg_fold256(c);
    if (threadIdx.x == 0)
        parts_rr[blockIdx.x] = c;
}

// p_0 = z_0 and the partials of rho_0 = dot(r_0, z_0)
__global__ __launch_bounds__(kCgBlock) void tri_start_direction(const double *__restrict__ r, const double *__restrict__ z, double *__restrict__ p,
                                                                int n, double *__restrict__ parts_rz)
{
    const long long stride = (long long)gridDim.x * kCgBlock;
    double e = 0.0;
    for (long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x; i < n; i += stride) {
        const double zv = z[i];
        p[i] = zv;
        const double s = r[i] * zv;
        e = e + s;
    }
    e = cg_fold256(e);
    if (threadIdx.x == 0)
        parts_rz[blockIdx.x] = e;
}

// one workgroup: bb, rr_0, rho_0, the threshold and step 0's rule into status block 0, rr_0 and rho_0 into the histories
__global__ __launch_bounds__(kCgBlock) void tri_start_finish(const double *__restrict__ parts_bb, const double *__restrict__ parts_rr,
                                                             const double *__restrict__ parts_rz, int nparts, double tol2,
                                                             TriStatus *__restrict__ st, double *__restrict__ hist_rr,
                                                             double *__restrict__ hist_rz)
{
    const double bb = cg_fold_parts(parts_bb, nparts);
    const double rr = cg_fold_parts(parts_rr, nparts);
    const double rho = cg_fold_parts(parts_rz, nparts);
    if (threadIdx.x != 0)
        return;
    TriStatus s;
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

// step k: prev = the status of step k - 1, parts_pq = the partials of dot(p, q).  r -= alpha q with the partials of dot(r, r).
__global__ __launch_bounds__(kCgBlock) void tri_residual(const double *__restrict__ q, double *__restrict__ r, int n, int nparts,
                                                         const double *__restrict__ parts_pq, const TriStatus *__restrict__ prev,
                                                         double *__restrict__ sigma_out, double *__restrict__ parts_rr)
{
    if (prev->stopped)
        return;
    const double sigma = cg_fold_parts(parts_pq, nparts);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        *sigma_out = sigma;
    if (!cg_finite(sigma) || !(sigma > 0.0))
        return;  // rule A: tri_direction reports it
    const double alpha = prev->rho / sigma;
    const long long stride = (long long)gridDim.x * kCgBlock;
    long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x;
    double c = 0.0;
    for (; i + (kCgTrips - 1) * stride < n; i += kCgTrips * stride) {
        double v[kCgTrips], aq[kCgTrips];
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            aq[u] = alpha * q[i + u * stride];  // rounded, then the difference is rounded
            v[u] = r[i + u * stride];
        }
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            v[u] = v[u] - aq[u];
            r[i + u * stride] = v[u];
            const double t = v[u] * v[u];
            c = c + t;
        }
    }
    for (; i < n; i += stride) {
        const double aq = alpha * q[i];
        const double v = r[i] - aq;
        r[i] = v;
        const double t = v * v;
        c = c + t;
    }
    c = cg_fold256(c);
    if (threadIdx.x == 0)
        parts_rr[blockIdx.x] = c;
}

// v_i = m_i * w_i between the two solves, in place: one rounded multiplication
__global__ __launch_bounds__(kCgBlock) void tri_scale(double *__restrict__ z, const double *__restrict__ m, int n)
{
    const long long stride = (long long)gridDim.x * kCgBlock;
    long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x;
    for (; i + (kCgTrips - 1) * stride < n; i += kCgTrips * stride) {
        double zv[kCgTrips], mv[kCgTrips];
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            zv[u] = z[i + u * stride];
            mv[u] = m[i + u * stride];
        }
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u)
            z[i + u * stride] = mv[u] * zv[u];
    }
    for (; i < n; i += stride)
        z[i] = m[i] * z[i];
}

// step k: x += alpha p; rule B; p = z + beta p unless the run stops here.  Workgroup 0 writes status block k and the histories.
__global__ __launch_bounds__(kCgBlock) void tri_direction(double *__restrict__ x, double *__restrict__ p, const double *__restrict__ z, int n,
                                                          int nparts, const double *__restrict__ parts_rr, const double *__restrict__ parts_rz,
                                                          const double *__restrict__ sigma_in, const TriStatus *__restrict__ prev,
                                                          TriStatus *__restrict__ cur, int step, int max_steps, double *__restrict__ hist_rr,
                                                          double *__restrict__ hist_rz, double *__restrict__ hist_sigma)
{
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    TriStatus s = *prev;
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
            double pv[kCgTrips], xv[kCgTrips], zv[kCgTrips];
#pragma unroll
            for (int u = 0; u < kCgTrips; ++u) {
                pv[u] = p[i + u * stride];
                xv[u] = x[i + u * stride];
                zv[u] = z[i + u * stride];
            }
#pragma unroll
            for (int u = 0; u < kCgTrips; ++u) {
                const double ap = alpha * pv[u], bp = beta * pv[u];
                x[i + u * stride] = xv[u] + ap;
                p[i + u * stride] = zv[u] + bp;
            }
        }
        for (; i < n; i += stride) {
            const double pv = p[i];
            const double ap = alpha * pv, bp = beta * pv;
            x[i] = x[i] + ap;
            p[i] = z[i] + bp;
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

using TriWork = KrylovWork<TriStatus>;  // r, p, q, z; the partials of three dots, sigma's word, the histories

}  // namespace

int pcg_tri_check_args(const char *fn, const void *h, const smvp_cg_opts_t *o, const smvp_pcg_result_t *result, const double *d_b,
                       const smvp_trsv_t *first, const smvp_trsv_t *second)
{
    // K14's checks; d_m may be NULL here, so d_b stands in for it (a null d_b is named first)
    if (int rc = pcg_check_args(fn, h, o, result, d_b, d_b))
        return rc;
    if (!first || !second)
        return smvp::fail(SMVP_ERR_INVALID, "%s: null %s plan", fn, !first ? "first" : "second");
    return SMVP_OK;
}

int pcg_tri_run(const char *fn, int device, int rows, int cols, const smvp_cg_opts_t *o, const double *d_b, const double *d_x0, double *d_x,
                smvp_trsv_t *first, const double *d_m, smvp_trsv_t *second, smvp_pcg_result_t *result, double *rr_each, double *rz_each,
                double *sigma_each, void *stream, const HandleProduct &product)
{
    if (rows != cols)
        return smvp::fail(SMVP_ERR_INVALID, "%s: conjugate gradients need a square matrix (%d x %d given)", fn, rows, cols);
    const int n = rows;
    for (const smvp_trsv_t *t : {(const smvp_trsv_t *)first, (const smvp_trsv_t *)second}) {
        const char *which = t == first ? "first" : "second";
        if (trsv_rows(t) != n)
            return smvp::fail(SMVP_ERR_INVALID, "%s: the %s plan solves %d rows, the handle has %d", fn, which, trsv_rows(t), n);
        if (trsv_device(t) != device)
            return smvp::fail(SMVP_ERR_INVALID, "%s: the %s plan lives on device %d, the handle on device %d", fn, which, trsv_device(t), device);
    }
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
    if (int rc = refuse_capture(st, "conjugate gradients preconditioned by triangular solves allocate and synchronise, so they cannot be "
                                    "captured (the stream is capturing)"))
        return rc;
    smvp_pcg_result_t res;
    memset(&res, 0, sizeof res);
    res.reason = SMVP_CG_CONVERGED;
    if (n == 0) {
        *result = res;
        return SMVP_OK;
    }

    TriWork w;
    w.stream = st;
    const int max_steps = o->max_steps, grid = cg_grid(n);
    const size_t small_doubles = 3 * (size_t)kCgGridCap + 1 + 3 * (size_t)max_steps + 2;
    const size_t pitch = ((size_t)n + 31) / 32 * 32;  // every vector on a 256-byte boundary, as vectors of their own would be
    if (hipMalloc((void **)&w.vec, sizeof(double) * 4 * pitch) != hipSuccess ||
        hipMalloc((void **)&w.small, sizeof(double) * small_doubles) != hipSuccess ||
        hipMalloc((void **)&w.st, 2 * sizeof(TriStatus)) != hipSuccess || hipHostMalloc((void **)&w.seen, sizeof(TriStatus)) != hipSuccess) {
        (void)hipGetLastError();
        return smvp::fail(SMVP_ERR_ALLOC, "%s: cannot allocate the workspace (%d elements, %d steps)", fn, n, max_steps);
    }
    double *r = w.vec, *p = r + pitch, *q = p + pitch, *z = q + pitch;
    double *parts_a = w.small, *parts_b = parts_a + kCgGridCap, *parts_c = parts_b + kCgGridCap, *sigma = parts_c + kCgGridCap;
    double *hist_rr = sigma + 1, *hist_rz = hist_rr + max_steps + 1, *hist_sigma = hist_rz + max_steps + 1;
    const double tol2 = o->tol * o->tol;

    // z = M^-1 r: first's solve out of r into z, the multiplication by m, second's solve in place
    auto apply = [&]() -> int {
        if (int rc = trsv_enqueue(fn, first, r, z, st))
            return rc;
        if (d_m)
            hipLaunchKernelGGL(tri_scale, dim3(grid), dim3(kCgBlock), 0, st, z, d_m, n);
        return trsv_enqueue(fn, second, z, z, st);
    };

    // step 0: x_0 into d_x, bb, r_0 = b - A x_0 (b itself without an x_0: no product), z_0 = M^-1 r_0, p_0 = z_0, rr_0, rho_0, the
    // first status block
    hipLaunchKernelGGL(tri_dot_parts, dim3(grid), dim3(kCgBlock), 0, st, d_b, d_b, n, parts_a);
    if (d_x0) {
        if (d_x0 != d_x)
            HIP_TRY(hipMemcpyAsync(d_x, d_x0, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
        if (int rc = product(d_x, q))
            return rc;
    } else {
        HIP_TRY(hipMemsetAsync(d_x, 0, sizeof(double) * (size_t)n, st));
    }
    hipLaunchKernelGGL(tri_start, dim3(grid), dim3(kCgBlock), 0, st, d_b, d_x0 ? q : nullptr, r, n, parts_b);
    if (int rc = apply())
        return rc;
    hipLaunchKernelGGL(tri_start_direction, dim3(grid), dim3(kCgBlock), 0, st, r, z, p, n, parts_c);
    hipLaunchKernelGGL(tri_start_finish, dim3(1), dim3(kCgBlock), 0, st, parts_a, parts_b, parts_c, grid, tol2, w.st, hist_rr, hist_rz);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(w.seen, w.st, sizeof(TriStatus), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    TriStatus hs = *w.seen;

    for (int k = 1; !hs.stopped; ++k) {
        const TriStatus *prev = w.st + ((k - 1) & 1);
        TriStatus *cur = w.st + (k & 1);
        if (int rc = product(p, q))
            return rc;
        hipLaunchKernelGGL(tri_dot_parts, dim3(grid), dim3(kCgBlock), 0, st, p, q, n, parts_a);
        hipLaunchKernelGGL(tri_residual, dim3(grid), dim3(kCgBlock), 0, st, q, r, n, grid, parts_a, prev, sigma, parts_b);
        if (int rc = apply())
            return rc;
        hipLaunchKernelGGL(tri_dot_parts, dim3(grid), dim3(kCgBlock), 0, st, r, z, n, parts_c);
        hipLaunchKernelGGL(tri_direction, dim3(grid), dim3(kCgBlock), 0, st, d_x, p, z, n, grid, parts_b, parts_c, sigma, prev, cur, k,
                           max_steps, hist_rr, hist_rz, hist_sigma);
        HIP_TRY(hipGetLastError());
        if (k % o->check_every == 0 || k == max_steps) {  // a looked step: the status block, nothing else, and only to leave the loop
            HIP_TRY(hipMemcpyAsync(w.seen, cur, sizeof(TriStatus), hipMemcpyDeviceToHost, st));
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
