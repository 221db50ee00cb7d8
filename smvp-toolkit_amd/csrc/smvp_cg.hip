// smvp_cg.hip -- K12: conjugate gradients on a handle's own product (smvp_csr_cg, smvp_tjds_cg) and the dot product whose order
// of additions include/smvp_amd.h defines (smvp_vector_dot).  New: the reference only ever multiplies.
//
// The dot.  G = min(ceil(n / 256), 2048) workgroups of 256 lanes.  Lane l of workgroup g owns slot s = 256 g + l and adds the
// rounded terms t_s, t_{s + 256 G}, ... in ascending order to an accumulator that starts at +0.0 (eight trips are loaded before
// the first is added; they are added in that order).  fold256 -- a __shfl_xor butterfly inside each wavefront, then
// ((w0 + w1) + w2) + w3 through LDS -- gives the workgroup's partial, and the same fold over a second level (lane l adds the
// partials l, l + 256, ... in ascending order) gives the dot.  No atomics: the order is part of the contract.
//
// A CG step k has the direction p_{k-1}, the residual r_{k-1}, x_{k-1} in the caller's d_x and q_k = A p_{k-1} (the handle's own
// launch, whatever its plan).  Beside the product it is three launches of the dot's grid over the vectors, ten vector passes:
//
//   cg_dot_parts    the partials of sigma_k = dot(p, q)                                                       (p, q read)
//   cg_residual     every workgroup folds those partials itself (at most 2048 doubles, from L2) and so holds the same sigma_k
//                   and alpha_k = rho_{k-1} / sigma_k; r -= alpha q, and the partials of rho_k = dot(r, r) in the same pass
//                   (q, r read, r written).  Workgroup 0 leaves sigma_k in a word of its own for the next launch;
//   cg_direction    every workgroup folds the partials of rho_k, forms beta_k and the stop rules itself; x += alpha p and, unless
//                   the run stops here, p = r + beta p (x, p, r read, x, p written).  Workgroup 0 writes the step's status
//                   block and the two history elements.
//
// No launch reads a word that another lane of the same launch writes, and every hand-off between workgroups is a launch boundary:
// the partials, sigma's word and the status block are written by one launch and read by later ones; the status block is
// ping-ponged by step parity because cg_direction reads step k - 1's while its workgroup 0 writes step k's.  The device evaluates
// the stop rules at every step.  Once one has fired, cg_residual and cg_direction of every later step see `stopped` in the status
// block, write nothing to x, r, p or the histories, and carry the block over; the host reads the block at looked steps only, and
// only to leave the loop.  Every operation on an element is one rounded IEEE operation (-ffp-contract=off, as everywhere).
#include "smvp_cg_common.h"
#include "smvp_engine.h"
#include "smvp_kernels.h"

#include <cmath>
#include <cstring>
#include <limits>

namespace smvp {

namespace {

// what a step leaves behind for the next step's lanes and, at a looked step, for the host
struct CgStatus {
    double rho;   // rho_updates: the squared residual norm of the last update
    double bb;    // dot(b, b)
    double thr;   // (tol * tol) * bb
    int stopped;  // a rule has fired: reason, steps and updates are final
    int reason;   // SMVP_CG_*
    int steps;    // products done
    int updates;  // updates of x done
};

__global__ __launch_bounds__(kCgBlock) void cg_dot_parts(const double *__restrict__ a, const double *__restrict__ b, int n,
                                                         double *__restrict__ parts)
{
    const double c = cg_fold256(cg_lane_dot(a, b, n));
    if (threadIdx.x == 0)
        parts[blockIdx.x] = c;
}

// one workgroup: the dot from its partials
__global__ __launch_bounds__(kCgBlock) void cg_dot_finish(const double *__restrict__ parts, int nparts, double *__restrict__ out)
{
    const double c = cg_fold_parts(parts, nparts);
    if (threadIdx.x == 0)
        *out = c;
}

// r_0 = b - q (q = A x_0), or b itself without a q; p_0 = r_0; the partials of rho_0 = dot(r_0, r_0)
__global__ __launch_bounds__(kCgBlock) void cg_start(const double *__restrict__ b, const double *__restrict__ q, double *__restrict__ r,
                                                     double *__restrict__ p, int n, double *__restrict__ parts)
{
    const long long stride = (long long)gridDim.x * kCgBlock;
    double c = 0.0;
    for (long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x; i < n; i += stride) {
        const double v = q ? b[i] - q[i] : b[i];
        r[i] = v;
        p[i] = v;
        const double t = v * v;
        c = c + t;
    }
    c = cg_fold256(c);
    if (threadIdx.x == 0)
        parts[blockIdx.x] = c;
}

// one workgroup: bb, rho_0, the threshold and step 0's rule into status block 0, rho_0 into the history
__global__ __launch_bounds__(kCgBlock) void cg_start_finish(const double *__restrict__ parts_bb, const double *__restrict__ parts_rr, int nparts,
                                                            double tol2, CgStatus *__restrict__ st, double *__restrict__ hist_rr)
{
    const double bb = cg_fold_parts(parts_bb, nparts);
    const double rho = cg_fold_parts(parts_rr, nparts);
    if (threadIdx.x != 0)
        return;
    CgStatus s;
    s.rho = rho;
    s.bb = bb;
    s.thr = tol2 * bb;
    const bool bad = !cg_finite(bb) || !cg_finite(rho);
    s.stopped = bad || rho <= s.thr;
    s.reason = bad ? SMVP_CG_NONFINITE : SMVP_CG_CONVERGED;
    s.steps = 0;
    s.updates = 0;
    st[0] = s;
    hist_rr[0] = rho;
}

// step k: prev = the status of step k - 1, parts_pq = the partials of dot(p, q).  r -= alpha q with the partials of dot(r, r).
__global__ __launch_bounds__(kCgBlock) void cg_residual(const double *__restrict__ q, double *__restrict__ r, int n, int nparts,
                                                        const double *__restrict__ parts_pq, const CgStatus *__restrict__ prev,
                                                        double *__restrict__ sigma_out, double *__restrict__ parts_rr)
{
    if (prev->stopped)
        return;
    const double sigma = cg_fold_parts(parts_pq, nparts);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        *sigma_out = sigma;
    if (!cg_finite(sigma) || !(sigma > 0.0))
        return;  // rule A: cg_direction reports it
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

// step k: x += alpha p; rule B; p = r + beta p unless the run stops here.  Workgroup 0 writes status block k and the histories.
__global__ __launch_bounds__(kCgBlock) void cg_direction(double *__restrict__ x, double *__restrict__ p, const double *__restrict__ r, int n,
                                                         int nparts, const double *__restrict__ parts_rr, const double *__restrict__ sigma_in,
                                                         const CgStatus *__restrict__ prev, CgStatus *__restrict__ cur, int step, int max_steps,
                                                         double *__restrict__ hist_rr, double *__restrict__ hist_sigma)
{
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    CgStatus s = *prev;
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
    const double rho = cg_fold_parts(parts_rr, nparts);
    const bool bad = !cg_finite(rho);
    const bool stop = bad || rho <= s.thr || step == max_steps;
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
            double pv[kCgTrips], xv[kCgTrips], rv[kCgTrips];
#pragma unroll
            for (int u = 0; u < kCgTrips; ++u) {
                pv[u] = p[i + u * stride];
                xv[u] = x[i + u * stride];
                rv[u] = r[i + u * stride];
            }
#pragma unroll
            for (int u = 0; u < kCgTrips; ++u) {
                const double ap = alpha * pv[u], bp = beta * pv[u];
                x[i + u * stride] = xv[u] + ap;
                p[i + u * stride] = rv[u] + bp;
            }
        }
        for (; i < n; i += stride) {
            const double pv = p[i];
            const double ap = alpha * pv, bp = beta * pv;
            x[i] = x[i] + ap;
            p[i] = r[i] + bp;
        }
    }
    if (first) {
        s.rho = rho;
        s.updates = step;
        s.stopped = stop;
        s.reason = bad ? SMVP_CG_NONFINITE : rho <= s.thr ? SMVP_CG_CONVERGED : SMVP_CG_MAX_STEPS;
        *cur = s;
        hist_sigma[step - 1] = sigma;
        hist_rr[step] = rho;
    }
}

using CgWork = KrylovWork<CgStatus>;  // r, p, q; the partials of two dots, sigma's word, the histories

}  // namespace

int cg_check_args(const char *fn, const void *h, const smvp_cg_opts_t *o, const smvp_cg_result_t *result, const double *d_b)
{
    if (!h || !o || !result || !d_b)
        return smvp::fail(SMVP_ERR_INVALID, "%s: null %s", fn, !h ? "handle" : !o ? "opts" : !result ? "result" : "d_b");
    if (o->struct_size != (unsigned)sizeof(smvp_cg_opts_t))
        return smvp::fail(SMVP_ERR_INVALID, "%s: smvp_cg_opts_t of %u bytes, this library's has %u: initialise it with "
                                            "smvp_cg_opts_default and build against this library's header",
                          fn, o->struct_size, (unsigned)sizeof(smvp_cg_opts_t));
    if (o->max_steps < 1 || o->check_every < 1 || !(o->tol >= 0.0) || !(o->tol <= std::numeric_limits<double>::max()))
        return smvp::fail(SMVP_ERR_INVALID, "%s: max_steps = %d, check_every = %d, tol = %g (need max_steps >= 1, check_every >= 1, "
                                            "tol >= 0 and finite)", fn, o->max_steps, o->check_every, o->tol);
    return SMVP_OK;
}

int cg_run(const char *fn, int device, int rows, int cols, const smvp_cg_opts_t *o, const double *d_b, const double *d_x0, double *d_x,
           smvp_cg_result_t *result, double *rr_each, double *sigma_each, void *stream, const HandleProduct &product)
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
    DeviceScope on(device);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = refuse_capture(st, "conjugate gradients allocate and synchronise, so they cannot be captured (the stream is capturing)"))
        return rc;
    smvp_cg_result_t res;
    memset(&res, 0, sizeof res);
    res.reason = SMVP_CG_CONVERGED;
    if (n == 0) {
        *result = res;
        return SMVP_OK;
    }

    CgWork w;
    w.stream = st;
    const int max_steps = o->max_steps, grid = cg_grid(n);
    const size_t small_doubles = 2 * (size_t)kCgGridCap + 1 + 2 * (size_t)max_steps + 1;
    const size_t pitch = ((size_t)n + 31) / 32 * 32;  // every vector on a 256-byte boundary, as vectors of their own would be
    if (hipMalloc((void **)&w.vec, sizeof(double) * 3 * pitch) != hipSuccess ||
        hipMalloc((void **)&w.small, sizeof(double) * small_doubles) != hipSuccess ||
        hipMalloc((void **)&w.st, 2 * sizeof(CgStatus)) != hipSuccess || hipHostMalloc((void **)&w.seen, sizeof(CgStatus)) != hipSuccess) {
        (void)hipGetLastError();
        return smvp::fail(SMVP_ERR_ALLOC, "%s: cannot allocate the workspace (%d elements, %d steps)", fn, n, max_steps);
    }
    double *r = w.vec, *p = r + pitch, *q = p + pitch;
    double *parts_a = w.small, *parts_b = parts_a + kCgGridCap, *sigma = parts_b + kCgGridCap;
    double *hist_rr = sigma + 1, *hist_sigma = hist_rr + max_steps + 1;
    const double tol2 = o->tol * o->tol;

    // step 0: x_0 into d_x, bb, r_0 = b - A x_0 (b itself without an x_0: no product), p_0 = r_0, rho_0, the first status block
    hipLaunchKernelGGL(cg_dot_parts, dim3(grid), dim3(kCgBlock), 0, st, d_b, d_b, n, parts_a);
    if (d_x0) {
        if (d_x0 != d_x)
            HIP_TRY(hipMemcpyAsync(d_x, d_x0, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
        if (int rc = product(d_x, q))
            return rc;
    } else {
        HIP_TRY(hipMemsetAsync(d_x, 0, sizeof(double) * (size_t)n, st));
    }
    hipLaunchKernelGGL(cg_start, dim3(grid), dim3(kCgBlock), 0, st, d_b, d_x0 ? q : nullptr, r, p, n, parts_b);
    hipLaunchKernelGGL(cg_start_finish, dim3(1), dim3(kCgBlock), 0, st, parts_a, parts_b, grid, tol2, w.st, hist_rr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(w.seen, w.st, sizeof(CgStatus), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    CgStatus hs = *w.seen;

    for (int k = 1; !hs.stopped; ++k) {
        const CgStatus *prev = w.st + ((k - 1) & 1);
        CgStatus *cur = w.st + (k & 1);
        if (int rc = product(p, q))
            return rc;
        hipLaunchKernelGGL(cg_dot_parts, dim3(grid), dim3(kCgBlock), 0, st, p, q, n, parts_a);
        hipLaunchKernelGGL(cg_residual, dim3(grid), dim3(kCgBlock), 0, st, q, r, n, grid, parts_a, prev, sigma, parts_b);
        hipLaunchKernelGGL(cg_direction, dim3(grid), dim3(kCgBlock), 0, st, d_x, p, r, n, grid, parts_b, sigma, prev, cur, k, max_steps,
                           hist_rr, hist_sigma);
        HIP_TRY(hipGetLastError());
        if (k % o->check_every == 0 || k == max_steps) {  // a looked step: the status block, nothing else, and only to leave the loop
            HIP_TRY(hipMemcpyAsync(w.seen, cur, sizeof(CgStatus), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            hs = *w.seen;
            if (k == max_steps && !hs.stopped)
                return smvp::fail(SMVP_ERR_HIP, "%s: the device did not stop at max_steps = %d", fn, max_steps);
        }
    }
    if (rr_each)
        HIP_TRY(hipMemcpy(rr_each, hist_rr, sizeof(double) * ((size_t)hs.updates + 1), hipMemcpyDeviceToHost));
    if (sigma_each && hs.steps > 0)
        HIP_TRY(hipMemcpy(sigma_each, hist_sigma, sizeof(double) * (size_t)hs.steps, hipMemcpyDeviceToHost));
    res.steps = hs.steps;
    res.updates = hs.updates;
    res.reason = hs.reason;
    res.rr = hs.rho;
    res.bb = hs.bb;
    *result = res;
    return SMVP_OK;
}

}  // namespace smvp

extern "C" void smvp_cg_opts_default(smvp_cg_opts_t *o)
{
    if (!o)
        return;
    memset(o, 0, sizeof *o);
    o->struct_size = (unsigned)sizeof *o;
    o->max_steps = 100;
    o->check_every = 10;
    o->tol = 1e-10;
}

extern "C" int smvp_vector_dot(int device, int n, const double *d_a, const double *d_b, double *result, void *stream)
{
    if (n < 0 || !result || (n > 0 && (!d_a || !d_b)))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_vector_dot: n = %d, d_a %s, d_b %s, result %s (need n >= 0, both vectors where n > 0, "
                                            "and a result)", n, d_a ? "given" : "null", d_b ? "given" : "null", result ? "given" : "null");
    if (n == 0) {
        *result = 0.0;
        return SMVP_OK;
    }
    smvp::DeviceScope on(device);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = smvp::refuse_capture(st, "smvp_vector_dot allocates and synchronises, so it cannot be captured (the stream is capturing)"))
        return rc;
    smvp::CgWork w;
    w.stream = st;
    if (hipMalloc((void **)&w.small, sizeof(double) * ((size_t)smvp::kCgGridCap + 1)) != hipSuccess) {
        (void)hipGetLastError();
        return smvp::fail(SMVP_ERR_ALLOC, "smvp_vector_dot: cannot allocate the partials");
    }
    const int grid = smvp::cg_grid(n);
    double *out = w.small + smvp::kCgGridCap, host = 0.0;
    hipLaunchKernelGGL(smvp::cg_dot_parts, dim3(grid), dim3(smvp::kCgBlock), 0, st, d_a, d_b, n, w.small);
    hipLaunchKernelGGL(smvp::cg_dot_finish, dim3(1), dim3(smvp::kCgBlock), 0, st, w.small, grid, out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&host, out, sizeof host, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *result = host;
    return SMVP_OK;
}
