// smvp_cg.hip -- conjugate gradients on a handle's own product, to the bits include/smvp_amd.h defines: K12 without a
// preconditioner (smvp_csr_cg, smvp_tjds_cg), K14 with a diagonal one (smvp_csr_pcg, smvp_tjds_pcg), K16 with M = T1 diag(m)^-1 T2
// from two of K15's triangular-solve plans the caller brings (smvp_csr_pcg_tri, smvp_tjds_pcg_tri); and the dot product whose
// order of additions the header defines (smvp_vector_dot).  New: the reference only ever multiplies.
//
// The dot.  G = min(ceil(n / 256), 2048) workgroups of 256 lanes.  Lane l of workgroup g owns slot s = 256 g + l and adds the
// rounded terms t_s, t_{s + 256 G}, ... in ascending order to an accumulator that starts at +0.0 (eight trips are loaded before
// the first is added; they are added in that order).  fold256 -- a __shfl_xor butterfly inside each wavefront, then
// ((w0 + w1) + w2) + w3 through LDS -- gives the workgroup's partial, and the same fold over a second level (lane l adds the
// partials l, l + 256, ... in ascending order) gives the dot.  No atomics: the order is part of the contract.
//
// One set of kernels, one host loop, and a compile-time variant (Precond) that says where z = M^-1 r comes from.  A step k has the
// direction p_{k-1}, the residual r_{k-1}, x_{k-1} in the caller's d_x, rho_{k-1} = dot(r_{k-1}, z_{k-1}) in the status block and
// q_k = A p_{k-1} (the handle's own launch, whatever its plan).  Beside the product it is launches of the dot's grid over the vectors:
//
//   krylov_dot_parts  the partials of sigma_k = dot(p, q)                                                     (p, q read)
//   cg_residual       every workgroup folds those partials itself and so holds the same sigma_k and alpha_k = rho_{k-1} / sigma_k;
//                     r -= alpha q and the partials of rr_k = dot(r, r) in the same pass (q, r read, r written).  Workgroup 0 leaves
//                     sigma_k in a word of its own for cg_direction;
//   cg_direction      every workgroup folds the partials of rr_k and rho_k, forms beta_k and the stop rules itself; x += alpha p and,
//                     unless the run stops here, p = z + beta p (x, p, z's source read, x, p written).  Workgroup 0 writes the
//                     step's status block and the history elements.
//
//                     none (K12)                    diagonal (K14)                       stored (K16)
//   z_i               r_i                           r_i / m_i, an IEEE division, never    read from a fourth vector z, which the two
//                                                   stored: a launch that needs it        solves (krylov_apply: first's out of r,
//                                                   divides again, the same bits          krylov_scale by m, second's in place) fill
//   start             r, p = r, partials of rr      r, p = r ./ m, partials of rr, rho    r, partials of rr; after the solves
//                                                                                         cg_start_direction: p = z, partials of rho
//   residual          one accumulator               reads m, two accumulators             one accumulator
//   rho's partials    are rr's                      from cg_residual                      krylov_dot_parts over (r, z) after the solves
//   direction         reads r                       reads r and m                         reads z
//   rules             no "not (rho > 0)" rule       K14's                                 K14's
//   launches, passes  3, 10                         3, 12                                 5 beside the solves (4 without an m), 15
//
// The launch discipline is smvp_cg_common.h's.  A step of K16 after the stop still rewrites z from an r that no longer changes.
#include "smvp_cg_common.h"
#include "smvp_engine.h"
#include "smvp_kernels.h"

#include <cmath>
#include <cstring>

namespace smvp {

namespace {

// what a step leaves behind for the next step's lanes and, at a looked step, for the host.  Without a preconditioner rho and rr
// hold the same number.
struct CgStatus {
    double rho;   // rho_updates = dot(r, z) of the last update
    double rr;    // dot(r, r) of the last update: what the stop rule looks at
    double bb;    // dot(b, b)
    double thr;   // (tol * tol) * bb
    int stopped;  // a rule has fired: reason, steps and updates are final
    int reason;   // SMVP_CG_*
    int steps;    // products done
    int updates;  // updates of x done
};

// one workgroup: the dot from its partials
__global__ __launch_bounds__(kCgBlock) void cg_dot_finish(const double *__restrict__ parts, int nparts, double *__restrict__ out)
{
    const double c = cg_fold_parts(parts, nparts);
    if (threadIdx.x == 0)
        *out = c;
}

// r_0 = b - q (q = A x_0), or b itself without a q, and the partials of rr_0 = dot(r_0, r_0).  none: p_0 = r_0.  diagonal:
// p_0 = z_0 = r_0 ./ m and the partials of rho_0 = dot(r_0, z_0).  stored: p_0 waits for the solves (cg_start_direction).
template <Precond P>
__global__ __launch_bounds__(kCgBlock) void cg_start(const double *__restrict__ b, const double *__restrict__ q, const double *__restrict__ m,
                                                     double *__restrict__ r, double *__restrict__ p, int n, double *__restrict__ parts_rr,
                                                     double *__restrict__ parts_rz)
{
    const long long stride = (long long)gridDim.x * kCgBlock;
    double c = 0.0, e = 0.0;
    for (long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x; i < n; i += stride) {
        const double v = q ? b[i] - q[i] : b[i];
        r[i] = v;
        if (P == Precond::none)
            p[i] = v;
        if (P == Precond::diagonal) {
            const double z = v / m[i];
            p[i] = z;
            const double s = v * z;
            e = e + s;
        }
        const double t = v * v;
        c = c + t;
    }
    c = cg_fold256(c);
    if (P == Precond::diagonal)
        e = cg_fold256(e);
    if (threadIdx.x == 0) {
        parts_rr[blockIdx.x] = c;
        if (P == Precond::diagonal)
            parts_rz[blockIdx.x] = e;
    }
}

// stored: p_0 = z_0 and the partials of rho_0 = dot(r_0, z_0)
__global__ __launch_bounds__(kCgBlock) void cg_start_direction(const double *__restrict__ r, const double *__restrict__ z, double *__restrict__ p,
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

// one workgroup: bb, rr_0, rho_0, the threshold and step 0's rule into status block 0, rr_0 and rho_0 into the histories.  OwnRho:
// rho has partials and a history of its own, and "not (rho_0 > 0)" is a breakdown; without, rho_0 is rr_0.
template <bool OwnRho>
__global__ __launch_bounds__(kCgBlock) void cg_start_finish(const double *__restrict__ parts_bb, const double *__restrict__ parts_rr,
                                                            const double *__restrict__ parts_rz, int nparts, double tol2,
                                                            CgStatus *__restrict__ st, double *__restrict__ hist_rr,
                                                            double *__restrict__ hist_rz)
{
    const double bb = cg_fold_parts(parts_bb, nparts);
    const double rr = cg_fold_parts(parts_rr, nparts);
    const double rho = OwnRho ? cg_fold_parts(parts_rz, nparts) : rr;
    if (threadIdx.x != 0)
        return;
    CgStatus s;
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
    st[0] = s;
    hist_rr[0] = rr;
    if (OwnRho)
        hist_rz[0] = rho;
}

// step k: prev = the status of step k - 1, parts_pq = the partials of dot(p, q).  r -= alpha q with the partials of dot(r, r);
// diagonal: and of dot(r, r ./ m), a second accumulator per lane in the dot's own order.
template <Precond P>
__global__ __launch_bounds__(kCgBlock) void cg_residual(const double *__restrict__ q, const double *__restrict__ m, double *__restrict__ r,
                                                        int n, int nparts, const double *__restrict__ parts_pq,
                                                        const CgStatus *__restrict__ prev, double *__restrict__ sigma_out,
                                                        double *__restrict__ parts_rr, double *__restrict__ parts_rz)
{
    constexpr bool kDiag = P == Precond::diagonal;
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
    double c = 0.0, e = 0.0;
    for (; i + (kCgTrips - 1) * stride < n; i += kCgTrips * stride) {
        double v[kCgTrips], aq[kCgTrips], mv[kCgTrips];
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            aq[u] = alpha * q[i + u * stride];  // rounded, then the difference is rounded
            v[u] = r[i + u * stride];
            if (kDiag)
                mv[u] = m[i + u * stride];
        }
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            v[u] = v[u] - aq[u];
            r[i + u * stride] = v[u];
            const double t = v[u] * v[u];
            c = c + t;
            if (kDiag) {
                const double z = v[u] / mv[u];
                const double s = v[u] * z;
                e = e + s;
            }
        }
    }
    for (; i < n; i += stride) {
        const double aq = alpha * q[i];
        const double v = r[i] - aq;
        r[i] = v;
        const double t = v * v;
        c = c + t;
        if (kDiag) {
            const double z = v / m[i];
            const double s = v * z;
            e = e + s;
        }
    }
    c = cg_fold256(c);
    if (kDiag)
        e = cg_fold256(e);
    if (threadIdx.x == 0) {
        parts_rr[blockIdx.x] = c;
        if (kDiag)
            parts_rz[blockIdx.x] = e;
    }
}

// step k: x += alpha p; rule B; p = z + beta p unless the run stops here.  zs is the vector z comes from: r (none: z = r; diagonal:
// z = r ./ m) or the stored z.  Workgroup 0 writes status block k and the histories.
template <Precond P>
__global__ __launch_bounds__(kCgBlock) void cg_direction(double *__restrict__ x, double *__restrict__ p, const double *__restrict__ zs,
                                                         const double *__restrict__ m, int n, int nparts,
                                                         const double *__restrict__ parts_rr, const double *__restrict__ parts_rz,
                                                         const double *__restrict__ sigma_in, const CgStatus *__restrict__ prev,
                                                         CgStatus *__restrict__ cur, int step, int max_steps, double *__restrict__ hist_rr,
                                                         double *__restrict__ hist_rz, double *__restrict__ hist_sigma)
{
    constexpr bool kDiag = P == Precond::diagonal, kOwnRho = P != Precond::none;
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
    const double rr = cg_fold_parts(parts_rr, nparts);
    const double rho = kOwnRho ? cg_fold_parts(parts_rz, nparts) : rr;
    const bool bad = !cg_finite(rr) || !cg_finite(rho);
    const bool down = kOwnRho && !(rho > 0.0);  // K12's rule B has no such rule
    const bool stop = bad || rr <= s.thr || down || step == max_steps;
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
            double pv[kCgTrips], xv[kCgTrips], zv[kCgTrips], mv[kCgTrips];
#pragma unroll
            for (int u = 0; u < kCgTrips; ++u) {
                pv[u] = p[i + u * stride];
                xv[u] = x[i + u * stride];
                zv[u] = zs[i + u * stride];
                if (kDiag)
                    mv[u] = m[i + u * stride];
            }
#pragma unroll
            for (int u = 0; u < kCgTrips; ++u) {
                const double ap = alpha * pv[u], bp = beta * pv[u];
                const double z = kDiag ? zv[u] / mv[u] : zv[u];
                x[i + u * stride] = xv[u] + ap;
                p[i + u * stride] = z + bp;
            }
        }
        for (; i < n; i += stride) {
            const double pv = p[i];
            const double ap = alpha * pv, bp = beta * pv;
            const double z = kDiag ? zs[i] / m[i] : zs[i];
            x[i] = x[i] + ap;
            p[i] = z + bp;
        }
    }
    if (first) {
        s.rho = rho;
        s.rr = rr;
        s.updates = step;
        s.stopped = stop;
        s.reason = bad ? SMVP_CG_NONFINITE : rr <= s.thr ? SMVP_CG_CONVERGED : down ? SMVP_CG_BREAKDOWN : SMVP_CG_MAX_STEPS;
        *cur = s;
        hist_sigma[step - 1] = sigma;
        hist_rr[step] = rr;
        if (kOwnRho)
            hist_rz[step] = rho;
    }
}

using CgWork = KrylovWork<CgStatus>;  // r, p, q (stored: and z); the partials of three dots, sigma's word, the histories

// the workspace and the loop of one run as variant P; the caller has checked everything and made the device current
template <Precond P>
int cg_steps(const char *fn, int n, const smvp_cg_opts_t *o, const double *d_b, const double *d_x0, double *d_x, const KrylovPrecond &M,
             smvp_pcg_result_t *result, double *rr_each, double *rz_each, double *sigma_each, hipStream_t st, const HandleProduct &product)
{
    constexpr bool kStored = P == Precond::stored, kOwnRho = P != Precond::none;
    CgWork w;
    w.stream = st;
    const int max_steps = o->max_steps, grid = cg_grid(n);
    const size_t pitch = krylov_pitch(n);
    if (int rc = krylov_alloc(w, fn, n, max_steps, (kStored ? 4 : 3) * pitch, 3 * (size_t)kCgGridCap + 1 + 3 * (size_t)max_steps + 2))
        return rc;
    double *r = w.vec, *p = r + pitch, *q = p + pitch, *z = kStored ? q + pitch : nullptr;
    double *parts_a = w.small, *parts_b = parts_a + kCgGridCap, *parts_c = parts_b + kCgGridCap, *sigma = parts_c + kCgGridCap;
    double *hist_rr = sigma + 1, *hist_rz = hist_rr + max_steps + 1, *hist_sigma = hist_rz + max_steps + 1;
    const double *m = P == Precond::diagonal ? M.d_m : nullptr;  // the kernels' own m; stored's m goes into krylov_apply only
    const double tol2 = o->tol * o->tol;
    const dim3 g(grid), blk(kCgBlock);

    // step 0: x_0 into d_x, bb, r_0 = b - A x_0 (b itself without an x_0: no product), z_0, p_0 = z_0, rr_0, rho_0, the first status
    // block
    hipLaunchKernelGGL(krylov_dot_parts, g, blk, 0, st, d_b, d_b, n, parts_a);
    if (int rc = krylov_first_x(product, d_x0, d_x, q, n, st))
        return rc;
    hipLaunchKernelGGL(cg_start<P>, g, blk, 0, st, d_b, d_x0 ? q : nullptr, m, r, p, n, parts_b, parts_c);
    if (kStored) {
        if (int rc = krylov_apply(fn, M, r, z, n, st))
            return rc;
        hipLaunchKernelGGL(cg_start_direction, g, blk, 0, st, r, z, p, n, parts_c);
    }
    hipLaunchKernelGGL(cg_start_finish<kOwnRho>, dim3(1), blk, 0, st, parts_a, parts_b, parts_c, grid, tol2, w.st, hist_rr, hist_rz);
    HIP_TRY(hipGetLastError());
    CgStatus hs;
    if (int rc = krylov_look(w, fn, w.st, 0, max_steps, &hs))
        return rc;

    for (int k = 1; !hs.stopped; ++k) {
        const CgStatus *prev = w.st + ((k - 1) & 1);
        CgStatus *cur = w.st + (k & 1);
        if (int rc = product(p, q))
            return rc;
        hipLaunchKernelGGL(krylov_dot_parts, g, blk, 0, st, p, q, n, parts_a);
        hipLaunchKernelGGL(cg_residual<P>, g, blk, 0, st, q, m, r, n, grid, parts_a, prev, sigma, parts_b, parts_c);
        if (kStored) {
            if (int rc = krylov_apply(fn, M, r, z, n, st))
                return rc;
            hipLaunchKernelGGL(krylov_dot_parts, g, blk, 0, st, r, z, n, parts_c);
        }
        hipLaunchKernelGGL(cg_direction<P>, g, blk, 0, st, d_x, p, kStored ? z : r, m, n, grid, parts_b, parts_c, sigma, prev, cur, k,
                           max_steps, hist_rr, hist_rz, hist_sigma);
        HIP_TRY(hipGetLastError());
        if (k % o->check_every == 0 || k == max_steps)
            if (int rc = krylov_look(w, fn, cur, k, max_steps, &hs))
                return rc;
    }
    if (int rc = krylov_history(rr_each, hist_rr, hs.updates + 1))
        return rc;
    if (int rc = krylov_history(rz_each, hist_rz, hs.updates + 1))
        return rc;
    if (int rc = krylov_history(sigma_each, hist_sigma, hs.steps))
        return rc;
    result->steps = hs.steps;
    result->updates = hs.updates;
    result->reason = hs.reason;
    result->rr = hs.rr;
    result->rz = hs.rho;
    result->bb = hs.bb;
    return SMVP_OK;
}

}  // namespace

int cg_check_args(const char *fn, const void *h, const smvp_cg_opts_t *o, const void *result, const double *d_b, Precond kind,
                  const KrylovPrecond &M)
{
    if (int rc = krylov_check_args(fn, "cg", h, o, result, d_b, kind == Precond::diagonal && !M.d_m))
        return rc;
    if (kind == Precond::stored && (!M.first || !M.second))
        return smvp::fail(SMVP_ERR_INVALID, "%s: null %s plan", fn, !M.first ? "first" : "second");
    return SMVP_OK;
}

int cg_run(const char *fn, int device, int rows, int cols, const smvp_cg_opts_t *o, const double *d_b, const double *d_x0, double *d_x,
           Precond kind, const KrylovPrecond &M, smvp_pcg_result_t *result, double *rr_each, double *rz_each, double *sigma_each,
           void *stream, const HandleProduct &product)
{
    if (int rc = krylov_check_operands(fn, "conjugate gradients need", device, rows, cols, M, d_b, d_x0, d_x))
        return rc;
    DeviceScope on(device);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = refuse_capture(st, kind == Precond::none
                                        ? "conjugate gradients allocate and synchronise, so they cannot be captured (the stream is capturing)"
                                    : kind == Precond::diagonal
                                        ? "preconditioned conjugate gradients allocate and synchronise, so they cannot be captured (the stream "
                                          "is capturing)"
                                        : "conjugate gradients preconditioned by triangular solves allocate and synchronise, so they cannot be "
                                          "captured (the stream is capturing)"))
        return rc;
    smvp_pcg_result_t res;
    memset(&res, 0, sizeof res);
    res.reason = SMVP_CG_CONVERGED;
    if (rows > 0) {
        int rc;
        if (kind == Precond::none)
            rc = cg_steps<Precond::none>(fn, rows, o, d_b, d_x0, d_x, M, &res, rr_each, rz_each, sigma_each, st, product);
        else if (kind == Precond::diagonal)
            rc = cg_steps<Precond::diagonal>(fn, rows, o, d_b, d_x0, d_x, M, &res, rr_each, rz_each, sigma_each, st, product);
        else
            rc = cg_steps<Precond::stored>(fn, rows, o, d_b, d_x0, d_x, M, &res, rr_each, rz_each, sigma_each, st, product);
        if (rc)
            return rc;
    }
    *result = res;
    return SMVP_OK;
}

// K12's result block has no rz: rho is rr
int cg_run(const char *fn, int device, int rows, int cols, const smvp_cg_opts_t *o, const double *d_b, const double *d_x0, double *d_x,
           smvp_cg_result_t *result, double *rr_each, double *sigma_each, void *stream, const HandleProduct &product)
{
    smvp_pcg_result_t res;
    if (int rc = cg_run(fn, device, rows, cols, o, d_b, d_x0, d_x, Precond::none, KrylovPrecond{}, &res, rr_each, nullptr, sigma_each, stream,
                        product))
        return rc;
    memset(result, 0, sizeof *result);
    result->steps = res.steps;
    result->updates = res.updates;
    result->reason = res.reason;
    result->rr = res.rr;
    result->bb = res.bb;
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
    hipLaunchKernelGGL(smvp::krylov_dot_parts, dim3(grid), dim3(smvp::kCgBlock), 0, st, d_a, d_b, n, w.small);
    hipLaunchKernelGGL(smvp::cg_dot_finish, dim3(1), dim3(smvp::kCgBlock), 0, st, w.small, grid, out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&host, out, sizeof host, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *result = host;
    return SMVP_OK;
}
