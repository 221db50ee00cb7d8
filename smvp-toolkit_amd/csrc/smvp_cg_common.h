// smvp_cg_common.h -- what the Krylov loops on a handle share (smvp_cg.hip: K12, K14, K16; smvp_bicgstab.hip: K13, K18; smvp_gmres.hip: K19; smvp_lsqr.hip: K22): the
// order-defined dot's building blocks as include/smvp_amd.h words them, the grid rule of every vector pass, the finite test, the two
// kernels both families launch, the checks every call makes before it touches the device, and the host side of a status loop around
// the holder of a call's workspace.  Everything lives in an unnamed namespace: each of the four files compiles its own copy, device
// code included.
//
// The launch discipline, for every solver of the four files (K19 ping-pongs its status block by writer, not by step parity; K22's closing launch reads the block before the one it writes).  No launch reads a word that another lane of the same launch writes, and
// every hand-off between workgroups is a launch boundary: every dot has partials of its own, written by one launch and folded by
// every workgroup of a later one (at most 2048 doubles, from L2), and a scalar that one launch folds reaches the later launches of
// the step through a word of its own, written by workgroup 0 with a plain store.  NO KERNEL WAITS ON A VALUE ANOTHER WORKGROUP
// WRITES (K15's solves keep that rule for themselves: a chain's levels meet at __syncthreads() of its one workgroup).  No atomics,
// no flags.  The status block is ping-ponged by step parity, because the step's last launch reads step k - 1's while its workgroup
// 0 writes step k's.  The device evaluates the stop rules at every step.  Once one has fired, every later launch of the solver's own
// kernels sees `stopped` in the status block, writes nothing to x, to the recurrence's vectors or to the histories, and the last
// one carries the block over; products, solves and scalings enqueued in vain write workspace vectors nobody reads again.  The host
// reads the block at looked steps only, and only to leave the loop.  Every operation on an element is one rounded IEEE operation
// (-ffp-contract=off, as everywhere).
#pragma once
#include "smvp_engine.h"

#include <hip/hip_runtime.h>

#include <limits>

namespace smvp {

namespace {

constexpr int kCgBlock = 256;     // four wavefronts
constexpr int kCgGridCap = 2048;  // workgroups of every vector pass: one grid trip = 2048 * 256 elements
constexpr int kCgTrips = 4;       // trips in flight per lane of a pass that also writes
constexpr int kCgDotTrips = 8;    // ... of the dot's pass, which only reads

__device__ inline bool cg_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// fold256 of the workgroup's 256 accumulators, in every lane; every lane calls it, and twice in a row is fine
__device__ inline double cg_fold256(double c)
{
    __shared__ double s_w[kCgBlock / 64];
#pragma unroll
    for (int h = 32; h > 0; h >>= 1)
        c = c + __shfl_xor(c, h, 64);  // lane 0 ends with c_j + c_{j+h} for h = 32 ... 1 (IEEE addition is commutative)
    __syncthreads();                   // (the last call's readers are done with s_w)
    if ((threadIdx.x & 63) == 0)
        s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// the second level: lane l adds the partials l, l + 256, ... in ascending order, then fold256
__device__ inline double cg_fold_parts(const double *__restrict__ parts, int nparts)
{
    double c = 0.0;
    for (int i = threadIdx.x; i < nparts; i += kCgBlock)
        c = c + parts[i];
    return cg_fold256(c);
}

// a lane's accumulator of a[i] * b[i] over its slots: the terms rounded, added in ascending order
__device__ inline double cg_lane_dot(const double *__restrict__ a, const double *__restrict__ b, int n)
{
    const long long stride = (long long)gridDim.x * kCgBlock;
    long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x;
    double c = 0.0;
    for (; i + (kCgDotTrips - 1) * stride < n; i += kCgDotTrips * stride) {
        double t[kCgDotTrips];
#pragma unroll
        for (int u = 0; u < kCgDotTrips; ++u)
            t[u] = a[i + u * stride] * b[i + u * stride];
#pragma unroll
        for (int u = 0; u < kCgDotTrips; ++u)
            c = c + t[u];
    }
    for (; i < n; i += stride) {
        const double t = a[i] * b[i];
        c = c + t;
    }
    return c;
}

// the partials of dot(a, b): one per workgroup
__global__ __launch_bounds__(kCgBlock) void krylov_dot_parts(const double *__restrict__ a, const double *__restrict__ b, int n,
                                                             double *__restrict__ parts)
{
    const double c = cg_fold256(cg_lane_dot(a, b, n));
    if (threadIdx.x == 0)
        parts[blockIdx.x] = c;
}

// w_i = m_i * w_i between a preconditioner's two solves, in place: one rounded multiplication
__global__ __launch_bounds__(kCgBlock) void krylov_scale(double *__restrict__ w, const double *__restrict__ m, int n)
{
    const long long stride = (long long)gridDim.x * kCgBlock;
    long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x;
    for (; i + (kCgTrips - 1) * stride < n; i += kCgTrips * stride) {
        double wv[kCgTrips], mv[kCgTrips];
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            wv[u] = w[i + u * stride];
            mv[u] = m[i + u * stride];
        }
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u)
            w[i + u * stride] = mv[u] * wv[u];
    }
    for (; i < n; i += stride)
        w[i] = m[i] * w[i];
}

inline int cg_grid(int n)
{
    const long long want = ((long long)n + kCgBlock - 1) / kCgBlock;
    return (int)(want < kCgGridCap ? want : kCgGridCap);
}

// ------------------------------------------------------------------------------------------------ before the device is touched
// handle, opts, result and d_b (and d_m where the solver cannot do without one), then the options: no HIP call.  family: "cg" or
// "bicgstab", as in smvp_<family>_opts_t.
template <class Opts>
int krylov_check_args(const char *fn, const char *family, const void *h, const Opts *o, const void *result, const double *d_b,
                      bool d_m_missing = false)
{
    if (!h || !o || !result || !d_b || d_m_missing)
        return smvp::fail(SMVP_ERR_INVALID, "%s: null %s", fn, !h ? "handle" : !o ? "opts" : !result ? "result" : !d_b ? "d_b" : "d_m");
    if (o->struct_size != (unsigned)sizeof(Opts))
        return smvp::fail(SMVP_ERR_INVALID, "%s: smvp_%s_opts_t of %u bytes, this library's has %u: initialise it with "
                                            "smvp_%s_opts_default and build against this library's header",
                          fn, family, o->struct_size, (unsigned)sizeof(Opts), family);
    if (o->max_steps < 1 || o->check_every < 1 || !(o->tol >= 0.0) || !(o->tol <= std::numeric_limits<double>::max()))
        return smvp::fail(SMVP_ERR_INVALID, "%s: max_steps = %d, check_every = %d, tol = %g (need max_steps >= 1, check_every >= 1, "
                                            "tol >= 0 and finite)", fn, o->max_steps, o->check_every, o->tol);
    return SMVP_OK;
}

// the matrix, the plans the caller brought and the operands, refused in the order every solver has kept.  needs: "conjugate
// gradients need" or "BiCGSTAB needs".  (operands_overlap is false for an operand that is not given.)
inline int krylov_check_operands(const char *fn, const char *needs, int device, int rows, int cols, const KrylovPrecond &M, const double *d_b,
                                 const double *d_x0, const double *d_x)
{
    if (rows != cols)
        return smvp::fail(SMVP_ERR_INVALID, "%s: %s a square matrix (%d x %d given)", fn, needs, rows, cols);
    const int n = rows;
    for (const smvp_trsv_t *t : {(const smvp_trsv_t *)M.first, (const smvp_trsv_t *)M.second}) {
        if (!t)
            continue;
        const char *which = t == M.first ? "first" : "second";
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
    if (operands_overlap(M.d_m, 1, n, d_x, 1, n, 1))
        return smvp::fail(SMVP_ERR_INVALID, "%s: d_m and d_x overlap", fn);
    return SMVP_OK;
}

// ------------------------------------------------------------------------------------------------------ the status loop's host side
// a call's workspace: freed on every way out, after what the call enqueued has finished.  Status is the loop's status block.
template <class Status>
struct KrylovWork {
    hipStream_t stream = nullptr;
    double *vec = nullptr;    // the loop's vectors
    double *small = nullptr;  // the partials of its dots, the words its launches hand on, the histories
    Status *st = nullptr;     // two blocks, by step parity
    Status *seen = nullptr;   // pinned host memory: where a looked step's block is copied to
    ~KrylovWork()
    {
        (void)hipStreamSynchronize(stream);
        if (seen)
            (void)hipHostFree(seen);
        for (void *v : {(void *)vec, (void *)small, (void *)st})
            if (v)
                (void)hipFree(v);
    }
};

// every vector of a workspace on a 256-byte boundary, as vectors of their own would be
inline size_t krylov_pitch(int n) { return ((size_t)n + 31) / 32 * 32; }

template <class Status>
int krylov_alloc(KrylovWork<Status> &w, const char *fn, int n, int max_steps, size_t vec_doubles, size_t small_doubles)
{
    if (hipMalloc((void **)&w.vec, sizeof(double) * vec_doubles) != hipSuccess ||
        hipMalloc((void **)&w.small, sizeof(double) * small_doubles) != hipSuccess ||
        hipMalloc((void **)&w.st, 2 * sizeof(Status)) != hipSuccess || hipHostMalloc((void **)&w.seen, sizeof(Status)) != hipSuccess) {
        (void)hipGetLastError();
        return smvp::fail(SMVP_ERR_ALLOC, "%s: cannot allocate the workspace (%d elements, %d steps)", fn, n, max_steps);
    }
    return SMVP_OK;
}

// x_0 into d_x and q = A x_0; without an x_0, zeros and no product (r_0 is b itself)
inline int krylov_first_x(const HandleProduct &product, const double *d_x0, double *d_x, double *q, int n, hipStream_t st)
{
    if (!d_x0) {
        HIP_TRY(hipMemsetAsync(d_x, 0, sizeof(double) * (size_t)n, st));
        return SMVP_OK;
    }
    if (d_x0 != d_x)
        HIP_TRY(hipMemcpyAsync(d_x, d_x0, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
    return product(d_x, q);
}

// a looked step k: the status block, nothing else, and only to leave the loop
template <class Status>
int krylov_look(KrylovWork<Status> &w, const char *fn, const Status *block, int k, int max_steps, Status *hs)
{
    HIP_TRY(hipMemcpyAsync(w.seen, block, sizeof(Status), hipMemcpyDeviceToHost, w.stream));
    HIP_TRY(hipStreamSynchronize(w.stream));
    *hs = *w.seen;
    if (k == max_steps && !hs->stopped)
        return smvp::fail(SMVP_ERR_HIP, "%s: the device did not stop at max_steps = %d", fn, max_steps);
    return SMVP_OK;
}

// the filled elements of a history the caller asked for
inline int krylov_history(double *each, const double *hist, int count)
{
    if (each && count > 0)
        HIP_TRY(hipMemcpy(each, hist, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
    return SMVP_OK;
}

// yhat = M^-1 y with M = T1 diag(m)^-1 T2, each part optional: first's solve out of y into yhat, yhat_i = m_i * yhat_i, second's
// solve in place.  Without a `first` the multiplication has no launch here: the kernel that wrote y wrote m .* y into yhat beside
// it, and `second` solves in place on that; with neither, `second` solves straight from y.
inline int krylov_apply(const char *fn, const KrylovPrecond &M, const double *y, double *yhat, int n, hipStream_t st)
{
    if (M.first) {
        if (int rc = trsv_enqueue(fn, M.first, y, yhat, st))
            return rc;
        if (M.d_m)
            hipLaunchKernelGGL(krylov_scale, dim3(cg_grid(n)), dim3(kCgBlock), 0, st, yhat, M.d_m, n);
    }
    if (M.second)
        return trsv_enqueue(fn, M.second, M.first || M.d_m ? yhat : y, yhat, st);
    return SMVP_OK;
}

}  // namespace

}  // namespace smvp
