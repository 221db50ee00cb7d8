// smvp_power.hip -- K11: the scaled (max-norm) power method on a handle's own product (smvp_csr_power_method,
// smvp_tjds_power_method; new: the reference only ever multiplies, comment at main-cli.c:401).
//
// Step k has the operand x_{k-1} and the product y_k = A x_{k-1} (the handle's own launch, whatever its plan).  Beside the product
// a step is three launches over the two vectors:
//
//   power_reduce   a grid-stride pass over (x_{k-1}, y_k) with a capped grid.  Every lane forms lambda_k = y_k[p] / x_{k-1}[p]
//                  itself, p being the index the last step's status block names (a uniform load: no launch of its own), and
//                  carries three things: the largest |y_k[r] - lambda_k x_{k-1}[r]|, the largest |y_k[r]| and the smallest index
//                  of that magnitude.  The wavefront (__shfl_xor) and then the workgroup (LDS, four wavefronts) reduce by the
//                  same rule and one lane stores the workgroup's partial.  A maximum and "the smaller index of equals" do not
//                  depend on the order they are combined in: no atomics, no counter, nothing to clear per step, one right answer;
//   power_finish   one workgroup combines the partials and writes m_k, p_k, lambda_k, res_k and the stop flags into the status
//                  block, and lambda_k / res_k into the device-side history;
//   power_scale    x_k[r] = y_k[r] / m_k (true division; a copy where not m_k > 0) into the next operand -- into the caller's
//                  d_x at the step the run stops at.
// The same reduce without an x gives p_0 from the start vector before step 1.
//
// NaN is left out with a self-comparison (v == v), never by how a comparison with NaN happens to come out.  The product
// lambda x is rounded before the difference is (-ffp-contract=off, as everywhere in the library).  Traffic per step beside the
// product: x and y read, y read, x written -- four vector passes where launch_normalize_max moves three; the fourth is the
// residual's.  The host reads the status block at looked steps only; between them nothing synchronises.
#include "smvp_engine.h"
#include "smvp_kernels.h"

#include <cmath>
#include <cstring>
#include <limits>

namespace smvp {

namespace {

constexpr int kPowerBlock = 256;     // four wavefronts
constexpr int kPowerGridCap = 2048;  // workgroups of the reduce pass (vector_absmax's cap): one grid trip = 2048 * 256 elements

// what one step leaves behind for the next step's lanes and, at a looked step, for the host
struct PowerStatus {
    double scale;       // m_k
    double eigenvalue;  // lambda_k
    double residual;    // res_k
    int index;          // p_k: where the next step reads its lambda
    int index_prev;     // p_{k-1}: where this step's lambda was read
    int nonfinite;      // lambda_k is NaN or +-Inf
    int zero;           // not (m_k > 0)
    int converged;      // res_k <= (tol |lambda_k|) |x_{k-1}[p_{k-1}]|
    int pad;
};

// the partials of the reduce pass, one per workgroup
struct PowerParts {
    double *mag;
    double *res;
    int *idx;
};

__device__ inline double power_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// (m, p) <- the better of (m, p) and (om, op): the larger magnitude, of equal magnitudes the smaller index; an index < 0 = nothing yet
__device__ inline void power_take(double &m, int &p, double om, int op)
{
    const bool take = op >= 0 && (p < 0 || om > m || (om == m && op < p));
    m = take ? om : m;
    p = take ? op : p;
}

// the workgroup's (m, p, res) in thread 0; every thread calls it
__device__ inline void power_block_reduce(double &m, int &p, double &res)
{
    __shared__ double s_m[kPowerBlock / 64], s_res[kPowerBlock / 64];
    __shared__ int s_p[kPowerBlock / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double om = __shfl_xor(m, off, 64), ores = __shfl_xor(res, off, 64);
        const int op = __shfl_xor(p, off, 64);
        power_take(m, p, om, op);
        res = ores > res ? ores : res;  // (neither is NaN)
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_m[wave] = m;
        s_p[wave] = p;
        s_res[wave] = res;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kPowerBlock / 64; ++w) {
            power_take(m, p, s_m[w], s_p[w]);
            res = s_res[w] > res ? s_res[w] : res;
        }
    }
}

// kResidual: y = y_k, x = x_{k-1}, st = the status of step k - 1.  Otherwise y is the start vector and x, st are not read.
template <bool kResidual>
__global__ __launch_bounds__(kPowerBlock) void power_reduce(const double *__restrict__ x, const double *__restrict__ y, int n,
                                                            const PowerStatus *__restrict__ st, PowerParts part)
{
    double lambda = 0.0;
    if (kResidual) {
        const int q = st->index;
        lambda = q >= 0 ? y[q] / x[q] : power_nan();
    }
    double m = 0.0, res = 0.0;
    int p = -1;
    const long long stride = (long long)gridDim.x * kPowerBlock;
    for (long long i = (long long)blockIdx.x * kPowerBlock + threadIdx.x; i < n; i += stride) {
        const double v = y[i];
        if (kResidual) {
            const double lx = lambda * x[i];  // rounded, then the difference is rounded
            const double d = fabs(v - lx);
            if (d == d && d > res)
                res = d;
        }
        const double a = fabs(v);
        if (a == a)
            power_take(m, p, a, (int)i);
    }
    power_block_reduce(m, p, res);
    if (threadIdx.x == 0) {
        part.mag[blockIdx.x] = m;
        part.idx[blockIdx.x] = p;
        part.res[blockIdx.x] = res;
    }
}

// one workgroup; step = k (1-based), history slot k - 1
template <bool kResidual>
__global__ __launch_bounds__(kPowerBlock) void power_finish(const double *__restrict__ x, const double *__restrict__ y, int nparts,
                                                            PowerParts part, PowerStatus *__restrict__ st, double tol,
                                                            double *__restrict__ hist_lambda, double *__restrict__ hist_res, int step)
{
    double m = 0.0, res = 0.0;
    int p = -1;
    for (int i = threadIdx.x; i < nparts; i += kPowerBlock) {
        power_take(m, p, part.mag[i], part.idx[i]);
        const double r = part.res[i];
        res = r > res ? r : res;
    }
    power_block_reduce(m, p, res);
    if (threadIdx.x != 0)
        return;
    PowerStatus s;
    s.scale = m;
    s.index = p;
    s.pad = 0;
    if (kResidual) {
        const int q = st->index;
        const double xq = q >= 0 ? x[q] : power_nan();
        const double lambda = q >= 0 ? y[q] / xq : power_nan();
        s.index_prev = q;
        s.eigenvalue = lambda;
        s.residual = res;
        s.nonfinite = !(fabs(lambda) <= 1.7976931348623157e308);
        s.zero = !(m > 0.0);
        const double bound = (tol * fabs(lambda)) * fabs(xq);
        s.converged = res <= bound;
        hist_lambda[step - 1] = lambda;
        hist_res[step - 1] = res;
    } else {
        s.index_prev = -1;
        s.eigenvalue = power_nan();
        s.residual = 0.0;
        s.nonfinite = s.zero = s.converged = 0;
    }
    *st = s;
}

// smvp_run_opts_t.normalize's rule with the divisor the finish left in the status block
__global__ __launch_bounds__(kPowerBlock) void power_scale(const double *__restrict__ y, double *__restrict__ out, int n,
                                                           const PowerStatus *__restrict__ st)
{
    const double m = st->scale;
    const long long i = (long long)blockIdx.x * kPowerBlock + threadIdx.x;
    if (i < n)
        out[i] = m > 0.0 ? y[i] / m : y[i];
}

// the call's workspace: freed on every way out, after what the call enqueued has finished
struct PowerWork {
    hipStream_t stream = nullptr;
    double *a = nullptr, *b = nullptr;  // the operand and the product
    double *hist = nullptr;             // lambda_1 .. lambda_max, then res_1 .. res_max
    void *parts = nullptr;
    PowerStatus *st = nullptr;
    ~PowerWork()
    {
        (void)hipStreamSynchronize(stream);
        for (void *q : {(void *)a, (void *)b, (void *)hist, parts, (void *)st})
            if (q)
                (void)hipFree(q);
    }
};

inline int reduce_grid(int n)
{
    const long long want = ((long long)n + kPowerBlock - 1) / kPowerBlock;
    return (int)(want < kPowerGridCap ? want : kPowerGridCap);
}

}  // namespace

int power_check_args(const char *fn, const void *h, const smvp_power_opts_t *o, const smvp_power_result_t *result)
{
    if (!h || !o || !result)
        return smvp::fail(SMVP_ERR_INVALID, "%s: null %s", fn, !h ? "handle" : !o ? "opts" : "result");
    if (o->struct_size != (unsigned)sizeof(smvp_power_opts_t))
        return smvp::fail(SMVP_ERR_INVALID, "%s: smvp_power_opts_t of %u bytes, this library's has %u: initialise it with "
                                            "smvp_power_opts_default and build against this library's header",
                          fn, o->struct_size, (unsigned)sizeof(smvp_power_opts_t));
    if (o->max_steps < 1 || o->check_every < 1 || !(o->tol >= 0.0) || !(o->tol <= std::numeric_limits<double>::max()))
        return smvp::fail(SMVP_ERR_INVALID, "%s: max_steps = %d, check_every = %d, tol = %g (need max_steps >= 1, check_every >= 1, "
                                            "tol >= 0 and finite)", fn, o->max_steps, o->check_every, o->tol);
    return SMVP_OK;
}

int power_run(const char *fn, int device, int rows, int cols, const smvp_power_opts_t *o, const double *d_x0, double *d_x,
              smvp_power_result_t *result, double *lambda_each, double *residual_each, void *stream, const HandleProduct &product)
{
    if (rows != cols)
        return smvp::fail(SMVP_ERR_INVALID, "%s: the power method needs a square matrix (%d x %d given)", fn, rows, cols);
    const int n = rows;
    if (n > 0 && !d_x)
        return smvp::fail(SMVP_ERR_INVALID, "%s: null d_x", fn);
    if (d_x0 != d_x && operands_overlap(d_x0, 1, n, d_x, 1, n, 1))
        return smvp::fail(SMVP_ERR_INVALID, "%s: d_x0 and d_x overlap without being the same vector", fn);
    DeviceScope on(device);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = refuse_capture(st, "the power method allocates and synchronises, so it cannot be captured (the stream is capturing)"))
        return rc;
    smvp_power_result_t r;
    r.steps = 0;
    r.reason = SMVP_POWER_ZERO;
    r.index = -1;
    r.eigenvalue = std::numeric_limits<double>::quiet_NaN();
    r.residual = 0.0;
    r.scale = 0.0;
    if (n == 0) {
        *result = r;
        return SMVP_OK;
    }

    PowerWork w;
    w.stream = st;
    const int max_steps = o->max_steps, grid = reduce_grid(n);
    const size_t part_bytes = (size_t)kPowerGridCap * (2 * sizeof(double) + sizeof(int));
    if (hipMalloc((void **)&w.a, sizeof(double) * (size_t)n) != hipSuccess || hipMalloc((void **)&w.b, sizeof(double) * (size_t)n) != hipSuccess ||
        hipMalloc((void **)&w.hist, sizeof(double) * 2 * (size_t)max_steps) != hipSuccess || hipMalloc(&w.parts, part_bytes) != hipSuccess ||
        hipMalloc((void **)&w.st, sizeof(PowerStatus)) != hipSuccess) {
        (void)hipGetLastError();
        return smvp::fail(SMVP_ERR_ALLOC, "%s: cannot allocate the workspace (%d elements, %d steps)", fn, n, max_steps);
    }
    PowerParts part;
    part.mag = static_cast<double *>(w.parts);
    part.res = part.mag + kPowerGridCap;
    part.idx = reinterpret_cast<int *>(part.res + kPowerGridCap);
    double *hist_lambda = w.hist, *hist_res = w.hist + max_steps;

    // x_0 into the workspace (d_x may be d_x0, and is written at the end only), p_0 from it
    if (d_x0)
        HIP_TRY(hipMemcpyAsync(w.a, d_x0, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
    else
        HIP_TRY(smvp::launch_fill(w.a, 1.0, n, st));
    hipLaunchKernelGGL(power_reduce<false>, dim3(grid), dim3(kPowerBlock), 0, st, nullptr, w.a, n, nullptr, part);
    hipLaunchKernelGGL(power_finish<false>, dim3(1), dim3(kPowerBlock), 0, st, nullptr, w.a, grid, part, w.st, 0.0, hist_lambda, hist_res, 0);
    HIP_TRY(hipGetLastError());

    const unsigned scale_grid = (unsigned)(((long long)n + kPowerBlock - 1) / kPowerBlock);
    PowerStatus hs{};
    int reason = -1, k = 0;
    while (reason < 0) {
        ++k;
        if (int rc = product(w.a, w.b))
            return rc;
        hipLaunchKernelGGL(power_reduce<true>, dim3(grid), dim3(kPowerBlock), 0, st, w.a, w.b, n, w.st, part);
        hipLaunchKernelGGL(power_finish<true>, dim3(1), dim3(kPowerBlock), 0, st, w.a, w.b, grid, part, w.st, o->tol, hist_lambda, hist_res, k);
        HIP_TRY(hipGetLastError());
        if (k % o->check_every == 0 || k == max_steps) {  // a looked step: the status block, nothing else
            HIP_TRY(hipMemcpyAsync(&hs, w.st, sizeof hs, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            reason = hs.nonfinite ? SMVP_POWER_NONFINITE : hs.zero ? SMVP_POWER_ZERO : hs.converged ? SMVP_POWER_CONVERGED :
                     k == max_steps ? SMVP_POWER_MAX_STEPS : -1;
        }
        hipLaunchKernelGGL(power_scale, dim3(scale_grid), dim3(kPowerBlock), 0, st, w.b, reason < 0 ? w.a : d_x, n, w.st);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (lambda_each)
        HIP_TRY(hipMemcpy(lambda_each, hist_lambda, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost));
    if (residual_each)
        HIP_TRY(hipMemcpy(residual_each, hist_res, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost));
    r.steps = k;
    r.reason = reason;
    r.index = hs.index_prev;
    r.eigenvalue = hs.eigenvalue;
    r.residual = hs.residual;
    r.scale = hs.scale;
    *result = r;
    return SMVP_OK;
}

}  // namespace smvp

extern "C" void smvp_power_opts_default(smvp_power_opts_t *o)
{
    if (!o)
        return;
    memset(o, 0, sizeof *o);
    o->struct_size = (unsigned)sizeof *o;
    o->max_steps = 100;
    o->check_every = 1;
    o->tol = 0.0;
}
