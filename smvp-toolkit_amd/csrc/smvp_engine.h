// smvp_engine.h -- what the files around the CSR handle (smvp_engine.hip) share with it, without its layout: the helpers of
// both handle files, what a TJDS handle (smvp_tjds.hip) needs of its nested CSR handles, and what the timed run (smvp_run.hip)
// needs of either handle.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <ctime>
#include <functional>
#include <string>
#include <vector>

#include "smvp_common.h"
#include "smvp_kernels.h"

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return smvp::fail(SMVP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace smvp {

// Runs the launches of one call on the handle's device, whatever the caller's current device is.
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    explicit DeviceScope(int device)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != device)
            switched = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceScope()
    {
        if (switched)
            (void)hipSetDevice(prev);
    }
};

int usable_device(int device);

// ---------------------------------------------------------------------------------------------- both handle files
inline double wall_ms()
{
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

// `count` elements of host memory as a device array of its own (never shorter than four elements)
template <class T>
int upload(T **dst, const T *src, size_t count)
{
    HIP_TRY(hipMalloc((void **)dst, std::max<size_t>(count, 4) * sizeof(T)));
    if (count)
        HIP_TRY(hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice));
    return SMVP_OK;
}

template <class T>
int upload(T **dst, const std::vector<T> &src) { return upload(dst, src.data(), src.size()); }

// a caller's array: adopted where it is on the device already, else uploaded
template <class T>
int to_device(T **dst, const T *src, size_t count, int mem_kind, bool *owned)
{
    *owned = mem_kind != SMVP_MEM_DEVICE;
    if (*owned)
        return upload(dst, src, count);
    *dst = const_cast<T *>(src);
    return SMVP_OK;
}

// The call allocates or synchronises: refused with `why` while `st` is capturing.
inline int refuse_capture(hipStream_t st, const char *why)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(st, &cs));
    if (cs != hipStreamCaptureStatusNone)
        return smvp::fail(SMVP_ERR_INVALID, "%s", why);
    return SMVP_OK;
}

// Do the byte ranges of two operands meet?  An operand is n rows of k doubles, ld doubles from one row to the next (a vector:
// ld = 1, k = 1); without rows it has no bytes.  kb: the columns of b where they are not a's (a vector against a block).
inline bool operands_overlap(const double *a, long long lda, int na, const double *b, long long ldb, int nb, int k, int kb = 0)
{
    const unsigned __int128 a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    const unsigned __int128 a1 = a0 + (na > 0 ? ((unsigned __int128)(na - 1) * (unsigned long long)lda + (unsigned)k) * 8u : 0);
    const unsigned __int128 b1 = b0 + (nb > 0 ? ((unsigned __int128)(nb - 1) * (unsigned long long)ldb + (unsigned)(kb ? kb : k)) * 8u : 0);
    return a && b && na > 0 && nb > 0 && a0 < b1 && b0 < a1;
}

// Device-resident index arrays are range-checked on the device (host arrays are checked on the host).
inline int check_device_indices(const int *d_a, long long n, int limit, const char *what)
{
    if (n <= 0)
        return SMVP_OK;
    int *d_bad = nullptr, h_bad = 0;
    HIP_TRY(hipMalloc((void **)&d_bad, sizeof(int)));
    hipError_t e = hipMemset(d_bad, 0, sizeof(int));
    if (e == hipSuccess)
        e = smvp::launch_find_out_of_range(d_a, n, limit, d_bad, nullptr);
    if (e == hipSuccess)
        e = hipMemcpy(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost);
    (void)hipFree(d_bad);
    if (e != hipSuccess)
        return smvp::fail(SMVP_ERR_HIP, "range check of %s failed: %s", what, hipGetErrorString(e));
    if (h_bad)
        return smvp::fail(SMVP_ERR_INVALID, "%s[%d] lies outside [0, %d)", what, h_bad - 1, limit);
    return SMVP_OK;
}

// What every product of operands X (x_rows rows) and Y (y_rows rows) of k columns checks before anything is enqueued, in this
// order: k and the leading dimensions, an operand that is needed and null, byte ranges that meet.  `fn` opens the message; a
// one-vector product (k = 1, ld = 1: the first check cannot fail) names its operands d_x / d_y.
inline int check_block_operands(const char *fn, int k, const double *X, long long ldx, int x_rows, const double *Y, long long ldy, int y_rows,
                                int nnz, bool block = true)
{
    const char *xn = block ? "d_X" : "d_x", *yn = block ? "d_Y" : "d_y";
    if (k < 1 || ldx < k || ldy < k)
        return smvp::fail(SMVP_ERR_INVALID, "%s: k = %d, ldx = %lld, ldy = %lld (need k >= 1, ldx >= k, ldy >= k)", fn, k, ldx, ldy);
    if ((nnz > 0 && !X) || (y_rows > 0 && !Y))
        return smvp::fail(SMVP_ERR_INVALID, "%s: null %s", fn, y_rows > 0 && !Y ? yn : xn);
    if (operands_overlap(X, ldx, x_rows, Y, ldy, y_rows, k))
        return smvp::fail(SMVP_ERR_INVALID, "%s: the byte ranges of %s and %s overlap", fn, xn, yn);
    return SMVP_OK;
}

// ------------------------------------------------------------------------- a TJDS handle and its nested CSR handles
// what a TJDS flavour borrows from its smvp_tjds owner (set before the tile plan is built)
struct TjdsSource {
    const int *pos = nullptr;
    const int *start_pos = nullptr;
    int num_diag = 0;
    // the two-phase product's second phase: `val` holds the products of the first phase (written anew before every launch: no value
    // cache, overflow entries by position), the operand is the unit vector (no x gather)
    bool unit_operand = false;
};

// A handle of a TJDS flavour (smvp_kernels.h kFlavorTjds*) over device arrays it borrows: planned for the owner kernel, released
// with smvp_csr_destroy, re-tiled with smvp_csr_set_kernel.
int csr_create_tjds(smvp_csr_t **out, int device, int rows, int cols, int nnz, const int *d_row_ptr, const int *d_col_ind,
                    const double *d_val, int flavor, const TjdsSource &src);
// The value cache of a tile-ordered stream (TilePlan::d_val_cache): its threshold and the entries it holds -- false, and zeros, for
// a handle that has no such stream; and the tile plan built anew for another threshold (plan_build_ms is left as it is).
bool csr_value_cache(const smvp_csr_t *h, int *min_tiles, long long *cached_entries);
int csr_replan_value_cache(smvp_csr_t *h, int min_tiles);
// the owner kernel as the handle launches it, with its template arguments: entries per thread, flavour (0, 0 without a handle), false
std::string csr_owner_kernel_name(const smvp_csr_t *h);
// bytes of device memory the current launch plan keeps beside row_ptr / col_ind / val
double csr_plan_bytes(const smvp_csr_t *h);

// what a plan beside the handle (K15, smvp_trsv.hip) borrows of a CSR handle: its device arrays, the host copy of row_ptr (valid as
// long as the handle lives) and where it stands
struct CsrView {
    int device, rows, cols, nnz, flavor;
    long long first_row;
    const int *d_row_ptr, *d_col_ind;
    const double *d_val;
    const int *h_row_ptr;
};
CsrView csr_view(const smvp_csr_t *h);
// K23 (smvp_reorder.hip): a plain-CSR handle on AUTO over three device arrays this library allocated itself -- the handle frees
// them when it is destroyed.  After a failure *out is NULL and the arrays are still the caller's to free.
int csr_create_owning(smvp_csr_t **out, int device, int rows, int cols, int nnz, int *d_row_ptr, int *d_col_ind, double *d_val);

// ---------------------------------------------------------------------------------------------------- the timed run
// Per format: the {first, last} tick pairs one stamped product writes (0: the current plan cannot time itself on the device -- see
// StampTimer), the grid of the repeating launch (0: no such form), `reps` products in one launch of it, and one product whose
// launch stamps its window (stamps == nullptr: the plain product).  The TJDS forms multiply the operand of smvp_tjds_set_x.
int csr_stamp_slots(const smvp_csr_t *h);
int csr_repeat_grid(const smvp_csr_t *h);
int csr_spmv_repeat(smvp_csr_t *h, const double *d_x, double *d_y, void *stream, unsigned long long *stamps, int reps, int grid,
                    unsigned *ctl_words, bool first_of_run, unsigned long long patience);
int csr_spmv_stamped(smvp_csr_t *h, const double *d_x, double *d_y, void *stream, unsigned long long *stamps);
int tjds_stamp_slots(const smvp_tjds_t *h);
int tjds_repeat_grid(const smvp_tjds_t *h);
int tjds_spmv_repeat(smvp_tjds_t *h, double *d_y, void *stream, unsigned long long *stamps, int reps, int grid, unsigned *ctl_words,
                     bool first_of_run, unsigned long long patience);
int tjds_spmv_stamped(smvp_tjds_t *h, double *d_y, void *stream, unsigned long long *stamps);

// ------------------------------------------------------------------------------------------- the power method (K11)
// smvp_power.hip runs the steps; the handle files check what is theirs to check and hand it their product (HandleProduct): y = A x for device
// vectors of the handle's size, enqueued on the call's stream.  power_check_args makes no HIP call (a null handle is refused on a
// box without a device); power_run checks the operands and the stream, then allocates, iterates and frees.
using HandleProduct = std::function<int(const double *d_x, double *d_y)>;
int power_check_args(const char *fn, const void *h, const smvp_power_opts_t *opts, const smvp_power_result_t *result);
int power_run(const char *fn, int device, int rows, int cols, const smvp_power_opts_t *opts, const double *d_x0, double *d_x,
              smvp_power_result_t *result, double *lambda_each, double *residual_each, void *stream, const HandleProduct &product);

// ------------------------------------------------------------------------------- the Krylov solvers (K12 to K14, K16, K18, K19)
// smvp_cg.hip, smvp_bicgstab.hip and smvp_gmres.hip run the steps around the same product hook, checked and handed over by the handle files as for
// K11.  The *_check_args make no HIP call; the *_run check the plans, the operands and the stream, then allocate, iterate and free.
// A preconditioner is M = T1 diag(m)^-1 T2: z = T2^-1 (m .* (T1^-1 r)), any part may be missing.  The plans are K15's
// (smvp_trsv.hip): trsv_enqueue is the launch loop smvp_trsv_solve itself goes through, with the operands checked and the plan's
// device current already; trsv_rows and trsv_device say what a plan was made for.
int trsv_rows(const smvp_trsv_t *t);
int trsv_device(const smvp_trsv_t *t);
int trsv_enqueue(const char *fn, smvp_trsv_t *t, const double *d_b, double *d_x, hipStream_t stream);
struct KrylovPrecond {
    smvp_trsv_t *first = nullptr;
    const double *d_m = nullptr;
    smvp_trsv_t *second = nullptr;
};

// conjugate gradients.  Where z = M^-1 r comes from: r itself (K12), r ./ m with M's d_m alone (K14), or a vector the two solves
// fill, with m between them where there is one (K16).  K12 fills its own result block, which has no rz.
enum class Precond { none, diagonal, stored };
int cg_check_args(const char *fn, const void *h, const smvp_cg_opts_t *opts, const void *result, const double *d_b, Precond kind,
                  const KrylovPrecond &M);
int cg_run(const char *fn, int device, int rows, int cols, const smvp_cg_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
           Precond kind, const KrylovPrecond &M, smvp_pcg_result_t *result, double *rr_each, double *rz_each, double *sigma_each,
           void *stream, const HandleProduct &product);
int cg_run(const char *fn, int device, int rows, int cols, const smvp_cg_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
           smvp_cg_result_t *result, double *rr_each, double *sigma_each, void *stream, const HandleProduct &product);

// conjugate gradients for k right-hand sides (K20, smvp_cg_multi.hip): k runs of K12 (d_m == NULL) or K14 that share every launch.
// The product is a block product of the handle (BlockProduct): Y = A X for the call's k columns, X and Y row-major device blocks with
// leading dimensions of their own, enqueued on the call's stream -- smvp_csr_spmm's / smvp_tjds_spmm's enqueue, which builds the
// handle's block-product plan where it has none.
using BlockProduct = std::function<int(const double *d_X, long long ldx, double *d_Y, long long ldy)>;
int cg_multi_check_args(const char *fn, const void *h, const smvp_cg_opts_t *opts, const void *results, const double *d_B);
int cg_multi_run(const char *fn, int device, int rows, int cols, const smvp_cg_opts_t *opts, int k, const double *d_B, long long ldb,
                 const double *d_X0, long long ldx0, double *d_X, long long ldx, const double *d_m, smvp_pcg_result_t *results,
                 double *rr_each, double *rz_each, double *sigma_each, void *stream, const BlockProduct &product);

// BiCGSTAB, two products a step.  M == nullptr: K13; else K18 with phat = M^-1 p and shat = M^-1 s, which pbicgstab_check_args
// refuses where all three parts are NULL.
int bicgstab_check_args(const char *fn, const void *h, const smvp_bicgstab_opts_t *opts, const smvp_bicgstab_result_t *result,
                        const double *d_b);
int pbicgstab_check_args(const char *fn, const void *h, const smvp_bicgstab_opts_t *opts, const smvp_bicgstab_result_t *result,
                         const double *d_b, const KrylovPrecond &M);
int bicgstab_run(const char *fn, int device, int rows, int cols, const smvp_bicgstab_opts_t *opts, const double *d_b, const double *d_x0,
                 double *d_x, const KrylovPrecond *M, smvp_bicgstab_result_t *result, double *rr_each, double *ss_each, void *stream,
                 const HandleProduct &product);

// restarted GMRES (K19, smvp_gmres.hip), one product a step.  M with all three parts NULL is plain GMRES.
int gmres_check_args(const char *fn, const void *h, const smvp_gmres_opts_t *opts, const smvp_gmres_result_t *result, const double *d_b);
int gmres_run(const char *fn, int device, int rows, int cols, const smvp_gmres_opts_t *opts, const double *d_b, const double *d_x0,
              double *d_x, const KrylovPrecond &M, smvp_gmres_result_t *result, double *rr_each, double *restart_each, void *stream,
              const HandleProduct &product);

// LSQR (K22, smvp_lsqr.hip), two products a step: forward is y = A x (cols -> rows elements), transposed y = A^T x (rows -> cols).
// The handle files make smvp_common.h's lsqr_check_args and their own checks of the handles first; lsqr_run checks the operands and
// the stream, then allocates, iterates and frees.  rows != cols is what it is for.
int lsqr_run(const char *fn, int device, int rows, int cols, const smvp_lsqr_opts_t *opts, const double *d_b, const double *d_x0,
             double *d_x, smvp_lsqr_result_t *result, double *rnorm_each, double *arnorm_each, void *stream, const HandleProduct &forward,
             const HandleProduct &transposed);

}  // namespace smvp
