// smvp_gmres.hip -- restarted GMRES on a handle's own product, A x = b for a general square matrix, to the bits include/smvp_amd.h
// defines: K19, right-preconditioned with K18's M = T1 diag(m)^-1 T2, each of the three parts optional and all three NULL allowed
// (smvp_csr_gmres, smvp_tjds_gmres).  New: the reference only multiplies.  The dot, its folds, the grid rule, the workspace holder,
// krylov_apply and the launch discipline are smvp_cg_common.h's; the solves are K15's kernels.
//
// A step k = c * restart + j of cycle c has the basis v_1 .. v_j, the columns 1 .. j - 1 of R, the rotations and g.  z = M^-1 v_j
// and w = A z come first (the handle's own launches).  Classical Gram-Schmidt, applied twice, is a fixed sequence of launches:
//
//   gm_multidot     the partials of h_i = dot(v_i, w) for i = 1 .. j in ONE launch.  A lane keeps kGmTrips of its w elements in
//                   registers and streams the basis past them, kGmChunk accumulators at a time (compile-time sizes: the accumulators
//                   stay in registers, no scratch).  Grid and slot-to-lane map are the dot's, so each h_i is `dot`'s bits.
//                   (v_1 .. v_j read once, w read ceil(j / kGmChunk) times)
//   gm_fold         one workgroup per coefficient: cg_fold_parts of its 2048 partials, one word per coefficient (and in the second
//                   pass the sum h_i + q_i beside it) -- the passes below read j words, not j * 2048 partials
//   gm_update<0>    w = w - h_i v_i, i ascending, per element, then the partials of the second pass's q_i = dot(v_i, w) by
//                   gm_multidot's loop, in the same launch: every lane reads back only elements it wrote itself
//   gm_fold         q_i, and h_i + q_i
//   gm_update<1>    w = w - q_i v_i with the partials of dot(w, w) in the same sweep
//   gm_close        every workgroup folds dot(w, w), takes the root and runs the step's j - 1 old rotations and the new one over the
//                   j + 1 words (plain doubles, every lane the same numbers), so every lane knows rules S1 and S2; workgroup 0,
//                   lane 0 writes column j of R, c_j, s_j, g, the history element and the status block; unless the run stops
//                   here, v_{j+1} = w / h_{j+1}.
//
// Beside the product and the solves that is six launches a step and 4 j + 6 + 2 ceil(j / kGmChunk) vector passes (the byte model is
// in DESIGN.md).  kGmChunk = 4 and kGmTrips = 2 are what the compiler keeps in registers: gm_multidot 44 VGPRs, gm_update 126, no
// scratch (8 coefficients at a time, or 4 trips, make it hoist every load of the loop body and spill).
// A cycle ends with the update of x -- gm_solve_y (one lane: the back-substitution), gm_form_u (u = V y, one pass over the basis),
// z = M^-1 u, gm_add_x -- and the next begins with r = b - A x (gm_residual, with the partials of tr_c) and gm_begin (every
// workgroup folds tr_c: the start rule, beta, v_1 = r / beta).
//
// The status block is ping-ponged by writer: gm_begin and gm_close read one block and write the other.  Once a rule has fired every
// later launch of these kernels sees `stopped` and writes nothing; the products and solves enqueued in vain write the workspace's w
// and z only.  The update of x at a stop has no fixed place in the enqueued sequence: the launches at a cycle's end act only while the
// run has not stopped, and once the host has seen `stopped` it enqueues the same launches once more, told to act on the stopped
// cycle's columns -- the basis, R and g they read have not changed since.
#include "smvp_cg_common.h"
#include "smvp_engine.h"
#include "smvp_kernels.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace smvp {

namespace {

constexpr int kGmMaxRestart = 64;
constexpr int kGmChunk = 4;  // coefficients a lane accumulates at a time
constexpr int kGmTrips = 2;  // of its w elements in registers while the basis streams past them

struct GmStatus {
    double bb;    // dot(b, b)
    double thr;   // (tol * tol) * bb
    double rr;    // rr_steps, or tr_c where the cycle has no step yet
    int stopped;  // a rule has fired: everything below is final
    int reason;   // SMVP_GMRES_*
    int steps;    // steps done
    int cycles;   // cycles started
    int columns;  // of the update that belongs to the stop (while running: columns of the cycle so far)
    int nrr;      // elements of the rr history
};

// the words the launches hand on, all in one array: R is restart x restart by columns
struct GmWords {
    double *coef;  // restart: the coefficients of the pass at hand
    double *hsum;  // restart: h_i, then h_i + q_i
    double *R;     // restart * restart
    double *cs;    // restart
    double *sn;    // restart
    double *gbar;  // restart + 1: gbar_1 = beta, gbar_{j+1} = -(s_j * gbar_j)
    double *g;     // restart: g_j = c_j * gbar_j, what the back-substitution reads
    double *y;     // restart
};

// a lane's accumulators of v_{i0 + a}[s] * w[s], a < CH, over its slots: cg_lane_dot's terms in cg_lane_dot's order; then the
// workgroup's partial of each into its set of `parts` (kCgGridCap doubles a set)
template <int CH>
__device__ inline void gm_chunk_parts(const double *__restrict__ V, size_t pitch, int i0, const double *w, int n, double *__restrict__ parts)
{
    const long long stride = (long long)gridDim.x * kCgBlock;
    long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x;
    const double *__restrict__ v0 = V + (size_t)i0 * pitch;
    double acc[CH];
#pragma unroll
    for (int a = 0; a < CH; ++a)
        acc[a] = 0.0;
    for (; i + (kGmTrips - 1) * stride < n; i += kGmTrips * stride) {
        double wv[kGmTrips];
#pragma unroll
        for (int u = 0; u < kGmTrips; ++u)
            wv[u] = w[i + u * stride];
#pragma unroll
        for (int a = 0; a < CH; ++a) {
            double t[kGmTrips];
#pragma unroll
            for (int u = 0; u < kGmTrips; ++u)
                t[u] = v0[(size_t)a * pitch + i + u * stride] * wv[u];
#pragma unroll
            for (int u = 0; u < kGmTrips; ++u)
                acc[a] = acc[a] + t[u];
        }
    }
    for (; i < n; i += stride) {
        const double wv = w[i];
#pragma unroll
        for (int a = 0; a < CH; ++a) {
            const double t = v0[(size_t)a * pitch + i] * wv;
            acc[a] = acc[a] + t;
        }
    }
#pragma unroll
    for (int a = 0; a < CH; ++a) {
        const double c = cg_fold256(acc[a]);
        if (threadIdx.x == 0)
            parts[(size_t)(i0 + a) * kCgGridCap + blockIdx.x] = c;
    }
}

// the partials of dot(v_i, w), i < j: whole chunks of kGmChunk coefficients, then the rest as chunks of 2 and 1
__device__ inline void gm_multidot_parts(const double *__restrict__ V, size_t pitch, int j, const double *w, int n, double *__restrict__ parts)
{
    static_assert(kGmChunk == 4, "the tail below is 2 + 1");
    int i0 = 0;
    for (; i0 + kGmChunk <= j; i0 += kGmChunk)
        gm_chunk_parts<kGmChunk>(V, pitch, i0, w, n, parts);
    if ((j - i0) & 2) {
        gm_chunk_parts<2>(V, pitch, i0, w, n, parts);
        i0 += 2;
    }
    if ((j - i0) & 1)
        gm_chunk_parts<1>(V, pitch, i0, w, n, parts);
}

__global__ __launch_bounds__(kCgBlock) void gm_multidot(const double *__restrict__ V, size_t pitch, int j, const double *__restrict__ w, int n,
                                                        double *__restrict__ parts, const GmStatus *__restrict__ prev)
{
    if (prev->stopped)
        return;
    gm_multidot_parts(V, pitch, j, w, n, parts);
}

// workgroup i: coefficient i of the pass from its partials; in the second pass h_i + q_i beside it
__global__ __launch_bounds__(kCgBlock) void gm_fold(const double *__restrict__ parts, int nparts, int second, double *__restrict__ coef,
                                                    double *__restrict__ hsum, const GmStatus *__restrict__ prev)
{
    if (prev->stopped)
        return;
    const double c = cg_fold_parts(parts + (size_t)blockIdx.x * kCgGridCap, nparts);
    if (threadIdx.x == 0) {
        coef[blockIdx.x] = c;
        hsum[blockIdx.x] = second ? hsum[blockIdx.x] + c : c;
    }
}

// w = w - coef_i v_i for i < j ascending, the product rounded, then the difference.  Second = false: then the partials of
// dot(v_i, w) on the new w (sets 0 .. j - 1 of parts).  Second = true: the partials of dot(w, w) in the same sweep (parts_ww).
template <bool Second>
__global__ __launch_bounds__(kCgBlock) void gm_update(const double *__restrict__ V, size_t pitch, int j, double *w, int n,
                                                      const double *__restrict__ coef, double *__restrict__ parts,
                                                      const GmStatus *__restrict__ prev)
{
    if (prev->stopped)
        return;
    const long long stride = (long long)gridDim.x * kCgBlock;
    long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x;
    double c = 0.0;
    for (; i + (kCgTrips - 1) * stride < n; i += kCgTrips * stride) {
        double wv[kCgTrips];
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u)
            wv[u] = w[i + u * stride];
#pragma unroll 4
        for (int a = 0; a < j; ++a) {
            const double h = coef[a];
            const double *__restrict__ v = V + (size_t)a * pitch;
            double hv[kCgTrips];
#pragma unroll
            for (int u = 0; u < kCgTrips; ++u)
                hv[u] = h * v[i + u * stride];
#pragma unroll
            for (int u = 0; u < kCgTrips; ++u)
                wv[u] = wv[u] - hv[u];
        }
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u) {
            w[i + u * stride] = wv[u];
            if (Second) {
                const double t = wv[u] * wv[u];
                c = c + t;
            }
        }
    }
    for (; i < n; i += stride) {
        double wv = w[i];
        for (int a = 0; a < j; ++a) {
            const double hv = coef[a] * V[(size_t)a * pitch + i];
            wv = wv - hv;
        }
        w[i] = wv;
        if (Second) {
            const double t = wv * wv;
            c = c + t;
        }
    }
    if (Second) {
        c = cg_fold256(c);
        if (threadIdx.x == 0)
            parts[blockIdx.x] = c;
    } else {
        gm_multidot_parts(V, pitch, j, w, n, parts);  // a lane's slots here are the slots it has just written
    }
}

// r = b - q (q = A x), or b itself without a q; the partials of tr = dot(r, r)
__global__ __launch_bounds__(kCgBlock) void gm_residual(const double *__restrict__ b, const double *__restrict__ q, double *__restrict__ r,
                                                        int n, double *__restrict__ parts, const GmStatus *__restrict__ prev)
{
    if (prev && prev->stopped)
        return;
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
        parts[blockIdx.x] = c;
}

// cycle c begins: every workgroup folds tr_c (cycle 0: and bb) and evaluates the start rule; v_1 = r / beta unless it fires.
// Workgroup 0 writes the status block, tr_c into the restart history (cycle 0: and into the rr history) and gbar_1 = beta.
__global__ __launch_bounds__(kCgBlock) void gm_begin(const double *__restrict__ r, double *__restrict__ v1, int n, int nparts,
                                                     const double *__restrict__ parts_bb, const double *__restrict__ parts_tr, double tol2,
                                                     const GmStatus *__restrict__ prev, GmStatus *__restrict__ cur, int cycle,
                                                     double *__restrict__ gbar, double *__restrict__ hist_rr, double *__restrict__ hist_tr)
{
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    GmStatus s;
    if (prev) {
        s = *prev;
        if (s.stopped) {
            if (first)
                *cur = s;
            return;
        }
    } else {
        s.bb = cg_fold_parts(parts_bb, nparts);
        s.thr = tol2 * s.bb;
        s.stopped = 0;
        s.reason = SMVP_GMRES_CONVERGED;
        s.steps = 0;
        s.columns = 0;
        s.nrr = 1;
    }
    const double tr = cg_fold_parts(parts_tr, nparts);
    const bool bad = !cg_finite(s.bb) || !cg_finite(tr);
    const bool stop = bad || tr <= s.thr;
    const double beta = sqrt(tr);
    if (first) {
        s.rr = tr;
        s.cycles = cycle + 1;
        s.columns = 0;
        if (stop) {
            s.stopped = 1;
            s.reason = bad ? SMVP_GMRES_NONFINITE : SMVP_GMRES_CONVERGED;
        }
        *cur = s;
        hist_tr[cycle] = tr;
        if (cycle == 0)
            hist_rr[0] = tr;
        gbar[0] = beta;
    }
    if (stop)
        return;
    const long long stride = (long long)gridDim.x * kCgBlock;
    for (long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x; i < n; i += stride)
        v1[i] = r[i] / beta;
}

// step `step`, column j (1 .. restart) of its cycle: h_{j+1}, the rotations, rules S1 and S2, v_{j+1}
__global__ __launch_bounds__(kCgBlock) void gm_close(const double *__restrict__ w, double *__restrict__ vnext, int n, int nparts,
                                                     const double *__restrict__ parts_ww, int j, int restart, GmWords words,
                                                     const GmStatus *__restrict__ prev, GmStatus *__restrict__ cur, int step, int max_steps,
                                                     double *__restrict__ hist_rr)
{
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    GmStatus s = *prev;
    if (s.stopped) {
        if (first)
            *cur = s;
        return;
    }
    const double hn = sqrt(cg_fold_parts(parts_ww, nparts));  // h_{j+1}
    double *__restrict__ Rj = words.R + (size_t)(j - 1) * restart;
    double hi = words.hsum[0];
    bool bad = !cg_finite(hn) || !cg_finite(hi);
    for (int i = 0; i + 1 < j; ++i) {
        const double hx = words.hsum[i + 1];
        bad = bad || !cg_finite(hx);
        const double ci = words.cs[i], si = words.sn[i];
        const double ch = ci * hi, sh = si * hx, cx = ci * hx, sx = si * hi;
        if (first)
            Rj[i] = ch + sh;
        hi = cx - sx;
    }
    const double hh = hi * hi, nn = hn * hn;
    const double d = sqrt(hh + nn);
    bad = bad || !cg_finite(d);
    s.steps = step;
    if (bad || d == 0.0) {  // rule S1
        if (first) {
            s.stopped = 1;
            s.reason = bad ? SMVP_GMRES_NONFINITE : SMVP_GMRES_BREAKDOWN;
            s.columns = j - 1;
            *cur = s;
        }
        return;
    }
    const double cj = hi / d, sj = hn / d;
    const double gb = words.gbar[j - 1];
    const double sg = sj * gb;
    const double gnext = -sg;
    const double rr = gnext * gnext;
    const int reason = rr <= s.thr ? SMVP_GMRES_CONVERGED : step == max_steps ? SMVP_GMRES_MAX_STEPS : -1;  // rule S2
    if (first) {
        Rj[j - 1] = d;
        words.cs[j - 1] = cj;
        words.sn[j - 1] = sj;
        words.g[j - 1] = cj * gb;
        words.gbar[j] = gnext;
        hist_rr[step] = rr;
        s.rr = rr;
        s.nrr = step + 1;
        s.columns = j;
        if (reason >= 0) {
            s.stopped = 1;
            s.reason = reason;
        }
        *cur = s;
    }
    if (reason >= 0)
        return;
    const long long stride = (long long)gridDim.x * kCgBlock;
    long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x;
    for (; i + (kCgTrips - 1) * stride < n; i += kCgTrips * stride) {
        double wv[kCgTrips];
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u)
            wv[u] = w[i + u * stride];
#pragma unroll
        for (int u = 0; u < kCgTrips; ++u)
            vnext[i + u * stride] = wv[u] / hn;
    }
    for (; i < n; i += stride)
        vnext[i] = w[i] / hn;
}

// the launches of an update act while the run has not stopped, or, forced, on the stopped cycle's columns
__device__ inline bool gm_update_acts(const GmStatus *st, int forced) { return forced || !st->stopped; }

// one lane: y from R y = g, last row first
__global__ void gm_solve_y(GmWords words, int restart, int cols, const GmStatus *__restrict__ st, int forced)
{
    if (blockIdx.x != 0 || threadIdx.x != 0 || !gm_update_acts(st, forced))
        return;
    for (int i = cols - 1; i >= 0; --i) {
        double acc = words.g[i];
        for (int l = i + 1; l < cols; ++l) {
            const double ry = words.R[(size_t)l * restart + i] * words.y[l];
            acc = acc - ry;
        }
        words.y[i] = acc / words.R[(size_t)i * restart + i];
    }
}

// u = y_1 v_1, then u = u + y_i v_i for i ascending: one pass over the basis
__global__ __launch_bounds__(kCgBlock) void gm_form_u(const double *__restrict__ V, size_t pitch, int cols, const double *__restrict__ y,
                                                      double *__restrict__ u, int n, const GmStatus *__restrict__ st, int forced)
{
    if (!gm_update_acts(st, forced))
        return;
    const long long stride = (long long)gridDim.x * kCgBlock;
    long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x;
    const double y0 = y[0];
    for (; i + (kCgTrips - 1) * stride < n; i += kCgTrips * stride) {
        double uv[kCgTrips];
#pragma unroll
        for (int t = 0; t < kCgTrips; ++t)
            uv[t] = y0 * V[i + t * stride];
#pragma unroll 4
        for (int a = 1; a < cols; ++a) {
            const double ya = y[a];
            const double *__restrict__ v = V + (size_t)a * pitch;
            double yv[kCgTrips];
#pragma unroll
            for (int t = 0; t < kCgTrips; ++t)
                yv[t] = ya * v[i + t * stride];
#pragma unroll
            for (int t = 0; t < kCgTrips; ++t)
                uv[t] = uv[t] + yv[t];
        }
#pragma unroll
        for (int t = 0; t < kCgTrips; ++t)
            u[i + t * stride] = uv[t];
    }
    for (; i < n; i += stride) {
        double uv = y0 * V[i];
        for (int a = 1; a < cols; ++a) {
            const double yv = y[a] * V[(size_t)a * pitch + i];
            uv = uv + yv;
        }
        u[i] = uv;
    }
}

// x = x + z
__global__ __launch_bounds__(kCgBlock) void gm_add_x(double *__restrict__ x, const double *__restrict__ z, int n,
                                                     const GmStatus *__restrict__ st, int forced)
{
    if (!gm_update_acts(st, forced))
        return;
    const long long stride = (long long)gridDim.x * kCgBlock;
    for (long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x; i < n; i += stride)
        x[i] = x[i] + z[i];
}

// yhat_i = m_i * y_i into a vector of its own: what krylov_apply expects of the kernel that wrote y where there is no `first`
__global__ __launch_bounds__(kCgBlock) void gm_scale_into(double *__restrict__ yhat, const double *__restrict__ y,
                                                          const double *__restrict__ m, int n)
{
    const long long stride = (long long)gridDim.x * kCgBlock;
    for (long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x; i < n; i += stride)
        yhat[i] = m[i] * y[i];
}

using GmWork = KrylovWork<GmStatus>;

// what the product multiplies: M^-1 y in z, or y itself without an M
const double *gm_apply(const char *fn, const KrylovPrecond &M, const double *y, double *z, int n, hipStream_t st, int *rc)
{
    *rc = SMVP_OK;
    if (!M.first && !M.d_m && !M.second)
        return y;
    if (!M.first && M.d_m)
        hipLaunchKernelGGL(gm_scale_into, dim3(cg_grid(n)), dim3(kCgBlock), 0, st, z, y, M.d_m, n);
    *rc = krylov_apply(fn, M, y, z, n, st);
    return z;
}

}  // namespace

int gmres_check_args(const char *fn, const void *h, const smvp_gmres_opts_t *o, const smvp_gmres_result_t *result, const double *d_b)
{
    if (int rc = krylov_check_args(fn, "gmres", h, o, result, d_b))
        return rc;
    if (o->restart < 1 || o->restart > kGmMaxRestart)
        return smvp::fail(SMVP_ERR_INVALID, "%s: restart = %d (need 1 .. %d)", fn, o->restart, kGmMaxRestart);
    return SMVP_OK;
}

int gmres_run(const char *fn, int device, int rows, int cols, const smvp_gmres_opts_t *o, const double *d_b, const double *d_x0, double *d_x,
              const KrylovPrecond &M, smvp_gmres_result_t *result, double *rr_each, double *restart_each, void *stream,
              const HandleProduct &product)
{
    if (int rc = krylov_check_operands(fn, "GMRES needs", device, rows, cols, M, d_b, d_x0, d_x))
        return rc;
    const int n = rows;
    DeviceScope on(device);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = refuse_capture(st, "GMRES allocates and synchronises, so it cannot be captured (the stream is capturing)"))
        return rc;
    smvp_gmres_result_t res;
    memset(&res, 0, sizeof res);
    res.reason = SMVP_GMRES_CONVERGED;
    if (n == 0) {
        *result = res;
        return SMVP_OK;
    }

    GmWork wk;
    wk.stream = st;
    const int max_steps = o->max_steps, grid = cg_grid(n);
    const int restart = std::min(o->restart, max_steps);  // a cycle never gets further than max_steps columns: the same run
    const int max_cycles = (max_steps + restart - 1) / restart;
    const size_t pitch = krylov_pitch(n), R = (size_t)restart;
    // restart + 1 basis vectors, w, u, z, r; the partials of `restart` dots, of dot(w, w), dot(r, r) and dot(b, b), then the words
    // (coef, hsum, R, c, s, gbar, g, y) and the two histories
    const size_t nwords = 2 * R + R * R + 2 * R + (R + 1) + 2 * R;
    if (int rc = krylov_alloc(wk, fn, n, max_steps, (R + 5) * pitch,
                              (R + 3) * (size_t)kCgGridCap + nwords + (size_t)max_steps + 1 + (size_t)max_cycles + 1))
        return rc;
    double *V = wk.vec, *w = V + (R + 1) * pitch, *u = w + pitch, *z = u + pitch, *r = z + pitch;
    double *parts = wk.small, *parts_ww = parts + R * kCgGridCap, *parts_tr = parts_ww + kCgGridCap, *parts_bb = parts_tr + kCgGridCap;
    GmWords words;
    words.coef = parts_bb + kCgGridCap;
    words.hsum = words.coef + R;
    words.R = words.hsum + R;
    words.cs = words.R + R * R;
    words.sn = words.cs + R;
    words.gbar = words.sn + R;
    words.g = words.gbar + R + 1;
    words.y = words.g + R;
    double *hist_rr = words.y + R, *hist_tr = hist_rr + max_steps + 1;
    const double tol2 = o->tol * o->tol;
    const dim3 g(grid), blk(kCgBlock);
    int rc = SMVP_OK;

    // x = x + M^-1 (V y) over `ncols` columns: at a cycle's end while the run goes on, or forced after the host has seen the stop
    auto update_x = [&](int ncols, const GmStatus *block, int forced) -> int {
        hipLaunchKernelGGL(gm_solve_y, dim3(1), dim3(64), 0, st, words, restart, ncols, block, forced);
        hipLaunchKernelGGL(gm_form_u, g, blk, 0, st, V, pitch, ncols, words.y, u, n, block, forced);
        int arc;
        const double *add = gm_apply(fn, M, u, z, n, st, &arc);
        if (arc)
            return arc;
        hipLaunchKernelGGL(gm_add_x, g, blk, 0, st, d_x, add, n, block, forced);
        return SMVP_OK;
    };

    // cycle 0: x_0 into d_x, bb, r = b - A x_0 (b itself without an x_0: no product), tr_0, the start rule, v_1
    int at = 0;  // the status block written last
    hipLaunchKernelGGL(krylov_dot_parts, g, blk, 0, st, d_b, d_b, n, parts_bb);
    if ((rc = krylov_first_x(product, d_x0, d_x, w, n, st)))
        return rc;
    hipLaunchKernelGGL(gm_residual, g, blk, 0, st, d_b, d_x0 ? w : nullptr, r, n, parts_tr, (const GmStatus *)nullptr);
    hipLaunchKernelGGL(gm_begin, g, blk, 0, st, r, V, n, grid, parts_bb, parts_tr, tol2, (const GmStatus *)nullptr, wk.st + at, 0, words.gbar,
                       hist_rr, hist_tr);
    HIP_TRY(hipGetLastError());
    GmStatus hs;
    if ((rc = krylov_look(wk, fn, wk.st + at, 0, max_steps, &hs)))
        return rc;

    for (int k = 1; !hs.stopped; ++k) {
        const int cycle = (k - 1) / restart, j = (k - 1) % restart + 1;
        const GmStatus *prev = wk.st + at;
        const double *vj = V + (size_t)(j - 1) * pitch;
        const double *zj = gm_apply(fn, M, vj, z, n, st, &rc);
        if (rc)
            return rc;
        if ((rc = product(zj, w)))
            return rc;
        hipLaunchKernelGGL(gm_multidot, g, blk, 0, st, V, pitch, j, w, n, parts, prev);
        hipLaunchKernelGGL(gm_fold, dim3(j), blk, 0, st, parts, grid, 0, words.coef, words.hsum, prev);
        hipLaunchKernelGGL(gm_update<false>, g, blk, 0, st, V, pitch, j, w, n, words.coef, parts, prev);
        hipLaunchKernelGGL(gm_fold, dim3(j), blk, 0, st, parts, grid, 1, words.coef, words.hsum, prev);
        hipLaunchKernelGGL(gm_update<true>, g, blk, 0, st, V, pitch, j, w, n, words.coef, parts_ww, prev);
        hipLaunchKernelGGL(gm_close, g, blk, 0, st, w, V + (size_t)j * pitch, n, grid, parts_ww, j, restart, words, prev, wk.st + (at ^ 1), k,
                           max_steps, hist_rr);
        at ^= 1;
        if (j == restart && k < max_steps) {  // the cycle's end and the next one's start (at max_steps the device has stopped)
            if ((rc = update_x(restart, wk.st + at, 0)))
                return rc;
            if ((rc = product(d_x, w)))
                return rc;
            hipLaunchKernelGGL(gm_residual, g, blk, 0, st, d_b, w, r, n, parts_tr, wk.st + at);
            hipLaunchKernelGGL(gm_begin, g, blk, 0, st, r, V, n, grid, (const double *)nullptr, parts_tr, tol2, wk.st + at, wk.st + (at ^ 1),
                               cycle + 1, words.gbar, hist_rr, hist_tr);
            at ^= 1;
        }
        HIP_TRY(hipGetLastError());
        if (k % o->check_every == 0 || k == max_steps)
            if ((rc = krylov_look(wk, fn, wk.st + at, k, max_steps, &hs)))
                return rc;
    }
    if (hs.columns > 0) {  // the stopped cycle's update: nothing it reads has changed since the stop
        if ((rc = update_x(hs.columns, wk.st + at, 1)))
            return rc;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    if ((rc = krylov_history(rr_each, hist_rr, hs.nrr)))
        return rc;
    if ((rc = krylov_history(restart_each, hist_tr, hs.cycles)))
        return rc;
    res.steps = hs.steps;
    res.cycles = hs.cycles;
    res.columns = hs.columns;
    res.reason = hs.reason;
    res.rr = hs.rr;
    res.bb = hs.bb;
    *result = res;
    return SMVP_OK;
}

}  // namespace smvp

extern "C" void smvp_gmres_opts_default(smvp_gmres_opts_t *o)
{
    if (!o)
        return;
    memset(o, 0, sizeof *o);
    o->struct_size = (unsigned)sizeof *o;
    o->max_steps = 100;
    o->check_every = 10;
    o->restart = 30;
    o->tol = 1e-10;
}
