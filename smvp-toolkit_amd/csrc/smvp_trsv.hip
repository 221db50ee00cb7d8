// smvp_trsv.hip -- K15: T x = b for a triangle T of a plain CSR handle's matrix as stored (smvp_csr_trsv_create, smvp_trsv_solve; new:
// the reference only multiplies).  The first kernels here that are not a product: the parallelism is the dependency graph's.  The
// host analysis (smvp_trsv_plan.cpp) sorts the rows into levels; rows of one level do not depend on each other, and every x[c] a
// row reads belongs to an earlier level.  Element i is the serial substitution loop's, bit for bit: s_i and d_i are summed from +0.0
// in ascending storage position, the product rounded before the sum (-ffp-contract=off), then one subtraction and one division.
//
// NO KERNEL WAITS ON A VALUE ANOTHER WORKGROUP WRITES IN THE SAME LAUNCH: no flags, no grid barrier, no atomics.  Between
// workgroups the order is that of the kernel boundaries on the stream; inside the one workgroup of a chain it is __syncthreads(),
// whose workgroup-scope release / acquire makes one wavefront's global stores visible to the others on the same CU.  A wrong
// dependency here can be a wrong number, never a hang.
//
//   trsv_level_rows<T>  one wide level: a group of T lanes per row of order[lo .. hi) (T from the triangle's mean row length, the
//                       rule of csr_vector_rows, over kTrsvChunk).  Lane j of the group takes kTrsvChunk consecutive entries of a
//                       pass: it loads col_ind, classifies (diagonal / inside the triangle / skipped), loads val and x[c] where
//                       they are needed and multiplies.  The additions then run through the lanes in ascending position
//                       (trsv_scan): lane j adds its chunk to what lane j - 1 holds, the running sums handed up by a DPP move, so
//                       the sums are the serial loop's.  A group takes kTrsvRows rows, dealt as in csr_diagonal_rows, and issues the
//                       first pass of all of them before it adds any; further passes of a long row follow, kTrsvTrips in flight.
//                       First build, declined: a lane per entry and a walk of the set bits of two ballots with a shuffle per
//                       entry -- about 120 cycles per entry added, 5.1 ms on memplus (profiles/trsv_measured.txt).
//   trsv_chain<PER>     a maximal run of levels of at most kTrsvChainWidth rows each: ONE workgroup, a barrier after every level.  A
//                       level of more than 128 rows gives every lane a row (PER = 1; 2 or 4 rows under the experiment option
//                       trsv_chain_width), which it walks alone; a thinner one gives every row a group of 2 .. 64 lanes, the most
//                       that leaves each row a group, and adds as trsv_level_rows does (a lone lane on memplus's rows of hundreds
//                       of entries was half of those 5.1 ms).  The loop over the
//                       levels is uniform and the barrier stands outside every branch, so every lane reaches every barrier whatever
//                       its rows' lengths (or without a row).  What the next level needs that does not depend on x -- its rows,
//                       their bounds, b_i -- is loaded in front of the barrier.
// A wide level of more than 2^31 / T rows is cut into launches of that many (launch_level: fewer than 2^32 threads each).
//   trsv_sweep_rows<T, FIRST>  K21 (smvp_csr_trsv_create_sweeps): not the solve but a fixed number of Jacobi sweeps on it, every
//                       sweep one launch of trsv_level_rows's shape over ALL rows -- natural order, a storage range per row instead
//                       of the whole row, the operand iterate in a scratch vector of the plan's (two, alternating), so that no
//                       launch reads what it writes.  A row of level l has the exact solve's bits after l sweeps.
//
// x is read and written in the same launch (other rows'; in a chain, rows of earlier levels) and d_x may be d_b: neither pointer is
// __restrict__ or const __restrict__, or the compiler could serve them from the scalar or read-only path and read stale values.
// b_i is read by the lane that writes x_i, before it does.  The matrix and the schedule are only read: those pointers are.
#include "smvp_engine.h"

#include <cmath>

namespace smvp {

namespace {

constexpr int kTrsvChainWidth = kVectorBlock;  // rows of the widest level a chain takes: a row per lane of its one workgroup.  The
                                               // plan option trsv_chain_width (256, 512 or 1024: a lane takes 1, 2 or 4 rows) is for
                                               // experiments: DESIGN section 4, K15 has the sweep
constexpr int kTrsvRows = 4;                   // rows a group of lanes takes: their first trips' loads are in flight together
constexpr int kTrsvChunk = 4;                  // consecutive entries of a row a lane of its group takes in one pass
constexpr int kTrsvTrips = 2;                  // further passes of a long row whose loads a lane keeps in flight together
constexpr int kTrsvUnroll = 8;                 // entries of its row whose loads a lane of a chain keeps in flight together
constexpr int kTrsvLong = 32;                  // a lone lane of a chain on a long row: so many entries in flight together (a chain is one
                                               // workgroup and may use the registers of four)

// what an entry is to row `row`: 0 skipped, 1 inside the triangle, 2 on the diagonal (skipped where the diagonal is unit)
__device__ inline int trsv_kind(int c, int row, int upper, int unit)
{
    if (c < 0)
        return 0;  // past the row's end
    if (c == row)
        return unit ? 0 : 2;
    return (upper ? c > row : c < row) ? 1 : 0;
}

// the value of the lane below (wave_shr:1; lane 0 of the wavefront reads 0.0): two DPP moves, no LDS
__device__ inline double trsv_from_lane_below(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// One pass over T * kTrsvChunk entries of a group's row: lane j of the group takes the kTrsvChunk CONSECUTIVE entries from p0 =
// base + j * kTrsvChunk on (those at z and beyond are nobody's).  trsv_load turns them into the operands of the two sums: ws = val *
// x[c] inside the triangle, wd = val on the diagonal, +0.0 for everything else.  Adding +0.0 is exact for every value a sum from
// +0.0 can take (it is never -0.0: only -0.0 + -0.0 gives that), so a skipped entry may be added as +0.0 and the loop below needs
// no masks.  GATHER = false (K21's launch 0) loads no x and no val inside the triangle: only wd is meant to be used.
template <bool GATHER = true>
__device__ inline void trsv_load(const int *__restrict__ col_ind, const double *__restrict__ val, const double *x, long long p0, int z,
                                 int row, int upper, int unit, double (&ws)[kTrsvChunk], double (&wd)[kTrsvChunk])
{
    int c[kTrsvChunk], kind[kTrsvChunk];
    double v[kTrsvChunk], xv[kTrsvChunk];
#pragma unroll
    for (int u = 0; u < kTrsvChunk; ++u)
        c[u] = p0 + u < z ? col_ind[p0 + u] : -1;
#pragma unroll
    for (int u = 0; u < kTrsvChunk; ++u) {
        kind[u] = trsv_kind(c[u], row, upper, unit);
        v[u] = (GATHER ? kind[u] != 0 : kind[u] == 2) ? val[p0 + u] : 0.0;
        xv[u] = GATHER && kind[u] == 1 ? x[c[u]] : 0.0;  // an earlier level's element: an earlier launch's, or stored in front of a barrier
    }
#pragma unroll
    for (int u = 0; u < kTrsvChunk; ++u) {
        ws[u] = kind[u] == 1 ? v[u] * xv[u] : 0.0;
        wd[u] = kind[u] == 2 ? v[u] : 0.0;
    }
}

// The additions of a pass in ascending position: n steps, n the lanes of the group that hold entries of this pass (the rest hold
// +0.0).  In step j lane j adds its chunk to what lane j - 1 held after step j - 1 (lane 0: to the sums carried in, s and d).  Every
// lane runs every step -- a lane's value is final once its step has come, and it recomputes the same value afterwards -- so there
// is no branch in it.  On return lane n - 1 holds the sums through this pass (n = 0: every lane still holds s and d).
__device__ inline void trsv_scan(const double (&ws)[kTrsvChunk], const double (&wd)[kTrsvChunk], int n, int lane, double &s, double &d)
{
    double sr = s, dr = d;
    for (int j = 0; j < n; ++j) {
        const double below_s = trsv_from_lane_below(sr), below_d = trsv_from_lane_below(dr);
        sr = lane == 0 ? s : below_s;
        dr = lane == 0 ? d : below_d;
#pragma unroll
        for (int u = 0; u < kTrsvChunk; ++u) {
            sr = sr + ws[u];
            dr = dr + wd[u];
        }
    }
    s = sr;
    d = dr;
}

// lanes of a group of T that hold entries of the pass over [base, z), and the lane that holds a row's sums after its last pass
__device__ inline int trsv_pass_lanes(long long base, int z, int T)
{
    const long long chunks = (z - base + kTrsvChunk - 1) / kTrsvChunk;
    return chunks >= T ? T : chunks > 0 ? (int)chunks : 0;
}
__device__ inline int trsv_last_lane(int a, int z, int T) { return z > a ? ((z - a - 1) / kTrsvChunk) & (T - 1) : 0; }

// A group's row from its second pass on (`base`: where that begins); s and d hold the first pass's sums in lane T - 1 (a further
// pass follows a full one) and are handed to every lane of the group before each further pass.  kTrsvTrips passes' loads are in
// flight together.
template <bool GATHER = true>
__device__ inline void trsv_further_passes(const int *__restrict__ col_ind, const double *__restrict__ val, const double *x, long long base,
                                           int z, int row, int T, int lane, int shift, int upper, int unit, double &s, double &d)
{
    for (; base < z; base += (long long)kTrsvTrips * T * kTrsvChunk) {
        double ws[kTrsvTrips][kTrsvChunk], wd[kTrsvTrips][kTrsvChunk];
#pragma unroll
        for (int u = 0; u < kTrsvTrips; ++u)
            trsv_load<GATHER>(col_ind, val, x, base + ((long long)u * T + lane) * kTrsvChunk, z, row, upper, unit, ws[u], wd[u]);
#pragma unroll
        for (int u = 0; u < kTrsvTrips; ++u) {
            const int n = trsv_pass_lanes(base + (long long)u * T * kTrsvChunk, z, T);
            if (n) {  // (the pass before was a full one: its sums are in lane T - 1)
                s = __shfl(s, shift + T - 1);
                d = __shfl(d, shift + T - 1);
                trsv_scan(ws[u], wd[u], n, lane, s, d);
            }
        }
    }
}

template <int T>
__global__ __launch_bounds__(kVectorBlock) void trsv_level_rows(const int *__restrict__ row_ptr, const int *__restrict__ col_ind,
                                                                 const double *__restrict__ val, const int *__restrict__ order,
                                                                 const double *b, double *x, long long lo, long long hi, int upper,
                                                                 int unit)
{
    constexpr int G = 64 / T;  // groups of a wavefront
    const long long wave = ((long long)blockIdx.x * kVectorBlock + threadIdx.x) >> 6;
    const int lane = threadIdx.x & (T - 1);
    const int shift = threadIdx.x & 63 & ~(T - 1);  // where the group's lanes lie in the wavefront
    const long long k0 = lo + wave * (kTrsvRows * G) + (shift / T);
    int row[kTrsvRows], a[kTrsvRows], z[kTrsvRows];
    double bi[kTrsvRows], ws[kTrsvRows][kTrsvChunk], wd[kTrsvRows][kTrsvChunk];
#pragma unroll
    for (int i = 0; i < kTrsvRows; ++i) {
        const long long k = k0 + i * G;
        row[i] = k < hi ? order[k] : -1;
    }
#pragma unroll
    for (int i = 0; i < kTrsvRows; ++i) {
        a[i] = z[i] = 0;
        bi[i] = 0.0;
        if (row[i] >= 0) {
            a[i] = row_ptr[row[i]];
            z[i] = row_ptr[row[i] + 1];
            if (lane == trsv_last_lane(a[i], z[i], T))
                bi[i] = b[row[i]];  // read by the lane that writes x[row]: d_b may be d_x
        }
    }
#pragma unroll
    for (int i = 0; i < kTrsvRows; ++i)  // the first pass of every row of the wavefront: all their loads before any addition
        trsv_load(col_ind, val, x, (long long)a[i] + lane * kTrsvChunk, z[i], row[i], upper, unit, ws[i], wd[i]);
#pragma unroll
    for (int i = 0; i < kTrsvRows; ++i) {
        double s = 0.0, d = 0.0;
        trsv_scan(ws[i], wd[i], trsv_pass_lanes(a[i], z[i], T), lane, s, d);
        trsv_further_passes(col_ind, val, x, (long long)a[i] + T * kTrsvChunk, z[i], row[i], T, lane, shift, upper, unit, s, d);
        if (lane == trsv_last_lane(a[i], z[i], T) && row[i] >= 0)
            x[row[i]] = unit ? bi[i] - s : (bi[i] - s) / d;
    }
}

// K21, one Jacobi sweep on the triangular system: xout_i = (b_i - s_i(xin)) / d_i for rows lo .. hi - 1 in natural order, the shape
// of trsv_level_rows with three differences.  There is no `order`: neighbouring groups take neighbouring rows and write neighbouring
// elements.  A row's bounds are the plan's storage range [begin_i, end_i), not the whole row: half of col_ind for a matrix stored in
// full with ascending columns.  And the operand iterate xin is another buffer than xout (the plan's scratch vectors, never d_x or
// d_b), written by the launch before and by nobody in this one, so it is const __restrict__; b and xout are not, d_x may be d_b.
// FIRST is launch 0, x(0)_i = (b_i - (+0.0)) / d_i: no gather and no val inside the triangle is loaded (xin is null), and with a
// unit diagonal not even the bounds.  b - (+0.0) is b for every b, a signed zero included.
template <int T, bool FIRST>
__global__ __launch_bounds__(kVectorBlock) void trsv_sweep_rows(const int *__restrict__ col_ind, const double *__restrict__ val,
                                                                 const int *__restrict__ begin, const int *__restrict__ end, const double *b,
                                                                 const double *__restrict__ xin, double *xout, long long lo, long long hi,
                                                                 int upper, int unit)
{
    constexpr int G = 64 / T;  // groups of a wavefront
    const long long wave = ((long long)blockIdx.x * kVectorBlock + threadIdx.x) >> 6;
    const int lane = threadIdx.x & (T - 1);
    const int shift = threadIdx.x & 63 & ~(T - 1);  // where the group's lanes lie in the wavefront
    const long long k0 = lo + wave * (kTrsvRows * G) + (shift / T);
    int row[kTrsvRows], a[kTrsvRows], z[kTrsvRows];
    double bi[kTrsvRows], ws[kTrsvRows][kTrsvChunk], wd[kTrsvRows][kTrsvChunk];
#pragma unroll
    for (int i = 0; i < kTrsvRows; ++i) {
        const long long k = k0 + i * G;
        row[i] = k < hi ? (int)k : -1;
        a[i] = z[i] = 0;
        bi[i] = 0.0;
        if (row[i] >= 0) {
            if (!(FIRST && unit)) {
                a[i] = begin[row[i]];
                z[i] = end[row[i]];
            }
            if (lane == trsv_last_lane(a[i], z[i], T))
                bi[i] = b[row[i]];  // read by the lane that writes xout[row]: on the last launch d_b may be d_x
        }
    }
#pragma unroll
    for (int i = 0; i < kTrsvRows; ++i)  // the first pass of every row of the wavefront: all their loads before any addition
        trsv_load<!FIRST>(col_ind, val, xin, (long long)a[i] + lane * kTrsvChunk, z[i], row[i], upper, unit, ws[i], wd[i]);
#pragma unroll
    for (int i = 0; i < kTrsvRows; ++i) {
        double s = 0.0, d = 0.0;
        trsv_scan(ws[i], wd[i], trsv_pass_lanes(a[i], z[i], T), lane, s, d);
        trsv_further_passes<!FIRST>(col_ind, val, xin, (long long)a[i] + T * kTrsvChunk, z[i], row[i], T, lane, shift, upper, unit, s, d);
        if (FIRST)
            s = 0.0;
        if (lane == trsv_last_lane(a[i], z[i], T) && row[i] >= 0)
            xout[row[i]] = unit ? bi[i] - s : (bi[i] - s) / d;
    }
}

// U entries of one lane's row from position p on (those at z and beyond are nobody's), added in ascending position
template <int U>
__device__ inline void trsv_walk(const int *__restrict__ col_ind, const double *__restrict__ val, const double *x, int p, int z, int row,
                                 int upper, int unit, double &s, double &d)
{
    int c[U], kind[U];
    double v[U], xv[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
        c[u] = p + u < z ? col_ind[p + u] : -1;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        kind[u] = trsv_kind(c[u], row, upper, unit);
        v[u] = kind[u] ? val[p + u] : 0.0;
        xv[u] = kind[u] == 1 ? x[c[u]] : 1.0;  // an earlier level's: an earlier launch's, or stored in front of a barrier
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (kind[u] == 1)
            s = s + v[u] * xv[u];
        else if (kind[u] == 2)
            d = d + v[u];
    }
}

// lanes a row of a chain's level of `width` rows gets: the largest power of two, 64 at the most, that leaves every row a group
__device__ inline int trsv_chain_lanes(int width)
{
    const int q = kVectorBlock / (width > 0 ? width : 1);
    return q >= 64 ? 64 : q >= 2 ? 1 << (31 - __builtin_clz(q)) : 1;
}

template <int PER>
__global__ __launch_bounds__(kVectorBlock) void trsv_chain(const int *__restrict__ row_ptr, const int *__restrict__ col_ind,
                                                            const double *__restrict__ val, const int *__restrict__ level_ptr,
                                                            const int *__restrict__ order, const double *b, double *x, int l0, int l1,
                                                            int upper, int unit)
{
    const int t = threadIdx.x;
    int T = 1;  // lanes a row of the level at hand gets (uniform)
    int row[PER], a[PER], z[PER];
    double bi[PER];
    // a level's rows, their bounds and b_i.  A level of more than 128 rows: lane t takes the rows t, t + 256, ... (at most PER: the
    // host put only levels of at most PER * 256 rows into a chain).  A thinner one: the group of T lanes t / T takes row t / T.
    // Nothing of this depends on x; x[row] has one writer.
    auto take = [&](int l) {
        const int lo = level_ptr[l], hi = level_ptr[l + 1];
        T = trsv_chain_lanes(hi - lo);
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int k = T > 1 ? (r == 0 ? lo + t / T : hi) : lo + t + r * kVectorBlock;
            row[r] = k < hi ? order[k] : -1;
        }
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            a[r] = z[r] = 0;
            if (row[r] >= 0) {
                a[r] = row_ptr[row[r]];
                z[r] = row_ptr[row[r] + 1];
                bi[r] = b[row[r]];
            }
        }
    };
    take(l0);
    for (int l = l0; l < l1; ++l) {  // uniform: every lane of the workgroup takes every turn and reaches every barrier
        if (T > 1) {  // a thin level: a group of lanes per row, the shape of trsv_level_rows
            const int lane = t & (T - 1), shift = t & 63 & ~(T - 1);
            double s = 0.0, d = 0.0, ws[kTrsvChunk], wd[kTrsvChunk];
            trsv_load(col_ind, val, x, (long long)a[0] + lane * kTrsvChunk, z[0], row[0], upper, unit, ws, wd);
            trsv_scan(ws, wd, trsv_pass_lanes(a[0], z[0], T), lane, s, d);
            trsv_further_passes(col_ind, val, x, (long long)a[0] + T * kTrsvChunk, z[0], row[0], T, lane, shift, upper, unit, s, d);
            if (lane == trsv_last_lane(a[0], z[0], T) && row[0] >= 0)
                x[row[0]] = unit ? bi[0] - s : (bi[0] - s) / d;
        } else {
#pragma unroll
            for (int r = 0; r < PER; ++r) {  // a row per lane
                double s = 0.0, d = 0.0;
                int p = a[r];
                for (; z[r] - p > kTrsvUnroll; p += kTrsvLong)
                    trsv_walk<kTrsvLong>(col_ind, val, x, p, z[r], row[r], upper, unit, s, d);
                for (; p < z[r]; p += kTrsvUnroll)
                    trsv_walk<kTrsvUnroll>(col_ind, val, x, p, z[r], row[r], upper, unit, s, d);
                if (row[r] >= 0)
                    x[row[r]] = unit ? bi[r] - s : (bi[r] - s) / d;
            }
        }
        if (l + 1 < l1)
            take(l + 1);  // in front of the barrier: the next level's loads that need no x are under way while the stores drain
        __syncthreads();
    }
}

template <int T>
void launch_level(const CsrView &m, const int *order, const double *b, double *x, long long lo, long long hi, int upper, int unit,
                  hipStream_t stream)
{
    const long long chunk = ((long long)1 << 31) / T;  // (a launch of fewer than 2^32 threads, a multiple of every wavefront's rows)
    constexpr long long kWaveRows = (long long)kTrsvRows * (64 / T);
    for (long long k0 = lo; k0 < hi; k0 += chunk) {
        const long long n = hi - k0 < chunk ? hi - k0 : chunk;
        const long long waves = (n + kWaveRows - 1) / kWaveRows;
        const unsigned grid = (unsigned)((waves * 64 + kVectorBlock - 1) / kVectorBlock);
        hipLaunchKernelGGL(trsv_level_rows<T>, dim3(grid), dim3(kVectorBlock), 0, stream, m.d_row_ptr, m.d_col_ind, m.d_val, order, b, x,
                           k0, k0 + n, upper, unit);
    }
}

// one sweep over rows 0 .. n - 1, cut like a wide level (xin == nullptr: launch 0)
template <int T>
void launch_sweep(const CsrView &m, const int *begin, const int *end, const double *b, const double *xin, double *xout, int unit,
                  int upper, hipStream_t stream)
{
    const long long chunk = ((long long)1 << 31) / T;
    constexpr long long kWaveRows = (long long)kTrsvRows * (64 / T);
    for (long long k0 = 0; k0 < m.rows; k0 += chunk) {
        const long long n = m.rows - k0 < chunk ? m.rows - k0 : chunk;
        const long long waves = (n + kWaveRows - 1) / kWaveRows;
        const unsigned grid = (unsigned)((waves * 64 + kVectorBlock - 1) / kVectorBlock);
        if (xin)
            hipLaunchKernelGGL((trsv_sweep_rows<T, false>), dim3(grid), dim3(kVectorBlock), 0, stream, m.d_col_ind, m.d_val, begin, end, b,
                               xin, xout, k0, k0 + n, upper, unit);
        else
            hipLaunchKernelGGL((trsv_sweep_rows<T, true>), dim3(grid), dim3(kVectorBlock), 0, stream, m.d_col_ind, m.d_val, begin, end, b,
                               xin, xout, k0, k0 + n, upper, unit);
    }
}

int pow2_lanes(double mean)
{
    int p = 2;
    while (p < 64 && p < mean)
        p <<= 1;
    return p;
}

}  // namespace

}  // namespace smvp

struct smvp_trsv {
    smvp::CsrView m{};
    int uplo = 0, diag = 0, lanes = 2, chains = 0, chain_width = 0;
    int *d_level_ptr = nullptr, *d_order = nullptr;
    smvp::TrsvSchedule sched;
    std::vector<smvp::TrsvLaunch> launches;
    long long entries = 0;
    double plan_bytes = 0.0, build_ms = 0.0;
    // K21, a sweeps plan (sweeps >= 0; -1: an exact plan, which has none of these): every row's storage range and the two vectors
    // a solve's iterates alternate between.  It has no d_level_ptr / d_order and no launches: the schedule is kept for the caller.
    int sweeps = -1;
    int *d_begin = nullptr, *d_end = nullptr;
    double *d_scratch[2] = {nullptr, nullptr};
};

extern "C" void smvp_trsv_destroy(smvp_trsv_t *t)
{
    if (!t)
        return;
    smvp::DeviceScope on(t->m.device);
    for (void *q : {(void *)t->d_level_ptr, (void *)t->d_order, (void *)t->d_begin, (void *)t->d_end, (void *)t->d_scratch[0],
                    (void *)t->d_scratch[1]})
        if (q)
            (void)hipFree(q);
    delete t;
}

namespace smvp {

namespace {

// smvp_csr_trsv_create (sweeps = -1) and smvp_csr_trsv_create_sweeps under the caller's name `fn`: the same checks, the same copy
// back of col_ind and the same host analysis; then the exact plan's schedule on the device, or K21's ranges and scratch vectors.
int trsv_create(const char *fn, smvp_trsv_t **out, const smvp_csr_t *h, int uplo, int diag, int sweeps, void *stream)
{
    if (!out)
        return fail(SMVP_ERR_INVALID, "%s: null out", fn);
    if (uplo != SMVP_TRSV_LOWER && uplo != SMVP_TRSV_UPPER)
        return fail(SMVP_ERR_INVALID, "%s: uplo = %d is neither SMVP_TRSV_LOWER nor SMVP_TRSV_UPPER", fn, uplo);
    if (diag != SMVP_TRSV_DIAG_STORED && diag != SMVP_TRSV_DIAG_UNIT)
        return fail(SMVP_ERR_INVALID, "%s: diag = %d is neither SMVP_TRSV_DIAG_STORED nor SMVP_TRSV_DIAG_UNIT", fn, diag);
    if (sweeps < -1 || sweeps > SMVP_TRSV_MAX_SWEEPS)
        return fail(SMVP_ERR_INVALID, "%s: sweeps = %d is outside [0, %d]", fn, sweeps, SMVP_TRSV_MAX_SWEEPS);
    if (!h)
        return fail(SMVP_ERR_INVALID, "%s: null handle", fn);
    const CsrView m = csr_view(h);
    if (m.flavor != kFlavorCsr)
        return fail(SMVP_ERR_UNSUPPORTED, "%s: plain CSR handles only (this one belongs to a TJDS matrix)", fn);
    if (m.first_row != 0)
        return fail(SMVP_ERR_UNSUPPORTED, "%s: a row block (first_row = %lld) holds no triangle of its own", fn, m.first_row);
    if (m.rows != m.cols)
        return fail(SMVP_ERR_INVALID, "%s: the handle's matrix is %d x %d, not square", fn, m.rows, m.cols);
    DeviceScope on(m.device);
    hipStream_t st = (hipStream_t)stream;
    const std::string why = std::string(fn) + ": the stream is capturing (the call copies back, allocates and waits: create the plan outside the capture)";
    if (int rc = refuse_capture(st, why.c_str()))
        return rc;
    const double t0 = wall_ms();
    std::vector<int> col((size_t)m.nnz);
    if (m.nnz > 0)
        HIP_TRY(hipMemcpyAsync(col.data(), m.d_col_ind, sizeof(int) * (size_t)m.nnz, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int asked = option("trsv_chain_width", kTrsvChainWidth);
    smvp_trsv *t = new smvp_trsv;
    t->m = m, t->uplo = uplo, t->diag = diag, t->sweeps = sweeps;
    int rc = trsv_analyse(m.rows, m.h_row_ptr, col.data(), uplo, &t->sched);
    const bool by_mean = option("trsv_lanes_by_mean", 0) != 0;
    if (sweeps < 0) {
        t->chain_width = asked >= 4 * kVectorBlock ? 4 * kVectorBlock : asked >= 2 * kVectorBlock ? 2 * kVectorBlock : kVectorBlock;
        if (rc == SMVP_OK)
            rc = upload(&t->d_level_ptr, t->sched.level_ptr);
        if (rc == SMVP_OK)
            rc = upload(&t->d_order, t->sched.order);
        if (rc == SMVP_OK) {
            trsv_launches(t->sched.level_ptr, t->chain_width, &t->launches, &t->chains);
            t->entries = t->sched.off_entries + (diag == SMVP_TRSV_DIAG_STORED ? t->sched.diag_entries : 0);
            // lanes a row of a wide level gets: from the geometric mean of the triangle's mean and longest row, over the chunk a lane
            // takes.  The mean alone (csr_vector_rows's rule) gave memplus, mean 4 and rows of up to 574, two lanes, and a level's
            // launch then lasts as long as its longest row's 72 passes; option trsv_lanes_by_mean = 1 keeps the mean's rule for the
            // comparison
            const double mean = m.rows > 0 ? (double)(t->sched.off_entries + t->sched.diag_entries) / m.rows : 0.0;
            t->lanes = pow2_lanes((by_mean ? mean : std::sqrt(mean * t->sched.max_row_entries)) / kTrsvChunk);
            t->plan_bytes = 4.0 * (double)(std::max<size_t>(t->sched.level_ptr.size(), 4) + std::max<size_t>(t->sched.order.size(), 4));
        }
    } else if (rc == SMVP_OK) {
        std::vector<int> begin, end;
        int longest = 0;
        trsv_ranges(m.rows, m.h_row_ptr, col.data(), uplo, diag, &begin, &end, &t->entries, &longest);
        rc = upload(&t->d_begin, begin);
        if (rc == SMVP_OK)
            rc = upload(&t->d_end, end);
        const size_t held = std::max<size_t>((size_t)m.rows, 4);
        auto scratch = [&](int k) {
            HIP_TRY(hipMalloc((void **)&t->d_scratch[k], held * sizeof(double)));
            return (int)SMVP_OK;
        };
        for (int k = 0; k < 2 && rc == SMVP_OK; ++k)
            rc = scratch(k);
        // lanes per row by K15's rule, from the ranges' mean and longest length
        const double mean = m.rows > 0 ? (double)t->entries / m.rows : 0.0;
        t->lanes = pow2_lanes((by_mean ? mean : std::sqrt(mean * longest)) / kTrsvChunk);
        t->plan_bytes = (double)held * (2.0 * sizeof(int) + 2.0 * sizeof(double));
    }
    if (rc != SMVP_OK) {
        smvp_trsv_destroy(t);
        return rc;
    }
    std::vector<int>().swap(t->sched.level_of_row);  // (the schedule is what a solve and smvp_trsv_schedule need)
    t->build_ms = wall_ms() - t0;
    *out = t;
    return SMVP_OK;
}

}  // namespace

}  // namespace smvp

extern "C" int smvp_csr_trsv_create(smvp_trsv_t **out, const smvp_csr_t *h, int uplo, int diag, void *stream)
{
    return smvp::trsv_create("smvp_csr_trsv_create", out, h, uplo, diag, -1, stream);
}

extern "C" int smvp_csr_trsv_create_sweeps(smvp_trsv_t **out, const smvp_csr_t *h, int uplo, int diag, int sweeps, void *stream)
{
    if (sweeps < 0)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_trsv_create_sweeps: sweeps = %d is outside [0, %d]", sweeps, SMVP_TRSV_MAX_SWEEPS);
    return smvp::trsv_create("smvp_csr_trsv_create_sweeps", out, h, uplo, diag, sweeps, stream);
}

extern "C" int smvp_trsv_sweeps(const smvp_trsv_t *t, int *sweeps)
{
    if (!t || !sweeps)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_trsv_sweeps: null %s", !t ? "plan" : "sweeps");
    *sweeps = t->sweeps;
    return SMVP_OK;
}

extern "C" int smvp_trsv_solve(smvp_trsv_t *t, const double *d_b, double *d_x, void *stream)
{
    using namespace smvp;
    if (!t)
        return fail(SMVP_ERR_INVALID, "smvp_trsv_solve: null plan");
    const int n = t->m.rows;
    if (n > 0 && (!d_b || !d_x))
        return fail(SMVP_ERR_INVALID, "smvp_trsv_solve: null %s", !d_b ? "d_b" : "d_x");
    if (d_b != d_x && operands_overlap(d_b, 1, n, d_x, 1, n, 1))
        return fail(SMVP_ERR_INVALID, "smvp_trsv_solve: the byte ranges of d_b and d_x overlap (d_x may be d_b itself, nothing between)");
    DeviceScope on(t->m.device);
    return trsv_enqueue("smvp_trsv_solve", t, d_b, d_x, (hipStream_t)stream);
}

int smvp::trsv_rows(const smvp_trsv_t *t) { return t->m.rows; }
int smvp::trsv_device(const smvp_trsv_t *t) { return t->m.device; }

// A solve's launches on `st`, for smvp_trsv_solve and for the solvers that apply a plan inside a step (K16 and K18, through
// krylov_apply): the operands are checked and the plan's device is current already.
int smvp::trsv_enqueue(const char *fn, smvp_trsv_t *t, const double *d_b, double *d_x, hipStream_t st)
{
    const int upper = t->uplo == SMVP_TRSV_UPPER, unit = t->diag == SMVP_TRSV_DIAG_UNIT;
    // K21: launch 0 writes x(0) from b alone; launch m reads b and scratch[(m - 1) & 1]; every launch but the last writes
    // scratch[m & 1], the last d_x.  d_x is never read, and every element of a scratch vector is written by the launch before the
    // one that reads it.
    for (int m = 0; t->sweeps >= 0 && t->m.rows > 0 && m <= t->sweeps; ++m) {
        const double *in = m ? t->d_scratch[(m - 1) & 1] : nullptr;
        double *out = m == t->sweeps ? d_x : t->d_scratch[m & 1];
        switch (t->lanes) {
        case 2: launch_sweep<2>(t->m, t->d_begin, t->d_end, d_b, in, out, unit, upper, st); break;
        case 4: launch_sweep<4>(t->m, t->d_begin, t->d_end, d_b, in, out, unit, upper, st); break;
        case 8: launch_sweep<8>(t->m, t->d_begin, t->d_end, d_b, in, out, unit, upper, st); break;
        case 16: launch_sweep<16>(t->m, t->d_begin, t->d_end, d_b, in, out, unit, upper, st); break;
        case 32: launch_sweep<32>(t->m, t->d_begin, t->d_end, d_b, in, out, unit, upper, st); break;
        default: launch_sweep<64>(t->m, t->d_begin, t->d_end, d_b, in, out, unit, upper, st); break;
        }
    }
    for (const TrsvLaunch &l : t->launches) {
        if (l.chain) {
            auto kernel = t->chain_width == kVectorBlock ? trsv_chain<1> : t->chain_width == 2 * kVectorBlock ? trsv_chain<2> : trsv_chain<4>;
            hipLaunchKernelGGL(kernel, dim3(1), dim3(kVectorBlock), 0, st, t->m.d_row_ptr, t->m.d_col_ind, t->m.d_val, t->d_level_ptr,
                               t->d_order, d_b, d_x, l.first, l.last, upper, unit);
            continue;
        }
        const long long lo = t->sched.level_ptr[(size_t)l.first], hi = t->sched.level_ptr[(size_t)l.last];
        switch (t->lanes) {
        case 2: launch_level<2>(t->m, t->d_order, d_b, d_x, lo, hi, upper, unit, st); break;
        case 4: launch_level<4>(t->m, t->d_order, d_b, d_x, lo, hi, upper, unit, st); break;
        case 8: launch_level<8>(t->m, t->d_order, d_b, d_x, lo, hi, upper, unit, st); break;
        case 16: launch_level<16>(t->m, t->d_order, d_b, d_x, lo, hi, upper, unit, st); break;
        case 32: launch_level<32>(t->m, t->d_order, d_b, d_x, lo, hi, upper, unit, st); break;
        default: launch_level<64>(t->m, t->d_order, d_b, d_x, lo, hi, upper, unit, st); break;
        }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(SMVP_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return SMVP_OK;
}

extern "C" int smvp_trsv_info(const smvp_trsv_t *t, smvp_trsv_info_t *out)
{
    if (!t || !out)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_trsv_info: null %s", !t ? "plan" : "out");
    if (out->struct_size != sizeof(smvp_trsv_info_t))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_trsv_info: struct_size = %u, this library's smvp_trsv_info_t has %zu bytes",
                          out->struct_size, sizeof(smvp_trsv_info_t));
    out->levels = t->sched.levels;
    out->max_level_width = t->sched.max_level_width;
    out->launches = t->sweeps < 0 ? (int)t->launches.size() : t->m.rows > 0 ? t->sweeps + 1 : 0;
    out->chains = t->chains;
    out->chain_width = t->chain_width;
    out->missing_diagonals = t->sched.missing_diagonals;
    out->lanes_per_row = t->lanes;
    out->entries = t->entries;
    out->plan_bytes = t->plan_bytes;
    out->build_ms = t->build_ms;
    return SMVP_OK;
}

extern "C" int smvp_trsv_schedule(const smvp_trsv_t *t, int *level_ptr, int *order)
{
    if (!t)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_trsv_schedule: null plan");
    if (level_ptr)
        std::copy(t->sched.level_ptr.begin(), t->sched.level_ptr.end(), level_ptr);
    if (order)
        std::copy(t->sched.order.begin(), t->sched.order.end(), order);
    return SMVP_OK;
}
