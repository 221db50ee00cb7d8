// smvp_ilu0.hip -- K17: the incomplete factorisation ILU(0) of a plain CSR handle's matrix on its own pattern (smvp_csr_ilu0_create,
// smvp_ilu0_factor; new: the reference only multiplies).  The factor F lives in ONE value array on A's row_ptr / col_ind: strictly
// below the diagonal L (unit diagonal implied), on and above it U -- what K15's LOWER / DIAG_UNIT and UPPER / DIAG_STORED plans
// solve with as stored.  Row i reads exactly the rows k < i for which (i, k) is stored: the dependency graph of the LOWER
// triangular solve, so the schedule and the launch shape are K15's (smvp_trsv_plan.cpp, smvp_trsv.hip): a launch per wide level,
// one workgroup with a barrier after every level per run of thin ones.  Every element of F is the serial loop's of the header,
// bit for bit: the pivots of a row in ascending k, one division by the final u_kk, every update the product rounded and then the
// difference rounded (-ffp-contract=off), an update whose column row i does not store skipped.
//
// NO KERNEL WAITS ON A VALUE ANOTHER WORKGROUP WRITES IN THE SAME LAUNCH: no flags, no grid barrier, no atomics.  Between
// workgroups the order is that of the kernel boundaries on the stream; inside the one workgroup of a chain it is __syncthreads(),
// as in trsv_chain.  Inside a row nothing goes from lane to lane through memory: every position t of row i has ONE owner lane for
// the whole row (offset j = t - row_ptr[i] belongs to lane j % T of the row's group of T lanes: neighbouring lanes, neighbouring
// entries), and the only thing the lanes of a group exchange is the multiplier l of the pivot at hand, by __shfl.
//
//   ilu0_row            a row by its group of T lanes (T = 1 .. 64, a power of two, inside one wavefront).  A row of at most
//                       kIluSlots * T entries lives in registers: the owner loads val_A[t] and col_ind[t] once, and stores F[t]
//                       once at the end.  The pivots are serial.  For the pivot at position p, column k: the owner of p divides its
//                       w[p] by F[diag_pos[k]] and hands l to the group; every lane then looks up, for each of its own t > p, column
//                       col_ind[t] in row k's upper part (diag_pos[k] + 1 .. row_ptr[k + 1]) by a binary search -- both rows are
//                       strictly ascending; the search is bounded by row k's length, and a lane's searches run side by side, their
//                       loads in flight together -- and subtracts l * F[q] where it matches.  The
//                       next pivot's column, diagonal position and row end depend on no value and are loaded a pivot ahead.
//                       A longer row (memplus has rows of 574 entries, spd_long of 700) keeps its w in F's own value array: each
//                       position is still read and written by its owner lane only, so same-thread program order is enough.
//   ilu0_level_rows<T>  one wide level: a group of T lanes per row of order[lo .. hi), T from the geometric mean of the mean and
//                       the longest row (K15's rule).  Tried and declined: 64 lanes a row for every wide level that holds a
//                       row too long for its registers, 12 entries a lane -- memplus x944 went from 102 to 183 ms, pwt x459 from
//                       5.2 to 6.8 (every short row of such a level then takes a wavefront).
//   ilu0_chain          a maximal run of levels of at most chain_width rows each: ONE workgroup, a barrier after every level.  A
//                       level of more than 128 rows gives every lane a row (and a second, third, fourth under the option
//                       trsv_chain_width); a thinner one gives every row a group of 2 .. 64 lanes.  A row that would need more
//                       than kIluLongTrips trips over its entries per pivot with those lanes (memplus's rows of hundreds of
//                       entries lie in its thin tail levels, where a level of more than 128 rows gave them ONE lane: 72 trips
//                       a pivot) is left out and taken by a whole wavefront afterwards, in front of the same barrier.  The loop over the levels is
//                       uniform and the barrier stands outside every branch.  Rows of earlier levels of the same chain are read
//                       from F, stored by other wavefronts in front of the barrier: K15's visibility argument.
//
// F is written and read in the same launch: its pointer is neither __restrict__ nor const, or the compiler could serve the reads
// from the scalar or read-only path and see stale values.  val_A, row_ptr, col_ind, order, level_ptr and diag_pos are only read.
#include "smvp_engine.h"

#include <cmath>

namespace smvp {

namespace {

constexpr int kIluChainWidth = kVectorBlock;  // as kTrsvChainWidth: the plan option trsv_chain_width says otherwise
constexpr int kIluSlots = 8;                  // entries of its row a lane keeps in registers (12 were tried with wider groups: slower, below)
constexpr int kIluLongTrips = 8;              // a chain leaves a row to a whole wavefront where its level's lanes would need more trips a pivot
constexpr int kIluChunk = 4;                  // K15's chunk in its lanes-per-row rule: the starting point the schedule shares

// Where each of U columns c[u] stands in col_ind[lo .. lo + n) (strictly ascending), or -1 (also where want[u] is false): U lower
// bounds side by side.  The number of turns depends on n alone -- len halves, rounding up, until it is 1 -- so the U searches
// take every turn together and their loads are in flight together; every load lies inside [lo, lo + n), whatever c[u] is.
// Invariant: the place of c[u], if it is stored, lies in [base[u], base[u] + len).
template <int U>
__device__ inline void ilu0_find(const int *__restrict__ col_ind, int lo, int n, const int (&c)[U], const bool (&want)[U], int (&q)[U])
{
    int base[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
        base[u] = lo;
    for (int len = n; len > 1; len -= len >> 1) {
        const int half = len >> 1;
        int cm[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            cm[u] = col_ind[base[u] + half - 1];
#pragma unroll
        for (int u = 0; u < U; ++u)
            base[u] = cm[u] < c[u] ? base[u] + half : base[u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
        q[u] = -1;
    if (n > 0) {
#pragma unroll
        for (int u = 0; u < U; ++u)
            q[u] = want[u] && col_ind[base[u]] == c[u] ? base[u] : -1;
    }
}

// what a pivot needs that depends on no value: its column k, where u_kk stands and where row k ends
struct IluPivot {
    int dk, zk;
};
__device__ inline IluPivot ilu0_pivot(const int *__restrict__ row_ptr, const int *__restrict__ col_ind, const int *__restrict__ diag_pos,
                                      int p, int end)
{
    IluPivot v{0, 0};
    if (p < end) {
        const int k = col_ind[p];
        v.dk = diag_pos[k];
        v.zk = row_ptr[k + 1];
    }
    return v;
}

// Row `row` (-1: none) by the group of T = 1 << lg lanes whose lanes lie at shift .. shift + T - 1 of the wavefront; `lane` is this
// lane's place in the group.  Every lane of the group takes the same branches and the same number of turns of the pivot loop (they
// depend on the row alone), so the group meets at every __shfl.
__device__ inline void ilu0_row(const int *__restrict__ row_ptr, const int *__restrict__ col_ind, const double *__restrict__ val,
                                const int *__restrict__ diag_pos, double *F, int row, int T, int lg, int lane, int shift)
{
    if (row < 0)
        return;
    const int a = row_ptr[row], z = row_ptr[row + 1], dp = diag_pos[row];  // the pivots stand at a .. dp - 1: the columns below `row`
    if (z - a <= kIluSlots * T) {
        int c[kIluSlots];
        double w[kIluSlots];
#pragma unroll
        for (int s = 0; s < kIluSlots; ++s) {
            const int t = a + s * T + lane;
            c[s] = t < z ? col_ind[t] : -1;
            w[s] = t < z ? val[t] : 0.0;
        }
        IluPivot at = ilu0_pivot(row_ptr, col_ind, diag_pos, a, dp);
        for (int p = a; p < dp; ++p) {
            const IluPivot next = ilu0_pivot(row_ptr, col_ind, diag_pos, p + 1, dp);
            const double ukk = F[at.dk];  // row k is final: an earlier launch's, or stored in front of a barrier
            const int owner = (p - a) & (T - 1), slot = (p - a) >> lg;
            double wp = 0.0;
#pragma unroll
            for (int s = 0; s < kIluSlots; ++s)
                wp = s == slot ? w[s] : wp;
            const double l = __shfl(wp / ukk, shift + owner);  // (the owner's quotient; the other lanes' is thrown away)
            bool want[kIluSlots];
            int q[kIluSlots];
#pragma unroll
            for (int s = 0; s < kIluSlots; ++s) {
                const int t = a + s * T + lane;
                want[s] = t > p && t < z;
                w[s] = t == p ? l : w[s];
            }
            if (at.zk > at.dk + 1) {  // (row k has an upper part: the same for the whole group)
                ilu0_find<kIluSlots>(col_ind, at.dk + 1, at.zk - at.dk - 1, c, want, q);
                double u[kIluSlots];
#pragma unroll
                for (int s = 0; s < kIluSlots; ++s)
                    u[s] = q[s] >= 0 ? F[q[s]] : 0.0;
#pragma unroll
                for (int s = 0; s < kIluSlots; ++s)
                    if (q[s] >= 0)
                        w[s] = w[s] - l * u[s];  // the product rounded, then the difference: no FMA; no match, no update
            }
            at = next;
        }
#pragma unroll
        for (int s = 0; s < kIluSlots; ++s) {
            const int t = a + s * T + lane;
            if (t < z)
                F[t] = w[s];
        }
        return;
    }
    // a row too long for the group's registers: w lives in F, every position read and written by its owner lane only
    for (int t = a + lane; t < z; t += T)
        F[t] = val[t];
    IluPivot at = ilu0_pivot(row_ptr, col_ind, diag_pos, a, dp);
    for (int p = a; p < dp; ++p) {
        const IluPivot next = ilu0_pivot(row_ptr, col_ind, diag_pos, p + 1, dp);
        const double ukk = F[at.dk];
        const int owner = (p - a) & (T - 1);
        double l = 0.0;
        if (lane == owner) {
            l = F[p] / ukk;
            F[p] = l;
        }
        l = __shfl(l, shift + owner);
        const int j0 = p - a + 1;  // the first offset beyond the pivot; this lane's first one from there on, kIluSlots at a time:
        if (at.zk > at.dk + 1)
            for (int t0 = a + j0 + ((lane - j0) & (T - 1)); t0 < z; t0 += kIluSlots * T) {
                int c[kIluSlots], q[kIluSlots];
                bool want[kIluSlots];
#pragma unroll
                for (int s = 0; s < kIluSlots; ++s) {
                    want[s] = t0 + s * T < z;
                    c[s] = want[s] ? col_ind[t0 + s * T] : -1;
                }
                ilu0_find<kIluSlots>(col_ind, at.dk + 1, at.zk - at.dk - 1, c, want, q);
                double u[kIluSlots], w[kIluSlots];
#pragma unroll
                for (int s = 0; s < kIluSlots; ++s) {
                    u[s] = q[s] >= 0 ? F[q[s]] : 0.0;
                    w[s] = q[s] >= 0 ? F[t0 + s * T] : 0.0;
                }
#pragma unroll
                for (int s = 0; s < kIluSlots; ++s)
                    if (q[s] >= 0)
                        F[t0 + s * T] = w[s] - l * u[s];
            }
        at = next;
    }
}

template <int T>
__global__ __launch_bounds__(kVectorBlock) void ilu0_level_rows(const int *__restrict__ row_ptr, const int *__restrict__ col_ind,
                                                                 const double *__restrict__ val, const int *__restrict__ order,
                                                                 const int *__restrict__ diag_pos, double *F, long long lo, long long hi)
{
    constexpr int lg = T == 1 ? 0 : T == 2 ? 1 : T == 4 ? 2 : T == 8 ? 3 : T == 16 ? 4 : T == 32 ? 5 : 6;
    const long long k = lo + ((long long)blockIdx.x * kVectorBlock + threadIdx.x) / T;
    const int row = k < hi ? order[k] : -1;
    ilu0_row(row_ptr, col_ind, val, diag_pos, F, row, T, lg, threadIdx.x & (T - 1), threadIdx.x & 63 & ~(T - 1));
}

// lanes a row of a chain's level of `width` rows gets: trsv_chain_lanes's rule
__device__ inline int ilu0_chain_lanes(int width)
{
    const int q = kVectorBlock / (width > 0 ? width : 1);
    return q >= 64 ? 64 : q >= 2 ? 1 << (31 - __builtin_clz(q)) : 1;
}

// Is a row of `len` entries too long for the T lanes its level would give it in a chain -- more than kIluLongTrips trips over its
// entries per pivot?  Such a row is left to a whole wavefront (ilu0_chain's second part).
__device__ inline bool ilu0_long(int len, int T) { return T < 64 && len > kIluLongTrips * kIluSlots * T; }

__global__ __launch_bounds__(kVectorBlock) void ilu0_chain(const int *__restrict__ row_ptr, const int *__restrict__ col_ind,
                                                            const double *__restrict__ val, const int *__restrict__ level_ptr,
                                                            const int *__restrict__ order, const int *__restrict__ diag_pos, double *F,
                                                            int l0, int l1)
{
    const int t = threadIdx.x;
    for (int l = l0; l < l1; ++l) {  // uniform: every lane of the workgroup takes every turn and reaches every barrier
        const int lo = level_ptr[l], hi = level_ptr[l + 1];
        const int T = ilu0_chain_lanes(hi - lo);
        if (T > 1) {  // a thin level: the group of T lanes t / T takes row t / T
            const int k = lo + t / T;
            int row = k < hi ? order[k] : -1;
            if (row >= 0 && ilu0_long(row_ptr[row + 1] - row_ptr[row], T))
                row = -1;  // (the same for the whole group)
            ilu0_row(row_ptr, col_ind, val, diag_pos, F, row, T, 31 - __builtin_clz(T), t & (T - 1), t & 63 & ~(T - 1));
        } else {
            for (int k = lo + t; k < hi; k += kVectorBlock) {  // a row per lane (the host put no level of more than four into a chain)
                const int row = order[k];
                if (!ilu0_long(row_ptr[row + 1] - row_ptr[row], 1))
                    ilu0_row(row_ptr, col_ind, val, diag_pos, F, row, 1, 0, 0, t & 63);
            }
        }
        // the level's long rows, a wavefront each, dealt to the workgroup's wavefronts in turn.  Every wavefront goes through the
        // level 64 rows at a time and finds the long ones by a ballot, so which rows are whose needs no list and no memory; the
        // ballot's mask and the count are the same in every lane, and rows of one level do not depend on each other
        if (T < 64) {
            const int wave = t >> 6, lane = t & 63;
            int seen = 0;
            for (int base = lo; base < hi; base += 64) {
                const int k = base + lane;
                bool is_long = false;
                if (k < hi) {
                    const int row = order[k];
                    is_long = ilu0_long(row_ptr[row + 1] - row_ptr[row], T);
                }
                for (unsigned long long mask = __ballot(is_long); mask; mask &= mask - 1)
                    if ((seen++ & (kVectorBlock / 64 - 1)) == wave)
                        ilu0_row(row_ptr, col_ind, val, diag_pos, F, order[base + __ffsll((long long)mask) - 1], 64, 6, lane, 0);
            }
        }
        __syncthreads();
    }
}

template <int T>
void launch_level(const CsrView &m, const int *order, const int *diag_pos, double *F, long long lo, long long hi, hipStream_t stream)
{
    const long long chunk = ((long long)1 << 31) / T;  // (a launch of fewer than 2^32 threads)
    for (long long k0 = lo; k0 < hi; k0 += chunk) {
        const long long n = hi - k0 < chunk ? hi - k0 : chunk;
        const unsigned grid = (unsigned)((n * T + kVectorBlock - 1) / kVectorBlock);
        hipLaunchKernelGGL(ilu0_level_rows<T>, dim3(grid), dim3(kVectorBlock), 0, stream, m.d_row_ptr, m.d_col_ind, m.d_val, order,
                           diag_pos, F, k0, k0 + n);
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

struct smvp_ilu0 {
    smvp::CsrView m{};  // A: its arrays are borrowed, val is read at every factorisation
    smvp_csr_t *F = nullptr;  // the factor as a handle: adopts A's row_ptr / col_ind and d_val below
    double *d_val = nullptr;
    int *d_level_ptr = nullptr, *d_order = nullptr, *d_diag_pos = nullptr;
    int lanes = 2, chains = 0, chain_width = 0;
    smvp::TrsvSchedule sched;
    std::vector<smvp::TrsvLaunch> launches;
    long long pivots = 0;
    double plan_bytes = 0.0, build_ms = 0.0;
};

namespace {

// one factorisation's launches on `st`: the device is current already
int ilu0_enqueue(const char *fn, const smvp_ilu0 *f, hipStream_t st)
{
    using namespace smvp;
    for (const TrsvLaunch &l : f->launches) {
        if (l.chain) {
            hipLaunchKernelGGL(ilu0_chain, dim3(1), dim3(kVectorBlock), 0, st, f->m.d_row_ptr, f->m.d_col_ind, f->m.d_val, f->d_level_ptr,
                               f->d_order, f->d_diag_pos, f->d_val, l.first, l.last);
            continue;
        }
        const long long lo = f->sched.level_ptr[(size_t)l.first], hi = f->sched.level_ptr[(size_t)l.last];
        switch (f->lanes) {
        case 2: launch_level<2>(f->m, f->d_order, f->d_diag_pos, f->d_val, lo, hi, st); break;
        case 4: launch_level<4>(f->m, f->d_order, f->d_diag_pos, f->d_val, lo, hi, st); break;
        case 8: launch_level<8>(f->m, f->d_order, f->d_diag_pos, f->d_val, lo, hi, st); break;
        case 16: launch_level<16>(f->m, f->d_order, f->d_diag_pos, f->d_val, lo, hi, st); break;
        case 32: launch_level<32>(f->m, f->d_order, f->d_diag_pos, f->d_val, lo, hi, st); break;
        default: launch_level<64>(f->m, f->d_order, f->d_diag_pos, f->d_val, lo, hi, st); break;
        }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(SMVP_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return SMVP_OK;
}

}  // namespace

extern "C" void smvp_ilu0_destroy(smvp_ilu0_t *f)
{
    if (!f)
        return;
    smvp::DeviceScope on(f->m.device);
    smvp_csr_destroy(f->F);  // (it adopted its arrays: none of them is freed there)
    for (void *q : {(void *)f->d_val, (void *)f->d_level_ptr, (void *)f->d_order, (void *)f->d_diag_pos})
        if (q)
            (void)hipFree(q);
    delete f;
}

extern "C" int smvp_csr_ilu0_create(smvp_ilu0_t **out, const smvp_csr_t *h, void *stream)
{
    using namespace smvp;
    if (!out || !h)
        return fail(SMVP_ERR_INVALID, "smvp_csr_ilu0_create: null %s", !out ? "out" : "handle");
    const CsrView m = csr_view(h);
    if (m.flavor != kFlavorCsr)
        return fail(SMVP_ERR_UNSUPPORTED, "smvp_csr_ilu0_create: plain CSR handles only (this one belongs to a TJDS matrix)");
    if (m.first_row != 0)
        return fail(SMVP_ERR_UNSUPPORTED, "smvp_csr_ilu0_create: a row block (first_row = %lld) holds no pivots of its own", m.first_row);
    if (m.rows != m.cols)
        return fail(SMVP_ERR_INVALID, "smvp_csr_ilu0_create: the handle's matrix is %d x %d, not square", m.rows, m.cols);
    DeviceScope on(m.device);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = refuse_capture(st, "smvp_csr_ilu0_create: the stream is capturing (the call copies back, allocates and waits: create the "
                                    "factorisation outside the capture)"))
        return rc;
    const double t0 = wall_ms();
    std::vector<int> col((size_t)m.nnz);
    if (m.nnz > 0)
        HIP_TRY(hipMemcpyAsync(col.data(), m.d_col_ind, sizeof(int) * (size_t)m.nnz, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<int> diag_pos((size_t)m.rows);
    if (int rc = ilu0_check("smvp_csr_ilu0_create", m.rows, m.h_row_ptr, col.data(), diag_pos.data(), nullptr))
        return rc;
    const int asked = option("trsv_chain_width", kIluChainWidth);
    smvp_ilu0 *f = new smvp_ilu0;
    f->m = m;
    f->chain_width = asked >= 4 * kVectorBlock ? 4 * kVectorBlock : asked >= 2 * kVectorBlock ? 2 * kVectorBlock : kVectorBlock;
    int rc = trsv_analyse(m.rows, m.h_row_ptr, col.data(), SMVP_TRSV_LOWER, &f->sched);
    if (rc == SMVP_OK)
        rc = upload(&f->d_level_ptr, f->sched.level_ptr);
    if (rc == SMVP_OK)
        rc = upload(&f->d_order, f->sched.order);
    if (rc == SMVP_OK)
        rc = upload(&f->d_diag_pos, diag_pos);
    if (rc == SMVP_OK && hipMalloc((void **)&f->d_val, sizeof(double) * std::max<size_t>((size_t)m.nnz, 4)) != hipSuccess)
        rc = fail(SMVP_ERR_HIP, "smvp_csr_ilu0_create: no device memory for the factor's %d values", m.nnz);
    if (rc == SMVP_OK) {
        std::vector<int>().swap(f->sched.level_of_row);
        trsv_launches(f->sched.level_ptr, f->chain_width, &f->launches, &f->chains);
        f->pivots = f->sched.off_entries;
        // lanes a row of a wide level gets: K15's rule on the whole rows -- the geometric mean of the mean and the longest row, over
        // K15's chunk.  A row of up to kIluSlots times as many entries stays in registers
        int longest = 0;
        for (int i = 0; i < m.rows; ++i)
            longest = std::max(longest, m.h_row_ptr[i + 1] - m.h_row_ptr[i]);
        const double mean = m.rows > 0 ? (double)m.nnz / m.rows : 0.0;
        f->lanes = pow2_lanes(std::sqrt(mean * longest) / kIluChunk);
        rc = ilu0_enqueue("smvp_csr_ilu0_create", f, st);  // the first factorisation: F is valid on return, and before its handle is planned
    }
    if (rc == SMVP_OK && hipStreamSynchronize(st) != hipSuccess)
        rc = fail(SMVP_ERR_HIP, "smvp_csr_ilu0_create: the first factorisation failed: %s", hipGetErrorString(hipGetLastError()));
    if (rc == SMVP_OK)
        rc = smvp_csr_create(&f->F, m.device, m.rows, m.cols, m.nnz, m.d_row_ptr, m.d_col_ind, f->d_val, SMVP_MEM_DEVICE, m.h_row_ptr);
    if (rc != SMVP_OK) {
        smvp_ilu0_destroy(f);
        return rc;
    }
    f->plan_bytes = 8.0 * (double)std::max<size_t>((size_t)m.nnz, 4) +
                    4.0 * (double)(std::max<size_t>(f->sched.level_ptr.size(), 4) + 2 * std::max<size_t>((size_t)m.rows, 4));
    f->build_ms = wall_ms() - t0;
    *out = f;
    return SMVP_OK;
}

extern "C" int smvp_ilu0_factor(smvp_ilu0_t *f, void *stream)
{
    if (!f)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_ilu0_factor: null factorisation");
    smvp::DeviceScope on(f->m.device);
    return ilu0_enqueue("smvp_ilu0_factor", f, (hipStream_t)stream);
}

extern "C" int smvp_ilu0_matrix(const smvp_ilu0_t *f, smvp_csr_t **F)
{
    if (!f || !F)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_ilu0_matrix: null %s", !f ? "factorisation" : "F");
    *F = f->F;
    return SMVP_OK;
}

extern "C" int smvp_ilu0_info(const smvp_ilu0_t *f, smvp_ilu0_info_t *out)
{
    if (!f || !out)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_ilu0_info: null %s", !f ? "factorisation" : "out");
    if (out->struct_size != sizeof(smvp_ilu0_info_t))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_ilu0_info: struct_size = %u, this library's smvp_ilu0_info_t has %zu bytes",
                          out->struct_size, sizeof(smvp_ilu0_info_t));
    out->levels = f->sched.levels;
    out->max_level_width = f->sched.max_level_width;
    out->launches = (int)f->launches.size();
    out->chains = f->chains;
    out->chain_width = f->chain_width;
    out->lanes_per_row = f->lanes;
    out->entries = f->m.nnz;
    out->pivots = f->pivots;
    out->plan_bytes = f->plan_bytes;
    out->build_ms = f->build_ms;
    return SMVP_OK;
}
