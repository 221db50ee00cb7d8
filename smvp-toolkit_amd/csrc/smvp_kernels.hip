// smvp_kernels.hip -- the CDNA4 (gfx950) SpMV kernels that are not the owner (tile) kernel or the column sweep: K1 (a
// sub-wavefront per row), the carry form of the tile kernel (csr_stream_tiles + csr_stream_carry_fixup), K3 (TJDS, column-major),
// the utility kernels and the line-spread probe, with their launchers.  The owner kernel K2' is smvp_owner_kernel.h, launched
// from smvp_owner.hip and smvp_owner_csr.hip; K4 is smvp_colsweep.hip.  Every file is compiled once: the Makefile says which
// two get the max-ILP scheduling strategy, and this one is not among them.
//
// The kernels of these files replace the two timed loops of the reference:
//   CSR   main-cli.c:410-416    for row: for j: y[row] += val[j] * x[col_ind[j]]
//   TJDS  main-cli.c:1013-1020  for diag: for j: y[row_ind[j]] += val[j] * x_perm[...]
// Both are HBM-bound streaming + gather/scatter work (2 flop per 12 B), so there
// is no MFMA here: what matters is that val/col_ind/row_ind are read exactly
// once with wide coalesced loads, that x is gathered through L2 / Infinity Cache,
// and that y is written once.
//
// Compiled with -ffp-contract=off: a product is rounded before it is added,
// like the reference's x86-64 build, so every row that is summed left to right
// by one lane is bit-identical to the serial CPU result.
#include "smvp_kernels.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace smvp {

// ---------------------------------------------------------------------------
// K1: CSR, one sub-wavefront of T lanes per row, __shfl_down sums.
// T = 64 is the classic wavefront-per-row kernel; smaller T packs 64/T rows
// into a wave for short rows.  Lane l of a row reads entries a+l, a+l+T, ...
// so a wave's loads are contiguous runs of col_ind / val.
// ---------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(kVectorBlock) void csr_vector_rows(
    const int *__restrict__ row_ptr, const int *__restrict__ col_ind, const double *__restrict__ val,
    const double *__restrict__ x, double *__restrict__ y, int rows, int row0)
{
    const long long gid = (long long)blockIdx.x * kVectorBlock + threadIdx.x;
    const long long row = row0 + gid / T;  // (launched in row chunks: a grid holds fewer than 2^32 threads)
    const int lane = threadIdx.x & (T - 1);
    int a = 0, z = 0;
    if (row < rows) {
        a = row_ptr[row];
        z = row_ptr[row + 1];
    }
    double acc = 0.0;
    for (int j = a + lane; j < z; j += T)
        acc += val[j] * x[col_ind[j]];
    acc = shfl_down_sum<T>(acc);
    if (lane == 0 && row < rows)
        y[row] = acc;
}

// ---------------------------------------------------------------------------
// K2: CSR, fixed-nnz tiles with an LDS-staged segmented reduction.
//
// Tile b owns entries [b*TILE, (b+1)*TILE): every block streams the same number
// of bytes whatever the row lengths are (memplus: 86 % of rows <= 8 entries,
// 28 % of entries in rows > 64).  Phase 1 loads col_ind / val with 16-byte
// per-lane loads, gathers x and parks the products in LDS.  Phase 2 walks the
// rows that START inside the tile (tile_row[b] .. tile_row[b+1]): one lane per
// short row sums its segment left to right out of LDS; rows longer than
// kLongRow are queued and summed by a whole wavefront with __shfl_down.
// Entries in front of the first owned row belong to a row that started in an
// earlier tile: their sum goes to carry[b] and csr_stream_carry_fixup adds the
// carries to y in tile order, so the result does not depend on timing and y
// needs no zeroing.
// ---------------------------------------------------------------------------
template <int VPT>
__global__ __launch_bounds__(kStreamBlock) void csr_stream_tiles(
    const int *__restrict__ row_ptr, const int *__restrict__ col_ind, const double *__restrict__ val,
    const double *__restrict__ x, double *__restrict__ y, const int *__restrict__ tile_row,
    double *__restrict__ carry, int rows, int nnz, int ntiles, int tile_group)
{
    constexpr int TILE = kStreamBlock * VPT;
    constexpr int QCAP = TILE / kLongRow + 1;
    __shared__ double prod[TILE];
    __shared__ int long_rows[QCAP];
    __shared__ int long_count;

    const int b = tile_of_block(blockIdx.x, tile_group);
    if (b >= ntiles)
        return;
    const int t = threadIdx.x;
    const long long s = (long long)b * TILE;
    const int e = (int)(s + TILE < (long long)nnz ? s + TILE : (long long)nnz);
    if (t == 0)
        long_count = 0;
    const int rlo = tile_row[b];
    const int rhi = tile_row[b + 1];

    // ---- phase 1: stream + gather + multiply.  The full-tile path is straight-line code so that
    // all VPT gathers of a lane are in flight together; a guarded version that branched per entry
    // ran 12-25 % slower (MI355X, memplus x944).
    const long long j0 = s + (long long)t * VPT;
    double p[VPT];
    if (j0 + VPT <= (long long)nnz) {
        int c[VPT];
        double v[VPT];
#pragma unroll
        for (int k = 0; k < VPT; k += 4)
            *reinterpret_cast<int4 *>(&c[k]) = *reinterpret_cast<const int4 *>(col_ind + j0 + k);
#pragma unroll
        for (int k = 0; k < VPT; k += 2)
            *reinterpret_cast<double2 *>(&v[k]) = *reinterpret_cast<const double2 *>(val + j0 + k);
#pragma unroll
        for (int k = 0; k < VPT; ++k)
            p[k] = v[k] * x[c[k]];
    } else {
#pragma unroll
        for (int k = 0; k < VPT; ++k)
            p[k] = (j0 + k < (long long)nnz) ? val[j0 + k] * x[col_ind[j0 + k]] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < VPT; k += 2)
        *reinterpret_cast<double2 *>(&prod[t * VPT + k]) = make_double2(p[k], p[k + 1]);
    __syncthreads();

    // ---- phase 2a: the head of the tile continues an earlier row
    const int lo = (int)s;  // nnz < 2^31
    if (t < 64) {
        const int first = rlo < rows ? row_ptr[rlo] : nnz;
        const int head = (first < e ? first : e) - lo;
        double acc = 0.0;
        for (int i = t; i < head; i += 64)
            acc += prod[i];
        acc = shfl_down_sum<64>(acc);
        if (t == 0)
            carry[b] = acc;
    }

    // ---- phase 2b: one lane per owned row, long rows deferred
    for (int r = rlo + t; r < rhi; r += kStreamBlock) {
        const int a = row_ptr[r];
        const int nxt = row_ptr[r + 1];
        const int z = nxt < e ? nxt : e;
        if (z - a <= kLongRow) {
            double acc = 0.0;
            for (int i = a - lo; i < z - lo; ++i)
                acc += prod[i];
            y[r] = acc;
        } else {
            long_rows[atomicAdd(&long_count, 1)] = r;
        }
    }
    __syncthreads();

    // ---- phase 2c: one wavefront per long row
    const int nlong = long_count;
    const int lane = t & 63;
    for (int q = t >> 6; q < nlong; q += kStreamBlock / 64) {
        const int r = long_rows[q];
        const int a = row_ptr[r];
        const int nxt = row_ptr[r + 1];
        const int z = nxt < e ? nxt : e;
        double acc = 0.0;
        for (int i = a - lo + lane; i < z - lo; i += 64)
            acc += prod[i];
        acc = shfl_down_sum<64>(acc);
        if (lane == 0)
            y[r] = acc;
    }
}

// One thread per tile; the head of each run of tiles that feed the same row adds
// their carries to that row in tile order.
__global__ __launch_bounds__(256) void csr_stream_carry_fixup(
    const int *__restrict__ carry_row, const double *__restrict__ carry, double *__restrict__ y, int ntiles)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= ntiles)
        return;
    const int r = carry_row[b];
    if (r < 0 || (b > 0 && carry_row[b - 1] == r))
        return;
    double acc = y[r];
    for (int k = b; k < ntiles && carry_row[k] == r; ++k)
        acc += carry[k];
    y[r] = acc;
}

// ---------------------------------------------------------------------------
// K3: TJDS, column-major.  Thread k of a block is permuted column k0 + k: it
// keeps x_perm[k] in a register and walks down its column, one jagged diagonal
// per step, so that at every step the block reads one contiguous run of val /
// row_ind.  The products scatter into y with hardware fp64 atomics (y zeroed by
// the caller, like main-cli.c:1008).  Work items cut the (column block,
// diagonal range) plane into pieces of at most kTjdsBlock x kTjdsDiagChunk
// entries so the few long columns do not serialise the launch.
// ---------------------------------------------------------------------------
template <bool OPERAND_BY_ROW>
__global__ __launch_bounds__(kTjdsBlock) void tjds_colmajor_scatter(
    const int *__restrict__ start_pos, const int *__restrict__ row_ind, const double *__restrict__ val,
    const double *__restrict__ x_perm, double *__restrict__ y, const int4 *__restrict__ work, int cols)
{
    const int4 w = work[blockIdx.x];  // x = first column, y = first diagonal, z = one past the last
    const int k = w.x + threadIdx.x;
    const double xk = (!OPERAND_BY_ROW && k < cols) ? x_perm[k] : 0.0;
    // all loads of the chunk first (they are independent), then the atomics: a loop that
    // loaded and added one diagonal at a time paid one memory round trip per diagonal
    int r[kTjdsDiagChunk];
    double v[kTjdsDiagChunk];
#pragma unroll
    for (int i = 0; i < kTjdsDiagChunk; ++i) {
        const int d = w.y + i;
        r[i] = -1;
        v[i] = 0.0;
        if (d < w.z) {
            const int base = start_pos[d];
            if (k < start_pos[d + 1] - base) {  // diagonal lengths never grow with d
                r[i] = row_ind[base + k];
                v[i] = val[base + k];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kTjdsDiagChunk; ++i) {
        if (r[i] >= 0) {
            // main-cli.c:1018 indexes the permuted operand by the row; the corrected
            // product uses the column's own entry
            const double xv = OPERAND_BY_ROW ? x_perm[r[i]] : xk;
            unsafeAtomicAdd(&y[r[i]], v[i] * xv);
        }
    }
}

// K3': the atomic-free TJDS product, phase 1.  Same traversal as tjds_colmajor_scatter -- thread k of a
// work item is permuted column k0 + k, holds x_perm[k] in a register and walks down its column -- but the
// product of entry j is stored to prod[j] (plain, coalesced store; row_ind is not even read).  Phase 2 sums
// each row's products through the row-inverted index built at create time (csr_stream_owner<4, true>):
// "store every contribution once, then sum per destination", fixed order, so the result is bit-reproducible
// and y needs no zeroing.
__global__ __launch_bounds__(kTjdsBlock) void tjds_colmajor_products(
    const int *__restrict__ start_pos, const double *__restrict__ val, const double *__restrict__ x_perm,
    double *__restrict__ prod, const int4 *__restrict__ work, int cols)
{
    const int4 w = work[blockIdx.x];
    const int k = w.x + threadIdx.x;
    const double xk = k < cols ? x_perm[k] : 0.0;
    int j[kTjdsDiagChunk];
    double v[kTjdsDiagChunk];
#pragma unroll
    for (int i = 0; i < kTjdsDiagChunk; ++i) {
        const int d = w.y + i;
        j[i] = -1;
        v[i] = 0.0;
        if (d < w.z) {
            const int base = start_pos[d];
            if (k < start_pos[d + 1] - base) {
                j[i] = base + k;
                v[i] = val[base + k];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kTjdsDiagChunk; ++i)
        if (j[i] >= 0)
            __builtin_nontemporal_store(v[i] * xk, &prod[j[i]]);
}

__global__ __launch_bounds__(256) void tjds_permute_operand(
    const int *__restrict__ perm, const double *__restrict__ x, double *__restrict__ x_perm, int cols)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < cols)
        x_perm[k] = x[perm[k]];
}

// first index (plus one) whose value lies outside [0, limit): adopted device arrays are checked
// before any kernel indexes with them
__global__ __launch_bounds__(256) void find_out_of_range(const int *__restrict__ a, long long n, int limit,
                                                          int *__restrict__ bad)
{
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int v = a[i];
        if (v < 0 || v >= limit)
            atomicMax(bad, (int)(i < 2147483646ll ? i + 1 : 2147483647ll));
    }
}

// max |v[i]| as the bit pattern of a non-negative double (those order like unsigned integers); *bits = 0 first
__global__ __launch_bounds__(256) void vector_absmax(const double *__restrict__ v, long long n,
                                                      unsigned long long *__restrict__ bits)
{
    double m = 0.0;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const double a = fabs(v[i]);
        m = a > m ? a : m;  // NaN entries are skipped
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(m, off, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0)
        atomicMax(bits, (unsigned long long)__double_as_longlong(m));
}

__global__ __launch_bounds__(256) void vector_divide(double *__restrict__ v, long long n,
                                                      const unsigned long long *__restrict__ bits)
{
    const double m = __longlong_as_double((long long)*bits);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && m > 0.0)
        v[i] = v[i] / m;
}

__global__ __launch_bounds__(256) void fill_value(double *__restrict__ p, double v, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n)
        p[i] = v;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
// rows [row0, row0 + n) of the vector kernel: one launch of n * lanes_per_row threads
static hipError_t launch_csr_vector_rows(int lanes_per_row, const int *row_ptr, const int *col_ind, const double *val,
                                         const double *x, double *y, int rows, int row0, int n, hipStream_t stream)
{
    const unsigned grid = (unsigned)(((long long)n * lanes_per_row + kVectorBlock - 1) / kVectorBlock);
#define SMVP_VEC_CASE(T)                                                                              \
    case T:                                                                                           \
        hipLaunchKernelGGL(csr_vector_rows<T>, dim3(grid), dim3(kVectorBlock), 0, stream, row_ptr,   \
                           col_ind, val, x, y, rows, row0);                                           \
        break;
    switch (lanes_per_row) {
        SMVP_VEC_CASE(2)
        SMVP_VEC_CASE(4)
        SMVP_VEC_CASE(8)
        SMVP_VEC_CASE(16)
        SMVP_VEC_CASE(32)
        SMVP_VEC_CASE(64)
    default:
        return hipErrorInvalidValue;
    }
#undef SMVP_VEC_CASE
    return hipGetLastError();
}

hipError_t launch_csr_vector(int lanes_per_row, const int *row_ptr, const int *col_ind, const double *val,
                             const double *x, double *y, int rows, hipStream_t stream)
{
    if (lanes_per_row < 1)
        return hipErrorInvalidValue;
    // at most 2^31 threads per launch (a multiple of the block): 32 or 64 lanes for each of 2^27 rows would pass the 2^32
    // threads a grid may hold
    const int chunk = (int)(((long long)1 << 31) / lanes_per_row);
    for (int row0 = 0; row0 < rows; row0 += chunk) {
        const int n = std::min(chunk, rows - row0);
        if (hipError_t e = launch_csr_vector_rows(lanes_per_row, row_ptr, col_ind, val, x, y, rows, row0, n, stream))
            return e;
        if (rows - row0 <= chunk)
            break;  // (row0 + chunk may not fit an int)
    }
    return hipSuccess;
}

hipError_t launch_csr_stream(int vpt, const int *row_ptr, const int *col_ind, const double *val,
                             const double *x, double *y, const int *tile_row, const int *carry_row,
                             double *carry, int rows, int nnz, int ntiles, hipStream_t stream)
{
    if (rows <= 0)
        return hipSuccess;
    const int group = tile_group(ntiles);
    const dim3 grid((unsigned)((ntiles + 8 * group - 1) / (8 * group)) * 8u * group);
    switch (vpt) {
    case 4:
        hipLaunchKernelGGL(csr_stream_tiles<4>, grid, dim3(kStreamBlock), 0, stream, row_ptr, col_ind, val, x, y,
                           tile_row, carry, rows, nnz, ntiles, group);
        break;
    case 8:
        hipLaunchKernelGGL(csr_stream_tiles<8>, grid, dim3(kStreamBlock), 0, stream, row_ptr, col_ind, val, x, y,
                           tile_row, carry, rows, nnz, ntiles, group);
        break;
    default:
        return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    if (ntiles > 1) {
        hipLaunchKernelGGL(csr_stream_carry_fixup, dim3((ntiles + 255) / 256), dim3(256), 0, stream, carry_row,
                           carry, y, ntiles);
        e = hipGetLastError();
    }
    return e;
}

hipError_t launch_tjds_products(const int *start_pos, const double *val, const double *x_perm, double *prod,
                                const int4 *work, int nwork, int cols, hipStream_t stream)
{
    if (nwork <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(tjds_colmajor_products, dim3(nwork), dim3(kTjdsBlock), 0, stream, start_pos, val, x_perm, prod,
                       work, cols);
    return hipGetLastError();
}

hipError_t launch_tjds_scatter(bool operand_by_row, const int *start_pos, const int *row_ind, const double *val,
                               const double *x_perm, double *y, const int4 *work, int nwork, int cols,
                               hipStream_t stream)
{
    if (nwork <= 0)
        return hipSuccess;
    if (operand_by_row)
        hipLaunchKernelGGL(tjds_colmajor_scatter<true>, dim3(nwork), dim3(kTjdsBlock), 0, stream, start_pos,
                           row_ind, val, x_perm, y, work, cols);
    else
        hipLaunchKernelGGL(tjds_colmajor_scatter<false>, dim3(nwork), dim3(kTjdsBlock), 0, stream, start_pos,
                           row_ind, val, x_perm, y, work, cols);
    return hipGetLastError();
}

hipError_t launch_tjds_permute(const int *perm, const double *x, double *x_perm, int cols, hipStream_t stream)
{
    if (cols <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(tjds_permute_operand, dim3((cols + 255) / 256), dim3(256), 0, stream, perm, x, x_perm, cols);
    return hipGetLastError();
}

hipError_t launch_find_out_of_range(const int *a, long long n, int limit, int *bad, hipStream_t stream)
{
    if (n <= 0)
        return hipSuccess;
    const long long want = (n + 255) / 256;
    hipLaunchKernelGGL(find_out_of_range, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, stream, a, n,
                       limit, bad);
    return hipGetLastError();
}

// v <- v / max|v| (left alone when the maximum is 0); scratch = one unsigned long long of device memory
hipError_t launch_normalize_max(double *v, long long n, unsigned long long *scratch, hipStream_t stream)
{
    if (n <= 0)
        return hipSuccess;
    hipError_t e = hipMemsetAsync(scratch, 0, sizeof(unsigned long long), stream);
    if (e != hipSuccess)
        return e;
    const long long want = (n + 255) / 256;
    hipLaunchKernelGGL(vector_absmax, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), 0, stream, v, n, scratch);
    hipLaunchKernelGGL(vector_divide, dim3((unsigned)want), dim3(256), 0, stream, v, n, scratch);
    return hipGetLastError();
}

hipError_t launch_fill(double *p, double v, long long n, hipStream_t stream)
{
    if (n <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(fill_value, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, v, n);
    return hipGetLastError();
}

// How scattered are the gathers of a CSR matrix?  Sample s of `samples` looks at kSpreadSpan consecutive entries --
// what one XCD's turn of 64 tiles of the tile kernel gathers -- and counts the distinct 128-byte lines of x they touch,
// by linear counting: every line sets one hashed bit of a 512 Kbit LDS map; the host turns the number of set bits into
// the estimate (engine: csr_gather_spread).  A count near the number of entries means that nearly every gather pulls
// its own line through the L2: the matrix is one for the column sweep.
__global__ __launch_bounds__(1024) void csr_line_spread(const int *__restrict__ col_ind, long long nnz, int samples,
                                                        int *__restrict__ set_bits)
{
    constexpr int WORDS = 16 * 1024;  // 512 Kbit
    __shared__ unsigned map[WORDS];
    __shared__ int total;
    for (int i = threadIdx.x; i < WORDS; i += 1024)
        map[i] = 0u;
    if (threadIdx.x == 0)
        total = 0;
    __syncthreads();
    const long long first = samples > 1 ? (nnz - kSpreadSpan) / (samples - 1) * blockIdx.x : 0;
    for (int i = threadIdx.x; i < kSpreadSpan; i += 1024) {
        const long long j = first + i;
        if (j < nnz) {
            const unsigned line = (unsigned)col_ind[j] >> 4;
            const unsigned h = (line * 2654435761u) >> (32 - 19);
            atomicOr(&map[h >> 5], 1u << (h & 31));
        }
    }
    __syncthreads();
    int n = 0;
    for (int i = threadIdx.x; i < WORDS; i += 1024)
        n += __popc(map[i]);
    atomicAdd(&total, n);
    __syncthreads();
    if (threadIdx.x == 0)
        set_bits[blockIdx.x] = total;
}

hipError_t launch_csr_line_spread(const int *col_ind, long long nnz, int samples, int *set_bits, hipStream_t stream)
{
    if (samples <= 0 || nnz < kSpreadSpan)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(csr_line_spread, dim3(samples), dim3(1024), 0, stream, col_ind, nnz, samples, set_bits);
    return hipGetLastError();
}

}  // namespace smvp
