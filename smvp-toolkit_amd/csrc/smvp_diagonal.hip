// smvp_diagonal.hip -- K14: the diagonal of a handle's matrix (smvp_csr_diagonal, smvp_tjds_diagonal; new: the reference only ever
// multiplies).  Element i of the result starts at +0.0 and adds every stored entry (i, i) in ascending storage position, so an
// absent diagonal and a lone stored -0.0 both read +0.0 and repeated entries add up in the order they are stored.  No plan, no
// atomics, no LDS, no barriers: both kernels read the handle's own arrays, every element of the result is written by one lane of
// one launch, and the bits are the same on every run.
//
//   csr_diagonal_rows<T>   a group of T lanes per row (T from the mean row length, the rule of csr_vector_rows), so a row of
//                          hundreds of entries is never one lane's walk.  Columns of adopted arrays need not be sorted: the whole
//                          row is examined.  The lanes compare col_ind with the row's diagonal column -- first_row + row for a row
//                          block; a column beyond `cols` matches nothing -- and the group's first lane walks the set bits of the
//                          ballot in ascending order, reading val there and nowhere else: col_ind is streamed, val is touched at
//                          matches only.  A group takes kDiagRows rows, dealt so that each turn of a wavefront reads one contiguous
//                          run of col_ind, and issues the first trip of all of them before it looks at any: with one row per group
//                          a wavefront had a few hundred bytes in flight behind two dependent loads (config 4: 1.03 ms, now
//                          0.50).  Further trips of a long row follow, kDiagTrips in flight.  Declined, measured: issuing the
//                          value loads of all eight rows' first matches together (106 VGPRs for 80; memplus x944 0.90 ms for
//                          0.63, config 4 0.67 for 0.50; profiles/pcg_measured.txt).
//   tjds_diagonal_columns  the traversal of K8 (tjds_transposed_columns): lane k walks down permuted column k, one jagged diagonal
//                          per step, so a wavefront reads contiguous runs of row_ind; it compares with perm[k], reads val at a
//                          match and stores to d[perm[k]].  A lane k in [cols, rows) owns no column and writes d[k] = +0.0 (perm
//                          is a permutation of [0, cols): no element has two writers); a column whose number is no row's (cols >
//                          rows) stores nothing.
// 32-bit positions as in K8: start_pos[d] + k < nnz for an active lane; lanes are counted unsigned.
#include "smvp_common.h"
#include "smvp_kernels.h"

namespace smvp {

namespace {

constexpr int kDiagRows = 8;    // rows a group of lanes takes: their first trips' col_ind loads are in flight together
constexpr int kDiagTrips = 4;   // further trips of T entries of a long row whose loads a lane keeps in flight together
constexpr int kDiagTBatch = 8;  // jagged diagonals whose row_ind loads a lane keeps in flight together (K8's depth)

template <int T>
__global__ __launch_bounds__(kVectorBlock) void csr_diagonal_rows(const int *__restrict__ row_ptr, const int *__restrict__ col_ind,
                                                                   const double *__restrict__ val, double *__restrict__ d, int rows,
                                                                   int cols, long long first_row, int chunk0)
{
    constexpr int G = 64 / T;  // groups of a wavefront
    constexpr unsigned long long kGroup = T == 64 ? ~0ull : (1ull << T) - 1;
    const long long wave = ((long long)blockIdx.x * kVectorBlock + threadIdx.x) >> 6;
    const int lane = threadIdx.x & (T - 1);
    const int shift = threadIdx.x & 63 & ~(T - 1);  // where the group's lanes lie in the wavefront's ballot
    // turn i of the wavefront: its G groups take G consecutive rows, so the turn's loads are one contiguous run of col_ind
    const long long row0 = chunk0 + wave * (kDiagRows * G) + (shift / T);
    int a[kDiagRows], z[kDiagRows], c[kDiagRows];
#pragma unroll
    for (int i = 0; i < kDiagRows; ++i) {
        const long long row = row0 + i * G;
        a[i] = z[i] = 0;
        if (row < rows) {
            a[i] = row_ptr[row];
            z[i] = row_ptr[row + 1];
        }
    }
#pragma unroll
    for (int i = 0; i < kDiagRows; ++i)  // the first T entries of every row of the wavefront: kDiagRows loads in flight per lane
        c[i] = (long long)a[i] + lane < z[i] ? col_ind[(long long)a[i] + lane] : -1;
#pragma unroll
    for (int i = 0; i < kDiagRows; ++i) {
        const long long row = row0 + i * G, want = first_row + row;
        const int target = want < cols ? (int)want : -2;  // (no stored column is negative; -1 stands for "past the row's end")
        double acc = 0.0;
        unsigned long long m = (__ballot(c[i] == target) >> shift) & kGroup;
        if (lane == 0)
            for (; m; m &= m - 1)  // a match is rare: the set bits in ascending position, one value each
                acc = acc + val[(long long)a[i] + __builtin_ctzll(m)];
        for (long long base = (long long)a[i] + T; base < z[i]; base += kDiagTrips * T) {  // a row longer than the group is wide
            int e[kDiagTrips];
#pragma unroll
            for (int u = 0; u < kDiagTrips; ++u) {
                const long long j = base + u * T + lane;
                e[u] = j < z[i] ? col_ind[j] : -1;
            }
#pragma unroll
            for (int u = 0; u < kDiagTrips; ++u) {
                m = (__ballot(e[u] == target) >> shift) & kGroup;
                if (lane == 0)
                    for (; m; m &= m - 1)
                        acc = acc + val[base + u * T + __builtin_ctzll(m)];
            }
        }
        if (lane == 0 && row < rows)
            d[row] = acc;
    }
}

__global__ __launch_bounds__(kTjdsBlock) void tjds_diagonal_columns(const int *__restrict__ start_pos, const int *__restrict__ row_ind,
                                                                    const double *__restrict__ val, const int *__restrict__ perm,
                                                                    double *__restrict__ dg, unsigned rows, unsigned cols, int num_diag)
{
    const unsigned k = blockIdx.x * (unsigned)kTjdsBlock + threadIdx.x;
    // the wavefront's first column: the longest of its 64, so its length is the wave's trip count
    const unsigned k_wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(k & ~63u));
    const int c = k < cols ? perm[k] : -2;  // (no stored row is negative)
    double acc = 0.0;
    for (int d = 0; d < num_diag; d += kDiagTBatch) {
        int base[kDiagTBatch + 1];
#pragma unroll
        for (int i = 0; i <= kDiagTBatch; ++i)
            base[i] = start_pos[d + i < num_diag ? d + i : num_diag];  // (uniform index: scalar loads)
        if ((unsigned)(base[1] - base[0]) <= k_wave)
            break;  // no column of this wavefront reaches diagonal d, nor any later one
        int r[kDiagTBatch];
#pragma unroll
        for (int i = 0; i < kDiagTBatch; ++i)  // a lane whose column has ended compares with -1 (a diagonal past the last has width 0)
            r[i] = k < (unsigned)(base[i + 1] - base[i]) ? row_ind[base[i] + (int)k] : -1;
#pragma unroll
        for (int i = 0; i < kDiagTBatch; ++i)
            if (r[i] == c)
                acc = acc + val[base[i] + (int)k];  // in diagonal order: ascending TJDS position inside the column
    }
    if (k < cols) {
        if ((unsigned)c < rows)
            dg[c] = acc;
    } else if (k < rows)
        dg[k] = 0.0;  // a row beyond the last column: no column owns it
}

template <int T>
void launch_rows(const int *row_ptr, const int *col_ind, const double *val, double *d, int rows, int cols, long long first_row,
                 hipStream_t stream)
{
    const long long chunk = ((long long)1 << 31) / T;  // (a launch of fewer than 2^32 threads, a multiple of every wavefront's rows)
    constexpr long long kWaveRows = (long long)kDiagRows * (64 / T);
    for (long long row0 = 0; row0 < rows; row0 += chunk) {
        const long long n = rows - row0 < chunk ? rows - row0 : chunk;
        const long long waves = (n + kWaveRows - 1) / kWaveRows;
        const unsigned grid = (unsigned)((waves * 64 + kVectorBlock - 1) / kVectorBlock);
        hipLaunchKernelGGL(csr_diagonal_rows<T>, dim3(grid), dim3(kVectorBlock), 0, stream, row_ptr, col_ind, val, d, rows, cols,
                           first_row, (int)row0);
    }
}

}  // namespace

hipError_t launch_csr_diagonal(int lanes_per_row, const int *row_ptr, const int *col_ind, const double *val, double *d, int rows,
                               int cols, long long first_row, hipStream_t stream)
{
    if (rows <= 0)
        return hipSuccess;
    switch (lanes_per_row) {
    case 2: launch_rows<2>(row_ptr, col_ind, val, d, rows, cols, first_row, stream); break;
    case 4: launch_rows<4>(row_ptr, col_ind, val, d, rows, cols, first_row, stream); break;
    case 8: launch_rows<8>(row_ptr, col_ind, val, d, rows, cols, first_row, stream); break;
    case 16: launch_rows<16>(row_ptr, col_ind, val, d, rows, cols, first_row, stream); break;
    case 32: launch_rows<32>(row_ptr, col_ind, val, d, rows, cols, first_row, stream); break;
    case 64: launch_rows<64>(row_ptr, col_ind, val, d, rows, cols, first_row, stream); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_tjds_diagonal(const int *start_pos, const int *row_ind, const double *val, const int *perm, double *d, int rows,
                                int cols, int num_diag, hipStream_t stream)
{
    const int lanes = rows > cols ? rows : cols;
    if (rows <= 0)
        return hipSuccess;
    const unsigned grid = (unsigned)(((long long)lanes + kTjdsBlock - 1) / kTjdsBlock);
    hipLaunchKernelGGL(tjds_diagonal_columns, dim3(grid), dim3(kTjdsBlock), 0, stream, start_pos, row_ind, val, perm, d, (unsigned)rows,
                       (unsigned)cols, num_diag);
    return hipGetLastError();
}

}  // namespace smvp
