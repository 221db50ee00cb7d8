// smvp_colsweep.hip -- K4, the column sweep: csr_colsweep, sweep_combine and their launchers.  Compiled with the max-ILP
// scheduling strategy (the Makefile's ILPFLAGS; config 4's structure 1.767 -> 1.60 ms).
#include "smvp_kernels.h"

// ---------------------------------------------------------------------------
// K4: CSR, column-swept row strips -- for matrices whose columns scatter over an operand far larger than L2
// (BASELINE config 4: 32 uniform columns per row over an 80 MB x).  The tile kernels (K2, K2') then run at the chip's
// L2-miss gather rate (about 54 G gathers/s, 8.4 % of HBM peak on config 4) whatever they do, because every gather
// fetches its own line from the Infinity Cache.  Here the entries are kept a second time (the plan; row_ptr /
// col_ind / val stay as they are), ordered by (row strip, column) with a 16-bit word per entry: the row's number inside
// the strip and the entry's turn (below).  One WAVEFRONT owns a strip of up to 2048 rows: it keeps the strip's sums in
// its own quarter of the workgroup's LDS and streams the strip's entries in ascending column order, 256 at a time, so
// all the wavefronts that run together gather from one window of x that slides over the operand once per product and
// fits the XCD's 4 MB L2 (measured 135 G gathers/s on config 4: 2.4 ms against 5.98).  The launches are cut into
// generations of workgroups that are resident together and start together (per_launch), which is what keeps their
// windows aligned; a strip's sums are complete when its wavefront ends.
//
// Every row is summed in ascending column order -- the order of the serial loop, main-cli.c:410-416 -- so the result
// is bit-identical to it and the same from run to run.  (Round 2 added the products with LDS atomics in arrival order.)
// A strip belongs to one wavefront, whose LDS instructions execute in program order, so only entries of one row that
// meet in the same chunk of 256 need ordering: the plan gives each entry its turn, the number of earlier entries of
// its row in its chunk, entries of equal turn never share a row, and the wavefront adds turn 0 (nearly everything),
// then turn 1, ...  Turns from kSweepTurnCap on (a dense row in a narrow band of columns: not what this kernel is for,
// but it must stay right) are added one lane at a time in stream order.  No atomics, no barriers.
// ---------------------------------------------------------------------------
namespace smvp {

// One iteration of a wavefront takes G chunks of its strip (G * 256 entries, G * 4 per lane): all their gathers are in
// flight together, the plan words of the next iteration are requested before the sums are touched, and the chunks are
// then added one after the other (a chunk's turns are counted inside the chunk, so this keeps every row in order).
template <int G>
__global__ __launch_bounds__(kSweepBlock) void csr_colsweep(
    const long long *__restrict__ strip_ptr, const int *__restrict__ e_col, const double *__restrict__ e_val,
    const unsigned short *__restrict__ e_row, const double *__restrict__ x, double *__restrict__ y, int rows, int strip_rows,
    int nstrips, int wg_first, int parts, double *__restrict__ ypart, long long ypart_stride)
{
    constexpr int U = kSweepUnroll, E = G * U;
    constexpr long long STEP = (long long)G * kSweepChunk;
    extern __shared__ double sums_all[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    // `strip` numbers the STREAMS: strip * 1 (parts == 1: a stream is a strip's) or real strip * parts + column part
    int strip = (wg_first + (int)blockIdx.x) * kSweepWaves + wave;
    bool live = strip < nstrips * parts;
    long long part_rows0 = -1;  // parts == kSweepXcdParts: where this wavefront's partial sums go in ypart
    if (parts == kSweepXcdParts) {
        // XCD-private column parts: workgroup b of a launch runs on XCD b % 8 and takes column part b % 8 of the four strips of row
        // group b / 8 -- every XCD gathers from its own eighth of x only; the wavefronts keep whole strips, the eight partial sums
        // of a row meet in ypart and are added part by part by sweep_combine (reproducible, not the serial loop's bits)
        const int b = wg_first + (int)blockIdx.x, part = b % kSweepXcdParts, real = (b / kSweepXcdParts) * kSweepWaves + wave;
        live = real < nstrips;
        strip = real * kSweepXcdParts + part;
        part_rows0 = (long long)part * ypart_stride + (long long)real * strip_rows;
        if (!live)
            return;
    }
    if (!live && parts == 1)
        return;  // (no barrier in the one-part form)
    // volatile: every access is issued where it stands -- another lane's earlier store must be seen; the LDS address
    // space is spelled out so that these stay ds_read / ds_write
    typedef __attribute__((address_space(3))) volatile double lds_double;
    lds_double *sums = (lds_double *)sums_all + (size_t)wave * strip_rows;
    const long long a = live ? strip_ptr[strip] : 0, z = live ? strip_ptr[strip + 1] : 0;

    // entry e of an iteration starting at `base`: stream position base + e * 64 + lane; w = row | turn << kSweepRowBits,
    // -1 where the stream has ended
    auto fetch = [&](long long base, int (&c)[E], double (&v)[E], int (&w)[E]) {
        if (base + STEP <= z) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const long long j = base + e * 64 + lane;
                c[e] = __builtin_nontemporal_load(e_col + j);
                v[e] = __builtin_nontemporal_load(e_val + j);
                w[e] = __builtin_nontemporal_load(e_row + j);
            }
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const long long j = base + e * 64 + lane;
                const bool in = j < z;
                c[e] = in ? e_col[j] : 0;
                v[e] = in ? e_val[j] : 0.0;
                w[e] = in ? (int)e_row[j] : -1;
            }
        }
    };
    int c[E], w[E];
    double v[E];
    if (a < z)
        fetch(a, c, v, w);
    for (int i = lane; i < strip_rows; i += 64)
        sums[i] = 0.0;
    for (long long base = a; base < z; base += STEP) {
        double p[E];
#pragma unroll
        for (int e = 0; e < E; ++e)
            p[e] = x[c[e]];
        int cn[E], wn[E];
        double vn[E];
        if (base + STEP < z)
            fetch(base + STEP, cn, vn, wn);
#pragma unroll
        for (int e = 0; e < E; ++e)
            p[e] = v[e] * p[e];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            int row[U], turn[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                row[u] = w[g * U + u] < 0 ? 0 : w[g * U + u] & ((1 << kSweepRowBits) - 1);
                turn[u] = w[g * U + u] >> kSweepRowBits;  // -1 stays -1: no entry
            }
            for (int k = 0;; ++k) {
                double cur[U];
                bool later = false;
#pragma unroll
                for (int u = 0; u < U; ++u)
                    cur[u] = sums[row[u]];  // every lane reads (row 0 where it has no entry): four reads in flight, no branches
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (turn[u] == k)
                        sums[row[u]] = cur[u] + p[g * U + u];
                    later = later || (turn[u] > k && turn[u] < kSweepTurnCap);
                }
                if (!__any(later))
                    break;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                unsigned long long m = __ballot(turn[u] == kSweepTurnCap);
                while (m) {  // lane by lane, i.e. in stream order
                    const int l = __ffsll((long long)m) - 1;
                    if (lane == l)
                        sums[row[u]] = sums[row[u]] + p[g * U + u];
                    m &= m - 1;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            c[e] = cn[e];
            v[e] = vn[e];
            w[e] = wn[e];
        }
    }
    if (parts == kSweepXcdParts) {
        const long long r0 = part_rows0 - (part_rows0 / ypart_stride) * ypart_stride;  // the strip's first row
        for (int i = lane; i < strip_rows && r0 + i < rows; i += 64)
            ypart[part_rows0 + i] = sums[i];  // (read again by sweep_combine: through the caches)
        return;
    }
    if (parts == 1) {
        const long long r0 = (long long)strip * strip_rows;
        for (int i = lane; i < strip_rows && r0 + i < rows; i += 64)
            __builtin_nontemporal_store(sums[i], &y[r0 + i]);
        return;
    }
    // Column parts: the wavefronts w * parts ... w * parts + parts - 1 of this workgroup hold the partial sums of ONE strip over
    // their parts of the columns (each summed in ascending column order); a row's sum is its partial sums added in the
    // order of the parts -- ascending columns still, but associated part by part: reproducible from run to run, within the
    // rounding bound, NOT the serial loop's bits.
    __syncthreads();
    const int strips_here = kSweepWaves / parts;
    lds_double *all = (lds_double *)sums_all;
    for (int s = 0; s < strips_here; ++s) {
        const long long r0 = ((long long)(wg_first + (int)blockIdx.x) * strips_here + s) * strip_rows;
        for (int i = (int)threadIdx.x; i < strip_rows && r0 + i < rows; i += kSweepBlock) {
            double acc = all[(size_t)(s * parts) * strip_rows + i];
            for (int q = 1; q < parts; ++q)
                acc += all[(size_t)(s * parts + q) * strip_rows + i];
            __builtin_nontemporal_store(acc, &y[r0 + i]);
        }
    }
}

// XCD-private column parts: y[r] = the eight partial sums of row r, added in the order of the parts
__global__ __launch_bounds__(256) void sweep_combine(const double *__restrict__ ypart, long long stride, double *__restrict__ y, int rows)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows)
        return;
    double acc = ypart[r];
#pragma unroll
    for (int q = 1; q < kSweepXcdParts; ++q)
        acc += ypart[(long long)q * stride + r];
    __builtin_nontemporal_store(acc, &y[r]);
}

// Chunks in flight per wavefront.  A launch generation is one workgroup per CU (four wavefronts): with tall strips two chunks
// in flight make up for the missing wavefronts, with short ones they only make the window race (the strips' streams are
// short).  Measured (MI355X, config 4's columns; ms for G = 1 / 2; profiles/r05_colsweep_heights.txt): strips of 2048 rows
// 2.55 / 2.25 (10 M rows), 0.497 / 0.444 (1.25 M rows); 1221 rows 0.315 / 0.287 (1.25 M), 0.632 / 0.575 (2.5 M); 814 rows
// 0.648 / 0.636; 611 rows 0.328 / 0.373; 512 rows 0.413 / 0.468; 407 rows 0.348 / 0.459 -- two from about 800 rows on.
// `asked` = 1 | 2 | 4 overrides (SMVP_CSR_SWEEP_PARAM's third field: experiments); 0 = the rule.  Asked once per plan build
// (the engine keeps the answer in the handle), never on a launch path.
int sweep_chunks_in_flight(int strip_rows, int asked)
{
    return asked == 1 || asked == 2 || asked == 4 ? asked : (strip_rows >= 768 ? 2 : 1);
}

// Strips taller than 2048 rows need more dynamic LDS (up to the CU's 160 KB) than a kernel gets unasked: asked for here, for every
// form of the kernel, on the CURRENT device -- once per plan build (the engine), never on a launch path; always the same
// maximum, so that plans of different heights on one device cannot take it from one another.
constexpr size_t kSweepMaxLds = 160u * 1024;
hipError_t prepare_csr_colsweep()
{
    for (const void *f : {(const void *)csr_colsweep<1>, (const void *)csr_colsweep<2>, (const void *)csr_colsweep<4>}) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSweepMaxLds);
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

hipError_t launch_csr_colsweep(const long long *strip_ptr, const int *e_col, const double *e_val, const unsigned short *e_row,
                               const double *x, double *y, int rows, int strip_rows, int parts, int per_launch, int g, double *ypart,
                               hipStream_t stream)
{
    if (rows <= 0)
        return hipSuccess;
    const bool xcd = parts == kSweepXcdParts;
    if ((parts != 1 && parts != 2 && parts != 4 && !xcd) || (xcd && (!ypart || (per_launch > 0 && per_launch % kSweepXcdParts != 0))))
        return hipErrorInvalidValue;
    const int nstrips = (rows + strip_rows - 1) / strip_rows;
    const int nwg = xcd ? (nstrips + kSweepWaves - 1) / kSweepWaves * kSweepXcdParts
                        : (int)(((long long)nstrips * parts + kSweepWaves - 1) / kSweepWaves);
    const long long ypart_stride = rows;
    const size_t lds = sizeof(double) * (size_t)strip_rows * kSweepWaves;
    if (per_launch <= 0)
        per_launch = nwg;
    if (lds > kSweepMaxLds)
        return hipErrorInvalidValue;  // (strips of more than 5120 rows; up to there prepare_csr_colsweep has asked for the LDS)
    for (int first = 0; first < nwg; first += per_launch) {
        const unsigned grid = (unsigned)(nwg - first < per_launch ? nwg - first : per_launch);
#define SMVP_SWEEP(GG)                                                                                                   \
    hipLaunchKernelGGL(csr_colsweep<GG>, dim3(grid), dim3(kSweepBlock), lds, stream, strip_ptr, e_col, e_val, e_row, x, y, \
                       rows, strip_rows, nstrips, first, parts, ypart, ypart_stride)
        if (g == 4)
            SMVP_SWEEP(4);
        else if (g == 2)
            SMVP_SWEEP(2);
        else
            SMVP_SWEEP(1);
#undef SMVP_SWEEP
    }
    if (xcd)
        hipLaunchKernelGGL(sweep_combine, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, ypart, ypart_stride, y, rows);
    return hipGetLastError();
}

}  // namespace smvp
