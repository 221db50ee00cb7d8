// smvp_reorder.hip -- K23, device side: the multicolour ordering of a square plain-CSR handle (smvp_csr_color), classes to a
// permutation (smvp_perm_from_classes), B = P A P^T as a handle of its own (smvp_csr_create_permuted) and out[p] = in[index[p]]
// (smvp_vector_gather).  The definition of the colouring is in smvp_reorder_host.cpp, which restates it on one core.
//
//   color_round<T>   one round of the colouring: a group of T lanes per vertex that has no colour yet.  The group walks the vertex's
//                    row (and the row of the second handle) in strides of T; for every neighbour of larger key it reads the
//                    neighbour's colour.  One still without a colour leaves the vertex for the next LAUNCH -- no lane ever waits
//                    on a value another workgroup writes.  Otherwise the lanes mark the colours of the window [w, w + 64) in a
//                    64-bit mask, the group ORs the masks, and the first clear bit is the colour; a full window is followed by a
//                    further walk with w += 64.  A colour is written once and only ever read as -1 or as its final value (relaxed
//                    atomic accesses at agent scope), so the colours do not depend on timing; only the number of rounds does.
//   the others       one thread per element or entry.
#include "smvp_engine.h"
#include "smvp_prim.h"

#include <cmath>
#include <cstring>

namespace smvp {

namespace {

constexpr int kColorBlock = 256;       // threads of a workgroup of color_round
constexpr int kColorMaxBlocks = 2048;  // workgroups of a round at the most (plan option color_max_blocks): 8 per compute unit
constexpr int kColorChunk = 4;         // as kTrsvChunk in K15's rule for the lanes of a row

__device__ inline int color_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void color_store(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <int T>
__device__ inline unsigned long long group_or(unsigned long long m)
{
#pragma unroll
    for (int off = T / 2; off > 0; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)m, off, T), hi = __shfl_xor((unsigned)(m >> 32), off, T);
        m |= (unsigned long long)hi << 32 | lo;
    }
    return m;
}

// the colours in [w, w + 64) that the neighbours of larger key in row v of one pattern hold, as a mask; *waits is set where one
// of them has no colour yet (first window only: later windows are walked after all of them had one)
template <int T>
__device__ inline unsigned long long color_walk(const int *__restrict__ row_ptr, const int *__restrict__ col_ind, const int *color, int v,
                                                unsigned kv, unsigned seed, int lane, int w, bool *waits)
{
    unsigned long long mask = 0;
    const int z = row_ptr[v + 1];
    for (int p = row_ptr[v] + lane; p < z; p += T) {
        const int u = col_ind[p];
        if (u == v || mix32((unsigned)u ^ seed) < kv)
            continue;
        const int c = color_load(color + u);
        if (c < 0)
            *waits = true;
        else if (c >= w && c - w < 64)
            mask |= 1ull << (c - w);
    }
    return mask;
}

// One round.  Every workgroup makes the same number of trips, and inside a trip the lanes of a group go the same way: the group's
// shuffles always find all T lanes.  *coloured grows by the vertices this launch gave a colour.
template <int T>
__global__ __launch_bounds__(kColorBlock) void color_round(const int *__restrict__ row_ptr, const int *__restrict__ col_ind,
                                                           const int *__restrict__ t_row_ptr, const int *__restrict__ t_col_ind, int *color,
                                                           int n, unsigned seed, int *coloured)
{
    constexpr int kGroups = kColorBlock / T;
    const int lane = threadIdx.x & (T - 1), group = threadIdx.x / T;
    int done = 0;
    for (long long first = (long long)blockIdx.x * kGroups; first < n; first += (long long)gridDim.x * kGroups) {
        const long long vl = first + group;
        const int v = (int)vl;
        bool open = vl < n;
        if (open)
            open = color_load(color + v) < 0;  // (T lanes read one word)
        bool waits = false;
        unsigned long long mask = 0;
        const unsigned kv = mix32((unsigned)v ^ seed);
        if (open) {
            mask = color_walk<T>(row_ptr, col_ind, color, v, kv, seed, lane, 0, &waits);
            if (t_row_ptr)
                mask |= color_walk<T>(t_row_ptr, t_col_ind, color, v, kv, seed, lane, 0, &waits);
        }
        mask = group_or<T>(mask);
        waits = group_or<T>(waits ? 1ull : 0ull) != 0;
        if (!open || waits)
            continue;
        int w = 0;
        while (mask == ~0ull) {  // (uniform inside the group)
            w += 64;
            bool none = false;
            mask = color_walk<T>(row_ptr, col_ind, color, v, kv, seed, lane, w, &none);
            if (t_row_ptr)
                mask |= color_walk<T>(t_row_ptr, t_col_ind, color, v, kv, seed, lane, w, &none);
            mask = group_or<T>(mask);
        }
        if (lane == 0) {
            color_store(color + v, w + __ffsll((long long)~mask) - 1);
            ++done;
        }
    }
    // one integer add per wavefront (every lane is here: the trips are uniform)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        done += __shfl_xor(done, off, 64);
    if ((threadIdx.x & 63) == 0 && done > 0)
        atomicAdd(coloured, done);
}

int pow2_lanes(double mean)
{
    int p = 2;
    while (p < 64 && p < mean)
        p <<= 1;
    return p;
}

hipError_t launch_color_round(int T, int blocks, const CsrView &m, const CsrView *t, int *color, unsigned seed, int *coloured, hipStream_t st)
{
    const int *trp = t ? t->d_row_ptr : nullptr, *tci = t ? t->d_col_ind : nullptr;
#define SMVP_COLOR_ROUND(L)                                                                                                       \
    case L:                                                                                                                       \
        hipLaunchKernelGGL(color_round<L>, dim3((unsigned)blocks), dim3(kColorBlock), 0, st, m.d_row_ptr, m.d_col_ind, trp, tci, color, \
                           m.rows, seed, coloured);                                                                               \
        break;
    switch (T) {
        SMVP_COLOR_ROUND(2)
        SMVP_COLOR_ROUND(4)
        SMVP_COLOR_ROUND(8)
        SMVP_COLOR_ROUND(16)
        SMVP_COLOR_ROUND(32)
    default:
        hipLaunchKernelGGL(color_round<64>, dim3((unsigned)blocks), dim3(kColorBlock), 0, st, m.d_row_ptr, m.d_col_ind, trp, tci, color, m.rows,
                           seed, coloured);
    }
#undef SMVP_COLOR_ROUND
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- permutations and vectors
__global__ __launch_bounds__(256) void fill_iota(int *a, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n)
        a[i] = i;
}

// inv[a[i]] = i
__global__ __launch_bounds__(256) void invert_permutation(const int *__restrict__ a, int *__restrict__ inv, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n)
        inv[a[i]] = i;
}

// counts[1 + class] += 1: integer adds, one right answer
__global__ __launch_bounds__(256) void count_classes(const int *__restrict__ cls, int n, int *counts)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n)
        atomicAdd(counts + 1 + cls[i], 1);
}

// inv[a[i]] = i for the elements of a inside [0, n) only; inv was preset to -1 (where two elements name one place, either stays)
__global__ __launch_bounds__(256) void scatter_in_range(const int *__restrict__ a, int *inv, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const int t = a[i];
        if (t >= 0 && t < n)
            inv[t] = i;
    }
}

// a is a permutation of 0 .. n-1 exactly when a[inv[p]] == p for every p: *bad = 1 + the first place (largest seen) that nothing names
__global__ __launch_bounds__(256) void check_inverse(const int *__restrict__ a, const int *__restrict__ inv, int n, int *bad)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < n) {
        const int i = inv[p];
        if (i < 0 || i >= n || a[i] != p)
            atomicMax(bad, p < 2147483646 ? p + 1 : 2147483647);
    }
}

// entry j of A as the entry of P A P^T: {new_of_old[row that holds j], new_of_old[col_ind[j]], val[j]}, in storage order (the row
// by bisection of row_ptr, as csr_swapped_coo finds it).  new_of_old was checked to be a permutation, col_ind by the handle.
__global__ __launch_bounds__(256) void csr_permuted_coo(const int *__restrict__ row_ptr, const int *__restrict__ col_ind,
                                                        const double *__restrict__ val, const int *__restrict__ new_of_old, int rows,
                                                        long long nnz, smvp_coo_t *__restrict__ coo)
{
    const long long stride = (long long)gridDim.x * 256;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < nnz; j += stride) {
        int lo = 0, hi = rows;  // row_ptr[lo] <= j < row_ptr[hi]
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (row_ptr[mid] <= j)
                lo = mid;
            else
                hi = mid;
        }
        smvp_coo_t e;
        e.row = new_of_old[lo];
        e.col = new_of_old[col_ind[j]];
        e.val = val[j];
        coo[j] = e;
    }
}

// out[p] = in[index[p]] as 64-bit words (every bit of a NaN travels); an index outside [0, n) is not followed: a quiet NaN
__global__ __launch_bounds__(256) void gather_words(const int *__restrict__ index, const unsigned long long *__restrict__ in,
                                                    unsigned long long *__restrict__ out, int n)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < n) {
        const int i = index[p];
        out[p] = i >= 0 && i < n ? in[i] : 0x7ff8000000000000ull;
    }
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

}  // namespace smvp

using smvp::CsrView;
using smvp::DeviceScope;
using smvp::fail;

extern "C" int smvp_csr_color(const smvp_csr_t *h, const smvp_csr_t *ht, const smvp_color_opts_t *opts, int *d_color, smvp_color_info_t *info,
                              void *stream)
{
    const char *fn = "smvp_csr_color";
    if (!h)
        return fail(SMVP_ERR_INVALID, "%s: null handle", fn);
    if (int rc = smvp::color_check_opts(fn, opts, info))
        return rc;
    const CsrView m = smvp::csr_view(h);
    CsrView t{};
    if (ht)
        t = smvp::csr_view(ht);
    for (const CsrView *a : {&m, (const CsrView *)&t}) {
        if (a == &t && !ht)
            continue;
        const char *name = a == &m ? "h" : "ht";
        if (a->flavor != smvp::kFlavorCsr)
            return fail(SMVP_ERR_UNSUPPORTED, "%s: plain CSR handles only (%s belongs to a TJDS matrix)", fn, name);
        if (a->first_row != 0)
            return fail(SMVP_ERR_UNSUPPORTED, "%s: %s is a row block (first_row = %lld): whole matrices only", fn, name, a->first_row);
    }
    if (m.rows != m.cols)
        return fail(SMVP_ERR_INVALID, "%s: the handle's matrix is %d x %d, not square", fn, m.rows, m.cols);
    if (ht && (t.rows != m.rows || t.cols != m.cols))
        return fail(SMVP_ERR_INVALID, "%s: ht is %d x %d, h is %d x %d", fn, t.rows, t.cols, m.rows, m.cols);
    if (ht && t.device != m.device)
        return fail(SMVP_ERR_INVALID, "%s: ht lives on device %d, h on device %d", fn, t.device, m.device);
    const int n = m.rows;
    if (n > 0 && !d_color)
        return fail(SMVP_ERR_INVALID, "%s: null d_color", fn);
    DeviceScope on(m.device);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = smvp::refuse_capture(st, "smvp_csr_color: the stream is capturing (the call allocates and reads a counter back after every round)"))
        return rc;
    smvp_color_opts_t o;
    smvp_color_opts_default(&o);
    if (opts)
        o = *opts;
    const double t0 = smvp::wall_ms();
    smvp_color_info_t out{};
    out.struct_size = sizeof out;
    out.entries = (long long)m.nnz + (ht ? t.nnz : 0);
    // lanes per vertex by K15's rule: from the geometric mean of the mean and the longest row (both patterns' rows together)
    int longest = 0;
    for (int r = 0; r < n; ++r)
        longest = std::max(longest, m.h_row_ptr[r + 1] - m.h_row_ptr[r] + (ht ? t.h_row_ptr[r + 1] - t.h_row_ptr[r] : 0));
    const double mean = n > 0 ? (double)out.entries / n : 0.0;
    const int T = smvp::pow2_lanes(std::sqrt(mean * longest) / smvp::kColorChunk);
    out.lanes_per_row = T;
    int total = 0;
    if (n > 0) {
        int *d_count = nullptr;
        if (hipMalloc((void **)&d_count, 4 * sizeof(int)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(SMVP_ERR_ALLOC, "%s: cannot allocate the counter", fn);
        }
        const long long want = ((long long)n * T + smvp::kColorBlock - 1) / smvp::kColorBlock;
        const int blocks = (int)std::min<long long>(want, std::max(1, smvp::option("color_max_blocks", smvp::kColorMaxBlocks)));
        hipError_t e = hipMemsetAsync(d_count, 0, 4 * sizeof(int), st);
        if (e == hipSuccess)
            e = hipMemsetAsync(d_color, 0xff, sizeof(int) * (size_t)n, st);  // -1 everywhere
        while (e == hipSuccess && total < n && out.rounds < o.max_rounds) {
            e = smvp::launch_color_round(T, blocks, m, ht ? &t : nullptr, d_color, o.seed, d_count, st);
            if (e == hipSuccess)
                e = hipMemcpyAsync(&total, d_count, sizeof(int), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess)
                e = hipStreamSynchronize(st);
            ++out.rounds;
        }
        if (e != hipSuccess)
            (void)hipStreamSynchronize(st);
        (void)hipFree(d_count);
        if (e != hipSuccess)
            return fail(SMVP_ERR_HIP, "%s: round %d failed: %s", fn, out.rounds, hipGetErrorString(e));
        if (total < n)
            return fail(SMVP_ERR_UNSUPPORTED, "%s: %d of %d vertices have a colour after max_rounds = %d launches", fn, total, n, o.max_rounds);
    }
    out.build_ms = smvp::wall_ms() - t0;
    if (info) {
        // the classes' sizes: the colours once on the host (nothing further is allocated on the device)
        std::vector<int> col((size_t)n), size;
        if (n > 0)
            HIP_TRY(hipMemcpy(col.data(), d_color, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
        for (int c : col) {
            if (c < 0 || c > n)
                return fail(SMVP_ERR_HIP, "%s: a colour of %d among %d vertices", fn, c, n);
            if ((size_t)c >= size.size())
                size.resize((size_t)c + 1, 0);
            ++size[(size_t)c];
        }
        out.colors = (int)size.size();
        out.largest_class = size.empty() ? 0 : *std::max_element(size.begin(), size.end());
        out.smallest_class = size.empty() ? 0 : *std::min_element(size.begin(), size.end());
        *info = out;
    }
    return SMVP_OK;
}

extern "C" int smvp_perm_from_classes(int device, int n, int classes, const int *d_class, int *d_old_of_new, int *d_new_of_old, int *class_ptr,
                                      void *stream)
{
    const char *fn = "smvp_perm_from_classes";
    if (n < 0 || classes < 0)
        return fail(SMVP_ERR_INVALID, "%s: %s < 0", fn, n < 0 ? "n" : "classes");
    if (n > 0 && (!d_class || !d_old_of_new || !d_new_of_old))
        return fail(SMVP_ERR_INVALID, "%s: null %s", fn, !d_class ? "d_class" : !d_old_of_new ? "d_old_of_new" : "d_new_of_old");
    if (n > 0 && classes == 0)
        return fail(SMVP_ERR_INVALID, "%s: d_class[0] lies outside [0, 0): %d elements and no class", fn, n);
    if (int rc = smvp::usable_device(device))
        return rc;
    DeviceScope on(device);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = smvp::refuse_capture(st, "smvp_perm_from_classes: the stream is capturing (the call allocates and waits)"))
        return rc;
    if (n == 0) {
        for (int c = 0; class_ptr && c <= classes; ++c)
            class_ptr[c] = 0;
        return SMVP_OK;
    }
    unsigned bits = 0;
    while (bits < 32 && ((unsigned long long)classes - 1) >> bits)
        ++bits;
    // one workspace: the flag of the check, 0 .. n-1, the sorted classes, the classes' counts, the scan's and the sort's storage
    size_t scan_bytes = 0, sort_bytes = 0;
    (void)smvp::prim::exclusive_scan(nullptr, scan_bytes, nullptr, nullptr, 0, (size_t)classes + 1, st);
    (void)smvp::prim::radix_sort_pairs<unsigned, int>(nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, (size_t)n, 0, bits, st);
    using smvp::prim::align_up;
    const size_t off_iota = 256, off_keys = off_iota + align_up(sizeof(int) * (size_t)n), off_counts = off_keys + align_up(sizeof(int) * (size_t)n),
                 off_scan = off_counts + align_up(sizeof(int) * ((size_t)classes + 1)), off_sort = off_scan + align_up(scan_bytes),
                 bytes = off_sort + align_up(sort_bytes);
    char *ws = nullptr;
    if (hipMalloc((void **)&ws, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(SMVP_ERR_ALLOC, "%s: cannot allocate %zu bytes of workspace (%d elements, %d classes)", fn, bytes, n, classes);
    }
    int *d_bad = (int *)ws, *d_iota = (int *)(ws + off_iota), *d_counts = (int *)(ws + off_counts);
    unsigned *d_keys = (unsigned *)(ws + off_keys);
    int bad = 0, rc = SMVP_OK;
    auto hip = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && rc == SMVP_OK)
            rc = fail(SMVP_ERR_HIP, "%s: %s failed: %s", fn, what, hipGetErrorString(e));
        return rc == SMVP_OK;
    };
    // the check first: nothing below indexes with a class before it has passed
    if (hip(hipMemsetAsync(d_bad, 0, sizeof(int), st), "hipMemsetAsync") &&
        hip(smvp::launch_find_out_of_range(d_class, n, classes, d_bad, st), "the range check") &&
        hip(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st), "hipMemcpyAsync") && hip(hipStreamSynchronize(st), "hipStreamSynchronize") &&
        bad)
        rc = fail(SMVP_ERR_INVALID, "%s: d_class[%d] lies outside [0, %d)", fn, bad - 1, classes);
    std::vector<int> ptr((size_t)classes + 1, 0);
    if (rc == SMVP_OK) {
        hipLaunchKernelGGL(smvp::fill_iota, dim3(smvp::blocks_of(n)), dim3(256), 0, st, d_iota, n);
        hip(hipGetLastError(), "fill_iota");
        size_t sb = sort_bytes;
        if (rc == SMVP_OK)
            hip(smvp::prim::radix_sort_pairs<unsigned, int>(ws + off_sort, sb, (const unsigned *)d_class, d_keys, d_iota, d_old_of_new, (size_t)n, 0,
                                                            bits, st),
                "the sort");
        if (rc == SMVP_OK) {
            hipLaunchKernelGGL(smvp::invert_permutation, dim3(smvp::blocks_of(n)), dim3(256), 0, st, d_old_of_new, d_new_of_old, n);
            hip(hipGetLastError(), "invert_permutation");
        }
        if (rc == SMVP_OK && class_ptr) {
            hip(hipMemsetAsync(d_counts, 0, sizeof(int) * ((size_t)classes + 1), st), "hipMemsetAsync");
            if (rc == SMVP_OK) {
                hipLaunchKernelGGL(smvp::count_classes, dim3(smvp::blocks_of(n)), dim3(256), 0, st, d_class, n, d_counts);
                hip(hipGetLastError(), "count_classes");
            }
            size_t cb = scan_bytes;
            // (counts[0] = 0 and counts[1 + c] = the size of class c: the inclusive sums are class_ptr)
            if (rc == SMVP_OK)
                hip(smvp::prim::inclusive_scan(ws + off_scan, cb, d_counts, d_counts, (size_t)classes + 1, st), "the scan");
            if (rc == SMVP_OK)
                hip(hipMemcpyAsync(ptr.data(), d_counts, sizeof(int) * ((size_t)classes + 1), hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
        }
        if (rc == SMVP_OK)
            hip(hipStreamSynchronize(st), "hipStreamSynchronize");
    }
    if (rc != SMVP_OK && rc != SMVP_ERR_INVALID)
        (void)hipStreamSynchronize(st);  // (nothing of this call may still use the workspace)
    (void)hipFree(ws);
    if (rc == SMVP_OK && class_ptr)
        memcpy(class_ptr, ptr.data(), sizeof(int) * ptr.size());
    return rc;
}

// B = P A P^T as a CSR handle of its own: smvp_csr_create_transposed's route with the entries mapped instead of swapped, after the
// permutation has been checked on the device
extern "C" int smvp_csr_create_permuted(smvp_csr_t **out, const smvp_csr_t *h, const int *d_new_of_old, void *stream)
{
    const char *fn = "smvp_csr_create_permuted";
    if (out)
        *out = nullptr;
    if (!out || !h)
        return fail(SMVP_ERR_INVALID, "%s: null %s", fn, out ? "handle" : "out");
    const CsrView m = smvp::csr_view(h);
    if (m.flavor != smvp::kFlavorCsr)
        return fail(SMVP_ERR_UNSUPPORTED, "%s: plain CSR handles only (this one belongs to a TJDS matrix)", fn);
    if (m.first_row != 0)
        return fail(SMVP_ERR_UNSUPPORTED, "%s: a row block (first_row = %lld) cannot be permuted on its own", fn, m.first_row);
    if (m.rows != m.cols)
        return fail(SMVP_ERR_INVALID, "%s: the handle's matrix is %d x %d, not square", fn, m.rows, m.cols);
    const int n = m.rows, nnz = m.nnz;
    if (n > 0 && !d_new_of_old)
        return fail(SMVP_ERR_INVALID, "%s: null d_new_of_old", fn);
    DeviceScope on(m.device);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = smvp::refuse_capture(st, "smvp_csr_create_permuted: allocates and synchronises, so it cannot be captured (the stream is capturing)"))
        return rc;
    // is d_new_of_old a permutation?  inv[new_of_old[i]] = i for the elements in range, then new_of_old[inv[p]] == p for every p
    if (n > 0) {
        int *inv = nullptr, bad = 0;  // n places and the flag behind them
        if (hipMalloc((void **)&inv, sizeof(int) * ((size_t)n + 4)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(SMVP_ERR_ALLOC, "%s: cannot allocate the check of the permutation (%d elements)", fn, n);
        }
        hipError_t e = hipMemsetAsync(inv, 0xff, sizeof(int) * (size_t)n, st);
        if (e == hipSuccess)
            e = hipMemsetAsync(inv + n, 0, sizeof(int), st);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(smvp::scatter_in_range, dim3(smvp::blocks_of(n)), dim3(256), 0, st, d_new_of_old, inv, n);
            hipLaunchKernelGGL(smvp::check_inverse, dim3(smvp::blocks_of(n)), dim3(256), 0, st, d_new_of_old, inv, n, inv + n);
            e = hipGetLastError();
        }
        if (e == hipSuccess)
            e = hipMemcpyAsync(&bad, inv + n, sizeof(int), hipMemcpyDeviceToHost, st);
        const hipError_t es = hipStreamSynchronize(st);
        (void)hipFree(inv);
        if (e != hipSuccess || es != hipSuccess)
            return fail(SMVP_ERR_HIP, "%s: the check of the permutation failed: %s", fn, hipGetErrorString(e != hipSuccess ? e : es));
        if (bad)
            return fail(SMVP_ERR_INVALID, "%s: d_new_of_old is no permutation of 0 .. %d: no element names place %d (an element is repeated or out of range)",
                        fn, n - 1, bad - 1);
    }
    int *b_row_ptr = nullptr, *b_col_ind = nullptr;
    double *b_val = nullptr;
    smvp_coo_t *coo = nullptr;
    auto release = [&]() {
        for (void *p : {(void *)b_row_ptr, (void *)b_col_ind, (void *)b_val, (void *)coo})
            if (p)
                (void)hipFree(p);
    };
    if (hipMalloc((void **)&b_row_ptr, sizeof(int) * ((size_t)n + 4)) != hipSuccess ||
        hipMalloc((void **)&b_col_ind, sizeof(int) * std::max<size_t>((size_t)nnz, 4)) != hipSuccess ||
        hipMalloc((void **)&b_val, sizeof(double) * std::max<size_t>((size_t)nnz, 4)) != hipSuccess ||
        hipMalloc((void **)&coo, sizeof(smvp_coo_t) * std::max<size_t>((size_t)nnz, 4)) != hipSuccess) {
        (void)hipGetLastError();
        release();
        return fail(SMVP_ERR_ALLOC, "%s: cannot allocate the permuted arrays and the entry list (%d entries)", fn, nnz);
    }
    int rc = SMVP_OK;
    if (nnz > 0 && n > 0) {
        const long long blocks = ((long long)nnz + 255) / 256;
        hipLaunchKernelGGL(smvp::csr_permuted_coo, dim3((unsigned)std::min<long long>(blocks, 1 << 20)), dim3(256), 0, st, m.d_row_ptr, m.d_col_ind,
                           m.d_val, d_new_of_old, n, (long long)nnz, coo);
        if (const hipError_t e = hipGetLastError(); e != hipSuccess)
            rc = fail(SMVP_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    }
    if (rc == SMVP_OK) {
        rc = smvp_csr_from_coo_device(coo, n, n, nnz, b_row_ptr, b_col_ind, b_val, stream);  // returns after the work on `stream`
        if (rc == SMVP_ERR_HIP && strstr(smvp_last_error(), "out of memory")) {
            (void)hipGetLastError();
            rc = fail(SMVP_ERR_ALLOC, "%s: cannot allocate the sort's buffers (%d entries)", fn, nnz);
        }
    }
    if (rc != SMVP_OK)
        (void)hipStreamSynchronize(st);  // (nothing of this call may still read the entry list)
    (void)hipFree(coo);
    coo = nullptr;
    smvp_csr_t *b = nullptr;
    if (rc == SMVP_OK) {
        rc = smvp::csr_create_owning(&b, m.device, n, n, nnz, b_row_ptr, b_col_ind, b_val);
        if (rc == SMVP_ERR_HIP && strstr(smvp_last_error(), "out of memory")) {
            (void)hipGetLastError();
            rc = fail(SMVP_ERR_ALLOC, "%s: cannot allocate the permuted handle's plan (%d entries)", fn, nnz);
        }
    }
    if (rc != SMVP_OK) {
        release();
        return rc;
    }
    *out = b;
    return SMVP_OK;
}

extern "C" int smvp_vector_gather(int device, int n, const int *d_index, const double *d_in, double *d_out, void *stream)
{
    const char *fn = "smvp_vector_gather";
    if (n < 0)
        return fail(SMVP_ERR_INVALID, "%s: n < 0", fn);
    if (n > 0 && (!d_index || !d_in || !d_out))
        return fail(SMVP_ERR_INVALID, "%s: null %s", fn, !d_index ? "d_index" : !d_in ? "d_in" : "d_out");
    if (smvp::operands_overlap(d_in, 1, n, d_out, 1, n, 1))
        return fail(SMVP_ERR_INVALID, "%s: the byte ranges of d_in and d_out overlap", fn);
    if (int rc = smvp::usable_device(device))
        return rc;
    if (n == 0)
        return SMVP_OK;
    DeviceScope on(device);
    hipLaunchKernelGGL(smvp::gather_words, dim3(smvp::blocks_of(n)), dim3(256), 0, (hipStream_t)stream, d_index, (const unsigned long long *)d_in,
                       (unsigned long long *)d_out, n);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess)
        return fail(SMVP_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return SMVP_OK;
}
