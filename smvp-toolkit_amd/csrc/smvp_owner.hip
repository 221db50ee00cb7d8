// smvp_owner.hip -- the owner (tile) kernel K2' (smvp_owner_kernel.h) under the compiler's default scheduling strategy: the plain
// launches of the TJDS flavours, the repeating form of every flavour that has one, the stamp reduction, and the launchers the
// engine calls.  The CSR flavours' plain launches are smvp_owner_csr.hip, which launch_csr_stream_owner hands them to.
#include "smvp_owner_kernel.h"

#include <cstdio>

namespace smvp {

// Not called.  It keeps the runtime header's __shfl_down in its general form in this unit.  Every shuffle here is 64 lanes wide
// (owner_body's giant-row sum, stamp_reduce), and where all callers of the header's function in a unit pass the same width the
// compiler specialises the function for it before it inlines it: the shuffle trees then come out as other instructions than in a
// unit that also shuffles inside sub-wavefronts (as these kernels' unit did while it also held csr_vector_rows), and the
// repeating forms get other registers -- the same sums, but memplus.mtx CSR -4.5 % and pwt.mtx TJDS +3.3 % per product of a
// repeating launch (profiles/kernel_units_split_measured.txt).  With one caller whose width is a variable, these kernels'
// instructions do not depend on which other kernels share their file.  A device function, not a kernel: no launch, no name.
__attribute__((used)) __device__ double shfl_any_width(double v, int width) { return __shfl_down(v, 1, width); }

// ---------------------------------------------------------------------------
// K2-repeat: `reps` products in ONE launch, each with a window of its own -- for the reference's own use case, -n 1000 on a
// matrix that lives in the caches (main-cli.c:402-420: the same product, the same x, n times).  A launch boundary costs such
// a product as much as the product (memplus.mtx: 3.0 us in the kernel, 4.9 us from dispatch to dispatch in a hipGraph, 6.4 us of
// loop wall per product: profiles/r04_cli_n1000.txt).  Here the workgroups stay: every one walks its share of the launch's
// grid once per product, and between two products all of them meet at a barrier that orders TIME only -- the products
// are independent (x is never changed, y is overwritten with the same values), so nothing has to become visible to anybody
// and the barrier needs no release / acquire fences (which are what a grid barrier mostly costs: MI355X_MICROARCH price
// list, barrier-xcd): arrivals are counted on about sqrt(workgroups) sharded counters (device-scope atomics run at the memory
// side, ~12 ns each on one address: different addresses take them in parallel), the last arrival of a shard counts on a top counter,
// everybody polls that one with sc1 loads.  Every wave stamps the wall clock when it passes the barrier into product i and
// when its last store of product i has been acknowledged: the same {first, last} slots the stamped single launches write,
// reduced by stamp_reduce -- windows that cannot overlap, one per product, inside one launch.
//
// The grid must be resident as a whole (the launcher sizes it from the occupancy query, with a margin); every poll is
// bounded all the same: a workgroup that waits longer than the launch's patience (50 ms unless the caller says otherwise --
// a product of a grid that is resident at once takes microseconds) sets the top counter's abort bit and the run's sticky
// give-up word, everybody leaves, launches of the same run queued behind it leave as they start, and the host -- which waits
// for the FIRST launch of a run before it queues the others -- falls back to single launches.
// ---------------------------------------------------------------------------
constexpr int kRepeatMaxShards = 32;
constexpr unsigned kRepeatAbort = 0x80000000u;

// ctl_words (kRepeatCtlWords unsigned, every word on a 128-byte line of its own): line 0 the STICKY give-up word of a run -- set by the
// launch that gives up, never cleared between the launches of one run, read by every workgroup of a later launch before it
// does anything: launches already enqueued behind one that gave up leave at once instead of waiting out their own patience;
// lines 1..32 the shard counters, 33..64 the go words, the last line the top counter (bit 31: this launch gave up).
struct RepeatCtl {
    unsigned *sticky = nullptr;  // the run's give-up word (see above)
    unsigned *shard = nullptr;   // `shards` counters, 32 words (128 B) apart
    unsigned *top = nullptr;     // one counter; bit 31 = abort
    unsigned *go = nullptr;      // `shards` generation words, 128 B apart: what the workgroups of a shard poll (sharded grids)
    unsigned long long *stamps = nullptr;  // reps * slots_per_product * 2
    int reps = 0, grid_virtual = 0, slots_per_product = 0;
    int shards = 1;              // 1: every workgroup counts on `top` itself (small grids); else about sqrt(workgroups), a power of two
    unsigned long long patience = 0;  // ticks of the 100 MHz wall clock a workgroup waits at one barrier before the launch gives up
};

template <int VPT, int FLAVOR>
__global__ __launch_bounds__(kStreamBlock) void csr_stream_owner_repeat(
    const int *__restrict__ row_ptr, const int *__restrict__ col_ind, const double *__restrict__ val,
    const double *__restrict__ x, double *__restrict__ y, const int *__restrict__ tile_row,
    const int *__restrict__ tile_next, int rows, int nnz_arg, int ntiles, int tile_group_arg, const OwnerExtra ex, const RepeatCtl ctl)
{
    __shared__ unsigned go;
    const int t = threadIdx.x;
    const unsigned nwg = gridDim.x, me = blockIdx.x;
    const unsigned S = (unsigned)ctl.shards;
    const unsigned sh = me % S;
    const unsigned members = (nwg - sh + S - 1) / S;   // workgroups of this shard
    const unsigned arrivals = S > 1 ? (nwg < S ? nwg : S) : nwg;  // what `top` counts per product: shards with members, or workgroups
    unsigned long long *stamp = ctl.stamps + 2 * ((size_t)me * (kStreamBlock / 64) + (t >> 6));
    // an earlier launch of this run gave up: so does this one, at once (and says so on its own top word, which the host reads)
    if (t == 0) {
        go = __hip_atomic_load(ctl.sticky, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 0u : 1u;
        if (!go)
            atomicOr(ctl.top, kRepeatAbort);
    }
    __syncthreads();
    if (!go)
        return;
    for (int rep = 0; rep < ctl.reps; ++rep) {
        // ---- every workgroup has finished product rep - 1 (its stores acknowledged) before anybody starts product rep
        __syncthreads();
        if (t == 0) {
            const unsigned gen = (unsigned)rep + 1u;
            const unsigned long long t0 = wall_clock64();
            unsigned seen = 0;
            if (S > 1) {
                // arrivals: shard counter, its last arrival on the top counter, ITS last arrival writes the generation into
                // every shard's go word -- which is what a shard's workgroups poll: polls and arrivals never meet on one
                // address (all workgroups polling the top counter held up the arrivals on it: 32 shards 7.0 us per product
                // against 4.96 with 8, memplus.mtx; a one-level form in which every workgroup's first wavefront polled all
                // shard counters ran at 7-15 us: the polls also slow the workgroups that are still multiplying;
                // profiles/r05_cli_n1000.txt)
                const unsigned before = atomicAdd(ctl.shard + 32 * sh, 1u);
                if (before + 1u == members * gen) {
                    const unsigned tb = atomicAdd(ctl.top, 1u);
                    // (a maximum, not a store: a go word that already says kRepeatAbort -- the largest unsigned in play --
                    // keeps saying it, whoever arrives last)
                    if ((tb & ~kRepeatAbort) + 1u == arrivals * gen)
                        for (unsigned q = 0; q < S; ++q)
                            __hip_atomic_fetch_max(ctl.go + 32 * q, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                for (;;) {
                    const unsigned g = __hip_atomic_load(ctl.go + 32 * sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (g >= gen && g != kRepeatAbort)
                        break;
                    if (g == kRepeatAbort) {
                        seen = kRepeatAbort;
                        break;
                    }
                    if (wall_clock64() - t0 > ctl.patience) {
                        atomicOr(ctl.top, kRepeatAbort);
                        __hip_atomic_store(ctl.sticky, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        for (unsigned q = 0; q < S; ++q)
                            __hip_atomic_fetch_max(ctl.go + 32 * q, kRepeatAbort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        seen = kRepeatAbort;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(2);
                }
            } else {
                atomicAdd(ctl.top, 1u);  // (result unused: no round trip in front of the poll)
                for (;;) {
                    seen = __hip_atomic_load(ctl.top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((seen & kRepeatAbort) || (seen & ~kRepeatAbort) >= arrivals * gen)
                        break;
                    if (wall_clock64() - t0 > ctl.patience) {
                        atomicOr(ctl.top, kRepeatAbort);
                        __hip_atomic_store(ctl.sticky, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        seen = kRepeatAbort;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
            }
            go = seen & kRepeatAbort ? 0u : 1u;
        }
        __syncthreads();
        if (!go)
            return;  // (uniform: the whole workgroup read the same word)
        if ((t & 63) == 0)
            stamp[0] = wall_clock64();
        for (int vb = (int)me; vb < ctl.grid_virtual; vb += (int)nwg) {
            if (vb != (int)me)
                __syncthreads();  // the previous tile's LDS is free
            // (a zero the compiler cannot see through, added to the lane's first entry: the per-lane stream addresses of phase 1
            // are then formed per tile as in the single launch instead of being kept in registers across this loop -- 85-87
            // instead of 73 registers at VPT 8, 60-62 instead of 47-50 at VPT 4, a workgroup per CU and a fifth of
            // repeat_capacity() fewer)
            int salt = 0;
            asm volatile("" : "+v"(salt));
            owner_body<VPT, FLAVOR, false>(row_ptr, col_ind, val, x, y, tile_row, tile_next, rows, nnz_arg, ntiles, tile_group_arg, ex, vb, salt);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if ((t & 63) == 0)
            stamp[1] = wall_clock64();
        stamp += 2 * (size_t)ctl.slots_per_product;
    }
}

// One workgroup per product of a stamped run: min of the waves' first ticks, max of their last.
__global__ __launch_bounds__(256) void stamp_reduce(const unsigned long long *__restrict__ stamps, int slots_per_product,
                                                    unsigned long long *__restrict__ first_last)
{
    __shared__ unsigned long long lo_s[256 / 64], hi_s[256 / 64];
    const unsigned long long *s = stamps + (size_t)blockIdx.x * slots_per_product * 2;
    unsigned long long lo = ~0ull, hi = 0ull;
    for (int i = threadIdx.x; i < slots_per_product; i += 256) {
        const unsigned long long f = s[2 * i], l = s[2 * i + 1];
        lo = f < lo ? f : lo;
        hi = l > hi ? l : hi;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long ol = __shfl_down(lo, off, 64), oh = __shfl_down(hi, off, 64);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
    }
    if ((threadIdx.x & 63) == 0) {
        lo_s[threadIdx.x >> 6] = lo;
        hi_s[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 256 / 64; ++w) {
            lo = lo_s[w] < lo ? lo_s[w] : lo;
            hi = hi_s[w] > hi ? hi_s[w] : hi;
        }
        first_last[2 * blockIdx.x] = lo;
        first_last[2 * blockIdx.x + 1] = hi;
    }
}

// grid of a launch of `ntiles` tiles (a multiple of 8 * group, see tile_of_block)
static unsigned owner_grid(int ntiles, int group) { return tile_grid_of(ntiles, group); }

// tiles per XCD turn by flavour.  CSR measured best at 64 (profiles/r01_tile_group_sweep.txt).  The tile-ordered TJDS stream: the
// group decides how often x_perm crosses the fabric -- a copy of memplus is 61 tiles, every XCD that gets some of them pulls
// the copy's part of x_perm -- but not the time (round 5, memplus x944, PMC FETCH per product / ms; x_perm's share in brackets):
// group 4: 2125 MB (388)   16: 2059 (333) 0.390   32: 1983 (258) 0.391   48: 1934 (211) 0.392   64: 1907 (185) 0.395   256: 1841 (126)
// pwt x459: 0.263-0.267 / 0.265-0.267 / 0.267-0.268 / 0.269-0.270 ms for 16 / 32 / 48 / 64.  32 moves 76 MB less at the same speed.
static int flavor_group(int flavor) { return flavor == kFlavorTjdsS || flavor == kFlavorTjdsH ? kTjdsTileGroup : kStreamTileGroup; }

int owner_stamp_slots(int ntiles, int flavor)
{
    return (int)owner_grid(ntiles, tile_group(ntiles, flavor_group(flavor))) * (kStreamBlock / 64);
}

hipError_t launch_csr_stream_owner(int vpt, int flavor, const OwnerLaunch &l, hipStream_t stream)
{
    if (l.rows <= 0)
        return hipSuccess;
    const int group = tile_group(l.ntiles, flavor_group(flavor));
    const dim3 grid(owner_grid(l.ntiles, group));
    OwnerExtra ex = owner_extra_of(l, l.stamps);
    ex.back_grid = l.backward ? (int)grid.x : 0;  // (both units' kernels read it: the CSR unit launches with this `ex`)
#define SMVP_OWNER_ST(V, F, S)                                                                                     \
    hipLaunchKernelGGL((csr_stream_owner<V, F, S>), grid, dim3(kStreamBlock), 0, stream, l.row_ptr, l.col_ind, l.val, \
                       l.x, l.y, l.tile_row, l.tile_next, l.rows, l.nnz, l.ntiles, group, ex)
#define SMVP_OWNER(V, F)                  \
    if (vpt == V && flavor == F) {        \
        if (l.stamps)                     \
            SMVP_OWNER_ST(V, F, true);    \
        else                              \
            SMVP_OWNER_ST(V, F, false);   \
        return hipGetLastError();         \
    }
#ifdef SMVP_PHASE_STAMPS   // (diagnostic builds keep every flavour here: one set of phase counters)
    SMVP_OWNER_CSR_FORMS(SMVP_OWNER)
    SMVP_OWNER_CSR_PACKED_FORMS(SMVP_OWNER)
#else
    // the CSR flavours are instantiated in smvp_owner_csr.hip, under the max-ILP scheduling strategy
    if (flavor == kFlavorCsr || flavor == kFlavorCsr16 || flavor == kFlavorCsr16P)
        return launch_owner_csr(vpt, flavor, l, ex, grid.x, group, stream);
#endif
    SMVP_OWNER_TJDS_FORMS(SMVP_OWNER)
#undef SMVP_OWNER
#undef SMVP_OWNER_ST
    return hipErrorInvalidValue;
}

// ---- the repeating form (csr_stream_owner_repeat): `reps` products in one launch
// Workgroups of the repeating launch for a plan of `ntiles` tiles: the plain launch's grid -- every workgroup its one tile per
// product, as in a launch of its own -- if that grid is resident at once with room to spare (the occupancy query can read one
// workgroup per CU high, MI355X_MICROARCH "Residency"); 0: the grid is larger (a capped grid whose workgroups walk several tiles
// per product runs each product slower than a launch of its own does -- memplus x2 ... x32: windows of 4.8 ... 17.9 us against
// 3.3 ... 12.8, profiles/r05_cli_n1000.txt -- so those matrices keep one launch per product), this (vpt, flavor) has no repeating
// form, or the device could not be asked.
template <int V, int F>
static int repeat_capacity()
{
    int per_cu = 0, dev = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, csr_stream_owner_repeat<V, F>, kStreamBlock, 0) != hipSuccess ||
        hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return per_cu > 1 ? (per_cu - 1) * cus * 3 / 4 : 0;  // three quarters of (one workgroup per CU fewer than the query's answer)
}

int owner_repeat_grid(int vpt, int flavor, int ntiles)
{
    if (ntiles <= 0)
        return 0;
    int cap = 0;
#define X(V, F)                     \
    if (vpt == V && flavor == F)    \
        cap = repeat_capacity<V, F>();
    SMVP_OWNER_REPEAT_FORMS(X)
#undef X
    if (cap <= 0)
        return 0;
    const int full = (int)owner_grid(ntiles, tile_group(ntiles, flavor_group(flavor)));
    return full <= cap ? full : 0;
}

// `reps` products, each stamped: stamps[reps][grid * 4][2]; ctl_words: kRepeatCtlWords unsigned -- the counters are cleared here
// for every launch, the sticky give-up word only for the first launch of a run.  Refuses (hipErrorInvalidValue, nothing is
// launched) a launch whose control block would be incomplete: no stamps, no control words, no products, no tiles to walk.
hipError_t launch_csr_stream_owner_repeat(int vpt, int flavor, const OwnerLaunch &l, int reps, int grid, unsigned *ctl_words,
                                          bool first_of_run, unsigned long long patience_ticks, hipStream_t stream)
{
    if (l.rows <= 0)
        return hipSuccess;
    const int group = tile_group(l.ntiles, flavor_group(flavor));
    RepeatCtl ctl{};
    ctl.sticky = ctl_words;
    ctl.shard = ctl_words + 32, ctl.go = ctl_words + 32 * (1 + kRepeatMaxShards), ctl.top = ctl_words + kRepeatCtlWords - 32;
    // arrivals cost about 12 ns each on one address: n / S on a shard, then S on the top counter
    // measured (profiles/r05_cli_n1000.txt): one level up to two dozen workgroups, 8 shards up to ~600, 16 beyond
    ctl.shards = grid <= 24 ? 1 : grid <= 640 ? 8 : 16;
    ctl.stamps = l.stamps;
    ctl.reps = reps, ctl.grid_virtual = (int)owner_grid(l.ntiles, group), ctl.slots_per_product = grid * (kStreamBlock / 64);
    ctl.patience = patience_ticks;
    if (reps <= 0 || grid <= 0 || ctl.grid_virtual <= 0 || !ctl.stamps || !ctl_words)
        return hipErrorInvalidValue;
    static_assert(kRepeatCtlWords == 32 * (2 + 2 * kRepeatMaxShards), "sticky + shards + go words + top, one 128-byte line each");
    hipError_t e = first_of_run ? hipMemsetAsync(ctl_words, 0, sizeof(unsigned) * kRepeatCtlWords, stream)
                                : hipMemsetAsync(ctl_words + 32, 0, sizeof(unsigned) * (kRepeatCtlWords - 32), stream);
    if (e != hipSuccess)
        return e;
    const OwnerExtra ex = owner_extra_of(l, nullptr);
#define X(V, F)                                                                                                                    \
    if (vpt == V && flavor == F) {                                                                                                 \
        hipLaunchKernelGGL((csr_stream_owner_repeat<V, F>), dim3((unsigned)grid), dim3(kStreamBlock), 0, stream, l.row_ptr, l.col_ind, \
                           l.val, l.x, l.y, l.tile_row, l.tile_next, l.rows, l.nnz, l.ntiles, group, ex, ctl);                     \
        return hipGetLastError();                                                                                                  \
    }
    SMVP_OWNER_REPEAT_FORMS(X)
#undef X
    return hipErrorInvalidValue;
}

#ifdef SMVP_PHASE_STAMPS
void debug_owner_phases()
{
    unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0}, z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_owner_phase), sizeof h) != hipSuccess || h[7] == 0)
        return;
    const double n = (double)h[7];
    fprintf(stderr, "[owner dbg] mean us per workgroup over %.0f: loads + gathers + LDS writes %.2f | barrier %.2f | lane-per-row sums %.2f | "
                    "barrier %.2f | long rows %.2f\n", n, h[0] * 0.01 / n, h[1] * 0.01 / n, h[2] * 0.01 / n, h[3] * 0.01 / n, h[4] * 0.01 / n);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_owner_phase), z, sizeof z);
}
#else
void debug_owner_phases() {}
#endif

hipError_t launch_stamp_reduce(const unsigned long long *stamps, int slots_per_product, int products,
                               unsigned long long *first_last, hipStream_t stream)
{
    if (products <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(stamp_reduce, dim3(products), dim3(256), 0, stream, stamps, slots_per_product, first_last);
    return hipGetLastError();
}

}  // namespace smvp
