// smvp_owner_kernel.h -- the device side of K2', the owner (tile) kernel: owner_body and the two kernel templates that wrap
// it, csr_stream_owner and read_once::csr_stream_owner, with the list of forms the library instantiates.  Two units include it
// and each is compiled once: smvp_owner.hip (default scheduling: the TJDS flavours' plain launches, the repeating form of every
// flavour, the stamp reduction) and smvp_owner_csr.hip (max-ILP scheduling, see the Makefile: the CSR flavours' plain launches).
// Nothing in this file depends on which of the two is being compiled.
#pragma once
#include "smvp_kernels.h"

namespace smvp {

// Blocks are dealt round-robin over the 8 XCDs (b and b+8 share an L2).  Tiles are
// handed out in groups: XCD i takes `group` consecutive tiles out of every run of
// 8*group, so an XCD's L2 sees neighbouring rows (and re-uses their x lines) while
// all eight XCDs stay within 8*group tiles of each other in memory.  Measured on
// MI355X (profiles/r01_tile_group_sweep.txt; % of HBM peak on memplus x944 / on the
// random model, L2->fabric read bytes per launch):
//   group 1     64.9 / 18.7   2.08 GB      group 128   64.4 / 21.8   1.68 GB
//   group 8     65.5 / 19.3   1.91 GB      group 512   62.2 / 21.7   1.61 GB
//   group 32    65.2 / 21.2   1.84 GB      group 2048  55.9 / 20.8   1.60 GB
// (one XCD per contiguous eighth of the matrix was 60.1 %).  64 keeps the speed of
// the small groups and most of the traffic saving of the large ones.
// Speed only: any placement gives the same result.  (tile_of_block itself lives in
// smvp_tile_map.h: K7 and K10, smvp_spmm.hip, deal their row blocks the same way.)
// The owner kernel deals its tiles in either direction, tile_of_block_swept: the plain launches of a
// handle whose matrix is larger than the 256 MiB Infinity Cache alternate, so a product starts on the
// tiles the one before it touched last -- what the cache still holds (DESIGN.md section 4, K2:
// memplus x944 +4.2 %, x300 +10.3 %; a matrix the caches hold keeps the forward sweep, where every
// XCD finds its own tiles in its L2).

// ---------------------------------------------------------------------------
// K2': the tiles of K2 (csr_stream_tiles, smvp_kernels.hip), but the tile in which a row STARTS finishes that row
// itself: it also loads the few entries past its end that belong to its last
// row (tile_next[b] = row_ptr[first row of the next tile] says how many) into an
// LDS overflow area.  No carries, no second launch, and every row of up to
// kLongRow entries is summed left to right by one lane -- bit-identical to the
// serial loop -- wherever it lies.  A tile in which no row starts exits at once.
// A last row that runs more than kStreamOver entries past the tile is finished
// by the whole workgroup straight from global memory; matrices with rows far
// longer than that are planned onto the carry kernel, K2, instead, which
// spreads such a row over many workgroups.
//
// Phase 1's lane layout (row-ordered flavours, VPT 4 and 8): neighbouring lanes take neighbouring entries.  A wavefront takes
// 64 * VPT consecutive entries; of each 128-entry slab of them lane l has entries 2 l and 2 l + 1.  Every load is then a
// contiguous run (double2 of val: 1 KiB per wave instruction; one 32-bit word of two 16-bit offsets: 256 B), a gather
// instruction covers 64 entries two apart instead of 64 entries eight apart (memplus: 21.5 instead of 36.5 distinct 64-byte
// lines of x per instruction, pwt: 11.8 instead of 20.9), and the double2 product stores go to LDS at a 16-byte lane stride.
// Until then lane t had the 8 consecutive entries 8 t ... 8 t + 7: every lane its own 64-byte line of val, and product
// stores at a 64-byte stride that put lanes t and t + 4 on one bank.  Measured on memplus x944, per launch
// (profiles/tile_lane_layout_measured.txt): vector-L1 accesses 138.7 M -> 108.8 M, LDS bank-conflict cycles 28.1 M -> 5.8 M,
// bytes unchanged, 0.2693 -> 0.2612 ms (median of seven alternated processes, every one faster than every one of the old
// layout); pwt x459 unchanged.  The L1 count fell by 22 %, not by the factor the distinct-line count predicts: the kernel is
// not bound by the L1's address path.  The lane-strided alternative (entry 64 k + l; 8-byte and 2-byte loads) was built and
// measured too: 115.3 M accesses, two thirds more load instructions, headline -1.2 %, pwt x459 +2.7 % -- not merged.
// prod[] holds every product at its row-major place whatever the layout, so phase 2 and every sum's order are untouched.
// Since then, at 2048-entry tiles, Csr16's offsets lie in the plan in the order the lanes hold them (smvp::col16_slot): one
// 16-byte load per lane instead of four 4-byte words, and products larger than the caches run the read_once:: form of the kernel
// below (profiles/col16_lane_order_measured.txt: memplus x944 0.2616 -> 0.2507 ms, pwt x459 -7.7 %).
//
// FLAVOR selects what an "entry" is (owner_entry below):
//   kFlavorCsr     CSR: value val[j], operand x[col_ind[j]]                       (main-cli.c:410-416)
//   kFlavorCsr16   the same product with 10 instead of 12 bytes per entry: for the tiles whose columns span less than 65536
//                  (banded and block-structured matrices: all of them) the plan keeps col_ind a second time as 16-bit
//                  offsets from the tile's smallest column; the tile adds its base (one scalar) back.  Wider tiles
//                  (col_base < 0), overflow entries and the slow paths read col_ind itself.
//   kFlavorCsr16P  kFlavorCsr16 at 2048-entry tiles with 1 + 2 + 8 * (escape share) instead of 10 bytes per entry: for the full narrow
//                  ("packable") tiles the plan keeps val a second time as one byte per entry, in col16_slot order -- an index into
//                  a table of the matrix's 64 most frequent bit patterns, or 255 -- and the values that are not in the table
//                  (escapes) wavefront by wavefront in the order the lanes hold them.  Every value is the double val holds, bit for
//                  bit, and every row is summed as kFlavorCsr16 sums it: y is bit-identical.  Wide tiles, the last partial tile,
//                  overflow entries and the slow paths read val itself.  (SMVP_CSR_KERNEL_STREAM_PACKED)
//                  What the plan says of a tile -- its rows, its column base, where its escapes lie, whether it is packable -- is
//                  six words of four arrays, requested together and waited for once, and a packable tile's phase 1 is
//                  straight-line: every stream load in one flight behind them, one wait, the gathers
//                  (profiles/tile_record_measured.txt).
//   kFlavorTjdsK   TJDS by rows: the stream lists, row by row, the TJDS positions p of the row's entries (`pos`) and
//                  their permuted columns k (`col_ind`): value val[p] gathered from the jagged-diagonal array,
//                  operand x_perm[k] (the one-kernel TJDS product, see ensure_row_gather in the engine)
//   kFlavorTjdsS   the same rows, but inside every tile the entries are listed in TJDS order (ascending position):
//                  the tile walks its piece of the jagged diagonals the way the format stores them -- neighbouring
//                  lanes read neighbouring val / x_perm entries, lane t takes entries t, t + 256, ... of the tile --
//                  and each product goes to the LDS slot of its row-major place (`col_ind` holds slot | diagonal << 11);
//                  the entries a tile needs from beyond its end are kept a second time in row order (ovf_*)
//   kFlavorTjdsH   kFlavorTjdsS with 4 bytes of index per entry instead of 8: two 16-bit halves of one word.  One is the LDS slot | the
//                  number, modulo 32, of the entry's RUN: a stretch of the tile's sorted entries inside one jagged diagonal
//                  and one aligned block of 2^16 positions (the tile's cached entries, which need only their column, are
//                  sorted by column and form runs by blocks of 2^16 columns).  The other is the low half of the position
//                  (cached: of the column).  The tile's run table holds {base, sub} per run: position = base + low half,
//                  operand index = position - sub (sub = start_pos of the run's diagonal; cached: 0).  An entry finds its
//                  run from the run of its group of 32 entries (`group_run`, one 16-bit word per group) and the 5-bit hint;
//                  the table sits in a wavefront's registers (a handful of runs per tile on banded matrices), so the two
//                  gathers follow the streams after two cross-lane reads.
// ---------------------------------------------------------------------------
typedef int int4v __attribute__((ext_vector_type(4)));               // clang vectors: what the non-temporal builtins take
typedef int int2v __attribute__((ext_vector_type(2)));
typedef double double2v __attribute__((ext_vector_type(2)));

// The streams every flavour reads are plain __restrict__ kernel parameters (the compiler then keeps the uniform plan
// reads on the scalar unit and is free to order the loads); what only some flavours need travels in this struct.
// Csr16P's four arrays travel in the words of four that only the TJDS flavours read (a flavour is one or the other; PackedArrays
// below is how the kernel reads them): the struct keeps its size, its fields and their types, so every other form of the kernel --
// and the repeating kernel, whose control block follows this struct in the argument block -- is the code it was before the flavour
// existed (as unions of two pointers the TjdsH forms already came out with other registers).
struct OwnerExtra {
    const int *pos = nullptr;                 // Tjds*: TJDS position of each stream entry                          (Csr16P: code8)
    const int *start_pos = nullptr;           // TjdsS
    const int *ovf_ptr = nullptr;             // TjdsS: ntiles + 1 bounds of the tiles' overflow entries in ovf_val / ovf_k   (Csr16P: esc_ptr)
    const double *ovf_val = nullptr;          // TjdsS: value ...                                                    (Csr16P: esc_val)
    const int *ovf_k = nullptr;               // TjdsS: ... and permuted column of the entries [e, tile_next) of each tile, row order
    const int *cache_ptr = nullptr;           // TjdsS: ntiles + 1 bounds of the tiles' runs in val_cache (a tile's last entries)
    const double *val_cache = nullptr;        // TjdsS: values of the entries whose val lines scatter over many tiles, tile by tile   (Csr16P: hot)
    const unsigned short *col16 = nullptr;    // Csr16: column - col_base[tile] per entry
    const int *col_base = nullptr;            // Csr16: smallest column of every tile
    const unsigned *word32 = nullptr;         // TjdsH, per entry: low 16 bits of its position (cached entries: of its permuted column) | (slot | run hint << kSlotBits) << 16
    const unsigned short *group_run = nullptr;  // TjdsH: per tile and group of 32 entries, the run (inside the tile) of its first entry
    const int *run_ptr = nullptr;             // TjdsH: ntiles + 1 bounds of the tiles' runs in run_tab
    const int *run_tab = nullptr;             // TjdsH: per run {base of its block of 2^16 positions, start_pos of its diagonal} (cached: {column block, 0})
    int unit_x = 0;                     // TjdsH: the operand is the unit vector -- no x gather; overflow entries are POSITIONS in ovf_k (their
                                    // values are read from val like everybody's: val changes from launch to launch, see the engine's TjdsSource)
    const unsigned short *row_rel = nullptr;  // every row's first entry relative to the first entry of the tile it
                                    // starts in (2 B per row read by the product instead of row_ptr's 4); nullptr: row_ptr itself
    unsigned long long *stamps = nullptr;     // STAMPED: per-wave {first, last} wall-clock ticks of this launch
    int back_grid = 0;                  // 0: the tiles are swept forward; else the launch's grid, and they are swept backward
                                    // (tile_of_block_swept; set by the plain launcher alone, the repeating launch stays forward)
};

// The ONE place an OwnerExtra is filled from a launch description (the plain launcher, the CSR unit's launcher through it, the
// repeating launcher): a field added to either struct is carried -- or left at its null default -- here and nowhere else.
inline OwnerExtra owner_extra_of(const OwnerLaunch &l, unsigned long long *stamps)
{
    OwnerExtra ex{};
    ex.pos = l.pos, ex.start_pos = l.start_pos, ex.ovf_ptr = l.ovf_ptr, ex.ovf_val = l.ovf_val, ex.ovf_k = l.ovf_k;
    ex.cache_ptr = l.cache_ptr, ex.val_cache = l.val_cache;
    ex.col16 = l.col16, ex.col_base = l.col_base;
    ex.unit_x = l.unit_x, ex.word32 = l.word32, ex.group_run = l.group_run, ex.run_ptr = l.run_ptr, ex.run_tab = l.run_tab;
    ex.row_rel = l.row_rel;
    ex.stamps = stamps;
    if (l.code8)  // Csr16P (never together with the TJDS arrays whose words these take)
        ex.pos = reinterpret_cast<const int *>(l.code8), ex.ovf_ptr = l.esc_ptr, ex.ovf_val = l.esc_val, ex.val_cache = l.hot;
    return ex;
}

// Csr16P's arrays as the kernel reads them out of an OwnerExtra (see there)
struct PackedArrays {
    const unsigned char *__restrict__ code8;  // per entry of a packable tile, in col16_slot order: 0 ... 63 = index into hot, kEscapeCode = escape
    const int *__restrict__ esc_ptr;          // 4 * ntiles + 1 starts of the wavefronts' runs in esc_val (a tile that is not packable: ~start, negative)
    const double *__restrict__ esc_val;       // the escapes' values in the order (tile, wavefront, lane, k), every run padded to an even count
    const double *__restrict__ hot;           // kHotValues doubles, the matrix's most frequent bit patterns
};
__device__ __forceinline__ PackedArrays packed_arrays_of(const OwnerExtra &ex)
{
    return {reinterpret_cast<const unsigned char *>(ex.pos), ex.ovf_ptr, ex.ovf_val, ex.val_cache};
}

// what the helpers below need of the kernel's arguments
struct OwnerArgs {
    const int *__restrict__ col_ind;
    const double *__restrict__ val;
    const double *__restrict__ x;
    const int *__restrict__ pos;
    const int *__restrict__ start_pos;
    const double *__restrict__ ovf_val;
    const int *__restrict__ ovf_k;
    int unit_x;   // TjdsH: overflow entries are positions, the operand is 1 (OwnerExtra::unit_x)
};

// one entry's product the slow way (tile tails, overflow beyond one block width, giant rows)
template <int FLAVOR>
__device__ __forceinline__ double owner_product_slow(const OwnerArgs &a, long long j)
{
    if constexpr (FLAVOR == kFlavorCsr || FLAVOR == kFlavorCsr16 || FLAVOR == kFlavorCsr16P)
        return a.val[j] * a.x[a.col_ind[j]];
    else if constexpr (FLAVOR == kFlavorTjdsK)
        return a.val[a.pos[j]] * a.x[a.col_ind[j]];
    else {
        const int p = a.pos[j];
        return a.val[p] * a.x[p - a.start_pos[(unsigned)a.col_ind[j] >> kSlotBits]];
    }
}

// product of overflow entry `i` of tile b (stream entry e + i, the i-th entry past the tile's end)
template <int FLAVOR>
__device__ __forceinline__ double owner_overflow_product(const OwnerArgs &a, int ovf_base, int e, int i)
{
    if constexpr (FLAVOR == kFlavorTjdsS || FLAVOR == kFlavorTjdsH)
        return a.unit_x ? a.val[a.ovf_k[ovf_base + i]] : a.ovf_val[ovf_base + i] * a.x[a.ovf_k[ovf_base + i]];
    else
        return owner_product_slow<FLAVOR>(a, (long long)e + i);
}

// Diagnostic builds only (make HIPFLAGS+=-DSMVP_PHASE_STAMPS): where a workgroup of the owner kernel spends its time.
// Thread 0 of every workgroup adds the 100 MHz wall-clock ticks between its phase boundaries to six global counters;
// smvp_debug_phase_stamps() (engine) prints and clears them.  The normal build contains none of this.
// (static: both owner units see this header.  In this build smvp_owner.hip launches every flavour, so its copy holds the one set
// of counters, which its debug_owner_phases reads; smvp_owner_csr.hip instantiates no kernel and its copy is never touched.)
#ifdef SMVP_PHASE_STAMPS
[[maybe_unused]] static __device__ unsigned long long g_owner_phase[8];
#define SMVP_PHASE(n)                                                                        \
    do {                                                                                     \
        if (threadIdx.x == 0 && (blockIdx.x & 127) == 5) {                                   \
            const unsigned long long now_ = wall_clock64();                                  \
            if ((n) > 0)                                                                     \
                atomicAdd(&g_owner_phase[(n)-1], now_ - phase_prev_);                        \
            else                                                                             \
                atomicAdd(&g_owner_phase[7], 1ull);                                          \
            phase_prev_ = now_;                                                              \
        }                                                                                    \
    } while (0)
#else
#define SMVP_PHASE(n) do { } while (0)
#endif

// Diagnostic builds only (make ... HIPFLAGS+=-DSMVP_TJDS_NEUTRALISE=mask; tools/tjds_traffic_by_stream.sh): the tile-ordered TJDS
// product with one of its streams taken out -- WRONG results, the PMC counters then show what that stream moves.
// 1: the x_perm gathers (operand 1.0)   2: the in-place val gathers (val[position])   4: the value cache's reads
// 8: the overflow entries (their index, value and operand loads).  The normal build contains none of this.
#ifndef SMVP_TJDS_NEUTRALISE
#define SMVP_TJDS_NEUTRALISE 0
#endif

// Csr16P: the 8 values of this lane's entries of a packable tile from its codes (code_lo, code_hi), its entry of the hot table and
// its pairs ev[] of the wavefront's escapes, without a further trip to memory and without a byte of LDS of its own: the
// wavefront's escapes are staged in ITS OWN 512-entry part of prod[] -- where its products land afterwards and which no other
// wavefront touches before the barrier (a wavefront has at most 512 escapes) -- and a hot value comes from the lane that holds
// it.  LDS executes one wavefront's accesses in order; the wavefront barriers and fences keep the compiler from moving the reads
// above the writes or the caller's product stores above the reads.
__device__ __forceinline__ void packed_decode(double *part, double2v ev0, double2v ev1, double2v ev2, double2v ev3, unsigned code_lo,
                                              unsigned code_hi, double hot, int lane, double (&v)[8])
{
    *reinterpret_cast<double2v *>(&part[2 * lane]) = ev0;
    *reinterpret_cast<double2v *>(&part[2 * lane + 128]) = ev1;
    *reinterpret_cast<double2v *>(&part[2 * lane + 256]) = ev2;
    *reinterpret_cast<double2v *>(&part[2 * lane + 384]) = ev3;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // this lane's escapes follow those of the lanes below it: entry k's share of them is a count of the set bits below
    // this lane in the wavefront's mask for entry k (no cross-lane data movement at all)
    unsigned code[8];
    int before = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        code[k] = ((k < 4 ? code_lo : code_hi) >> (8 * (k & 3))) & 0xffu;
        const unsigned long long mask = __ballot(code[k] == (unsigned)kEscapeCode);
        before = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, (unsigned)before));
    }
    const int hot_lo = __double2loint(hot), hot_hi = __double2hiint(hot);
    int mine = 0;  // escapes among this lane's entries 0 ... k - 1
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const bool escaped = code[k] == (unsigned)kEscapeCode;
        const int from = (int)(code[k] & 63u) << 2;
        const double hot_k = __hiloint2double(__builtin_amdgcn_ds_bpermute(from, hot_hi), __builtin_amdgcn_ds_bpermute(from, hot_lo));
        // (every lane reads, an entry that did not escape from a place inside the part that it then ignores: all eight
        // reads and the sixteen cross-lane reads go out together and are waited for once -- behind a branch per entry
        // the compiler waited for each read by itself)
        const double esc_k = part[(before + mine) & (64 * 8 - 1)];
        v[k] = escaped ? esc_k : hot_k;
        mine += escaped ? 1 : 0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The body of the owner kernel for workgroup number `block` of the launch's grid (the plain kernel passes blockIdx.x; the
// repeating kernel below walks the same grid several times).  Every thread of the workgroup leaves through the same exit.
// STREAMED: the full tiles' val loads (CSR flavours, VPT 4 and 8) and Csr16's 16-byte offset loads carry the read-once hint.
template <int VPT, int FLAVOR, bool STAMPED, bool STREAMED = false>
__device__ __forceinline__ void owner_body(
    const int *__restrict__ row_ptr, const int *__restrict__ col_ind, const double *__restrict__ val,
    const double *__restrict__ x, double *__restrict__ y, const int *__restrict__ tile_row,
    const int *__restrict__ tile_next, int rows, int nnz_arg, int ntiles, int tile_group_arg, const OwnerExtra &ex, const int block, const int lane_salt = 0)
{
    // (Csr16P: ex.pos, ex.ovf_ptr, ex.ovf_val and ex.val_cache are NOT TJDS data but the packed arrays -- see OwnerExtra.  a.pos and
    // a.ovf_val below are then code8 and esc_val under other types; the helpers that take `a` read them for the TJDS flavours alone,
    // each behind `if constexpr` on FLAVOR, never behind a runtime test.  A flavour that reads them otherwise must not share the words.)
    const OwnerArgs a = {col_ind, val, x, ex.pos, ex.start_pos, ex.ovf_val, ex.ovf_k, FLAVOR == kFlavorTjdsH ? ex.unit_x : 0};
    constexpr int TILE = kStreamBlock * VPT;
    constexpr int QCAP = (TILE + kStreamOver) / kLongRow + 1;
    constexpr bool PACKED = FLAVOR == kFlavorCsr16P;  // Csr16 whose packable tiles read codes and escapes instead of val
    static_assert(!PACKED || VPT == 8, "the packed values are laid out for 2048-entry tiles");
    constexpr bool CSR = FLAVOR == kFlavorCsr || FLAVOR == kFlavorCsr16 || PACKED;
    constexpr bool COL16 = FLAVOR == kFlavorCsr16 || PACKED;
    constexpr bool HALF = FLAVOR == kFlavorTjdsH;
    constexpr bool TJDS = FLAVOR == kFlavorTjdsK || FLAVOR == kFlavorTjdsS || HALF;
    constexpr bool SORTED = FLAVOR == kFlavorTjdsS || HALF;  // entries in TJDS order inside the tile, lane-strided
    static_assert(TILE <= (1 << kSlotBits), "slot bits");
    __shared__ double prod[TILE + kStreamOver];
    __shared__ int long_rows[QCAP];  // rows longer than kLongRow and their LDS segments, filled in phase 2b
    __shared__ int long_a[QCAP];
    __shared__ int long_z[QCAP];
    __shared__ int long_count;
    __shared__ double wave_sum[kStreamBlock / 64];

    const int t = threadIdx.x;
#ifdef SMVP_PHASE_STAMPS
    unsigned long long phase_prev_ = 0;
#endif
    // optional device-side timing: every wave notes when it started and (after its last store has been
    // acknowledged) when it finished; max(last) - min(first) over the launch is the product's own duration,
    // free of launch and event overhead (the engine reduces the slots, see stamp_reduce)
    unsigned long long *stamp = nullptr;
    if constexpr (STAMPED) {
        if constexpr (FLAVOR == kFlavorCsr16P)  // (the wavefront's number as a scalar: the pointer then costs this form no vector register pair)
            stamp = ex.stamps + 2 * ((size_t)block * (kStreamBlock / 64) + __builtin_amdgcn_readfirstlane(t >> 6));
        else
            stamp = ex.stamps + 2 * ((size_t)block * (kStreamBlock / 64) + (t >> 6));
        if ((t & 63) == 0)
            stamp[0] = wall_clock64();
    }
#define SMVP_OWNER_EXIT()                                         \
    do {                                                          \
        if constexpr (STAMPED) {                                  \
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      \
            if ((t & 63) == 0)                                    \
                stamp[1] = wall_clock64();                        \
        }                                                         \
        return;                                                   \
    } while (0)

    const int b = tile_of_block_swept(block, tile_group_arg, ex.back_grid);
    if (b >= ntiles)
        SMVP_OWNER_EXIT();
    const int nnz = nnz_arg;
    const long long s = (long long)b * TILE;

    // ---- phase 1: stream + gather + multiply.  Straight-line code, ordered so that nothing waits on more
    // than one dependent round trip: the tile's own index / value loads go out first (they depend on nothing
    // but the block index), then the plan words, then row_ptr for phase 2 and the overflow entries, then ALL
    // gathers (index -> operand is the one dependence that cannot be avoided).  (Csr16P holds itself to it in the emitted code:
    // the plan words go out in one flight of scalar loads, and a packable tile's loads stand in one block of their own, `fast` below.)
    // Lane layout of the row-ordered flavours (Csr, Csr16, TjdsK; the K2' block above has the reasons and the counts): a
    // wavefront takes 64 * VPT consecutive entries of the tile in slabs of 128, and of every slab its lane l has the two
    // entries 2 l and 2 l + 1 -- one 16-byte val load, one 4-byte word of two 16-bit offsets (8 bytes of col_ind / pos), two
    // gathers next to its neighbours', one 16-byte LDS store at the pair's row-major place.  lane_entry(k) is the offset in
    // the tile of this lane's entry k, for the loads, the gathers and prod[] alike.  In the last, partial tile a lane may
    // own entries that exist and entries that do not, so EVERY lane of that tile takes the slow path, entry by entry, each
    // tested by itself (before, only the lanes at and past the end did; the others loaded their 8 entries together).  One
    // tile per matrix, and its longest lane is as slow as before; a matrix of one or a few tiles at VPT 4 / 8 pays it.
    const int e0 = (t >> 6) * (64 * VPT) + (VPT > 1 ? 2 : 1) * (t & 63) + lane_salt;  // (VPT == 1: t.  lane_salt is 0: see the repeat kernel)
    auto lane_entry = [e0](int k) { return e0 + 128 * (k >> 1) + (k & 1); };
    const long long j0 = s + e0;  // VPT == 1: this lane's one entry
    int c[VPT];     // operand index
    int pj[VPT];    // Tjds*: position in val
    double v[VPT];
    const bool full_tile = s + TILE <= (long long)nnz;  // every lane's entries exist (always, except in the last tile)
    int grp[HALF ? VPT : 1];  // TjdsH: run (inside the tile) of the first entry of this entry's group of 32
    // Csr16P: is this tile packable (block-uniform); this lane's 8 codes, its entry of the hot table, its pairs of the wavefront's
    // run [esc_at, esc_end) of escapes
    [[maybe_unused]] bool packed_tile = false;
    [[maybe_unused]] unsigned code_lo = 0, code_hi = 0;
    [[maybe_unused]] int esc_at = 0, esc_end = 0;
    [[maybe_unused]] double hot = 0.0;
    [[maybe_unused]] double2v ev[PACKED ? 4 : 1];
    // Csr16P: the tile's plan words -- its rows, the end of its last row, its column base, this wavefront's run of escapes (whose
    // first word also says whether the tile is packable): six words of four arrays that depend on nothing but the tile number, so
    // all four scalar loads go out together and are waited for ONCE.  `fast`: a full packable tile of a plan with row_rel takes the
    // block below for its phase 1; every other tile the generic code, which finds these words loaded.
    [[maybe_unused]] int pw_rlo = 0, pw_rhi = 0, pw_zend = 0, pw_base = 0;
    bool fast = false;
    [[maybe_unused]] double fast_p[PACKED ? VPT : 1], fast_po = 0.0;  // what the fast block hands to the common code: p[], po, rp_*
    [[maybe_unused]] int fast_rp[4] = {0, 0, 0, 0};
    if constexpr (PACKED) {
        SMVP_PHASE(0);  // (diagnostic builds: this flavour's first phase starts at entry, the plan words' trip included)
        const PackedArrays pk = packed_arrays_of(ex);
        const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
        esc_at = pk.esc_ptr[4 * b + wv];
        const int esc_next = pk.esc_ptr[4 * b + wv + 1];
        pw_rlo = tile_row[b], pw_rhi = tile_row[b + 1];
        pw_zend = tile_next[b];
        pw_base = ex.col_base[b];
        // (pinned: the compiler otherwise moves the loads whose words are used only behind the exit below past it -- a second trip)
        asm volatile("" ::"s"(esc_next), "s"(pw_zend), "s"(pw_base));
        if (pw_rlo == pw_rhi)
            SMVP_OWNER_EXIT();  // all of this tile continues a row owned by an earlier tile
        esc_end = esc_next < 0 ? ~esc_next : esc_next;  // (the next tile may be one that is not packable)
        packed_tile = esc_at >= 0;  // the same for the four wavefronts of a tile
        fast = full_tile && packed_tile && ex.row_rel != nullptr;
        if (fast) {
            // ---- phase 1 of a packable tile, straight-line: everything that depends on the plan words alone goes out in one flight
            // -- hot[lane], the 8 codes, the masked escape pairs, the 8 offsets, this lane's row bounds for phase 2, the overflow
            // entry -- then ONE wait, the offsets' unpacking, all gathers, the values' decode under them, the multiply.  No branch
            // on a loaded word stands between two loads (a packable tile is narrow: no test of the base, no col_ind alternative).
            const unsigned short *__restrict__ row_rel = ex.row_rel;
            const int rlo = pw_rlo, rhi = pw_rhi, zend = pw_zend, base = pw_base;
            const int lo = (int)s, ext = zend - (lo + TILE);
            const bool over0 = ext <= kStreamOver && t < ext;  // (not the giant row's tile) this lane fetches overflow entry e + t
            const int my = (t >> 6) * (64 * VPT) + (t & 63) * VPT;  // this lane's 8 entries in col16_slot order
            hot = pk.hot[t & 63];
            const int2v *codes = reinterpret_cast<const int2v *>(pk.code8 + s + my);
            const int2v cw = STREAMED ? __builtin_nontemporal_load(codes) : *codes;
            auto escapes = [&](int i) {  // pair i of this lane's, or zeros past the run's end
                const int at = esc_at + 2 * (t & 63) + 128 * i;
                double2v pair = {0.0, 0.0};
                if (at < esc_end) {
                    const double2v *src = reinterpret_cast<const double2v *>(pk.esc_val + at);
                    pair = STREAMED ? __builtin_nontemporal_load(src) : *src;
                }
                return pair;
            };
            const double2v ev0 = escapes(0), ev1 = escapes(1), ev2 = escapes(2), ev3 = escapes(3);
            const int4v *offs = reinterpret_cast<const int4v *>(ex.col16 + s + my);
            const int4v w = STREAMED ? __builtin_nontemporal_load(offs) : *offs;
            const int r1 = rlo + t, r2 = r1 + kStreamBlock;
            if (r1 < rhi) {
                fast_rp[0] = row_rel[r1];
                fast_rp[1] = r1 + 1 < rhi ? (int)row_rel[r1 + 1] : zend - lo;
            }
            if (r2 < rhi) {
                fast_rp[2] = row_rel[r2];
                fast_rp[3] = r2 + 1 < rhi ? (int)row_rel[r2 + 1] : zend - lo;
            }
            int co = 0;
            double vo = 0.0;
            if (over0) {
                co = a.col_ind[lo + TILE + t];
                vo = a.val[lo + TILE + t];
            }
            code_lo = (unsigned)cw.x, code_hi = (unsigned)cw.y;
            double xk[VPT];
#pragma unroll
            for (int k = 0; k < VPT; k += 2) {
                xk[k] = a.x[base + (int)((unsigned)w[k / 2] & 0xffffu)];
                xk[k + 1] = a.x[base + (int)((unsigned)w[k / 2] >> 16)];
            }
            double xo = over0 ? a.x[(unsigned)co] : 0.0;  // (unsigned: no sign extension, hence no wait, inside the overflow branch)
            packed_decode(prod + (t >> 6) * (64 * VPT), ev0, ev1, ev2, ev3, code_lo, code_hi, hot, t & 63, v);
            // (the overflow product needs nothing of the decode: pinned behind it, or the scheduler moves it -- and the wait for
            // all gathers with it -- in front of the decode, which then no longer runs under the gathers)
            asm volatile("" : "+v"(xo));
#pragma unroll
            for (int k = 0; k < VPT; ++k)
                fast_p[k] = v[k] * xk[k];
            fast_po = vo * xo;
        }
    }
    // TjdsH: the tile's run table ({base, sub} per run), one run per lane, requested with the tile's own streams: an entry
    // then takes its run's words from its wavefront's copy by cross-lane reads instead of a second, dependent trip to memory
    // in front of the gathers (tiles with more than 64 runs read the rest from memory)
    int run0 = 0;
    int2 run_tbl = make_int2(0, 0);
    if constexpr (HALF) {
        if (full_tile) {
            run0 = ex.run_ptr[b];
            const int nruns = ex.run_ptr[b + 1] - run0;
            const int ln = t & 63;
            if (ln < nruns)
                run_tbl = reinterpret_cast<const int2 *>(ex.run_tab)[run0 + ln];
        }
    }
    if constexpr (HALF) {
        if (full_tile) {
#pragma unroll
            for (int k = 0; k < VPT; ++k) {
                if constexpr (VPT == 1) {  // 256-entry tiles: a matrix that lives in the caches and is multiplied again and again
                    pj[k] = (int)ex.word32[s + k * kStreamBlock + t];
                } else {
                    pj[k] = (int)__builtin_nontemporal_load(ex.word32 + s + k * kStreamBlock + t);  // low half of the position | (slot | run hint) << 16
                }
                // the two group words of this wavefront's 64 entries are one aligned 32-bit word at a wave-uniform address: a
                // scalar load instead of a vector one per lane
                const unsigned gw = reinterpret_cast<const unsigned *>(ex.group_run)[((size_t)b * (TILE / 32) + k * (kStreamBlock / 32) +
                                                                                     2 * __builtin_amdgcn_readfirstlane(t >> 6)) >> 1];
                grp[k] = (t & 32) ? (int)(gw >> 16) : (int)(gw & 0xffffu);
            }
        }
    } else if constexpr (SORTED) {
        if (full_tile) {
#pragma unroll
            for (int k = 0; k < VPT; ++k) {
                if constexpr (VPT > 1) {  // read once: non-temporal loads leave the L2 to the val / x_perm lines neighbouring tiles share
                    pj[k] = __builtin_nontemporal_load(a.pos + s + k * kStreamBlock + t);
                    c[k] = __builtin_nontemporal_load(a.col_ind + s + k * kStreamBlock + t);
                } else {
                    pj[k] = a.pos[s + k * kStreamBlock + t];
                    c[k] = a.col_ind[s + k * kStreamBlock + t];  // slot | diagonal << kSlotBits
                }
            }
        }
    } else if (full_tile && !fast) {
        if constexpr (VPT >= 4) {
            auto load_cols = [&]() {
#pragma unroll
                for (int k = 0; k < VPT; k += 2)
                    *reinterpret_cast<int2 *>(&c[k]) = *reinterpret_cast<const int2 *>(a.col_ind + s + lane_entry(k));
            };
            if constexpr (PACKED) {
                // Packed values: everything a packable tile reads instead of val goes out here, ahead of the tile's offsets (whose
                // unpacking waits for them inside its branch: after these, the wait covers one flight of loads and not two), and
                // none of it depends on a loaded code -- the lane's 8 codes (one 8-byte load, 512 contiguous bytes per wavefront),
                // hot[lane] (the table is 512 bytes that every tile reads: an L2 hit) and the wavefront's run of escapes, read
                // coalesced: its bounds are among the tile's plan words, lane l takes the pairs at start + 2 l + 128 i.
                // Runs start at even places and have even (padded) lengths, so a pair is 16-byte aligned and whole inside the run.
                // (This is the generic path: a packable tile comes here only in a plan without row_rel; esc_at and esc_end are set.)
                const PackedArrays pk = packed_arrays_of(ex);
                if (packed_tile) {
                    const int2v *mine = reinterpret_cast<const int2v *>(pk.code8 + s + ((t >> 6) * (64 * VPT) + (t & 63) * VPT));
                    const int2v cw = STREAMED ? __builtin_nontemporal_load(mine) : *mine;
                    code_lo = (unsigned)cw.x, code_hi = (unsigned)cw.y;
                    hot = pk.hot[t & 63];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int at = esc_at + 2 * (t & 63) + 128 * i;
                        ev[i] = double2v{0.0, 0.0};
                        if (at < esc_end) {
                            const double2v *src = reinterpret_cast<const double2v *>(pk.esc_val + at);
                            ev[i] = STREAMED ? __builtin_nontemporal_load(src) : *src;
                        }
                    }
                }
            }
            if constexpr (COL16) {
                int base;
                if constexpr (PACKED)
                    base = pw_base;
                else
                    base = ex.col_base[b];
                if (base >= 0) {
                    if constexpr (VPT == 8) {
                        // the plan keeps the offsets of a narrow 2048-entry tile in the order the lanes hold the entries
                        // (smvp::col16_slot): this lane's 8 offsets are one 16-byte load, and a wave instruction covers 1 KiB once
                        const unsigned short *mine = ex.col16 + s + ((t >> 6) * (64 * VPT) + (t & 63) * VPT + lane_salt);
                        unsigned w[VPT / 2];
                        if constexpr (STREAMED)
                            *reinterpret_cast<int4v *>(w) = __builtin_nontemporal_load(reinterpret_cast<const int4v *>(mine));
                        else
                            *reinterpret_cast<int4v *>(w) = *reinterpret_cast<const int4v *>(mine);
#pragma unroll
                        for (int k = 0; k < VPT; k += 2)
                            c[k] = base + (int)(w[k / 2] & 0xffffu), c[k + 1] = base + (int)(w[k / 2] >> 16);
                    } else {
                        // 1024-entry tiles keep the plain order (one 8-byte load per lane measured 1.5-3 % slower than these two)
#pragma unroll
                        for (int k = 0; k < VPT; k += 2) {  // two 16-bit offsets per 4-byte load
                            const unsigned w = *reinterpret_cast<const unsigned *>(ex.col16 + s + lane_entry(k));
                            c[k] = base + (int)(w & 0xffffu), c[k + 1] = base + (int)(w >> 16);
                        }
                    }
                } else {  // a tile whose columns span 65536 or more
                    load_cols();
                }
            } else {
                load_cols();
            }
            if constexpr (TJDS) {  // (read once: non-temporal)
#pragma unroll
                for (int k = 0; k < VPT; k += 2)
                    *reinterpret_cast<int2v *>(&pj[k]) = __builtin_nontemporal_load(reinterpret_cast<const int2v *>(a.pos + s + lane_entry(k)));
            }
            if constexpr (CSR) {
                if (!PACKED || !packed_tile) {
#pragma unroll
                    for (int k = 0; k < VPT; k += 2) {  // (each instruction covers 1 KiB of val exactly once)
                        if constexpr (STREAMED)
                            *reinterpret_cast<double2v *>(&v[k]) = __builtin_nontemporal_load(reinterpret_cast<const double2v *>(a.val + s + lane_entry(k)));
                        else
                            *reinterpret_cast<double2 *>(&v[k]) = *reinterpret_cast<const double2 *>(a.val + s + lane_entry(k));
                    }
                }
            }
        } else {  // VPT == 1: 256-entry tiles for matrices too small to fill the chip with 1024-entry ones
            c[0] = a.col_ind[j0];
            if constexpr (TJDS)
                pj[0] = a.pos[j0];
            if constexpr (CSR)
                v[0] = a.val[j0];
        }
    }
    int rlo, rhi;
    if constexpr (PACKED) {
        rlo = pw_rlo, rhi = pw_rhi;  // (a tile in which no row starts left right after its plan words)
    } else {
        rlo = tile_row[b];
        rhi = tile_row[b + 1];
        if (rlo == rhi)
            SMVP_OWNER_EXIT();  // all of this tile continues a row owned by an earlier tile
        SMVP_PHASE(0);
    }
    const int lo = (int)s;  // nnz < 2^31
    const int e = (int)(s + TILE < (long long)nnz ? s + TILE : (long long)nnz);
    int zend;  // row_ptr[rhi]: end of the last owned row, >= e
    if constexpr (PACKED)
        zend = pw_zend;
    else
        zend = tile_next[b];
    const int ext = zend - e;
    // bounds of owned row r as offsets from the tile's first entry: from the plan's 16-bit offsets where it keeps them (the
    // last owned row ends at zend), else from row_ptr
    const unsigned short *__restrict__ row_rel = ex.row_rel;
    auto row_bounds = [&](int r, int &ra, int &rz) {
        if (row_rel) {
            ra = row_rel[r];
            rz = r + 1 < rhi ? (int)row_rel[r + 1] : zend - lo;
        } else {
            ra = row_ptr[r] - lo;
            rz = row_ptr[r + 1] - lo;
        }
    };
    const bool giant = ext > kStreamOver;
    if (t == 0)
        long_count = 0;
    const bool over0 = !giant && t < ext;  // this lane fetches overflow entry e + t
    double p[VPT];
    double po = 0.0;
    int rp_a = 0, rp_b = 0, rp_a2 = 0, rp_b2 = 0;  // bounds of this lane's first two rows of phase 2 (rlo + t, rlo + t + 256), from the tile's first entry
    int ovf_base = 0, cache0 = 0, in_place = 0;
    if constexpr (SORTED) {
        ovf_base = ex.ovf_ptr[b];
        cache0 = ex.cache_ptr[b];
        in_place = (e - lo) - (ex.cache_ptr[b + 1] - cache0);  // entries of this tile whose value is read from val itself
    }
    if constexpr (SORTED) {
        if (full_tile && rlo + t < rhi)
            row_bounds(rlo + t, rp_a, rp_b);
        if (full_tile && rlo + t + kStreamBlock < rhi)
            row_bounds(rlo + t + kStreamBlock, rp_a2, rp_b2);
        int co = 0;
        double vo = 0.0;
        const bool unit_x = HALF && ex.unit_x;
        if (over0 && !(SMVP_TJDS_NEUTRALISE & 8)) {
            co = a.ovf_k[ovf_base + t];
            if (!unit_x)
                vo = a.ovf_val[ovf_base + t];
        }
        if (full_tile) {
            int slot[VPT];
#pragma unroll
            for (int k = 0; k < VPT; ++k) {
                if constexpr (HALF)
                    c[k] = (int)((unsigned)pj[k] >> 16), pj[k] &= 0xffff;  // the entry's word: low half of the position | (slot | run hint) << 16
                slot[k] = c[k] & ((1 << kSlotBits) - 1);
                if constexpr (HALF) {
                    const int r = grp[k] + (((c[k] >> kSlotBits) - grp[k]) & 31);
                    int base = __shfl(run_tbl.x, r & 63), sub = __shfl(run_tbl.y, r & 63);
                    if (r >= 64) {
                        const int2 w = reinterpret_cast<const int2 *>(ex.run_tab)[run0 + r];
                        base = w.x, sub = w.y;
                    }
                    pj[k] += base;
                    c[k] = pj[k] - sub;
                } else {
                    c[k] = pj[k] - a.start_pos[(unsigned)c[k] >> kSlotBits];
                }
            }
            double xk[VPT];
            // the tile's last `cached` entries take their value from the tile's own run of the cache (coalesced) instead
            // of val[position]: their val lines are shared with many other tiles (see mark_scattered_lines)
#pragma unroll
            for (int k = 0; k < VPT; ++k) {
                const int idx = k * kStreamBlock + t;
                const double *src = idx < in_place ? a.val + pj[k] : ex.val_cache + (cache0 + (idx - in_place));
                if ((SMVP_TJDS_NEUTRALISE & 2) && idx < in_place)
                    v[k] = 1.0;
                else if ((SMVP_TJDS_NEUTRALISE & 4) && idx >= in_place)
                    v[k] = 1.0;
                else
                    v[k] = *src;
            }
            double xo = 0.0;
            if (unit_x) {  // second phase of the two-phase product: val holds products, the overflow entries' too (by position)
#pragma unroll
                for (int k = 0; k < VPT; ++k)
                    xk[k] = 1.0;
                if (over0)
                    vo = a.val[co], xo = 1.0;
            } else {
#pragma unroll
                for (int k = 0; k < VPT; ++k)
                    xk[k] = (SMVP_TJDS_NEUTRALISE & 1) ? 1.0 : a.x[c[k]];
                xo = over0 && !(SMVP_TJDS_NEUTRALISE & 8) ? a.x[co] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < VPT; ++k)
                prod[slot[k]] = v[k] * xk[k];
            po = vo * xo;
        } else {  // the last, partial tile
            for (int k = 0; k < VPT; ++k) {
                const int idx = k * kStreamBlock + t;
                if (s + idx < (long long)nnz) {
                    if constexpr (HALF) {
                        const unsigned w32 = ex.word32[s + idx];
                        const int m = (int)(w32 >> 16), g = ex.group_run[(size_t)b * (TILE / 32) + (idx >> 5)];
                        const int r = g + (((m >> kSlotBits) - g) & 31);
                        const int2 w = reinterpret_cast<const int2 *>(ex.run_tab)[ex.run_ptr[b] + r];
                        const int pw = w.x + (int)(w32 & 0xffffu);
                        const double vv = idx < in_place ? a.val[pw] : ex.val_cache[cache0 + (idx - in_place)];
                        prod[m & ((1 << kSlotBits) - 1)] = unit_x ? vv : vv * a.x[pw - w.y];
                    } else {
                        const int pw = a.pos[s + idx];
                        const double vv = idx < in_place ? a.val[pw] : ex.val_cache[cache0 + (idx - in_place)];
                        const int m = a.col_ind[s + idx];
                        prod[m & ((1 << kSlotBits) - 1)] = vv * a.x[pw - a.start_pos[(unsigned)m >> kSlotBits]];
                    }
                }
            }
            if (over0)
                po = unit_x ? a.val[co] : vo * a.x[co];
        }
    } else if (fast) {  // Csr16P: phase 1 of this tile is done, above
        if constexpr (PACKED) {
#pragma unroll
            for (int k = 0; k < VPT; ++k)
                p[k] = fast_p[k];
            po = fast_po, rp_a = fast_rp[0], rp_b = fast_rp[1], rp_a2 = fast_rp[2], rp_b2 = fast_rp[3];
        }
    } else if (full_tile) {
        if (rlo + t < rhi)  // this lane's first row in phase 2
            row_bounds(rlo + t, rp_a, rp_b);
        if (rlo + t + kStreamBlock < rhi)  // ... and its second: with short rows a tile holds more rows than lanes, and a row_ptr read
            row_bounds(rlo + t + kStreamBlock, rp_a2, rp_b2);  // behind the barrier is a whole memory round trip in phase 2 (in-kernel
                                                               // stamps on the near part of the random model, 4.3 entries per row:
                                                               // phase 2 took 4.1 of the workgroup's 9.9 us)
        int co = 0, pjo = 0;
        double vo = 0.0;
        if (over0) {
            co = a.col_ind[e + t];
            if constexpr (TJDS)
                pjo = a.pos[e + t];
            if constexpr (CSR)
                vo = a.val[e + t];
        }
        double xk[VPT];
        if constexpr (TJDS) {
#pragma unroll
            for (int k = 0; k < VPT; ++k)
                v[k] = a.val[pj[k]];
            if (over0)
                vo = a.val[pjo];
        }
#pragma unroll
        for (int k = 0; k < VPT; ++k)
            xk[k] = a.x[c[k]];
        const double xo = over0 ? a.x[co] : 0.0;
        if constexpr (PACKED) {
            if (packed_tile)  // (the values of a packable tile: from the codes, under the gathers)
                packed_decode(prod + (t >> 6) * (64 * VPT), ev[0], ev[1], ev[2], ev[3], code_lo, code_hi, hot, t & 63, v);
        }
#pragma unroll
        for (int k = 0; k < VPT; ++k)
            p[k] = v[k] * xk[k];
        po = vo * xo;
    } else {
#pragma unroll
        for (int k = 0; k < VPT; ++k)
            p[k] = (s + lane_entry(k) < (long long)nnz) ? owner_product_slow<FLAVOR>(a, s + lane_entry(k)) : 0.0;
        if (over0)
            po = owner_product_slow<FLAVOR>(a, e + t);
    }
    if constexpr (!SORTED) {  // every product at its row-major place
        if constexpr (VPT >= 2) {
#pragma unroll
            for (int k = 0; k < VPT; k += 2)
                *reinterpret_cast<double2 *>(&prod[lane_entry(k)]) = make_double2(p[k], p[k + 1]);
        } else {
            prod[t] = p[0];
        }
    }
    if (over0)
        prod[e - lo + t] = po;
    if (!giant)  // rare: the last row runs more than one block width past the tile
        for (int i = t + kStreamBlock; i < ext; i += kStreamBlock)
            prod[e - lo + i] = owner_overflow_product<FLAVOR>(a, ovf_base, e, i);
    SMVP_PHASE(1);
    __syncthreads();
    SMVP_PHASE(2);

    // ---- phase 2b: one lane per owned row; its bounds were fetched with the tile (no global read after
    // the barrier for the first kStreamBlock rows); long rows are queued in LDS with their bounds
    // Each lane's first two rows (their bounds came with the tile) are finished without touching memory in between: a
    // row_ptr read in the same loop as the y stores made the compiler wait for vmcnt(0) every round, i.e. for the
    // previous round's STORES to be acknowledged (CDNA4 counts stores in vmcnt) -- 3 of a workgroup's 10 us on short
    // rows (in-kernel stamps).  Only a tile with more than 512 rows goes on to the loop that reads row_ptr.
    const int last = rhi - 1;
    auto finish_row = [&](int r, int ra, int rz) {
        if (rz - ra <= kLongRow) {
            // left to right, like the serial loop; the LDS reads go out four at a time, the adds stay in order
            double acc = 0.0;
            for (int i = ra; i < rz; i += 4) {
                const double v0 = prod[i], v1 = prod[i + 1 < rz ? i + 1 : i], v2 = prod[i + 2 < rz ? i + 2 : i],
                             v3 = prod[i + 3 < rz ? i + 3 : i];
                acc += v0;
                if (i + 1 < rz)
                    acc += v1;
                if (i + 2 < rz)
                    acc += v2;
                if (i + 3 < rz)
                    acc += v3;
            }
            // (256-entry tiles are what matrices that live in the caches get: there a plain store is acknowledged by the L2,
            // sooner than a non-temporal one by memory -- and the product's window ends with that acknowledgement)
            if constexpr (VPT == 1)
                y[r] = acc;
            else
                __builtin_nontemporal_store(acc, &y[r]);
        } else {
            const int q = atomicAdd(&long_count, 1);
            long_rows[q] = r;
            long_a[q] = ra;
            long_z[q] = rz;
        }
    };
    int r_next = rlo + t;
    if (full_tile) {
        if (r_next < rhi && !(giant && r_next == last))
            finish_row(r_next, rp_a, rp_b);
        r_next += kStreamBlock;
        if (r_next < rhi && !(giant && r_next == last))
            finish_row(r_next, rp_a2, rp_b2);
        r_next += kStreamBlock;
    }
    for (int r = r_next; r < rhi; r += kStreamBlock) {
        if (giant && r == last)
            continue;
        int ra, rz;
        row_bounds(r, ra, rz);
        finish_row(r, ra, rz);
    }
    SMVP_PHASE(3);
    __syncthreads();
    SMVP_PHASE(4);

    // ---- phase 2c: one wavefront per long row (measured: handing a long row to the finder's own wavefront
    // by ballot, without this queue and barrier, was 0-2 % slower -- the long rows of a tile then share one wave)
    const int nlong = long_count;
    const int lane = t & 63;
    for (int q = t >> 6; q < nlong; q += kStreamBlock / 64) {
        const int zq = long_z[q];
        double acc = 0.0;
        for (int i = long_a[q] + lane; i < zq; i += 64)
            acc += prod[i];
        acc = wave_sum_dpp(acc);
        if (lane == 0)
            y[long_rows[q]] = acc;
    }
    SMVP_PHASE(5);

    // ---- phase 2d: a last row that runs far past the tile: LDS part + the rest from global memory
    if (giant) {
        const int ra = row_ptr[last];
        double acc = 0.0;
        for (int i = ra - lo + t; i < e - lo; i += kStreamBlock)
            acc += prod[i];
        for (int j = e + t; j < zend; j += 4 * kStreamBlock) {
            double pg[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int jj = j + u * kStreamBlock;
                pg[u] = jj < zend ? owner_overflow_product<FLAVOR>(a, ovf_base, e, jj - e) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                acc += pg[u];
        }
        acc = shfl_down_sum<64>(acc);
        if (lane == 0)
            wave_sum[t >> 6] = acc;
        __syncthreads();
        if (t == 0) {
            double total = 0.0;
#pragma unroll
            for (int w = 0; w < kStreamBlock / 64; ++w)
                total += wave_sum[w];
            y[last] = total;
        }
    }
    SMVP_OWNER_EXIT();
#undef SMVP_OWNER_EXIT
}

template <int VPT, int FLAVOR, bool STAMPED>
__global__ __launch_bounds__(kStreamBlock) void csr_stream_owner(
    const int *__restrict__ row_ptr, const int *__restrict__ col_ind, const double *__restrict__ val,
    const double *__restrict__ x, double *__restrict__ y, const int *__restrict__ tile_row,
    const int *__restrict__ tile_next, int rows, int nnz_arg, int ntiles, int tile_group_arg, const OwnerExtra ex)
{
    owner_body<VPT, FLAVOR, STAMPED>(row_ptr, col_ind, val, x, y, tile_row, tile_next, rows, nnz_arg, ntiles, tile_group_arg, ex,
                                     (int)blockIdx.x);
}

// The same kernel with the read-once hint on its value and offset streams (owner_body's STREAMED), for the plain CSR launches
// of a plan that asks for it (OwnerLaunch::read_once: a product larger than the caches, see the engine's kReadOnceMinBytes).
// A second kernel and not a uniform word of the launch: with the hint behind a uniform branch, the compiler first merged the
// two loads into one without it, and once they were kept apart (other vector types) the hinted path ran 15 % SLOWER than
// without the hint (memplus x944 0.2930 ms against 0.2552) where this form runs 3 % faster
// (profiles/col16_lane_order_measured.txt).  In a namespace of its own so that its name in a profile is still
// csr_stream_owner<VPT, FLAVOR, STAMPED>, which is what describe() says and the tools look for.
namespace read_once {
template <int VPT, int FLAVOR, bool STAMPED>
__global__ __launch_bounds__(kStreamBlock) void csr_stream_owner(
    const int *__restrict__ row_ptr, const int *__restrict__ col_ind, const double *__restrict__ val,
    const double *__restrict__ x, double *__restrict__ y, const int *__restrict__ tile_row,
    const int *__restrict__ tile_next, int rows, int nnz_arg, int ntiles, int tile_group_arg, const OwnerExtra ex)
{
    owner_body<VPT, FLAVOR, STAMPED, true>(row_ptr, col_ind, val, x, y, tile_row, tile_next, rows, nnz_arg, ntiles, tile_group_arg, ex,
                                           (int)blockIdx.x);
}
}  // namespace read_once

// The forms the library instantiates, X(entries per thread, flavour), each written once: the launch ladders of both units and
// the repeating forms expand from these lists, so a form added here exists everywhere it should and nowhere else.
// CSR flavours: the 1024- and 2048-entry tiles also have the read-once twin, the 256-entry tile has not.
#define SMVP_OWNER_CSR_WIDE_FORMS(X) X(4, kFlavorCsr) X(8, kFlavorCsr) X(4, kFlavorCsr16) X(8, kFlavorCsr16)
#define SMVP_OWNER_CSR_FORMS(X) X(1, kFlavorCsr) SMVP_OWNER_CSR_WIDE_FORMS(X)
// Csr16P: 2048-entry tiles only; plain and read-once single launches (and their stamped twins), no repeating form -- the timed
// entry points run a packed plan as stamped single launches (owner_repeat_grid answers 0, the repeating launcher refuses it).
#define SMVP_OWNER_CSR_PACKED_FORMS(X) X(8, kFlavorCsr16P)
// TJDS flavours: the tile-ordered ones (TjdsS, TjdsH) also have a repeating form, the row-ordered one (TjdsK) has not.
#define SMVP_OWNER_TJDS_TILE_FORMS(X) \
    X(1, kFlavorTjdsS) X(4, kFlavorTjdsS) X(8, kFlavorTjdsS) X(1, kFlavorTjdsH) X(4, kFlavorTjdsH) X(8, kFlavorTjdsH)
#define SMVP_OWNER_TJDS_FORMS(X) X(1, kFlavorTjdsK) X(4, kFlavorTjdsK) X(8, kFlavorTjdsK) SMVP_OWNER_TJDS_TILE_FORMS(X)
// csr_stream_owner_repeat (smvp_owner.hip)
#define SMVP_OWNER_REPEAT_FORMS(X) SMVP_OWNER_CSR_FORMS(X) SMVP_OWNER_TJDS_TILE_FORMS(X)

// The plain launches of the CSR flavours (smvp_owner_csr.hip: max-ILP scheduling suits them -- memplus x944 0.2866 -> 0.2800 ms --
// and costs the TJDS flavours 2-3 %).  launch_csr_stream_owner in smvp_owner.hip prepares `ex`, grid and group.
hipError_t launch_owner_csr(int vpt, int flavor, const OwnerLaunch &l, const OwnerExtra &ex, unsigned grid_x, int group, hipStream_t stream);

}  // namespace smvp
