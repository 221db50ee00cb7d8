// smvp_engine.hip -- the CSR handle: a device-resident CSR matrix and its launch plans.
//
// This file owns what the reference keeps in CSRData (main-cli.c:61-66) once it is in HBM, and the per-matrix launch plans;
// the TJDS handle (TJDSData, :70-75) lives in smvp_tjds.hip and nests handles of this file.  The conversion halves live in
// smvp_convert.cpp (host); the timed iteration loop and the two reference-shaped compute entry points live in smvp_run.hip.
// Both see this handle through smvp_engine.h only.
#include "smvp_engine.h"

#include <cmath>
#include <cstring>

using smvp::check_block_operands;
using smvp::check_device_indices;
using smvp::DeviceScope;
using smvp::kMaxEntries;
using smvp::refuse_capture;
using smvp::TjdsSource;
using smvp::to_device;
using smvp::upload;
using smvp::usable_device;
using smvp::wall_ms;

int smvp::usable_device(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return smvp::fail(SMVP_ERR_NO_DEVICE, "no HIP device is visible (this engine has no CPU path)");
    if (device < 0 || device >= n)
        return smvp::fail(SMVP_ERR_INVALID, "device %d out of range (%d visible)", device, n);
    return SMVP_OK;
}

// ===========================================================================
// CSR
// ===========================================================================
// The launch plans of a CSR handle.  Each is a plain struct with one release function that frees what the struct owns and
// resets it to its default value (the idiom of smvp::BinnedPlan / free_binned_plan); what a caller asked for and must survive
// a re-plan -- the tile size, the value cache's threshold -- stays on the handle.

// STREAM / STREAM_CARRY: tiles of 256 * smvp_csr::vpt entries, and the tile-ordered streams of the TJDS flavours; build_tile_plan
struct TilePlan {
    int ntiles = 0;
    int *d_tile_row = nullptr;
    int *d_tile_next = nullptr;   // STREAM: row_ptr[first row of the next tile]
    // STREAM, plain CSR, tiles of 1024 / 2048 entries whose columns all span < 65536: col_ind a second time as 16-bit
    // offsets from the tile's smallest column (10 instead of 12 bytes per entry; csr_stream_owner<., kFlavorCsr16, .>)
    // (at 2048-entry tiles a full narrow tile's offsets lie in the order the kernel's lanes hold its entries, smvp::col16_slot:
    // the array serves the tile size it was laid out for, col16_tile, and no other)
    unsigned short *d_col16 = nullptr;
    int *d_col_base = nullptr;
    int col16_tile = 0;
    // STREAM: every row's first entry as a 16-bit offset from the first entry of the tile the row
    // starts in -- what phase 2 reads instead of row_ptr (2 instead of 4 bytes per row)
    unsigned short *d_row_rel = nullptr;
    int *d_carry_row = nullptr;   // STREAM_CARRY
    double *d_carry = nullptr;    // STREAM_CARRY
    // TjdsS: per-tile TJDS-ordered streams and the tiles' overflow entries
    int *d_pos_sorted = nullptr, *d_meta = nullptr, *d_ovf_ptr = nullptr, *d_ovf_k = nullptr;
    double *d_ovf_val = nullptr;  // TjdsS / H: the overflow entries' values (read coalesced by the tile that finishes the row)
    // TjdsS: values of the entries whose val lines scatter over cache_min_tiles tiles or more, kept tile by tile (0: none).
    // A line split over two or three tiles is the edge between neighbouring tiles (they run together on one XCD: an L2
    // hit); from four on its entries belong to unrelated rows.  Measured on memplus x944 (profiles/r03_tjds_forms_measured.txt):
    // none 0.555 ms / 3.66 GB moved, >= 8 tiles 0.461 / 2.92 (20 % of the values cached), >= 4 tiles 0.444 / 2.73 (35 %).
    int *d_cache_ptr = nullptr;
    double *d_val_cache = nullptr;
    int cached_total = 0, ovf_total = 0;
    // TjdsH: the 16-bit second word of every entry, the tiles' runs (start_pos of each run's diagonal), each group of 32's run
    unsigned short *d_group_run = nullptr;
    unsigned *d_word32 = nullptr;
    int *d_run_ptr = nullptr, *d_run_tab = nullptr;
    int runs_total = 0;
    // STREAM: the direction of the next plain launch's sweep over the tiles.  It flips with every such launch (a handle is
    // used by one stream at a time), so a product starts where the one before it ended -- on what the Infinity Cache still
    // holds; sweep_alternate = 0 (a matrix the caches hold, or plan option "csr_sweep_alternate" 0; decided when the plan is
    // built): always forward
    int sweep_alternate = 1, sweep_backward = 0;
    // STREAM, plain CSR: the single launches read val and the 16-bit offsets of full tiles with the read-once hint (decided when
    // the plan is built: kReadOnceMinBytes or plan option "csr_read_once")
    int read_once = 0;
    // STREAM_PACKED (csr_stream_owner<8, kFlavorCsr16P, .>): the values of the packable tiles -- full, with 16-bit offsets -- a second
    // time: a code per entry in smvp::col16_slot order, the table of the 64 most frequent bit patterns the codes index, the
    // start of every wavefront's run of escapes (4 * ntiles + 1) and the escapes themselves; smvp::build_packed_values.
    // packed_doubles: entries a product still reads as 8-byte values (escapes, and the entries of tiles that are not packable).
    unsigned char *d_code8 = nullptr;
    double *d_hot = nullptr, *d_esc_val = nullptr;
    int *d_esc_ptr = nullptr;
    long long packed_doubles = 0, esc_slots = 0;
    int packed_bounded = 0;  // (set by AUTO for the build it asks for: stop at the count where the share is over its bound)
};

// COLSWEEP: the entries a second time, every strip sorted by column (built on the device); build_sweep_plan
struct SweepPlan {
    int rb = 0, per_launch = 0;  // rows per workgroup (four wavefronts), workgroups that start together
    int parts = 1;               // column parts per strip (1: every row summed in the serial loop's order; 2 / 4 / 8: see sweep_param)
    int g = 0;                   // chunks in flight per wavefront (fixed when the plan is built)
    long long *d_ptr = nullptr;
    int *d_col = nullptr;
    double *d_val = nullptr;
    unsigned short *d_row = nullptr;
    double *d_part = nullptr;    // XCD-private column parts: 8 * rows partial sums
};

// BINNED: the entries a second time, split by |column - row| > band: the near part as the window plan bin.nw (K6) or,
// where that does not suit, as CSR arrays of its own run by the tile kernel through the nested handle `near`; the far
// part as the two streams and the bins of smvp_binned.hip; build_binned
struct BinnedSide {
    smvp::BinnedPlan bin;
    smvp_csr *near = nullptr;
    // with the window plan: pass A (it needs x only) goes onto a stream of its own, ahead of the near part, and
    // the near part's workgroups take the CUs as pass A's last ones leave them
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
};

// smvp_csr_spmm (K7, smvp_spmm.hip): the rows ordered by length inside blocks of kSpmmBlockRows, built by the first call
// and kept whatever the SpMV plan is (it depends on row_ptr only)
struct SpmmPlan {
    int *d_order = nullptr;
    bool planned = false;
    double build_ms = 0.0;
};

struct smvp_csr {
    int device = 0;
    int rows = 0, cols = 0, nnz = 0;
    long long row0 = 0;  // global number of this handle's first row (a row block of a sharded matrix; 0 for a whole matrix):
                         // where the diagonal lies -- the binned plan's near / far split and its windows of x go by it
    int *d_row_ptr = nullptr;
    int *d_col_ind = nullptr;
    double *d_val = nullptr;
    bool own_row_ptr = false, own_col_ind = false, own_val = false;
    std::vector<int> h_row_ptr;  // kept for re-planning
    int max_row_len = 0;

    // what an entry of the stream is (smvp_kernels.h kFlavor*): plain CSR, or a TJDS matrix regrouped by rows (the one-kernel
    // TJDS product; as kFlavorTjdsH with unit_operand the second phase of the two-phase product); the TJDS flavours
    // borrow these arrays from their smvp_tjds owner
    int flavor = smvp::kFlavorCsr;
    TjdsSource src;  // src.pos: what the TjdsK kernel reads; TjdsS / H: the row-major stream the tiles are sorted from
    int cache_min_tiles = 2;    // TjdsS / H, see TilePlan::d_val_cache; 2: every val line that is not one tile's alone (measured, r04)
    bool plain_only = false;    // a nested handle: AUTO stays on the tile kernels

    int kernel = SMVP_CSR_KERNEL_AUTO;  // resolved: never AUTO once a plan exists
    int lanes_per_row = 64;             // VECTOR
    int vpt = 4;                        // STREAM: entries per thread (tile = 256 * vpt)
    bool tile_chosen = false;           // the caller named the tile size (smvp_csr_set_kernel param): the plan keeps it
    double spread = -2.0;     // share of gathers that pull their own line of x (csr_gather_spread); -2: not measured yet
    double far_share = -2.0;  // share of entries with |column - row| > kBinNearBand; -2: not measured yet
    double plan_build_ms = 0.0;  // host wall time of the last plan build

    TilePlan tile;
    SweepPlan sweep;
    BinnedSide binned;
    SpmmPlan spmm;
};

namespace {

void free_tile_plan(TilePlan *p)
{
    for (void *q : {(void *)p->d_tile_row, (void *)p->d_tile_next, (void *)p->d_col16, (void *)p->d_col_base, (void *)p->d_row_rel,
                    (void *)p->d_carry_row, (void *)p->d_carry, (void *)p->d_pos_sorted, (void *)p->d_meta, (void *)p->d_ovf_ptr,
                    (void *)p->d_ovf_k, (void *)p->d_ovf_val, (void *)p->d_cache_ptr, (void *)p->d_val_cache, (void *)p->d_group_run,
                    (void *)p->d_word32, (void *)p->d_run_ptr, (void *)p->d_run_tab, (void *)p->d_code8, (void *)p->d_hot, (void *)p->d_esc_ptr,
                    (void *)p->d_esc_val})
        if (q)
            (void)hipFree(q);
    *p = TilePlan{};
}

void free_sweep_plan(SweepPlan *p)
{
    for (void *q : {(void *)p->d_ptr, (void *)p->d_col, (void *)p->d_val, (void *)p->d_row, (void *)p->d_part})
        if (q)
            (void)hipFree(q);
    *p = SweepPlan{};
}

void free_binned_side(BinnedSide *p)
{
    smvp_csr_destroy(p->near);
    smvp::free_binned_plan(&p->bin);
    if (p->side)
        (void)hipStreamDestroy(p->side);
    for (hipEvent_t e : {p->ev_fork, p->ev_join})
        if (e)
            (void)hipEventDestroy(e);
    *p = BinnedSide{};
}

void free_spmm_plan(SpmmPlan *p)
{
    if (p->d_order)
        (void)hipFree(p->d_order);
    *p = SpmmPlan{};
}

// the derived quantities the plans are read through
inline bool tile_ordered(int flavor) { return flavor == smvp::kFlavorTjdsS || flavor == smvp::kFlavorTjdsH; }
inline bool stream_family(int k) { return k == SMVP_CSR_KERNEL_STREAM || k == SMVP_CSR_KERNEL_STREAM_PACKED; }  // the owner (tile) kernel
inline bool runs_on_tile_plan(int k) { return k != SMVP_CSR_KERNEL_VECTOR && k != SMVP_CSR_KERNEL_COLSWEEP && k != SMVP_CSR_KERNEL_BINNED; }
// what the owner kernel is launched with: `flavor`, but for plain CSR with 16-bit column offsets (try_column_offsets builds them
// for plain CSR only, so for a TJDS flavour this is `flavor`)
// (and with packed values, which build_tile_plan_parts builds for STREAM_PACKED only and only on top of the offsets)
inline int owner_flavor(const smvp_csr *h) { return h->tile.d_code8 ? smvp::kFlavorCsr16P : h->tile.d_col16 ? smvp::kFlavorCsr16 : h->flavor; }
inline double csr_matrix_bytes(const smvp_csr *h) { return 12.0 * h->nnz + 4.0 * (h->rows + 1.0); }
// rows of one strip of the column sweep: a workgroup's kSweepWaves wavefronts share rb rows, or rb * parts where every strip is cut
// into column parts (one wavefront each); XCD-private parts run on whole strips
inline int sweep_strip_rows(const SweepPlan &s) { return (s.parts == smvp::kSweepXcdParts ? s.rb : s.rb * s.parts) / smvp::kSweepWaves; }

// Rows per workgroup of the column sweep (four strips) and how many workgroups start together.  A block of rb rows streams
// rb * (mean row length) entries in column order, 1024 per pass of its workgroup (256 per strip), so its window moves
// 1024 * cols / (rb * mean) columns of x per pass: the taller the block, the slower the window and the better the
// XCD's L2 holds what the resident workgroups gather.  The workgroups start in even generations of at most 256, one per
// CU -- those that start late drift out of the others' window (2.5 M rows, 305 workgroups: 2 x 153 0.883 ms, all at once
// 0.926; 5 M rows: 3 x 204 1.331 against 1.540) -- so a height also decides how full the chip is: 1.25 M rows as 153
// workgroups of 8192 rows keep 60 % of the CUs busy (0.439 ms), as 3 x 204 of 2048 rows 80 % (0.411 ms).  Measured at equal
// fill, 8192 rows run at 1.0, 4096 at 0.86, 2048 at 0.80 of the rate (config 4: 2.25 / 2.62 ms); the height is the one with
// the best fill x rate, never so short that a pass moves the window by more than ~1.3 MB (tools/exp_colsweep.py,
// profiles/r03_colsweep_measured.txt).
// Round 5: the height need not be a power of two.  With generations of at most 256 workgroups the heights 8192 / 4096 / 2048
// leave a rank's block of BASELINE config 4 (1.25 M rows) either 40 % of the CUs idle (153 workgroups of 8192 rows) or three
// generations -- and every generation makes each of the eight L2s pull all of x again (8 x 80 MB: 1.9 GB for 0.56 GB of the
// block's own entries).  Candidates are now also the heights that cut the rows into EXACTLY g x 256
// workgroups, g = 1, 2, ...: 1.25 M rows as 256 workgroups of 4884 rows are one full generation.  The rate of a height in
// between is read off the measured ones on a log scale.
// Round 6: strips as tall as the LDS allows.  Every generation of workgroups makes all eight L2s pull all of x again, and a
// generation covers 256 x (rows per workgroup) rows: taller strips = fewer generations (config 4: two instead of five).  A taller
// strip's column-sorted stream is also denser (1954-row strips: a mean gap of 160 columns, 4883-row strips: 64), so adjacent lanes
// of one gather instruction share a line of x -- one L2 request -- more often: worth a few per cent by itself (the column-parts
// experiment, profiles/r06_colsweep_column_parts.txt).  The 16-bit row word spends 13 bits on the row (turns capped at 7), the
// four strips of a workgroup may fill the CU's LDS (kSweepMaxRb rows = 160 KB of sums), and config 4 whole runs
// 1.98 -> 1.73-1.86 ms as 2 generations of 256 x 19532 rows.
constexpr int kSweepMaxRb = 20480;
double sweep_rate(int rb)
{
    // (20480 rows: round 6 -- strips of up to 5120 rows, the four of a workgroup fill the CU's 160 KB of LDS; config 4 whole:
    // 7816 rows 161.7 G gathers/s, 9768 166.1, 13024 171.2, 19536 177.7 -- profiles/r06_colsweep_tall_strips.txt)
    const struct { double lg, rate; } pts[] = {{10.0, 0.70}, {11.0, 0.80}, {12.0, 0.86}, {13.0, 1.0}, {14.32, 1.10}};
    constexpr int N = (int)(sizeof pts / sizeof pts[0]);
    const double lg = std::log2((double)std::max(rb, 1));
    if (lg <= pts[0].lg)
        return pts[0].rate * std::max(0.25, lg / pts[0].lg);
    for (int i = 0; i + 1 < N; ++i)
        if (lg <= pts[i + 1].lg)
            return pts[i].rate + (pts[i + 1].rate - pts[i].rate) * (lg - pts[i].lg) / (pts[i + 1].lg - pts[i].lg);
    return pts[N - 1].rate;
}

void choose_sweep_shape(int rows, int cols, int nnz, int want_rb, int *rb, int *per_launch)
{
    const double mean = rows > 0 ? std::max(1.0, (double)nnz / rows) : 1.0;
    int floor_rb = 1024;
    while (floor_rb < 8192 && (double)floor_rb * mean * 160.0 < (double)cols)
        floor_rb <<= 1;
    auto generations = [](int nrb) { return (nrb + 255) / 256; };
    std::vector<int> heights;
    for (int hgt : {kSweepMaxRb, 16384, 8192, 4096, 2048, 1024})
        if (hgt >= floor_rb)
            heights.push_back(hgt);
    // ... and the heights of whole generations; those may be half as tall as the floor (a full chip outweighs the faster window:
    // a 312 K-row chunk of config 4 as 256 x 1224 rows 0.0975 ms, as 153 x 2048 rows 0.134; profiles/r05_colsweep_heights.txt)
    for (int g = 1; g <= 16 && rows > 0; ++g) {
        const long long want = ((long long)rows + 256ll * g - 1) / (256ll * g);  // rows per workgroup for g full generations
        const int h4 = (int)std::min<long long>(kSweepMaxRb, (want + 3) / 4 * 4);  // four strips per workgroup
        if (h4 >= std::max(1024, floor_rb / 2))
            heights.push_back(h4);
    }
    int r = floor_rb;
    double best = -1.0;
    int best_gen = 1 << 30;
    for (int hgt : heights) {
        const int nrb = (rows + hgt - 1) / hgt;
        const int gen = std::max(1, generations(nrb));
        const double score = (double)nrb / (gen * 256.0) * sweep_rate(hgt);
        // (a tie within 1 % goes to fewer generations: each costs 8 x the operand in L2 fills)
        if (score > best * 1.01 || (score > best * 0.99 && gen < best_gen)) {
            best = std::max(best, score);
            best_gen = gen;
            r = hgt;
        }
    }
    if (want_rb > 0)
        r = want_rb;
    const int nrb = (rows + r - 1) / r;
    const int gen = std::max(1, generations(nrb));  // no rows: one (empty) generation
    *rb = r;
    *per_launch = std::max(1, (nrb + gen - 1) / gen);
}

// The column sweep's kernel parameter: rows per workgroup (a multiple of 4, 0 = chosen) in the low 24 bits and, above them, log2 of
// the COLUMN PARTS per strip (round 6).  With parts = 1 a workgroup's four wavefronts own four strips; with parts = 2 / 4 they own
// two strips / one strip whose stream is cut into column halves / quarters, one wavefront and one array of partial sums each:
// the strip is 2x / 4x as tall for the same rows per workgroup -- a block of rows too short to fill the LDS with four strips
// (one rank's eighth of config 4: 256 workgroups x 4884 rows = four strips of 1221) gets the denser streams of a tall strip
// (one strip of 4884) -- and a row's sum is its partial sums added part by part: reproducible, inside the rounding bound, no
// longer the serial loop's bits.  Never chosen by AUTO (which keeps the serial order); SMVP_CSR_SWEEP_PARTS(rb, parts) asks for it.
// Above the parts (bits 26-27): chunks in flight per wavefront for experiments -- 0 = the rule (sweep_chunks_in_flight), 1 / 2 / 3 = one /
// two / four (what the environment switch SMVP_SWEEP_G used to say; tools/exp_colsweep.py --g).
constexpr int kSweepPartsShift = 24, kSweepChunksShift = 26;
inline int sweep_param_rb(int param) { return param & ((1 << kSweepPartsShift) - 1); }
inline int sweep_param_parts(int param) { return 1 << ((param >> kSweepPartsShift) & 3); }  // (8 = one part per XCD, below)
inline int sweep_param_chunks(int param) { const int c = (param >> kSweepChunksShift) & 3; return c == 3 ? 4 : c; }
bool sweep_param_ok(int param)
{
    const int rb = sweep_param_rb(param), parts = sweep_param_parts(param);
    if (param < 0 || (param >> (kSweepChunksShift + 2)) != 0)
        return false;
    if (rb == 0)
        return true;  // (height chosen; the parts are honoured where the chosen height leaves room for them)
    if (parts == smvp::kSweepXcdParts)  // XCD-private parts: the workgroup's four strips are whole strips of rb / 4 rows
        return rb >= 256 && rb % 4 == 0 && rb <= kSweepMaxRb;
    return rb >= 256 && rb % 4 == 0 && (long long)rb * parts <= kSweepMaxRb;
}

int build_sweep_plan(smvp_csr *h, int want)
{
    SweepPlan &s = h->sweep;
    free_sweep_plan(&s);
    const int want_rb = sweep_param_rb(want);
    s.parts = sweep_param_parts(want);
    const bool xcd = s.parts == smvp::kSweepXcdParts;
    if (xcd) {
        // XCD-private column parts (SMVP_CSR_SWEEP_PARTS(rb, 8)): a generation of 256 workgroups = 32 row groups x 8 parts; the height is the
        // caller's, or the one that cuts the rows into whole generations with the tallest strips the LDS takes
        int rb = want_rb;
        if (rb == 0) {
            const long long per_gen_max = 32ll * kSweepMaxRb;
            const long long gens = std::max<long long>(1, ((long long)h->rows + per_gen_max - 1) / per_gen_max);
            rb = (int)std::min<long long>(kSweepMaxRb, std::max<long long>(256, (((long long)h->rows + 32 * gens - 1) / (32 * gens) + 3) / 4 * 4));
        }
        s.rb = rb;
        s.per_launch = 256;
    } else {
        choose_sweep_shape(h->rows, h->cols, h->nnz, want_rb, &s.rb, &s.per_launch);
        while (s.parts > 1 && (long long)s.rb * s.parts > kSweepMaxRb)
            s.parts >>= 1;  // (a chosen height may leave room for fewer parts than asked)
    }
    const int strip_rows = sweep_strip_rows(s);
    s.g = smvp::sweep_chunks_in_flight(strip_rows, sweep_param_chunks(want));
    if (const hipError_t pe = smvp::prepare_csr_colsweep(); pe != hipSuccess)
        return smvp::fail(SMVP_ERR_HIP, "the column sweep cannot have its LDS: %s", hipGetErrorString(pe));
    const int nstrips = (h->rows + strip_rows - 1) / strip_rows;
    const size_t n = (size_t)std::max(h->nnz, 4);
    if (hipMalloc((void **)&s.d_ptr, ((size_t)nstrips * s.parts + 2) * sizeof(long long)) != hipSuccess ||
        hipMalloc((void **)&s.d_col, n * sizeof(int)) != hipSuccess ||
        hipMalloc((void **)&s.d_val, n * sizeof(double)) != hipSuccess ||
        hipMalloc((void **)&s.d_row, n * sizeof(unsigned short)) != hipSuccess ||
        (xcd && hipMalloc((void **)&s.d_part, sizeof(double) * smvp::kSweepXcdParts * (size_t)std::max(h->rows, 1)) != hipSuccess))
        return smvp::fail(SMVP_ERR_ALLOC, "cannot allocate the column-sweep plan (%d entries)", h->nnz);
    return smvp::build_colsweep_plan(h->d_row_ptr, h->d_col_ind, h->d_val, h->rows, h->cols, h->nnz, strip_rows, s.parts, smvp::kSweepChunk,
                                     smvp::kSweepRowBits, smvp::kSweepTurnCap, s.d_ptr, s.d_col, s.d_val, s.d_row, nullptr);
}

// Share of the gathers of a (large) CSR matrix that pull their own 128-byte line of x through the L2, estimated on
// kSpreadSamples runs of 64 K consecutive entries -- one XCD's turn of the tile kernel -- by linear counting
// (smvp_kernels.hip: csr_line_spread; the column sweep itself is smvp_colsweep.hip): distinct lines / entries, 0 ... 1.  -1: too small to sample, or the probe failed.
constexpr int kSpreadSamples = 64;
double csr_gather_spread(const smvp_csr *h)
{
    if ((long long)h->nnz < (long long)kSpreadSamples * smvp::kSpreadSpan || !h->d_col_ind)
        return -1.0;
    int *d_bits = nullptr;
    if (hipMalloc((void **)&d_bits, sizeof(int) * kSpreadSamples) != hipSuccess)
        return -1.0;
    int bits[kSpreadSamples];
    hipError_t e = smvp::launch_csr_line_spread(h->d_col_ind, h->nnz, kSpreadSamples, d_bits, nullptr);
    if (e == hipSuccess)
        e = hipMemcpy(bits, d_bits, sizeof bits, hipMemcpyDeviceToHost);
    (void)hipFree(d_bits);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return -1.0;
    }
    const double m = 512.0 * 1024.0;  // bits in the map
    double lines = 0.0;
    for (int b : bits)
        lines += -m * std::log(std::max(1.0 - b / m, 1.0 / m));  // linear counting: n = -m ln(share of clear bits)
    return std::min(1.0, lines / ((double)kSpreadSamples * smvp::kSpreadSpan));
}

// AUTO picks the column sweep when the tile kernel would be bound by L2-miss gathers and the sweep's window can hold:
//  * the operand is at least twice an XCD's 4 MB L2 (else the tile kernel's gathers hit anyway; measured on uniform
//    rows of 32: 8 MB operand 0.340 -> 0.205 ms, 16 MB 0.907 -> 0.403, 32 MB 2.20 -> 0.81, 80 MB 6.2 -> 2.45), rows
//    of at least 4 entries on average;
//  * most gathers pull their own line: spread >= kSweepMinSpread.  Tile kernel: spread * nnz / 54 G lines/s (measured:
//    config 4, spread 0.95, 5.98 ms; the SURVEY 8(d) random model, 0.42, 1.03 ms); sweep: nnz / 133 G/s;
//  * a workgroup's 8192 rows hold enough entries that a pass moves its window by about 1 MB at most
//    (choose_sweep_shape) -- the random model's 7 entries per row over 16.7 M columns do not, and the sweep loses there
//    (profiles/r02_colsweep_measured.txt);
//  * no row is so long that its strip becomes the critical path; the matrix is worth a second copy (>= 4 M entries).
constexpr double kSweepMinSpread = 0.6;

// the two figures AUTO's choice rests on, measured when first asked for and kept until a re-plan forgets them (-1: not available)
double measured_spread(smvp_csr *h)
{
    if (h->spread < -1.5)
        h->spread = h->flavor == smvp::kFlavorCsr ? csr_gather_spread(h) : -1.0;
    return h->spread;
}

double measured_far_share(smvp_csr *h)
{
    if (h->far_share < -1.5) {
        double share = -1.0;
        if (h->flavor != smvp::kFlavorCsr ||
            smvp::csr_far_share(h->d_row_ptr, h->d_col_ind, h->rows, h->nnz, smvp::kBinNearBand, h->row0, &share, nullptr) != SMVP_OK) {
            (void)hipGetLastError();
            share = -1.0;
        }
        h->far_share = share;
    }
    return h->far_share;
}

bool sweep_suits(smvp_csr *h)
{
    if (h->plain_only || h->flavor != smvp::kFlavorCsr || h->nnz < 4 * 1024 * 1024 || h->rows < 4096)
        return false;
    const double mean = (double)h->nnz / h->rows;
    if (mean < 4.0 || (double)h->cols * 8.0 < 8.0 * 1024 * 1024 || 8192.0 * mean * 160.0 < (double)h->cols ||
        (double)h->max_row_len > 256.0 * mean)
        return false;
    return measured_spread(h) >= kSweepMinSpread;
}

// AUTO picks the binned plan (near part on the tile kernel, far part in two LDS-binned passes: smvp_binned.hip) where the
// tile kernel is held back by gathers that miss the L2 and the column sweep does not fit:
//  * a large matrix (>= 4 M entries) over an operand of at least 16 MB;
//  * a good share of the gathers pull their own line of x: spread >= kBinnedMinSpread (the SURVEY 8(d) random model: 0.40,
//    tile kernel 1.03 ms; kron(I, memplus), pwt x459, a narrow band: < 0.1, which stay on the tile kernel);
//  * and those gathers are what the split removes: at least kBinnedMinFarShare of the entries lie further than
//    kBinNearBand from the diagonal (the model: 0.39).  A matrix whose scattered gathers are close to the diagonal
//    gains nothing from the split.
// The column sweep is asked first (spread >= 0.6 and rows long enough for its window: BASELINE config 4).
constexpr double kBinnedMinSpread = 0.2, kBinnedMinFarShare = 0.1;
bool binned_suits(smvp_csr *h)
{
    if (h->plain_only || h->flavor != smvp::kFlavorCsr || h->nnz < 4 * 1024 * 1024 || h->rows < 4096 ||
        (double)h->cols * 8.0 < 16.0 * 1024 * 1024)
        return false;
    return measured_spread(h) >= kBinnedMinSpread && measured_far_share(h) >= kBinnedMinFarShare;
}

// tile_row[b]  = first row whose first entry lies at or after b*TILE
// carry_row[b] = row that the entries in front of that row belong to, or -1
// 16-bit column offsets for the plain CSR tile kernel where every tile's columns are close together (banded and
// block-structured matrices): 10 instead of 12 bytes per entry.  Tried for 2048-entry tiles first on large matrices --
// with the narrower stream the larger tile wins (memplus x944: 0.2965 ms against 0.3131 with 1024-entry tiles; 32-bit
// columns: 0.319 / 0.325) -- unless the caller named the tile size.  Leaves h->vpt at the tile size that fits, or the
// handle without offsets.  An error where the two arrays cannot be allocated or their build fails.
int try_column_offsets(smvp_csr *h)
{
    if (h->flavor != smvp::kFlavorCsr || !stream_family(h->kernel) || h->vpt < 4 || h->nnz <= 0 ||
        smvp::option("csr_col16", 1) == 0)  // (plan option: 0 keeps the 32-bit columns)
        return SMVP_OK;
    std::vector<int> tiles;
    if (!h->tile_chosen && h->nnz >= 12 * 1024 * 1024)  // memplus x59 / x118 / x236 (7.4 / 14.9 / 29.8 M entries), 1024- against
        tiles.push_back(2048);                           // 2048-entry tiles: 0.0220 / 0.0364 / 0.0851 against 0.0219 / 0.0345 / 0.0787 ms
    tiles.push_back(smvp::kStreamBlock * h->vpt);
    const size_t max_tiles = ((size_t)h->nnz + 1023) / 1024 + 1;
    int *col_base = nullptr;
    unsigned short *col16 = nullptr;
    // memory that runs out and a build that fails are the plan's failure, as with every other array of it; columns that do not fit
    // only leave the handle without the second copy
    int rc = SMVP_OK;
    if (hipMalloc((void **)&col_base, max_tiles * sizeof(int)) != hipSuccess ||
        hipMalloc((void **)&col16, ((size_t)h->nnz + 8) * sizeof(unsigned short)) != hipSuccess)
        rc = smvp::fail(SMVP_ERR_ALLOC, "cannot allocate the 16-bit column offsets (%d entries)", h->nnz);
    for (size_t i = 0; i < tiles.size() && rc == SMVP_OK; ++i) {
        int fits = 0;
        rc = smvp::build_column_offsets(h->d_col_ind, h->nnz, tiles[i], col_base, col16, &fits, nullptr);
        if (rc == SMVP_OK && fits) {
            h->vpt = tiles[i] / smvp::kStreamBlock;
            h->tile.d_col_base = col_base;
            h->tile.d_col16 = col16;
            h->tile.col16_tile = tiles[i];
            return SMVP_OK;
        }
    }
    (void)hipGetLastError();  // no second copy: the kernel reads col_ind itself
    for (void *p : {(void *)col16, (void *)col_base})
        if (p)
            (void)hipFree(p);
    return rc;
}

// A handle's plain launches of the tile kernel sweep the tiles forward and backward in turn where one product's algorithmic
// bytes exceed this: a product then starts on what the one before it left in the 256 MiB Infinity Cache (a cyclic sweep over
// more than the cache holds hits nothing).  Not below it: backward, XCD i takes the tiles XCD 7 - i had, so a matrix that
// lives in the L2s or in the Infinity Cache finds its lines in another XCD's L2 -- memplus x16 (30 MB) ran 27 % slower
// alternating, x40 / x100 (75 / 187 MB) 0.8 / 0.3 % slower, x200 (374 MB) 8 % faster (profiles/sweep_direction_measured.txt).
constexpr double kSweepAlternateMinBytes = 256.0 * 1024 * 1024;

// The single launches of the plain CSR tile kernel read val -- and the 16-bit column offsets, where a lane's are one 16-byte
// load -- with non-temporal loads where one product's algorithmic bytes exceed this: every line of them is read once per
// product, and a product that large finds nothing of them in the caches anyway.  Not below it: a matrix that the L2s or the
// Infinity Cache hold, wholly or in good part, is slower with the hint (profiles/col16_lane_order_measured.txt has the curve).
constexpr double kReadOnceMinBytes = 1024.0 * 1024 * 1024;

// The packed family: AUTO picks it where it would have picked STREAM at 2048-entry tiles with the 16-bit offsets in use, one
// product's algorithmic bytes exceed kReadOnceMinBytes (below that the caches hold the matrix and the decode cannot pay) and the
// share of the entries that are still read as 8-byte values -- counted exactly when the plan is built -- is at most this.
// Measured (profiles/packed_values_measured.txt, section 4: the headline's structure and pwt x459 with their values replaced, PACKED
// against STREAM alternated in one process; gain on memplus x944 / pwt x459):
//   share 0     +19.9 % / +20.5 %      0.5   +7.1 % / +8.5 %      0.6   +2.9 % / +4.0 %      0.7   -0.7 % / +1.9 %
//         0.25  +14.9 % / +15.6 %      0.55  +4.0 % / +6.2 %      0.65  +1.3 % / +3.4 %      0.75  -1.4 % / -1.0 %     1   -13.8 % / -11.9 %
// The blocks of STREAM itself spread by 0.1-0.3 % in most rows of that table and by 2.6-3.0 % in the two in which a block fell into
// the headline's other mode: 0.55 is the largest share at which the family wins by more than the largest of those spreads on both.
constexpr double kPackedMaxEscapeShare = 0.55;

inline double tile_product_bytes(const smvp_csr *h) { return 12.0 * (double)h->nnz + 12.0 * h->rows + 8.0 * h->cols; }

// STREAM_PACKED on top of a tile plan with 2048-entry tiles and 16-bit offsets.  bounded (AUTO's question): where more than
// kPackedMaxEscapeShare of the entries would still be read as doubles the build stops at the count and the plan is left without
// the arrays (SMVP_OK; TilePlan::d_code8 tells); the family set by name is built whatever the share.
int attach_packed_values(smvp_csr *h, bool bounded)
{
    TilePlan &t = h->tile;
    if (!t.d_col16 || h->vpt * smvp::kStreamBlock != smvp::kCol16LaneOrderTile)
        return smvp::fail(SMVP_ERR_UNSUPPORTED, "the packed values need 2048-entry tiles whose columns fit 16-bit offsets: this matrix's do not");
    return smvp::build_packed_values(h->d_val, h->nnz, t.d_col_base, &t.d_code8, &t.d_hot, &t.d_esc_ptr, &t.d_esc_val, &t.packed_doubles,
                                     &t.esc_slots, bounded ? (long long)(kPackedMaxEscapeShare * (double)h->nnz) : -1ll, nullptr);
}

int build_tile_plan_parts(smvp_csr *h, bool packed_bounded)
{
    TilePlan &t = h->tile;
    free_tile_plan(&t);
    t.packed_bounded = packed_bounded;
    if (int rc = try_column_offsets(h))
        return rc;
    const int tile = smvp::kStreamBlock * h->vpt;
    const long long nnz = h->nnz;
    const int ntiles = (int)std::max<long long>(1, (nnz + tile - 1) / tile);
    std::vector<int> tile_row((size_t)ntiles + 1), carry_row((size_t)ntiles), tile_next((size_t)ntiles);
    const int *rp = h->h_row_ptr.data();
    int r = 0;
    for (int b = 0; b < ntiles; ++b) {
        const long long s = (long long)b * tile;
        const long long e = std::min(s + tile, nnz);
        while (r < h->rows && rp[r] < s)
            ++r;
        tile_row[(size_t)b] = r;
        const long long first = r < h->rows ? rp[r] : nnz;
        carry_row[(size_t)b] = (std::min(first, e) > s) ? r - 1 : -1;
    }
    tile_row[(size_t)ntiles] = h->rows;
    for (int b = 0; b < ntiles; ++b)
        tile_next[(size_t)b] = rp[tile_row[(size_t)b + 1]];
    if (int rc = upload(&t.d_tile_row, tile_row))
        return rc;
    if (stream_family(h->kernel)) {
        if (int rc = upload(&t.d_tile_next, tile_next))
            return rc;
        if (h->rows > 0 && smvp::option("csr_rowrel", 1) != 0) {  // (plan option: 0 = keep row_ptr)
            std::vector<unsigned short> rel((size_t)h->rows);
            for (int b = 0; b < ntiles; ++b) {
                const long long s0 = (long long)b * tile;
                for (int rr = tile_row[(size_t)b]; rr < tile_row[(size_t)b + 1]; ++rr)
                    rel[(size_t)rr] = (unsigned short)(rp[rr] - s0);  // 0 ... tile (tile: trailing rows without entries)
            }
            if (int rc = upload(&t.d_row_rel, rel))
                return rc;
        }
    } else {
        if (int rc = upload(&t.d_carry_row, carry_row))
            return rc;
        HIP_TRY(hipMalloc((void **)&t.d_carry, std::max(ntiles, 1) * sizeof(double)));
        HIP_TRY(hipMemset(t.d_carry, 0, std::max(ntiles, 1) * sizeof(double)));
    }
    t.ntiles = ntiles;
    // plan option: 0 = every product sweeps forward, 1 = the plain launches alternate whatever the size; default: they alternate
    // where one product's bytes do not fit the Infinity Cache anyway (see kSweepAlternateMinBytes)
    const int alternate = smvp::option("csr_sweep_alternate", -1);
    const double product_bytes = tile_product_bytes(h);
    t.sweep_alternate = alternate < 0 ? product_bytes > kSweepAlternateMinBytes : alternate != 0;
    // plan option: 0 / 1 = the single launches' val and col16 loads never / always carry the read-once hint; default: by size
    const int read_once = smvp::option("csr_read_once", -1);
    t.read_once = h->flavor != smvp::kFlavorCsr ? 0 : read_once < 0 ? product_bytes > kReadOnceMinBytes : read_once != 0;
    if (h->kernel == SMVP_CSR_KERNEL_STREAM_PACKED)
        if (int rc = attach_packed_values(h, t.packed_bounded != 0))
            return rc;
    if (tile_ordered(h->flavor)) {
        // every tile's entries in TJDS order + what each tile reads past its end, in row order
        std::vector<int> ovf_ptr((size_t)ntiles + 1, 0);
        for (int b = 0; b < ntiles; ++b) {
            const long long e = std::min((long long)(b + 1) * tile, nnz);
            const bool owns = tile_row[(size_t)b] != tile_row[(size_t)b + 1];
            ovf_ptr[(size_t)b + 1] = ovf_ptr[(size_t)b] + (owns ? (int)(tile_next[(size_t)b] - e) : 0);
        }
        const int total = ovf_ptr[(size_t)ntiles];
        t.ovf_total = total;
        if (int rc = upload(&t.d_ovf_ptr, ovf_ptr))
            return rc;
        const size_t n = (size_t)std::max(h->nnz, 4), m = (size_t)std::max(total, 4);
        const bool half = h->flavor == smvp::kFlavorTjdsH;
        const TjdsSource &src = h->src;
        // (the last two: the flavour's index word per entry and its second array -- TjdsH word32 and the tiles' run_ptr, TjdsS
        // pos_sorted and meta)
        if (hipMalloc((void **)&t.d_ovf_val, m * sizeof(double)) != hipSuccess ||
            hipMalloc((void **)&t.d_ovf_k, m * sizeof(int)) != hipSuccess ||
            hipMalloc((void **)&t.d_cache_ptr, ((size_t)ntiles + 2) * sizeof(int)) != hipSuccess ||
            hipMalloc(half ? (void **)&t.d_word32 : (void **)&t.d_pos_sorted, n * sizeof(int)) != hipSuccess ||
            hipMalloc(half ? (void **)&t.d_run_ptr : (void **)&t.d_meta, (half ? (size_t)ntiles + 2 : n) * sizeof(int)) != hipSuccess)
            return smvp::fail(SMVP_ERR_ALLOC, "cannot allocate the tile-ordered TJDS streams");
        if (int rc = half ? smvp::build_tile_half_streams(src.pos, h->nnz, tile, src.start_pos, src.num_diag, h->d_val, h->cache_min_tiles,
                                                          t.d_word32, t.d_cache_ptr, t.d_run_ptr, &t.d_val_cache, &t.d_run_tab,
                                                          &t.d_group_run, &t.cached_total, &t.runs_total, nullptr)
                          : smvp::sort_tile_windows(src.pos, h->nnz, tile, src.start_pos, src.num_diag, smvp::kSlotBits, h->d_val,
                                                    h->cache_min_tiles, t.d_pos_sorted, t.d_meta, t.d_cache_ptr, &t.d_val_cache,
                                                    &t.cached_total, nullptr))
            return rc;
        if (int rc = smvp::build_tile_overflow(src.pos, t.d_ovf_ptr, total, ntiles, tile, h->nnz, src.start_pos, src.num_diag, h->d_val,
                                               t.d_ovf_val, t.d_ovf_k, src.unit_operand ? 1 : 0, nullptr))
            return rc;
    }
    return SMVP_OK;
}

// A build that fails leaves the handle without a tile plan (smvp_csr_spmv then refuses it), never with the arrays built so far.
int build_tile_plan(smvp_csr *h, bool packed_bounded = false)
{
    const int rc = build_tile_plan_parts(h, packed_bounded);
    if (rc != SMVP_OK)
        free_tile_plan(&h->tile);
    return rc;
}

int pow2_at_least(double v)
{
    int p = 2;
    while (p < 64 && p < v)
        p <<= 1;
    return p;
}

// AUTO: fixed-nnz tiles are insensitive to row-length skew and keep short rows
// at full lane use -- the owner-completes form unless some row is so long that
// one workgroup finishing it alone would be the critical path (then the carry
// form, which spreads a row over its tiles).  The wavefront-per-row kernel is
// never picked: measured on uniform rows of 64 / 128 / 400 entries it runs at
// 0.98 / 0.86 / 0.87 of the tile kernel's rate, and far below it on skewed rows.
constexpr int kOwnerMaxRow = 16 * 1024;

// false: `param` is no tile size the resolved kernel is compiled for (nothing is changed then)
bool choose_csr_kernel(smvp_csr *h, int kernel, int param)
{
    const double mean = h->rows > 0 ? (double)h->nnz / h->rows : 0.0;
    if (kernel == SMVP_CSR_KERNEL_AUTO)
        kernel = h->max_row_len > kOwnerMaxRow ? SMVP_CSR_KERNEL_STREAM_CARRY
                 : sweep_suits(h)              ? SMVP_CSR_KERNEL_COLSWEEP
                 : binned_suits(h)             ? SMVP_CSR_KERNEL_BINNED
                                               : SMVP_CSR_KERNEL_STREAM;
    if (kernel == SMVP_CSR_KERNEL_STREAM && param != 0 && param != 256 && param != 1024 && param != 2048)
        return false;
    if (kernel == SMVP_CSR_KERNEL_STREAM_CARRY && param != 0 && param != 1024 && param != 2048)
        return false;
    if (kernel == SMVP_CSR_KERNEL_STREAM_PACKED && param != 0 && param != smvp::kCol16LaneOrderTile)
        return false;
    if (kernel == SMVP_CSR_KERNEL_COLSWEEP && !sweep_param_ok(param))
        return false;
    if (kernel == SMVP_CSR_KERNEL_BINNED && param < 0)
        return false;
    h->kernel = kernel;
    if (kernel == SMVP_CSR_KERNEL_COLSWEEP || kernel == SMVP_CSR_KERNEL_BINNED)
        return true;
    if (kernel == SMVP_CSR_KERNEL_VECTOR) {
        h->lanes_per_row = param > 0 ? param : pow2_at_least(mean);
    } else {
        if (kernel == SMVP_CSR_KERNEL_STREAM_PACKED)
            param = smvp::kCol16LaneOrderTile;  // the one tile size the family has: the plan keeps it like one the caller named
        int tile = param > 0 ? param : 0;
        h->tile_chosen = param > 0;
        if (tile == 0) {  // 1024 measured 1-4 % ahead of 2048 on memplus x944 and pwt x459; 256-entry tiles when
            tile = (kernel == SMVP_CSR_KERNEL_STREAM && h->nnz < 512 * 1024) ? 256 : 1024;  // 1024 would leave CUs idle
            if ((tile_ordered(h->flavor)) && tile == 1024 && h->nnz >= 12 * 1024 * 1024)
                tile = 2048;  // more entries per val line inside a tile.  With the value cache and the 16-bit second word (round 3),
                              // memplus x59 / x118 / x236 / x472 (7.4 / 14.9 / 29.8 / 59.5 M entries), 1024 against 2048:
                              // 0.0285 / 0.0530 / 0.1157 / 0.2327 against 0.0280 / 0.0493 / 0.1070 / 0.2151 ms
        }
        h->vpt = tile / smvp::kStreamBlock;
    }
    return true;
}

// AUTO has resolved to STREAM and the tile plan stands: does the packed family take over (kPackedMaxEscapeShare has the rule)?
// Plan option "csr_packed": 0 = never; 1 = wherever the tiles allow and whatever the size (the plan moves to 2048-entry tiles
// for it), the escape share still decides; default: by the rule.  Memory that runs out, or tiles that do not suit, leave the
// handle on STREAM; only a tile plan that cannot be rebuilt is an error.
int auto_packed_values(smvp_csr *h)
{
    const int wanted = smvp::option("csr_packed", -1);
    if (wanted == 0 || h->flavor != smvp::kFlavorCsr || h->plain_only || h->nnz <= 0)
        return SMVP_OK;
    const bool tiles_suit = h->tile.d_col16 && h->vpt * smvp::kStreamBlock == smvp::kCol16LaneOrderTile;
    if (wanted < 0 && !(tiles_suit && tile_product_bytes(h) > kReadOnceMinBytes))
        return SMVP_OK;
    // (either way the build is the bounded one: it ends at the exact count where the share is over the bound, the arrays are
    // there only where the family pays)
    if (tiles_suit) {
        if (attach_packed_values(h, true) == SMVP_OK && h->tile.d_code8)
            h->kernel = SMVP_CSR_KERNEL_STREAM_PACKED;
        else
            (void)hipGetLastError();  // (a failed build leaves no array: the handle stays on STREAM, its plan as it stands)
        return SMVP_OK;
    }
    choose_csr_kernel(h, SMVP_CSR_KERNEL_STREAM_PACKED, 0);
    if (build_tile_plan(h, true) == SMVP_OK && h->tile.d_code8)
        return SMVP_OK;
    (void)hipGetLastError();
    choose_csr_kernel(h, SMVP_CSR_KERNEL_STREAM, 0);
    return build_tile_plan(h);
}

}  // namespace

// (declared ahead of its definition: the binned plan nests a handle of its own for the near part)
static int csr_create_impl(smvp_csr_t **out, int device, int rows, int cols, int nnz, const int *row_ptr, const int *col_ind, const double *val,
                           int mem_kind, const int *host_row_ptr, int flavor, const TjdsSource *src = nullptr, bool plain_only = false,
                           long long first_row = 0);

// The binned plan: near / far split on the device; the near part as the window plan (smvp_near_window.hip) where that suits,
// else behind a nested handle that stays on the tile kernels.
static int build_binned(smvp_csr *h, int band)
{
    free_binned_side(&h->binned);
    // both passes (and K6) ask for more than 64 KB of dynamic LDS: a device that refuses makes the PLAN fail here -- AUTO then
    // falls back to the tile kernel (plan_csr) -- instead of every later product
    if (hipError_t le = smvp::binned_reserve_lds(); le != hipSuccess) {
        (void)hipGetLastError();
        return smvp::fail(SMVP_ERR_UNSUPPORTED, "the binned plan needs 154 KB of LDS per workgroup: %s", hipGetErrorString(le));
    }
    const bool window = smvp::option("binned_near", 0) == 0;  // (plan option: 1 keeps the near part on the tile kernel)
    if (int rc = smvp::build_binned_plan(h->d_row_ptr, h->d_col_ind, h->d_val, h->rows, h->cols, h->nnz, band, h->row0, window, &h->binned.bin, nullptr))
        return rc;
    if (h->binned.bin.nw.on) {
        if (smvp::option("binned_overlap", 1) != 0 && h->binned.bin.nf > 0) {  // (plan option: 0 = pass A behind the near part, one stream)
            HIP_TRY(hipStreamCreateWithFlags(&h->binned.side, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&h->binned.ev_fork, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&h->binned.ev_join, hipEventDisableTiming));
        }
        return SMVP_OK;
    }
    return csr_create_impl(&h->binned.near, h->device, h->rows, h->cols, h->binned.bin.nnz_near, h->binned.bin.near_ptr, h->binned.bin.near_col, h->binned.bin.near_val,
                           SMVP_MEM_DEVICE, nullptr, smvp::kFlavorCsr, nullptr, true, h->row0);
}

// Plans a handle: resolves `kernel` (choose_csr_kernel: a `param` the resolved kernel rejects changes nothing), releases the
// plans the resolved kernel does not use, builds the one it does -- VECTOR has none -- and records plan_build_ms.  Where the
// second copy of the entries that COLSWEEP and BINNED keep does not fit (or cannot be built) the handle goes back to the tile
// kernel, which needs none: silently at creation (AUTO's choice; only the tile plan's own failure is an error), with the error
// still reported from smvp_csr_set_kernel -- the handle stays usable, and if even the tile plan fails it is left without a
// plan, which smvp_csr_spmv refuses.
static int plan_csr(smvp_csr *h, int kernel, int param, bool silent_fallback)
{
    if (!choose_csr_kernel(h, kernel, param))
        return smvp::fail(SMVP_ERR_INVALID, "entries per tile must be 256 (stream only), 1024 or 2048 (stream-packed: 2048) for the kernel "
                                            "this matrix resolves to (column sweep: 256 ... 20480 rows per block, a multiple of 4; binned: the near band, >= 0)");
    const double t0 = wall_ms();
    free_sweep_plan(&h->sweep);
    free_binned_side(&h->binned);
    int rc = SMVP_OK;
    if (runs_on_tile_plan(h->kernel)) {
        rc = build_tile_plan(h);
        if (rc == SMVP_OK && kernel == SMVP_CSR_KERNEL_AUTO && h->kernel == SMVP_CSR_KERNEL_STREAM)
            rc = auto_packed_values(h);
        if (rc != SMVP_OK && h->kernel == SMVP_CSR_KERNEL_STREAM_PACKED) {
            // the family was asked for by name and the matrix's tiles do not suit it, or its arrays do not fit: back to STREAM,
            // like the two other plans that keep a copy of the values
            const std::string why = smvp_last_error();
            (void)hipGetLastError();
            choose_csr_kernel(h, SMVP_CSR_KERNEL_STREAM, 0);
            const int tile_rc = build_tile_plan(h);
            rc = silent_fallback ? tile_rc : smvp::fail(rc, "%s", why.c_str());
        }
    } else {
        free_tile_plan(&h->tile);
        if (h->kernel != SMVP_CSR_KERNEL_VECTOR)
            rc = h->kernel == SMVP_CSR_KERNEL_COLSWEEP ? build_sweep_plan(h, param) : build_binned(h, param);
        if (rc != SMVP_OK) {
            const std::string why = smvp_last_error();
            (void)hipGetLastError();
            free_sweep_plan(&h->sweep);
            free_binned_side(&h->binned);
            h->spread = -1.0;
            choose_csr_kernel(h, SMVP_CSR_KERNEL_STREAM, 0);
            const int tile_rc = build_tile_plan(h);  // (a failure leaves no tile plan)
            rc = silent_fallback ? tile_rc : smvp::fail(rc, "%s", why.c_str());
        }
    }
    h->plan_build_ms = wall_ms() - t0;
    return rc;
}

static int csr_create_impl(smvp_csr_t **out, int device, int rows, int cols, int nnz, const int *row_ptr, const int *col_ind, const double *val,
                           int mem_kind, const int *host_row_ptr, int flavor, const TjdsSource *src, bool plain_only, long long first_row)
{
    const bool plain = flavor == smvp::kFlavorCsr;
    if (!out || rows < 0 || cols < 0 || nnz < 0 || !row_ptr ||
        (nnz > 0 && ((!col_ind && !tile_ordered(flavor)) || !val)))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_create: bad argument");
    if (mem_kind != SMVP_MEM_HOST && mem_kind != SMVP_MEM_DEVICE)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_create: bad mem_kind");
    if (nnz > kMaxEntries)
        return smvp::fail(SMVP_ERR_UNSUPPORTED, "smvp_csr_create: %d entries: shard blocks this large by rows", nnz);
    if (int rc = usable_device(device))
        return rc;
    DeviceScope on(device);

    smvp_csr *h = new smvp_csr;
    h->device = device;
    h->flavor = flavor;
    h->plain_only = plain_only;
    h->row0 = first_row;
    if (src)
        h->src = *src;
    if (h->src.unit_operand)
        h->cache_min_tiles = 0;
    h->rows = rows, h->cols = cols, h->nnz = nnz;
    h->h_row_ptr.resize((size_t)rows + 1);
    int rc = SMVP_OK;
    if (mem_kind == SMVP_MEM_HOST || host_row_ptr) {
        memcpy(h->h_row_ptr.data(), mem_kind == SMVP_MEM_HOST ? row_ptr : host_row_ptr, sizeof(int) * ((size_t)rows + 1));
    } else if (hipMemcpy(h->h_row_ptr.data(), row_ptr, sizeof(int) * ((size_t)rows + 1), hipMemcpyDeviceToHost) != hipSuccess) {
        rc = smvp::fail(SMVP_ERR_HIP, "smvp_csr_create: cannot read row_ptr back from the device");
    }
    // The kernels index with these; a malformed row_ptr would read out of bounds.
    if (rc == SMVP_OK) {
        const std::vector<int> &rp = h->h_row_ptr;
        bool ok = rp[0] == 0 && rp[(size_t)rows] == nnz;
        for (int r = 0; r < rows && ok; ++r) {
            ok = rp[(size_t)r] <= rp[(size_t)r + 1];
            h->max_row_len = std::max(h->max_row_len, rp[(size_t)r + 1] - rp[(size_t)r]);
        }
        if (!ok)
            rc = smvp::fail(SMVP_ERR_INVALID, "smvp_csr_create: row_ptr is not a non-decreasing 0..nnz sequence");
    }
    if (rc == SMVP_OK && mem_kind == SMVP_MEM_HOST) {
        for (int j = 0; j < nnz; ++j)
            if (col_ind[j] < 0 || col_ind[j] >= cols) {
                rc = smvp::fail(SMVP_ERR_INVALID, "smvp_csr_create: col_ind[%d] = %d outside [0, %d)", j, col_ind[j], cols);
                break;
            }
    }
    if (rc == SMVP_OK && mem_kind == SMVP_MEM_DEVICE &&
        (((uintptr_t)col_ind | (plain ? (uintptr_t)val : 0)) & 15u) != 0)
        rc = smvp::fail(SMVP_ERR_INVALID, "smvp_csr_create: adopted device arrays must be 16-byte aligned");
    if (rc == SMVP_OK && mem_kind == SMVP_MEM_DEVICE && col_ind)
        rc = check_device_indices(col_ind, nnz, cols, "smvp_csr_create: col_ind");
    if (rc == SMVP_OK)
        rc = to_device(&h->d_row_ptr, row_ptr, (size_t)rows + 1, mem_kind, &h->own_row_ptr);
    if (rc == SMVP_OK && col_ind)
        rc = to_device(&h->d_col_ind, col_ind, (size_t)nnz, mem_kind, &h->own_col_ind);
    if (rc == SMVP_OK)
        rc = to_device(&h->d_val, val, (size_t)nnz, mem_kind, &h->own_val);
    if (rc == SMVP_OK) {
        const double t0 = wall_ms();
        // every flavour but plain CSR exists for the owner-completes kernel only
        rc = plan_csr(h, plain ? SMVP_CSR_KERNEL_AUTO : SMVP_CSR_KERNEL_STREAM, 0, true);
        h->plan_build_ms = wall_ms() - t0;  // (with what AUTO measured to choose)
    }
    if (rc != SMVP_OK) {
        smvp_csr_destroy(h);
        return rc;
    }
    *out = h;
    return SMVP_OK;
}

int smvp::csr_create_tjds(smvp_csr_t **out, int device, int rows, int cols, int nnz, const int *d_row_ptr, const int *d_col_ind,
                          const double *d_val, int flavor, const TjdsSource &src)
{
    return csr_create_impl(out, device, rows, cols, nnz, d_row_ptr, d_col_ind, d_val, SMVP_MEM_DEVICE, nullptr, flavor, &src);
}

int smvp::csr_create_owning(smvp_csr_t **out, int device, int rows, int cols, int nnz, int *d_row_ptr, int *d_col_ind, double *d_val)
{
    *out = nullptr;
    smvp_csr_t *h = nullptr;
    if (int rc = csr_create_impl(&h, device, rows, cols, nnz, d_row_ptr, d_col_ind, d_val, SMVP_MEM_DEVICE, nullptr, smvp::kFlavorCsr))
        return rc;
    h->own_row_ptr = h->own_col_ind = h->own_val = true;
    *out = h;
    return SMVP_OK;
}

bool smvp::csr_value_cache(const smvp_csr_t *h, int *min_tiles, long long *cached_entries)
{
    const bool on = h && tile_ordered(h->flavor);
    if (min_tiles)
        *min_tiles = on ? h->cache_min_tiles : 0;
    if (cached_entries)
        *cached_entries = on ? h->tile.cached_total : 0;
    return on;
}

int smvp::csr_replan_value_cache(smvp_csr_t *h, int min_tiles)
{
    h->cache_min_tiles = min_tiles;
    return build_tile_plan(h);
}

extern "C" int smvp_csr_create(smvp_csr_t **out, int device, int rows, int cols, int nnz,
                               const int *row_ptr, const int *col_ind, const double *val,
                               int mem_kind, const int *host_row_ptr)
{
    return csr_create_impl(out, device, rows, cols, nnz, row_ptr, col_ind, val, mem_kind, host_row_ptr, smvp::kFlavorCsr);
}

// A row block [first_row, first_row + rows) of a larger matrix (what a rank of a sharded product holds): the same handle,
// but plans that go by the distance from the diagonal -- the binned plan's near / far split, its windows of x, AUTO's
// far share -- take the diagonal where it really lies.  Without this every block beyond the first 4096 rows looked all far.
extern "C" int smvp_csr_create_block(smvp_csr_t **out, int device, int rows, int cols, int nnz,
                                     const int *row_ptr, const int *col_ind, const double *val,
                                     int mem_kind, const int *host_row_ptr, long long first_row)
{
    if (first_row < 0)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_create_block: first_row < 0");
    return csr_create_impl(out, device, rows, cols, nnz, row_ptr, col_ind, val, mem_kind, host_row_ptr, smvp::kFlavorCsr, nullptr,
                           false, first_row);
}

// share (0 ... 1) of the entries further than the binned plan's default band from the diagonal: what AUTO's choice rests on
extern "C" int smvp_csr_far_share(smvp_csr_t *h, double *share)
{
    if (!h || !share)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_far_share: bad argument");
    DeviceScope on(h->device);
    *share = measured_far_share(h);
    return SMVP_OK;
}

extern "C" int smvp_csr_set_kernel(smvp_csr_t *h, int kernel, int param)
{
    if (!h)
        return smvp::fail(SMVP_ERR_INVALID, "null handle");
    if (h->flavor != smvp::kFlavorCsr && kernel != SMVP_CSR_KERNEL_STREAM)
        return smvp::fail(SMVP_ERR_UNSUPPORTED, "this matrix flavour runs on the stream kernel only");
    if (kernel < SMVP_CSR_KERNEL_AUTO || kernel > SMVP_CSR_KERNEL_STREAM_PACKED)
        return smvp::fail(SMVP_ERR_INVALID, "unknown CSR kernel %d", kernel);
    if (kernel == SMVP_CSR_KERNEL_VECTOR && param != 0 &&
        (param < 2 || param > 64 || (param & (param - 1)) != 0))
        return smvp::fail(SMVP_ERR_INVALID, "lanes per row must be a power of two in [2, 64]");
    DeviceScope on(h->device);
    // the documented re-plan after col_ind of adopted arrays changed in place: what AUTO measured belongs to the columns that
    // were there, so both figures are forgotten and taken again by whoever asks next (AUTO below, or the two getters)
    h->spread = h->far_share = -2.0;
    return plan_csr(h, kernel, param, false);
}

extern "C" int smvp_csr_get_kernel(const smvp_csr_t *h, int *kernel, int *param)
{
    if (!h)
        return smvp::fail(SMVP_ERR_INVALID, "null handle");
    if (kernel)
        *kernel = h->kernel;
    if (param)
        *param = h->kernel == SMVP_CSR_KERNEL_VECTOR ? h->lanes_per_row
                 : h->kernel == SMVP_CSR_KERNEL_COLSWEEP ? (h->sweep.rb | ((h->sweep.parts == 8 ? 3 : h->sweep.parts == 4 ? 2 : h->sweep.parts == 2 ? 1 : 0) << kSweepPartsShift))
                 : h->kernel == SMVP_CSR_KERNEL_BINNED   ? h->binned.bin.band
                                                         : h->vpt * smvp::kStreamBlock;
    return SMVP_OK;
}

extern "C" int smvp_csr_gather_spread(smvp_csr_t *h, double *spread)
{
    if (!h || !spread)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_gather_spread: bad argument");
    DeviceScope on(h->device);
    *spread = measured_spread(h);
    return SMVP_OK;
}

static int fill_owner_launch(const smvp_csr_t *h, const double *d_x, double *d_y, unsigned long long *stamps, smvp::OwnerLaunch *out)
{
    if (h->tile.d_col16 && h->tile.col16_tile != smvp::kStreamBlock * h->vpt)  // (every re-plan rebuilds them: a plan bug, not a caller's)
        return smvp::fail(SMVP_ERR_INVALID, "the 16-bit column offsets were laid out for %d-entry tiles, the launch has %d-entry tiles",
                          h->tile.col16_tile, smvp::kStreamBlock * h->vpt);
    smvp::OwnerLaunch &l = *out;
    l.row_ptr = h->d_row_ptr, l.col_ind = h->d_col_ind, l.val = h->d_val, l.x = d_x, l.y = d_y;
    l.tile_row = h->tile.d_tile_row, l.tile_next = h->tile.d_tile_next;
    l.pos = h->src.pos, l.start_pos = h->src.start_pos;
    if (tile_ordered(h->flavor)) {
        l.pos = h->tile.d_pos_sorted, l.col_ind = h->tile.d_meta;
        l.ovf_ptr = h->tile.d_ovf_ptr, l.ovf_val = h->tile.d_ovf_val, l.ovf_k = h->tile.d_ovf_k;
        l.cache_ptr = h->tile.d_cache_ptr, l.val_cache = h->tile.d_val_cache;
        l.word32 = h->tile.d_word32, l.group_run = h->tile.d_group_run, l.run_ptr = h->tile.d_run_ptr, l.run_tab = h->tile.d_run_tab;
    }
    l.stamps = stamps;
    l.rows = h->rows, l.nnz = h->nnz, l.ntiles = h->tile.ntiles;
    l.col16 = h->tile.d_col16, l.col_base = h->tile.d_col_base;
    l.code8 = h->tile.d_code8, l.hot = h->tile.d_hot, l.esc_ptr = h->tile.d_esc_ptr, l.esc_val = h->tile.d_esc_val;
    l.row_rel = h->tile.d_row_rel;
    l.read_once = h->tile.read_once;
    l.unit_x = h->src.unit_operand ? 1 : 0;
    return SMVP_OK;
}

// `reps` products of the tile kernel in ONE launch, each product's window stamped (csr_stream_owner_repeat); grid from
// csr_repeat_grid.  The products are those of csr_spmv_stamped, bit for bit: the same kernel body walks the same tiles.
int smvp::csr_repeat_grid(const smvp_csr_t *h)
{
    if (!h || h->kernel != SMVP_CSR_KERNEL_STREAM || !h->tile.d_tile_row || h->rows <= 0)  // (STREAM_PACKED has no repeating form)
        return 0;
    DeviceScope on(h->device);
    return smvp::owner_repeat_grid(h->vpt, owner_flavor(h), h->tile.ntiles);
}

int smvp::csr_spmv_repeat(smvp_csr_t *h, const double *d_x, double *d_y, void *stream, unsigned long long *stamps, int reps, int grid,
                          unsigned *ctl_words, bool first_of_run, unsigned long long patience)
{
    DeviceScope on(h->device);
    smvp::OwnerLaunch l{};
    if (int rc = fill_owner_launch(h, d_x, d_y, stamps, &l))
        return rc;
    const hipError_t e = smvp::launch_csr_stream_owner_repeat(h->vpt, owner_flavor(h), l, reps, grid, ctl_words,
                                                              first_of_run, patience, (hipStream_t)stream);
    if (e != hipSuccess)
        return smvp::fail(SMVP_ERR_HIP, "repeating CSR launch failed: %s", hipGetErrorString(e));
    return SMVP_OK;
}

// what a launch of smvp_csr_spmv returned, as the call's result
static int launched(hipError_t e)
{
    return e == hipSuccess ? (int)SMVP_OK : smvp::fail(SMVP_ERR_HIP, "CSR launch failed: %s", hipGetErrorString(e));
}

// stamps: device-side timing slots of this launch (owner kernel only), or nullptr
int smvp::csr_spmv_stamped(smvp_csr_t *h, const double *d_x, double *d_y, void *stream, unsigned long long *stamps)
{
    if (!h || (h->rows > 0 && !d_y) || (h->nnz > 0 && !d_x))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_spmv: bad argument");
    if ((h->kernel == SMVP_CSR_KERNEL_COLSWEEP && !h->sweep.d_ptr) || (h->kernel == SMVP_CSR_KERNEL_BINNED && !h->binned.near && !h->binned.bin.nw.on) ||
        (runs_on_tile_plan(h->kernel) && !h->tile.d_tile_row))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_spmv: the handle has no launch plan (a re-plan failed earlier)");
    DeviceScope on(h->device);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (h->kernel == SMVP_CSR_KERNEL_BINNED) {
        // the near part writes every row of y; pass A puts the far products into the bins; pass B adds each row's far sum.
        // (With the near part on the TILE kernel, pass A was tried beside it twice.  On a stream of its own its one workgroup per
        // CU -- 132 KB of LDS -- only got onto a CU once the tile kernel's six had drained: one after the other anyway,
        // 0.777 against 0.757 ms.  As one persistent workgroup per CU enqueued AHEAD of the near product the two did share
        // the CUs -- and pass A then took 264 instead of 238 us while the near product finished 241 us after it instead of
        // 303: 0.7485 against 0.7540 ms.  What one gains the other loses: profiles/r04_binned_measured.txt.)
        if (h->binned.bin.nw.on && h->binned.side) {
            // The window plan's near part and pass A are both one-workgroup-per-CU kernels (148 / 132 KB of LDS): enqueued
            // side by side -- pass A first, on a stream of its own: it needs x only -- their workgroups share the chip one
            // CU at a time, the near part's take the CUs that pass A's last workgroups leave, and a kernel that mostly
            // reads runs beside one that writes 40 % of its bytes: 0.683-0.697 -> 0.651-0.669 ms on the random model
            // (profiles/r04_binned_measured.txt, section 12; the near part first: 0.668-0.670).  Pass B waits for both.
            HIP_TRY(hipEventRecord(h->binned.ev_fork, st));
            HIP_TRY(hipStreamWaitEvent(h->binned.side, h->binned.ev_fork, 0));
            if (int rc = launched(smvp::launch_binned_products(h->binned.bin, d_x, h->binned.side)))
                return rc;
            // From here on pass A is in flight on the side stream, reading x and writing the bins: whatever fails below, the
            // caller's stream is joined to it before the error goes back -- the caller may free x or destroy the handle next.
            int rc = SMVP_OK;
            hipError_t je = hipEventRecord(h->binned.ev_join, h->binned.side);
            if (je == hipSuccess) {
                rc = launched(smvp::launch_near_window(h->binned.bin.nw, d_x, d_y, st));
                je = hipStreamWaitEvent(st, h->binned.ev_join, 0);
            }
            if (je != hipSuccess) {
                (void)hipStreamSynchronize(h->binned.side);  // the join could not be enqueued: wait for pass A here
                return smvp::fail(SMVP_ERR_HIP, "joining the binned plan's side stream failed: %s", hipGetErrorString(je));
            }
            if (rc != SMVP_OK)
                return rc;
            return launched(smvp::launch_binned_sums(h->binned.bin, d_y, st));
        }
        if (h->binned.bin.nw.on) {
            if (int rc = launched(smvp::launch_near_window(h->binned.bin.nw, d_x, d_y, st)))
                return rc;
        } else if (int rc = smvp::csr_spmv_stamped(h->binned.near, d_x, d_y, stream, nullptr))
            return rc;
        if (int rc = launched(smvp::launch_binned_products(h->binned.bin, d_x, st)))
            return rc;
        e = smvp::launch_binned_sums(h->binned.bin, d_y, st);
    } else if (h->kernel == SMVP_CSR_KERNEL_COLSWEEP)
        e = smvp::launch_csr_colsweep(h->sweep.d_ptr, h->sweep.d_col, h->sweep.d_val, h->sweep.d_row, d_x, d_y, h->rows,
                                      sweep_strip_rows(h->sweep), h->sweep.parts, h->sweep.per_launch, h->sweep.g, h->sweep.d_part, st);
    else if (h->kernel == SMVP_CSR_KERNEL_VECTOR)
        e = smvp::launch_csr_vector(h->lanes_per_row, h->d_row_ptr, h->d_col_ind, h->d_val, d_x, d_y, h->rows, st);
    else if (stream_family(h->kernel)) {
        smvp::OwnerLaunch l{};
        if (int rc = fill_owner_launch(h, d_x, d_y, stamps, &l))
            return rc;
        // the plain single launch, stamped or not, of a CSR handle, of a binned plan's near handle and of a TJDS handle's
        // tile-ordered stream (all come through here): this one sweeps the way the last one did not
        l.backward = h->tile.sweep_backward;
        h->tile.sweep_backward = h->tile.sweep_alternate ? !l.backward : 0;
        e = smvp::launch_csr_stream_owner(h->vpt, owner_flavor(h), l, st);
    } else
        e = smvp::launch_csr_stream(h->vpt, h->d_row_ptr, h->d_col_ind, h->d_val, d_x, d_y, h->tile.d_tile_row,
                                    h->tile.d_carry_row, h->tile.d_carry, h->rows, h->nnz, h->tile.ntiles, st);
    return launched(e);
}

extern "C" int smvp_csr_spmv(smvp_csr_t *h, const double *d_x, double *d_y, void *stream)
{
    return smvp::csr_spmv_stamped(h, d_x, d_y, stream, nullptr);
}

// What the solvers on a CSR handle (K11 to K14, K16, K18, K19, K22; the steps are smvp_power.hip's, smvp_cg.hip's, smvp_bicgstab.hip's,
// smvp_gmres.hip's and smvp_lsqr.hip's) share: the
// product is smvp_csr_spmv's on the current plan, which it leaves as it is, and a handle that belongs to a TJDS matrix is refused.
static smvp::HandleProduct csr_product(smvp_csr_t *h, void *stream)
{
    return [h, stream](const double *x, double *y) { return smvp_csr_spmv(h, x, y, stream); };
}

static int refuse_tjds_flavor(const char *fn, const smvp_csr_t *h)
{
    if (h->flavor != smvp::kFlavorCsr)
        return smvp::fail(SMVP_ERR_UNSUPPORTED, "%s: plain CSR handles only (this one belongs to a TJDS matrix)", fn);
    return SMVP_OK;
}

extern "C" int smvp_csr_power_method(smvp_csr_t *h, const smvp_power_opts_t *opts, const double *d_x0, double *d_x,
                                     smvp_power_result_t *result, double *lambda_each, double *residual_each, void *stream)
{
    if (int rc = smvp::power_check_args("smvp_csr_power_method", h, opts, result))
        return rc;
    if (int rc = refuse_tjds_flavor("smvp_csr_power_method", h))
        return rc;
    return smvp::power_run("smvp_csr_power_method", h->device, h->rows, h->cols, opts, d_x0, d_x, result, lambda_each, residual_each, stream,
                           csr_product(h, stream));
}

extern "C" int smvp_csr_cg(smvp_csr_t *h, const smvp_cg_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                           smvp_cg_result_t *result, double *rr_each, double *sigma_each, void *stream)
{
    if (int rc = smvp::cg_check_args("smvp_csr_cg", h, opts, result, d_b, smvp::Precond::none, {}))
        return rc;
    if (int rc = refuse_tjds_flavor("smvp_csr_cg", h))
        return rc;
    return smvp::cg_run("smvp_csr_cg", h->device, h->rows, h->cols, opts, d_b, d_x0, d_x, result, rr_each, sigma_each, stream,
                        csr_product(h, stream));
}

extern "C" int smvp_csr_pcg(smvp_csr_t *h, const smvp_cg_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                            const double *d_m, smvp_pcg_result_t *result, double *rr_each, double *rz_each, double *sigma_each,
                            void *stream)
{
    const smvp::KrylovPrecond M{nullptr, d_m, nullptr};
    if (int rc = smvp::cg_check_args("smvp_csr_pcg", h, opts, result, d_b, smvp::Precond::diagonal, M))
        return rc;
    if (int rc = refuse_tjds_flavor("smvp_csr_pcg", h))
        return rc;
    return smvp::cg_run("smvp_csr_pcg", h->device, h->rows, h->cols, opts, d_b, d_x0, d_x, smvp::Precond::diagonal, M, result, rr_each, rz_each,
                        sigma_each, stream, csr_product(h, stream));
}

extern "C" int smvp_csr_pcg_tri(smvp_csr_t *h, const smvp_cg_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                                smvp_trsv_t *first, const double *d_m, smvp_trsv_t *second, smvp_pcg_result_t *result, double *rr_each,
                                double *rz_each, double *sigma_each, void *stream)
{
    const smvp::KrylovPrecond M{first, d_m, second};
    if (int rc = smvp::cg_check_args("smvp_csr_pcg_tri", h, opts, result, d_b, smvp::Precond::stored, M))
        return rc;
    if (int rc = refuse_tjds_flavor("smvp_csr_pcg_tri", h))
        return rc;
    return smvp::cg_run("smvp_csr_pcg_tri", h->device, h->rows, h->cols, opts, d_b, d_x0, d_x, smvp::Precond::stored, M, result, rr_each, rz_each,
                        sigma_each, stream, csr_product(h, stream));
}

// K14: the diagonal from the handle's own arrays (val is read in place: adopted values changed in place are seen).  No plan, nothing
// of the handle is written; the group of lanes a row gets follows the mean row length, the VECTOR plan's rule.
extern "C" int smvp_csr_diagonal(const smvp_csr_t *h, double *d_diag, void *stream)
{
    if (!h || (h->rows > 0 && !d_diag))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_diagonal: null %s", !h ? "handle" : "d_diag");
    if (int rc = refuse_tjds_flavor("smvp_csr_diagonal", h))
        return rc;
    DeviceScope on(h->device);
    const hipError_t e = smvp::launch_csr_diagonal(pow2_at_least(h->rows > 0 ? (double)h->nnz / h->rows : 0.0), h->d_row_ptr, h->d_col_ind,
                                                   h->d_val, d_diag, h->rows, h->cols, h->row0, (hipStream_t)stream);
    if (e != hipSuccess)
        return smvp::fail(SMVP_ERR_HIP, "smvp_csr_diagonal: launch failed: %s", hipGetErrorString(e));
    return SMVP_OK;
}

// K15 (smvp_trsv.hip) plans beside the handle: what it borrows
smvp::CsrView smvp::csr_view(const smvp_csr_t *h)
{
    return {h->device, h->rows, h->cols, h->nnz, h->flavor, h->row0, h->d_row_ptr, h->d_col_ind, h->d_val, h->h_row_ptr.data()};
}

extern "C" int smvp_csr_bicgstab(smvp_csr_t *h, const smvp_bicgstab_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                                 smvp_bicgstab_result_t *result, double *rr_each, double *ss_each, void *stream)
{
    if (int rc = smvp::bicgstab_check_args("smvp_csr_bicgstab", h, opts, result, d_b))
        return rc;
    if (int rc = refuse_tjds_flavor("smvp_csr_bicgstab", h))
        return rc;
    return smvp::bicgstab_run("smvp_csr_bicgstab", h->device, h->rows, h->cols, opts, d_b, d_x0, d_x, nullptr, result, rr_each, ss_each, stream,
                              csr_product(h, stream));
}

extern "C" int smvp_csr_pbicgstab(smvp_csr_t *h, const smvp_bicgstab_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                                  smvp_trsv_t *first, const double *d_m, smvp_trsv_t *second, smvp_bicgstab_result_t *result,
                                  double *rr_each, double *ss_each, void *stream)
{
    const smvp::KrylovPrecond M{first, d_m, second};
    if (int rc = smvp::pbicgstab_check_args("smvp_csr_pbicgstab", h, opts, result, d_b, M))
        return rc;
    if (int rc = refuse_tjds_flavor("smvp_csr_pbicgstab", h))
        return rc;
    return smvp::bicgstab_run("smvp_csr_pbicgstab", h->device, h->rows, h->cols, opts, d_b, d_x0, d_x, &M, result, rr_each, ss_each, stream,
                              csr_product(h, stream));
}

extern "C" int smvp_csr_gmres(smvp_csr_t *h, const smvp_gmres_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                              smvp_trsv_t *first, const double *d_m, smvp_trsv_t *second, smvp_gmres_result_t *result, double *rr_each,
                              double *restart_each, void *stream)
{
    if (int rc = smvp::gmres_check_args("smvp_csr_gmres", h, opts, result, d_b))
        return rc;
    if (int rc = refuse_tjds_flavor("smvp_csr_gmres", h))
        return rc;
    return smvp::gmres_run("smvp_csr_gmres", h->device, h->rows, h->cols, opts, d_b, d_x0, d_x, smvp::KrylovPrecond{first, d_m, second}, result,
                           rr_each, restart_each, stream, csr_product(h, stream));
}

// K22: h is M x N, ht the caller's handle of A^T; each multiplies on its own current plan, which it keeps
extern "C" int smvp_csr_lsqr(smvp_csr_t *h, smvp_csr_t *ht, const smvp_lsqr_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                             smvp_lsqr_result_t *result, double *rnorm_each, double *arnorm_each, void *stream)
{
    const char *fn = "smvp_csr_lsqr";
    if (int rc = smvp::lsqr_check_args(fn, h, ht, true, opts, result, d_b))
        return rc;
    for (const smvp_csr_t *a : {(const smvp_csr_t *)h, (const smvp_csr_t *)ht}) {
        if (int rc = refuse_tjds_flavor(fn, a))
            return rc;
        if (a->row0 != 0)
            return smvp::fail(SMVP_ERR_UNSUPPORTED, "%s: %s is a row block (first_row = %lld): whole matrices only", fn, a == h ? "h" : "ht", a->row0);
    }
    if (ht->rows != h->cols || ht->cols != h->rows || ht->nnz != h->nnz)
        return smvp::fail(SMVP_ERR_INVALID, "%s: ht is %d x %d with %d entries, the transpose of h (%d x %d, %d entries) is not", fn, ht->rows,
                          ht->cols, ht->nnz, h->rows, h->cols, h->nnz);
    if (ht->device != h->device)
        return smvp::fail(SMVP_ERR_INVALID, "%s: ht lives on device %d, h on device %d", fn, ht->device, h->device);
    return smvp::lsqr_run(fn, h->device, h->rows, h->cols, opts, d_b, d_x0, d_x, result, rnorm_each, arnorm_each, stream, csr_product(h, stream),
                          csr_product(ht, stream));
}

// the owner kernel, whose launch can time itself on the device?
int smvp::csr_stamp_slots(const smvp_csr_t *h)
{
    return h && stream_family(h->kernel) && h->tile.d_tile_row ? smvp::owner_stamp_slots(h->tile.ntiles, h->flavor) : 0;
}

std::string smvp::csr_owner_kernel_name(const smvp_csr_t *h)
{
    char name[64];
    snprintf(name, sizeof name, "csr_stream_owner<%d, %d, false>", h ? h->vpt : 0, h ? owner_flavor(h) : 0);
    return name;
}

extern "C" int smvp_csr_describe(const smvp_csr_t *h, char *kernel_name, size_t cap, double *alg_bytes)
{
    if (!h)
        return smvp::fail(SMVP_ERR_INVALID, "null handle");
    if (kernel_name && cap) {
        if (h->kernel == SMVP_CSR_KERNEL_BINNED && h->binned.bin.nw.on)
            snprintf(kernel_name, cap, "csr_binned: csr_near_window + csr_binned_far_products<2> + csr_binned_far_sums<%d, %d, 2>", h->binned.bin.slots,
                     h->binned.bin.threads_b);
        else if (h->kernel == SMVP_CSR_KERNEL_BINNED)
            snprintf(kernel_name, cap, "csr_binned: %s + csr_binned_far_products<2> + csr_binned_far_sums<%d, %d, 2>",
                     smvp::csr_owner_kernel_name(h->binned.near).c_str(), h->binned.bin.slots, h->binned.bin.threads_b);
        else if (h->kernel == SMVP_CSR_KERNEL_COLSWEEP)
            if (h->sweep.parts == smvp::kSweepXcdParts)
                snprintf(kernel_name, cap, "csr_colsweep<%d> (8 column parts, one per XCD) + sweep_combine", h->sweep.g);
            else if (h->sweep.parts > 1)
                snprintf(kernel_name, cap, "csr_colsweep<%d> (%d column parts)", h->sweep.g, h->sweep.parts);
            else
                snprintf(kernel_name, cap, "csr_colsweep<%d>", h->sweep.g);
        else if (h->kernel == SMVP_CSR_KERNEL_VECTOR)
            snprintf(kernel_name, cap, "csr_vector_rows<%d>", h->lanes_per_row);
        else if (stream_family(h->kernel))
            snprintf(kernel_name, cap, "%s", smvp::csr_owner_kernel_name(h).c_str());
        else
            snprintf(kernel_name, cap, "csr_stream_tiles<%d>", h->vpt);
    }
    if (alg_bytes)
        *alg_bytes = csr_matrix_bytes(h) + 8.0 * h->cols + 8.0 * h->rows;
    return SMVP_OK;
}

// kernel launches one product of the current plan takes (the column sweep starts its workgroups in generations)
extern "C" int smvp_csr_plan_launches(const smvp_csr_t *h, int *launches)
{
    if (!h || !launches)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_plan_launches: bad argument");
    *launches = 1;
    if (h->kernel == SMVP_CSR_KERNEL_COLSWEEP && h->sweep.rb > 0 && h->sweep.per_launch > 0) {
        const bool xcd = h->sweep.parts == smvp::kSweepXcdParts;
        const int nwg = (h->rows + h->sweep.rb - 1) / h->sweep.rb * (xcd ? smvp::kSweepXcdParts : 1);
        *launches = std::max(1, (nwg + h->sweep.per_launch - 1) / h->sweep.per_launch) + (xcd ? 1 : 0);  // (+ sweep_combine)
    } else if (h->kernel == SMVP_CSR_KERNEL_STREAM_CARRY && h->tile.ntiles > 1) {
        *launches = 2;
    } else if (h->kernel == SMVP_CSR_KERNEL_BINNED && h->binned.bin.nw.on) {
        *launches = 1 + (h->binned.bin.nw.n_out > 0 ? 1 : 0) + (h->binned.bin.nf > 0 ? 2 : 0);
    } else if (h->kernel == SMVP_CSR_KERNEL_BINNED && h->binned.near) {
        int near = 1;
        (void)smvp_csr_plan_launches(h->binned.near, &near);
        *launches = near + (h->binned.bin.nf > 0 ? 2 : 0);
    }
    return SMVP_OK;
}

// bytes of device memory the current launch plan keeps beside row_ptr / col_ind / val
double smvp::csr_plan_bytes(const smvp_csr_t *h)
{
    const double n = h->nnz, t = h->tile.ntiles;
    if (h->kernel == SMVP_CSR_KERNEL_BINNED)
        return (double)h->binned.bin.plan_bytes + (h->binned.near ? smvp::csr_plan_bytes(h->binned.near) : 0.0);
    if (h->kernel == SMVP_CSR_KERNEL_COLSWEEP) {
        const bool xcd = h->sweep.parts == smvp::kSweepXcdParts;
        const int strip_rows = std::max(1, sweep_strip_rows(h->sweep));
        return 14.0 * n + 8.0 * ((double)((h->rows + strip_rows - 1) / strip_rows) * h->sweep.parts + 2) + (xcd ? 64.0 * h->rows : 0.0);
    }
    if (h->kernel == SMVP_CSR_KERNEL_VECTOR)
        return 0.0;
    double b = 4.0 * (t + 1) + 4.0 * t;  // tile_row + tile_next (or carry_row)
    if (h->kernel == SMVP_CSR_KERNEL_STREAM_CARRY)
        b += 8.0 * t;
    if (h->tile.d_col16)
        b += 2.0 * n + 4.0 * (n / 1024 + 1);
    if (h->tile.d_row_rel)
        b += 2.0 * h->rows;
    if (h->tile.d_code8)  // a code per entry, the hot table, four run starts per tile, the escapes (padded)
        b += 1.0 * n + 8.0 * smvp::kHotValues + 4.0 * (4.0 * t + 1) + 8.0 * (double)h->tile.esc_slots;
    if (tile_ordered(h->flavor)) {
        b += 4.0 * (t + 1) + 12.0 * h->tile.ovf_total + 4.0 * (t + 2) + 8.0 * h->tile.cached_total;
        b += h->flavor == smvp::kFlavorTjdsH ? 4.0 * n + 4.0 * (t + 2) + 8.0 * h->tile.runs_total + 2.0 * (n / 32 + 1) : 8.0 * n;
    }
    return b;
}

extern "C" int smvp_csr_plan_info(const smvp_csr_t *h, smvp_plan_info_t *out)
{
    if (!h || !out)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_plan_info: bad argument");
    out->matrix_bytes = csr_matrix_bytes(h);
    out->plan_bytes = smvp::csr_plan_bytes(h);
    out->build_ms = h->plan_build_ms;
    return SMVP_OK;
}

// K7's enqueue, for smvp_csr_spmm and for K20's steps: the arguments are checked and the handle's device is current.  The first call
// on a handle builds the plan (and synchronises `st`).
static int csr_spmm_enqueue(smvp_csr_t *h, int k, const double *d_X, long long ldx, double *d_Y, long long ldy, hipStream_t st)
{
    if (!h->spmm.planned) {
        if (int rc = refuse_capture(st, "smvp_csr_spmm: the first call on a handle builds its plan and cannot be captured "
                                        "(call it once outside the capture)"))
            return rc;
        const double t0 = wall_ms();
        int *order = h->spmm.d_order;  // (kept from a call whose build failed)
        if (h->rows > 0 && !order && hipMalloc((void **)&order, sizeof(int) * (size_t)h->rows) != hipSuccess)
            return smvp::fail(SMVP_ERR_ALLOC, "smvp_csr_spmm: cannot allocate the plan (%d rows)", h->rows);
        h->spmm.d_order = order;
        if (int rc = smvp::build_spmm_order(h->d_row_ptr, h->rows, h->max_row_len, h->spmm.d_order, st))
            return rc;
        h->spmm.planned = true;
        h->spmm.build_ms = wall_ms() - t0;
    }
    const hipError_t e = smvp::launch_csr_spmm(h->d_row_ptr, h->d_col_ind, h->d_val, h->spmm.d_order, d_X, ldx, d_Y, ldy, h->rows, k, st);
    if (e != hipSuccess)
        return smvp::fail(SMVP_ERR_HIP, "smvp_csr_spmm: launch failed: %s", hipGetErrorString(e));
    return SMVP_OK;
}

// K7: every argument is checked before anything is enqueued; the first call builds the plan (and synchronises `stream`)
extern "C" int smvp_csr_spmm(smvp_csr_t *h, int k, const double *d_X, long long ldx, double *d_Y, long long ldy, void *stream)
{
    if (!h)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_spmm: null handle");
    if (h->flavor != smvp::kFlavorCsr)
        return smvp::fail(SMVP_ERR_UNSUPPORTED, "smvp_csr_spmm: plain CSR handles only (this one belongs to a TJDS matrix)");
    if (int rc = check_block_operands("smvp_csr_spmm", k, d_X, ldx, h->cols, d_Y, ldy, h->rows, h->nnz))  // X(c, v), c < cols; Y(r, v), r < rows
        return rc;
    DeviceScope on(h->device);
    return csr_spmm_enqueue(h, k, d_X, ldx, d_Y, ldy, (hipStream_t)stream);
}

// K20: k runs of K12 (d_m == NULL) or K14 around K7's enqueue on all k directions; the SpMV plan is neither used nor touched
extern "C" int smvp_csr_cg_multi(smvp_csr_t *h, const smvp_cg_opts_t *opts, int k, const double *d_B, long long ldb, const double *d_X0,
                                 long long ldx0, double *d_X, long long ldx, const double *d_m, smvp_pcg_result_t *results, double *rr_each,
                                 double *rz_each, double *sigma_each, void *stream)
{
    if (int rc = smvp::cg_multi_check_args("smvp_csr_cg_multi", h, opts, results, d_B))
        return rc;
    if (int rc = refuse_tjds_flavor("smvp_csr_cg_multi", h))
        return rc;
    return smvp::cg_multi_run("smvp_csr_cg_multi", h->device, h->rows, h->cols, opts, k, d_B, ldb, d_X0, ldx0, d_X, ldx, d_m, results, rr_each,
                              rz_each, sigma_each, stream, [h, k, stream](const double *X, long long ldX, double *Y, long long ldY) {
                                  return csr_spmm_enqueue(h, k, X, ldX, Y, ldY, (hipStream_t)stream);
                              });
}

extern "C" int smvp_csr_spmm_describe(const smvp_csr_t *h, int k, char *kernel_name, size_t cap, double *alg_bytes, smvp_plan_info_t *plan)
{
    if (!h)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_spmm_describe: null handle");
    if (h->flavor != smvp::kFlavorCsr)
        return smvp::fail(SMVP_ERR_UNSUPPORTED, "smvp_csr_spmm_describe: plain CSR handles only");
    if (k < 1)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_spmm_describe: k = %d (need k >= 1)", k);
    if (kernel_name && cap)
        smvp::spmm_kernel_name(k, kernel_name, cap);
    if (alg_bytes)
        *alg_bytes = csr_matrix_bytes(h) + 8.0 * k * ((double)h->cols + h->rows);
    if (plan) {
        plan->matrix_bytes = csr_matrix_bytes(h);
        plan->plan_bytes = h->spmm.planned ? 4.0 * h->rows : 0.0;
        plan->build_ms = h->spmm.planned ? h->spmm.build_ms : 0.0;
    }
    return SMVP_OK;
}

extern "C" int smvp_csr_device_arrays(const smvp_csr_t *h, const int **d_row_ptr, const int **d_col_ind, const double **d_val)
{
    if (!h)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_device_arrays: null handle");
    if (h->flavor != smvp::kFlavorCsr)
        return smvp::fail(SMVP_ERR_UNSUPPORTED, "smvp_csr_device_arrays: plain CSR handles only (this one belongs to a TJDS matrix)");
    if (d_row_ptr)
        *d_row_ptr = h->d_row_ptr;
    if (d_col_ind)
        *d_col_ind = h->d_col_ind;
    if (d_val)
        *d_val = h->d_val;
    return SMVP_OK;
}

// A^T as a CSR handle of its own: the entries with row and column swapped, in storage order, through the device converter (a
// stable sort by the new row, then the new column: rows of A^T get ascending columns, ties in h's storage order)
extern "C" int smvp_csr_create_transposed(smvp_csr_t **out, const smvp_csr_t *h, void *stream)
{
    if (out)
        *out = nullptr;
    if (!out || !h)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_create_transposed: null %s", out ? "handle" : "out");
    if (h->flavor != smvp::kFlavorCsr)
        return smvp::fail(SMVP_ERR_UNSUPPORTED, "smvp_csr_create_transposed: plain CSR handles only (this one belongs to a TJDS matrix)");
    DeviceScope on(h->device);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = refuse_capture(st, "smvp_csr_create_transposed: allocates and synchronises, so it cannot be captured "
                                    "(the stream is capturing)"))
        return rc;
    const int t_rows = h->cols, t_cols = h->rows, nnz = h->nnz;
    int *t_row_ptr = nullptr, *t_col_ind = nullptr;
    double *t_val = nullptr;
    smvp_coo_t *coo = nullptr;
    auto release = [&]() {
        for (void *p : {(void *)t_row_ptr, (void *)t_col_ind, (void *)t_val, (void *)coo})
            if (p)
                (void)hipFree(p);
    };
    if (hipMalloc((void **)&t_row_ptr, sizeof(int) * ((size_t)t_rows + 4)) != hipSuccess ||
        hipMalloc((void **)&t_col_ind, sizeof(int) * std::max<size_t>((size_t)nnz, 4)) != hipSuccess ||
        hipMalloc((void **)&t_val, sizeof(double) * std::max<size_t>((size_t)nnz, 4)) != hipSuccess ||
        hipMalloc((void **)&coo, sizeof(smvp_coo_t) * std::max<size_t>((size_t)nnz, 4)) != hipSuccess) {
        (void)hipGetLastError();
        release();
        return smvp::fail(SMVP_ERR_ALLOC, "smvp_csr_create_transposed: cannot allocate the transposed arrays and the entry list (%d entries)", nnz);
    }
    int rc = SMVP_OK;
    const hipError_t e = smvp::launch_csr_swapped_coo(h->d_row_ptr, h->d_col_ind, h->d_val, h->rows, nnz, coo, st);
    if (e != hipSuccess)
        rc = smvp::fail(SMVP_ERR_HIP, "smvp_csr_create_transposed: launch failed: %s", hipGetErrorString(e));
    if (rc == SMVP_OK) {
        rc = smvp_csr_from_coo_device(coo, t_rows, t_cols, nnz, t_row_ptr, t_col_ind, t_val, stream);  // returns after the work on `stream`
        if (rc == SMVP_ERR_HIP && strstr(smvp_last_error(), "out of memory")) {
            (void)hipGetLastError();
            rc = smvp::fail(SMVP_ERR_ALLOC, "smvp_csr_create_transposed: cannot allocate the sort's buffers (%d entries)", nnz);
        }
    }
    if (rc != SMVP_OK)
        (void)hipStreamSynchronize(st);  // (nothing of this call may still read the entry list)
    (void)hipFree(coo);
    coo = nullptr;
    smvp_csr_t *t = nullptr;
    if (rc == SMVP_OK) {
        rc = csr_create_impl(&t, h->device, t_rows, t_cols, nnz, t_row_ptr, t_col_ind, t_val, SMVP_MEM_DEVICE, nullptr, smvp::kFlavorCsr);
        if (rc == SMVP_ERR_HIP && strstr(smvp_last_error(), "out of memory")) {
            (void)hipGetLastError();
            rc = smvp::fail(SMVP_ERR_ALLOC, "smvp_csr_create_transposed: cannot allocate the transposed handle's plan (%d entries)", nnz);
        }
    }
    if (rc != SMVP_OK) {
        release();
        return rc;
    }
    t->own_row_ptr = t->own_col_ind = t->own_val = true;  // (adopted from this call: the handle frees them)
    *out = t;
    return SMVP_OK;
}

extern "C" void smvp_csr_destroy(smvp_csr_t *h)
{
    if (!h)
        return;
    DeviceScope on(h->device);
    smvp::debug_owner_phases();  // (print in diagnostic builds only)
    smvp::debug_binned_phases();
    free_tile_plan(&h->tile);
    free_sweep_plan(&h->sweep);
    free_binned_side(&h->binned);
    free_spmm_plan(&h->spmm);
    if (h->own_row_ptr && h->d_row_ptr)
        (void)hipFree(h->d_row_ptr);
    if (h->own_col_ind && h->d_col_ind)
        (void)hipFree(h->d_col_ind);
    if (h->own_val && h->d_val)
        (void)hipFree(h->d_val);
    delete h;
}
