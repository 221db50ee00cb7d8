/*
 * smvp_amd.h -- C ABI of the MI355X-native SpMV engine (libsmvp_amd.so).
 *
 * This is the drop-in boundary for smvp-toolkit's CSR / TJDS path.  The
 * reference has no plugin or FFI layer: its boundary is the pair of C functions
 * main() calls (main-cli.c:325 smvp_csr_compute, main-cli.c:734
 * smvp_tjds_compute) plus the Matrix Market reader and the report writer around
 * them.  Each entry point below names the reference interface it replaces.
 * Paths are relative to the reference checkout (smvp-toolkit v0.6.4).
 *
 * Conventions
 *   - plain C types only; every function returns an int status (0 = SMVP_OK);
 *     the reference's functions cannot fail and its CLI exits on error, so the
 *     CLI in smvp-toolkit_amd/cli maps these codes onto the same messages.
 *   - indices are 32-bit `int`, values `double`, exactly like the reference
 *     (main-cli.c:42-47, 61-75).
 *   - inputs are never modified (the reference sorts the caller's COO array in
 *     place, main-cli.c:340,766) and outputs go to caller-owned buffers (the
 *     reference returns a malloc'd y it never frees, main-cli.c:370,468).
 *   - "d_" pointers are device (HBM) addresses, `stream` is a hipStream_t passed
 *     as void* (NULL = the null stream).  A handle belongs to one device; calls
 *     on different handles are independent, calls on one handle are not
 *     re-entrant.
 *   - there is no CPU fallback: compute entry points return
 *     SMVP_ERR_NO_DEVICE when no HIP device is usable.
 */
#ifndef SMVP_AMD_H
#define SMVP_AMD_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMVP_VERSION_MAJOR 0
#define SMVP_VERSION_MINOR 6
#define SMVP_VERSION_REVISION 4 /* report header keeps the reference's version string, main-cli.c:7-9,294 */

/* ------------------------------------------------------------------ status */
enum {
    SMVP_OK = 0,
    SMVP_ERR_INVALID = 1,     /* bad argument / inconsistent arrays */
    SMVP_ERR_NO_DEVICE = 2,   /* no usable HIP device: the product has no CPU path */
    SMVP_ERR_HIP = 3,         /* a HIP runtime call failed (see smvp_last_error) */
    SMVP_ERR_ALLOC = 4,
    SMVP_ERR_IO = 5,
    SMVP_ERR_UNSUPPORTED = 6,
    /* Matrix Market codes keep mmio's numbers (mmio/mmio.h:75-81) */
    SMVP_MM_COULD_NOT_READ_FILE = 11,
    SMVP_MM_PREMATURE_EOF = 12,
    SMVP_MM_NOT_MTX = 13,
    SMVP_MM_NO_HEADER = 14,
    SMVP_MM_UNSUPPORTED_TYPE = 15,
    SMVP_MM_LINE_TOO_LONG = 16,
    SMVP_MM_COULD_NOT_WRITE_FILE = 17
};
const char *smvp_last_error(void);     /* thread-local text of the last failure */
const char *smvp_version_string(void); /* "0.6.4" */
/* Plan options for experiments and tests (process-wide; read where a plan or handle is built or a file is parsed, never on a launch
 * path; value < 0 = back to the library's default).  What earlier rounds read from the environment -- the library reads no
 * environment variable any more:
 *   "csr_col16" 0: the CSR tile kernel keeps 32-bit columns           "csr_rowrel" 0: its second phase reads row_ptr
 *   "binned_near" 1: the binned plan's near part on the tile kernel   "binned_overlap" 0: pass A behind the near part, one stream
 *   "csr_sweep_alternate" 0: every product of the tile kernel sweeps its tiles forward; 1: a handle's plain launches alternate
 *                            forward / backward whatever the size (default: where one product's bytes exceed the Infinity Cache);
 *                            the results are the same bits either way
 *   "csr_read_once" 0 / 1: the plain CSR tile kernel's single launches never / always read val and the 16-bit column offsets
 *                            with the read-once (non-temporal) hint (default: where one product's bytes exceed 1 GiB); the same
 *                            bits either way
 *   "tjds_index" 0 | 1 | 2: 16-bit position words (default) / 32-bit sorted / 32-bit columns
 *   "sharded_threads" 1: the sharded layer's issuing threads with one GPU too     "mm_threads" n: the reader's threads (1 = serial)
 *   "trsv_chain_width" 256 | 512 | 1024: the widest level a triangular solve's chain takes (default 256), read by smvp_csr_trsv_create and
 *                      smvp_csr_ilu0_create
 *   "trsv_lanes_by_mean" 1: a wide level's lanes per row from the triangle's mean row length alone (default: mean and longest row)
 *   "color_max_blocks" n >= 1: the workgroups of one round of smvp_csr_color at the most (default 2048); the colours are the same
 * Unknown names are SMVP_ERR_INVALID. */
int smvp_set_option(const char *name, int value);
int smvp_get_option(const char *name, int *value); /* -1 = not set */

/* -------------------------------------------------------------------- types */
/* One stored entry, 0-based.  Replaces MMRawData, main-cli.c:42-47. */
typedef struct smvp_coo {
    int row;
    int col;
    double val;
} smvp_coo_t;

/* Replaces MM_typecode (mmio/mmio.h:17): [0]='M', [1]='C'oordinate|'A'rray,
 * [2]='R'eal|'C'omplex|'P'attern|'I'nteger, [3]='G'eneral|'S'ymmetric|'H'ermitian|s'K'ew. */
typedef char smvp_mm_typecode[4];

/* Replaces struct _time_data_ (main-cli.c:87-95) without the flexible array:
 * the per-iteration times go to a caller-owned double[iters]. */
typedef struct smvp_time_stats {
    double time_total, time_avg, time_stdev, time_min, time_max; /* milliseconds */
} smvp_time_stats_t;

/* ------------------------------------------------------ Matrix Market input */
/* Replace mm_read_banner (mmio/mmio.c:96) and mm_read_mtx_crd_size
 * (mmio/mmio.c:180): same accepted inputs, same return codes. */
int smvp_mm_read_banner(FILE *f, smvp_mm_typecode *matcode);
int smvp_mm_read_mtx_crd_size(FILE *f, int *rows, int *cols, int *nnz);
/* Replaces the entry loop in main(), main-cli.c:1426-1441: reads `nnz` entries
 * into caller-owned storage, 1-based -> 0-based, pattern files get val = 1,
 * symmetric storage is NOT mirrored.  A short file gives SMVP_MM_PREMATURE_EOF
 * (the reference would carry on with uninitialised entries). */
int smvp_mm_read_coo_entries(FILE *f, const smvp_mm_typecode matcode, int nnz, smvp_coo_t *out);
/* Convenience for non-C callers: open + banner + size (+ entries). */
int smvp_mm_read_header_path(const char *path, smvp_mm_typecode *matcode, int *rows, int *cols, int *nnz);
int smvp_mm_read_coo_path(const char *path, smvp_coo_t *out, int capacity,
                          smvp_mm_typecode *matcode, int *rows, int *cols, int *nnz);

/* Optional, NOT what the reference does (main-cli.c:1427-1441 multiplies the stored triangle of a symmetric file as it
 * stands, and so does everything here by default): mirror the off-diagonal entries of symmetric / hermitian (real) /
 * skew-symmetric storage so that the full matrix is multiplied.  General files are copied.  `out` may not alias `coo`. */
int smvp_mm_expanded_count(const smvp_mm_typecode matcode, const smvp_coo_t *coo, int nnz, int *count);
int smvp_mm_expand_symmetric(const smvp_mm_typecode matcode, const smvp_coo_t *coo, int nnz, int rows, int cols,
                             smvp_coo_t *out, int capacity, int *nnz_out);

/* Binary cache of a loaded matrix (new: the reference parses the text on every run): CSR arrays behind a header that
 * names the .mtx they were made from -- its size and the FNV-1a 64 of its bytes -- plus a checksum of the arrays.
 * flags bit 0 = symmetric storage was expanded.  smvp_cache_read_header fails with SMVP_ERR_IO when there is no
 * cache and with SMVP_ERR_INVALID when the file is not one, or was made from other bytes than mtx_path now holds. */
int smvp_cache_write_csr(const char *cache_path, const char *mtx_path, const smvp_mm_typecode matcode, int flags,
                         int rows, int cols, int nnz, const int *row_ptr, const int *col_ind, const double *val);
int smvp_cache_read_header(const char *cache_path, const char *mtx_path, smvp_mm_typecode *matcode, int *flags,
                           int *rows, int *cols, int *nnz);
int smvp_cache_read_csr(const char *cache_path, int rows, int nnz, int *row_ptr, int *col_ind, double *val);
int smvp_coo_from_csr(int rows, const int *row_ptr, const int *col_ind, const double *val, smvp_coo_t *out);

/* ------------------------------------------------------- format conversion */
/* Replaces the CSR build inside smvp_csr_compute, main-cli.c:340-365.
 * row_ptr[rows+1], col_ind[nnz], val[nnz]; entries ordered by (row, col) with
 * ties kept in input order.  Bit-identical to the reference's arrays whenever
 * the reference's are defined (no empty rows); empty rows get the standard
 * prefix-sum row_ptr. */
int smvp_csr_from_coo(const smvp_coo_t *coo, int rows, int nnz,
                      int *row_ptr, int *col_ind, double *val);
/* Replaces the TJDS build inside smvp_tjds_compute, main-cli.c:766-967.
 * perm[cols]: original column at permuted position k (columns by length
 * descending, ties by original index ascending, main-cli.c:209-223,868);
 * start_pos[*num_diag + 1] with the terminator start_pos[D] = nnz always
 * written (the reference omits it when the last diagonal has one entry,
 * main-cli.c:951-966); row_ind[nnz], val[nnz] in (diagonal, permuted column)
 * order.  start_pos_capacity must be >= D + 1 (rows + 1 always suffices when no
 * (row, col) pair repeats).  Optional outputs may be NULL:
 *   ref_num_tjdiag    the diagonal count the reference derives (main-cli.c:865:
 *                     length of ORIGINAL column 0) -- used by ref-quirks mode;
 *   last_diag_single  1 when the reference would leave the terminator unwritten. */
int smvp_tjds_from_coo(const smvp_coo_t *coo, int rows, int cols, int nnz,
                       int *perm, int *start_pos, int start_pos_capacity,
                       int *row_ind, double *val,
                       int *num_diag, int *ref_num_tjdiag, int *last_diag_single);

/* The same two conversions on the GPU (next row of SURVEY 8(f)): every pointer is a device
 * address, outputs are bit-identical to the host versions above.  Radix sort + scans instead of
 * the reference's qsorts and its O(nnz * cols) renumbering (main-cli.c:894-904).  Both return
 * after the work on `stream` has finished.  Like smvp_csr_create and smvp_tjds_create they take at
 * most 2^31 - 1 - 65536 = 2 147 418 111 entries (SMVP_ERR_UNSUPPORTED above, before any work). */
int smvp_csr_from_coo_device(const smvp_coo_t *d_coo, int rows, int cols, int nnz,
                             int *d_row_ptr, int *d_col_ind, double *d_val, void *stream);
int smvp_tjds_from_coo_device(const smvp_coo_t *d_coo, int rows, int cols, int nnz,
                              int *d_perm, int *d_start_pos, int start_pos_capacity,
                              int *d_row_ind, double *d_val,
                              int *num_diag, int *ref_num_tjdiag, int *last_diag_single, void *stream);

/* ---------------------------------------------------------- device / engine */
int smvp_device_count(int *count);
int smvp_device_info(int device, char *name, size_t name_cap, int *compute_units,
                     size_t *hbm_bytes);

/* CSR kernel families (smvp_csr_set_kernel).  AUTO picks STREAM; STREAM_PACKED instead where STREAM would run 2048-entry tiles
 * with 16-bit offsets, one product moves more than 1 GiB and at most 55 % of the values are not among the matrix's 64 most
 * frequent ones (counted exactly when the plan is built); STREAM_CARRY when some row is longer
 * than 16384 entries; COLSWEEP for a large matrix whose gathers scatter over an operand much larger than
 * the L2 (measured at create time on samples of col_ind: spread >= 0.6, rows long enough for the sweep's
 * window); BINNED for a large matrix of which a good share (>= 10 %) of the entries lies far from the
 * diagonal and scatters (spread >= 0.2) -- SURVEY 8(d)'s memplus-shaped random model.  Every family gives
 * the same result from run to run, bit for bit.
 * COLSWEEP, BINNED, STREAM_PACKED, the 16-bit column offsets of STREAM and the TJDS value cache keep (parts of) the entries a
 * second time, copied when the plan is built: a handle over adopted device arrays (SMVP_MEM_DEVICE) whose
 * val / col_ind are then changed in place must be re-planned (smvp_csr_set_kernel) or re-created.  (smvp_csr_spmm keeps no
 * second copy: its plan depends on row_ptr alone, and it reads val / col_ind themselves.)  A handle made by
 * smvp_csr_create_transposed is a second copy of all the entries: after such a change it is stale and must be created again.
 * Family by family, for val changed in place (tests/test_gpu_adopted.py holds every sentence):
 *   VECTOR, STREAM, STREAM_CARRY   read val itself: the next smvp_csr_spmv multiplies the new values, without any call (STREAM's
 *                                  second copy is of columns only);
 *   COLSWEEP, BINNED,              keep a copy of the values: call smvp_csr_set_kernel (the same kernel and param will do) first;
 *   STREAM_PACKED
 *   AUTO                           is one of the above: call smvp_csr_set_kernel(h, SMVP_CSR_KERNEL_AUTO, 0) unless
 *                                  smvp_csr_get_kernel names a family of the first line.
 * After col_ind changed in place call smvp_csr_set_kernel on every family (smvp_csr_spmm alone needs no call): the plan, its
 * describe() and its plan bytes are then those of a new handle over the same arrays, and AUTO chooses for the columns that are
 * there now (the gather spread and the far share are measured again).  A re-plan does not check the indices again: the caller
 * keeps changed columns inside [0, cols).  row_ptr may not be changed.  The arrays themselves are only ever read: every plan
 * builder, the ones that sort included, leaves them bit for bit as they were, smvp_csr_destroy frees none of them, and
 * several handles may share them. */
enum {
    SMVP_CSR_KERNEL_AUTO = 0,
    SMVP_CSR_KERNEL_VECTOR = 1,      /* one (sub-)wavefront per row, __shfl_down sums */
    SMVP_CSR_KERNEL_STREAM = 2,      /* fixed-nnz tiles, LDS-staged segmented reduction; a row is finished by
                                        the tile it starts in (one launch).  For the tiles whose columns span less than 65536 (if
                                        most are such) the plan keeps col_ind a second time as 16-bit offsets from the tile's
                                        smallest column and the product reads those (same sums, fewer bytes); it also keeps every
                                        row's first entry as a 16-bit offset from the first entry of the tile the row starts in,
                                        which the per-row sums read instead of row_ptr */
    SMVP_CSR_KERNEL_STREAM_CARRY = 3, /* same tiles; a row that crosses tiles is combined from per-tile carries
                                         by a second small launch (for matrices with extremely long rows) */
    SMVP_CSR_KERNEL_COLSWEEP = 4,     /* for columns scattered over an operand far larger than L2: strips of rows whose
                                         entries (kept a second time, sorted by column) are streamed so that all
                                         resident wavefronts gather from one L2-sized window of x; every row is
                                         summed in ascending order of the strip's stream, i.e. of the columns: for
                                         rows stored with ascending columns (what smvp_csr_from_coo and the reference
                                         build) bit-identical to main-cli.c:410-416; for a row whose col_ind is not
                                         ascending the sum is reproducible and within the rounding bound, but its
                                         order is not the serial loop's.  param: rows per workgroup of four strips
                                         (256 ... 20480, a multiple of 4; 0 = chosen from the block's rows: the height with the best share of busy CUs x rate,
                                         which may be the one that cuts the rows into whole generations of 256 workgroups).
                                         SMVP_CSR_SWEEP_PARTS(rb, parts), parts = 2 or 4 (rb * parts <= 20480): the workgroup's
                                         wavefronts share two strips / one strip, each taking a half / quarter of the columns
                                         into partial sums of its own -- strips 2x / 4x as tall for the same rows per workgroup,
                                         which is what a block of few rows (one rank's share of a sharded matrix) lacks; a row's
                                         sum is then its partial sums added part by part: the same from run to run, inside the
                                         rounding bound, NOT bit-identical to the serial loop.  parts = 8: one column part per XCD
                                         (workgroup b of a launch runs on XCD b % 8 and sweeps eighth b % 8 of the columns for
                                         the four whole strips of row group b / 8; the eight partial sums of a row meet in 8 *
                                         rows doubles of scratch and are added by a second kernel).  Never picked by AUTO */
    SMVP_CSR_KERNEL_BINNED = 5,       /* for matrices with a band around the diagonal plus many entries far from it
                                         (anywhere in an operand much larger than the L2): the entries are kept a second
                                         time, split by |column - row| > band.  The near part is summed out of a row
                                         block's window of x in LDS (rows of a block of 8192 sorted by length, every
                                         lane its own row left to right; a row of more than 16 near entries by a
                                         wavefront) -- or runs on STREAM where that does not suit (band > 4096, or a
                                         block with more than 1024 such long rows).  The far part never gathers from
                                         memory either: pass A -- one workgroup per block of 16384
                                         columns, that block of x in LDS -- stores every far product into bins ordered
                                         (row block, column block); pass B -- one workgroup per row block -- sums each
                                         row's far products in ascending column order and adds them to the near sum.
                                         No atomics.  Pass A runs beside the near part on a stream the handle owns
                                         (ordered against the caller's stream by events); a handle is therefore used by
                                         one stream at a time, like every plan that keeps buffers.  param: the band
                                         (0 = 4096) */
    SMVP_CSR_KERNEL_STREAM_PACKED = 6 /* STREAM at 2048-entry tiles with the values of the packable tiles -- the full tiles that read
                                         16-bit offsets -- kept a second time in packed form: one byte per entry that indexes a
                                         table of the matrix's 64 most frequent values (by bit pattern: -0.0 is not +0.0, a NaN
                                         keeps its payload), and the values that are not in the table wavefront by wavefront.  A
                                         product reads 1 + 2 + 8 * (share of such values) bytes per entry instead of 10; every
                                         value it multiplies is the double val held when the plan was built and every row is summed
                                         as STREAM sums it: y is bit-identical to STREAM's at 2048-entry tiles.  Wide tiles, the
                                         last, partial tile and the entries a tile reads past its end read val itself.  For
                                         circuit, stencil, graph and unit-weight matrices larger than the caches.  param: 0 or
                                         2048.  Refused (SMVP_ERR_UNSUPPORTED, the handle goes back to STREAM) where the 16-bit
                                         offsets are not in use.  The timed entry points run it as single stamped launches */
};
enum {
    SMVP_MEM_HOST = 0,  /* arrays are host memory: copied to the device */
    SMVP_MEM_DEVICE = 1 /* arrays are device memory: adopted, must outlive the handle */
};

typedef struct smvp_csr smvp_csr_t;   /* device-resident CSR matrix + launch plan */
typedef struct smvp_tjds smvp_tjds_t; /* device-resident TJDS matrix + launch plan */

/* Device-side half of smvp_csr_compute (main-cli.c:343-370): the three arrays
 * live in HBM, laid out exactly as CSRData (main-cli.c:61-66).  At most 2^31 - 1 - 65536 =
 * 2 147 418 111 entries (smvp_tjds_create too): more is SMVP_ERR_UNSUPPORTED.  row_ptr is
 * always read from the host copy as well to build the launch plan, so with
 * SMVP_MEM_DEVICE pass the host row_ptr in `host_row_ptr` (NULL = copy it back).
 * Adopted col_ind and val (SMVP_MEM_DEVICE) must be 16-byte aligned -- the tile kernels read them four and two at a time --
 * or the call is refused with SMVP_ERR_INVALID and *out is left alone; row_ptr needs no more than an int's alignment. */
int smvp_csr_create(smvp_csr_t **out, int device, int rows, int cols, int nnz,
                    const int *row_ptr, const int *col_ind, const double *val,
                    int mem_kind, const int *host_row_ptr);
/* The same handle for a ROW BLOCK [first_row, first_row + rows) of a larger matrix -- what one rank of a sharded product
 * holds (smvp_sharded.hip creates its chunks with it; new design, the reference is one thread): row_ptr is the block's own
 * (0-based), col_ind stays global.  Plans that go by the distance from the diagonal -- BINNED's near / far split and its
 * LDS windows of x, AUTO's far share -- then take the diagonal where it lies in the whole matrix: column first_row + r for
 * local row r.  (Without it every block beyond the first few thousand rows looks all far.)  The results are the same. */
int smvp_csr_create_block(smvp_csr_t **out, int device, int rows, int cols, int nnz,
                          const int *row_ptr, const int *col_ind, const double *val,
                          int mem_kind, const int *host_row_ptr, long long first_row);
int smvp_csr_set_kernel(smvp_csr_t *h, int kernel, int param); /* param: lanes per row (VECTOR) / nnz per tile (STREAM), 0 = default */
int smvp_csr_get_kernel(const smvp_csr_t *h, int *kernel, int *param);
/* What AUTO's choice of COLSWEEP rests on: the share (0 ... 1) of the matrix's gathers that pull their own
 * 128-byte line of x through the L2, estimated on 64 samples of 65536 consecutive entries of col_ind (measured
 * on first use, kept until the next smvp_csr_set_kernel); -1 for matrices of fewer than 4 M entries, which are not sampled. */
int smvp_csr_gather_spread(smvp_csr_t *h, double *spread);
/* What AUTO's choice of BINNED rests on besides the spread: the share (0 ... 1) of the entries further than 4096 from the
 * diagonal (of the whole matrix: smvp_csr_create_block); measured on first use, kept until the next smvp_csr_set_kernel; -1 where
 * it could not be. */
int smvp_csr_far_share(smvp_csr_t *h, double *share);
/* The timed product, main-cli.c:410-416: d_y[0..rows) = A * d_x[0..cols).  Asynchronous
 * on `stream`; d_y is fully overwritten (no pre-zeroing needed).
 * Values -- what every kernel family, parameter and plan option is held to (tests/test_gpu_special_values.py), the reference
 * being the serial loop  acc = 0.0; for j in row_ptr[r] .. row_ptr[r+1]: acc += val[j] * x[col_ind[j]]  with every product
 * rounded before the add (-ffp-contract=off):
 *   - An element of x influences exactly the rows that store an entry in its column: a NaN or an Inf in a column no entry
 *     uses changes no bit of y, wherever the column lies (padding, staged windows and column blocks never multiply it in).
 *   - Stored zeros are multiplied: a stored 0.0 or -0.0 under an infinite x makes its row NaN.
 *   - With non-finite products a row is what the serial loop gives: NaN if a product is NaN or the row has products of
 *     +Inf and of -Inf, else +Inf / -Inf if it has such a product; the other rows are finite and within the rounding
 *     bound of DESIGN.md, whatever the order a family sums in (as long as no sum of finite products overflows).
 *   - y never holds -0.0: the sum starts from +0.0, so a row of -0.0 products, an exact cancellation and an empty row are +0.0.
 *   - Subnormal values, products and sums are kept, not flushed.
 *   - The sign and payload of a NaN are unspecified.
 *   - The serial loop's very bits: COLSWEEP without column parts on rows stored with ascending columns, and STREAM on rows of
 *     up to 32 entries (STREAM_CARRY: where such a row lies inside one tile); see SMVP_CSR_KERNEL_*. */
int smvp_csr_spmv(smvp_csr_t *h, const double *d_x, double *d_y, void *stream);
/* Name of the dominant kernel symbol of the current plan and its algorithmic
 * byte count per launch: 12*nnz + 4*(rows+1) + 8*cols + 8*rows. */
int smvp_csr_describe(const smvp_csr_t *h, char *kernel_name, size_t cap, double *alg_bytes);
/* Kernel launches per product of the current plan: 1, except STREAM_CARRY (2: tiles + carry fix-up), COLSWEEP
 * (its workgroups start in generations that are resident together; config 4 on one GPU: 5) and BINNED (3: near part,
 * far products, far sums; one more where rows that keep their far entries near are summed apart). */
int smvp_csr_plan_launches(const smvp_csr_t *h, int *launches);
/* What the current launch plan costs (the reference has no counterpart: its set-up is the three qsorts and the
 * O(nnz * N) renumbering of main-cli.c:340,766-926, untimed): bytes of HBM the format's own arrays take, bytes the plan
 * keeps beside them (second copies included), and the host wall time the last plan build took, device work included. */
typedef struct smvp_plan_info {
    double matrix_bytes; /* CSR: 12 nnz + 4 (rows + 1); TJDS: 12 nnz + 4 (D + 1) + 4 cols */
    double plan_bytes;
    double build_ms;
} smvp_plan_info_t;
int smvp_csr_plan_info(const smvp_csr_t *h, smvp_plan_info_t *out);
/* k products that share one read of the matrix (new: the reference multiplies by one x, main-cli.c:410-416):
 *   d_Y[r*ldy + v] = sum_{j in row r} val[j] * d_X[col_ind[j]*ldx + v]     r < rows, v < k
 * X is cols x k and Y rows x k, both row-major doubles with leading dimensions ldx >= k, ldy >= k (a contiguous (n, k) array,
 * or a slice of columns of a wider one; column-major operands are not supported).
 *   - Bits: every Y(r, v) is bit for bit the serial loop on column v -- acc = 0.0; for j in row_ptr[r] .. row_ptr[r+1]:
 *     acc += val[j] * X(col_ind[j], v), each product rounded before the add -- for every row length, k, ldx, ldy, whatever
 *     SpMV plan the handle holds, on every stream and after any history of calls.  (Stronger than smvp_csr_spmv, whose
 *     default kernel keeps the serial order only on rows of up to 32 entries.)
 *   - Writes: Y(r, v) for v < k is overwritten (an empty row gets +0.0; no pre-zeroing); Y(r, v) for k <= v < ldy is never
 *     touched.
 *   - The matrix is read once per 16 vectors: ceil(k / 16) passes.
 *   - SMVP_ERR_INVALID, before anything is enqueued, for: a NULL handle; k < 1, ldx < k or ldy < k; a NULL d_X with nnz > 0
 *     or a NULL d_Y with rows > 0; byte ranges of X and Y that overlap; a capturing stream on a handle whose SpMM plan is not
 *     built yet (make one call outside the capture first, as for the SpMV plans).  SMVP_ERR_UNSUPPORTED for a handle that is
 *     not plain CSR.
 *   - Asynchronous on `stream`.  The first call on a handle builds the SpMM plan (one int per row, from row_ptr alone) and
 *     synchronises `stream`.  With adopted arrays (SMVP_MEM_DEVICE), val / col_ind changed in place are seen by the next call
 *     without a re-plan. */
int smvp_csr_spmm(smvp_csr_t *h, int k, const double *d_X, long long ldx, double *d_Y, long long ldy, void *stream);
/* The kernel symbols of a product with k vectors (one per pass), its algorithmic bytes 12 nnz + 4 (rows + 1) + 8 k (cols + rows)
 * (SURVEY 8(d) with k operands, whatever the number of passes), and in `plan` (may be NULL) the SpMM plan's bytes and build
 * time -- zero until the first smvp_csr_spmm.  smvp_csr_plan_info keeps describing the SpMV plan only. */
int smvp_csr_spmm_describe(const smvp_csr_t *h, int k, char *kernel_name, size_t cap, double *alg_bytes, smvp_plan_info_t *plan);
/* ------------------------------------------------------------ transposed product */
/* y = A^T x (new: the reference multiplies by A only).  For an M x N matrix, x of M doubles, y of N doubles:
 *     y[c] = acc,  acc = 0.0;  for every stored entry (r, c) of column c, in ascending r, entries with equal (r, c) in storage
 *                              order:  acc += val * x[r]      (each product rounded before the add, -ffp-contract=off)
 * i.e. the serial loop of main-cli.c:410-416 run over the CSR arrays of A^T as smvp_csr_from_coo builds them from the entries
 * with row and column swapped.  A column without entries gets +0.0; y is fully overwritten (no pre-zeroing).  "Storage order" is
 * the TJDS position for a TJDS handle and the CSR position for a CSR handle; for arrays built by this library's converters from
 * one COO list the two are the same order, and both routes below give the same bits.
 *
 * Route 1, smvp_csr_create_transposed: A^T as an ordinary CSR handle, built on the device.  *out is a new, independent plain-CSR
 * handle of the N x M matrix A^T on h's device: it owns its three arrays, holds a host copy of its row_ptr, starts on AUTO and
 * outlives h; everything a CSR handle offers works on it (smvp_csr_spmv, smvp_csr_set_kernel, smvp_csr_spmm, ...).  Its rows
 * have ascending columns (= ascending rows of A), ties in h's storage order: bit for bit smvp_csr_from_coo of the swapped
 * entries, whatever order h's col_ind has inside a row.  The entries are written as a COO list (16 B per entry), sorted by
 * smvp_csr_from_coo_device and adopted; the list and the sort's buffers are freed before the call returns, and it returns after
 * the work on `stream` has finished.  A row block (smvp_csr_create_block) is accepted: the result is a whole-matrix handle
 * whose columns are the block's local rows.  SMVP_ERR_INVALID for a NULL handle / out or a capturing stream (nothing is
 * enqueued; the capture stays valid); SMVP_ERR_UNSUPPORTED for a handle that is not plain CSR; SMVP_ERR_ALLOC when memory runs
 * out (nothing leaked).  *out is NULL after every failure.  It is a second copy in the sense of the note at SMVP_CSR_KERNEL_*:
 * after val / col_ind of adopted arrays (SMVP_MEM_DEVICE) are changed in place, the transposed handle is stale -- create it again. */
int smvp_csr_create_transposed(smvp_csr_t **out, const smvp_csr_t *h, void *stream);
/* The device addresses a plain-CSR handle multiplies from (its own copies, or the adopted arrays), valid until the handle is
 * destroyed; NULL outputs are skipped.  SMVP_ERR_UNSUPPORTED for a handle that is not plain CSR. */
int smvp_csr_device_arrays(const smvp_csr_t *h, const int **d_row_ptr, const int **d_col_ind, const double **d_val);
void smvp_csr_destroy(smvp_csr_t *h);

/* Device-side half of smvp_tjds_compute (main-cli.c:756-763,944-967): val,
 * row_ind, start_pos as TJDSData (main-cli.c:70-75) plus perm.  Adopted arrays (SMVP_MEM_DEVICE) need no alignment beyond
 * their element's own (8 bytes for val, 4 for the others): unlike smvp_csr_create there is no 16-byte rule and no refusal,
 * in any mode and in the transposed products -- every kernel reads them one element at a time. */
int smvp_tjds_create(smvp_tjds_t **out, int device, int rows, int cols, int nnz, int num_diag,
                     const int *perm, const int *start_pos, const int *row_ind,
                     const double *val, int mem_kind);
/* Replaces the operand permutation main-cli.c:907-923: x_perm[k] = x[perm[k]],
 * kept inside the handle.  Call again whenever x changes. */
int smvp_tjds_set_x(smvp_tjds_t *h, const double *d_x, void *stream);
/* The timed product, main-cli.c:1013-1020, in its corrected form
 * y[row_ind[j]] += val[j] * x_perm[j - start_pos[d]].  In the default mode (ROW_GATHER) and in TWO_PHASE d_y is
 * overwritten; in ATOMIC mode (and ref-quirks mode) d_y must be zero on entry -- the reference
 * zeroes it outside its timed window, main-cli.c:1008 -- and smvp_tjds_zero_y does that on the
 * same stream (it is a no-op when the mode does not need it, so it is always safe to call).
 * Values: as stated at smvp_csr_spmv, in every mode and stream form, with and without the value cache -- an element of x
 * (an element of x_perm, a lane past a diagonal's end, a slot of the run tables) influences exactly the rows that store an
 * entry in its column; stored zeros are multiplied; a row's class under non-finite products is the serial loop's; y never
 * holds -0.0; subnormals are kept (by the fp64 hardware atomic add of ATOMIC mode too); the sign and payload of a NaN are
 * unspecified.  ROW_GATHER and TWO_PHASE give the same bits from run to run; ATOMIC adds in the order the hardware takes
 * the atomics, so its finite rows are only within the rounding bound -- exact where every order gives the same sum.
 * Adopted arrays (SMVP_MEM_DEVICE) whose val is changed in place: ATOMIC and TWO_PHASE read val itself, so the next
 * smvp_tjds_spmv multiplies the new values without any call; ROW_GATHER keeps copies (the value cache, and with or without it
 * the values a tile reads past its end) and needs smvp_tjds_set_value_cache or re-creation first, see there. */
int smvp_tjds_zero_y(smvp_tjds_t *h, double *d_y, void *stream);
int smvp_tjds_spmv(smvp_tjds_t *h, double *d_y, void *stream);
/* How the scatter is carried out.
 * ROW_GATHER (default): ONE kernel per product.  At create time the entries are regrouped by row (val / row_ind /
 *   start_pos / perm are only read); every tile of 2048 entries lists its entries in TJDS order and walks its piece of
 *   the jagged diagonals the way the format stores them, the products meet in LDS and one lane (or wave) per row sums
 *   them in ascending TJDS position -- no atomics, bit-reproducible, y needs no zeroing.
 * TWO_PHASE: products stored once per entry (column-major kernel: thread k walks down permuted column k with x_perm[k] in a
 *   register), then summed per row by the one-kernel form's tile kernel reading the products where that reads val (no value
 *   cache, no operand) -- same order of summation, same bits, two launches and 16 B per entry more traffic.
 * ATOMIC: one column-major pass, fp64 atomic adds into a zeroed y (order varies from run to run).  Ref-quirks mode
 *   always runs this form.
 * The plans of the first two are built on the device the first time the mode is selected. */
enum {
    SMVP_TJDS_MODE_AUTO = 0,               /* = ROW_GATHER */
    SMVP_TJDS_MODE_ATOMIC = 1,
    SMVP_TJDS_MODE_TWO_PHASE = 2,
    SMVP_TJDS_MODE_ROW_GATHER = 3
};
int smvp_tjds_set_mode(smvp_tjds_t *h, int mode);
int smvp_tjds_set_tile(smvp_tjds_t *h, int entries_per_tile); /* ROW_GATHER: 256, 1024 or 2048 entries per workgroup (re-plans) */
/* ROW_GATHER's value cache.  Far down the jagged diagonals only the long columns are left: neighbours in val are
 * entries of unrelated rows, and a 128-byte line of val would be pulled through the L2 once for each of them.  The plan
 * therefore keeps a second copy of the values of every val line whose 16 entries belong to `min_tiles` or more
 * different tiles (default 2: every line that is not one tile's alone -- 56 % of the values of memplus x944, 21 % of pwt
 * x459; 4 until round 4), stored tile by tile and read coalesced; all other values are read from val itself.
 * 0 = no cache (every value from val).  The sums and their order do not depend on it.  A handle over adopted device
 * arrays (SMVP_MEM_DEVICE) must be re-created, or this called again, after val has been changed in place: with the same
 * min_tiles is enough, and with 0 it is needed as well (the values a tile reads past its end are a copy with or without the
 * cache). */
int smvp_tjds_set_value_cache(smvp_tjds_t *h, int min_tiles);
int smvp_tjds_get_value_cache(const smvp_tjds_t *h, int *min_tiles, long long *cached_entries);
/* Reference-defect emulation for parity with the committed TJDS reports
 * (diagonal count from original column 0, missing terminator, operand indexed
 * by row: main-cli.c:865,951-966,1018).  A host-side edit of the launch plan of the atomic kernel. */
int smvp_tjds_set_ref_quirks(smvp_tjds_t *h, int enable, int ref_num_tjdiag, int last_diag_single);
int smvp_tjds_describe(const smvp_tjds_t *h, char *kernel_name, size_t cap, double *alg_bytes);
int smvp_tjds_plan_info(const smvp_tjds_t *h, smvp_plan_info_t *out); /* plan: x_perm, the work items, the selected modes' plans */
/* Route 2 of the transposed product (definition above smvp_csr_create_transposed), kernel K8: d_y[0..cols) = A^T * d_x[0..rows)
 * from the handle's own val / row_ind / start_pos / perm -- TJDS stores A by columns, so permuted column k is a row of A^T and
 * one lane sums it from top to bottom.  No second copy (val of adopted arrays changed in place is seen by the next call, and
 * by smvp_tjds_spmm_transposed's), no plan, no atomics; asynchronous on `stream` and capturable into a
 * hipGraph from the first call.  Every y[c] is the definition's bits for every column length, the same on every run.  It reads
 * neither the permuted operand of smvp_tjds_set_x nor any mode's plan: the result does not depend on smvp_tjds_set_mode /
 * set_tile / set_value_cache / set_ref_quirks, and a forward smvp_tjds_spmv after it gives the bits it gave before it without
 * a new smvp_tjds_set_x.  A column is walked by one lane however long it is (as smvp_csr_spmm walks a row).
 * SMVP_ERR_INVALID, before anything is enqueued, for: a NULL handle; a NULL d_x with nnz > 0; a NULL d_y with cols > 0; byte
 * ranges of x and y that overlap. */
int smvp_tjds_spmv_transposed(smvp_tjds_t *h, const double *d_x, double *d_y, void *stream);
/* Its kernel symbol and algorithmic bytes 12 nnz + 4 (D + 1) + 4 cols + 8 rows + 8 cols (SURVEY 8(d)'s TJDS figure with x and y
 * changing places, plus perm, which this product reads once where the forward one reads the permuted operand). */
int smvp_tjds_transposed_describe(const smvp_tjds_t *h, char *kernel_name, size_t cap, double *alg_bytes);
/* The block form of route 2, kernel K9: d_Y[c*ldy + v] = (A^T X)(c, v) for c < cols, v < k, from the handle's own val / row_ind /
 * start_pos / perm.  For an M x N matrix X is M x k and Y is N x k, both row-major doubles with leading dimensions ldx >= k,
 * ldy >= k: the operand conventions of smvp_csr_spmm with the rows and columns of A changing places (a contiguous (n, k) array,
 * or a slice of columns of a wider one; column-major operands are not supported).
 *   - Bits: every Y(c, v) is bit for bit the transposed-product definition above smvp_csr_create_transposed applied to column v
 *     of X -- acc = 0.0; for the stored entries of column c in ascending row, ties in TJDS storage order: acc += val * X(r, v),
 *     each product rounded before the add (-ffp-contract=off) -- for every column length, k, ldx and ldy, on every stream, the
 *     same on every run.  For k = 1, ldx = ldy = 1 these are the bits of smvp_tjds_spmv_transposed.
 *   - Writes: Y(c, v) for v < k is overwritten (no pre-zeroing); a column without entries gets +0.0; Y(c, v) for k <= v < ldy is
 *     never touched; Y never holds -0.0.
 *   - Values: as stated at smvp_csr_spmv -- an element of X influences exactly the outputs whose column stores an entry in its
 *     row (a lane whose column has ended leaves its product out with a select and never multiplies by 0); stored zeros are
 *     multiplied; subnormals are kept.
 *   - State: no plan and no second copy.  The call reads nothing of smvp_tjds_set_x, the modes' plans, the value cache or the
 *     ref-quirks edit, so its result does not depend on them; it is capturable into a hipGraph from the first call on a fresh
 *     handle; a forward smvp_tjds_spmv after it gives the bits it gave before, without a new smvp_tjds_set_x.
 *   - The matrix is read once per 16 vectors: ceil(k / 16) passes.
 *   - SMVP_ERR_INVALID, before anything is enqueued, for: a NULL handle; k < 1, ldx < k or ldy < k; a NULL d_X with nnz > 0 or
 *     a NULL d_Y with cols > 0; byte ranges of X ((rows - 1) ldx + k doubles) and Y ((cols - 1) ldy + k doubles) that overlap.
 *   - Asynchronous on `stream`. */
int smvp_tjds_spmm_transposed(smvp_tjds_t *h, int k, const double *d_X, long long ldx, double *d_Y, long long ldy, void *stream);
/* The kernel symbols of a product with k vectors (one per pass, joined by " + ") and its algorithmic bytes
 * 12 nnz + 4 (D + 1) + 4 cols + 8 k (rows + cols): smvp_tjds_transposed_describe's figure with k operands, whatever the number
 * of passes.  (The leading dimensions are not known here: for k = 1 the symbol is the one-lane pass's; a call with k = 1 and
 * ldx = ldy = 1 runs smvp_tjds_spmv_transposed's kernel, which gives the same bits.) */
int smvp_tjds_spmm_transposed_describe(const smvp_tjds_t *h, int k, char *kernel_name, size_t cap, double *alg_bytes);
/* The forward block product from a TJDS handle, kernel K10: d_Y[r*ldy + v] = (A X)(r, v) for r < rows, v < k.  For an M x N
 * matrix X is N x k and Y is M x k, both row-major doubles with leading dimensions ldx >= k, ldy >= k: the operand conventions of
 * smvp_csr_spmm (a contiguous (n, k) array, or a slice of columns of a wider one; column-major operands are not supported).
 *   - Bits: Y(r, v) = acc, where acc = 0.0 and then, for the stored positions j with row_ind[j] == r in ascending TJDS position
 *     j: acc += val[j] * X(perm[j - start_pos[d(j)]], v), d(j) being the jagged diagonal that holds j and each product rounded
 *     before the add (-ffp-contract=off) -- the corrected product of main-cli.c:1013-1020 run serially on column v of X.  It
 *     holds for every row length, k, ldx and ldy, on every stream, the same bits on every run.  It is the order of summation
 *     smvp_tjds_spmv documents for ROW_GATHER and TWO_PHASE, kept serially on rows of every length; bit equality with
 *     smvp_tjds_spmv itself is not promised (its tile kernel keeps the serial order only on short rows).
 *   - Writes: Y(r, v) for v < k is overwritten (no pre-zeroing); a row without entries gets +0.0; Y(r, v) for k <= v < ldy is
 *     never touched; Y never holds -0.0.
 *   - Values: as stated at smvp_csr_spmv -- an element of X influences exactly the rows that store an entry in its column (a slot
 *     past a row's end is left out with a select and never multiplied by 0); stored zeros are multiplied; subnormals are kept.
 *   - State: the call reads nothing of smvp_tjds_set_x's operand, any mode's plan, the value cache or the ref-quirks edit, so its
 *     result does not depend on smvp_tjds_set_mode / set_tile / set_value_cache / set_ref_quirks; a forward smvp_tjds_spmv after
 *     it gives the bits it gave before it, without a new smvp_tjds_set_x.
 *   - Plan: the first call on a handle builds the SpMM plan on the device and synchronises `stream`; later calls are
 *     asynchronous on `stream`.  The plan is the entries regrouped by row: ptr[rows + 1]; pos[nnz], the TJDS positions, ascending
 *     inside a row; col[nnz], the original column perm[pos - start_pos[d]]; and smvp_csr_spmm's one int per row (rows longest
 *     first inside blocks of 4096 rows, stable) -- 4 (rows + 1) + 8 nnz + 4 rows bytes in buffers of its own, shared with no
 *     mode's plan and freed by smvp_tjds_destroy.  smvp_tjds_plan_info does not count it: its bytes and build time come out of
 *     smvp_tjds_spmm_describe.  val is read through pos, not copied: with adopted arrays (SMVP_MEM_DEVICE) val changed in place is
 *     seen by the next call without any other call; row_ind, start_pos and perm may not be changed.
 *   - The matrix is read once per 16 vectors: ceil(k / 16) passes.
 *   - SMVP_ERR_INVALID, before anything is enqueued, for: a NULL handle; k < 1, ldx < k or ldy < k; a NULL d_X with nnz > 0 or
 *     a NULL d_Y with rows > 0; byte ranges of X ((cols - 1) ldx + k doubles) and Y ((rows - 1) ldy + k doubles) that overlap; a
 *     capturing stream on a handle whose SpMM plan is not built yet (the capture stays valid and nothing is written: make one
 *     call outside the capture first). */
int smvp_tjds_spmm(smvp_tjds_t *h, int k, const double *d_X, long long ldx, double *d_Y, long long ldy, void *stream);
/* The kernel symbols of a product with k vectors (one per pass, joined by " + ", cut at `cap`), its algorithmic bytes
 * 12 nnz + 4 (D + 1) + 4 cols + 8 k (rows + cols) whatever the number of passes, and in `plan` (may be NULL) the SpMM plan's bytes
 * 4 (rows + 1) + 8 nnz + 4 rows and build time -- zero until the first smvp_tjds_spmm, as for smvp_csr_spmm_describe.
 * SMVP_ERR_INVALID for a NULL handle or k < 1, with the outputs untouched. */
int smvp_tjds_spmm_describe(const smvp_tjds_t *h, int k, char *kernel_name, size_t cap, double *alg_bytes, smvp_plan_info_t *plan);
void smvp_tjds_destroy(smvp_tjds_t *h);

/* -------------------------------------------------------------- the power method */
/* The scaled (max-norm) power method on a handle the caller already holds, kernel K11 (new: the reference only multiplies; the
 * comment at main-cli.c:401 names power iteration as the product the assignment asked for).  It is smvp_run_opts_t's iterate +
 * normalize loop with an eigenvalue estimate, a residual and a stop rule, run on the device.  Everything below is defined through
 * maxima, a selection by index and correctly rounded IEEE operations, so every number has one right answer whatever order the
 * device reduces in.
 *
 * For a square n x n handle, step k = 1, 2, ... has the operand x_{k-1}; x_0 is the caller's start vector, or all ones.
 *   absmax(v)    m = the largest |v_r| over the r whose v_r is not NaN, 0.0 if there is none; p = the SMALLEST r with |v_r| == m
 *                among those, -1 if there is none.
 *   y_k          the handle's own product of x_{k-1}: bit for bit what smvp_csr_spmv (current plan) or smvp_tjds_set_x +
 *                smvp_tjds_spmv (current mode) gives for that operand.
 *   p_{k-1}      the index of absmax(x_{k-1}).
 *   lambda_k     y_k[p_{k-1}] / x_{k-1}[p_{k-1}], the correctly rounded quotient; NaN when p_{k-1} = -1.
 *   res_k        the largest |y_k[r] - lambda_k * x_{k-1}[r]| over the r where that value is not NaN, 0.0 if there is none.  The
 *                product is rounded, then the difference is rounded: no FMA (-ffp-contract=off, as everywhere in the library).
 *   (m_k, p_k)   absmax(y_k).
 *   x_k          y_k / m_k if m_k > 0, else y_k unchanged: the rule of smvp_run_opts_t.normalize, true IEEE division.  x_k is
 *                therefore bit for bit the k-th iterate of the iterate + normalize path on the same plan.
 * Looked steps are the k with k % check_every == 0, and k == max_steps.  Only at a looked step is a stop rule evaluated; the
 * first that holds, in this order, is the `reason`:
 *   1. SMVP_POWER_NONFINITE   lambda_k is NaN or +-Inf;
 *   2. SMVP_POWER_ZERO        not (m_k > 0): the iterate vanished;
 *   3. SMVP_POWER_CONVERGED   res_k <= (tol * |lambda_k|) * |x_{k-1}[p_{k-1}]|, evaluated in doubles in that order (tol = 0 stops
 *                             early only on a residual of exactly 0);
 *   4. SMVP_POWER_MAX_STEPS   k == max_steps.
 * The reason belongs to the step the run stopped at: with check_every > 1 an iterate that vanished or went NaN at a step nobody
 * looked at simply carries on (a zero iterate stays zero, a NaN spreads: the next looked step sees it).
 * On every path whose product is the same from run to run -- every CSR family, TJDS ROW_GATHER and TWO_PHASE -- every reported
 * number and every bit of x_k is a pure function of the handle's single products (tests/power_method.py restates it in numpy;
 * tests/test_gpu_power_method.py holds the library to those bits).  The sign and payload of a NaN are unspecified. */
enum { SMVP_POWER_CONVERGED = 0, SMVP_POWER_MAX_STEPS = 1, SMVP_POWER_ZERO = 2, SMVP_POWER_NONFINITE = 3 };
typedef struct smvp_power_opts {
    unsigned struct_size; /* set by smvp_power_opts_default, checked as for smvp_run_opts_t */
    int max_steps;        /* >= 1; default 100 */
    int check_every;      /* >= 1; default 1 */
    double tol;           /* >= 0, finite; default 0 */
} smvp_power_opts_t;
void smvp_power_opts_default(smvp_power_opts_t *o);
typedef struct smvp_power_result {
    int steps;         /* products done */
    int reason;        /* SMVP_POWER_* */
    int index;         /* p_{steps-1}: where lambda was read */
    double eigenvalue; /* lambda_steps */
    double residual;   /* res_steps */
    double scale;      /* m_steps */
} smvp_power_result_t;
/*   - d_x0: n doubles, NULL = all ones.  d_x: n doubles, receives x_steps; it may be the same pointer as d_x0 (any other overlap
 *     is SMVP_ERR_INVALID) and is written once, at the step the run stops at.
 *   - lambda_each / residual_each: caller-owned HOST arrays of max_steps doubles, or NULL.  Filled for the steps done, the steps
 *     nobody looked at included (from a device-side history copied back once at the end); left untouched beyond them.
 *   - The call returns after the work on `stream` has finished.  It allocates its workspace per call -- two vectors, the reduce
 *     pass's partials, the history, a status block -- and frees it on every way out.  Between looked steps nothing synchronises
 *     with the host; at a looked step the host reads the status block (48 bytes) and nothing else.  Beside the product a step is
 *     three launches and four passes over a vector (x and y read, y read, x written), one pass more than the normalisation of
 *     iterate + normalize: the residual's.
 *   - SMVP_ERR_INVALID for: a NULL handle, opts or result (a NULL handle before any HIP call); a struct_size that is not this
 *     library's; max_steps < 1, check_every < 1, tol negative, NaN or infinite; rows != cols; a NULL d_x with n > 0; a capturing
 *     stream.  Nothing is enqueued then, d_x and *result are left untouched, and a capturing stream's capture stays valid.
 *   - SMVP_ERR_UNSUPPORTED (likewise) for a CSR handle that is not plain CSR, and for a TJDS handle in ATOMIC mode or with
 *     ref-quirks on: the one is not reproducible, the other no product of a changing operand (iterate refuses it too).
 *   - n == 0: SMVP_OK, steps 0, reason SMVP_POWER_ZERO, index -1, eigenvalue NaN, residual and scale 0.
 *   - State: a CSR handle's plan is untouched -- smvp_csr_spmv after the call gives the bits it gave before.  A TJDS handle's
 *     permuted operand is afterwards that of the last operand, x_{steps-1}: call smvp_tjds_set_x again before the next
 *     smvp_tjds_spmv, as after any change of x.  A handle is used by one stream at a time, as ever. */
int smvp_csr_power_method(smvp_csr_t *h, const smvp_power_opts_t *opts, const double *d_x0, double *d_x,
                          smvp_power_result_t *result, double *lambda_each, double *residual_each, void *stream);
int smvp_tjds_power_method(smvp_tjds_t *h, const smvp_power_opts_t *opts, const double *d_x0, double *d_x,
                           smvp_power_result_t *result, double *lambda_each, double *residual_each, void *stream);

/* ------------------------------------------------- conjugate gradients and the dot product */
/* A x = b for a symmetric positive definite A on a handle the caller already holds, kernel K12 (new: the reference only
 * multiplies).  Conjugate gradients need sums, and a sum has one right answer only once its order of additions is fixed.  So the
 * order is part of this contract: with it, every number below is again a pure function of the handle's single products.
 *
 * dot(a, b) for n doubles.  B = 256 lanes per workgroup, G = min(ceil(n / 256), 2048) workgroups.
 *   terms      t_i = a_i * b_i, rounded.  No FMA anywhere (-ffp-contract=off, as everywhere in the library).
 *   lanes      lane l of workgroup g owns slot s = 256 g + l.  Its accumulator starts at +0.0 and adds t_s, t_{s + 256 G},
 *              t_{s + 2 * 256 G}, ... in ascending order (a slot beyond n - 1 adds nothing).
 *   fold256    of a workgroup's 256 accumulators c_0 .. c_255: inside each of the four wavefronts (64 consecutive lanes), for
 *              h = 32, 16, 8, 4, 2, 1: c_j <- c_j + c_{j+h} for j < h; then ((w0 + w1) + w2) + w3 over the four wavefronts'
 *              c_0.
 *   partials   workgroup g's partial is fold256 of its accumulators.
 *   result     fold256 of a second level, in which lane l starts at +0.0 and adds the partials l, l + 256, l + 512, ... in
 *              ascending order.
 *   n = 0      gives +0.0.
 * An accumulator that starts at +0.0 never becomes -0.0, so adding +0.0 terms is the same as not adding: a restatement may pad
 * (tests/cg_method.py is one, in numpy; tests/test_gpu_cg.py holds the library to its bits).
 *
 * smvp_vector_dot gives that dot of two device vectors in the HOST double `result`.  It allocates its partials, returns after the
 * work on `stream` has finished and refuses a capturing stream.  SMVP_ERR_INVALID for n < 0, a NULL d_a or d_b with n > 0, a NULL
 * result. */
int smvp_vector_dot(int device, int n, const double *d_a, const double *d_b, double *result, void *stream);

/* Plain conjugate gradients on a square n x n handle.  `dot` is the one above; every other operation is one correctly rounded
 * IEEE operation per element (alpha * p_i is rounded, then the sum is rounded).
 *   bb    = dot(b, b)            thr = (tol * tol) * bb   (tol * tol rounded on the host, the product on the device)
 *   x_0   = d_x0, or zeros if NULL
 *   r_0   = b - A x_0            (d_x0 == NULL: r_0 = b bit for bit, no product is run)
 *   p_0   = r_0                  rho_0 = dot(r_0, r_0)
 *   step 0 rule:   NONFINITE if bb or rho_0 is NaN or +-Inf;  CONVERGED if rho_0 <= thr
 *   step k = 1, 2, ...:
 *     q_k     = A p_{k-1}        the handle's own product, bit for bit: smvp_csr_spmv (current plan), or smvp_tjds_set_x +
 *                                smvp_tjds_spmv (current mode)
 *     sigma_k = dot(p_{k-1}, q_k)
 *     rule A:   NONFINITE if sigma_k is NaN or +-Inf;  BREAKDOWN if not (sigma_k > 0)      -> x stays x_{k-1}, updates = k - 1
 *     alpha_k = rho_{k-1} / sigma_k
 *     x_k = x_{k-1} + alpha_k * p_{k-1}        r_k = r_{k-1} - alpha_k * q_k
 *     rho_k   = dot(r_k, r_k)
 *     rule B:   NONFINITE if rho_k is NaN or +-Inf;  CONVERGED if rho_k <= thr;  MAX_STEPS if k == max_steps
 *                                                                                         -> x = x_k, updates = k
 *     beta_k  = rho_k / rho_{k-1}              p_k = r_k + beta_k * p_{k-1}
 * No square root is taken: the histories and the result hold squared norms.
 * The device evaluates the rules at EVERY step; the first that holds, in the order written, is the `reason`, and from then on
 * nothing is written to x or to the histories.  The host reads a status block at looked steps only -- step 0, every k with
 * k % check_every == 0, and k == max_steps -- and only to leave the loop: steps, updates, reason, both histories and every bit of
 * d_x do not depend on check_every (which decides how many products are enqueued in vain, and how often the host waits).  This is
 * stronger than the power method's "the reason belongs to the looked step": a converged x is never iterated past.
 * Symmetry and definiteness are the caller's contract and are not checked; SMVP_CG_BREAKDOWN is what a matrix that is visibly
 * not positive definite gets (smvp_csr_bicgstab below is for a general matrix).  A diagonal preconditioner: smvp_csr_pcg below.
 * k right-hand sides in one call, sharing every read of the matrix: smvp_csr_cg_multi (K20) below.  The sharded handles are out of
 * scope. */
enum { SMVP_CG_CONVERGED = 0, SMVP_CG_MAX_STEPS = 1, SMVP_CG_BREAKDOWN = 2, SMVP_CG_NONFINITE = 3 };
typedef struct smvp_cg_opts {
    unsigned struct_size; /* set by smvp_cg_opts_default, checked as for smvp_run_opts_t */
    int max_steps;        /* >= 1; default 100 */
    int check_every;      /* >= 1; default 10 */
    double tol;           /* >= 0, finite; default 1e-10: stop at |r| <= tol |b| */
} smvp_cg_opts_t;
void smvp_cg_opts_default(smvp_cg_opts_t *o);
typedef struct smvp_cg_result {
    int steps;   /* products of a direction done (the one for r_0 is not counted) */
    int updates; /* updates of x done: steps, or steps - 1 after rule A */
    int reason;  /* SMVP_CG_* */
    int pad;
    double rr;   /* rho_updates */
    double bb;   /* dot(b, b) */
} smvp_cg_result_t;
/*   - d_b: n doubles.  d_x0: n doubles, NULL = zeros.  d_x: n doubles; the iterates live in it, and it holds x_updates afterwards.
 *     d_x may be the same pointer as d_x0; any other overlap of the two, and any overlap of d_b and d_x, is SMVP_ERR_INVALID.
 *     After SMVP_ERR_HIP the content of d_x is unspecified.
 *   - rr_each: a caller-owned HOST array of max_steps + 1 doubles, filled 0 .. updates with rho.  sigma_each: max_steps doubles,
 *     filled 0 .. steps - 1 with sigma_1 .. sigma_steps.  Either may be NULL.  Both come from a device-side history copied back
 *     once at the end, and are left untouched beyond the filled elements.
 *   - The call returns after the work on `stream` has finished.  It allocates its workspace per call -- three vectors, the
 *     partials of two dots, the histories, two status blocks -- and frees it on every way out.  Beside the product a step is three
 *     launches and ten passes over a vector (p, q read; q, r read, r written; x, p, r read, x, p written).
 *   - SMVP_ERR_INVALID for: a NULL handle, opts, result or d_b (before any HIP call); a struct_size that is not this library's;
 *     max_steps < 1, check_every < 1, tol negative, NaN or infinite; rows != cols; a NULL d_x with n > 0; the overlaps above; a
 *     capturing stream.  Nothing is enqueued then, d_x and *result are left untouched, and a capturing stream's capture stays valid.
 *   - SMVP_ERR_UNSUPPORTED (likewise) for a CSR handle that is not plain CSR, and for a TJDS handle in ATOMIC mode or with
 *     ref-quirks on, as for the power method.
 *   - n == 0: SMVP_OK, steps 0, updates 0, reason SMVP_CG_CONVERGED, rr = bb = +0.0.
 *   - State: a CSR handle's plan is untouched -- smvp_csr_spmv after the call gives the bits it gave before.  A TJDS handle's
 *     permuted operand is afterwards that of the last direction multiplied: call smvp_tjds_set_x again before the next
 *     smvp_tjds_spmv, as after any change of x.  A handle is used by one stream at a time, as ever. */
int smvp_csr_cg(smvp_csr_t *h, const smvp_cg_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                smvp_cg_result_t *result, double *rr_each, double *sigma_each, void *stream);
int smvp_tjds_cg(smvp_tjds_t *h, const smvp_cg_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                 smvp_cg_result_t *result, double *rr_each, double *sigma_each, void *stream);

/* ------------------------------------------------- the diagonal of a handle */
/* d_diag[i], i = 0 .. rows - 1, from the handle's own arrays, kernel K14 (new: the reference only ever multiplies).  Every one of
 * the `rows` doubles is written.  Element i starts at +0.0 and adds every stored entry (i, i) in ascending storage position: for
 * CSR the position inside the row (columns need not be sorted: the whole row is examined), for TJDS the TJDS position inside the
 * column.  So an absent diagonal reads +0.0, a lone stored -0.0 reads +0.0 (as smvp_csr_spmv's y never holds -0.0), and repeated
 * diagonal entries add up in storage order; both formats give the same bits for the same entries in the same order.  An element
 * i >= cols is +0.0.  On a handle of smvp_csr_create_block the diagonal of local row r lies at global column first_row + r.
 *   - Asynchronous on `stream`.  The calls neither allocate nor synchronise, need no plan and no smvp_tjds_set_x, can be captured
 *     from the first call on, and leave the handle's state alone: a product afterwards gives the bits it gave before.
 *   - `val` is read in place: adopted values changed in place are seen by the next call.
 *   - No atomics: the same bits on every run.  Only the index array is streamed; `val` is read at the matches.
 *   - SMVP_ERR_INVALID for a NULL handle, and for a NULL d_diag with rows > 0; SMVP_ERR_UNSUPPORTED for a smvp_csr_t that is not
 *     plain CSR (the inner handles of a TJDS matrix), as for the solvers.  Nothing is enqueued then. */
int smvp_csr_diagonal(const smvp_csr_t *h, double *d_diag, void *stream);
int smvp_tjds_diagonal(const smvp_tjds_t *h, double *d_diag, void *stream);

/* ------------------------------------------------- conjugate gradients with a diagonal preconditioner */
/* Conjugate gradients on a square n x n handle, preconditioned with M = diag(d_m), kernel K14.  d_m holds n doubles: usually what
 * smvp_csr_diagonal / smvp_tjds_diagonal gave (Jacobi), but any positive vector is accepted.  Options, `dot` and the reason codes
 * are K12's, unchanged: smvp_cg_opts_t, the dot above, SMVP_CG_*.  Every other operation is one correctly rounded IEEE operation per
 * element (alpha * p_i is rounded, then the sum is rounded); z_i = r_i / m_i is an IEEE double division -- no reciprocal is taken,
 * no FMA is used.
 *   bb    = dot(b, b)            thr = (tol * tol) * bb   (tol * tol rounded on the host, the product on the device)
 *   x_0   = d_x0, or zeros if NULL
 *   r_0   = b - A x_0            (d_x0 == NULL: r_0 = b bit for bit, no product is run)
 *   z_0   = r_0 ./ m             p_0 = z_0
 *   rr_0  = dot(r_0, r_0)        rho_0 = dot(r_0, z_0)
 *   step 0 rule:   NONFINITE if bb, rr_0 or rho_0 is NaN or +-Inf;  CONVERGED if rr_0 <= thr;  BREAKDOWN if not (rho_0 > 0)
 *   step k = 1, 2, ...:
 *     q_k     = A p_{k-1}        the handle's own product, bit for bit: smvp_csr_spmv (current plan), or smvp_tjds_set_x +
 *                                smvp_tjds_spmv (current mode)
 *     sigma_k = dot(p_{k-1}, q_k)
 *     rule A:   NONFINITE if sigma_k is NaN or +-Inf;  BREAKDOWN if not (sigma_k > 0)      -> x stays x_{k-1}, updates = k - 1
 *     alpha_k = rho_{k-1} / sigma_k
 *     x_k = x_{k-1} + alpha_k * p_{k-1}        r_k = r_{k-1} - alpha_k * q_k        z_k = r_k ./ m
 *     rr_k    = dot(r_k, r_k)                  rho_k = dot(r_k, z_k)
 *     rule B:   NONFINITE if rr_k or rho_k is NaN or +-Inf;  CONVERGED if rr_k <= thr;  BREAKDOWN if not (rho_k > 0);
 *               MAX_STEPS if k == max_steps                                               -> x = x_k, updates = k
 *     beta_k  = rho_k / rho_{k-1}              p_k = z_k + beta_k * p_{k-1}
 * No square root is taken: the histories and the result hold squared norms.
 * The stop rule looks at the residual's own norm rr, not at rho = r.z: smvp_csr_cg can be swapped for smvp_csr_pcg under the same
 * tol.  d_m is not validated: a zero or negative element shows up as NONFINITE or BREAKDOWN under the rules above (step 0's
 * BREAKDOWN is what an M that is visibly not positive definite gets).  With d_m all ones every number is smvp_csr_cg's, bit for bit.
 * The device evaluates the rules at EVERY step; the first that holds, in the order written, is the `reason`, and from then on
 * nothing is written to x or to the histories.  The host reads a status block at looked steps only -- step 0, every k with
 * k % check_every == 0, and k == max_steps -- and only to leave the loop: steps, updates, reason, the three histories and every bit
 * of d_x do not depend on check_every.  A preconditioner made of two triangular solves (symmetric Gauss-Seidel, an incomplete
 * factorisation: the caller's, or K17's ILU(0)) is smvp_csr_pcg_tri, K16, below.  Preconditioned BiCGSTAB is smvp_csr_pbicgstab, K18,
 * further below.  k right-hand sides under one d_m in one call: smvp_csr_cg_multi (K20), below.  The sharded handles are out of
 * scope. */
typedef struct smvp_pcg_result {
    int steps;   /* products of a direction done (the one for r_0 is not counted) */
    int updates; /* updates of x done: steps, or steps - 1 after rule A */
    int reason;  /* SMVP_CG_* */
    int pad;
    double rr;   /* rr_updates: the squared residual norm that belongs to d_x */
    double rz;   /* rho_updates = dot(r, z), likewise */
    double bb;   /* dot(b, b) */
} smvp_pcg_result_t;
/*   - d_b, d_m: n doubles each.  d_x0: n doubles, NULL = zeros.  d_x: n doubles; the iterates live in it, and it holds x_updates
 *     afterwards.  d_x may be the same pointer as d_x0; any other overlap of the two, and any overlap of d_x with d_b or d_m, is
 *     SMVP_ERR_INVALID.  d_b and d_m are only read.  After SMVP_ERR_HIP the content of d_x is unspecified.
 *   - rr_each, rz_each: caller-owned HOST arrays of max_steps + 1 doubles, filled 0 .. updates with rr and rho.  sigma_each:
 *     max_steps doubles, filled 0 .. steps - 1 with sigma_1 .. sigma_steps.  Any of the three may be NULL.  They come from a
 *     device-side history copied back once at the end, and are left untouched beyond the filled elements.
 *   - The call returns after the work on `stream` has finished.  It allocates its workspace per call -- three vectors (z is never
 *     stored: r_i / m_i is divided again where it is needed, the same bits), the partials of three dots, the histories, two status
 *     blocks -- and frees it on every way out.  Beside the product a step is three launches and twelve passes over a vector (p, q
 *     read; q, r, m read, r written; x, p, r, m read, x, p written): K12's ten and two reads of m.
 *   - SMVP_ERR_INVALID for: a NULL handle, opts, result, d_b or d_m (before any HIP call); a struct_size that is not this library's;
 *     max_steps < 1, check_every < 1, tol negative, NaN or infinite; rows != cols; a NULL d_x with n > 0; the overlaps above; a
 *     capturing stream.  Nothing is enqueued then, d_x and *result are left untouched, and a capturing stream's capture stays valid.
 *   - SMVP_ERR_UNSUPPORTED (likewise) for a CSR handle that is not plain CSR, and for a TJDS handle in ATOMIC mode or with
 *     ref-quirks on, as for the power method.
 *   - n == 0: SMVP_OK, steps 0, updates 0, reason SMVP_CG_CONVERGED, rr = rz = bb = +0.0.
 *   - State: as after smvp_csr_cg / smvp_tjds_cg -- a CSR handle's plan is untouched; a TJDS handle's permuted operand is afterwards
 *     that of the last direction multiplied: call smvp_tjds_set_x again before the next smvp_tjds_spmv. */
int smvp_csr_pcg(smvp_csr_t *h, const smvp_cg_opts_t *opts, const double *d_b, const double *d_x0, double *d_x, const double *d_m,
                 smvp_pcg_result_t *result, double *rr_each, double *rz_each, double *sigma_each, void *stream);
int smvp_tjds_pcg(smvp_tjds_t *h, const smvp_cg_opts_t *opts, const double *d_b, const double *d_x0, double *d_x, const double *d_m,
                  smvp_pcg_result_t *result, double *rr_each, double *rz_each, double *sigma_each, void *stream);

/* ------------------------------------------------- conjugate gradients for k right-hand sides */
/* k independent conjugate-gradient runs on one square n x n handle that share every read of the matrix and every launch, kernel
 * K20: the loop around the block products smvp_csr_spmm (K7) and smvp_tjds_spmm (K10).  It is NOT block CG: the columns share no
 * Krylov space, so every number of a column still has one right answer.  One entry point covers plain CG (d_m == NULL: K12's rules)
 * and a diagonal preconditioner (d_m given: K14's rules; n doubles shared by all columns).
 *
 * Operands.  B, X0 and X are n x k row-major device blocks with leading dimensions of their own, each >= k: smvp_csr_spmm's
 * conventions -- a contiguous (n, k) array, or a column slice of a wider one.  Element (i, v) of B lies at d_B[i * ldb + v].  Padding
 * columns of X are never written.  d_X0 == NULL is zeros (ldx0 is then ignored).  d_X may be d_X0 with ldx == ldx0; any other
 * overlap of the byte ranges of d_X0 and d_X, and any overlap of d_X with d_B or d_m, is SMVP_ERR_INVALID.  d_B, d_X0 and d_m are
 * only read.  After SMVP_ERR_HIP the content of d_X is unspecified.
 *
 * Bits.  Column v of every output is the run this header already defines: with d_m == NULL the smvp_csr_cg run on b = B(:, v),
 * x_0 = X0(:, v), with d_m given the smvp_csr_pcg run on the same operands -- the same dot, the same order of additions, the same
 * rules in the same order, every rule evaluated on the device at every step -- with ONE difference: q_k is column v of
 * smvp_csr_spmm / smvp_tjds_spmm on the k directions, i.e. the serial loop over the row for CSR and the row's entries in ascending
 * TJDS position for TJDS.  It does not depend on the handle's SpMV plan or TJDS mode.  No number of column v depends on k, on v, on
 * the other columns' contents (a NaN column included), on any leading dimension, on check_every or on the stream.  Where the
 * handle's single product is itself the serial loop on every row -- the default kernel on rows of at most 32 entries, see
 * smvp_csr_spmm's "Bits" -- every number equals the one-vector call's, bit for bit.
 *
 * Columns stop on their own.  Each column has its own status block and its own steps / updates / reason.  Once a column's rule has
 * fired nothing is written to that column of X or to its histories.  The host loop ends when all columns have stopped; until then
 * a stopped column is still multiplied (in vain) by the block product, which cannot disturb the others because the block product's
 * columns are independent.  Stopped columns are not compacted away.
 *   - results: a HOST array of k blocks; results[v] is column v's smvp_pcg_result_t as smvp_csr_pcg fills it.  With d_m == NULL
 *     rz = rr.
 *   - rr_each, rz_each: caller-owned HOST arrays of k * (max_steps + 1) doubles; column v's history is contiguous at
 *     [v * (max_steps + 1) + j], filled j = 0 .. updates_v.  sigma_each: k * max_steps doubles, column v at [v * max_steps + j],
 *     filled j = 0 .. steps_v - 1.  Everything beyond the filled elements is left untouched.  Any of the three may be NULL, and
 *     rz_each is left untouched when d_m is NULL.  They come from device-side histories copied back once at the end.
 *   - The host reads the k status blocks at looked steps only -- step 0, every step that is a multiple of check_every, and
 *     max_steps -- and only to leave the loop.
 *   - The call returns after the work on `stream` has finished.  It allocates its workspace per call -- R, P and Q (n x k, ld = k),
 *     the partials of three dots per column (at most 2048 each), a few words per column, the histories, 2 x k status blocks -- and
 *     frees it on every way out.  Beside the block product (one launch per 16 columns) a step is two launches of one workgroup per
 *     column and three passes per group of at most 16 columns: 10 k passes over a vector (12 k with d_m), as k runs of K12 / K14.
 *   - SMVP_ERR_INVALID for everything smvp_csr_cg / smvp_csr_pcg refuse (a NULL d_m excepted: it selects plain CG), and for: k < 1;
 *     a leading dimension below k; a NULL results; a capturing stream.  Nothing is enqueued then, d_X and results are left
 *     untouched, and a capturing stream's capture stays valid.
 *   - SMVP_ERR_UNSUPPORTED (likewise) for a CSR handle that is not plain CSR.  A TJDS handle is accepted in EVERY mode, ATOMIC and
 *     ref-quirks included: smvp_tjds_spmm's bits depend on neither.
 *   - n == 0: SMVP_OK, and every results[v] has steps 0, updates 0, reason SMVP_CG_CONVERGED, rr = rz = bb = +0.0.
 *   - State: a CSR handle's SpMV plan is untouched -- smvp_csr_spmv after the call gives the bits it gave before.  The first call
 *     builds the handle's block-product plan if it has none, as the first smvp_csr_spmm / smvp_tjds_spmm would (4 bytes per row; for
 *     TJDS 8 bytes per entry and 8 per row), and keeps it.  A TJDS handle's permuted operand and forward state are untouched, as
 *     smvp_tjds_spmm promises: unlike after smvp_tjds_cg, a smvp_tjds_spmv after the call needs no new smvp_tjds_set_x.  `val` is
 *     read in place: adopted values changed in place are seen by the next call.
 * Out of scope: true block CG, compaction of stopped columns, the triangular-solve preconditioners of K16 (K15 has no solve for k
 * vectors), BiCGSTAB and GMRES for k right-hand sides, the sharded handles, column-major operands. */
int smvp_csr_cg_multi(smvp_csr_t *h, const smvp_cg_opts_t *opts, int k, const double *d_B, long long ldb, const double *d_X0,
                      long long ldx0, double *d_X, long long ldx, const double *d_m, smvp_pcg_result_t *results, double *rr_each,
                      double *rz_each, double *sigma_each, void *stream);
int smvp_tjds_cg_multi(smvp_tjds_t *h, const smvp_cg_opts_t *opts, int k, const double *d_B, long long ldb, const double *d_X0,
                       long long ldx0, double *d_X, long long ldx, const double *d_m, smvp_pcg_result_t *results, double *rr_each,
                       double *rz_each, double *sigma_each, void *stream);

/* ------------------------------------------------- sparse triangular solves */
/* T x = b where T is a triangle of a square plain-CSR handle's matrix AS STORED, kernel K15 (new: the reference only multiplies).
 * The operation under a Gauss-Seidel or SOR sweep, symmetric Gauss-Seidel / SSOR preconditioning and the application of an
 * incomplete factorisation the caller brings.  Entries of the other triangle are skipped, not refused: a sweep on a full A needs
 * no extracted copy.  Rows are taken in ascending order (LOWER) or descending order (UPPER):
 *   s_i = +0.0;  d_i = +0.0
 *   for every stored entry p of row i in ascending storage position (columns need not be sorted, repeats allowed):
 *     c = col_ind[p]
 *     c == i                          : d_i = d_i + val[p]            (smvp_csr_diagonal's rule; skipped, val not read, for DIAG_UNIT)
 *     c <  i (LOWER) / c > i (UPPER)  : s_i = s_i + val[p] * x[c]     (the product rounded, then the sum rounded: no FMA, as everywhere)
 *     otherwise                       : skipped
 *   x_i = (b_i - s_i) / d_i     (DIAG_STORED: one IEEE subtraction, one IEEE division, no reciprocal)
 *   x_i =  b_i - s_i            (DIAG_UNIT)
 * d_i is not validated: a missing or zero diagonal gives +-Inf or NaN by the rules above, as d_m does in smvp_csr_pcg.  How a row's
 * entries are loaded is the library's business (a lane per row, or a group of lanes); the order of the additions is the one written,
 * so every element of x has one right answer, the serial substitution loop's, the same on every run.
 *
 * Levels.  level(i) = 0 if row i has no stored off-diagonal entry inside the triangle, else 1 + the largest level(c) over those
 * entries.  Levels are structural: an explicitly stored 0.0 counts.  The schedule's `order` lists the rows by (level, row index)
 * ascending, for both uplo; level_ptr (levels + 1 elements) delimits the levels in it.  Rows of one level do not depend on each
 * other.  A level of more than chain_width rows is one launch over its rows; a maximal run of consecutive levels of at most
 * chain_width rows each (a chain) is one launch of one workgroup with a workgroup barrier between its levels, so
 * launches = wide levels + chains.  No kernel waits on a value another workgroup writes in the same launch -- no flags, no grid
 * barrier, no atomics: the order between workgroups comes from the kernel boundaries on the stream alone.
 *
 * Out of scope: TJDS handles (the format stores by columns: it needs a column-oriented solve), sharded handles, a block of k
 * right-hand sides, the transposed solve T^T x = b (for a symmetric matrix stored in full the other uplo serves) and an analysis
 * on the device.  The solver that uses two plans as a preconditioner is smvp_csr_pcg_tri / smvp_tjds_pcg_tri, K16, below; the
 * incomplete factorisation that gives it two triangles on one handle is smvp_csr_ilu0_create, K17, below that. */
enum { SMVP_TRSV_LOWER = 0, SMVP_TRSV_UPPER = 1 };
enum { SMVP_TRSV_DIAG_STORED = 0, SMVP_TRSV_DIAG_UNIT = 1 };
typedef struct smvp_trsv smvp_trsv_t; /* a plan: borrows the handle's arrays, owns level_ptr / order on the device (a sweeps plan,
                                         K21 below: the rows' storage ranges and two scratch vectors) */
typedef struct smvp_trsv_info {
    unsigned struct_size;  /* set by the caller to sizeof(smvp_trsv_info_t) before the call; another size is SMVP_ERR_INVALID */
    int levels;
    int max_level_width;   /* rows of the widest level */
    int launches;          /* kernels one solve enqueues: wide levels + chains */
    int chains;
    int chain_width;       /* a level of at most so many rows joins a chain: the library's constant, 256, unless the plan option
                              "trsv_chain_width" said otherwise when the plan was made */
    int missing_diagonals; /* rows with no stored (i, i): reported for both diag settings */
    int lanes_per_row;     /* lanes a row of a wide level gets (from the triangle's mean and longest row) */
    long long entries;     /* stored entries one solve reads: the triangle's off-diagonals, plus the diagonal matches for DIAG_STORED */
    double plan_bytes;     /* device memory the plan owns: level_ptr and order */
    double build_ms;       /* host wall time of smvp_csr_trsv_create: copies back, analysis, counting sort, upload */
} smvp_trsv_info_t;
/*   - smvp_csr_trsv_create: the level recurrence is sequential, so the analysis runs on the HOST in one O(nnz) pass: row_ptr is the
 *     handle's host copy, col_ind comes back from the device once (the handle keeps no host copy of it, adopted or uploaded); then a
 *     counting sort by level and one upload of level_ptr and order.  build_ms reports the cost.  The call waits for `stream`,
 *     allocates, and refuses a capturing stream.  The plan holds pointers into the handle's row_ptr / col_ind / val and copies no
 *     matrix data: the handle must outlive it.  `val` changed in place is seen by the next solve; a changed STRUCTURE needs a new
 *     plan.  Any number of plans per handle (lower and upper together is the normal case).  The handle's own state and plans are
 *     untouched: a product afterwards gives the bits it gave before.
 *   - smvp_trsv_solve: d_b and d_x are n doubles on the handle's device.  Asynchronous on `stream`; allocates nothing, synchronises
 *     nothing and can be captured from the first call on: the graph is a plain chain of kernels with no parallel branches.  d_x ==
 *     d_b (exactly the same pointer) is allowed -- row i reads b_i before it writes x_i; any other overlap is SMVP_ERR_INVALID.
 *     Every one of the n doubles of d_x is written, and nothing else.  A plan is used by one stream at a time.
 *   - smvp_trsv_schedule: level_ptr (levels + 1 ints) and order (n ints) into caller-owned HOST arrays; either may be NULL.
 *   - SMVP_ERR_INVALID (nothing enqueued, outputs untouched, smvp_last_error names the argument): a NULL out, h, t, or a NULL d_b /
 *     d_x with n > 0; uplo / diag out of range; rows != cols; the partial overlap above; a capturing stream at create.
 *     SMVP_ERR_UNSUPPORTED: a handle that is not plain CSR (as for smvp_csr_diagonal), and a row block (first_row != 0).
 *   - n == 0: everything succeeds with levels 0, launches 0.
 *   - smvp_csr_trsv_levels is the analysis itself on HOST arrays, no device touched: level_of_row (rows ints) and *levels.
 *     SMVP_ERR_INVALID for uplo out of range, rows < 0, a NULL row_ptr / level_of_row with rows > 0, a NULL col_ind with entries, a
 *     NULL levels, a row_ptr that is not a non-decreasing sequence from 0, a column outside [0, rows); the outputs are untouched. */
int smvp_csr_trsv_create(smvp_trsv_t **out, const smvp_csr_t *h, int uplo, int diag, void *stream);
int smvp_trsv_solve(smvp_trsv_t *t, const double *d_b, double *d_x, void *stream);
int smvp_trsv_info(const smvp_trsv_t *t, smvp_trsv_info_t *out);
int smvp_trsv_schedule(const smvp_trsv_t *t, int *level_ptr, int *order);
void smvp_trsv_destroy(smvp_trsv_t *t);
int smvp_csr_trsv_levels(int rows, const int *row_ptr, const int *col_ind, int uplo, int *level_of_row, int *levels);

/* ------------------------------------------------- Jacobi sweeps on a triangular system, as a plan */
/* A fixed number of Jacobi sweeps on T x = b instead of the exact solve, kernel K21 (new: the reference only multiplies).  A
 * preconditioner is an approximation anyway (Anzt, Chow, Dongarra: iterative sparse triangular solves for preconditioning), and a
 * sweep is one fully parallel pass over the triangle: a solve is sweeps + 1 launches whatever the number of levels.  The result of
 * smvp_csr_trsv_create_sweeps is an ordinary smvp_trsv_t: smvp_trsv_solve, _info, _schedule, _destroy and every solver that takes
 * plans (K16, K18, K19) accept it as they stand.
 *
 * The per-row rule is K15's: d_i is the sum from +0.0 of the stored (i, i) in ascending storage position (not read for DIAG_UNIT);
 * s_i(x) the sum from +0.0 of val[p] * x[c] over the stored entries inside the triangle in ascending storage position, the product
 * rounded, then the sum, no FMA; the other triangle is skipped.  The solve is
 *   x(0)_i   = (b_i - (+0.0)) / d_i            (DIAG_UNIT: b_i - (+0.0), which is b_i, a signed zero included)
 *   x(m+1)_i = (b_i - s_i(x(m))) / d_i         (DIAG_UNIT: b_i - s_i(x(m))),   m = 0 .. sweeps - 1
 *   x = x(sweeps)
 * Every sweep reads only the previous iterate, never an element written by the same launch: every element of every iterate has
 * one right answer, whatever the order between workgroups.  Consequences:
 *   - sweeps = 0 is a division by the diagonal.
 *   - x(m)_i equals the exact solve's x_i, bit for bit, for every row of level <= m (a row of level l reads rows of levels < l
 *     only, by the same rule in the same order).  So sweeps >= levels - 1 gives smvp_trsv_solve's result on a plan of
 *     smvp_csr_trsv_create, bit for bit; smvp_trsv_info's `levels` says which count is exact.
 *   - For a symmetric A the LOWER and UPPER plans with the same `sweeps` and m = diagonal() give a symmetric positive definite
 *     M^-1 = P^T D P (P = sum of the first sweeps + 1 powers of -D^-1 L, applied to D^-1), and so do the LOWER / UNIT and
 *     UPPER / STORED plans of its ILU(0): smvp_*_pcg_tri stays valid.  Unequal sweep counts are the caller's risk, as M's
 *     symmetry always was.
 *   - A missing or zero diagonal gives +-Inf or NaN by the same rules, unvalidated.
 *   - Where a row's off-diagonals inside the triangle outweigh its diagonal, intermediate iterates grow before nilpotency brings
 *     them back.  Nothing about that is validated.
 *
 *   - smvp_csr_trsv_create_sweeps makes smvp_csr_trsv_create's checks and refusals (plain CSR, square, no row block, no capturing
 *     stream) and runs the same host analysis: levels, missing_diagonals, max_level_width and smvp_trsv_schedule mean what they
 *     mean for an exact plan.  From col_ind it computes one storage range [begin_i, end_i) per row, the smallest that holds all of
 *     the row's entries inside the triangle and (DIAG_STORED) on the diagonal; a sweep walks only that range, which adds the same
 *     values in the same order as a walk of the row, everything outside being of the skipped kind.  Rows with ascending columns
 *     get a tight range (a sweep then reads half of a full matrix's col_ind); unsorted rows a loose one that is still right.
 *     The plan owns begin and end (n ints each) and two scratch vectors of n doubles between which a solve's iterates alternate;
 *     it borrows row_ptr / col_ind / val as K15's plans do: `val` changed in place is seen by the next solve, a changed
 *     structure needs a new plan.  0 <= sweeps <= SMVP_TRSV_MAX_SWEEPS, anything else is SMVP_ERR_INVALID.
 *   - smvp_trsv_solve on such a plan: launch 0 writes x(0) reading only b; launch m reads b and the scratch vector launch m - 1
 *     wrote; the last launch writes d_x, which is never read, so d_x == d_b works as before.  Nothing depends on what the scratch
 *     vectors held.  It allocates nothing, synchronises nothing, and is capturable from the plan's first call: a plain chain of
 *     kernels.  A plan is used by one stream at a time (two solves in flight would share the scratch vectors).
 *   - smvp_trsv_info on such a plan: launches = sweeps + 1 (0 for n = 0); chains = 0 and chain_width = 0; lanes_per_row as used
 *     (K15's rule on the ranges' mean and longest length); entries = the stored entries inside the ranges, which one sweep reads
 *     (launch 0 reads val on the diagonal only, and nothing at all for DIAG_UNIT); plan_bytes = the bytes of the four buffers.
 *   - smvp_trsv_sweeps: *sweeps = the plan's count, -1 for a plan of smvp_csr_trsv_create.  A NULL t or sweeps is SMVP_ERR_INVALID.
 * Out of scope: TJDS and sharded handles, k right-hand sides, a sweep count chosen by the library, a residual-based stop inside a
 * solve, a compacted copy of the triangle, asynchronous sweeps that read the iterate they write, block-Jacobi variants. */
enum { SMVP_TRSV_MAX_SWEEPS = 4096 };
int smvp_csr_trsv_create_sweeps(smvp_trsv_t **out, const smvp_csr_t *h, int uplo, int diag, int sweeps, void *stream);
int smvp_trsv_sweeps(const smvp_trsv_t *t, int *sweeps);   /* -1 for a plan of smvp_csr_trsv_create */

/* ------------------------------------------------- conjugate gradients preconditioned by two triangular solves */
/* Conjugate gradients on a square n x n handle's own product, preconditioned with M = T1 diag(m)^-1 T2, kernel K16 (new: the
 * reference only multiplies).  `first` and `second` are plans of smvp_csr_trsv_create; z = M^-1 r is
 *   w   = T1^-1 r      smvp_trsv_solve(first, r, z): K15's bits
 *   v_i = m_i * w_i    one rounded multiplication; skipped entirely when d_m == NULL
 *   z   = T2^-1 v      smvp_trsv_solve(second, z, z): in place
 * The plans are the caller's and may belong to ANY plain-CSR handle of n rows on the handle's device; the product may be a CSR or a
 * TJDS handle's.
 *   - Symmetric Gauss-Seidel on A itself: first = LOWER / DIAG_STORED on A, d_m = smvp_csr_diagonal of A, second = UPPER /
 *     DIAG_STORED on A: M = (D + L) D^-1 (D + U).  The solves skip the other triangle: no extracted copy is needed.
 *   - An incomplete factorisation A ~ F F^T the caller brings: first = LOWER / DIAG_STORED on a handle of F, second = UPPER /
 *     DIAG_STORED on smvp_csr_create_transposed of it, d_m = NULL.
 *   - An ILU(0) the library computes (smvp_csr_ilu0_create, K17, below): first = LOWER / DIAG_UNIT and second = UPPER /
 *     DIAG_STORED, both on the factorisation's one handle, d_m = NULL.  No transposed copy is needed.
 *   - SSOR with omega != 1 needs a handle whose diagonal is scaled by 1 / omega (and d_m to match): building it is the caller's
 *     business.
 * Everything else is smvp_csr_pcg's word for word with z = M^-1 r in place of r ./ m: smvp_cg_opts_t, SMVP_CG_*, smvp_pcg_result_t
 * (rr, rz, bb), the dot above, step 0 and its rule, rule A, rule B in its order (NONFINITE if rr_k or rho_k is NaN or +-Inf;
 * CONVERGED if rr_k <= thr; BREAKDOWN if not (rho_k > 0); MAX_STEPS), the stop rule on rr and not on rho, alpha * p_i rounded before
 * the sum, no FMA.  The device evaluates the rules at EVERY step, nothing is written to d_x or to the histories once one has
 * fired, and no result depends on check_every.
 * M's symmetry and definiteness are the caller's contract; nothing is validated.  A zero diagonal in a triangle shows as NONFINITE,
 * an M that is visibly not positive definite as BREAKDOWN.  With first = LOWER / DIAG_STORED and second = UPPER / DIAG_UNIT on a
 * handle that stores only a diagonal d, and d_m = NULL, every number is smvp_csr_pcg's with m = d, bit for bit: z_i = (r_i - s_i) /
 * d_i with s_i = +0.0, and r_i - (+0.0) is r_i, a signed zero included.
 *   - Operands, histories and n == 0 as for smvp_csr_pcg; d_x may be d_x0.  d_m, where given, is n doubles, only read, and must
 *     not overlap d_x.
 *   - The call returns after the work on `stream` has finished.  It allocates its workspace per call -- four vectors (r, p, q and
 *     z: z cannot be re-derived element by element, so it is stored), the partials of three dots, the histories, two status blocks
 *     -- and frees it on every way out.  Beside the product and the two solves' launches a step is five launches (four without
 *     d_m) and fifteen passes over a vector (p, q read; q, r read, r written; z, m read, z written; r, z read; x, p, z read, x, p
 *     written).  No kernel waits on a value another workgroup writes.
 *   - SMVP_ERR_INVALID for everything smvp_csr_pcg refuses (a NULL d_m excepted), and for: a NULL first or second; a plan whose row
 *     count is not n or whose device is not the handle's; d_m overlapping d_x; a capturing stream.  SMVP_ERR_UNSUPPORTED as for
 *     smvp_csr_pcg.  Nothing is enqueued then, d_x and *result are left untouched, and a capturing stream's capture stays valid.
 *     first == second is allowed.
 *   - State: the handle as after smvp_csr_pcg / smvp_tjds_pcg.  The plans are used on `stream` for the duration of the call (a
 *     plan is used by one stream at a time, as ever) and are unchanged afterwards, as are the handles they borrow: smvp_trsv_solve
 *     gives the bits it gave before.  `val` of either handle changed in place is seen by the next call.
 * Out of scope: omega inside the library, the sharded handles, a block of k right-hand sides (smvp_csr_cg_multi, K20, takes a
 * diagonal preconditioner only: K15 has no solve for k vectors).  BiCGSTAB preconditioned by the same
 * M, for a matrix that is not symmetric, is smvp_csr_pbicgstab, K18, below. */
int smvp_csr_pcg_tri(smvp_csr_t *h, const smvp_cg_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                     smvp_trsv_t *first, const double *d_m, smvp_trsv_t *second, smvp_pcg_result_t *result, double *rr_each,
                     double *rz_each, double *sigma_each, void *stream);
int smvp_tjds_pcg_tri(smvp_tjds_t *h, const smvp_cg_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                      smvp_trsv_t *first, const double *d_m, smvp_trsv_t *second, smvp_pcg_result_t *result, double *rr_each,
                      double *rz_each, double *sigma_each, void *stream);

/* ------------------------------------------------- incomplete LU factorisation, ILU(0) */
/* A ~ L U on A's own pattern, computed on the device from a plain-CSR handle, kernel K17 (new: the reference only multiplies): the
 * preconditioner K15 and K16 were built for.  The factor F lives in ONE CSR array on A's row_ptr / col_ind: strictly below the
 * diagonal L, its unit diagonal implied; on and above the diagonal U.  K15 solves with a triangle of a matrix as stored, stored or
 * unit diagonal, the other triangle skipped -- so a LOWER / DIAG_UNIT plan and an UPPER / DIAG_STORED plan on F's one handle ARE
 * M = L U for smvp_csr_pcg_tri / smvp_tjds_pcg_tri with d_m = NULL.
 * The handle must be plain CSR with first_row == 0 and rows == cols; every row's col_ind must be STRICTLY ASCENDING (sorted, no
 * repeated column) and every row must store (i, i).  diag_pos[i] is the position of (i, i).  F has values of its own:
 *   for i = 0 .. n-1, in this order:
 *     w[p] = val_A[p]                                       for every position p of row i
 *     for p ascending over row i while col_ind[p] < i:      (the pivots k = col_ind[p], ascending)
 *       w[p] = w[p] / F[diag_pos[k]]                        one IEEE division by the FINAL u_kk; no reciprocal
 *       for every position q of row k with col_ind[q] > k:  (q = diag_pos[k] + 1 .. row_ptr[k+1] - 1, final values of row k)
 *         if row i stores column col_ind[q], at position t (then t > p):
 *           w[t] = w[t] - w[p] * F[q]                       the product rounded, then the difference rounded: no FMA
 *     F[p] = w[p]                                           for every position p of row i
 * Every w[t] gets at most one update per pivot and the pivots come in ascending k, so each element of F has one right answer,
 * however a row's columns are spread over lanes: the serial loop's, bit for bit, the same on every run.  An update that does not
 * exist is skipped, its product never formed (0 * Inf would make a NaN).  Pivots are not validated: a zero or vanishing u_kk gives
 * +-Inf or NaN by the rules above, as d_i does in K15; a caller who wants to know calls smvp_csr_diagonal on F.
 * Row i reads exactly the rows k < i for which (i, k) is stored: the dependency graph of the LOWER triangular solve.  The schedule,
 * the launches (wide levels + chains, plan option "trsv_chain_width" as read at create) and the rule are K15's: no kernel waits on
 * a value another workgroup writes in the same launch -- no flags, no grid barrier, no atomics.
 * Out of scope: IC(0) as a format of its own, ILU(k) and thresholds, pivoting or diagonal shifts, TJDS and sharded handles, an
 * analysis on the device, and coalescing or sorting a matrix that does not qualify.  The solver that uses the two plans for a
 * non-symmetric A is smvp_csr_pbicgstab / smvp_tjds_pbicgstab, K18, below. */
typedef struct smvp_ilu0 smvp_ilu0_t; /* borrows A's arrays; owns F's values, F's handle, level_ptr / order / diag_pos on the device */
typedef struct smvp_ilu0_info {
    unsigned struct_size;  /* set by the caller to sizeof(smvp_ilu0_info_t) before the call; another size is SMVP_ERR_INVALID */
    int levels;            /* of the LOWER triangle of A's pattern: smvp_trsv_info's for a LOWER plan */
    int max_level_width;
    int launches;          /* kernels one factorisation enqueues: wide levels + chains */
    int chains;
    int chain_width;
    int lanes_per_row;     /* lanes a row of a wide level gets (from the mean and the longest row) */
    long long entries;     /* nnz: values one factorisation reads from A and writes to F */
    long long pivots;      /* stored entries below the diagonal = divisions */
    double plan_bytes;     /* device memory the object owns: F's values, level_ptr, order, diag_pos */
    double build_ms;       /* host wall time of smvp_csr_ilu0_create: copy back, check, analysis, uploads, the first factorisation,
                              F's handle */
} smvp_ilu0_info_t;
/*   - smvp_csr_ilu0_create has smvp_csr_trsv_create's shape and cost: col_ind comes back from the device once, the host runs
 *     smvp_csr_ilu0_check and K15's LOWER analysis, level_ptr / order / diag_pos go up, F's values (nnz doubles, 16-byte aligned) are
 *     allocated, the first factorisation runs -- F is valid on return -- and F is made as an ordinary plain-CSR handle that ADOPTS
 *     h's own d_row_ptr / d_col_ind and the new value array (SMVP_MEM_DEVICE; handles may share arrays).  The call waits for
 *     `stream`, allocates, and refuses a capturing stream.  h's own state and plans are untouched, and h must outlive f.  Any number
 *     of factorisations and K15 plans per handle.
 *   - smvp_ilu0_factor factorises h's CURRENT val again (adopted arrays changed in place; a Newton or time-step loop's new matrix on
 *     the old pattern).  Asynchronous on `stream`; allocates nothing, synchronises nothing and can be captured from its first call
 *     on: a plain chain of kernels with no parallel branches.  It reads only A's val, and on return of the work every element of
 *     F's values has been written anew.  K15 plans made on F earlier see the new factors without any call: they borrow val.  An f
 *     is used by one stream at a time.
 *   - smvp_ilu0_matrix: F's handle, BORROWED -- owned and destroyed by f; never pass it to smvp_csr_destroy.  F's own product
 *     (smvp_csr_spmv on F) follows the rules above for adopted values changed in place, smvp_ilu0_factor being such a change:
 *     VECTOR / STREAM / STREAM_CARRY and smvp_csr_spmm need nothing, COLSWEEP / BINNED need smvp_csr_set_kernel first.
 *   - SMVP_ERR_INVALID (nothing enqueued, outputs untouched): a NULL argument, a wrong struct_size, rows != cols, a capturing stream
 *     at create.  SMVP_ERR_UNSUPPORTED (likewise): a handle that is not plain CSR, a row block, a row whose columns are not strictly
 *     ascending, a row without a stored diagonal; smvp_last_error names the first offending row and what is wrong with it.
 *   - n == 0: everything succeeds with 0 levels and 0 launches.
 *   - smvp_csr_ilu0_check and smvp_csr_ilu0_host are the check and the loop above on HOST arrays, no device touched.  The check
 *     writes diag_pos (rows ints; may be NULL) and *bad_row = -1 (may be NULL) on success; on refusal diag_pos is untouched and
 *     *bad_row is the first offending row: SMVP_ERR_INVALID for rows < 0, a NULL row_ptr with rows > 0, a NULL col_ind with entries,
 *     a row_ptr that is not a non-decreasing sequence from 0, a column outside [0, rows); SMVP_ERR_UNSUPPORTED for columns not
 *     strictly ascending and for a missing diagonal.  smvp_csr_ilu0_host refuses the same and writes nothing then; val_out (nnz
 *     doubles) may be val itself.  It is the definition on one core: the only CPU baseline the library has. */
int smvp_csr_ilu0_create(smvp_ilu0_t **out, const smvp_csr_t *h, void *stream);
int smvp_ilu0_factor(smvp_ilu0_t *f, void *stream);
int smvp_ilu0_matrix(const smvp_ilu0_t *f, smvp_csr_t **F);
int smvp_ilu0_info(const smvp_ilu0_t *f, smvp_ilu0_info_t *out);
void smvp_ilu0_destroy(smvp_ilu0_t *f);
int smvp_csr_ilu0_check(int rows, const int *row_ptr, const int *col_ind, int *diag_pos, int *bad_row);
int smvp_csr_ilu0_host(int rows, const int *row_ptr, const int *col_ind, const double *val, double *val_out);

/* ------------------------------------------------- BiCGSTAB */
/* A x = b for a general (non-symmetric) square A on a handle the caller already holds, kernel K13 (new: the reference only
 * multiplies).  It needs only y = A x.  `dot` is the one above, unchanged; every other operation is one correctly rounded IEEE
 * operation per element, with no FMA (-ffp-contract=off, as everywhere in the library): with the dot's order fixed, every number
 * below is a pure function of the handle's single products.
 *   bb = dot(b, b)        thr = (tol * tol) * bb      (tol * tol rounded on the host, the product on the device)
 *   x_0 = d_x0, or zeros if NULL
 *   r_0 = b - A x_0       (d_x0 == NULL: r_0 = b bit for bit, no product is run)
 *   rhat = r_0  (kept for the whole run)      p_0 = r_0      rho_0 = rr_0 = dot(r_0, r_0)
 *   step 0 rule:  NONFINITE if bb or rr_0 is NaN or +-Inf;  CONVERGED if rr_0 <= thr
 *   step k = 1, 2, ...:
 *     v     = A p_{k-1}                      the handle's own product, bit for bit: smvp_csr_spmv (current plan), or
 *                                            smvp_tjds_set_x + smvp_tjds_spmv (current mode)
 *     sigma = dot(rhat, v)
 *     rule A:  NONFINITE if sigma is NaN or +-Inf;  BREAKDOWN if sigma == 0               -> x stays x_{k-1}, half = 0
 *     alpha = rho_{k-1} / sigma
 *     s     = r_{k-1} - alpha * v            (alpha * v_i rounded, then the difference rounded)
 *     ss    = dot(s, s)
 *     rule H:  NONFINITE if ss is NaN or +-Inf                                             -> x stays x_{k-1}, half = 0
 *              CONVERGED if ss <= thr                                                      -> x = x_{k-1} + alpha * p_{k-1}, half = 1
 *     t     = A s                            the handle's own product
 *     ts = dot(t, s)      tt = dot(t, t)
 *     rule T:  NONFINITE if ts or tt is NaN or +-Inf                                       -> x stays x_{k-1}, half = 0
 *              BREAKDOWN if not (tt > 0)                                                   -> x = x_{k-1} + alpha * p_{k-1}, half = 1
 *     omega = ts / tt
 *     x_k = (x_{k-1} + alpha * p_{k-1}) + omega * s      (each product rounded; the additions in this order)
 *     r_k = s - omega * t
 *     rr_k = dot(r_k, r_k)      rho_k = dot(rhat, r_k)
 *     rule B (the first that holds):  NONFINITE if rr_k or rho_k is NaN or +-Inf;  CONVERGED if rr_k <= thr;
 *              MAX_STEPS if k == max_steps;  BREAKDOWN if omega == 0 or rho_k == 0        -> x = x_k, half = 0, full = k
 *     beta = (rho_k / rho_{k-1}) * (alpha / omega)       (two quotients rounded, then their product)
 *     p_k  = r_k + beta * (p_{k-1} - omega * v)          (omega * v_i rounded, the difference, beta times it, the sum: four roundings)
 * No square root is taken: the histories and the result hold squared norms.  The residual is the recurrence's, not b - A x: the
 * two differ by rounding, and no true-residual check is made.
 * The device evaluates the rules at EVERY step; the first that holds, in the order written, is the `reason`, and from then on
 * nothing is written to x or to the histories.  The host reads a status block at looked steps only -- step 0, every k with
 * k % check_every == 0, and k == max_steps -- and only to leave the loop: steps, full, half, reason, rr, both histories and every bit
 * of d_x do not depend on check_every (which decides how many products are enqueued in vain, and how often the host waits), exactly
 * as for conjugate gradients.
 * Restarts, a true-residual check and the sharded handles are out of scope.  Preconditioning is smvp_csr_pbicgstab /
 * smvp_tjds_pbicgstab, K18, below. */
enum { SMVP_BICGSTAB_CONVERGED = 0, SMVP_BICGSTAB_MAX_STEPS = 1, SMVP_BICGSTAB_BREAKDOWN = 2, SMVP_BICGSTAB_NONFINITE = 3 };
typedef struct smvp_bicgstab_opts {
    unsigned struct_size; /* set by smvp_bicgstab_opts_default, checked as for smvp_cg_opts_t */
    int max_steps;        /* >= 1; default 100 */
    int check_every;      /* >= 1; default 10 */
    double tol;           /* >= 0, finite; default 1e-10: stop at |r| <= tol |b| */
} smvp_bicgstab_opts_t;
void smvp_bicgstab_opts_default(smvp_bicgstab_opts_t *o);
typedef struct smvp_bicgstab_result {
    int steps;   /* the step the run stopped in (0 at step 0); up to two products per step were enqueued, the one for r_0 not counted */
    int full;    /* complete updates of x: steps, or steps - 1 where rule A, H or T fired */
    int half;    /* 1: d_x additionally holds the alpha * p half update of step `steps` */
    int reason;  /* SMVP_BICGSTAB_* */
    double rr;   /* the squared norm of the residual that belongs to d_x: ss of the last step when half = 1, else rr_full */
    double bb;   /* dot(b, b) */
} smvp_bicgstab_result_t;
/*   - d_b: n doubles.  d_x0: n doubles, NULL = zeros.  d_x: n doubles; the iterates live in it, and it holds x_full (plus the half
 *     update where half = 1) afterwards.  d_x may be the same pointer as d_x0; any other overlap of the two, and any overlap of d_b
 *     and d_x, is SMVP_ERR_INVALID.  After SMVP_ERR_HIP the content of d_x is unspecified.
 *   - rr_each: a caller-owned HOST array of max_steps + 1 doubles, filled 0 .. full with rr.  ss_each: max_steps doubles, filled
 *     with ss of every step that reached rule H (the step in which rule H or T fired included, the one in which rule A fired not).
 *     Either may be NULL.  Both come from a device-side history copied back once at the end, and are left untouched beyond the
 *     filled elements.  (ss is never -0.0 -- an accumulator starts at +0.0 -- so a caller who needs the count of ss_each may fill
 *     it with -0.0 first, as the Python binding does.)
 *   - The call returns after the work on `stream` has finished.  It allocates its workspace per call -- five vectors, the partials
 *     of six dots, four words, the histories, two status blocks -- and frees it on every way out.  Beside the two products a step
 *     is five launches and eighteen passes over a vector: rhat, v read (sigma's partials); v, r read, s written over r with ss's
 *     partials; t, s read (the partials of ts and tt, two accumulators per lane); x, p, s, t, rhat read, x, r written with the
 *     partials of rr and rho; r, p, v read, p written.
 *   - SMVP_ERR_INVALID for: a NULL handle, opts, result or d_b (before any HIP call); a struct_size that is not this library's;
 *     max_steps < 1, check_every < 1, tol negative, NaN or infinite; rows != cols; a NULL d_x with n > 0; the overlaps above; a
 *     capturing stream.  Nothing is enqueued then, d_x and *result are left untouched, and a capturing stream's capture stays valid.
 *   - SMVP_ERR_UNSUPPORTED (likewise) for a CSR handle that is not plain CSR, and for a TJDS handle in ATOMIC mode or with
 *     ref-quirks on, as for the power method.
 *   - n == 0: SMVP_OK, steps 0, full 0, half 0, reason SMVP_BICGSTAB_CONVERGED, rr = bb = +0.0.
 *   - State: a CSR handle's plan is untouched -- smvp_csr_spmv after the call gives the bits it gave before.  A TJDS handle's
 *     permuted operand is afterwards that of the last vector multiplied: call smvp_tjds_set_x again before the next
 *     smvp_tjds_spmv, as after any change of x.  A handle is used by one stream at a time, as ever. */
int smvp_csr_bicgstab(smvp_csr_t *h, const smvp_bicgstab_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                      smvp_bicgstab_result_t *result, double *rr_each, double *ss_each, void *stream);
int smvp_tjds_bicgstab(smvp_tjds_t *h, const smvp_bicgstab_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                       smvp_bicgstab_result_t *result, double *rr_each, double *ss_each, void *stream);

/* ------------------------------------------------- preconditioned BiCGSTAB */
/* Right-preconditioned BiCGSTAB on a square n x n handle's own product, kernel K18 (new: the reference only multiplies): BiCGSTAB
 * above with K16's M = T1 diag(m)^-1 T2, the solver ILU(0) (K17) was missing for a matrix that is not symmetric.  smvp_bicgstab_opts_t,
 * smvp_bicgstab_result_t and SMVP_BICGSTAB_* are K13's, unchanged.  `first` and `second` are plans of smvp_csr_trsv_create on ANY
 * plain-CSR handle of n rows on the handle's device; the product may be a CSR or a TJDS handle's.  Write yhat = M^-1 y for
 *   w   = T1^-1 y      smvp_trsv_solve(first, y, yhat): K15's bits;  w = y when first == NULL
 *   w_i = m_i * w_i    one rounded multiplication; skipped entirely when d_m == NULL
 *   yhat = T2^-1 w     smvp_trsv_solve(second, ...), in place on w;  yhat = w when second == NULL
 * Each of first, d_m and second may be NULL on its own; all three NULL is SMVP_ERR_INVALID (that run is smvp_csr_bicgstab's).
 *   - Jacobi: first = second = NULL, d_m = 1 ./ diagonal (smvp_csr_diagonal / smvp_tjds_diagonal and one reciprocal, the caller's):
 *     one multiplication, no plan and no CSR copy, so it works from a TJDS handle too.
 *   - ILU(0): first = LOWER / DIAG_UNIT and second = UPPER / DIAG_STORED on smvp_ilu0_matrix, d_m = NULL.
 *   - Symmetric Gauss-Seidel: first = LOWER / DIAG_STORED and second = UPPER / DIAG_STORED on A itself, d_m = smvp_csr_diagonal of
 *     A: M = (D + L) D^-1 (D + U), no extracted copy.
 * `dot` is the one above; every other operation is one correctly rounded IEEE operation per element, no FMA, every product rounded
 * before its sum: every number below is a pure function of the handle's single products and K15's solves.
 *   bb = dot(b, b)        thr = (tol * tol) * bb      (tol * tol rounded on the host, the product on the device)
 *   x_0 = d_x0, or zeros if NULL
 *   r_0 = b - A x_0       (d_x0 == NULL: r_0 = b bit for bit, no product is run)
 *   rhat = r_0  (kept for the whole run)      p_0 = r_0      rho_0 = rr_0 = dot(r_0, r_0)
 *   step 0 rule:  NONFINITE if bb or rr_0 is NaN or +-Inf;  CONVERGED if rr_0 <= thr      (M is not applied at step 0's rule)
 *   step k = 1, 2, ...:
 *     phat  = M^-1 p_{k-1}
 *     v     = A phat                         the handle's own product, bit for bit, as for K13
 *     sigma = dot(rhat, v)
 *     rule A:  NONFINITE if sigma is NaN or +-Inf;  BREAKDOWN if sigma == 0               -> x stays x_{k-1}, half = 0
 *     alpha = rho_{k-1} / sigma
 *     s     = r_{k-1} - alpha * v            (alpha * v_i rounded, then the difference rounded)
 *     ss    = dot(s, s)
 *     rule H:  NONFINITE if ss is NaN or +-Inf                                             -> x stays x_{k-1}, half = 0
 *              CONVERGED if ss <= thr                                                      -> x = x_{k-1} + alpha * phat, half = 1
 *     shat  = M^-1 s
 *     t     = A shat                         the handle's own product
 *     ts = dot(t, s)      tt = dot(t, t)
 *     rule T:  NONFINITE if ts or tt is NaN or +-Inf                                       -> x stays x_{k-1}, half = 0
 *              BREAKDOWN if not (tt > 0)                                                   -> x = x_{k-1} + alpha * phat, half = 1
 *     omega = ts / tt
 *     x_k = (x_{k-1} + alpha * phat) + omega * shat      (each product rounded; the additions in this order)
 *     r_k = s - omega * t
 *     rr_k = dot(r_k, r_k)      rho_k = dot(rhat, r_k)
 *     rule B (the first that holds):  NONFINITE if rr_k or rho_k is NaN or +-Inf;  CONVERGED if rr_k <= thr;
 *              MAX_STEPS if k == max_steps;  BREAKDOWN if omega == 0 or rho_k == 0        -> x = x_k, half = 0, full = k
 *     beta = (rho_k / rho_{k-1}) * (alpha / omega)       (two quotients rounded, then their product)
 *     p_k  = r_k + beta * (p_{k-1} - omega * v)          (four roundings, as for K13)
 * No square root is taken.  With right preconditioning r is the recurrence's residual of the ORIGINAL system, so the stop rule
 * stays rr <= thr: smvp_csr_bicgstab can be swapped for smvp_csr_pbicgstab under the same tol.  The two differ from b - A x by
 * rounding, and no true-residual check is made.  Nothing of M is validated: a zero stored diagonal in a triangle, or a NaN in m,
 * shows as NONFINITE by rule A.
 * The device evaluates the rules at EVERY step; the first that holds, in the order written, is the `reason`, and from then on
 * nothing is written to x or to the histories.  The host reads a status block at looked steps only -- step 0, every k with
 * k % check_every == 0, and k == max_steps -- and only to leave the loop: steps, full, half, reason, rr, both histories and every bit
 * of d_x do not depend on check_every.  A step enqueued in vain runs both products and up to four solves: with plans, a caller wants
 * a small check_every.
 * Two identities follow, and the tests hold the device to both.  With first = LOWER / DIAG_STORED and second = UPPER / DIAG_UNIT on a
 * handle that stores only a unit diagonal, and d_m = NULL, every number is smvp_csr_bicgstab's, bit for bit: (y_i - (+0.0)) / 1.0 is
 * y_i, a signed zero included.  The same holds with both plans NULL and d_m all ones.
 *   - Operands, histories and n == 0 as for smvp_csr_bicgstab; d_x may be d_x0.  d_m, where given, is n doubles, only read, and must
 *     not overlap d_x.
 *   - The call returns after the work on `stream` has finished.  It allocates its workspace per call -- seven vectors (r, p, v, t,
 *     rhat, phat, shat), the partials of six dots, four words, the histories, two status blocks -- and frees it on every way out.
 *     Beside the two products and the solves' own launches a step is five launches and nineteen passes over a vector: rhat, v read;
 *     v, r read, s written over r; t, s read; x, phat, shat, s, t, rhat read, x, r written; r, p, v read, p written.  Without a
 *     `first` the multiplication by m costs no launch: the kernel that writes p (or s) reads m and writes phat (or shat) in the same
 *     pass -- Jacobi is five launches and 23 passes -- and `second` then solves in place on that.  With a `first` it is a launch of
 *     its own between the solves, as in K16.  With neither `first` nor d_m, `second` solves straight from p or s.  The bits are
 *     the same either way.  No kernel waits on a value another workgroup writes; no atomics, no flags.
 *   - SMVP_ERR_INVALID for everything smvp_csr_bicgstab refuses, and for: first, d_m and second all NULL; a plan whose row count is
 *     not n or whose device is not the handle's; d_m overlapping d_x; a capturing stream.  SMVP_ERR_UNSUPPORTED as for
 *     smvp_csr_bicgstab.  Nothing is enqueued then, d_x and *result are left untouched, and a capturing stream's capture stays valid.
 *     first == second is allowed.
 *   - State: the handle as after smvp_csr_bicgstab / smvp_tjds_bicgstab.  The plans are used on `stream` for the duration of the
 *     call (a plan is used by one stream at a time, as ever) and are unchanged afterwards, as are the handles they borrow:
 *     smvp_trsv_solve gives the bits it gave before.  `val` of either handle changed in place (smvp_ilu0_factor is such a change)
 *     is seen by the next call.
 * Out of scope: left or split preconditioning, restarts and a true-residual check, a block of k right-hand sides, the sharded
 * handles, and building the reciprocal diagonal (one reciprocal of smvp_csr_diagonal's output, the caller's). */
int smvp_csr_pbicgstab(smvp_csr_t *h, const smvp_bicgstab_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                       smvp_trsv_t *first, const double *d_m, smvp_trsv_t *second, smvp_bicgstab_result_t *result, double *rr_each,
                       double *ss_each, void *stream);
int smvp_tjds_pbicgstab(smvp_tjds_t *h, const smvp_bicgstab_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                        smvp_trsv_t *first, const double *d_m, smvp_trsv_t *second, smvp_bicgstab_result_t *result, double *rr_each,
                        double *ss_each, void *stream);

/* ------------------------------------------------- restarted GMRES */
/* Right-preconditioned restarted GMRES(m) on a square n x n handle's own product, kernel K19 (new: the reference only multiplies):
 * what a caller reaches for when BiCGSTAB above stalls or breaks down.  It minimises the residual over the Krylov space, so the
 * estimate never rises inside a cycle.  The orthogonalisation is classical Gram-Schmidt applied twice ("CGS2"): a fixed sequence of
 * launches that needs no host decision.  M = T1 diag(m)^-1 T2 is exactly K18's and yhat = M^-1 y is computed as there; each of
 * first, d_m and second may be NULL, and ALL THREE NULL IS ALLOWED HERE: that is plain GMRES (z = v_j, no launch).  `dot` is the one
 * above, unchanged; every other operation is one correctly rounded IEEE operation, on an element or on a scalar, with no FMA;
 * sqrt is the correctly rounded IEEE root.
 *   bb = dot(b, b)      thr = (tol * tol) * bb          (as K13)
 *   x = d_x0, or zeros if NULL;   k = 0 (steps done)
 *   cycle c = 0, 1, ...:
 *     r = b - A x                 (cycle 0 with d_x0 == NULL: r = b bit for bit, no product)
 *     tr_c = dot(r, r)            -> restart_each[c];  for c = 0 also rr_each[0]
 *     start rule:  NONFINITE if bb or tr_c is NaN or +-Inf;  CONVERGED if tr_c <= thr        -> x as it stands, columns = 0
 *     beta = sqrt(tr_c)    v_1 = r / beta  (true division per element)    g_1 = beta
 *     for j = 1 .. restart:       k = k + 1
 *       z = M^-1 v_j   (z = v_j without M)          w = A z   (the handle's own product, bit for bit)
 *       h_i  = dot(v_i, w)                 i = 1 .. j      (each one is `dot`'s bits)
 *       w    = w - h_i * v_i   for i = 1 .. j ascending    (product rounded, difference rounded, per element)
 *       q_i  = dot(v_i, w)                 i = 1 .. j      (second pass, on the updated w)
 *       w    = w - q_i * v_i   for i = 1 .. j ascending
 *       h_i  = h_i + q_i                                   (one rounded addition)
 *       h_{j+1} = sqrt(dot(w, w))
 *       for i = 1 .. j-1:  t = (c_i*h_i) + (s_i*h_{i+1});  h_{i+1} = (c_i*h_{i+1}) - (s_i*h_i);  h_i = t
 *       d = sqrt((h_j*h_j) + (h_{j+1}*h_{j+1}))
 *       rule S1:  NONFINITE if any of h_1 .. h_{j+1} (before the rotations) or d is NaN or +-Inf;  BREAKDOWN if d == 0
 *                                                                                            -> update with columns = j - 1
 *       c_j = h_j / d    s_j = h_{j+1} / d    R_{1..j-1, j} = h_{1..j-1}    R_{jj} = d
 *       g_{j+1} = -(s_j * g_j)     g_j = c_j * g_j         rr_k = g_{j+1} * g_{j+1}  -> rr_each[k]
 *       rule S2 (first that holds):  CONVERGED if rr_k <= thr;  MAX_STEPS if k == max_steps  -> update with columns = j
 *       v_{j+1} = w / h_{j+1}
 *     (j == restart without a stop: update with columns = restart, next cycle)
 *   update with `cols` columns (nothing for cols = 0):
 *     y_i for i = cols .. 1:  acc = g_i;  for l = i+1 .. cols ascending: acc = acc - (R_il * y_l);  y_i = acc / R_ii
 *     u = y_1 * v_1;  u = u + (y_i * v_i) for i = 2 .. cols ascending;   x = x + M^-1 u
 * Squared norms: the histories and the result hold squared residual norms, as everywhere.  Happy breakdown: h_{j+1} == 0 needs no
 * rule -- it gives s_j = 0 and rr_k = +0.0 <= thr, hence CONVERGED; v_{j+1} is only formed after S2 has passed.  No scaling is done
 * against overflow of the squares: that case shows as NONFINITE.  rr_k is the recurrence's estimate of the residual of the ORIGINAL
 * system, because the preconditioning is on the right, so tol means what it means for K13 and K18; tr_c is a true residual, which
 * every restart gets for free.  bb, every tr_c and every rr_k are never -0.0.  Nothing of M is validated, as for K18.
 * The device evaluates the rules at EVERY step and at every cycle start; after a stop nothing more is written to x, the basis, R, g
 * or the histories.  The host reads a status block at looked steps only -- step 0, every k with k % check_every == 0, and
 * k == max_steps -- and only to leave the loop: every result, both histories and every bit of d_x do not depend on check_every.
 * The update of x at a stop in mid-cycle has no fixed place in the enqueued sequence: the update launches enqueued at a cycle's end
 * act only while the run has not stopped, and once the host has seen the stop it enqueues the same launches once more, told to act
 * on the stopped cycle's columns; nothing they read has changed since.  No kernel waits on a value another workgroup writes; no
 * atomics, no flags; every scalar hand-off is a launch boundary.
 * Out of scope: the basis is non-flexible (the update applies M^-1 once to V y; no second basis is stored); left or split
 * preconditioning, flexible GMRES, deflation, a single-pass or modified Gram-Schmidt variant, several right-hand sides and the
 * sharded handles. */
enum { SMVP_GMRES_CONVERGED = 0, SMVP_GMRES_MAX_STEPS = 1, SMVP_GMRES_BREAKDOWN = 2, SMVP_GMRES_NONFINITE = 3 };
typedef struct smvp_gmres_opts {
    unsigned struct_size; /* set by smvp_gmres_opts_default, checked as for smvp_cg_opts_t */
    int max_steps;        /* >= 1; default 100 */
    int check_every;      /* >= 1; default 10 */
    int restart;          /* 1 .. 64; default 30: the columns of a cycle */
    double tol;           /* >= 0, finite; default 1e-10: stop at |r| <= tol |b| */
} smvp_gmres_opts_t;
void smvp_gmres_opts_default(smvp_gmres_opts_t *o);
typedef struct smvp_gmres_result {
    int steps;   /* steps done: products with a basis vector (those for a cycle's r are not counted) */
    int cycles;  /* cycles started */
    int columns; /* of the last update: j or j - 1 of the step that stopped the run, 0 after a start rule */
    int reason;  /* SMVP_GMRES_* */
    double rr;   /* rr_steps; tr_c after a start rule, or where rule S1 fired in a cycle's first step */
    double bb;   /* dot(b, b) */
} smvp_gmres_result_t;
/*   - d_b, d_x0, d_x, d_m, first and second as for smvp_csr_pbicgstab: d_x may be d_x0, any other overlap of d_x with d_x0, d_b
 *     or d_m is SMVP_ERR_INVALID; the plans are smvp_csr_trsv_create's on any plain-CSR handle of n rows on the handle's device.
 *   - rr_each: a caller-owned HOST array of max_steps + 1 doubles, filled 0 .. steps (0 .. steps - 1 where rule S1 ended the run).
 *     restart_each: ceil(max_steps / restart) + 1 doubles, filled 0 .. cycles - 1.  Either may be NULL; both are left untouched
 *     beyond the filled elements.
 *   - The call returns after the work on `stream` has finished.  It allocates its workspace per call and frees it on every way
 *     out: min(restart, max_steps) + 1 basis vectors, then w, u, z and r; the partials of `restart` dots (2048 doubles each) and of
 *     dot(w, w), dot(r, r) and dot(b, b), then R, c, s, g, y, the coefficient words, the histories and two status blocks.
 *   - Beside the product and the solves' own launches step j of a cycle is six launches: the multi-dot (v_1 .. v_j read once, w
 *     once per 4 coefficients), a fold of one workgroup per coefficient, the first update with the second pass's partials (the basis
 *     read twice, w read, written and read back), a fold, the second update with dot(w, w)'s partials (the basis read once, w read
 *     and written), and the close of the step (w read, v_{j+1} written): 4 j + 6 + 2 ceil(j / 4) passes over a vector.  An update
 *     of x is a one-lane back-substitution, one pass over `cols` basis vectors, the solves, and x = x + z; a cycle's start is one
 *     product and two launches.
 *   - SMVP_ERR_INVALID and SMVP_ERR_UNSUPPORTED as for smvp_csr_pbicgstab, except that first, d_m and second all NULL is accepted;
 *     restart outside 1 .. 64 is SMVP_ERR_INVALID.  Nothing is enqueued then, d_x and *result are left untouched, and a capturing
 *     stream's capture stays valid.
 *   - n == 0: SMVP_OK, steps 0, cycles 0, columns 0, reason SMVP_GMRES_CONVERGED, rr = bb = +0.0.
 *   - State: the handle and the plans as after smvp_csr_pbicgstab / smvp_tjds_pbicgstab: a CSR handle's plan is untouched, a TJDS
 *     handle needs smvp_tjds_set_x again, smvp_trsv_solve gives the bits it gave before. */
int smvp_csr_gmres(smvp_csr_t *h, const smvp_gmres_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                   smvp_trsv_t *first, const double *d_m, smvp_trsv_t *second, smvp_gmres_result_t *result, double *rr_each,
                   double *restart_each, void *stream);
int smvp_tjds_gmres(smvp_tjds_t *h, const smvp_gmres_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                    smvp_trsv_t *first, const double *d_m, smvp_trsv_t *second, smvp_gmres_result_t *result, double *rr_each,
                    double *restart_each, void *stream);

/* ------------------------------------------------- LSQR: least squares for a rectangular matrix */
/* min |A x - b|_2 for ANY M x N handle -- tall, wide, square, rank deficient -- by LSQR (Paige and Saunders), kernel K22 (new: the
 * reference only multiplies).  It is the one solver here that takes rows != cols, and the loop around the transposed product
 * above: a step is one product with A and one with A^T.  For a consistent system it returns a solution (from x_0 = 0 the one of
 * least norm), else a least-squares solution.  `dot` is K12's, unchanged; sqrt is the correctly rounded IEEE root (as in K19);
 * every other operation is one correctly rounded IEEE operation, on an element or on a scalar, with no FMA.  Every bracket below
 * is one rounded operation.
 * The bidiagonalisation's vectors are stored UNNORMALISED: uh_k = beta_k u_k (M doubles) and vh_k = alpha_k v_k (N doubles); each
 * scaling is folded into the next pass that reads the vector, and no pass exists only to divide a vector by its norm.
 *   bnorm = sqrt(dot(b, b))          thr = tol * bnorm
 *   x = d_x0, or zeros if NULL;      uh_1 = b - A x_0    (d_x0 == NULL: uh_1 = b bit for bit, no product)
 *   beta_1 = sqrt(dot(uh_1, uh_1))
 *   p = A^T uh_1;   vh_1[i] = p[i] / beta_1;   alpha_1 = sqrt(dot(vh_1, vh_1))
 *       (beta_1 zero, NaN or +-Inf: vh_1 is not formed and alpha_1 = +0.0)
 *   phibar_1 = beta_1;  rhobar_1 = alpha_1;  A2 = alpha_1 * alpha_1;  anorm_0 = sqrt(A2);  rnorm_0 = beta_1;
 *   arnorm_0 = beta_1 * alpha_1                                        -> rnorm_each[0], arnorm_each[0]
 *   step 0 rules:  NONFINITE if bnorm, beta_1, alpha_1, anorm_0 or arnorm_0 is NaN or +-Inf;  CONVERGED if beta_1 <= thr;
 *                  LEAST_SQUARES if alpha_1 == 0                       -> x = x_0, steps = updates = 0
 *   w_1[i] = vh_1[i] / alpha_1
 *   step k = 1, 2, ...:
 *     q = A vh_k                     the handle's own product, bit for bit
 *     uh_{k+1}[i] = (q[i] / alpha_k) - (alpha_k * (uh_k[i] / beta_k));          beta_{k+1} = sqrt(dot(uh_{k+1}, uh_{k+1}))
 *     p = A^T uh_{k+1}               ht's own product (CSR), smvp_tjds_spmv_transposed (TJDS), bit for bit
 *     vh_{k+1}[i] = (p[i] / beta_{k+1}) - (beta_{k+1} * (vh_k[i] / alpha_k));   alpha_{k+1} = sqrt(dot(vh_{k+1}, vh_{k+1}))
 *         (beta_{k+1} zero, NaN or +-Inf: vh_{k+1} is not formed and alpha_{k+1} = +0.0)
 *     rho = sqrt((rhobar_k * rhobar_k) + (beta_{k+1} * beta_{k+1}));   c = rhobar_k / rho;   s = beta_{k+1} / rho
 *     theta = s * alpha_{k+1};   rhobar_{k+1} = -(c * alpha_{k+1});   phi = c * phibar_k;   phibar_{k+1} = s * phibar_k
 *     tx = phi / rho;   tw = theta / rho
 *     A2 = (A2 + (beta_{k+1} * beta_{k+1})) + (alpha_{k+1} * alpha_{k+1});   anorm_k = sqrt(A2)
 *     ac = alpha_{k+1} * |c|;   rnorm_k = phibar_{k+1};   arnorm_k = phibar_{k+1} * ac
 *     rule N:  NONFINITE if beta_{k+1}, alpha_{k+1}, rho, tx, tw, anorm_k, rnorm_k or arnorm_k is NaN or +-Inf
 *                                     -> x stays x_{k-1}, updates = k - 1; rnorm, arnorm, anorm and A2 stay step k - 1's
 *     x_k[i] = x_{k-1}[i] + (tx * w_k[i])                              rnorm_k, arnorm_k -> rnorm_each[k], arnorm_each[k]
 *     rule S (first that holds):  CONVERGED if rnorm_k <= thr;  LEAST_SQUARES if ac <= atol * anorm_k;  MAX_STEPS if k == max_steps
 *                                     -> x = x_k, updates = k
 *     w_{k+1}[i] = (vh_{k+1}[i] / alpha_{k+1}) - (tw * w_k[i])
 * rnorm is the recurrence's estimate phibar of |b - A x|, arnorm its estimate of |A^T (b - A x)|, anorm the running estimate of
 * |A|_F: NORMS, not squares, because this method takes roots anyway.  CONVERGED is the residual rule |r| <= tol |b|;
 * LEAST_SQUARES is the normal-equations rule |A^T r| <= atol |A|_F |r|, with |r| cancelled on both sides.
 * Two ends that are no breakdown, and in which no quotient by zero is consumed.  beta_{k+1} == 0: the Krylov space is exhausted
 * and the system is solved; alpha_{k+1} = +0.0, s = 0, c = +-1, rnorm_k = 0, the step completes its update of x and ends as
 * CONVERGED, for every tol.  alpha_{k+1} == 0 with beta_{k+1} > 0: A^T uh_{k+1} = 0, x_k is a least-squares solution; ac = 0, the
 * step completes its update and ends as LEAST_SQUARES, for every atol, unless it converged; at step 0 this is b orthogonal to
 * range(A), and x_0 stands.  No scaling is done against overflow of the squares: that case shows as NONFINITE.
 * The device evaluates the rules at EVERY step; once one has fired nothing more is written to x or to the histories.  The host
 * reads a status block at looked steps only -- step 0, every k with k % check_every == 0, and k == max_steps -- and only to
 * leave the loop: no result, history element or bit of d_x depends on check_every or on the stream.  No kernel waits on a
 * value another workgroup writes; no atomics, no flags; every scalar hand-off is a launch boundary.
 * That ht holds A^T is the caller's contract, as symmetry is for K12, and is not checked beyond its shape.
 * Out of scope: damping (Tikhonov's lambda), the acond and xnorm estimates and a conlim rule, LSMR and CGLS, preconditioning,
 * several right-hand sides, the sharded handles, and a CSR route that builds its own A^T (the library makes no hidden second
 * copy: smvp_csr_create_transposed is the caller's call). */
enum { SMVP_LSQR_CONVERGED = 0, SMVP_LSQR_LEAST_SQUARES = 1, SMVP_LSQR_MAX_STEPS = 2, SMVP_LSQR_NONFINITE = 3 };
typedef struct smvp_lsqr_opts {
    unsigned struct_size; /* set by smvp_lsqr_opts_default, checked as for smvp_cg_opts_t */
    int max_steps;        /* >= 1; default 100 */
    int check_every;      /* >= 1; default 10 */
    int pad;
    double tol;           /* >= 0, finite; default 1e-10: CONVERGED at |r| <= tol |b| */
    double atol;          /* >= 0, finite; default 1e-10: LEAST_SQUARES at |A^T r| <= atol |A|_F |r| */
} smvp_lsqr_opts_t;
void smvp_lsqr_opts_default(smvp_lsqr_opts_t *o);
typedef struct smvp_lsqr_result {
    int steps;     /* steps done: pairs of products (those for uh_1 and vh_1 are not counted) */
    int updates;   /* updates of x done: steps, or steps - 1 after rule N */
    int reason;    /* SMVP_LSQR_* */
    int pad;
    double rnorm;  /* rnorm_updates */
    double arnorm; /* arnorm_updates */
    double anorm;  /* anorm_updates */
    double bnorm;  /* sqrt(dot(b, b)) */
} smvp_lsqr_result_t;
/*   - h is M x N.  smvp_csr_lsqr: ht is the caller's handle of A^T, normally smvp_csr_create_transposed(h): REQUIRED, plain CSR,
 *     N x M, h's nnz, on h's device.  q = A vh is smvp_csr_spmv(h) on h's current plan, p = A^T uh is smvp_csr_spmv(ht) on ht's
 *     own; both plans may be any SMVP_CSR_KERNEL_* and are left as they are.  smvp_tjds_lsqr: one handle and no second copy;
 *     q = A vh is smvp_tjds_set_x + smvp_tjds_spmv in the current mode, p = A^T uh is smvp_tjds_spmv_transposed (K8).
 *   - d_b: M doubles.  d_x0: N doubles, NULL = zeros.  d_x: N doubles; the iterates live in it, and it holds x_updates afterwards.
 *     d_x may be the same pointer as d_x0; any other overlap of the two, and any overlap of d_b and d_x, is SMVP_ERR_INVALID.
 *     d_b is only read.  After SMVP_ERR_HIP the content of d_x is unspecified.
 *   - rnorm_each, arnorm_each: caller-owned HOST arrays of max_steps + 1 doubles each, filled 0 .. updates.  Either may be NULL.
 *     Both come from a device-side history copied back once at the end, and are left untouched beyond the filled elements.
 *   - The call returns after the work on `stream` has finished.  It allocates its workspace per call -- uh and q (M doubles each),
 *     vh, p and w (N each), the partials of three dots, one word, the histories, two status blocks -- and frees it on every way out.
 *   - Beside the two products a step is TWO launches and eleven passes over a vector.  Pass U, after q = A vh_k: every workgroup
 *     folds the partials of dot(vh_k, vh_k) and closes step k - 1 (its scalars and rules; workgroup 0 writes the status block
 *     and the histories), applies step k - 1's updates of x and w (vh, w, x read, w, x written: 5 passes over N) and writes
 *     uh_{k+1} with the partials of its dot (q, uh read, uh written: 3 passes over M).  Pass V, after p = A^T uh_{k+1}: every
 *     workgroup folds those partials to beta_{k+1} and writes vh_{k+1} with the partials of its dot (p, vh read, vh written:
 *     3 passes over N).  A step's close thus rides in the next step's pass U.  At a looked step the close is launched on its own
 *     (pass U without its uh half) so that the host can read its status block, and the next step's pass U has nothing to close:
 *     a third launch at looked steps only, the same arithmetic either way.  Step 0 is four launches of its own, the fill or copy of x and one or two products.
 *   - SMVP_ERR_INVALID for: a NULL handle, ht (CSR), opts, result or d_b (before any HIP call); a struct_size that is not this
 *     library's; max_steps < 1, check_every < 1, tol or atol negative, NaN or infinite; an ht that is not N x M with h's nnz on
 *     h's device; a NULL d_x with N > 0; the overlaps above; a capturing stream.  SMVP_ERR_UNSUPPORTED for: a CSR handle (h or ht)
 *     that is not plain CSR or is a row block with first_row != 0; a TJDS handle in ATOMIC mode or with ref-quirks on, as for
 *     every solver.  Nothing is enqueued then, d_x and *result are left untouched, and a capturing stream's capture stays valid.
 *   - M == 0 or N == 0: SMVP_OK, steps 0, updates 0, reason SMVP_LSQR_CONVERGED, all four norms and element 0 of both
 *     histories +0.0; with M == 0 < N, d_x holds x_0 (zeros without one).  d_b may not be NULL even then.
 *   - State: both CSR handles' plans are untouched -- smvp_csr_spmv on h and on ht gives the bits it gave before.  A TJDS handle's
 *     permuted operand is afterwards that of the last vh multiplied: call smvp_tjds_set_x again before the next smvp_tjds_spmv.
 *     A handle is used by one stream at a time, as ever. */
int smvp_csr_lsqr(smvp_csr_t *h, smvp_csr_t *ht, const smvp_lsqr_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                  smvp_lsqr_result_t *result, double *rnorm_each, double *arnorm_each, void *stream);
int smvp_tjds_lsqr(smvp_tjds_t *h, const smvp_lsqr_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                   smvp_lsqr_result_t *result, double *rnorm_each, double *arnorm_each, void *stream);

/* ------------------------------------------------------------ multicolour reordering */
/* Colour the rows on the device, number them colour by colour, build B = P A P^T, kernel K23 (new: the reference only multiplies).
 * A triangular solve (K15) and an ILU(0) (K17) cost one launch per level of their dependency graph, and natural orderings are deep
 * (lap2d(1024): 2047 levels).  In B a row of colour c reads only rows of colours < c (LOWER) or > c (UPPER), so every plan made on
 * B has at most `colors` levels.  B is an ordinary plain-CSR handle: K15 to K21 take it as it is.
 *
 * The colouring has ONE right answer.  Vertices are the rows 0 .. n-1 of the square handle h.  N(v) = the columns u != v stored in
 * row v of h and, where ht is given (normally smvp_csr_create_transposed(h): the rows that store v), in row v of ht; repeats and
 * explicit zeros count once, the diagonal does not count.  With a structurally symmetric h, or with ht, N is symmetric and the
 * colouring is proper: no stored (i, j), i != j, joins two rows of one colour.  With an unsymmetric h and no ht the result is still
 * the defined one, merely not proper: that can cost levels later, never a wrong number (the plans analyse B themselves).
 *     key(v)   = mix32((uint32)v ^ seed)
 *     mix32(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16      (32-bit wrap-around; a bijection)
 *     color(v) = the smallest integer >= 0 that is not color(u) for any u in N(v) with key(u) > key(v)
 *     depth(v) = 0 if no u in N(v) has a larger key, else 1 + the largest depth(u) over those u
 * colors = 1 + max color(v) <= 1 + max |N(v)|, every colour below it is used; depth = 1 + max depth(v).  This is serial greedy
 * colouring in descending key order, and what a Jones-Plassmann round scheme computes whatever its timing.
 *
 * smvp_csr_color runs rounds, one launch each.  d_color starts at -1 everywhere (written by the call).  A group of lanes_per_row
 * lanes (2 .. 64, K15's rule on the rows' mean and longest length) takes a vertex without a colour and walks its row(s); a
 * neighbour of larger key that has no colour yet leaves the vertex for the next launch -- no lane ever waits on a value another
 * workgroup writes -- otherwise the group takes the first colour no such neighbour holds, in windows of 64 colours.  The host
 * reads a counter after every round and stops when all n are coloured: 1 <= rounds <= depth for n > 0, and only `rounds` depends
 * on timing.  The call therefore synchronises `stream`, allocates nothing but the counter, and leaves both handles' state alone
 * (their products give the bits they gave before).
 *   - SMVP_ERR_INVALID: a NULL h; a NULL d_color with n > 0; rows != cols; an ht of other dimensions or on another device; a
 *     struct_size (opts or info) that is not this library's; max_rounds < 1; a capturing stream (nothing is enqueued, the capture
 *     stays valid).  SMVP_ERR_UNSUPPORTED: a handle (h or ht) that is not plain CSR or is a row block; a run not finished after
 *     max_rounds launches -- d_color is then unspecified, nothing is leaked.  SMVP_ERR_ALLOC as elsewhere.  Outputs are untouched
 *     after every other failure.  n = 0 succeeds with colors 0 and rounds 0.
 *   - info (may be NULL; set struct_size first): entries = the stored entries one full round reads (h's and ht's); build_ms = the
 *     rounds' host wall time.  largest_class / smallest_class are counted on the host from one copy of d_color.
 * smvp_csr_color_host is the definition on one core, no device touched: color (rows ints), *colors and *depth.  t_row_ptr /
 * t_col_ind are both NULL or both set.  SMVP_ERR_INVALID for rows < 0, a NULL output, a NULL array that is needed, one of the two
 * t_ arrays alone, a row_ptr that does not start at 0 or decreases, a column outside [0, rows); nothing is written then. */
typedef struct smvp_color_opts {
    unsigned struct_size; /* sizeof(smvp_color_opts_t), set by smvp_color_opts_default */
    unsigned seed;        /* default 0 */
    int max_rounds;       /* default 4096 */
} smvp_color_opts_t;
void smvp_color_opts_default(smvp_color_opts_t *o);
typedef struct smvp_color_info {
    unsigned struct_size;
    int colors, rounds, largest_class, smallest_class, lanes_per_row;
    long long entries;
    double build_ms;
} smvp_color_info_t;
int smvp_csr_color(const smvp_csr_t *h, const smvp_csr_t *ht, const smvp_color_opts_t *opts, int *d_color, smvp_color_info_t *info,
                   void *stream);
int smvp_csr_color_host(int rows, const int *row_ptr, const int *col_ind, const int *t_row_ptr, const int *t_col_ind, unsigned seed,
                        int *color, int *colors, int *depth);
/* Classes (colours, or any labels in [0, classes)) to a permutation: the new order is by (class, old index) ascending, so it is
 * stable.  d_old_of_new[p] = the element that lands at p, d_new_of_old[d_old_of_new[p]] = p (n ints each, on `device`);
 * class_ptr (HOST, classes + 1 ints, may be NULL) delimits the classes in the new order.  Built on the library's stable radix sort
 * and prefix sums; one workspace is allocated and freed, and the call returns after the work on `stream` has finished.  An element
 * of d_class outside [0, classes) is SMVP_ERR_INVALID, found by a check kernel before anything indexes with it: nothing is written.
 * SMVP_ERR_INVALID also for n < 0, classes < 0, a NULL device array with n > 0, a capturing stream. */
int smvp_perm_from_classes(int device, int n, int classes, const int *d_class, int *d_old_of_new, int *d_new_of_old, int *class_ptr,
                           void *stream);
/* B = P A P^T as a handle: B(new_of_old[r], new_of_old[c]) = A(r, c) for ANY permutation the caller brings (a colouring is one
 * source; an RCM or a nested dissection from elsewhere another).  *out is bit for bit smvp_csr_from_coo of the entries
 * (new_of_old[r], new_of_old[c], val) listed in h's storage order: rows have ascending columns, ties in storage order, so a matrix
 * without repeats that stores its diagonal qualifies for ILU(0).  It is smvp_csr_create_transposed's route and contract: one kernel
 * writes the mapped COO list, smvp_csr_from_coo_device sorts it, the arrays are adopted; the result is an independent handle on
 * AUTO that outlives h; a capturing stream is refused; SMVP_ERR_ALLOC leaks nothing; *out is NULL after every failure; the result
 * is stale after h's val changes in place.  d_new_of_old (n ints on h's device) is validated on the device before any kernel
 * indexes with it: a repeated or out-of-range element is SMVP_ERR_INVALID with nothing built.  Square plain-CSR handles only
 * (rows != cols: SMVP_ERR_INVALID; a TJDS flavour or a row block: SMVP_ERR_UNSUPPORTED).
 * B is a matrix in its own right: its product adds a row in ascending NEW column order, so (B P x) is P (A x) in exact
 * arithmetic only -- the bits are B's, defined by B's arrays, not A's. */
int smvp_csr_create_permuted(smvp_csr_t **out, const smvp_csr_t *h, const int *d_new_of_old, void *stream);
/* d_out[p] = d_in[d_index[p]], p < n: with old_of_new this is P x, with new_of_old on the result x again, every bit of every
 * element (signed zeros, NaN payloads).  Asynchronous on `stream`, allocates nothing, capturable.  An index outside [0, n) is not
 * followed: that element of d_out gets a quiet NaN.  d_out must not overlap d_in (SMVP_ERR_INVALID, as a NULL array with n > 0
 * and n < 0). */
int smvp_vector_gather(int device, int n, const int *d_index, const double *d_in, double *d_out, void *stream);

/* ------------------------------------------- several GPUs, one host process */
/* New design (the reference is one CPU thread): the matrix is cut into `ngpus` row blocks balanced by entries
 * (smvp_partition_rows); GPU g holds block g -- cut again into `chunks` row chunks, each its own CSR / TJDS handle --
 * plus all of x and produces its slice of y; the exchange (RCCL ncclAllGather or direct peer pushes over xGMI, below) puts
 * the full y on every GPU, chunk c travelling while chunk c+1 is multiplied.  devices NULL = 0 .. ngpus-1.  librccl is dlopen'ed on first use.
 * (bench.py does the same with one process per GPU.)  No multi-GPU box is available to this project's tests: on
 * hardware the RCCL path has run with ONE GPU only; the N > 1 logic of this layer runs in the test suite through
 * SMVP_EXCHANGE_COPIES / _DIRECT with 2 ... 8 virtual ranks on one GPU, the Python layer's through gloo.
 * When a rank fails inside a product its peers' collectives may never complete: smvp_sharded_spmv reports the error and
 * marks the handle unusable (later calls fail at once, smvp_sharded_destroy aborts the communicators instead of waiting). */
typedef struct smvp_sharded smvp_sharded_t;
/* How the y blocks travel (round 5: a measured choice, SURVEY 7 "hard parts" -- a ring all-gather pushes 7 blocks through
 * one xGMI link, direct pushes use all seven):
 *   RCCL    ncclAllGather over xGMI into a padded wire buffer, one communicator rank per GPU, then one small kernel per
 *           GPU places the pieces at their rows;
 *   COPIES  every rank pushes its chunk STRAIGHT INTO EVERY RANK'S FULL VECTOR with hipMemcpyAsync (peer access; the
 *           copy engines, no compute unit involved) -- no wire buffer, no padding, no placement pass;
 *   DIRECT  the same pushes by ONE kernel per chunk whose workgroups store to the peers' vectors over xGMI (one launch
 *           instead of N copy calls, all links at once);
 *   AUTO    (default) at handle creation every form that is available -- RCCL needs distinct devices and a librccl that
 *           loads, the pushes need peer access -- moves one product's y once, timed; the fastest is kept
 *           (smvp_sharded_exchange_info reports the times, smvp_sharded_set_exchange switches).
 * COPIES and DIRECT order the ranks with events and a host-side meeting point of the issuing threads, and accept a device
 * list that names one device several times ("virtual ranks": more ranks than GPUs must be asked for with one of these two
 * by name): the whole N-GPU code path then runs on a one-GPU box.  All forms give the same bits. */
enum { SMVP_EXCHANGE_RCCL = 0, SMVP_EXCHANGE_COPIES = 1, SMVP_EXCHANGE_DIRECT = 2, SMVP_EXCHANGE_AUTO = 3 };
typedef struct smvp_shard_opts {
    unsigned struct_size; /* sizeof(smvp_shard_opts_t) of the header the caller was built with: set by
                             smvp_shard_opts_default, checked by the create calls (a caller built against another layout
                             is refused instead of being misread) */
    int chunks;   /* row chunks per GPU (the granularity of the product / all-gather overlap); 0 = 4 when ngpus > 1, else 1 */
    int balance;  /* 1 (default): blocks and chunks balanced by entries; 0: equal heights */
    int exchange; /* SMVP_EXCHANGE_* (default AUTO); with COPIES / DIRECT ngpus may exceed the visible devices (devices NULL = g % visible) */
} smvp_shard_opts_t;
void smvp_shard_opts_default(smvp_shard_opts_t *o);
int smvp_csr_sharded_create(smvp_sharded_t **out, int ngpus, const int *devices, int rows, int cols, int nnz,
                            const int *row_ptr, const int *col_ind, const double *val); /* host CSR arrays */
int smvp_csr_sharded_create_ex(smvp_sharded_t **out, int ngpus, const int *devices, int rows, int cols, int nnz,
                               const int *row_ptr, const int *col_ind, const double *val, const smvp_shard_opts_t *opts);
int smvp_tjds_sharded_create(smvp_sharded_t **out, int ngpus, const int *devices, const smvp_coo_t *coo,
                             int rows, int cols, int nnz); /* an independent TJDS per row chunk */
int smvp_tjds_sharded_create_ex(smvp_sharded_t **out, int ngpus, const int *devices, const smvp_coo_t *coo,
                                int rows, int cols, int nnz, const smvp_shard_opts_t *opts);
int smvp_sharded_set_csr_kernel(smvp_sharded_t *h, int kernel, int param); /* smvp_csr_set_kernel on every chunk */
/* The exchange of one product's y (every chunk, nothing to overlap with), timed `reps` times under every available form;
 * a handle created with AUTO then keeps the fastest.  Called by the create calls for AUTO (reps = 3). */
int smvp_sharded_probe_exchange(smvp_sharded_t *h, int reps);
/* active: the SMVP_EXCHANGE_* in use; available: bit e set = form e can be selected; ms[3]: milliseconds of the last probe by
 * form (RCCL, COPIES, DIRECT; < 0: not measured); rccl_ranks: what the communicator itself reports (ncclCommCount), 0
 * without one.  NULL = skip. */
int smvp_sharded_exchange_info(const smvp_sharded_t *h, int *active, int *available, double *ms, int *rccl_ranks);
int smvp_sharded_set_exchange(smvp_sharded_t *h, int exchange); /* one of the available forms (not AUTO) */
int smvp_sharded_set_x(smvp_sharded_t *h, const double *x_host); /* NULL = ones; replicated to every GPU */
/* One product, asynchronous: the chunk products on every GPU and, by `allgather`, the exchange of y:
 * 0 none; SMVP_GATHER_OVERLAPPED: chunk c is gathered (communication stream) while chunk c+1 is multiplied;
 * SMVP_GATHER_AFTER: all gathers after all products.  timed != 0 brackets it with an event pair per GPU. */
enum { SMVP_GATHER_NONE = 0, SMVP_GATHER_OVERLAPPED = 1, SMVP_GATHER_AFTER = 2 };
int smvp_sharded_spmv(smvp_sharded_t *h, int allgather, int timed);
int smvp_sharded_synchronize(smvp_sharded_t *h, double *ms_of_last_timed_product); /* max over the GPUs */
/* power iteration: the gathered y (optionally divided by its largest magnitude) becomes x on every GPU;
 * call between two smvp_sharded_spmv(h, 1, ..), after which the all-gather is what feeds the next product.
 * Asynchronous, ordered behind the product on every GPU's stream: no smvp_sharded_synchronize is needed before or after it.
 * normalize: the rule of smvp_run_opts_t.normalize, applied by every GPU to its own gathered copy (the same data, the same
 * arithmetic: the same bits everywhere).  It is the gathered vectors (smvp_sharded_get_y(.., gathered = 1, ..)) that are
 * normalised; the local slices (gathered = 0) keep the raw product.  Steps chained this way give, bit for bit, what the same
 * handle gives when the caller reads the gathered y, normalises it and hands it back through smvp_sharded_set_x.
 * SMVP_ERR_INVALID on a matrix that is not square; nothing is changed then. */
int smvp_sharded_feed_back(smvp_sharded_t *h, int normalize);
int smvp_sharded_get_y(smvp_sharded_t *h, int slot, int gathered, double *y_host);
int smvp_sharded_info(const smvp_sharded_t *h, int *ngpus, int *rows_per_gpu); /* rows_per_gpu = the tallest block */
/* bounds[ngpus + 1] of the row blocks and chunk_bounds[ngpus * (chunks + 1)] of their chunks, global rows (NULL = skip) */
int smvp_sharded_layout(const smvp_sharded_t *h, int *chunks, int *bounds, int *chunk_bounds);
void smvp_sharded_destroy(smvp_sharded_t *h);

#define SMVP_CSR_SWEEP_PARTS(rows_per_block, parts) ((rows_per_block) | (((parts) == 8 ? 3 : (parts) == 4 ? 2 : (parts) == 2 ? 1 : 0) << 24))
/* for experiments: the same with the 256-entry chunks a wavefront keeps in flight forced to 1, 2 or 4 (0 = the library's rule) */
#define SMVP_CSR_SWEEP_PARAM(rows_per_block, parts, chunks) \
    (SMVP_CSR_SWEEP_PARTS(rows_per_block, parts) | (((chunks) == 4 ? 3 : (chunks) == 2 ? 2 : (chunks) == 1 ? 1 : 0) << 26))

/* ------------------------------------------------ reference-shaped entry points */
typedef struct smvp_run_opts {
    unsigned struct_size; /* sizeof(smvp_run_opts_t) of the caller's header: set by smvp_run_opts_default, checked by the
                             compute calls -- a struct that was never passed through smvp_run_opts_default, or was built
                             against another layout, is refused with SMVP_ERR_INVALID instead of being misread */
    int device;         /* HIP device ordinal */
    int csr_kernel;     /* SMVP_CSR_KERNEL_* */
    int csr_param;      /* 0 = default */
    int tjds_ref_quirks;/* 1: reproduce the reference's defective TJDS output */
    int convert_on_device; /* 1: COO -> CSR / TJDS on the GPU (smvp_*_from_coo_device), 0: on the host */
    int ngpus;          /* 0 or 1: one GPU (`device`); N > 1: row blocks on GPUs 0..N-1 + RCCL all-gather of y */
    int iterate;        /* 1: power iteration, x_{k+1} = A x_k for `iters` steps -- the product the assignment asked
                           for (comment at main-cli.c:401); square matrices; y = the last iterate; each step timed */
    int normalize;      /* with iterate: divide every iterate by its largest magnitude (keeps 1000 steps finite).  The divisor
                           is the largest |element| among the elements that are not NaN; an iterate whose largest magnitude
                           is 0 is left as it is (no 0 / 0); an infinite one turns the finite elements into zeros of their
                           sign and the infinite ones into NaN; NaN elements stay NaN.  Each quotient is the correctly rounded
                           IEEE quotient (subnormal divisors included), so the iterate is a pure function of the product.
                           The iterated result is, bit for bit, that of the same handle's single products chained by the
                           caller with this rule in between -- on every path whose product is reproducible from run to run
                           (every CSR family, TJDS ROW_GATHER and TWO_PHASE, ngpus > 1; not TJDS ATOMIC) */
    int tjds_mode;      /* SMVP_TJDS_MODE_* for smvp_tjds_compute (AUTO = ROW_GATHER) */
    int timing;         /* SMVP_TIMING_*: how each product is timed */
    int shard_exchange; /* ngpus > 1: SMVP_EXCHANGE_* (default AUTO; COPIES / DIRECT: ngpus may exceed the visible GPUs -- virtual ranks) */
    int repeat_patience_us; /* SMVP_TIMING_DEVICE, the repeating kernel: microseconds a workgroup waits at the barrier between two
                           products before the launch gives up and the run falls back to one launch per product (0 = 50 000;
                           negative = none at all: whoever has to wait gives up -- the fallback's test) */
    const double *x;    /* host operand, NULL = all ones (main-cli.c:368-369) */
} smvp_run_opts_t;
void smvp_run_opts_default(smvp_run_opts_t *o);

/* How the per-product window of main-cli.c:408-419 is taken.  EVENTS: a hipEvent pair around each product's
 * launches.  DEVICE: the kernel times itself -- every wave notes the device's constant-rate wall clock when it
 * starts and when its last store has been acknowledged; the product's time is max(last) - min(first) -- and up to 1024
 * products run as ONE launch of a repeating form of the kernel whose workgroups stay resident and meet at a (fence-free: the
 * products are independent) barrier between two products; where that form is not available (or gives up: the grid must be
 * resident as a whole) the products are replayed one launch each from a hipGraph.  AUTO picks DEVICE for launches of up to 4096 workgroups of the tile
 * kernels (where an event pair would measure mostly itself: the reference's own sample matrices), else EVENTS.  DEVICE and
 * DEVICE_GRAPH are refused (SMVP_ERR_UNSUPPORTED) where no launch can stamp itself: any other kernel, several GPUs, a changing
 * operand, and a matrix without rows, whose product launches nothing (AUTO times that one with events). */
enum { SMVP_TIMING_AUTO = 0, SMVP_TIMING_EVENTS = 1, SMVP_TIMING_DEVICE = 2,
       SMVP_TIMING_DEVICE_GRAPH = 3 /* DEVICE, but one launch per product replayed from a hipGraph: what DEVICE falls back to */ };
typedef struct smvp_run_info {
    int timing;            /* SMVP_TIMING_EVENTS or SMVP_TIMING_DEVICE (also for DEVICE_GRAPH: repeat_launches / graph_replays tell the
                              form): what the last smvp_*_compute on this thread used */
    int graph_replays;     /* hipGraph launches it took (0 = plain launches) */
    double wall_ms;        /* host wall time of the whole timed loop, launches, timing and waits included */
    double device_clock_khz; /* DEVICE: rate of the clock the times were taken with */
    int repeat_launches;   /* DEVICE: launches of the repeating kernel it took -- up to 1024 products per launch, every product's
                              window stamped between device-side barriers (0: one launch per product) */
    int repeat_gave_up;    /* DEVICE: 1 = a launch of the repeating kernel gave up at a barrier (its grid was not resident as a whole) and
                              the run was done over, one launch per product */
} smvp_run_info_t;
int smvp_last_run_info(smvp_run_info_t *out);

/* Replaces  double *smvp_csr_compute(MMRawData*, int rows, int nnz, int iters,
 *                                    struct _time_data_*)      main-cli.c:325-469
 * COO in -> CSR build -> upload -> `iters` products, each timed on its own with
 * hipEvents around the product only (the reference's clock_gettime window,
 * main-cli.c:408-419) -> y[rows] and time_each_ms[iters] out, stats reduced as
 * main-cli.c:428-456.  `cols` is new: the reference assumes a square matrix. */
int smvp_csr_compute(const smvp_coo_t *coo, int rows, int cols, int nnz, int iters,
                     const smvp_run_opts_t *opts, double *y, double *time_each_ms,
                     smvp_time_stats_t *stats);
/* Replaces  double *smvp_tjds_compute(MMRawData*, int rows, int cols, int nnz,
 *                                     int iters, struct _time_data_*)  main-cli.c:734-1162 */
int smvp_tjds_compute(const smvp_coo_t *coo, int rows, int cols, int nnz, int iters,
                      const smvp_run_opts_t *opts, double *y, double *time_each_ms,
                      smvp_time_stats_t *stats);

/* ------------------------------------------------------------ stats + report */
/* Replaces the reduction at main-cli.c:428-456 and calcStDevDouble (:114-130;
 * population standard deviation -- the reference's reads uninitialised locals). */
int smvp_time_stats(const double *time_each_ms, int iters, smvp_time_stats_t *out);
/* Replaces generateReportText, main-cli.c:246-320: writes
 * <report_dir>/smvp-toolbox_report_<alg_name>_<unix_time>.txt (opened "a+") with
 * the reference's exact text.  report_dir NULL or "" = current directory;
 * unix_time 0 = time(NULL).  The path written is returned in out_path if given. */
int smvp_generate_report_text(const char *input_file_name, const char *report_dir,
                              const char *alg_name, int nnz, int rows, int iters,
                              const double *y, const smvp_time_stats_t *stats,
                              unsigned long unix_time, char *out_path, size_t out_path_cap);

/* ------------------------------------------------------------- CISR export */
/* Replaces  void smvp_cisr_coegen(MMRawData*, int rows, int nnz, int slotCount)   main-cli.c:473-729
 * (-g / --cisr-gen, -s / --slots): the matrix dealt row by row onto `slots` channels and written as a Xilinx Vivado
 * .coe block-RAM image -- the reference prints it to stdout, here it goes to `out`.  Host only (no GPU).  Returns
 * SMVP_ERR_UNSUPPORTED where the reference prints "slot_group_iter overran fInputNonZeros!" and exits
 * (main-cli.c:596-600; always with one slot).  Parity unpinned: the reference holds no .coe output. */
int smvp_cisr_coegen(const smvp_coo_t *coo, int rows, int nnz, int slots, FILE *out);
int smvp_cisr_coegen_path(const smvp_coo_t *coo, int rows, int nnz, int slots, const char *path);

/* ------------------------------------------------------ synthetic workloads */
/* SURVEY 8(d) / BASELINE.json configs: matrices generated straight into CSR,
 * a pure function of (kind, seed, global row) so any row block can be produced
 * independently (row-block sharding needs no communication). */
enum {
    SMVP_SYNTH_MEMPLUS_SHAPED = 1, /* memplus's row-length histogram + band structure, scaled */
    SMVP_SYNTH_UNIFORM = 2         /* `param` nnz per row, uniform distinct columns */
};
/* Row lengths for global rows [row_begin, row_end): lens[row_end-row_begin]. */
int smvp_synth_row_lengths(int kind, uint64_t seed, int64_t rows_total, int64_t cols_total,
                           int param, int64_t row_begin, int64_t row_end, int *lens);
/* Fill col_ind/val for the block given its (local, 0-based) row_ptr; columns
 * sorted ascending and distinct inside a row; values uniform in [-1, 1). */
int smvp_synth_fill(int kind, uint64_t seed, int64_t rows_total, int64_t cols_total,
                    int param, int64_t row_begin, int64_t row_end, const int *row_ptr,
                    int *col_ind, double *val, int threads);
/* Row-block partition balanced by nnz: bounds[parts+1], bounds[0]=0, bounds[parts]=rows. */
int smvp_partition_rows(const int *row_ptr, int rows, int parts, int *bounds);
/* x[i] uniform in [0, 1): the top 53 bits of splitmix64's finaliser of (seed + i), times 2^-53.  The operand of the
 * command line's --x random (seed 67890); the reference only ever multiplies by ones (main-cli.c:368-369). */
int smvp_vector_random(double *x, int64_t n, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* SMVP_AMD_H */
