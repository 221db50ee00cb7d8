// smvp_common.h -- internal helpers shared by the host-side translation units.
#pragma once
#include "smvp_amd.h"

#include <cstdarg>
#include <cstdio>
#include <vector>

namespace smvp {
// The most entries a matrix may have (smvp_csr_create, smvp_tjds_create and the device-side converters): 32-bit indices like
// the reference's; the kernels and plan builders add up to a few thousand to an entry index and round grids up to whole tiles
constexpr long long kMaxEntries = 2147483647ll - 65536;

// Records a message for smvp_last_error() and hands back `code`.
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void clear_error();
int option(const char *name, int fallback);  // smvp_set_option's value, or `fallback` where it is not set (smvp_error.cpp)

// K15, the host analysis of a triangular solve (smvp_trsv_plan.cpp): the levels of the `uplo` triangle's rows, the rows listed by
// (level, row) ascending, and what the triangle holds; then the launches of a schedule -- [first, last) levels each, a chain (one
// workgroup, a barrier between its levels) or one wide level
struct TrsvSchedule {
    std::vector<int> level_of_row, level_ptr, order;
    int levels = 0, max_level_width = 0, missing_diagonals = 0, max_row_entries = 0;  // (the longest row of the triangle, its diagonal included)
    long long off_entries = 0, diag_entries = 0;  // stored entries strictly inside the triangle / on the diagonal
};
struct TrsvLaunch {
    int first, last;
    bool chain;
};
int trsv_analyse(int rows, const int *row_ptr, const int *col_ind, int uplo, TrsvSchedule *out);
void trsv_launches(const std::vector<int> &level_ptr, int chain_width, std::vector<TrsvLaunch> *out, int *chains);
// K21, a sweeps plan's storage range per row: what a sweep reads of the row; their total and the longest
void trsv_ranges(int rows, const int *row_ptr, const int *col_ind, int uplo, int diag, std::vector<int> *begin, std::vector<int> *end,
                 long long *entries, int *longest);

// K17, what an ILU(0) asks of a CSR pattern (smvp_ilu0_plan.cpp): smvp_csr_ilu0_check under the caller's name `fn`, the arguments
// checked for null already
int ilu0_check(const char *fn, int rows, const int *row_ptr, const int *col_ind, int *diag_pos, int *bad_row);

// K22, what smvp_csr_lsqr (needs_ht) and smvp_tjds_lsqr refuse before any HIP call (smvp_lsqr_args.cpp): a NULL handle, ht, opts,
// result or d_b, a struct_size that is not this library's, options out of range
int lsqr_check_args(const char *fn, const void *h, const void *ht, bool needs_ht, const smvp_lsqr_opts_t *opts, const void *result,
                    const double *d_b);

// K23, the multicolour ordering (smvp_reorder_host.cpp, smvp_reorder.hip): the key of vertex v is mix32(v ^ seed), a bijection on
// 32-bit words; and what smvp_csr_color refuses of its two structs before any HIP call (either may be NULL)
#ifdef __HIP__
#define SMVP_HOST_DEVICE __host__ __device__
#else
#define SMVP_HOST_DEVICE
#endif
SMVP_HOST_DEVICE inline unsigned mix32(unsigned x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
int color_check_opts(const char *fn, const smvp_color_opts_t *opts, const smvp_color_info_t *info);
}  // namespace smvp

// internal, device side (smvp_convert_device.hip): see its definition
struct ihipStream_t;
namespace smvp {
int build_row_inverse(const int *d_row_ind, int nnz, int rows, int *d_inv_ptr, int *d_inv_pos, ihipStream_t *stream);
int build_row_gather_plan(const int *d_row_ind, const int *d_start_pos, int num_diag, int nnz, int rows,
                          int *d_seg_ptr, int *d_pos, int *d_kcol, ihipStream_t *stream);
int build_colsweep_plan(const int *d_row_ptr, const int *d_col_ind, const double *d_val, int rows, int cols, int nnz, int strip_rows,
                        int parts, int chunk, int row_bits, int turn_cap, long long *d_strip_ptr, int *d_e_col, double *d_e_val,
                        unsigned short *d_e_row, ihipStream_t *stream);
int sort_tile_windows(const int *d_pos, int nnz, int tile, const int *d_start_pos, int num_diag, int slot_bits,
                      const double *d_val, int cache_min_tiles, int *d_pos_sorted, int *d_meta, int *d_cache_ptr,
                      double **d_val_cache, int *cached_total, ihipStream_t *stream);
int build_tile_half_streams(const int *d_pos, int nnz, int tile, const int *d_start_pos, int num_diag, const double *d_val,
                            int cache_min_tiles, unsigned *d_word32, int *d_cache_ptr, int *d_run_ptr,
                            double **d_val_cache, int **d_run_tab, unsigned short **d_group_run, int *cached_total,
                            int *runs_total, ihipStream_t *stream);
int build_column_offsets(const int *d_col_ind, int nnz, int tile, int *d_col_base, unsigned short *d_col16, int *fits,
                         ihipStream_t *stream);
// kFlavorCsr16P: the values of the packable tiles (full, d_col_base[tile] >= 0; 2048-entry tiles) a second time as codes and escapes.
// Allocates the four arrays (the caller frees them; all null after a failure).  *doubles_read = the entries one product still reads
// as 8-byte values: the escapes, counted exactly, and every entry of a tile that is not packable.  max_doubles >= 0: where that count
// is larger, the build ends once it is known -- SMVP_OK, the count, and no array (the escapes are never allocated); < 0: no bound.
int build_packed_values(const double *d_val, int nnz, const int *d_col_base, unsigned char **d_code8, double **d_hot, int **d_esc_ptr,
                        double **d_esc_val, long long *doubles_read, long long *esc_slots, long long max_doubles, ihipStream_t *stream);
int build_tile_overflow(const int *d_pos, const int *d_ovf_ptr, int total, int ntiles, int tile, int nnz,
                        const int *d_start_pos, int num_diag, const double *d_val, double *d_ovf_val, int *d_ovf_k, int positions,
                        ihipStream_t *stream);
}
