// smvp_tjds.hip -- the TJDS handle: a device-resident TJDS matrix and its launch plans.
//
// This file owns what the reference keeps in TJDSData (main-cli.c:70-75) once it is in HBM.  Two of its plans run on the tile
// kernel through a nested CSR handle (smvp_engine.hip), which this file creates, re-plans and reads through the functions of
// smvp_engine.h only: the layout of smvp_csr is not visible here.
#include "smvp_engine.h"

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

// The launch plans of a TJDS handle, in the idiom of the CSR handle's (TilePlan / free_tile_plan): each is a plain struct with
// one release function that frees what the struct owns and resets it to its default value.  The modes' plans are built on
// first use of the mode and kept when the mode changes.

// ATOMIC, the first phase of TWO_PHASE, and every mode with ref-quirks on: the column-major work items; build_tjds_plan
// (rebuilt when the ref-quirks mode changes)
struct TjdsWorkPlan {
    bool quirks = false;
    int *d_start_pos = nullptr;  // start_pos as the kernel should see it
    int4 *d_work = nullptr;
    int nwork = 0;
    long long planned_nnz = 0;
};

// ROW_GATHER, the one-kernel product: the entries regrouped by row -- segment bounds and TJDS positions, plus the permuted
// columns when the 32-bit form is used; `csr` is the owner-kernel plan over that stream (the tile-ordered form keeps its own
// sorted copies); ensure_row_gather
struct RowGatherPlan {
    int *d_ptr = nullptr;  // rows + 1
    int *d_pos = nullptr;  // nnz, row order
    int *d_k = nullptr;    // nnz, kFlavorTjdsK only
    smvp_csr_t *csr = nullptr;
};

// TWO_PHASE: per-entry products + their sum per row through the row-inverted index; ensure_two_phase
struct TwoPhasePlan {
    double *d_prod = nullptr;   // nnz doubles
    int *d_inv_ptr = nullptr;   // rows + 1
    int *d_inv_pos = nullptr;   // nnz: positions j grouped by row_ind[j], ascending inside a row
    smvp_csr_t *csr = nullptr;  // the tile-ordered stream over (inv_ptr, inv_pos) with prod as its values, no operand
};

// smvp_tjds_spmm (K10, smvp_spmm.hip): the entries regrouped by row in buffers of its own (not the two plans' above: they
// come and go with the modes), built by the first call and kept whatever the mode is
struct TjdsSpmmPlan {
    int *d_ptr = nullptr;    // rows + 1
    int *d_pos = nullptr;    // nnz: TJDS positions, ascending inside a row
    int *d_col = nullptr;    // nnz: the original column perm[pos - start_pos[d]]
    int *d_order = nullptr;  // rows: K7's row order
    bool planned = false;
    double build_ms = 0.0;
};

struct smvp_tjds {
    int device = 0;
    int rows = 0, cols = 0, nnz = 0, num_diag = 0;
    int *d_perm = nullptr;
    int *d_start_pos = nullptr;  // num_diag + 1 entries (+1 pad)
    int *d_row_ind = nullptr;
    double *d_val = nullptr;
    bool own_perm = false, own_start_pos = false, own_row_ind = false, own_val = false;
    std::vector<int> h_start_pos;

    double *d_x_perm = nullptr;  // max(rows, cols) doubles
    bool x_set = false;

    int mode = SMVP_TJDS_MODE_ROW_GATHER;

    RowGatherPlan rg;  // (tests/test_gpu_transposed.py reads rg.csr out of the handle's memory: the members up to here keep their places)
    TwoPhasePlan two;
    TjdsSpmmPlan spmm;
    TjdsWorkPlan work;
    double plan_build_ms = 0.0;  // host wall time of the plan builds so far (work items + the modes' plans)
};

namespace {

void free_work_plan(TjdsWorkPlan *p)
{
    for (void *q : {(void *)p->d_start_pos, (void *)p->d_work})
        if (q)
            (void)hipFree(q);
    *p = TjdsWorkPlan{};
}

void free_row_gather(RowGatherPlan *p)
{
    smvp_csr_destroy(p->csr);
    for (void *q : {(void *)p->d_ptr, (void *)p->d_pos, (void *)p->d_k})
        if (q)
            (void)hipFree(q);
    *p = RowGatherPlan{};
}

void free_two_phase(TwoPhasePlan *p)
{
    smvp_csr_destroy(p->csr);
    for (void *q : {(void *)p->d_prod, (void *)p->d_inv_ptr, (void *)p->d_inv_pos})
        if (q)
            (void)hipFree(q);
    *p = TwoPhasePlan{};
}

void free_tjds_spmm_plan(TjdsSpmmPlan *p)
{
    for (void *q : {(void *)p->d_ptr, (void *)p->d_pos, (void *)p->d_col, (void *)p->d_order})
        if (q)
            (void)hipFree(q);
    *p = TjdsSpmmPlan{};
}

// val + row_ind, start_pos, perm
inline double tjds_matrix_bytes(const smvp_tjds *h) { return 12.0 * h->nnz + 4.0 * (h->num_diag + 1.0) + 4.0 * h->cols; }

int build_tjds_plan(smvp_tjds *h, bool quirks, int ref_num_tjdiag, int last_diag_single)
{
    TjdsWorkPlan &w = h->work;
    free_work_plan(&w);

    // start_pos as the product loop sees it, plus two readable pads
    std::vector<int> sp((size_t)h->num_diag + 3, 0);
    for (int d = 0; d <= h->num_diag; ++d)
        sp[(size_t)d] = h->h_start_pos[(size_t)d];
    int diag_limit = h->num_diag;
    if (quirks) {
        // main-cli.c:865 + :1013: diagonals 0 .. ref_num_tjdiag inclusive;
        // main-cli.c:951-966: terminator never written after a one-entry last
        // diagonal, and the malloc'd array reads as zero there.
        if (last_diag_single)
            sp[(size_t)h->num_diag] = 0;
        diag_limit = std::min(h->num_diag, ref_num_tjdiag + 1);
    }
    std::vector<int4> work;
    long long planned = 0;
    for (int d0 = 0; d0 < diag_limit; d0 += smvp::kTjdsDiagChunk) {
        const int d1 = std::min(d0 + smvp::kTjdsDiagChunk, diag_limit);
        const int width = sp[(size_t)d0 + 1] - sp[(size_t)d0];  // widest diagonal of the chunk
        for (int k0 = 0; k0 < width; k0 += smvp::kTjdsBlock)
            work.push_back(make_int4(k0, d0, d1, 0));
        for (int d = d0; d < d1; ++d)
            planned += std::max(0, sp[(size_t)d + 1] - sp[(size_t)d]);
    }
    if (int rc = upload(&w.d_start_pos, sp))
        return rc;
    if (int rc = upload(&w.d_work, work))
        return rc;
    w.nwork = (int)work.size();
    w.quirks = quirks;
    w.planned_nnz = planned;
    return SMVP_OK;
}

// How the row-gather stream names an entry: tile-ordered streams with two 16-bit words per entry -- the low half of the
// position and slot | run hint -- plus the tiles' run tables (kFlavorTjdsH, 4 bytes of index per entry: the default); the same
// order with the 32-bit position and a 32-bit slot | diagonal word (kFlavorTjdsS, 8 bytes; needs the diagonals to fit 21 bits);
// or 32-bit permuted columns in row
// order (kFlavorTjdsK).  The plan option "tjds_index" = 0 | 1 | 2 selects (smvp_set_option; the tests run all three).
int row_gather_index(const smvp_tjds *h)
{
    const int e = smvp::option("tjds_index", 0);
    const bool fits_sorted = ((long long)std::max(h->num_diag - 1, 0) >> (32 - smvp::kSlotBits)) == 0;
    if (e == 2)
        return smvp::kFlavorTjdsK;
    if (e == 1 && fits_sorted)
        return smvp::kFlavorTjdsS;
    return smvp::kFlavorTjdsH;
}

int ensure_row_gather(smvp_tjds *h)
{
    RowGatherPlan &p = h->rg;
    if (p.csr)
        return SMVP_OK;
    free_row_gather(&p);
    const size_t n = (size_t)std::max(h->nnz, 4);
    const int index = row_gather_index(h);
    if (hipMalloc((void **)&p.d_ptr, ((size_t)h->rows + 4) * sizeof(int)) != hipSuccess ||
        hipMalloc((void **)&p.d_pos, n * sizeof(int)) != hipSuccess ||
        (index == smvp::kFlavorTjdsK && hipMalloc((void **)&p.d_k, n * sizeof(int)) != hipSuccess))
        return smvp::fail(SMVP_ERR_ALLOC, "TJDS: cannot allocate the row-gather plan");
    // the true start_pos (the work plan's may carry the ref-quirks edit)
    if (int rc = smvp::build_row_gather_plan(h->d_row_ind, h->d_start_pos, h->num_diag, h->nnz, h->rows, p.d_ptr, p.d_pos, p.d_k, nullptr))
        return rc;
    TjdsSource src;
    src.pos = p.d_pos, src.start_pos = h->d_start_pos, src.num_diag = h->num_diag;
    return smvp::csr_create_tjds(&p.csr, h->device, h->rows, std::max(h->cols, 1), h->nnz, p.d_ptr, p.d_k, h->d_val, index, src);
}

// (buffers kept from a call whose build failed are used again)
int ensure_two_phase(smvp_tjds *h)
{
    TwoPhasePlan &p = h->two;
    if (p.csr)
        return SMVP_OK;
    const size_t n = (size_t)std::max(h->nnz, 4);
    if ((!p.d_prod && hipMalloc((void **)&p.d_prod, n * sizeof(double)) != hipSuccess) ||
        (!p.d_inv_pos && hipMalloc((void **)&p.d_inv_pos, n * sizeof(int)) != hipSuccess) ||
        (!p.d_inv_ptr && hipMalloc((void **)&p.d_inv_ptr, ((size_t)h->rows + 4) * sizeof(int)) != hipSuccess))
        return smvp::fail(SMVP_ERR_ALLOC, "TJDS: cannot allocate the two-phase buffers");
    if (int rc = smvp::build_row_inverse(h->d_row_ind, h->nnz, h->rows, p.d_inv_ptr, p.d_inv_pos, nullptr))
        return rc;
    // the second phase walks the products the way the one-kernel form walks val: every tile's entries in TJDS order (neighbouring
    // lanes read neighbouring products), one 32-bit index word per entry, no operand (round 5; before: a unit-value CSR over the
    // row-inverted index, every product a gather of its own: 0.83 ms on memplus x944)
    TjdsSource src;
    src.pos = p.d_inv_pos, src.start_pos = h->d_start_pos, src.num_diag = h->num_diag, src.unit_operand = true;
    return smvp::csr_create_tjds(&p.csr, h->device, h->rows, std::max(h->cols, 1), h->nnz, p.d_inv_ptr, nullptr, p.d_prod,
                                 smvp::kFlavorTjdsH, src);
}

int ensure_mode_plan(smvp_tjds *h)
{
    switch (h->mode) {
    case SMVP_TJDS_MODE_ROW_GATHER:
        return ensure_row_gather(h);
    case SMVP_TJDS_MODE_TWO_PHASE:
        return ensure_two_phase(h);
    default:
        return SMVP_OK;
    }
}

bool overwrites_y(const smvp_tjds *h) { return h->mode != SMVP_TJDS_MODE_ATOMIC && !h->work.quirks; }

}  // namespace

extern "C" int smvp_tjds_create(smvp_tjds_t **out, int device, int rows, int cols, int nnz, int num_diag,
                                const int *perm, const int *start_pos, const int *row_ind,
                                const double *val, int mem_kind)
{
    if (!out || rows < 0 || cols < 0 || nnz < 0 || num_diag < 0 || !start_pos || (cols > 0 && !perm) ||
        (nnz > 0 && (!row_ind || !val)))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_create: bad argument");
    if (mem_kind != SMVP_MEM_HOST && mem_kind != SMVP_MEM_DEVICE)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_create: bad mem_kind");
    if (nnz > kMaxEntries)
        return smvp::fail(SMVP_ERR_UNSUPPORTED, "smvp_tjds_create: %d entries: shard blocks this large by rows", nnz);
    if (int rc = usable_device(device))
        return rc;
    DeviceScope on(device);

    smvp_tjds *h = new smvp_tjds;
    h->device = device;
    h->rows = rows, h->cols = cols, h->nnz = nnz, h->num_diag = num_diag;
    h->h_start_pos.resize((size_t)num_diag + 1);
    int rc = SMVP_OK;
    if (mem_kind == SMVP_MEM_HOST)
        memcpy(h->h_start_pos.data(), start_pos, sizeof(int) * ((size_t)num_diag + 1));
    else if (hipMemcpy(h->h_start_pos.data(), start_pos, sizeof(int) * ((size_t)num_diag + 1), hipMemcpyDeviceToHost) != hipSuccess)
        rc = smvp::fail(SMVP_ERR_HIP, "smvp_tjds_create: cannot read start_pos back from the device");
    if (rc == SMVP_OK) {
        // diagonals start at 0, end at nnz, and never get longer; the first one
        // has at most `cols` entries -- the kernel's indexing relies on all of it
        const std::vector<int> &sp = h->h_start_pos;
        bool ok = sp[0] == 0 && sp[(size_t)num_diag] == nnz;
        int prev = cols;
        for (int d = 0; d < num_diag && ok; ++d) {
            const int len = sp[(size_t)d + 1] - sp[(size_t)d];
            ok = len >= 1 && len <= prev;
            prev = len;
        }
        if (!ok)
            rc = smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_create: start_pos is not a valid jagged-diagonal index");
    }
    if (rc == SMVP_OK && mem_kind == SMVP_MEM_HOST) {
        for (int j = 0; j < nnz && rc == SMVP_OK; ++j)
            if (row_ind[j] < 0 || row_ind[j] >= rows)
                rc = smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_create: row_ind[%d] = %d outside [0, %d)", j, row_ind[j], rows);
        for (int k = 0; k < cols && rc == SMVP_OK; ++k)
            if (perm[k] < 0 || perm[k] >= cols)
                rc = smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_create: perm[%d] = %d outside [0, %d)", k, perm[k], cols);
    }
    if (rc == SMVP_OK && mem_kind == SMVP_MEM_DEVICE)
        rc = check_device_indices(row_ind, nnz, rows, "smvp_tjds_create: row_ind");
    if (rc == SMVP_OK && mem_kind == SMVP_MEM_DEVICE)
        rc = check_device_indices(perm, cols, cols, "smvp_tjds_create: perm");
    if (rc == SMVP_OK)
        rc = to_device(&h->d_perm, perm, (size_t)cols, mem_kind, &h->own_perm);
    if (rc == SMVP_OK)
        rc = to_device(&h->d_start_pos, start_pos, (size_t)num_diag + 1, mem_kind, &h->own_start_pos);
    if (rc == SMVP_OK)
        rc = to_device(&h->d_row_ind, row_ind, (size_t)nnz, mem_kind, &h->own_row_ind);
    if (rc == SMVP_OK)
        rc = to_device(&h->d_val, val, (size_t)nnz, mem_kind, &h->own_val);
    if (rc == SMVP_OK) {
        const size_t n = (size_t)std::max(std::max(rows, cols), 1);
        if (hipMalloc((void **)&h->d_x_perm, n * sizeof(double)) != hipSuccess ||
            hipMemset(h->d_x_perm, 0, n * sizeof(double)) != hipSuccess)
            rc = smvp::fail(SMVP_ERR_ALLOC, "smvp_tjds_create: cannot allocate the permuted operand");
    }
    const double t0 = wall_ms();
    if (rc == SMVP_OK)
        rc = build_tjds_plan(h, false, 0, 0);
    if (rc == SMVP_OK)
        rc = ensure_mode_plan(h);
    h->plan_build_ms = wall_ms() - t0;
    if (rc != SMVP_OK) {
        smvp_tjds_destroy(h);
        return rc;
    }
    *out = h;
    return SMVP_OK;
}

extern "C" int smvp_tjds_set_mode(smvp_tjds_t *h, int mode)
{
    if (!h || mode < SMVP_TJDS_MODE_AUTO || mode > SMVP_TJDS_MODE_ROW_GATHER)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_set_mode: bad argument");
    DeviceScope on(h->device);
    const int before = h->mode;
    h->mode = mode == SMVP_TJDS_MODE_AUTO ? SMVP_TJDS_MODE_ROW_GATHER : mode;
    const double t0 = wall_ms();
    if (int rc = ensure_mode_plan(h)) {
        h->mode = before;
        return rc;
    }
    h->plan_build_ms += wall_ms() - t0;
    return SMVP_OK;
}

extern "C" int smvp_tjds_set_x(smvp_tjds_t *h, const double *d_x, void *stream)
{
    if (!h || (h->cols > 0 && !d_x))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_set_x: bad argument");
    DeviceScope on(h->device);
    hipError_t e = smvp::launch_tjds_permute(h->d_perm, d_x, h->d_x_perm, h->cols, (hipStream_t)stream);
    if (e != hipSuccess)
        return smvp::fail(SMVP_ERR_HIP, "operand permute launch failed: %s", hipGetErrorString(e));
    h->x_set = true;
    return SMVP_OK;
}

extern "C" int smvp_tjds_zero_y(smvp_tjds_t *h, double *d_y, void *stream)
{
    if (!h || (h->rows > 0 && !d_y))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_zero_y: bad argument");
    if (overwrites_y(h))
        return SMVP_OK;  // the row-gather and two-phase products overwrite y
    DeviceScope on(h->device);
    if (h->rows > 0)
        HIP_TRY(hipMemsetAsync(d_y, 0, sizeof(double) * (size_t)h->rows, (hipStream_t)stream));
    return SMVP_OK;
}

int smvp::tjds_spmv_stamped(smvp_tjds_t *h, double *d_y, void *stream, unsigned long long *stamps)
{
    if (!h || (h->rows > 0 && !d_y))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_spmv: bad argument");
    if (!h->x_set)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_spmv: call smvp_tjds_set_x first");
    const TjdsWorkPlan &w = h->work;
    if (w.quirks && h->rows != h->cols)
        return smvp::fail(SMVP_ERR_UNSUPPORTED, "ref-quirks mode indexes the operand by row and needs a square matrix");
    DeviceScope on(h->device);
    if (!w.quirks && h->mode == SMVP_TJDS_MODE_ROW_GATHER)
        return smvp::csr_spmv_stamped(h->rg.csr, h->d_x_perm, d_y, stream, stamps);
    if (h->mode == SMVP_TJDS_MODE_TWO_PHASE && !w.quirks) {
        hipError_t e1 = smvp::launch_tjds_products(w.d_start_pos, h->d_val, h->d_x_perm, h->two.d_prod, w.d_work, w.nwork, h->cols,
                                                   (hipStream_t)stream);
        if (e1 != hipSuccess)
            return smvp::fail(SMVP_ERR_HIP, "TJDS products launch failed: %s", hipGetErrorString(e1));
        return smvp_csr_spmv(h->two.csr, h->two.d_prod, d_y, stream);
    }
    hipError_t e = smvp::launch_tjds_scatter(w.quirks, w.d_start_pos, h->d_row_ind, h->d_val, h->d_x_perm, d_y, w.d_work, w.nwork,
                                             h->cols, (hipStream_t)stream);
    if (e != hipSuccess)
        return smvp::fail(SMVP_ERR_HIP, "TJDS launch failed: %s", hipGetErrorString(e));
    return SMVP_OK;
}

extern "C" int smvp_tjds_spmv(smvp_tjds_t *h, double *d_y, void *stream)
{
    return smvp::tjds_spmv_stamped(h, d_y, stream, nullptr);
}

// What the solvers on a TJDS handle (K11 to K14, K16, K18, K19, K22) share: the product is smvp_tjds_set_x + smvp_tjds_spmv in the current mode,
// which has to be one that overwrites y and gives the same bits on every run.  The steps are smvp_power.hip's, smvp_cg.hip's and
// smvp_bicgstab.hip's; the solves of K16 and K18 are the caller's plans' (on CSR handles of their own: a TJDS handle has no
// triangular solve; Jacobi needs none).
static smvp::HandleProduct tjds_product(smvp_tjds_t *h, void *stream)
{
    return [h, stream](const double *x, double *y) {
        if (int rc = smvp_tjds_set_x(h, x, stream))
            return rc;
        return smvp_tjds_spmv(h, y, stream);
    };
}

static int refuse_unless_overwrites_y(const char *fn, const smvp_tjds_t *h)
{
    if (!overwrites_y(h))
        return smvp::fail(SMVP_ERR_UNSUPPORTED, "%s: %s", fn, h->work.quirks ? "ref-quirks TJDS indexes the operand by row: it is no product "
                          "of a changing operand" : "ATOMIC mode adds in the order the hardware takes the atomics: the steps would not be reproducible");
    return SMVP_OK;
}

extern "C" int smvp_tjds_power_method(smvp_tjds_t *h, const smvp_power_opts_t *opts, const double *d_x0, double *d_x,
                                      smvp_power_result_t *result, double *lambda_each, double *residual_each, void *stream)
{
    if (int rc = smvp::power_check_args("smvp_tjds_power_method", h, opts, result))
        return rc;
    if (int rc = refuse_unless_overwrites_y("smvp_tjds_power_method", h))
        return rc;
    return smvp::power_run("smvp_tjds_power_method", h->device, h->rows, h->cols, opts, d_x0, d_x, result, lambda_each, residual_each, stream,
                           tjds_product(h, stream));
}

extern "C" int smvp_tjds_cg(smvp_tjds_t *h, const smvp_cg_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                            smvp_cg_result_t *result, double *rr_each, double *sigma_each, void *stream)
{
    if (int rc = smvp::cg_check_args("smvp_tjds_cg", h, opts, result, d_b, smvp::Precond::none, {}))
        return rc;
    if (int rc = refuse_unless_overwrites_y("smvp_tjds_cg", h))
        return rc;
    return smvp::cg_run("smvp_tjds_cg", h->device, h->rows, h->cols, opts, d_b, d_x0, d_x, result, rr_each, sigma_each, stream, tjds_product(h, stream));
}

extern "C" int smvp_tjds_pcg(smvp_tjds_t *h, const smvp_cg_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                             const double *d_m, smvp_pcg_result_t *result, double *rr_each, double *rz_each, double *sigma_each,
                             void *stream)
{
    const smvp::KrylovPrecond M{nullptr, d_m, nullptr};
    if (int rc = smvp::cg_check_args("smvp_tjds_pcg", h, opts, result, d_b, smvp::Precond::diagonal, M))
        return rc;
    if (int rc = refuse_unless_overwrites_y("smvp_tjds_pcg", h))
        return rc;
    return smvp::cg_run("smvp_tjds_pcg", h->device, h->rows, h->cols, opts, d_b, d_x0, d_x, smvp::Precond::diagonal, M, result, rr_each, rz_each,
                        sigma_each, stream, tjds_product(h, stream));
}

extern "C" int smvp_tjds_pcg_tri(smvp_tjds_t *h, const smvp_cg_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                                 smvp_trsv_t *first, const double *d_m, smvp_trsv_t *second, smvp_pcg_result_t *result, double *rr_each,
                                 double *rz_each, double *sigma_each, void *stream)
{
    const smvp::KrylovPrecond M{first, d_m, second};
    if (int rc = smvp::cg_check_args("smvp_tjds_pcg_tri", h, opts, result, d_b, smvp::Precond::stored, M))
        return rc;
    if (int rc = refuse_unless_overwrites_y("smvp_tjds_pcg_tri", h))
        return rc;
    return smvp::cg_run("smvp_tjds_pcg_tri", h->device, h->rows, h->cols, opts, d_b, d_x0, d_x, smvp::Precond::stored, M, result, rr_each, rz_each,
                        sigma_each, stream, tjds_product(h, stream));
}

// K14: the diagonal from the handle's own arrays (the true start_pos, not the ref-quirks edit of the plan; val is read in place).  No
// plan, no x_perm, nothing of the forward product's state is read or written.
extern "C" int smvp_tjds_diagonal(const smvp_tjds_t *h, double *d_diag, void *stream)
{
    if (!h || (h->rows > 0 && !d_diag))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_diagonal: null %s", !h ? "handle" : "d_diag");
    DeviceScope on(h->device);
    const hipError_t e = smvp::launch_tjds_diagonal(h->d_start_pos, h->d_row_ind, h->d_val, h->d_perm, d_diag, h->rows, h->cols,
                                                    h->num_diag, (hipStream_t)stream);
    if (e != hipSuccess)
        return smvp::fail(SMVP_ERR_HIP, "smvp_tjds_diagonal: launch failed: %s", hipGetErrorString(e));
    return SMVP_OK;
}

extern "C" int smvp_tjds_bicgstab(smvp_tjds_t *h, const smvp_bicgstab_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                                  smvp_bicgstab_result_t *result, double *rr_each, double *ss_each, void *stream)
{
    if (int rc = smvp::bicgstab_check_args("smvp_tjds_bicgstab", h, opts, result, d_b))
        return rc;
    if (int rc = refuse_unless_overwrites_y("smvp_tjds_bicgstab", h))
        return rc;
    return smvp::bicgstab_run("smvp_tjds_bicgstab", h->device, h->rows, h->cols, opts, d_b, d_x0, d_x, nullptr, result, rr_each, ss_each, stream,
                              tjds_product(h, stream));
}

extern "C" int smvp_tjds_pbicgstab(smvp_tjds_t *h, const smvp_bicgstab_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                                   smvp_trsv_t *first, const double *d_m, smvp_trsv_t *second, smvp_bicgstab_result_t *result,
                                   double *rr_each, double *ss_each, void *stream)
{
    const smvp::KrylovPrecond M{first, d_m, second};
    if (int rc = smvp::pbicgstab_check_args("smvp_tjds_pbicgstab", h, opts, result, d_b, M))
        return rc;
    if (int rc = refuse_unless_overwrites_y("smvp_tjds_pbicgstab", h))
        return rc;
    return smvp::bicgstab_run("smvp_tjds_pbicgstab", h->device, h->rows, h->cols, opts, d_b, d_x0, d_x, &M, result, rr_each, ss_each, stream,
                              tjds_product(h, stream));
}

extern "C" int smvp_tjds_gmres(smvp_tjds_t *h, const smvp_gmres_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                               smvp_trsv_t *first, const double *d_m, smvp_trsv_t *second, smvp_gmres_result_t *result, double *rr_each,
                               double *restart_each, void *stream)
{
    if (int rc = smvp::gmres_check_args("smvp_tjds_gmres", h, opts, result, d_b))
        return rc;
    if (int rc = refuse_unless_overwrites_y("smvp_tjds_gmres", h))
        return rc;
    return smvp::gmres_run("smvp_tjds_gmres", h->device, h->rows, h->cols, opts, d_b, d_x0, d_x, smvp::KrylovPrecond{first, d_m, second}, result,
                           rr_each, restart_each, stream, tjds_product(h, stream));
}

// K22: the one handle gives both products, A v in the current mode and A^T u by K8 from the same arrays
extern "C" int smvp_tjds_lsqr(smvp_tjds_t *h, const smvp_lsqr_opts_t *opts, const double *d_b, const double *d_x0, double *d_x,
                              smvp_lsqr_result_t *result, double *rnorm_each, double *arnorm_each, void *stream)
{
    if (int rc = smvp::lsqr_check_args("smvp_tjds_lsqr", h, nullptr, false, opts, result, d_b))
        return rc;
    if (int rc = refuse_unless_overwrites_y("smvp_tjds_lsqr", h))
        return rc;
    return smvp::lsqr_run("smvp_tjds_lsqr", h->device, h->rows, h->cols, opts, d_b, d_x0, d_x, result, rnorm_each, arnorm_each, stream,
                          tjds_product(h, stream),
                          [h, stream](const double *x, double *y) { return smvp_tjds_spmv_transposed(h, x, y, stream); });
}

// the row-gather product (which overwrites y) through the owner kernel of `rg`, on the operand of smvp_tjds_set_x
int smvp::tjds_stamp_slots(const smvp_tjds_t *h)
{
    return h && !h->work.quirks && h->mode == SMVP_TJDS_MODE_ROW_GATHER ? smvp::csr_stamp_slots(h->rg.csr) : 0;
}

int smvp::tjds_repeat_grid(const smvp_tjds_t *h) { return smvp::csr_repeat_grid(h->rg.csr); }

int smvp::tjds_spmv_repeat(smvp_tjds_t *h, double *d_y, void *stream, unsigned long long *stamps, int reps, int grid, unsigned *ctl_words,
                           bool first_of_run, unsigned long long patience)
{
    return smvp::csr_spmv_repeat(h->rg.csr, h->d_x_perm, d_y, stream, stamps, reps, grid, ctl_words, first_of_run, patience);
}

// (adds nothing to plan_build_ms)
extern "C" int smvp_tjds_set_ref_quirks(smvp_tjds_t *h, int enable, int ref_num_tjdiag, int last_diag_single)
{
    if (!h || (enable && ref_num_tjdiag < 0))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_set_ref_quirks: bad argument");
    DeviceScope on(h->device);
    return build_tjds_plan(h, enable != 0, ref_num_tjdiag, last_diag_single);
}

extern "C" int smvp_tjds_describe(const smvp_tjds_t *h, char *kernel_name, size_t cap, double *alg_bytes)
{
    if (!h)
        return smvp::fail(SMVP_ERR_INVALID, "null handle");
    if (kernel_name && cap) {
        if (h->work.quirks || h->mode == SMVP_TJDS_MODE_ATOMIC)
            snprintf(kernel_name, cap, "tjds_colmajor_scatter<%s>", h->work.quirks ? "true" : "false");
        else if (h->mode == SMVP_TJDS_MODE_TWO_PHASE)
            snprintf(kernel_name, cap, "tjds_colmajor_products + %s", smvp::csr_owner_kernel_name(h->two.csr).c_str());
        else
            snprintf(kernel_name, cap, "%s", smvp::csr_owner_kernel_name(h->rg.csr).c_str());
    }
    if (alg_bytes)  // (the entries the work plan covers, and no perm: not tjds_matrix_bytes)
        *alg_bytes = 12.0 * h->work.planned_nnz + 4.0 * (h->num_diag + 1.0) + 8.0 * h->cols + 8.0 * h->rows;
    return SMVP_OK;
}

// K8: y = A^T x from the handle's own arrays (the true start_pos, not the ref-quirks edit of the plan) and the caller's x.  No plan,
// no x_perm, nothing of the forward product's state is read or written; every argument is checked before anything is enqueued.
extern "C" int smvp_tjds_spmv_transposed(smvp_tjds_t *h, const double *d_x, double *d_y, void *stream)
{
    if (!h)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_spmv_transposed: null handle");
    if (int rc = check_block_operands("smvp_tjds_spmv_transposed", 1, d_x, 1, h->rows, d_y, 1, h->cols, h->nnz, false))  // x[0 .. rows), y[0 .. cols)
        return rc;
    DeviceScope on(h->device);
    const hipError_t e = smvp::launch_tjds_transposed(h->d_start_pos, h->d_row_ind, h->d_val, h->d_perm, d_x, d_y, h->cols,
                                                      h->num_diag, (hipStream_t)stream);
    if (e != hipSuccess)
        return smvp::fail(SMVP_ERR_HIP, "smvp_tjds_spmv_transposed: launch failed: %s", hipGetErrorString(e));
    return SMVP_OK;
}

extern "C" int smvp_tjds_transposed_describe(const smvp_tjds_t *h, char *kernel_name, size_t cap, double *alg_bytes)
{
    if (!h)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_transposed_describe: null handle");
    if (kernel_name && cap)
        snprintf(kernel_name, cap, "%s", smvp::tjds_transposed_kernel_name());
    if (alg_bytes)
        *alg_bytes = tjds_matrix_bytes(h) + 8.0 * h->rows + 8.0 * h->cols;
    return SMVP_OK;
}

// K9: Y = A^T X for k vectors from the handle's own arrays and the caller's X, as K8 for one: no plan, nothing of the forward
// product's state is read or written; every argument is checked before anything is enqueued.
extern "C" int smvp_tjds_spmm_transposed(smvp_tjds_t *h, int k, const double *d_X, long long ldx, double *d_Y, long long ldy, void *stream)
{
    if (!h)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_spmm_transposed: null handle");
    if (int rc = check_block_operands("smvp_tjds_spmm_transposed", k, d_X, ldx, h->rows, d_Y, ldy, h->cols, h->nnz))  // X(r, v), r < rows; Y(c, v), c < cols
        return rc;
    DeviceScope on(h->device);
    const hipError_t e = smvp::launch_tjds_spmm_transposed(h->d_start_pos, h->d_row_ind, h->d_val, h->d_perm, d_X, ldx, d_Y, ldy,
                                                           h->cols, h->num_diag, k, (hipStream_t)stream);
    if (e != hipSuccess)
        return smvp::fail(SMVP_ERR_HIP, "smvp_tjds_spmm_transposed: launch failed: %s", hipGetErrorString(e));
    return SMVP_OK;
}

extern "C" int smvp_tjds_spmm_transposed_describe(const smvp_tjds_t *h, int k, char *kernel_name, size_t cap, double *alg_bytes)
{
    if (!h)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_spmm_transposed_describe: null handle");
    if (k < 1)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_spmm_transposed_describe: k = %d (need k >= 1)", k);
    if (kernel_name && cap)
        smvp::tjds_spmm_transposed_kernel_name(k, kernel_name, cap);
    if (alg_bytes)
        *alg_bytes = tjds_matrix_bytes(h) + 8.0 * k * ((double)h->rows + h->cols);
    return SMVP_OK;
}

// K10's enqueue, for smvp_tjds_spmm and for K20's steps: the arguments are checked and the handle's device is current.  The first
// call on a handle builds the plan (and synchronises `st`).
static int tjds_spmm_enqueue(smvp_tjds_t *h, int k, const double *d_X, long long ldx, double *d_Y, long long ldy, hipStream_t st)
{
    TjdsSpmmPlan &p = h->spmm;
    if (!p.planned) {
        if (int rc = refuse_capture(st, "smvp_tjds_spmm: the first call on a handle builds its plan and cannot be captured "
                                        "(call it once outside the capture)"))
            return rc;
        const double t0 = wall_ms();
        const size_t n = (size_t)std::max(h->nnz, 4);  // (buffers kept from a call whose build failed are used again)
        if ((!p.d_ptr && hipMalloc((void **)&p.d_ptr, ((size_t)h->rows + 4) * sizeof(int)) != hipSuccess) ||
            (!p.d_pos && hipMalloc((void **)&p.d_pos, n * sizeof(int)) != hipSuccess) ||
            (!p.d_col && hipMalloc((void **)&p.d_col, n * sizeof(int)) != hipSuccess) ||
            (!p.d_order && hipMalloc((void **)&p.d_order, (size_t)std::max(h->rows, 4) * sizeof(int)) != hipSuccess))
            return smvp::fail(SMVP_ERR_ALLOC, "smvp_tjds_spmm: cannot allocate the plan (%d rows, %d entries)", h->rows, h->nnz);
        if (int rc = smvp::build_tjds_spmm_plan(h->d_row_ind, h->d_start_pos, h->d_perm, h->num_diag, h->nnz, h->rows, p.d_ptr, p.d_pos,
                                                p.d_col, p.d_order, st))
            return rc;
        p.planned = true;
        p.build_ms = wall_ms() - t0;
    }
    const hipError_t e = smvp::launch_tjds_spmm(p.d_ptr, p.d_pos, p.d_col, h->d_val, p.d_order, d_X, ldx, d_Y, ldy, h->rows, k, st);
    if (e != hipSuccess)
        return smvp::fail(SMVP_ERR_HIP, "smvp_tjds_spmm: launch failed: %s", hipGetErrorString(e));
    return SMVP_OK;
}

// K10: Y = A X for k vectors from the handle's own arrays (the true start_pos, not the ref-quirks edit) through a plan of its own
// and the caller's X: no x_perm, no mode's plan, no value cache is read or written.  Every argument is checked before anything
// is enqueued; the first call builds the plan (and synchronises `stream`).
extern "C" int smvp_tjds_spmm(smvp_tjds_t *h, int k, const double *d_X, long long ldx, double *d_Y, long long ldy, void *stream)
{
    if (!h)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_spmm: null handle");
    if (int rc = check_block_operands("smvp_tjds_spmm", k, d_X, ldx, h->cols, d_Y, ldy, h->rows, h->nnz))  // X(c, v), c < cols; Y(r, v), r < rows
        return rc;
    DeviceScope on(h->device);
    return tjds_spmm_enqueue(h, k, d_X, ldx, d_Y, ldy, (hipStream_t)stream);
}

// K20: k runs of K12 (d_m == NULL) or K14 around K10's enqueue on all k directions.  K10's bits depend neither on the mode nor on
// ref-quirks, so every handle is accepted; x_perm and the forward product's state are neither read nor written.
extern "C" int smvp_tjds_cg_multi(smvp_tjds_t *h, const smvp_cg_opts_t *opts, int k, const double *d_B, long long ldb, const double *d_X0,
                                  long long ldx0, double *d_X, long long ldx, const double *d_m, smvp_pcg_result_t *results,
                                  double *rr_each, double *rz_each, double *sigma_each, void *stream)
{
    if (int rc = smvp::cg_multi_check_args("smvp_tjds_cg_multi", h, opts, results, d_B))
        return rc;
    return smvp::cg_multi_run("smvp_tjds_cg_multi", h->device, h->rows, h->cols, opts, k, d_B, ldb, d_X0, ldx0, d_X, ldx, d_m, results, rr_each,
                              rz_each, sigma_each, stream, [h, k, stream](const double *X, long long ldX, double *Y, long long ldY) {
                                  return tjds_spmm_enqueue(h, k, X, ldX, Y, ldY, (hipStream_t)stream);
                              });
}

extern "C" int smvp_tjds_spmm_describe(const smvp_tjds_t *h, int k, char *kernel_name, size_t cap, double *alg_bytes, smvp_plan_info_t *plan)
{
    if (!h)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_spmm_describe: null handle");
    if (k < 1)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_spmm_describe: k = %d (need k >= 1)", k);
    if (kernel_name && cap)
        smvp::tjds_spmm_kernel_name(k, kernel_name, cap);
    if (alg_bytes)
        *alg_bytes = tjds_matrix_bytes(h) + 8.0 * k * ((double)h->rows + h->cols);
    if (plan) {
        plan->matrix_bytes = tjds_matrix_bytes(h);
        plan->plan_bytes = h->spmm.planned ? 4.0 * (h->rows + 1.0) + 8.0 * h->nnz + 4.0 * h->rows : 0.0;
        plan->build_ms = h->spmm.planned ? h->spmm.build_ms : 0.0;
    }
    return SMVP_OK;
}

// Which values the one-kernel product keeps a second copy of: those of val lines whose 16 entries belong to
// `min_tiles` tiles or more (0: none -- every value is read from val itself).  Rebuilds the plan.
extern "C" int smvp_tjds_set_value_cache(smvp_tjds_t *h, int min_tiles)
{
    if (!h || !h->rg.csr || min_tiles < 0 || min_tiles > 16)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_set_value_cache: needs the row-gather plan and 0 <= min_tiles <= 16");
    if (!smvp::csr_value_cache(h->rg.csr, nullptr, nullptr))
        return min_tiles == 0 ? (int)SMVP_OK
                              : smvp::fail(SMVP_ERR_UNSUPPORTED, "the value cache belongs to the tile-ordered TJDS stream");
    DeviceScope on(h->device);
    return smvp::csr_replan_value_cache(h->rg.csr, min_tiles);
}

extern "C" int smvp_tjds_get_value_cache(const smvp_tjds_t *h, int *min_tiles, long long *cached_entries)
{
    if (!h)
        return smvp::fail(SMVP_ERR_INVALID, "null handle");
    (void)smvp::csr_value_cache(h->rg.csr, min_tiles, cached_entries);
    return SMVP_OK;
}

extern "C" int smvp_tjds_plan_info(const smvp_tjds_t *h, smvp_plan_info_t *out)
{
    if (!h || !out)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_plan_info: bad argument");
    const double n = h->nnz;
    out->matrix_bytes = tjds_matrix_bytes(h);
    double b = 8.0 * std::max(h->rows, h->cols);             // x_perm
    b += 4.0 * (h->num_diag + 3.0) + 16.0 * h->work.nwork;   // the column-major work items (atomic / two-phase / ref-quirks)
    if (h->rg.csr)
        b += 4.0 * (h->rows + 4.0) + 4.0 * n + (h->rg.d_k ? 4.0 * n : 0.0) + smvp::csr_plan_bytes(h->rg.csr);
    if (h->two.csr)
        b += 8.0 * n + 4.0 * (h->rows + 4.0) + 4.0 * n + smvp::csr_plan_bytes(h->two.csr);
    out->plan_bytes = b;
    out->build_ms = h->plan_build_ms;
    return SMVP_OK;
}

// tile size of the row-gather product (development knob; 256, 1024 or 2048 entries)
extern "C" int smvp_tjds_set_tile(smvp_tjds_t *h, int entries_per_tile)
{
    if (!h || !h->rg.csr)
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_set_tile: the handle has no row-gather plan");
    return smvp_csr_set_kernel(h->rg.csr, SMVP_CSR_KERNEL_STREAM, entries_per_tile);
}

extern "C" void smvp_tjds_destroy(smvp_tjds_t *h)
{
    if (!h)
        return;
    DeviceScope on(h->device);
    free_work_plan(&h->work);
    free_row_gather(&h->rg);
    free_two_phase(&h->two);
    free_tjds_spmm_plan(&h->spmm);
    if (h->own_perm && h->d_perm)
        (void)hipFree(h->d_perm);
    if (h->own_start_pos && h->d_start_pos)
        (void)hipFree(h->d_start_pos);
    if (h->own_row_ind && h->d_row_ind)
        (void)hipFree(h->d_row_ind);
    if (h->own_val && h->d_val)
        (void)hipFree(h->d_val);
    if (h->d_x_perm)
        (void)hipFree(h->d_x_perm);
    delete h;
}
