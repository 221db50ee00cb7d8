// smvp_lsqr_args.cpp -- K22, host side: the defaults of smvp_lsqr_opts_t and what smvp_csr_lsqr / smvp_tjds_lsqr refuse before they
// make any HIP call (no HIP in this file: it is part of the host-san build, whose driver calls the check as the entry points do).
// The fields are checked the way smvp_cg_common.h's krylov_check_args checks its own, atol as tol.
#include "smvp_common.h"

#include <cstring>
#include <limits>

namespace smvp {

int lsqr_check_args(const char *fn, const void *h, const void *ht, bool needs_ht, const smvp_lsqr_opts_t *o, const void *result,
                    const double *d_b)
{
    const bool no_ht = needs_ht && !ht;
    if (!h || no_ht || !o || !result || !d_b)
        return fail(SMVP_ERR_INVALID, "%s: null %s", fn, !h ? "handle" : no_ht ? "ht (the handle of A^T: smvp_csr_create_transposed makes one)"
                                                         : !o ? "opts" : !result ? "result" : "d_b");
    if (o->struct_size != (unsigned)sizeof(smvp_lsqr_opts_t))
        return fail(SMVP_ERR_INVALID, "%s: smvp_lsqr_opts_t of %u bytes, this library's has %u: initialise it with "
                                      "smvp_lsqr_opts_default and build against this library's header",
                    fn, o->struct_size, (unsigned)sizeof(smvp_lsqr_opts_t));
    const double big = std::numeric_limits<double>::max();
    if (o->max_steps < 1 || o->check_every < 1 || !(o->tol >= 0.0) || !(o->tol <= big) || !(o->atol >= 0.0) || !(o->atol <= big))
        return fail(SMVP_ERR_INVALID, "%s: max_steps = %d, check_every = %d, tol = %g, atol = %g (need max_steps >= 1, check_every >= 1, "
                                      "tol and atol >= 0 and finite)", fn, o->max_steps, o->check_every, o->tol, o->atol);
    return SMVP_OK;
}

}  // namespace smvp

extern "C" void smvp_lsqr_opts_default(smvp_lsqr_opts_t *o)
{
    if (!o)
        return;
    memset(o, 0, sizeof *o);
    o->struct_size = (unsigned)sizeof *o;
    o->max_steps = 100;
    o->check_every = 10;
    o->tol = 1e-10;
    o->atol = 1e-10;
}
