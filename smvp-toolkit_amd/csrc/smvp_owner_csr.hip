// smvp_owner_csr.hip -- the plain launches of the owner (tile) kernel's CSR flavours, kFlavorCsr, kFlavorCsr16 and (2048-entry tiles
// only) kFlavorCsr16P, the read-once forms included.  This file is compiled with the max-ILP scheduling strategy (the Makefile's ILPFLAGS), which is all that sets
// it apart from smvp_owner.hip: the kernel is the one of smvp_owner_kernel.h, and launch_csr_stream_owner there prepares `ex`,
// grid and group.
#include "smvp_owner_kernel.h"

namespace smvp {

#ifdef SMVP_PHASE_STAMPS   // the diagnostic build: every flavour is launched from smvp_owner.hip, nothing is instantiated here
hipError_t launch_owner_csr(int, int, const OwnerLaunch &, const OwnerExtra &, unsigned, int, hipStream_t) { return hipErrorInvalidValue; }
#else
hipError_t launch_owner_csr(int vpt, int flavor, const OwnerLaunch &l, const OwnerExtra &ex, unsigned grid_x, int group, hipStream_t stream)
{
    const dim3 grid(grid_x);
#define SMVP_OWNER_ST(K, V, F, S)                                                                                  \
    hipLaunchKernelGGL((K<V, F, S>), grid, dim3(kStreamBlock), 0, stream, l.row_ptr, l.col_ind, l.val, \
                       l.x, l.y, l.tile_row, l.tile_next, l.rows, l.nnz, l.ntiles, group, ex)
#define SMVP_OWNER(K, V, F)               \
    if (vpt == V && flavor == F) {        \
        if (l.stamps)                     \
            SMVP_OWNER_ST(K, V, F, true); \
        else                              \
            SMVP_OWNER_ST(K, V, F, false);\
        return hipGetLastError();         \
    }
#define SMVP_OWNER_ONCE(V, F) SMVP_OWNER(read_once::csr_stream_owner, V, F)
#define SMVP_OWNER_PLAIN(V, F) SMVP_OWNER(csr_stream_owner, V, F)
    if (l.read_once) {  // (the 256-entry tiles have no such form and take the plain one)
        SMVP_OWNER_CSR_WIDE_FORMS(SMVP_OWNER_ONCE)
        SMVP_OWNER_CSR_PACKED_FORMS(SMVP_OWNER_ONCE)
    }
    SMVP_OWNER_CSR_FORMS(SMVP_OWNER_PLAIN)
    SMVP_OWNER_CSR_PACKED_FORMS(SMVP_OWNER_PLAIN)
#undef SMVP_OWNER_PLAIN
#undef SMVP_OWNER_ONCE
#undef SMVP_OWNER
#undef SMVP_OWNER_ST
    return hipErrorInvalidValue;
}
#endif  // SMVP_PHASE_STAMPS

}  // namespace smvp
