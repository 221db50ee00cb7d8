// smvp_engine.h -- what the timed run (smvp_run.hip) needs of the handles (smvp_engine.hip), without their layout.
#pragma once
#include <hip/hip_runtime.h>

#include "smvp_common.h"

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return smvp::fail(SMVP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace smvp {

// Runs the launches of one call on the handle's device, whatever the caller's current device is.
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    explicit DeviceScope(int device)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != device)
            switched = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceScope()
    {
        if (switched)
            (void)hipSetDevice(prev);
    }
};

int usable_device(int device);

// Per format: the {first, last} tick pairs one stamped product writes (0: the current plan cannot time itself on the device -- see
// StampTimer), the grid of the repeating launch (0: no such form), `reps` products in one launch of it, and one product whose
// launch stamps its window (stamps == nullptr: the plain product).  The TJDS forms multiply the operand of smvp_tjds_set_x.
int csr_stamp_slots(const smvp_csr_t *h);
int csr_repeat_grid(const smvp_csr_t *h);
int csr_spmv_repeat(smvp_csr_t *h, const double *d_x, double *d_y, void *stream, unsigned long long *stamps, int reps, int grid,
                    unsigned *ctl_words, bool first_of_run, unsigned long long patience);
int csr_spmv_stamped(smvp_csr_t *h, const double *d_x, double *d_y, void *stream, unsigned long long *stamps);
int tjds_stamp_slots(const smvp_tjds_t *h);
int tjds_repeat_grid(const smvp_tjds_t *h);
int tjds_spmv_repeat(smvp_tjds_t *h, double *d_y, void *stream, unsigned long long *stamps, int reps, int grid, unsigned *ctl_words,
                     bool first_of_run, unsigned long long patience);
int tjds_spmv_stamped(smvp_tjds_t *h, double *d_y, void *stream, unsigned long long *stamps);

}  // namespace smvp
