// smvp_cg_common.h -- what the Krylov loops on a handle share (smvp_cg.hip, K12; smvp_bicgstab.hip, K13): the order-defined dot's
// building blocks as include/smvp_amd.h words them, the grid rule of every vector pass, the finite test and the holder of a call's
// workspace.  Everything lives in an unnamed namespace: each of the two files compiles its own copy, device code included.
#pragma once
#include "smvp_engine.h"

#include <hip/hip_runtime.h>

namespace smvp {

namespace {

constexpr int kCgBlock = 256;     // four wavefronts
constexpr int kCgGridCap = 2048;  // workgroups of every vector pass: one grid trip = 2048 * 256 elements
constexpr int kCgTrips = 4;       // trips in flight per lane of a pass that also writes
constexpr int kCgDotTrips = 8;    // ... of the dot's pass, which only reads

__device__ inline bool cg_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// fold256 of the workgroup's 256 accumulators, in every lane; every lane calls it, and twice in a row is fine
__device__ inline double cg_fold256(double c)
{
    __shared__ double s_w[kCgBlock / 64];
#pragma unroll
    for (int h = 32; h > 0; h >>= 1)
        c = c + __shfl_xor(c, h, 64);  // lane 0 ends with c_j + c_{j+h} for h = 32 ... 1 (IEEE addition is commutative)
    __syncthreads();                   // (the last call's readers are done with s_w)
    if ((threadIdx.x & 63) == 0)
        s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// the second level: lane l adds the partials l, l + 256, ... in ascending order, then fold256
__device__ inline double cg_fold_parts(const double *__restrict__ parts, int nparts)
{
    double c = 0.0;
    for (int i = threadIdx.x; i < nparts; i += kCgBlock)
        c = c + parts[i];
    return cg_fold256(c);
}

// a lane's accumulator of a[i] * b[i] over its slots: the terms rounded, added in ascending order
__device__ inline double cg_lane_dot(const double *__restrict__ a, const double *__restrict__ b, int n)
{
    const long long stride = (long long)gridDim.x * kCgBlock;
    long long i = (long long)blockIdx.x * kCgBlock + threadIdx.x;
    double c = 0.0;
    for (; i + (kCgDotTrips - 1) * stride < n; i += kCgDotTrips * stride) {
        double t[kCgDotTrips];
#pragma unroll
        for (int u = 0; u < kCgDotTrips; ++u)
            t[u] = a[i + u * stride] * b[i + u * stride];
#pragma unroll
        for (int u = 0; u < kCgDotTrips; ++u)
            c = c + t[u];
    }
    for (; i < n; i += stride) {
        const double t = a[i] * b[i];
        c = c + t;
    }
    return c;
}

// a call's workspace: freed on every way out, after what the call enqueued has finished.  Status is the loop's status block.
template <class Status>
struct KrylovWork {
    hipStream_t stream = nullptr;
    double *vec = nullptr;    // the loop's vectors
    double *small = nullptr;  // the partials of its dots, the words its launches hand on, the histories
    Status *st = nullptr;     // two blocks, by step parity
    Status *seen = nullptr;   // pinned host memory: where a looked step's block is copied to
    ~KrylovWork()
    {
        (void)hipStreamSynchronize(stream);
        if (seen)
            (void)hipHostFree(seen);
        for (void *v : {(void *)vec, (void *)small, (void *)st})
            if (v)
                (void)hipFree(v);
    }
};

inline int cg_grid(int n)
{
    const long long want = ((long long)n + kCgBlock - 1) / kCgBlock;
    return (int)(want < kCgGridCap ? want : kCgGridCap);
}

}  // namespace

}  // namespace smvp
