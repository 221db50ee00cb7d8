// Test-only: counts the resources libsmvp_amd takes from the HIP runtime and gives back.
//
// Not part of libsmvp_amd.so.  lib/libsmvp_amd_counted.so links the library's own objects plus this unit with the linker's
// --wrap=SYMBOL for every HIP call by which the library obtains or returns a resource (COUNTED_WRAPS in the Makefile): the
// objects' undefined hipMalloc then binds to __wrap_hipMalloc below, and __real_hipMalloc is the runtime's function.  Whatever
// else lives in the process (torch's allocator) calls the runtime directly and is not seen here, so the counters hold the
// library's resources only.  The RCCL communicators of the sharded layer are reached through dlopen()ed pointers, not through
// imported symbols: they are out of scope.
//
// Per kind (device memory, pinned host memory, stream, event, graph, graph exec): live objects, live bytes, calls that obtain,
// calls that release, and a map from handle to size.  A release of something that never came through a wrapper is a FOREIGN
// FREE: it is counted and NOT passed on to the runtime (a caller's adopted array stays intact and the test that found the bug
// can go on to report it).  A release of nullptr is passed on and counted as nothing.
//
// smvp_test_fail_*(nth), for device memory, pinned memory, streams and events: the nth obtaining call of that kind from now on fails once with hipErrorOutOfMemory without reaching
// the runtime (1 = the next one); -1 disarms.  Thread-safe: the sharded layer issues from threads.
//
// smvp_test_fill_allocations(mode, first, last): what a fresh allocation holds.  The library is correct only if every word it
// allocates is written before it is read, or cleared by one of its own memsets; a fresh process usually gets cleared pages, so a
// forgotten write shows only where the allocator hands back used memory.  Armed, every successful hipMalloc / hipHostMalloc of
// the library is filled before the wrapper returns: mode 1 = every 32-bit word 0x00000001 (a tail of 1..3 bytes goes on with
// that word's bytes, 01 00 00), mode 2 = every byte 0xFF, mode 0 = off (the default).  Device memory is filled by the
// runtime's memset and the wrapper waits for it with hipDeviceSynchronize: the library works on non-blocking streams, which do
// not wait for the null stream.  Pinned memory is filled on the host.  first / last: only the obtaining calls (device and
// pinned memory in one sequence, refused ones counted) with these ordinals are filled, counted from 0 at the arming call;
// last < 0 = no upper end, so 0, -1 fills all of them -- a failing scenario is narrowed to one allocation by halving the
// window.  A fill that fails never changes what the allocation returns: it is counted, and the runtime's sticky error is read
// off.  tests/test_gpu_fresh_memory.py.
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstring>
#include <mutex>
#include <unordered_map>

namespace {

enum Kind { kDevice = 0, kPinned, kStream, kEvent, kGraph, kGraphExec, kKinds };

struct State {
    std::mutex mu;
    std::unordered_map<const void *, size_t> live[kKinds];
    long long live_bytes[kKinds] = {};
    long long obtains[kKinds] = {};     // calls of an obtaining wrapper, refused ones included
    long long releases[kKinds] = {};    // calls of a releasing wrapper (a release of nullptr is not counted)
    long long fail_in[kKinds] = {};     // > 0: that many obtaining calls from now, the last of them fails; 0: disarmed
    long long foreign = 0;
    long long refused = 0;
    int fill_mode = 0;                  // 0 off, 1 words of 0x00000001, 2 bytes of 0xFF
    long long fill_first = 0, fill_last = -1;   // the window of ordinals that are filled; last < 0: no upper end
    long long fill_ordinal = 0;         // device and pinned obtaining calls since the arming call
    long long fills = 0, fill_bytes = 0, fill_failed = 0;
};

State &state() {
    static State *s = new State;        // never destroyed: the library's own statics may release after this unit's would be gone
    return *s;
}

// true: this obtaining call is the one to refuse
bool begin_obtain(Kind k, int *fill = nullptr) {
    State &s = state();
    std::lock_guard<std::mutex> lock(s.mu);
    s.obtains[k]++;
    if (fill) {                         // (the ordinal is taken here, with the refusal decided under the same lock)
        const long long ordinal = s.fill_ordinal++;
        *fill = ordinal >= s.fill_first && (s.fill_last < 0 || ordinal <= s.fill_last) ? s.fill_mode : 0;
    }
    if (s.fail_in[k] > 0 && --s.fail_in[k] == 0) {
        s.refused++;
        return true;
    }
    return false;
}

void record(Kind k, const void *p, size_t bytes) {
    if (!p)
        return;
    State &s = state();
    std::lock_guard<std::mutex> lock(s.mu);
    s.live[k][p] = bytes;
    s.live_bytes[k] += (long long)bytes;
}

// true: pass the release on to the runtime
bool begin_release(Kind k, const void *p) {
    State &s = state();
    if (!p)
        return k == kDevice || k == kPinned;    // releasing nothing: counted as nothing; only a free of nullptr is defined, so only that is passed on
    std::lock_guard<std::mutex> lock(s.mu);
    s.releases[k]++;
    auto it = s.live[k].find(p);
    if (it == s.live[k].end()) {
        s.foreign++;
        return false;
    }
    s.live_bytes[k] -= (long long)it->second;
    s.live[k].erase(it);
    return true;
}

void count_fill(size_t bytes, bool ok) {
    State &s = state();
    std::lock_guard<std::mutex> lock(s.mu);
    if (ok) {
        s.fills++;
        s.fill_bytes += (long long)bytes;
    } else {
        s.fill_failed++;
    }
}

const unsigned char kOneWord[4] = {1, 0, 0, 0};    // 0x00000001 as it lies in memory

void fill_device(void *p, size_t bytes, int mode) {
    if (!p || !bytes)
        return;
    hipError_t e;
    if (mode == 2) {
        e = hipMemset(p, 0xFF, bytes);
    } else {
        const size_t words = bytes / 4, tail = bytes % 4;
        e = words ? hipMemsetD32((hipDeviceptr_t)p, 1, words) : hipSuccess;
        if (e == hipSuccess && tail)
            e = hipMemcpy((char *)p + 4 * words, kOneWord, tail, hipMemcpyHostToDevice);
    }
    const hipError_t w = hipDeviceSynchronize();
    if (e != hipSuccess || w != hipSuccess)
        (void)hipGetLastError();        // the allocation succeeded: its caller must not find this error
    count_fill(bytes, e == hipSuccess && w == hipSuccess);
}

void fill_host(void *p, size_t bytes, int mode) {
    if (!p || !bytes)
        return;
    if (mode == 2) {
        std::memset(p, 0xFF, bytes);
    } else {
        for (size_t i = 0; i < bytes; i++)
            ((unsigned char *)p)[i] = kOneWord[i % 4];
    }
    count_fill(bytes, true);
}

int arm(Kind k, int nth) {
    State &s = state();
    std::lock_guard<std::mutex> lock(s.mu);
    s.fail_in[k] = nth > 0 ? nth : 0;
    return 0;
}

}   // namespace

extern "C" {

hipError_t __real_hipMalloc(void **, size_t);
hipError_t __real_hipFree(void *);
hipError_t __real_hipHostMalloc(void **, size_t, unsigned int);
hipError_t __real_hipHostFree(void *);
hipError_t __real_hipStreamCreate(hipStream_t *);
hipError_t __real_hipStreamCreateWithFlags(hipStream_t *, unsigned int);
hipError_t __real_hipStreamDestroy(hipStream_t);
hipError_t __real_hipEventCreate(hipEvent_t *);
hipError_t __real_hipEventCreateWithFlags(hipEvent_t *, unsigned int);
hipError_t __real_hipEventDestroy(hipEvent_t);
hipError_t __real_hipStreamEndCapture(hipStream_t, hipGraph_t *);
hipError_t __real_hipGraphDestroy(hipGraph_t);
hipError_t __real_hipGraphInstantiate(hipGraphExec_t *, hipGraph_t, hipGraphNode_t *, char *, size_t);
hipError_t __real_hipGraphExecDestroy(hipGraphExec_t);

// built with -fvisibility=hidden into the counted library: only the smvp_test_* functions join its exported entry points
#define SMVP_TEST_API __attribute__((visibility("default")))

hipError_t __wrap_hipMalloc(void **ptr, size_t size) {
    int fill = 0;
    if (begin_obtain(kDevice, &fill)) {
        if (ptr)
            *ptr = nullptr;             // as the runtime leaves it when memory runs out
        return hipErrorOutOfMemory;
    }
    const hipError_t e = __real_hipMalloc(ptr, size);
    if (e == hipSuccess && ptr) {
        record(kDevice, *ptr, size);
        if (fill)
            fill_device(*ptr, size, fill);
    }
    return e;
}

hipError_t __wrap_hipFree(void *ptr) {
    return begin_release(kDevice, ptr) ? __real_hipFree(ptr) : hipSuccess;
}

hipError_t __wrap_hipHostMalloc(void **ptr, size_t size, unsigned int flags) {
    int fill = 0;
    if (begin_obtain(kPinned, &fill)) {
        if (ptr)
            *ptr = nullptr;
        return hipErrorOutOfMemory;
    }
    const hipError_t e = __real_hipHostMalloc(ptr, size, flags);
    if (e == hipSuccess && ptr) {
        record(kPinned, *ptr, size);
        if (fill)
            fill_host(*ptr, size, fill);
    }
    return e;
}

hipError_t __wrap_hipHostFree(void *ptr) {
    return begin_release(kPinned, ptr) ? __real_hipHostFree(ptr) : hipSuccess;
}

hipError_t __wrap_hipStreamCreate(hipStream_t *s) {
    if (begin_obtain(kStream))
        return hipErrorOutOfMemory;
    const hipError_t e = __real_hipStreamCreate(s);
    if (e == hipSuccess && s)
        record(kStream, *s, 0);
    return e;
}

hipError_t __wrap_hipStreamCreateWithFlags(hipStream_t *s, unsigned int flags) {
    if (begin_obtain(kStream))
        return hipErrorOutOfMemory;
    const hipError_t e = __real_hipStreamCreateWithFlags(s, flags);
    if (e == hipSuccess && s)
        record(kStream, *s, 0);
    return e;
}

hipError_t __wrap_hipStreamDestroy(hipStream_t s) {
    return begin_release(kStream, s) ? __real_hipStreamDestroy(s) : hipSuccess;
}

hipError_t __wrap_hipEventCreate(hipEvent_t *ev) {
    if (begin_obtain(kEvent))
        return hipErrorOutOfMemory;
    const hipError_t e = __real_hipEventCreate(ev);
    if (e == hipSuccess && ev)
        record(kEvent, *ev, 0);
    return e;
}

hipError_t __wrap_hipEventCreateWithFlags(hipEvent_t *ev, unsigned int flags) {
    if (begin_obtain(kEvent))
        return hipErrorOutOfMemory;
    const hipError_t e = __real_hipEventCreateWithFlags(ev, flags);
    if (e == hipSuccess && ev)
        record(kEvent, *ev, 0);
    return e;
}

hipError_t __wrap_hipEventDestroy(hipEvent_t ev) {
    return begin_release(kEvent, ev) ? __real_hipEventDestroy(ev) : hipSuccess;
}

hipError_t __wrap_hipStreamEndCapture(hipStream_t s, hipGraph_t *graph) {
    (void)begin_obtain(kGraph);         // counted; no switch: the library goes on without a graph where it cannot have one
    const hipError_t e = __real_hipStreamEndCapture(s, graph);
    if (e == hipSuccess && graph)
        record(kGraph, *graph, 0);
    return e;
}

hipError_t __wrap_hipGraphDestroy(hipGraph_t g) {
    return begin_release(kGraph, g) ? __real_hipGraphDestroy(g) : hipSuccess;
}

hipError_t __wrap_hipGraphInstantiate(hipGraphExec_t *exec, hipGraph_t g, hipGraphNode_t *err_node, char *log, size_t log_size) {
    (void)begin_obtain(kGraphExec);
    const hipError_t e = __real_hipGraphInstantiate(exec, g, err_node, log, log_size);
    if (e == hipSuccess && exec)
        record(kGraphExec, *exec, 0);
    return e;
}

hipError_t __wrap_hipGraphExecDestroy(hipGraphExec_t exec) {
    return begin_release(kGraphExec, exec) ? __real_hipGraphExecDestroy(exec) : hipSuccess;
}

// out[4 * kind + 0..3] = live objects, live bytes, obtaining calls, releasing calls (kinds in the order of the enum above);
// out[24] = foreign frees, out[25] = calls refused by a switch.  Returns the number of values a full snapshot has (26); writes
// at most n of them.
SMVP_TEST_API int smvp_test_resources(long long *out, int n) {
    State &s = state();
    std::lock_guard<std::mutex> lock(s.mu);
    long long v[4 * kKinds + 2];
    for (int k = 0; k < kKinds; k++) {
        v[4 * k + 0] = (long long)s.live[k].size();
        v[4 * k + 1] = s.live_bytes[k];
        v[4 * k + 2] = s.obtains[k];
        v[4 * k + 3] = s.releases[k];
    }
    v[4 * kKinds] = s.foreign;
    v[4 * kKinds + 1] = s.refused;
    for (int i = 0; out && i < n && i < 4 * kKinds + 2; i++)
        out[i] = v[i];
    return 4 * kKinds + 2;
}

SMVP_TEST_API int smvp_test_fail_device_alloc(int nth) { return arm(kDevice, nth); }
SMVP_TEST_API int smvp_test_fail_host_alloc(int nth) { return arm(kPinned, nth); }
SMVP_TEST_API int smvp_test_fail_stream_create(int nth) { return arm(kStream, nth); }
SMVP_TEST_API int smvp_test_fail_event_create(int nth) { return arm(kEvent, nth); }

// mode 0 / 1 / 2 as at the head of this file; the ordinals start again at 0.  Returns 0, or -1 for a mode it does not know
// (nothing changes then).
SMVP_TEST_API int smvp_test_fill_allocations(int mode, long long first, long long last) {
    if (mode < 0 || mode > 2)
        return -1;
    State &s = state();
    std::lock_guard<std::mutex> lock(s.mu);
    s.fill_mode = mode;
    s.fill_first = first;
    s.fill_last = last;
    s.fill_ordinal = 0;
    return 0;
}

// out[0..2] = fills done, bytes filled, fills failed, since the process began
SMVP_TEST_API void smvp_test_fill_stats(long long out[3]) {
    State &s = state();
    std::lock_guard<std::mutex> lock(s.mu);
    out[0] = s.fills;
    out[1] = s.fill_bytes;
    out[2] = s.fill_failed;
}

// What an allocation of `bytes` holds when the library gets it: allocates through the wrapper, copies the content to host_out
// (room for `bytes`), frees through the wrapper.  Returns the first HIP error met, 0 = none.
SMVP_TEST_API int smvp_test_probe_fill(size_t bytes, unsigned char *host_out) {
    void *p = nullptr;
    hipError_t e = __wrap_hipMalloc(&p, bytes);
    if (e != hipSuccess)
        return (int)e;
    if (p && bytes && host_out)
        e = hipMemcpy(host_out, p, bytes, hipMemcpyDeviceToHost);
    const hipError_t f = __wrap_hipFree(p);
    return (int)(e != hipSuccess ? e : f);
}

}   // extern "C"
