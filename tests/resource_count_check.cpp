// Stand-alone check of tests/resource_count.cpp's bookkeeping, CPU only: the __real_* functions are fakes over malloc, the
// wrappers are called by name; the memset, copy and synchronise calls the fill switch makes are fakes too, which write the
// malloc block (of exactly the size asked for, so a fill one byte too long is AddressSanitizer's to find).  Built by
// `make resource-check` with -fsanitize=address,undefined and run as its own process by tests/test_resource_count_host.py.
// Exit status 0 and "resource_count_check ok" = pass.
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

extern "C" {
hipError_t __wrap_hipMalloc(void **, size_t);
hipError_t __wrap_hipFree(void *);
hipError_t __wrap_hipHostMalloc(void **, size_t, unsigned int);
hipError_t __wrap_hipHostFree(void *);
hipError_t __wrap_hipStreamCreate(hipStream_t *);
hipError_t __wrap_hipStreamCreateWithFlags(hipStream_t *, unsigned int);
hipError_t __wrap_hipStreamDestroy(hipStream_t);
hipError_t __wrap_hipEventCreate(hipEvent_t *);
hipError_t __wrap_hipEventCreateWithFlags(hipEvent_t *, unsigned int);
hipError_t __wrap_hipEventDestroy(hipEvent_t);
hipError_t __wrap_hipStreamEndCapture(hipStream_t, hipGraph_t *);
hipError_t __wrap_hipGraphDestroy(hipGraph_t);
hipError_t __wrap_hipGraphInstantiate(hipGraphExec_t *, hipGraph_t, hipGraphNode_t *, char *, size_t);
hipError_t __wrap_hipGraphExecDestroy(hipGraphExec_t);
int smvp_test_resources(long long *, int);
int smvp_test_fail_device_alloc(int);
int smvp_test_fail_host_alloc(int);
int smvp_test_fail_stream_create(int);
int smvp_test_fail_event_create(int);
int smvp_test_fill_allocations(int, long long, long long);
void smvp_test_fill_stats(long long[3]);
int smvp_test_probe_fill(size_t, unsigned char *);

// ---- the fake runtime: every object is a malloc block; calls into it are counted
static std::atomic<long long> g_real_calls{0};
static hipError_t fake_new(void **out, size_t size) {
    g_real_calls++;
    *out = malloc(size ? size : 1);
    return *out ? hipSuccess : hipErrorOutOfMemory;
}
static hipError_t fake_delete(void *p) {
    g_real_calls++;
    free(p);
    return hipSuccess;
}
hipError_t __real_hipMalloc(void **p, size_t n) {
    if (n == 0) {
        g_real_calls++;
        *p = nullptr;
        return hipSuccess;
    }
    return fake_new(p, n);
}
hipError_t __real_hipFree(void *p) { return fake_delete(p); }
hipError_t __real_hipHostMalloc(void **p, size_t n, unsigned int) { return fake_new(p, n); }
hipError_t __real_hipHostFree(void *p) { return fake_delete(p); }
hipError_t __real_hipStreamCreate(hipStream_t *s) { return fake_new((void **)s, 8); }
hipError_t __real_hipStreamCreateWithFlags(hipStream_t *s, unsigned int) { return fake_new((void **)s, 8); }
hipError_t __real_hipStreamDestroy(hipStream_t s) { return fake_delete(s); }
hipError_t __real_hipEventCreate(hipEvent_t *e) { return fake_new((void **)e, 8); }
hipError_t __real_hipEventCreateWithFlags(hipEvent_t *e, unsigned int) { return fake_new((void **)e, 8); }
hipError_t __real_hipEventDestroy(hipEvent_t e) { return fake_delete(e); }
hipError_t __real_hipStreamEndCapture(hipStream_t, hipGraph_t *g) { return fake_new((void **)g, 8); }
hipError_t __real_hipGraphDestroy(hipGraph_t g) { return fake_delete(g); }
hipError_t __real_hipGraphInstantiate(hipGraphExec_t *x, hipGraph_t, hipGraphNode_t *, char *, size_t) { return fake_new((void **)x, 8); }
hipError_t __real_hipGraphExecDestroy(hipGraphExec_t x) { return fake_delete(x); }

// ---- what the fill calls directly (it wraps none of these): "device memory" is the malloc block, a memset is pending until
// the next synchronise, and g_fail_memsets > 0 makes that many memsets fail and leave a sticky error behind
static std::atomic<long long> g_memsets{0}, g_syncs{0}, g_pending{0}, g_sticky{0}, g_fail_memsets{0};
static bool memset_fails() {
    if (g_fail_memsets.load() > 0 && g_fail_memsets.fetch_sub(1) > 0) {
        g_sticky = 1;
        return true;
    }
    return false;
}
hipError_t hipMemset(void *p, int value, size_t n) {
    g_memsets++;
    if (memset_fails())
        return hipErrorInvalidValue;
    std::memset(p, value, n);
    g_pending++;
    return hipSuccess;
}
hipError_t hipMemsetD32(hipDeviceptr_t p, int value, size_t count) {
    g_memsets++;
    if (memset_fails())
        return hipErrorInvalidValue;
    for (size_t i = 0; i < count; i++)
        std::memcpy((char *)p + 4 * i, &value, 4);
    g_pending++;
    return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind) {
    std::memcpy(dst, src, n);
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) {
    g_syncs++;
    g_pending = 0;
    return hipSuccess;
}
hipError_t hipGetLastError(void) {
    return g_sticky.exchange(0) ? hipErrorInvalidValue : hipSuccess;
}
}

static int g_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "line %d: CHECK(%s) failed\n", __LINE__, #cond); \
            g_failed++;                                                          \
        }                                                                        \
    } while (0)

enum { LIVE = 0, BYTES = 1, OBTAINS = 2, RELEASES = 3, FOREIGN = 24, REFUSED = 25, N = 26 };
struct Snap {
    long long v[N];
    long long at(int kind, int what) const { return v[4 * kind + what]; }
};
static Snap snap() {
    Snap s;
    CHECK(smvp_test_resources(s.v, N) == N);
    return s;
}

static void balance_and_bytes() {
    const Snap a = snap();
    void *p = nullptr, *q = nullptr, *h = nullptr;
    CHECK(__wrap_hipMalloc(&p, 100) == hipSuccess && p);
    CHECK(__wrap_hipMalloc(&q, 28) == hipSuccess && q);
    CHECK(__wrap_hipHostMalloc(&h, 40, 0) == hipSuccess && h);
    Snap b = snap();
    CHECK(b.at(0, LIVE) == a.at(0, LIVE) + 2 && b.at(0, BYTES) == a.at(0, BYTES) + 128 && b.at(0, OBTAINS) == a.at(0, OBTAINS) + 2);
    CHECK(b.at(1, LIVE) == a.at(1, LIVE) + 1 && b.at(1, BYTES) == a.at(1, BYTES) + 40);
    CHECK(__wrap_hipFree(p) == hipSuccess);
    b = snap();
    CHECK(b.at(0, LIVE) == a.at(0, LIVE) + 1 && b.at(0, BYTES) == a.at(0, BYTES) + 28 && b.at(0, RELEASES) == a.at(0, RELEASES) + 1);
    CHECK(__wrap_hipFree(q) == hipSuccess && __wrap_hipHostFree(h) == hipSuccess);
    b = snap();
    for (int k = 0; k < 6; k++)
        CHECK(b.at(k, LIVE) == a.at(k, LIVE) && b.at(k, BYTES) == a.at(k, BYTES));
    CHECK(b.v[FOREIGN] == a.v[FOREIGN]);
    // a zero-byte allocation gives nullptr: nothing is live, and freeing nullptr counts as nothing
    void *z = (void *)&a;
    CHECK(__wrap_hipMalloc(&z, 0) == hipSuccess && z == nullptr);
    CHECK(__wrap_hipFree(nullptr) == hipSuccess);
    const Snap c = snap();
    CHECK(c.at(0, LIVE) == a.at(0, LIVE) && c.v[FOREIGN] == a.v[FOREIGN] && c.at(0, RELEASES) == b.at(0, RELEASES));
    // a short snapshot writes no more than it was given room for
    long long two[3] = {-7, -7, -7};
    CHECK(smvp_test_resources(two, 2) == N && two[2] == -7 && two[0] == c.v[0]);
    CHECK(smvp_test_resources(nullptr, 0) == N);
}

static void handles() {
    const Snap a = snap();
    hipStream_t s1 = nullptr, s2 = nullptr;
    hipEvent_t e1 = nullptr, e2 = nullptr;
    hipGraph_t g = nullptr;
    hipGraphExec_t x = nullptr;
    CHECK(__wrap_hipStreamCreate(&s1) == hipSuccess && __wrap_hipStreamCreateWithFlags(&s2, 1) == hipSuccess);
    CHECK(__wrap_hipEventCreate(&e1) == hipSuccess && __wrap_hipEventCreateWithFlags(&e2, 2) == hipSuccess);
    CHECK(__wrap_hipStreamEndCapture(s1, &g) == hipSuccess && g);
    CHECK(__wrap_hipGraphInstantiate(&x, g, nullptr, nullptr, 0) == hipSuccess && x);
    Snap b = snap();
    CHECK(b.at(2, LIVE) == a.at(2, LIVE) + 2 && b.at(3, LIVE) == a.at(3, LIVE) + 2 && b.at(4, LIVE) == a.at(4, LIVE) + 1 &&
          b.at(5, LIVE) == a.at(5, LIVE) + 1);
    CHECK(__wrap_hipGraphDestroy(g) == hipSuccess && __wrap_hipGraphExecDestroy(x) == hipSuccess);
    CHECK(__wrap_hipEventDestroy(e1) == hipSuccess && __wrap_hipEventDestroy(e2) == hipSuccess);
    CHECK(__wrap_hipStreamDestroy(s1) == hipSuccess && __wrap_hipStreamDestroy(s2) == hipSuccess);
    b = snap();
    for (int k = 0; k < 6; k++)
        CHECK(b.at(k, LIVE) == a.at(k, LIVE));
    CHECK(b.v[FOREIGN] == a.v[FOREIGN]);
}

static void foreign_frees() {
    const Snap a = snap();
    double mine[4] = {1, 2, 3, 4};      // "a caller's array": never obtained through a wrapper
    const long long real_before = g_real_calls.load();
    CHECK(__wrap_hipFree(mine) == hipSuccess);
    CHECK(__wrap_hipHostFree(mine) == hipSuccess);
    CHECK(__wrap_hipStreamDestroy((hipStream_t)mine) == hipSuccess);
    CHECK(__wrap_hipEventDestroy((hipEvent_t)mine) == hipSuccess);
    CHECK(g_real_calls.load() == real_before);      // none reached the runtime: the array is intact
    CHECK(mine[3] == 4);
    Snap b = snap();
    CHECK(b.v[FOREIGN] == a.v[FOREIGN] + 4);
    // a second free of the same pointer is foreign too; a device pointer is not a pinned one
    void *p = nullptr;
    CHECK(__wrap_hipMalloc(&p, 16) == hipSuccess);
    CHECK(__wrap_hipHostFree(p) == hipSuccess);
    CHECK(snap().v[FOREIGN] == a.v[FOREIGN] + 5 && snap().at(0, LIVE) == a.at(0, LIVE) + 1);
    CHECK(__wrap_hipFree(p) == hipSuccess);
    const long long real_mid = g_real_calls.load();
    CHECK(__wrap_hipFree(p) == hipSuccess);
    CHECK(g_real_calls.load() == real_mid);
    b = snap();
    CHECK(b.v[FOREIGN] == a.v[FOREIGN] + 6 && b.at(0, LIVE) == a.at(0, LIVE) && b.at(0, BYTES) == a.at(0, BYTES));
}

static void nth_failure() {
    const Snap a = snap();
    void *p[5] = {};
    smvp_test_fail_device_alloc(3);
    const long long real_before = g_real_calls.load();
    CHECK(__wrap_hipMalloc(&p[0], 8) == hipSuccess);
    CHECK(__wrap_hipMalloc(&p[1], 8) == hipSuccess);
    p[2] = (void *)&a;
    CHECK(__wrap_hipMalloc(&p[2], 8) == hipErrorOutOfMemory && p[2] == nullptr);
    CHECK(g_real_calls.load() == real_before + 2);  // the refusal did not reach the runtime
    CHECK(__wrap_hipMalloc(&p[3], 8) == hipSuccess);    // once only
    Snap b = snap();
    CHECK(b.v[REFUSED] == a.v[REFUSED] + 1 && b.at(0, LIVE) == a.at(0, LIVE) + 3 && b.at(0, OBTAINS) == a.at(0, OBTAINS) + 4);
    // re-arming, disarming, and one kind's switch leaves the others alone
    smvp_test_fail_device_alloc(1);
    CHECK(__wrap_hipMalloc(&p[4], 8) == hipErrorOutOfMemory);
    smvp_test_fail_device_alloc(2);
    smvp_test_fail_device_alloc(-1);
    CHECK(__wrap_hipMalloc(&p[4], 8) == hipSuccess);
    CHECK(__wrap_hipMalloc(&p[2], 8) == hipSuccess);
    smvp_test_fail_host_alloc(1);
    void *h = nullptr, *d = nullptr;
    CHECK(__wrap_hipMalloc(&d, 8) == hipSuccess);
    CHECK(__wrap_hipHostMalloc(&h, 8, 0) == hipErrorOutOfMemory && h == nullptr);
    CHECK(__wrap_hipHostMalloc(&h, 8, 0) == hipSuccess);
    hipStream_t s = nullptr, s2 = nullptr;
    hipEvent_t e = nullptr, e2 = nullptr;
    smvp_test_fail_stream_create(2);
    smvp_test_fail_event_create(1);
    CHECK(__wrap_hipStreamCreateWithFlags(&s, 0) == hipSuccess && __wrap_hipStreamCreate(&s2) != hipSuccess && s2 == nullptr);
    CHECK(__wrap_hipEventCreateWithFlags(&e, 0) != hipSuccess && e == nullptr && __wrap_hipEventCreate(&e2) == hipSuccess);
    CHECK(__wrap_hipStreamDestroy(s) == hipSuccess && __wrap_hipEventDestroy(e2) == hipSuccess);
    CHECK(__wrap_hipHostFree(h) == hipSuccess && __wrap_hipFree(d) == hipSuccess);
    for (void *q : p)
        CHECK(__wrap_hipFree(q) == hipSuccess);
    b = snap();
    for (int k = 0; k < 6; k++)
        CHECK(b.at(k, LIVE) == a.at(k, LIVE) && b.at(k, BYTES) == a.at(k, BYTES));
    CHECK(b.v[FOREIGN] == a.v[FOREIGN] && b.v[REFUSED] == a.v[REFUSED] + 5);
}

static void threads() {
    const Snap a = snap();
    const int T = 8, ROUNDS = 2000;
    std::atomic<long long> refused{0};
    smvp_test_fail_device_alloc(T * ROUNDS / 2);    // exactly one of the threads meets it
    std::vector<std::thread> pool;
    for (int t = 0; t < T; t++)
        pool.emplace_back([&, t] {
            for (int i = 0; i < ROUNDS; i++) {
                void *p = nullptr;
                hipEvent_t e = nullptr;
                if (__wrap_hipMalloc(&p, (size_t)(t + 1) * 8) != hipSuccess)
                    refused++;
                if (__wrap_hipEventCreate(&e) != hipSuccess)
                    std::abort();
                (void)snap();
                if (__wrap_hipFree(p) != hipSuccess || __wrap_hipEventDestroy(e) != hipSuccess)     // (p is nullptr after the refusal)
                    std::abort();
            }
        });
    for (auto &th : pool)
        th.join();
    const Snap b = snap();
    CHECK(refused.load() == 1 && b.v[REFUSED] == a.v[REFUSED] + 1);
    CHECK(b.at(0, OBTAINS) == a.at(0, OBTAINS) + T * ROUNDS && b.at(0, RELEASES) == a.at(0, RELEASES) + T * ROUNDS - 1);     // (one free of nullptr)
    CHECK(b.at(3, OBTAINS) == a.at(3, OBTAINS) + T * ROUNDS);
    for (int k = 0; k < 6; k++)
        CHECK(b.at(k, LIVE) == a.at(k, LIVE) && b.at(k, BYTES) == a.at(k, BYTES));
    CHECK(b.v[FOREIGN] == a.v[FOREIGN]);
}

struct Fills {
    long long v[3];
    long long done() const { return v[0]; }
    long long bytes() const { return v[1]; }
    long long failed() const { return v[2]; }
};
static Fills fills() {
    Fills f;
    smvp_test_fill_stats(f.v);
    return f;
}

// every byte of p[0..n) is what `mode` puts there (mode 0: the 0xAB the caller wrote into it)
static bool holds(const unsigned char *p, size_t n, int mode) {
    static const unsigned char one[4] = {1, 0, 0, 0};
    for (size_t i = 0; i < n; i++)
        if (p[i] != (mode == 2 ? 0xFF : mode == 1 ? one[i % 4] : 0xAB))
            return false;
    return true;
}

static void fill_off_by_default() {
    const Fills a = fills();
    const long long sets = g_memsets.load(), syncs = g_syncs.load();
    void *p = nullptr, *h = nullptr;
    CHECK(__wrap_hipMalloc(&p, 64) == hipSuccess && __wrap_hipHostMalloc(&h, 64, 0) == hipSuccess);
    unsigned char out[5] = {};
    CHECK(smvp_test_probe_fill(5, out) == 0);
    const Fills b = fills();
    CHECK(b.done() == a.done() && b.bytes() == a.bytes() && b.failed() == a.failed());
    CHECK(g_memsets.load() == sets && g_syncs.load() == syncs);
    CHECK(__wrap_hipFree(p) == hipSuccess && __wrap_hipHostFree(h) == hipSuccess);
    CHECK(smvp_test_fill_allocations(3, 0, -1) == -1 && smvp_test_fill_allocations(-1, 0, -1) == -1);      // unknown modes change nothing
    CHECK(smvp_test_probe_fill(5, out) == 0 && fills().done() == a.done());
}

// the malloc blocks have exactly the size asked for: a fill one byte too long is AddressSanitizer's to find, one too short is holds()'s
static void fill_coverage() {
    const size_t sizes[] = {0, 1, 3, 4, 5, 4096 + 3};
    for (int mode = 1; mode <= 2; mode++) {
        CHECK(smvp_test_fill_allocations(mode, 0, -1) == 0);
        for (size_t n : sizes) {
            const Fills a = fills();
            const long long syncs = g_syncs.load();
            void *p = (void *)&a, *h = nullptr;
            CHECK(__wrap_hipMalloc(&p, n) == hipSuccess && (n == 0) == (p == nullptr));
            CHECK(g_pending.load() == 0);                       // waited for before the wrapper returned
            CHECK(n == 0 || g_syncs.load() == syncs + 1);
            CHECK(holds((const unsigned char *)p, n, mode));
            CHECK(__wrap_hipHostMalloc(&h, n, 0) == hipSuccess && h);
            CHECK(holds((const unsigned char *)h, n, mode));
            const Fills b = fills();
            CHECK(b.done() == a.done() + (n ? 2 : 0) && b.bytes() == a.bytes() + 2 * (long long)n && b.failed() == a.failed());
            CHECK(__wrap_hipFree(p) == hipSuccess && __wrap_hipHostFree(h) == hipSuccess);
            std::vector<unsigned char> out(n + 1, 0x5C);
            CHECK(smvp_test_probe_fill(n, out.data()) == 0 && holds(out.data(), n, mode) && out[n] == 0x5C);
        }
    }
    CHECK(smvp_test_fill_allocations(0, 0, -1) == 0);
    const Fills a = fills();
    unsigned char out[8];
    std::memset(out, 0xAB, sizeof out);
    void *p = nullptr;
    CHECK(__wrap_hipMalloc(&p, 8) == hipSuccess && fills().done() == a.done());     // off again
    CHECK(__wrap_hipFree(p) == hipSuccess);
}

static void fill_leaves_a_refused_allocation_alone() {
    CHECK(smvp_test_fill_allocations(2, 0, -1) == 0);
    const Fills a = fills();
    const long long sets = g_memsets.load();
    void *p = (void *)&a, *h = (void *)&a;
    smvp_test_fail_device_alloc(1);
    smvp_test_fail_host_alloc(1);
    CHECK(__wrap_hipMalloc(&p, 16) == hipErrorOutOfMemory && p == nullptr);
    CHECK(__wrap_hipHostMalloc(&h, 16, 0) == hipErrorOutOfMemory && h == nullptr);
    const Fills b = fills();
    CHECK(b.done() == a.done() && b.failed() == a.failed() && g_memsets.load() == sets);
    CHECK(smvp_test_fill_allocations(0, 0, -1) == 0);
}

static void fill_window() {
    // ordinals count device and pinned obtaining calls, refused ones too, from 0 at the arming call; [2, 4] here
    CHECK(smvp_test_fill_allocations(1, 2, 4) == 0);
    const Fills a = fills();
    void *p[7] = {};
    bool filled[7];
    smvp_test_fail_device_alloc(3);                             // ordinal 3 is refused: it takes its ordinal with it
    for (int i = 0; i < 7; i++) {
        hipError_t e;
        if (i == 1 || i == 4)
            e = __wrap_hipHostMalloc(&p[i], 8, 0);
        else
            e = __wrap_hipMalloc(&p[i], 8);
        CHECK((e == hipSuccess) == (i != 3));                   // the 3rd device call is i = 3 (i = 1 is pinned)
        filled[i] = p[i] && holds((const unsigned char *)p[i], 8, 1);
        if (p[i] && !filled[i])
            std::memset(p[i], 0xAB, 8);
    }
    CHECK(!filled[0] && !filled[1] && filled[2] && !filled[3] && filled[4] && !filled[5] && !filled[6]);
    CHECK(fills().done() == a.done() + 2 && fills().bytes() == a.bytes() + 16);
    for (int i = 0; i < 7; i++)
        CHECK((i == 1 || i == 4 ? __wrap_hipHostFree(p[i]) : __wrap_hipFree(p[i])) == hipSuccess);
    // arming again starts the ordinals again; last < 0 has no upper end; a window of one
    CHECK(smvp_test_fill_allocations(2, 1, 1) == 0);
    void *q[3] = {};
    for (int i = 0; i < 3; i++) {
        CHECK(__wrap_hipMalloc(&q[i], 4) == hipSuccess);
        CHECK(holds((const unsigned char *)q[i], 4, 2) == (i == 1));
        CHECK(__wrap_hipFree(q[i]) == hipSuccess);
    }
    CHECK(smvp_test_fill_allocations(2, 2, -1) == 0);
    for (int i = 0; i < 5; i++) {
        CHECK(__wrap_hipMalloc(&q[0], 4) == hipSuccess);
        CHECK(holds((const unsigned char *)q[0], 4, 2) == (i >= 2));
        CHECK(__wrap_hipFree(q[0]) == hipSuccess);
    }
    CHECK(smvp_test_fill_allocations(0, 0, -1) == 0);
}

static void fill_that_fails() {
    CHECK(smvp_test_fill_allocations(1, 0, -1) == 0);
    const Fills a = fills();
    const Snap s = snap();
    void *p = nullptr;
    g_fail_memsets = 1;
    CHECK(__wrap_hipMalloc(&p, 64) == hipSuccess && p);        // the allocation's own result stands
    CHECK(hipGetLastError() == hipSuccess);                     // the sticky error was read off
    CHECK(g_pending.load() == 0);
    Fills b = fills();
    CHECK(b.failed() == a.failed() + 1 && b.done() == a.done() && b.bytes() == a.bytes());
    CHECK(snap().at(0, LIVE) == s.at(0, LIVE) + 1 && snap().at(0, BYTES) == s.at(0, BYTES) + 64);
    CHECK(__wrap_hipFree(p) == hipSuccess);
    g_fail_memsets = 1;
    CHECK(smvp_test_fill_allocations(2, 0, -1) == 0);
    CHECK(__wrap_hipMalloc(&p, 7) == hipSuccess && p && hipGetLastError() == hipSuccess);
    b = fills();
    CHECK(b.failed() == a.failed() + 2 && b.done() == a.done());
    CHECK(__wrap_hipFree(p) == hipSuccess);
    CHECK(__wrap_hipMalloc(&p, 7) == hipSuccess && holds((const unsigned char *)p, 7, 2));      // the next one is filled as before
    CHECK(__wrap_hipFree(p) == hipSuccess);
    CHECK(smvp_test_fill_allocations(0, 0, -1) == 0);
}

static void fill_from_threads() {
    CHECK(smvp_test_fill_allocations(1, 0, -1) == 0);
    const Fills a = fills();
    const int T = 8, ROUNDS = 500;
    std::atomic<long long> wrong{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < T; t++)
        pool.emplace_back([&, t] {
            for (int i = 0; i < ROUNDS; i++) {
                void *p = nullptr, *h = nullptr;
                const size_t n = (size_t)(t + 1) * 8 + (size_t)(i % 4);
                if (__wrap_hipMalloc(&p, n) != hipSuccess || __wrap_hipHostMalloc(&h, n, 0) != hipSuccess)
                    std::abort();
                if (!holds((const unsigned char *)p, n, 1) || !holds((const unsigned char *)h, n, 1))
                    wrong++;
                (void)fills();
                if (__wrap_hipFree(p) != hipSuccess || __wrap_hipHostFree(h) != hipSuccess)
                    std::abort();
            }
        });
    for (auto &th : pool)
        th.join();
    long long bytes = 0;
    for (int t = 0; t < T; t++)
        for (int i = 0; i < ROUNDS; i++)
            bytes += 2 * ((t + 1) * 8 + i % 4);
    const Fills b = fills();
    CHECK(wrong.load() == 0);
    CHECK(b.done() == a.done() + 2 * T * ROUNDS && b.bytes() == a.bytes() + bytes && b.failed() == a.failed());
    CHECK(smvp_test_fill_allocations(0, 0, -1) == 0);
}

int main() {
    fill_off_by_default();
    balance_and_bytes();
    handles();
    foreign_frees();
    nth_failure();
    threads();
    fill_coverage();
    fill_leaves_a_refused_allocation_alone();
    fill_window();
    fill_that_fails();
    fill_from_threads();
    const Snap end = snap();
    for (int k = 0; k < 6; k++)
        CHECK(end.at(k, LIVE) == 0 && end.at(k, BYTES) == 0);
    if (g_failed) {
        std::fprintf(stderr, "resource_count_check: %d checks failed\n", g_failed);
        return 1;
    }
    std::printf("resource_count_check ok\n");
    return 0;
}
