// Stand-alone check of tests/resource_count.cpp's bookkeeping, CPU only: the __real_* functions are fakes over malloc, the
// wrappers are called by name.  Built by `make resource-check` with -fsanitize=address,undefined and run as its own process
// by tests/test_resource_count_host.py.  Exit status 0 and "resource_count_check ok" = pass.
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
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

int main() {
    balance_and_bytes();
    handles();
    foreign_frees();
    nth_failure();
    threads();
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
