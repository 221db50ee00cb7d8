// smvp_run.hip -- the device queries and the two reference-shaped compute entry points.
//
//   smvp_csr_compute   replaces main-cli.c:325-469
//   smvp_tjds_compute  replaces main-cli.c:734-1162
// The timed iteration loop (main-cli.c:402-420, :1004-1024) with hipEvents, or the kernel's own stamps, in place of
// clock_gettime.  The handles are smvp_engine.hip's: this file creates them through the C ABI and times their products
// through smvp_engine.h.
#include "smvp_engine.h"
#include "smvp_kernels.h"

#include <algorithm>
#include <cstring>
#include <ctime>
#include <vector>

// ===========================================================================
// device queries
// ===========================================================================
extern "C" int smvp_device_count(int *count)
{
    if (!count)
        return smvp::fail(SMVP_ERR_INVALID, "null argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        n = 0;
    *count = n;
    return SMVP_OK;
}

extern "C" int smvp_device_info(int device, char *name, size_t name_cap, int *compute_units, size_t *hbm_bytes)
{
    if (int rc = smvp::usable_device(device))
        return rc;
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, device));
    if (name && name_cap) {
        if (p.name[0])
            snprintf(name, name_cap, "%s (%s)", p.name, p.gcnArchName);
        else  // some driver stacks leave the marketing name empty
            snprintf(name, name_cap, "%s", p.gcnArchName);
    }
    if (compute_units)
        *compute_units = p.multiProcessorCount;
    if (hbm_bytes)
        *hbm_bytes = p.totalGlobalMem;
    return SMVP_OK;
}

// ===========================================================================
// reference-shaped entry points
// ===========================================================================
extern "C" void smvp_run_opts_default(smvp_run_opts_t *o)
{
    if (!o)
        return;
    memset(o, 0, sizeof *o);
    o->struct_size = (unsigned)sizeof *o;
    o->shard_exchange = SMVP_EXCHANGE_AUTO;
    o->csr_kernel = SMVP_CSR_KERNEL_AUTO;
    o->tjds_mode = SMVP_TJDS_MODE_AUTO;
    o->timing = SMVP_TIMING_AUTO;
}

namespace {

constexpr int kEventRing = 1024;

// Scope guard for the scratch the two entry points allocate.
struct RunScratch {
    std::vector<double> ms;   // per-product times, filled as the event ring is drained
    double *d_x = nullptr, *d_y = nullptr;
    double *d_result = nullptr;                          // where the last product was written (d_x or d_y when iterating)
    unsigned long long *d_norm = nullptr;                // scratch of the normalisation
    void *d_coo = nullptr;                               // convert_on_device: the uploaded COO
    int *d_i0 = nullptr, *d_i1 = nullptr, *d_i2 = nullptr;  // ... and the arrays built from it
    double *d_v = nullptr;
    std::vector<hipEvent_t> ev;
    hipStream_t stream = nullptr;
    smvp_csr_t *csr = nullptr;
    smvp_tjds_t *tjds = nullptr;
    ~RunScratch()
    {
        for (hipEvent_t e : ev)
            (void)hipEventDestroy(e);
        if (d_norm)
            (void)hipFree(d_norm);
        if (d_x)
            (void)hipFree(d_x);
        if (d_y)
            (void)hipFree(d_y);
        if (stream)
            (void)hipStreamDestroy(stream);
        smvp_csr_destroy(csr);
        smvp_tjds_destroy(tjds);
        for (void *p : {d_coo, (void *)d_i0, (void *)d_i1, (void *)d_i2, (void *)d_v})
            if (p)
                (void)hipFree(p);
    }
};

int prepare_run(RunScratch &s, int rows, int cols, int iters, const smvp_run_opts_t *o)
{
    HIP_TRY(hipStreamCreate(&s.stream));
    HIP_TRY(hipMalloc((void **)&s.d_x, sizeof(double) * (size_t)std::max(std::max(cols, rows), 1)));
    HIP_TRY(hipMalloc((void **)&s.d_y, sizeof(double) * (size_t)std::max(std::max(cols, rows), 1)));
    HIP_TRY(hipMalloc((void **)&s.d_norm, sizeof(unsigned long long)));
    s.d_result = s.d_y;
    if (o->x) {
        HIP_TRY(hipMemcpy(s.d_x, o->x, sizeof(double) * (size_t)cols, hipMemcpyHostToDevice));
    } else {
        // vectorInit(rows, onesVector, 1), main-cli.c:368-369 / :761-762
        hipError_t e = smvp::launch_fill(s.d_x, 1.0, std::max(cols, rows), s.stream);
        if (e != hipSuccess)
            return smvp::fail(SMVP_ERR_HIP, "fill launch failed: %s", hipGetErrorString(e));
    }
    // a ring of event pairs, drained every kEventRing products: -n may be in the millions
    s.ev.assign((size_t)std::min(iters, kEventRing) * 2, nullptr);
    for (auto &e : s.ev)
        HIP_TRY(hipEventCreate(&e));
    s.ms.assign((size_t)iters, 0.0);
    return SMVP_OK;
}

// events of product i
inline hipEvent_t &ev_start(RunScratch &s, int i) { return s.ev[(size_t)2 * (i % kEventRing)]; }
inline hipEvent_t &ev_stop(RunScratch &s, int i) { return s.ev[(size_t)2 * (i % kEventRing) + 1]; }

// after product i has been enqueued: when the ring is full (or i is the last product) wait and read it out
int drain_ring(RunScratch &s, int i, int iters)
{
    if ((i + 1) % kEventRing != 0 && i + 1 != iters)
        return SMVP_OK;
    HIP_TRY(hipStreamSynchronize(s.stream));
    for (int k = i - (i % kEventRing); k <= i; ++k) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev_start(s, k), ev_stop(s, k)));
        s.ms[(size_t)k] = (double)ms;
    }
    return SMVP_OK;
}

int finish_run(RunScratch &s, int rows, int iters, double *y, double *time_each_ms, smvp_time_stats_t *stats)
{
    HIP_TRY(hipStreamSynchronize(s.stream));
    if (time_each_ms)
        memcpy(time_each_ms, s.ms.data(), sizeof(double) * (size_t)iters);
    if (stats)
        smvp_time_stats(s.ms.data(), iters, stats);
    if (rows > 0)
        HIP_TRY(hipMemcpy(y, s.d_result, sizeof(double) * (size_t)rows, hipMemcpyDeviceToHost));
    return SMVP_OK;
}

int check_iterate(const smvp_run_opts_t *o, int rows, int cols)
{
    if (o->struct_size != (unsigned)sizeof(smvp_run_opts_t))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_run_opts_t of %u bytes, this library's has %u: initialise it with "
                                            "smvp_run_opts_default and build against this library's header",
                          o->struct_size, (unsigned)sizeof(smvp_run_opts_t));
    if (o->iterate && rows != cols)
        return smvp::fail(SMVP_ERR_INVALID, "power iteration needs a square matrix (%d x %d given)", rows, cols);
    if (o->timing < SMVP_TIMING_AUTO || o->timing > SMVP_TIMING_DEVICE_GRAPH)
        return smvp::fail(SMVP_ERR_INVALID, "unknown timing method %d", o->timing);
    return SMVP_OK;
}

thread_local smvp_run_info_t g_last_run = {SMVP_TIMING_EVENTS, 0, 0.0, 0.0, 0, 0};

double host_ms()
{
    timespec t;
    clock_gettime(CLOCK_MONOTONIC_RAW, &t);  // the reference's clock, main-cli.c:408
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

// Per-product times of launches too short for an event pair to time.  The reference brackets its product with
// clock_gettime (main-cli.c:408-419): nothing but the product is inside the window.  A hipEvent pair around a launch
// of a few microseconds measures mostly the events themselves (an empty launch between two events reads 6.6 us on
// MI355X, memplus.mtx's CSR kernel runs 3.8 us), so for such launches the kernel times itself: every wave writes the
// constant-rate wall clock when it starts and when its last store has been acknowledged, stamp_reduce takes
// max(last) - min(first) per product.  The products of a run are captured into one hipGraph (kStampRing products per
// replay, their timing slots baked into the nodes) so that the host's launch rate is not what the run waits for.
constexpr int kStampRing = 256;        // products per graph replay (even: power iteration swaps x and y)
constexpr int kStampMaxSlots = 16384;  // waves per launch up to which the kernel times itself (4096 workgroups)

struct StampTimer {
    unsigned long long *d_stamps = nullptr, *d_first_last = nullptr;
    unsigned *d_ctl = nullptr;  // the repeating launch's barrier counters
    hipGraphExec_t exec = nullptr;
    int exec_n = 0;
    ~StampTimer()
    {
        if (exec)
            (void)hipGraphExecDestroy(exec);
        if (d_stamps)
            (void)hipFree(d_stamps);
        if (d_first_last)
            (void)hipFree(d_first_last);
        if (d_ctl)
            (void)hipFree(d_ctl);
    }
};

// `iters` products on s.stream, each timed on its own.  pre(y): work the reference keeps outside its window (clearing
// y); product(x, y, stamps): the launches of one product.  stamp_slots > 0: the product can time itself on the device.
// repeat_grid > 0: the product has a repeating form -- repeat(x, y, stamps, reps, grid, ctl_words) enqueues `reps` products as
// ONE launch that stamps every product's window (needs no `pre`); used for device-timed runs unless SMVP_TIMING_DEVICE_GRAPH asks
// for one launch per product.
template <class Pre, class Product, class Repeat>
int run_timed_products(RunScratch &s, int rows, int iters, const smvp_run_opts_t *o, int stamp_slots, Pre pre, Product product,
                       int repeat_grid, Repeat repeat)
{
    double *xc = s.d_x, *yc = s.d_y;
    const bool device_asked = o->timing == SMVP_TIMING_DEVICE || o->timing == SMVP_TIMING_DEVICE_GRAPH;
    const bool stamped = o->timing != SMVP_TIMING_EVENTS && !o->iterate && stamp_slots > 0 && (device_asked || stamp_slots <= kStampMaxSlots);
    if (device_asked && !stamped)
        return smvp::fail(SMVP_ERR_UNSUPPORTED, "device-side timing needs the tile kernel of one GPU, a matrix with rows and no --iterate");
    g_last_run.timing = stamped ? SMVP_TIMING_DEVICE : SMVP_TIMING_EVENTS;
    g_last_run.graph_replays = 0;
    g_last_run.repeat_launches = 0;
    g_last_run.repeat_gave_up = 0;
    const unsigned long long patience = smvp::repeat_patience_ticks(o->repeat_patience_us);
    HIP_TRY(hipStreamSynchronize(s.stream));
    const double t0 = host_ms();
    bool repeated = false;
    int khz = 0;
    if (stamped) {
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev));
        if (khz <= 0)
            return smvp::fail(SMVP_ERR_HIP, "the device reports no wall-clock rate");
        g_last_run.device_clock_khz = khz;
    }
    if (stamped && repeat_grid > 0 && o->timing != SMVP_TIMING_DEVICE_GRAPH) {
        // Up to kRepeatRing products per launch of the repeating kernel, the launches of a run enqueued one behind the other:
        // every launch's windows are reduced on the device into first_last[product] and its give-up word is set aside; the
        // host waits once per kRepeatSuper products -- and once for the FIRST launch of the run, before it queues any other.  A
        // launch that gave up at one of its barriers (the grid was not resident as a whole: another stream, thread or process on
        // the device -- the occupancy query the grid was sized from knows nothing of those) sends the whole run to the single
        // launches below: it has waited `repeat_patience_us` (50 ms) at most, and launches queued behind it read the run's
        // sticky give-up word and leave as they start.
        constexpr int kRepeatRing = 1024, kRepeatSuper = 1 << 20;
        StampTimer st;
        unsigned *d_tops = nullptr;
        const int slots = repeat_grid * (smvp::kStreamBlock / 64);
        const size_t per_product = (size_t)slots * 2;
        int ring = std::min(iters, kRepeatRing);
        while (ring > 64 && sizeof(unsigned long long) * per_product * (size_t)ring > (64u << 20))
            ring /= 2;  // (stamps of one launch: at most 64 MB)
        const int super = std::min(iters, kRepeatSuper), launches_per_super = (super + ring - 1) / ring;
        HIP_TRY(hipMalloc((void **)&st.d_stamps, sizeof(unsigned long long) * per_product * (size_t)ring));
        HIP_TRY(hipMalloc((void **)&st.d_first_last, sizeof(unsigned long long) * 2 * (size_t)super + sizeof(unsigned) * (size_t)launches_per_super));
        HIP_TRY(hipMalloc((void **)&st.d_ctl, sizeof(unsigned) * smvp::kRepeatCtlWords));
        d_tops = reinterpret_cast<unsigned *>(st.d_first_last + 2 * (size_t)super);
        std::vector<unsigned long long> fl((size_t)super * 2);
        std::vector<unsigned> tops((size_t)launches_per_super);
        repeated = true;
        for (int s0 = 0; s0 < iters && repeated; s0 += super) {
            const int ns = std::min(super, iters - s0);
            int launches = 0;
            for (int i0 = 0; i0 < ns; i0 += ring, ++launches) {
                const int n = std::min(ring, ns - i0);
                const bool first_of_run = s0 == 0 && i0 == 0;
                if (int rc = repeat(xc, yc, st.d_stamps, n, repeat_grid, st.d_ctl, first_of_run, patience))
                    return rc;
                HIP_TRY(smvp::launch_stamp_reduce(st.d_stamps, slots, n, st.d_first_last + 2 * (size_t)i0, s.stream));
                HIP_TRY(hipMemcpyAsync(d_tops + launches, st.d_ctl + smvp::kRepeatCtlWords - 32, sizeof(unsigned), hipMemcpyDeviceToDevice, s.stream));
                if (first_of_run && ns > n) {  // more launches would follow: has this one held?
                    HIP_TRY(hipMemcpyAsync(tops.data(), d_tops, sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
                    HIP_TRY(hipStreamSynchronize(s.stream));
                    if (tops[0] & 0x80000000u) {
                        repeated = false;
                        break;
                    }
                }
            }
            if (!repeated)
                break;
            HIP_TRY(hipMemcpyAsync(fl.data(), st.d_first_last, sizeof(unsigned long long) * 2 * (size_t)ns, hipMemcpyDeviceToHost, s.stream));
            HIP_TRY(hipMemcpyAsync(tops.data(), d_tops, sizeof(unsigned) * (size_t)launches, hipMemcpyDeviceToHost, s.stream));
            HIP_TRY(hipStreamSynchronize(s.stream));
            for (int l = 0; l < launches; ++l)
                if (tops[(size_t)l] & 0x80000000u)
                    repeated = false;  // gave up at a barrier: nothing of this run is trusted
            if (!repeated)
                break;
            g_last_run.repeat_launches += launches;
            for (int k = 0; k < ns; ++k)
                s.ms[(size_t)(s0 + k)] = (double)(fl[2 * (size_t)k + 1] - fl[2 * (size_t)k]) / (double)khz;
        }
        if (!repeated) {
            g_last_run.repeat_launches = 0;
            g_last_run.repeat_gave_up = 1;
        }
        s.d_result = yc;
    }
    if (stamped && !repeated) {
        StampTimer st;
        const size_t per_product = (size_t)stamp_slots * 2;
        const int ring = std::min(iters, kStampRing);
        HIP_TRY(hipMalloc((void **)&st.d_stamps, sizeof(unsigned long long) * per_product * (size_t)ring));
        HIP_TRY(hipMalloc((void **)&st.d_first_last, sizeof(unsigned long long) * 2 * (size_t)ring));
        std::vector<unsigned long long> fl((size_t)ring * 2);
        bool use_graph = true;
        for (int i0 = 0; i0 < iters; i0 += ring) {
            const int n = std::min(ring, iters - i0);
            auto enqueue = [&]() -> int {
                for (int k = 0; k < n; ++k) {
                    if (int rc = pre(yc))
                        return rc;
                    if (int rc = product(xc, yc, st.d_stamps + per_product * (size_t)k))
                        return rc;
                }
                return SMVP_OK;
            };
            if (use_graph && st.exec_n != n) {
                if (st.exec)
                    (void)hipGraphExecDestroy(st.exec);
                st.exec = nullptr;
                st.exec_n = 0;
                hipGraph_t graph = nullptr;
                bool ok = hipStreamBeginCapture(s.stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
                int rc = ok ? enqueue() : SMVP_OK;
                if (ok)
                    ok = hipStreamEndCapture(s.stream, &graph) == hipSuccess && graph && rc == SMVP_OK;
                if (ok)
                    ok = hipGraphInstantiate(&st.exec, graph, nullptr, nullptr, 0) == hipSuccess;
                if (graph)
                    (void)hipGraphDestroy(graph);
                if (rc != SMVP_OK)
                    return rc;
                if (!ok) {  // no graph support for this sequence: plain launches, still timed on the device
                    (void)hipGetLastError();
                    st.exec = nullptr;
                    use_graph = false;
                } else {
                    st.exec_n = n;
                }
            }
            if (use_graph) {
                HIP_TRY(hipGraphLaunch(st.exec, s.stream));
                ++g_last_run.graph_replays;
            } else if (int rc = enqueue()) {
                return rc;
            }
            HIP_TRY(smvp::launch_stamp_reduce(st.d_stamps, stamp_slots, n, st.d_first_last, s.stream));
            HIP_TRY(hipMemcpyAsync(fl.data(), st.d_first_last, sizeof(unsigned long long) * 2 * (size_t)n,
                                   hipMemcpyDeviceToHost, s.stream));
            HIP_TRY(hipStreamSynchronize(s.stream));
            for (int k = 0; k < n; ++k)
                s.ms[(size_t)(i0 + k)] = (double)(fl[2 * (size_t)k + 1] - fl[2 * (size_t)k]) / (double)khz;
        }
        s.d_result = yc;
    } else if (!stamped) {
        for (int i = 0; i < iters; ++i) {
            if (int rc = pre(yc))
                return rc;
            HIP_TRY(hipEventRecord(ev_start(s, i), s.stream));
            if (int rc = product(xc, yc, nullptr))
                return rc;
            HIP_TRY(hipEventRecord(ev_stop(s, i), s.stream));
            if (o->iterate && o->normalize)  // scaling the iterate is not part of the product: outside the window,
                HIP_TRY(smvp::launch_normalize_max(yc, rows, s.d_norm, s.stream));  // on one GPU and on several alike
            if (int rc = drain_ring(s, i, iters))
                return rc;
            s.d_result = yc;
            if (o->iterate)
                std::swap(xc, yc);  // x_{k+1} = y_k
        }
    }
    HIP_TRY(hipStreamSynchronize(s.stream));
    g_last_run.wall_ms = host_ms() - t0;
    return SMVP_OK;
}

}  // namespace

extern "C" int smvp_last_run_info(smvp_run_info_t *out)
{
    if (!out)
        return smvp::fail(SMVP_ERR_INVALID, "null argument");
    *out = g_last_run;
    return SMVP_OK;
}

// opts.ngpus > 1: the same timed loop over row blocks on several GPUs; the window is the local products
// plus the all-gather of y, the longest GPU counts (smvp_sharded.hip)
static int sharded_compute(bool tjds, const smvp_coo_t *coo, int rows, int cols, int nnz, int iters,
                           const smvp_run_opts_t *o, double *y, double *time_each_ms, smvp_time_stats_t *stats)
{
    if (o->timing == SMVP_TIMING_DEVICE || o->timing == SMVP_TIMING_DEVICE_GRAPH)  // the in-kernel stamps time one launch of one GPU; a sharded product is several
        return smvp::fail(SMVP_ERR_UNSUPPORTED, "device-side timing is not available with more than one GPU (use events)");
    smvp_sharded_t *h = nullptr;
    smvp_shard_opts_t so;
    smvp_shard_opts_default(&so);
    so.exchange = o->shard_exchange;
    int rc;
    if (tjds) {
        rc = smvp_tjds_sharded_create_ex(&h, o->ngpus, nullptr, coo, rows, cols, nnz, &so);
    } else {
        std::vector<int> row_ptr((size_t)rows + 1), col_ind((size_t)std::max(nnz, 1));
        std::vector<double> val((size_t)std::max(nnz, 1));
        rc = smvp_csr_from_coo(coo, rows, nnz, row_ptr.data(), col_ind.data(), val.data());
        if (rc == SMVP_OK)
            rc = smvp_csr_sharded_create_ex(&h, o->ngpus, nullptr, rows, cols, nnz, row_ptr.data(), col_ind.data(), val.data(), &so);
    }
    std::vector<double> local;
    if (!time_each_ms) {
        local.resize((size_t)iters);
        time_each_ms = local.data();
    }
    if (rc == SMVP_OK && !tjds && (o->csr_kernel != SMVP_CSR_KERNEL_AUTO || o->csr_param != 0))
        rc = smvp_sharded_set_csr_kernel(h, o->csr_kernel, o->csr_param);
    if (rc == SMVP_OK)
        rc = smvp_sharded_set_x(h, o->x);
    for (int i = 0; rc == SMVP_OK && i < iters; ++i) {
        rc = smvp_sharded_spmv(h, SMVP_GATHER_OVERLAPPED, 1);
        if (rc == SMVP_OK)
            rc = smvp_sharded_synchronize(h, &time_each_ms[i]);
        if (rc == SMVP_OK && o->iterate && (i + 1 < iters || o->normalize))
            rc = smvp_sharded_feed_back(h, o->normalize);  // the gathered y is the next operand on every GPU
    }
    if (rc == SMVP_OK)
        rc = smvp_sharded_get_y(h, 0, 1, y);
    if (rc == SMVP_OK && stats)
        smvp_time_stats(time_each_ms, iters, stats);
    smvp_sharded_destroy(h);
    return rc;
}

extern "C" int smvp_csr_compute(const smvp_coo_t *coo, int rows, int cols, int nnz, int iters,
                                const smvp_run_opts_t *opts, double *y, double *time_each_ms,
                                smvp_time_stats_t *stats)
{
    smvp_run_opts_t def;
    smvp_run_opts_default(&def);
    const smvp_run_opts_t *o = opts ? opts : &def;
    if (iters < 1 || rows < 0 || cols < 0 || nnz < 0 || (rows > 0 && !y))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_csr_compute: bad argument");
    if (int rc = check_iterate(o, rows, cols))
        return rc;
    if (o->ngpus > 1)
        return sharded_compute(false, coo, rows, cols, nnz, iters, o, y, time_each_ms, stats);
    if (int rc = smvp::usable_device(o->device))
        return rc;
    smvp::DeviceScope on(o->device);

    RunScratch s;
    if (o->convert_on_device) {
        // COO goes to HBM as it is; sort + scan there; the arrays stay where they were built
        HIP_TRY(hipMalloc(&s.d_coo, sizeof(smvp_coo_t) * (size_t)std::max(nnz, 1)));
        HIP_TRY(hipMalloc((void **)&s.d_i0, sizeof(int) * ((size_t)rows + 1)));
        HIP_TRY(hipMalloc((void **)&s.d_i1, sizeof(int) * (size_t)std::max(nnz, 1)));
        HIP_TRY(hipMalloc((void **)&s.d_v, sizeof(double) * (size_t)std::max(nnz, 1)));
        if (nnz > 0)
            HIP_TRY(hipMemcpy(s.d_coo, coo, sizeof(smvp_coo_t) * (size_t)nnz, hipMemcpyHostToDevice));
        if (int rc = smvp_csr_from_coo_device((const smvp_coo_t *)s.d_coo, rows, cols, nnz, s.d_i0, s.d_i1, s.d_v, nullptr))
            return rc;
        if (int rc = smvp_csr_create(&s.csr, o->device, rows, cols, nnz, s.d_i0, s.d_i1, s.d_v, SMVP_MEM_DEVICE, nullptr))
            return rc;
    } else {
        std::vector<int> row_ptr((size_t)rows + 1), col_ind((size_t)std::max(nnz, 1));
        std::vector<double> val((size_t)std::max(nnz, 1));
        if (int rc = smvp_csr_from_coo(coo, rows, nnz, row_ptr.data(), col_ind.data(), val.data()))
            return rc;
        if (int rc = smvp_csr_create(&s.csr, o->device, rows, cols, nnz, row_ptr.data(), col_ind.data(), val.data(),
                                     SMVP_MEM_HOST, nullptr))
            return rc;
    }
    if (o->csr_kernel != SMVP_CSR_KERNEL_AUTO || o->csr_param != 0)
        if (int rc = smvp_csr_set_kernel(s.csr, o->csr_kernel, o->csr_param))
            return rc;
    if (int rc = prepare_run(s, rows, cols, iters, o))
        return rc;

    // The reference clears y before every product, outside its timed window (main-cli.c:405).  Every CSR kernel
    // here overwrites all of y, so nothing is cleared per product; y is poisoned with NaN once instead, so that a
    // kernel that skipped a row could not hide behind a cleared (or an earlier) result.
    HIP_TRY(hipMemsetAsync(s.d_y, 0xff, sizeof(double) * (size_t)std::max(rows, 1), s.stream));
    smvp_csr_t *A = s.csr;
    // (a matrix without rows launches nothing -- launch_csr_stream_owner returns at once -- so nobody would write the stamps that
    // stamp_reduce reads: such a product is not stamped, AUTO times it with events and explicit device timing is refused)
    const int slots = rows > 0 ? smvp::csr_stamp_slots(A) : 0;
    const int rgrid = slots > 0 ? smvp::csr_repeat_grid(A) : 0;  // the tile kernel's repeating form: n products per launch
    if (int rc = run_timed_products(
            s, rows, iters, o, slots, [](double *) { return (int)SMVP_OK; },
            [A, &s](const double *x, double *yy, unsigned long long *stamps) { return smvp::csr_spmv_stamped(A, x, yy, s.stream, stamps); }, rgrid,
            [A, &s](const double *x, double *yy, unsigned long long *stamps, int reps, int grid, unsigned *ctl, bool first, unsigned long long patience) {
                return smvp::csr_spmv_repeat(A, x, yy, s.stream, stamps, reps, grid, ctl, first, patience);
            }))
        return rc;
    return finish_run(s, rows, iters, y, time_each_ms, stats);
}

extern "C" int smvp_tjds_compute(const smvp_coo_t *coo, int rows, int cols, int nnz, int iters,
                                 const smvp_run_opts_t *opts, double *y, double *time_each_ms,
                                 smvp_time_stats_t *stats)
{
    smvp_run_opts_t def;
    smvp_run_opts_default(&def);
    const smvp_run_opts_t *o = opts ? opts : &def;
    if (iters < 1 || rows < 0 || cols < 0 || nnz < 0 || (rows > 0 && !y))
        return smvp::fail(SMVP_ERR_INVALID, "smvp_tjds_compute: bad argument");
    if (int rc = check_iterate(o, rows, cols))
        return rc;
    if (o->iterate && o->tjds_ref_quirks)
        return smvp::fail(SMVP_ERR_UNSUPPORTED, "ref-quirks TJDS indexes the operand by row: it has no meaning for a changing operand");
    if (o->ngpus > 1) {
        if (o->tjds_ref_quirks)
            return smvp::fail(SMVP_ERR_UNSUPPORTED, "ref-quirks TJDS is a whole-matrix artefact: use one GPU");
        return sharded_compute(true, coo, rows, cols, nnz, iters, o, y, time_each_ms, stats);
    }
    if (int rc = smvp::usable_device(o->device))
        return rc;
    smvp::DeviceScope on(o->device);

    int num_diag = 0, ref_num = 0, last_single = 0;
    RunScratch s;
    if (o->convert_on_device) {
        const int cap = std::max(rows, nnz) + 2;
        HIP_TRY(hipMalloc(&s.d_coo, sizeof(smvp_coo_t) * (size_t)std::max(nnz, 1)));
        HIP_TRY(hipMalloc((void **)&s.d_i0, sizeof(int) * (size_t)std::max(cols, 1)));   // perm
        HIP_TRY(hipMalloc((void **)&s.d_i1, sizeof(int) * (size_t)std::max(nnz, 1)));    // row_ind
        HIP_TRY(hipMalloc((void **)&s.d_i2, sizeof(int) * (size_t)cap));                 // start_pos
        HIP_TRY(hipMalloc((void **)&s.d_v, sizeof(double) * (size_t)std::max(nnz, 1)));
        if (nnz > 0)
            HIP_TRY(hipMemcpy(s.d_coo, coo, sizeof(smvp_coo_t) * (size_t)nnz, hipMemcpyHostToDevice));
        if (int rc = smvp_tjds_from_coo_device((const smvp_coo_t *)s.d_coo, rows, cols, nnz, s.d_i0, s.d_i2, cap, s.d_i1,
                                               s.d_v, &num_diag, &ref_num, &last_single, nullptr))
            return rc;
        if (int rc = smvp_tjds_create(&s.tjds, o->device, rows, cols, nnz, num_diag, s.d_i0, s.d_i2, s.d_i1, s.d_v,
                                      SMVP_MEM_DEVICE))
            return rc;
    } else {
        std::vector<int> perm((size_t)std::max(cols, 1)), start_pos((size_t)std::max(rows, nnz) + 2),
            row_ind((size_t)std::max(nnz, 1));
        std::vector<double> val((size_t)std::max(nnz, 1));
        if (int rc = smvp_tjds_from_coo(coo, rows, cols, nnz, perm.data(), start_pos.data(), (int)start_pos.size(),
                                        row_ind.data(), val.data(), &num_diag, &ref_num, &last_single))
            return rc;
        if (int rc = smvp_tjds_create(&s.tjds, o->device, rows, cols, nnz, num_diag, perm.data(), start_pos.data(),
                                      row_ind.data(), val.data(), SMVP_MEM_HOST))
            return rc;
    }
    if (o->tjds_ref_quirks)
        if (int rc = smvp_tjds_set_ref_quirks(s.tjds, 1, ref_num, last_single))
            return rc;
    if (int rc = prepare_run(s, rows, cols, iters, o))
        return rc;
    if (int rc = smvp_tjds_set_x(s.tjds, s.d_x, s.stream))  // main-cli.c:907-923, setup
        return rc;

    if (o->tjds_mode != SMVP_TJDS_MODE_AUTO)
        if (int rc = smvp_tjds_set_mode(s.tjds, o->tjds_mode))
            return rc;
    HIP_TRY(hipMemsetAsync(s.d_y, 0xff, sizeof(double) * (size_t)std::max(rows, 1), s.stream));  // NaN, as in the CSR path
    smvp_tjds_t *T = s.tjds;
    const int slots = rows > 0 ? smvp::tjds_stamp_slots(T) : 0;  // (no rows: nothing is launched, nothing stamped -- as in the CSR path)
    bool first = true;
    const bool iterate = o->iterate != 0;
    if (int rc = run_timed_products(
            s, rows, iters, o, slots,
            [T, &s](double *yy) { return smvp_tjds_zero_y(T, yy, s.stream); },  // main-cli.c:1008, outside the window
            [T, &s, &first, iterate](const double *x, double *yy, unsigned long long *stamps) {
                if (iterate && !first)  // a new operand: its permutation is part of this product
                    if (int rc = smvp_tjds_set_x(T, x, s.stream))
                        return rc;
                first = false;
                return smvp::tjds_spmv_stamped(T, yy, s.stream, stamps);
            },
            slots > 0 ? smvp::tjds_repeat_grid(T) : 0,  // (tjds_stamp_slots: the row-gather product, which overwrites y and needs no `pre`)
            [T, &s](const double *, double *yy, unsigned long long *stamps, int reps, int grid, unsigned *ctl, bool first, unsigned long long patience) {
                return smvp::tjds_spmv_repeat(T, yy, s.stream, stamps, reps, grid, ctl, first, patience);
            }))
        return rc;
    return finish_run(s, rows, iters, y, time_each_ms, stats);
}
