// hip_backend.hip -- the HIP side of libfnft_amd.so: the extern "C" shim (sections 2 and 3 of
// include/fnft_amd.h plus the internal entries the C drivers call) over NftPlan<HipBackend> and the batched cores.  The
// kernels are instantiated in hip_kernels_*.hip (see hip_be.h).  gfx950 only.
// Every entry makes its call in one of two ways, and the rules of DESIGN.md ("The shim") hold by their construction:
//   - on a plan (the tree plan and the three batched plans share PlanHandle): PlanCall takes the plan's lock, selects
//     its device and sets its stream -- one call at a time per plan; batch_destroy waits for the last stream;
//   - on host pointers: HostCall finds the current device, takes that device's lock where the entry shares state
//     (HostState: the cached plans, the peeler) and owns the back end; the entry returns through done(), which waits
//     for the stream on a failing branch before the entry's plans and arenas hand their blocks back to the pool.
#include <map>
#include <memory>
#include <mutex>
#include <tuple>

#include "hip_be.h"
#include "nft_nsev_inverse.h"
#include "nft_plan_cache.h"
#include "../../include/fnft_amd.h"

thread_local std::string g_last_error;
// fnft__misc.c:379-380
extern "C" void fnft_amd__warn(const char *msg, const char *func, int line);   // fnft_nsev_host.c
static const char *const kNotBandlimitedMsg =
    "Signal does not appear to be bandlimited. Interpolation step may be inaccurate. Try to reduce the step size, "
    "or switch to a discretization that does not require interpolation";
using Plan = NftPlan<HipBackend>;

// ---- cache of released device blocks (HipBackend::alloc / free) ------------------------------------------------------
// Sizes are rounded up to a bucket (powers of two below 1 MiB, four steps per octave above: at most 25 % slack) so
// that the work arrays of a repeated call find the blocks of the previous one.  At most kPoolMaxCached bytes per
// process stay cached; fnft_amd_release_cached() returns everything to the driver.
namespace {
struct DevPool {
    std::mutex m;
    std::multimap<std::pair<int, size_t>, void *> idle;    // (device, bucket) -> block
    std::map<void *, std::pair<int, size_t>> live;         // block -> (device, bucket)
    size_t cached = 0;
    static constexpr size_t kPoolMaxCached = (size_t)6 << 30;
    static size_t bucket(size_t b)
    {
        if (b < 256) b = 256;
        size_t p = 256;
        while (p < b) p *= 2;
        if (p <= ((size_t)1 << 20)) return p;
        const size_t step = p / 8;          // p/2 < b <= p: buckets p/2 + k*p/8
        return (b + step - 1) / step * step;
    }
    void trim_locked(int device)
    {
        for (auto it = idle.begin(); it != idle.end();) {
            if (device < 0 || it->first.first == device) {
                cached -= it->first.second;
                (void)hipFree(it->second);
                it = idle.erase(it);
            } else ++it;
        }
    }
};
DevPool &pool() { static DevPool *p = new DevPool(); return *p; }   // never destroyed: blocks outlive static teardown
}  // namespace

void *fa_pool_alloc(size_t bytes)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { g_last_error = "hipGetDevice failed"; return nullptr; }
    DevPool &P = pool();
    const size_t bk = DevPool::bucket(bytes);
    std::lock_guard<std::mutex> lk(P.m);
    auto it = P.idle.find(std::make_pair(dev, bk));
    void *p = nullptr;
    if (it != P.idle.end()) {
        p = it->second;
        P.idle.erase(it);
        P.cached -= bk;
    } else {
        if (hipMalloc(&p, bk) != hipSuccess) {
            (void)hipGetLastError();
            P.trim_locked(dev);   // out of memory: give the cached blocks back and try once more
            if (!hip_ok(hipMalloc(&p, bk), "hipMalloc")) return nullptr;
        }
    }
    P.live[p] = std::make_pair(dev, bk);
    return p;
}

void fa_pool_free(void *p)
{
    DevPool &P = pool();
    std::lock_guard<std::mutex> lk(P.m);
    auto it = P.live.find(p);
    if (it == P.live.end()) { (void)hipFree(p); return; }
    const std::pair<int, size_t> key = it->second;
    P.live.erase(it);
    if (P.cached + key.second > DevPool::kPoolMaxCached) { (void)hipFree(p); return; }
    P.idle.insert(std::make_pair(key, p));
    P.cached += key.second;
}

// Device rule of the library (documented in include/fnft_amd.h): the host-pointer entry points
// compute on the calling thread's CURRENT HIP device (hipGetDevice; what torch.cuda.set_device or
// hipSetDevice selected) and never change it; device-resident plans live on the device given to
// fnft_amd_plan_create, and every plan call restores the caller's current device before returning.
static bool device_valid(int device)
{
    int n = 0;
    if (!hip_ok(hipGetDeviceCount(&n), "hipGetDeviceCount") || n <= 0) {
        if (g_last_error.empty()) g_last_error = "no HIP device";
        return false;
    }
    if (device < 0 || device >= n) { g_last_error = "device index out of range"; return false; }
    return true;
}
// the calling thread's current device, or -1 (no usable device)
static int current_device()
{
    int n = 0, dev = 0;
    if (!hip_ok(hipGetDeviceCount(&n), "hipGetDeviceCount") || n <= 0) {
        if (g_last_error.empty()) g_last_error = "no HIP device";
        return -1;
    }
    if (!hip_ok(hipGetDevice(&dev), "hipGetDevice")) return -1;
    return dev;
}
// selects `device` for the scope and puts the caller's device back afterwards
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int device)
    {
        if (!device_valid(device)) return;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = (prev == device) || hip_ok(hipSetDevice(device), "hipSetDevice");
    }
    ~DeviceGuard()
    {
        if (ok && prev >= 0) {
            int now = -1;
            if (hipGetDevice(&now) == hipSuccess && now != prev) (void)hipSetDevice(prev);
        }
    }
};

// ---- the parts of the plans' entry points that do not depend on the plan -----------------------------------------------
// One handle for the tree plan and the three batched plans: the back end, the plan core (NftPlan, NftInverseBatch,
// NftDiscSpecPlan, NftSlowPlan), the device it lives on, the stream of its last call (destroy waits for it), the status
// words finish reads back, and the lock that makes calls on one plan take turns.  The public opaque types add their few
// own fields.
template <class CoreT> struct PlanHandle {
    typedef CoreT Core;
    HipBackend be;
    std::unique_ptr<Core> core;   // after be: its arenas hand the blocks back through be
    int device = 0;
    hipStream_t last_stream = nullptr;
    std::vector<int> st;
    std::mutex mtx;
};
struct fnft_amd_plan : PlanHandle<Plan> {
    int nse_disc = 0;
    int kdv_disc = -1;   // >= 0: plan made by fnft_amd_kdvv_plan_create
    int real_mode = -1;  // KdV plans: -1 ask the device whether the potential is real (default), 0 complex path, 1 real path
};
struct fnft_amd_inverse_plan : PlanHandle<NftInverseBatch<HipBackend>> {
    int cstype = 0;
    size_t K = 0;                 // fnft_amd_inverse_plan_create_discrete: bound states per signal (>= 1)
};
struct fnft_amd_discspec_plan : PlanHandle<NftDiscSpecPlan<HipBackend>> {
    const unsigned long long *last_K = nullptr;   // d_K_out of the last call
    std::vector<unsigned long long> kout;
    std::vector<int> wn;                          // a guess-free plan's warning bits, read by finish
};
struct fnft_amd_slow_plan : PlanHandle<NftSlowPlan<HipBackend>> {
    std::vector<int> wn;
};

// create, first half: the handle and its core from the accepted sizes and options.  No core constructor makes a HIP call
// (they size things and nothing else), so every size or option check of a create entry -- a core's too_large() included
// -- returns its code on a machine without a GPU.  NULL: out of host memory.
template <class H, class... A> static std::unique_ptr<H> batch_new(A &&...args)
{
    std::unique_ptr<H> h(new (std::nothrow) H());
    if (h) h->core.reset(new (std::nothrow) typename H::Core(h->be, std::forward<A>(args)...));
    if (h && !h->core) h.reset();
    return h;
}
// create, second half: the first HIP call (the device), then the core's workspace
template <class H> static FNFT_INT batch_init(H **plan, std::unique_ptr<H> h, int device)
{
    if (!h) return FNFT_EC_NOMEM;
    DeviceGuard dg(device);
    if (!dg.ok) return FNFT_EC_OTHER;
    h->device = device;
    const int rc = h->core->init();
    (void)h->be.sync();           // what init enqueued is done before a call arrives on another stream, or the core goes
    if (rc != NFT_SUCCESS || h->be.failed) {
        h.reset();                // on the plan's device
        return rc != NFT_SUCCESS ? rc : FNFT_EC_NOMEM;
    }
    *plan = h.release();
    return FNFT_SUCCESS;
}

// destroy: the pool hands the plan's blocks to the next allocation, so nothing it enqueued may still be writing them
static void plan_quiesce(hipStream_t last_stream)
{
    if (last_stream) (void)hipStreamSynchronize(last_stream);
    (void)hipDeviceSynchronize();
}
template <class H> static void batch_destroy(H *plan)
{
    if (!plan) return;
    {
        DeviceGuard dg(plan->device);
        plan_quiesce(plan->last_stream);
        plan->core.reset();
        plan->be.destroy_events();
    }
    delete plan;
}

// one call on a plan: its lock, its device, its stream.  last_stream != NULL (the *_device entries): the stream is also
// the one destroy waits for, and the failure flag starts clear.  Without a stream (a setting, or a read that belongs on
// the stream of the call before it) the plan's stream stays what it is.
struct PlanCall {
    std::lock_guard<std::mutex> lk;
    DeviceGuard dg;
    const bool ok;
    PlanCall(std::mutex &m, int device) : lk(m), dg(device), ok(dg.ok) {}
    PlanCall(std::mutex &m, int device, HipBackend &be, hipStream_t *last_stream, void *stream) : PlanCall(m, device)
    {
        if (!ok) return;
        be.stream = (hipStream_t)stream;
        if (last_stream) {
            *last_stream = (hipStream_t)stream;
            be.failed = false;
        }
    }
};

// Richardson extrapolation for the calls that follow, after the entry's own argument checks.  The first enabling call
// waits for the plan's last stream and allocates the coarse pass (the core's enable_richardson); disabling keeps it.
template <class H> static FNFT_INT plan_set_richardson(H *plan, int enabled)
{
    PlanCall call(plan->mtx, plan->device);
    if (!call.ok) return FNFT_EC_OTHER;
    typename H::Core &pl = *plan->core;
    if (!enabled || pl.rich_ready()) {
        pl.rich_on = enabled != 0;
        return FNFT_SUCCESS;
    }
    if (plan->be.sync() != NFT_SUCCESS) return FNFT_EC_OTHER;   // what the last call enqueued: the coarse pass's uploads follow
    const int rc = pl.enable_richardson();
    (void)plan->be.sync();
    if (rc != NFT_SUCCESS) return rc;
    return plan->be.failed ? FNFT_EC_NOMEM : FNFT_SUCCESS;
}

// finish: wait for the stream and read the status words (read: the core's own call, which fills plan->st), then every
// signal's word through the plan's mapping to_status(b, word) -- which also stores the plan's second per-signal output
template <class H, class Read, class Map>
static FNFT_INT batch_finish(H *plan, void *stream, FNFT_INT *status, Read read, Map to_status)
{
    PlanCall call(plan->mtx, plan->device, plan->be, nullptr, stream);
    if (!call.ok) return FNFT_EC_OTHER;
    const int rc = read();
    if (rc != NFT_SUCCESS || plan->be.failed) return FNFT_EC_OTHER;
    FNFT_INT first = FNFT_SUCCESS;
    for (size_t b = 0; b < plan->st.size(); b++) {
        const FNFT_INT s = to_status(b, plan->st[b]);
        if (status) status[b] = s;
        if (s != FNFT_SUCCESS && first == FNFT_SUCCESS) first = s;
    }
    return first;
}

// ---- host-pointer entry points: what they keep between calls, and how they make a call ----------------------------------
// They compute on the calling thread's current device.  What they keep there between calls is that device's alone: the
// lock that makes the calls sharing it take turns (SURVEY 8b allows an internal mutex; calls on different devices run
// concurrently), the plans of fnft_nsev and fnft_kdvv by size and scheme, and the resident layer peeler.  Device-resident
// plans are the caller's, with their own lock.  fnft_amd_release_cached empties a device's state.
struct Peeler {
    HipBackend be;
    NftLayerPeelingDev<HipBackend> lp;
    Peeler() : lp(be, 1.0, 1, 1) {}
};
struct HostState {
    std::mutex mtx;
    PlanCache<std::tuple<size_t, size_t, int, size_t>, fnft_amd_plan, fnft_amd_plan_destroy> nsev;   // (D, M, disc, nskip)
    PlanCache<std::tuple<size_t, size_t, int>, fnft_amd_plan, fnft_amd_plan_destroy> kdvv;           // (D, M, disc)
    Peeler peeler;
};
static HostState &host_state(int device)
{
    static auto *r = new DeviceRegistry<HostState>();   // never destroyed: plans outlive static teardown, like the pool
    return r->of(device);
}

// a call that failed may have left work queued on its stream: wait for it, so that the plans and arenas of the call hand
// their blocks back to the pool from an idle stream.  A call that succeeded has waited already and gains nothing here.
static FNFT_INT drained(HipBackend &be, FNFT_INT rc)
{
    if (rc != FNFT_SUCCESS || be.failed) (void)hipStreamSynchronize(be.stream);
    return be.failed ? FNFT_EC_OTHER : rc;
}

// one host-pointer call: the current device (!ok: none), its lock unless the entry shares nothing (kNoLock: it builds its
// plan, runs it and lets it go), and the back end.  Every entry returns through done(rc); its plans and arenas are
// declared after the HostCall, so they are destroyed after the return expression has drained the stream.
struct HostCall {
    enum Lock { kLock, kNoLock };
    const int dev;
    const bool ok;
    HostState *const hs;
    std::unique_lock<std::mutex> lk;
    HipBackend be;
    explicit HostCall(Lock lock = kLock, void *stream = nullptr)
        : dev(current_device()), ok(dev >= 0), hs(ok && lock == kLock ? &host_state(dev) : nullptr)
    {
        if (hs) lk = std::unique_lock<std::mutex>(hs->mtx);
        be.stream = (hipStream_t)stream;
    }
    FNFT_INT done(FNFT_INT rc) { return drained(be, rc); }
};

// a cached plan's pass over host arrays: two staging blocks from the pool, the n_in values in, run(d_in, d_out), the
// n_out values out (out NULL: none).  The caller's arrays are ordinary pageable memory: hipMemcpy moves them at the link
// rate once their pages are resident.
template <class Run>
static FNFT_INT staged_run(HostCall &call, const void *in, size_t n_in, void *out, size_t n_out, Run run)
{
    DevArena<HipBackend> tmp(call.be);
    cplx *d_in = nullptr, *d_out = nullptr;
    if (!tmp.get(d_in, n_in) || !tmp.get(d_out, n_out)) return call.done(FNFT_EC_NOMEM);
    FNFT_INT rc = FNFT_SUCCESS;
    if (!hip_ok(hipMemcpy(d_in, in, n_in * sizeof(cplx), hipMemcpyHostToDevice), "hipMemcpy(H2D)")) rc = FNFT_EC_OTHER;
    if (rc == FNFT_SUCCESS) rc = run(d_in, d_out);
    if (rc == FNFT_SUCCESS && out && n_out)
        if (!hip_ok(hipMemcpy(out, d_out, n_out * sizeof(cplx), hipMemcpyDeviceToHost), "hipMemcpy(D2H)"))
            rc = FNFT_EC_OTHER;
    return call.done(rc);
}

extern "C" {

int fnft_amd_device_count(void)
{
    int n = 0;
    if (!hip_ok(hipGetDeviceCount(&n), "hipGetDeviceCount")) return -1;
    return n;
}

const char *fnft_amd_last_error(void) { return g_last_error.c_str(); }

FNFT_INT fnft_amd_plan_create(fnft_amd_plan_t **plan, FNFT_UINT D, FNFT_UINT M, FNFT_UINT batch,
                              fnft_nse_discretization_t discretization, int device)
{
    return fnft_amd_plan_create_sub(plan, D, M, batch, discretization, device, 1);
}

FNFT_INT fnft_amd_plan_create_sub(fnft_amd_plan_t **plan, FNFT_UINT D, FNFT_UINT M, FNFT_UINT batch,
                                  fnft_nse_discretization_t discretization, int device, FNFT_UINT nskip)
{
    if (!plan || D < 2 || batch < 1 || nskip < 1) return FNFT_EC_INVALID_ARGUMENT;
    const int akns = nft_nse_to_akns((int)discretization);
    if (akns < 0) return FNFT_EC_NOT_YET_IMPLEMENTED;
    const int ups = nft_nse_upsampling((int)discretization);
    if (ups == 1 && nskip != 1) return FNFT_EC_NOT_YET_IMPLEMENTED;
    if (ups == 2 && D <= 2) return FNFT_EC_INVALID_ARGUMENT;   // fnft__misc.c:331-332
    const size_t Dtree = (ups == 1) ? (size_t)D : 2 * nft_sub_count((size_t)D, (size_t)nskip);
    auto h = batch_new<fnft_amd_plan>(Dtree, (size_t)M, (size_t)batch, akns, nft_akns_degree(akns));
    if (h) {
        h->nse_disc = (int)discretization;
        h->core->set_front((size_t)D, (size_t)nskip, ups);
#ifdef FNFT_AMD_ABLATION   // diagnostic builds only; the product library reads no environment variable
        if (const char *dbg = getenv("FNFT_AMD_DBG")) h->core->dbg_flags = atoi(dbg);
#endif
    }
    return batch_init(plan, std::move(h), device);
}

void fnft_amd_plan_destroy(fnft_amd_plan_t *plan) { batch_destroy(plan); }

FNFT_UINT fnft_amd_plan_workspace_bytes(const fnft_amd_plan_t *plan) { return plan ? plan->core->workspace_bytes() : 0; }

// NftPlan::enable_richardson / run_richardson
FNFT_INT fnft_amd_plan_set_richardson(fnft_amd_plan_t *plan, int enabled)
{
    if (!plan || plan->kdv_disc >= 0 || plan->core->M == 0 || plan->core->Din < 3) return FNFT_EC_INVALID_ARGUMENT;
    if (plan->core->nskip > 1) return FNFT_EC_NOT_YET_IMPLEMENTED;
    return plan_set_richardson(plan, enabled);
}

int fnft_amd_plan_device(const fnft_amd_plan_t *plan) { return plan ? plan->device : -1; }

int fnft_amd_plan_last_warnings(const fnft_amd_plan_t *plan) { return plan ? plan->core->last_warn : 0; }

// host wall-clock stages of the calling thread's last discrete-spectrum call (measurement only)
double fnft_amd_discspec_stage_ms(FNFT_UINT i, char *name, FNFT_UINT name_cap)
{
    const std::vector<NftDsStage> &v = nft_ds_stages();
    if (i >= v.size()) return -1.0;
    if (name && name_cap) {
        size_t n = strlen(v[i].what);
        if (n >= name_cap) n = name_cap - 1;
        memcpy(name, v[i].what, n);
        name[n] = 0;
    }
    return v[i].ms;
}

// measurement and tests only (not declared in include/fnft_amd.h): 0 makes the tree of this plan run its last inverse
// column pass itself instead of leaving it to the chirp transform's first kernel (NftPlan::tune_fuse_root)
extern "C" int fnft_amd_debug_root_handover(fnft_amd_plan_t *plan, int enabled)
{
    if (!plan) return -1;
    PlanCall call(plan->mtx, plan->device);
    if (!call.ok) return FNFT_EC_OTHER;
    plan->core->tune_fuse_root = enabled ? 1 : 0;
    return 0;
}

#ifdef FNFT_AMD_TUNING
// diagnostic builds only: tuning parameters of a plan (which: 0 = row-kernel stagger)
extern "C" int fnft_amd_debug_tune(fnft_amd_plan_t *plan, int which, int value)
{
    if (!plan) return -1;
    if (which == 0) plan->core->tune_stagger = value;
    return 0;
}
#endif

#ifdef FNFT_AMD_STAMPS
// diagnostic builds only: stamp the row kernel of split level `level` (16 u64 per wave, 4096 waves max);
// read back after the stream has been synchronised
extern "C" int fnft_amd_debug_stamps(fnft_amd_plan_t *plan, int level, unsigned long long *host, size_t n)
{
    if (!plan) return -1;
    DeviceGuard dg(plan->device);
    Plan &pl = *plan->core;
    if (!pl.dbg_stamps) {
        if (!pl.mem.get(pl.dbg_stamps, (size_t)4096 * 16)) return -1;
        (void)hipMemset(pl.dbg_stamps, 0, (size_t)4096 * 16 * 8);
    }
    pl.stamp_level = level;
    if (host && n) {
        (void)hipDeviceSynchronize();
        (void)hipMemcpy(host, pl.dbg_stamps, n * 8, hipMemcpyDeviceToHost);
    }
    return 0;
}
#endif

int fnft_amd_current_device(void) { return current_device(); }

void fnft_amd_plan_set_timing(fnft_amd_plan_t *plan, int enabled)
{
    if (plan) plan->be.timing = enabled != 0;
}

double fnft_amd_plan_last_ms(const fnft_amd_plan_t *plan, int which)
{
    if (!plan) return -1.0;
    switch (which) {
    case 0: return plan->be.elapsed_ms(0, 1);
    case 1: return plan->be.elapsed_ms(1, 2);
    case 2: return plan->be.elapsed_ms(0, 2);
    default: return -1.0;
    }
}

void fnft_amd_plan_set_launch_timing(fnft_amd_plan_t *plan, int enabled)
{
    if (!plan) return;
    plan->be.launch_timing = enabled != 0;
    plan->be.launches_used = 0;
}

FNFT_UINT fnft_amd_plan_launch_count(const fnft_amd_plan_t *plan)
{
    return plan ? plan->be.launches_used : 0;
}

// time and kernel name of launch i of a back end's per-launch timers
static double launch_ms_of(const HipBackend &be, FNFT_UINT i, char *name, FNFT_UINT name_cap)
{
    if (i >= be.launches_used) return -1.0;
    const HipBackend::LaunchRec &r = be.launches[i];
    if (name && name_cap) {
        // __PRETTY_FUNCTION__ of run<K>: "... [K = KMidSym<true>]"
        const char *k = strstr(r.name, "K = ");
        k = k ? k + 4 : r.name;
        size_t n = strlen(k);
        if (n && k[n - 1] == ']') n--;
        if (n >= name_cap) n = name_cap - 1;
        memcpy(name, k, n);
        name[n] = 0;
    }
    float ms = -1.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) return -1.0;
    return (double)ms;
}

double fnft_amd_plan_launch_ms(const fnft_amd_plan_t *plan, FNFT_UINT i, char *name, FNFT_UINT name_cap)
{
    return plan ? launch_ms_of(plan->be, i, name, name_cap) : -1.0;
}

FNFT_INT fnft_amd_nsev_contspec_device(fnft_amd_plan_t *plan, const void *d_q, void *d_contspec,
                                       const FNFT_REAL *T, const FNFT_REAL *XI, FNFT_INT kappa,
                                       fnft_nsev_cstype_t contspec_type,
                                       FNFT_INT normalization_flag, void *stream)
{
    if (!plan || !d_q || !T || !(T[0] < T[1])) return FNFT_EC_INVALID_ARGUMENT;
    if (d_contspec && (!XI || !(XI[0] < XI[1]))) return FNFT_EC_INVALID_ARGUMENT;
    if (kappa != 1 && kappa != -1) return FNFT_EC_INVALID_ARGUMENT;
    const int cst = (int)contspec_type;
    if (cst < 0 || cst > 2) return FNFT_EC_INVALID_ARGUMENT;
    PlanCall call(plan->mtx, plan->device, plan->be, &plan->last_stream, stream);
    if (!call.ok) return FNFT_EC_OTHER;
    Plan &pl = *plan->core;
    plan->be.mark(0);
    double Tsub[2];
    int rc = pl.run_front(d_q, T, kappa, Tsub);
    if (rc == NFT_SUCCESS) rc = pl.run_tree();
    plan->be.mark(1);
    if (rc == NFT_SUCCESS && d_contspec && pl.M > 0) {
        Plan::Contspec cs;
        cs.T[0] = Tsub[0]; cs.T[1] = Tsub[1]; cs.XI[0] = XI[0]; cs.XI[1] = XI[1];
        cs.nse_disc = plan->nse_disc;
        cs.cstype = cst;
        cs.normalization_flag = normalization_flag;
        rc = pl.run_contspec(d_contspec, cs);
        if (rc == NFT_SUCCESS && pl.rich_on) rc = pl.run_richardson(d_q, T, kappa, d_contspec, cs);
    }
    plan->be.mark(2);
    if (plan->be.failed) return FNFT_EC_OTHER;
    return rc;
}

// nsev_compute_contspec (src/fnft_nsev.c:744-891) on a caller-supplied transfer matrix in device memory
FNFT_INT fnft_amd_nsev_contspec_from_tm_device(fnft_amd_plan_t *plan, const void *d_tm, FNFT_INT W, void *d_contspec,
                                               const FNFT_REAL *T, const FNFT_REAL *XI,
                                               fnft_nsev_cstype_t contspec_type, void *stream)
{
    if (!plan || plan->kdv_disc >= 0 || !d_tm || !d_contspec || !T || !(T[0] < T[1]) || !XI || !(XI[0] < XI[1]))
        return FNFT_EC_INVALID_ARGUMENT;
    const int cst = (int)contspec_type;
    if (cst < 0 || cst > 2 || plan->core->M == 0) return FNFT_EC_INVALID_ARGUMENT;
    PlanCall call(plan->mtx, plan->device, plan->be, &plan->last_stream, stream);
    if (!call.ok) return FNFT_EC_OTHER;
    Plan &pl = *plan->core;
    Plan::Contspec cs;
    cs.T[0] = T[0]; cs.T[1] = T[1]; cs.XI[0] = XI[0]; cs.XI[1] = XI[1];
    cs.nse_disc = plan->nse_disc;
    cs.cstype = cst;
    cs.normalization_flag = 1;
    const int rc = pl.run_contspec_tm(d_contspec, cs, d_tm, (int)W);
    if (plan->be.failed) return FNFT_EC_OTHER;
    return rc;
}

// a(lambda), b(lambda) of the plan's last tree run at n arbitrary complex lambda per signal (Plan::run_eval)
FNFT_INT fnft_amd_nsev_eval_device(fnft_amd_plan_t *plan, const FNFT_REAL *T, const void *d_lambda, FNFT_UINT n,
                                   FNFT_UINT lambda_stride, FNFT_INT derivative_flag, void *d_out, void *stream)
{
    if (!plan || !T || !d_lambda || !d_out || !(T[0] < T[1]) || (lambda_stride != 0 && lambda_stride < n))
        return FNFT_EC_INVALID_ARGUMENT;
    if (plan->kdv_disc >= 0 || !plan->core->tree_valid) return -FNFT_EC_INVALID_ARGUMENT;
    if (plan->core->nskip > 1) return FNFT_EC_NOT_YET_IMPLEMENTED;
    if (n == 0) return FNFT_SUCCESS;
    PlanCall call(plan->mtx, plan->device, plan->be, &plan->last_stream, stream);
    if (!call.ok) return FNFT_EC_OTHER;
    Plan &pl = *plan->core;
    const int rc = pl.run_eval(T, plan->nse_disc, (const cplx *)d_lambda, n, lambda_stride, derivative_flag != 0,
                               (cplx *)d_out);
    if (plan->be.failed) return FNFT_EC_OTHER;
    return rc;
}

// ---- KdV ----------------------------------------------------------------------------------------
FNFT_INT fnft_amd_kdvv_plan_create(fnft_amd_plan_t **plan, FNFT_UINT D, FNFT_UINT M, FNFT_UINT batch,
                                   fnft_kdv_discretization_t discretization, int device)
{
    if (!plan || D < 2 || batch < 1 || M < 1) return FNFT_EC_INVALID_ARGUMENT;
    const int kd = (int)discretization;
    if (kd < 0) return FNFT_EC_INVALID_ARGUMENT;
    if (kd > (int)fnft_kdv_discretization_2SPLIT8B) return FNFT_EC_NOT_YET_IMPLEMENTED;
    const int akns = kd + 1;   // same scheme names, fnft__kdv_discretization.c:86-150
    auto h = batch_new<fnft_amd_plan>((size_t)D, (size_t)M, (size_t)batch, akns, nft_akns_degree(akns));
    if (h) {
        h->nse_disc = -1;
        h->kdv_disc = kd;
        h->core->kdv = true;
    }
    return batch_init(plan, std::move(h), device);
}

FNFT_INT fnft_amd_kdvv_contspec_device(fnft_amd_plan_t *plan, const void *d_u, void *d_contspec,
                                       const FNFT_REAL *T, const FNFT_REAL *XI, void *stream)
{
    if (!plan || plan->kdv_disc < 0 || !d_u || !d_contspec || !T || !(T[0] < T[1]) || !XI || !(XI[0] < XI[1]))
        return FNFT_EC_INVALID_ARGUMENT;
    PlanCall call(plan->mtx, plan->device, plan->be, &plan->last_stream, stream);
    if (!call.ok) return FNFT_EC_OTHER;
    Plan &pl = *plan->core;
    plan->be.mark(0);
    // a real potential takes the real-coefficient tree (nft_real.h: half the transforms and bytes); in the default mode
    // the device is asked first -- one small kernel and a 4-byte read-back, i.e. this call then waits for the stream once
    bool real = plan->real_mode == 1;
    if (plan->real_mode < 0) {
        RealCheckParams R;
        R.q = (const cplx *)d_u;
        R.n = (long long)(pl.batch * pl.D);
        R.flag = pl.status + 1;
        plan->be.run<KRealCheck>((int)std::min<long long>(1024, (R.n + 255) / 256), 1, R);
        int flag = 1;
        plan->be.d2h(&flag, pl.status + 1, sizeof(int));
        if (plan->be.sync() != NFT_SUCCESS) return FNFT_EC_OTHER;
        if (flag) plan->be.memset0(pl.status + 1, sizeof(int));
        real = (flag == 0);
    }
    pl.want_real = real;
    double Tsub[2];
    int rc = pl.run_front(d_u, T, 1, Tsub);
    if (rc == NFT_SUCCESS) rc = pl.run_tree();
    plan->be.mark(1);
    if (rc == NFT_SUCCESS)
        rc = pl.run_contspec_kdv(d_contspec, T, XI, plan->kdv_disc == (int)fnft_kdv_discretization_2SPLIT2A);
    plan->be.mark(2);
    if (plan->be.failed) return FNFT_EC_OTHER;
    return rc;
}

FNFT_INT fnft_amd_kdvv_plan_set_real_mode(fnft_amd_plan_t *plan, int mode)
{
    if (!plan || plan->kdv_disc < 0 || mode < -1 || mode > 1) return FNFT_EC_INVALID_ARGUMENT;
    PlanCall call(plan->mtx, plan->device);
    if (!call.ok) return FNFT_EC_OTHER;
    plan->real_mode = mode;
    return FNFT_SUCCESS;
}

FNFT_INT fnft_amd_plan_finish(fnft_amd_plan_t *plan, void *stream)
{
    if (!plan) return FNFT_EC_INVALID_ARGUMENT;
    PlanCall call(plan->mtx, plan->device, plan->be, nullptr, stream);
    if (!call.ok) return FNFT_EC_OTHER;
    return plan->core->read_status();
}

FNFT_INT fnft_amd_plan_get_transfer_matrix(fnft_amd_plan_t *plan, FNFT_UINT b,
                                           FNFT_COMPLEX *result_host, FNFT_UINT *deg, FNFT_INT *W)
{
    if (!plan || !result_host || !plan->core->tree_valid || b >= plan->core->batch)
        return FNFT_EC_INVALID_ARGUMENT;
    PlanCall call(plan->mtx, plan->device);   // on the stream of the call that ran the tree
    if (!call.ok) return FNFT_EC_OTHER;
    Plan &pl = *plan->core;
    pl.export_tm();
    const size_t per = 4 * (pl.res_deg + 1);
    plan->be.d2h(result_host, pl.tm_out + b * per, per * sizeof(cplx));
    int w = 0;
    plan->be.d2h(&w, pl.wexp[pl.cur] + b, sizeof(int));
    const int rc = plan->be.sync();
    if (deg) *deg = pl.res_deg;
    if (W) *W = w;
    return rc;
}

// Device variant: the transfer matrix of signal b goes to a DEVICE buffer of 4*(deg+1) complex128 (same layout),
// enqueued on `stream`; *deg and *W are returned to the host (this call waits for the stream: W is read back).
FNFT_INT fnft_amd_plan_get_transfer_matrix_device(fnft_amd_plan_t *plan, FNFT_UINT b, void *d_result,
                                                  FNFT_UINT *deg, FNFT_INT *W, void *stream)
{
    if (!plan || !d_result || !plan->core->tree_valid || b >= plan->core->batch) return FNFT_EC_INVALID_ARGUMENT;
    PlanCall call(plan->mtx, plan->device, plan->be, nullptr, stream);
    if (!call.ok) return FNFT_EC_OTHER;
    Plan &pl = *plan->core;
    pl.export_tm();
    const size_t per = 4 * (pl.res_deg + 1);
    if (!hip_ok(hipMemcpyAsync(d_result, pl.tm_out + b * per, per * sizeof(cplx), hipMemcpyDeviceToDevice,
                               plan->be.stream), "hipMemcpyAsync(D2D)"))
        return FNFT_EC_OTHER;
    int w = 0;
    plan->be.d2h(&w, pl.wexp[pl.cur] + b, sizeof(int));
    const int rc = plan->be.sync();
    if (deg) *deg = pl.res_deg;
    if (W) *W = w;
    return rc;
}

// ---- section 2: private-layer seam, host buffers ----------------------------------------------

FNFT_UINT fnft__poly_fmult2x2_numel(const FNFT_UINT deg, const FNFT_UINT n)
{
    return 4 * (deg + 1) * (n == 0 ? 0 : nft_nextpow2(n));
}

FNFT_INT fnft__poly_fmult2x2(FNFT_UINT *const d, FNFT_UINT n, FNFT_COMPLEX *const p,
                             FNFT_COMPLEX *const result, FNFT_INT *const W_ptr)
{
    HostCall call(HostCall::kNoLock);
    if (!call.ok) return FNFT_EC_OTHER;
    return call.done(api_poly_fmult2x2(call.be, d, n, p, result, W_ptr));
}

// fnft__poly_fmult2x2 on matrices that are already in device memory (the root's step of a sample-axis split: the G
// block matrices arrive by RCCL): d_p holds n matrices of degree deg in the reference's input layout, d_result
// (4 * (n*deg + 1) complex128) receives the product in the reference's result layout, normalised; *W_out its exponent.
// Runs on `stream` of the calling thread's current device; waits for the stream once (W is read back).
FNFT_INT fnft_amd_poly_fmult2x2_device(FNFT_UINT deg, FNFT_UINT n, const void *d_p, void *d_result, FNFT_UINT *deg_out,
                                       FNFT_INT *W_out, void *stream)
{
    if (deg == 0 || n == 0 || !d_p || !d_result || !W_out || deg > 0x7fffffff) return FNFT_EC_INVALID_ARGUMENT;
    HostCall call(HostCall::kLock, stream);
    if (!call.ok) return FNFT_EC_OTHER;
    HipBackend &be = call.be;
    Plan pl(be, n, 0, 1, -1, (int)deg);
    int rc = pl.init();
    if (rc == NFT_SUCCESS) rc = pl.load_level0_from_device(d_p);
    if (rc == NFT_SUCCESS) rc = pl.run_tree();
    if (rc == NFT_SUCCESS) {
        pl.export_tm((cplx *)d_result, (size_t)(pl.res_deg + 1), false);
        int W = 0;
        be.d2h(&W, pl.wexp[pl.cur], sizeof(int));
        rc = be.sync();
        *W_out = W;
        if (deg_out) *deg_out = pl.res_deg;
    }
    return call.done(rc);
}

// ---- scalar products and single pair products (src/private/fnft__poly_fmult.c:35-38,45-121,152-328) ----------
// They ride on the 2x2 tree: a scalar polynomial p is the matrix diag(p, p), whose products have the scalar
// product in entry 11.
FNFT_UINT fnft__poly_fmult_numel(const FNFT_UINT deg, const FNFT_UINT n)
{
    return (deg + 1) * (n == 0 ? 0 : nft_nextpow2(n));
}

FNFT_INT fnft__poly_fmult(FNFT_UINT *const d, FNFT_UINT n, FNFT_COMPLEX *const p, FNFT_INT *const W_ptr)
{
    if (!d || !p || n == 0 || *d == 0) return FNFT_EC_INVALID_ARGUMENT;
    HostCall call(HostCall::kNoLock);
    if (!call.ok) return FNFT_EC_OTHER;
    const size_t deg = *d, w = deg + 1;
    std::vector<std::complex<double>> m(fnft__poly_fmult2x2_numel(deg, n)), r(m.size());
    for (size_t i = 0; i < n * w; i++) {
        m[i] = p[i];                  // entry 11
        m[3 * n * w + i] = p[i];      // entry 22
    }
    size_t dd = deg;
    const FNFT_INT rc = call.done(api_poly_fmult2x2(call.be, &dd, n, m.data(), r.data(), W_ptr));
    if (rc != FNFT_SUCCESS) return rc;
    for (size_t i = 0; i <= dd; i++) p[i] = r[i];
    *d = dd;
    return FNFT_SUCCESS;
}

// fft_wrapper_next_fft_length(2*(deg+1)-1), include/private/fnft__fft_wrapper.h:43-48 (kiss_fft_next_fast_size):
// the length callers of the reference size buf0..buf2 with
FNFT_INT fnft__poly_fmult_two_polys_len(const FNFT_UINT deg)
{
    size_t n = 2 * (deg + 1) - 1;
    for (;; n++) {
        size_t m = n;
        while (m % 2 == 0) m /= 2;
        while (m % 3 == 0) m /= 3;
        while (m % 5 == 0) m /= 5;
        if (m <= 1) return (FNFT_INT)n;
    }
}

static int two_polys_product(HipBackend &be, size_t deg, const std::complex<double> *p1, const std::complex<double> *p2,
                             std::complex<double> *out /* 2*deg+1 */)
{
    const size_t w = deg + 1;
    std::vector<std::complex<double>> m(fnft__poly_fmult2x2_numel(deg, 2)), r(m.size());
    for (size_t i = 0; i < w; i++) {
        m[i] = p1[i];           m[w + i] = p2[i];                  // entry 11 of both factors
        m[6 * w + i] = p1[i];   m[7 * w + i] = p2[i];              // entry 22
    }
    size_t dd = deg;
    const int rc = api_poly_fmult2x2(be, &dd, 2, m.data(), r.data(), nullptr);
    if (rc != FNFT_SUCCESS) return rc;
    for (size_t i = 0; i <= 2 * deg; i++) out[i] = r[i];
    return FNFT_SUCCESS;
}

// src/private/fnft__poly_fmult.c:50-121.  plan_fwd / plan_inv are the reference's KissFFT / FFTW handles: the GPU
// does its own transforms and ignores them (pass whatever the caller has, or NULL).  The reference keeps the
// SPECTRA of p1 / p2 in buf1 / buf2 between calls (a NULL factor means "the one of the previous call") and, in
// modes 2 / 3, a partial sum of spectra in `result`; here the same buffers carry the COEFFICIENTS instead --
// what a sequence of calls returns in the coefficient domain (modes 0, 1, 3) is the same.
FNFT_INT fnft__poly_fmult_two_polys(const FNFT_UINT deg, FNFT_COMPLEX const *const p1, FNFT_COMPLEX const *const p2,
                                    FNFT_COMPLEX *const result, void *plan_fwd, void *plan_inv, FNFT_COMPLEX *const buf0,
                                    FNFT_COMPLEX *const buf1, FNFT_COMPLEX *const buf2, const FNFT_UINT mode)
{
    (void)plan_fwd; (void)plan_inv; (void)buf0;
    if (!result || !buf1 || !buf2 || mode > 3) return FNFT_EC_INVALID_ARGUMENT;
    HostCall call(HostCall::kNoLock);
    if (!call.ok) return FNFT_EC_OTHER;
    const size_t w = deg + 1, wr = 2 * deg + 1;
    if (p1) for (size_t i = 0; i < w; i++) buf1[i] = p1[i];
    if (p2) for (size_t i = 0; i < w; i++) buf2[i] = p2[i];
    std::vector<std::complex<double>> prod(wr);
    if (deg == 0) prod[0] = buf1[0] * buf2[0];
    else {
        const FNFT_INT rc = call.done(two_polys_product(call.be, deg, buf1, buf2, prod.data()));
        if (rc != FNFT_SUCCESS) return rc;
    }
    switch (mode) {
    case 0: for (size_t i = 0; i < wr; i++) result[i] = prod[i]; break;
    case 1: for (size_t i = 0; i < wr; i++) result[i] += prod[i]; break;
    case 2: for (size_t i = 0; i < wr; i++) result[i] = prod[i]; break;    // partial sum kept for a mode-3 call
    default: for (size_t i = 0; i < wr; i++) result[i] += prod[i]; break;  // mode 3: partial sum + this product
    }
    return FNFT_SUCCESS;
}

// src/private/fnft__poly_fmult.c:239-328: one 2x2 product, entries at the given strides; plans, buffers and
// mode_offset (where the reference parks spectra) are not needed and ignored
FNFT_INT fnft__poly_fmult_two_polys2x2(const FNFT_UINT deg, FNFT_COMPLEX const *const p1_11, const FNFT_UINT p1_stride,
                                       FNFT_COMPLEX const *const p2_11, const FNFT_UINT p2_stride,
                                       FNFT_COMPLEX *const result_11, const FNFT_UINT result_stride, void *plan_fwd,
                                       void *plan_inv, FNFT_COMPLEX *const buf0, FNFT_COMPLEX *const buf1,
                                       FNFT_COMPLEX *const buf2, const FNFT_UINT mode_offset)
{
    (void)plan_fwd; (void)plan_inv; (void)buf0; (void)buf1; (void)buf2; (void)mode_offset;
    if (!p1_11 || !p2_11 || !result_11 || deg == 0) return FNFT_EC_INVALID_ARGUMENT;
    HostCall call(HostCall::kNoLock);
    if (!call.ok) return FNFT_EC_OTHER;
    const size_t w = deg + 1, wr = 2 * deg + 1;
    std::vector<std::complex<double>> m(fnft__poly_fmult2x2_numel(deg, 2)), r(m.size());
    for (int e = 0; e < 4; e++)
        for (size_t i = 0; i < w; i++) {
            m[(size_t)e * 2 * w + i] = p1_11[(size_t)e * p1_stride + i];
            m[(size_t)e * 2 * w + w + i] = p2_11[(size_t)e * p2_stride + i];
        }
    size_t dd = deg;
    const FNFT_INT rc = call.done(api_poly_fmult2x2(call.be, &dd, 2, m.data(), r.data(), nullptr));
    if (rc != FNFT_SUCCESS) return rc;
    for (int e = 0; e < 4; e++)
        for (size_t i = 0; i < wr; i++) result_11[(size_t)e * result_stride + i] = r[(size_t)e * wr + i];
    return FNFT_SUCCESS;
}

// include/private/fnft__nse_finvscatter.h (src/private/fnft__nse_finvscatter.c:234-366): samples from a transfer
// matrix by layer peeling, every array on the device (NftLayerPeelingDev, nft_nsev_inverse.h)
// argument errors of the private seams are raised like the reference raises them (E_INVALID_ARGUMENT(name): code + text
// through the error hook, src/fnft_errwarn.c), not returned bare
extern "C" FNFT_INT fnft_amd__raise(FNFT_INT ec, const char *func, int line, const char *msg);   // fnft_nsev_host.c
static FNFT_INT seam_invalid(const char *func, int line, const char *arg)
{
    const std::string msg = std::string("Invalid argument ") + arg + ".";
    return fnft_amd__raise(FNFT_EC_INVALID_ARGUMENT, func, line, msg.c_str());
}
#define SEAM_CHECK(cond, arg) do { if (cond) return seam_invalid(__func__, __LINE__, #arg); } while (0)

FNFT_INT fnft__nse_finvscatter(const FNFT_UINT deg, FNFT_COMPLEX *const transfer_matrix, FNFT_COMPLEX *const q,
                               const FNFT_REAL eps_t, const FNFT_INT kappa, const fnft_nse_discretization_t discretization)
{
    // argument checks in the reference's order, :242-260
    SEAM_CHECK(deg == 0, deg);
    SEAM_CHECK(!transfer_matrix, transfer_matrix);
    SEAM_CHECK(!q, q);
    SEAM_CHECK(!(eps_t > 0.0), eps_t);
    SEAM_CHECK(kappa != -1 && kappa != 1, kappa);
    const int akns = nft_nse_to_akns((int)discretization);
    const int ddeg = akns < 0 ? 0 : nft_akns_degree(akns);
    SEAM_CHECK(ddeg == 0, discretization);
    const size_t D = deg / (size_t)ddeg;
    if (D < 2 || (D & (D - 1)) != 0) return FNFT_EC_OTHER;           // not a power of two, :259-260
    // the base case exists for the two degree-1 schemes only, :164-211
    const bool modal = discretization == fnft_nse_discretization_2SPLIT2_MODAL;
    SEAM_CHECK(!modal && discretization != fnft_nse_discretization_2SPLIT2A, discretization);
    HostCall call;
    if (!call.ok) return FNFT_EC_OTHER;
    // the device's resident peeler, on its own back end: its pair-product plans (one per degree) and work arrays are
    // reused by later calls; a failure, or a size beyond 2^18 samples (workspace footprint), releases everything again
    Peeler &pp = call.hs->peeler;
    pp.be.failed = false;
    pp.lp.eps_t = eps_t;
    pp.lp.kappa = (int)kappa;
    pp.lp.modal = modal ? 1 : 0;
    const FNFT_INT rc = drained(pp.be, pp.lp.run_host(deg, transfer_matrix, q));
    if (rc != FNFT_SUCCESS || deg > ((size_t)1 << 18)) pp.lp.destroy();
    return rc;
}

// ---- fnft_nsev_inverse (driver: fnft_nsev_inverse_host.c) ---------------------------------------------------------
// include/private/fnft__poly_specfact.h (src/private/fnft__poly_specfact.c:25-140)
FNFT_INT fnft__poly_specfact(const FNFT_UINT deg, FNFT_COMPLEX const *const poly, FNFT_COMPLEX *const result,
                             const FNFT_UINT oversampling_factor, const FNFT_INT kappa)
{
    SEAM_CHECK(deg == 0, deg);                                   // :31-38
    SEAM_CHECK(!poly, poly);
    SEAM_CHECK(!result, result);
    SEAM_CHECK(oversampling_factor == 0, oversampling_factor);
    SEAM_CHECK(kappa != 0 && kappa != 1 && kappa != -1, kappa);  // :105-107
    HostCall call;
    if (!call.ok) return FNFT_EC_OTHER;
    NftInverseDev<HipBackend> inv(call.be);
    int warn = 0;
    const FNFT_INT rc = call.done(inv.specfact_host(deg, poly, result, oversampling_factor, (int)kappa, &warn));
    if (rc == FNFT_SUCCESS && warn) fnft_amd__warn("Ill-posed spectral factorization problem.", "fnft__poly_specfact", __LINE__);
    return rc;
}

extern "C" FNFT_INT fnft_amd__inverse_transfer_matrix(FNFT_UINT M, FNFT_COMPLEX *contspec, const FNFT_REAL *XI, FNFT_UINT K,
                                                      const FNFT_COMPLEX *bound_states, FNFT_UINT D, const FNFT_REAL *T,
                                                      FNFT_UINT deg, FNFT_COMPLEX *tm, FNFT_INT kappa, int cstype,
                                                      int method, FNFT_UINT max_iter, FNFT_UINT oversampling,
                                                      FNFT_REAL phase_factor, int *warn_specfact, int *warn_maxiter)
{
    HostCall call;
    if (!call.ok) return FNFT_EC_OTHER;
    NftInverseDev<HipBackend> inv(call.be);
    return call.done(inv.transfer_matrix(M, contspec, XI, K, bound_states, D, T, deg, tm, (int)kappa, cstype, method,
                                         max_iter, oversampling, phase_factor, warn_specfact, warn_maxiter));
}

// src/fnft_nsev_inverse.c:680-903: host bookkeeping (sorting, residues -> norming constants), device Darboux steps
extern "C" FNFT_INT fnft_amd__inverse_add_discrete(FNFT_UINT K, const FNFT_COMPLEX *bound_states,
                                                   const FNFT_COMPLEX *normconsts_or_residues, FNFT_UINT D,
                                                   FNFT_COMPLEX *q, const FNFT_REAL *T, int contspec_flag, int residues,
                                                   int seed_method)
{
    typedef std::complex<double> cd;
    if (K == 0 || !bound_states || !normconsts_or_residues) return FNFT_EC_INVALID_ARGUMENT;
    HostCall call;
    if (!call.ok) return FNFT_EC_OTHER;
    HipBackend &be = call.be;
    std::vector<cd> bs(bound_states, bound_states + K), nc(normconsts_or_residues, normconsts_or_residues + K);
    for (size_t i = 0; i < K; i++)            // descending imaginary part, the reference's exchange sort (:742-754)
        for (size_t j = i + 1; j < K; j++)
            if (bs[i].imag() < bs[j].imag()) { std::swap(bs[i], bs[j]); std::swap(nc[i], nc[j]); }
    for (size_t i = 0; i + 1 < K; i++)
        if (bs[i + 1] == bs[i]) return call.done(FNFT_EC_SANITY_CHECK_FAILED);   // :756-761
    int rc = FNFT_SUCCESS;
    if (residues) {                                                    // :771-795
        std::vector<cd> acs(K, cd(1.0, 0.0)), ap(K), bdummy(K);
        if (contspec_flag) {
            // the non-solitonic part of the potential contributes to the residues: a(lambda_k) of the seed, BO scheme
            NftDiscSpec<HipBackend> ds(be);
            NftDiscSpec<HipBackend>::Prepared P(be);
            rc = ds.prepare(D, q, T, D, (int)fnft_nse_discretization_2SPLIT4B, P, false);
            if (rc == FNFT_SUCCESS) rc = ds.scatter(P, K, bs.data(), acs.data(), ap.data(), bdummy.data(), true);
            if (rc != FNFT_SUCCESS || be.failed) return call.done(rc);
        }
        for (size_t i = 0; i < K; i++) {
            cd tmp = acs[i];
            for (size_t j = 0; j < K; j++)
                if (j != i) tmp = tmp * (bs[i] - bs[j]) / (bs[i] - std::conj(bs[j]));
            nc[i] = (nc[i] / cd(0.0, 2.0 * bs[i].imag())) * tmp;
        }
    }
    int mode;
    if (contspec_flag == 0 && !seed_method) mode = 0;
    else if ((contspec_flag == 0 && seed_method) || (contspec_flag == 1 && !seed_method)) mode = 1;
    else return call.done(FNFT_EC_INVALID_ARGUMENT);                   // :890-891
    NftInverseDev<HipBackend> inv(be);
    return call.done(inv.add_discrete(K, bs.data(), nc.data(), D, q, T, mode));
}

// ---- batched, device-resident fnft_nsev_inverse (continuous part) ----------------------------------------------------
// Argument checks follow fnft_nsev_inverse (fnft_nsev_inverse_host.c) in its order and with its codes; those that only
// depend on sizes and options run at create time, before any HIP call.
static FNFT_INT inv_subroutine(const char *func, int line, FNFT_INT ec)
{
    return fnft_amd__raise(-std::abs((int)ec), func, line, "Subroutine failure.");
}

// continuous-spectrum options of a plan with a continuous part: *cstype (0 rho, 1 b(xi), 2 B(tau)), or the error,
// raised in the name of the public entry `func`
static FNFT_INT inv_cstype(const char *func, const fnft_nsev_inverse_opts_t &o, FNFT_UINT D, FNFT_UINT M, int *cstype)
{
    *cstype = 0;
    switch (o.contspec_type) {
    case fnft_nsev_inverse_cstype_REFLECTION_COEFFICIENT:
        if (o.contspec_inversion_method != fnft_nsev_inverse_csmethod_DEFAULT
            && o.contspec_inversion_method != fnft_nsev_inverse_csmethod_TFMATRIX_CONTAINS_REFL_COEFF)
            return inv_subroutine(func, __LINE__, seam_invalid(func, __LINE__, "opts->contspec_inversion_method"));
        break;
    case fnft_nsev_inverse_cstype_B_OF_XI:
        *cstype = 1;
        break;
    case fnft_nsev_inverse_cstype_B_OF_TAU:
        *cstype = 2;
        if (M != D) return inv_subroutine(func, __LINE__, seam_invalid(func, __LINE__, "M"));
        if (o.contspec_inversion_method != fnft_nsev_inverse_csmethod_DEFAULT)
            return inv_subroutine(func, __LINE__, seam_invalid(func, __LINE__, "opts->contspec_inversion_method"));
        break;
    default:
        return seam_invalid(func, __LINE__, "opts->contspec_type");
    }
    if (*cstype != 0 && o.oversampling_factor == 0)                   // fnft__poly_specfact.c:37-38
        return inv_subroutine(func, __LINE__, FNFT_EC_INVALID_ARGUMENT);
    return FNFT_SUCCESS;
}

// what a *_device entry returns after its core's run(): a failure is raised in the name of the public entry
static FNFT_INT batch_run_result(const HipBackend &be, int rc, const char *func, int line)
{
    if (be.failed) return FNFT_EC_OTHER;
    return rc == NFT_SUCCESS ? FNFT_SUCCESS : inv_subroutine(func, line, rc);
}

// the plan and its workspace, once the options are accepted.  K = 0: no discrete part
static FNFT_INT inv_plan_new(fnft_amd_inverse_plan_t **plan, FNFT_UINT D, FNFT_UINT M, FNFT_UINT batch,
                             const fnft_nsev_inverse_opts_t &o, int device, int cstype, FNFT_UINT K, int ds_mode,
                             int residues)
{
    auto h = batch_new<fnft_amd_inverse_plan>((size_t)D, (size_t)M, (size_t)batch, cstype, (size_t)o.oversampling_factor,
                                              o.discretization == fnft_nse_discretization_2SPLIT2_MODAL ? 1 : 0,
                                              (size_t)K, ds_mode, residues);
    if (h) { h->cstype = cstype; h->K = K; }
    return batch_init(plan, std::move(h), device);
}

// step size and phase factor exactly as the host driver forms them (fnft_nsev_inverse_host.c)
static FNFT_REAL inv_phase_factor(const fnft_amd_inverse_plan &plan, const FNFT_REAL *T, FNFT_REAL *eps_t_out)
{
    const size_t D = plan.core->D;
    const FNFT_REAL eps_t = (T[1] - T[0]) / (D - 1);
    const FNFT_REAL pf_rho = -2.0 * (T[1] + eps_t * 0.5) + eps_t;
    const FNFT_REAL pf_b = -eps_t * D - (T[1] + eps_t * 0.5) - (T[0] - eps_t * 0.5) + eps_t;
    *eps_t_out = eps_t;
    return plan.cstype == 0 ? pf_rho : pf_b;
}

FNFT_INT fnft_amd_inverse_plan_create(fnft_amd_inverse_plan_t **plan, FNFT_UINT D, FNFT_UINT M, FNFT_UINT batch,
                                      fnft_nsev_inverse_opts_t const *opts, int device)
{
    SEAM_CHECK(!plan, plan);
    SEAM_CHECK(M % 2 != 0, M);                                        // fnft_nsev_inverse_host.c, in its order
    SEAM_CHECK(M < D, M);
    SEAM_CHECK(D < 2 || (D & (D - 1)) != 0, D);
    SEAM_CHECK(batch == 0, batch);
    const fnft_nsev_inverse_opts_t o = opts ? *opts : fnft_nsev_inverse_default_opts();
    SEAM_CHECK(o.discretization != fnft_nse_discretization_2SPLIT2A
               && o.discretization != fnft_nse_discretization_2SPLIT2_MODAL, opts->discretization);
    if (o.contspec_inversion_method == fnft_nsev_inverse_csmethod_TFMATRIX_CONTAINS_AB_FROM_ITER
        || o.contspec_inversion_method == fnft_nsev_inverse_csmethod_USE_SEED_POTENTIAL_INSTEAD)
        return fnft_amd__raise(FNFT_EC_NOT_YET_IMPLEMENTED, __func__, __LINE__,
                               "Not yet implemented (batched inverse: iterative or seed-potential method).");
    int cstype = 0;
    const FNFT_INT rc = inv_cstype(__func__, o, D, M, &cstype);
    if (rc != FNFT_SUCCESS) return rc;
    return inv_plan_new(plan, D, M, batch, o, device, cstype, 0, 0, 0);
}

void fnft_amd_inverse_plan_destroy(fnft_amd_inverse_plan_t *plan) { batch_destroy(plan); }

FNFT_UINT fnft_amd_inverse_plan_workspace_bytes(const fnft_amd_inverse_plan_t *plan)
{
    return plan ? plan->core->workspace_bytes() : 0;
}

FNFT_INT fnft_amd_nsev_inverse_device(fnft_amd_inverse_plan_t *plan, const void *d_contspec, const FNFT_REAL *XI,
                                      void *d_q, const FNFT_REAL *T, FNFT_INT kappa, void *stream)
{
    SEAM_CHECK(!plan, plan);
    if (plan->K) return inv_subroutine(__func__, __LINE__, seam_invalid(__func__, __LINE__, "plan"));   // K > 0 plan
    SEAM_CHECK(!d_contspec, contspec);
    SEAM_CHECK(!d_q, q);
    SEAM_CHECK(T == NULL || !(T[0] < T[1]), T);
    SEAM_CHECK(kappa != +1 && kappa != -1, kappa);
    SEAM_CHECK(XI == NULL && plan->cstype != 2, XI);
    if (plan->cstype == 2 && T[0] != -T[1])                           // :643-647
        return inv_subroutine(__func__, __LINE__, seam_invalid(__func__, __LINE__, "T"));
    PlanCall call(plan->mtx, plan->device, plan->be, &plan->last_stream, stream);
    if (!call.ok) return FNFT_EC_OTHER;
    FNFT_REAL eps_t;
    const FNFT_REAL pf = inv_phase_factor(*plan, T, &eps_t);
    const int rc = plan->core->run((const cplx *)d_contspec, XI, (cplx *)d_q, eps_t, (int)kappa, pf);
    return batch_run_result(plan->be, rc, __func__, __LINE__);
}

// K > 0: the continuous part as above (M > 0) or none (M = 0), then the discrete part (fnft_nsev_inverse_host.c and
// src/fnft_nsev_inverse.c:680-903, in their order and with their codes)
FNFT_INT fnft_amd_inverse_plan_create_discrete(fnft_amd_inverse_plan_t **plan, FNFT_UINT D, FNFT_UINT M, FNFT_UINT K,
                                               FNFT_UINT batch, fnft_nsev_inverse_opts_t const *opts, int device)
{
    SEAM_CHECK(!plan, plan);
    SEAM_CHECK(M > 0 && M % 2 != 0, M);                               // fnft_nsev_inverse_host.c, in its order
    SEAM_CHECK(M > 0 && M < D, M);
    SEAM_CHECK(D < 2 || (D & (D - 1)) != 0, D);
    SEAM_CHECK(batch == 0, batch);
    const fnft_nsev_inverse_opts_t o = opts ? *opts : fnft_nsev_inverse_default_opts();
    SEAM_CHECK(o.discretization != fnft_nse_discretization_2SPLIT2A
               && o.discretization != fnft_nse_discretization_2SPLIT2_MODAL, opts->discretization);
    if (K == 0) {
        if (M == 0)
            return fnft_amd__raise(FNFT_EC_SANITY_CHECK_FAILED, __func__, __LINE__,
                                   "Sanity check failed (Neither contspec nor discspec provided.).");
        return seam_invalid(__func__, __LINE__, "K");                 // K = 0: fnft_amd_inverse_plan_create
    }
    if (K > NftInverseDiscBatch<HipBackend>::kMaxGridY)
        return fnft_amd__raise(FNFT_EC_NOT_YET_IMPLEMENTED, __func__, __LINE__,
                               "Not yet implemented (batched inverse: more than 65535 bound states per signal).");
    if (o.contspec_inversion_method == fnft_nsev_inverse_csmethod_TFMATRIX_CONTAINS_AB_FROM_ITER)
        return fnft_amd__raise(FNFT_EC_NOT_YET_IMPLEMENTED, __func__, __LINE__,
                               "Not yet implemented (batched inverse: iterative method).");
    const bool seed = o.contspec_inversion_method == fnft_nsev_inverse_csmethod_USE_SEED_POTENTIAL_INSTEAD;
    int cstype = 0;
    if (M > 0) {
        const FNFT_INT rc = inv_cstype(__func__, o, D, M, &cstype);
        if (rc != FNFT_SUCCESS) return rc;
        // b(xi) with the seed method: the drop-in computes the continuous part and then refuses the combination
        // (:890-891); here before anything runs
        if (seed) return inv_subroutine(__func__, __LINE__, seam_invalid(__func__, __LINE__, "opts->contspec_inversion_method"));
    }
    const int ds_mode = (M == 0 && !seed) ? 0 : 1;
    const int residues = o.discspec_type == fnft_nsev_inverse_dstype_RESIDUES ? 1 : 0;
    return inv_plan_new(plan, D, M, batch, o, device, cstype, K, ds_mode, residues);
}

FNFT_INT fnft_amd_nsev_inverse_discrete_device(fnft_amd_inverse_plan_t *plan, const void *d_contspec,
                                               const FNFT_REAL *XI, const void *d_bound_states,
                                               const void *d_normconsts_or_residues, void *d_q, const FNFT_REAL *T,
                                               FNFT_INT kappa, void *stream)
{
    SEAM_CHECK(!plan, plan);
    if (!plan->K) return inv_subroutine(__func__, __LINE__, seam_invalid(__func__, __LINE__, "plan"));  // K = 0 plan
    const size_t M = plan->core->M;
    SEAM_CHECK(M > 0 && !d_contspec, contspec);                        // fnft_nsev_inverse_host.c, in its order
    SEAM_CHECK(M == 0 && d_contspec, M);                               // a contspec with M = 0 fails M < D there
    SEAM_CHECK(!d_q, q);
    SEAM_CHECK(T == NULL || !(T[0] < T[1]), T);
    SEAM_CHECK(kappa != +1 && kappa != -1, kappa);
    if (kappa != +1)
        return fnft_amd__raise(FNFT_EC_SANITY_CHECK_FAILED, __func__, __LINE__,
                               "Sanity check failed (Discrete spectrum is present only in the focussing case(kappa=1).).");
    SEAM_CHECK(!d_bound_states, bound_states);
    SEAM_CHECK(!d_normconsts_or_residues, normconsts_or_residues);
    SEAM_CHECK(M > 0 && XI == NULL && plan->cstype != 2, XI);
    if (M > 0 && plan->cstype == 2 && T[0] != -T[1])                  // :643-647
        return inv_subroutine(__func__, __LINE__, seam_invalid(__func__, __LINE__, "T"));
    PlanCall call(plan->mtx, plan->device, plan->be, &plan->last_stream, stream);
    if (!call.ok) return FNFT_EC_OTHER;
    FNFT_REAL eps_t;
    const FNFT_REAL pf = inv_phase_factor(*plan, T, &eps_t);
    const int rc = plan->core->run_discrete((const cplx *)d_contspec, XI, (const cplx *)d_bound_states,
                                            (const cplx *)d_normconsts_or_residues, (cplx *)d_q, T, eps_t, (int)kappa, pf);
    return batch_run_result(plan->be, rc, __func__, __LINE__);
}

FNFT_INT fnft_amd_inverse_plan_finish(fnft_amd_inverse_plan_t *plan, void *stream, FNFT_INT *status, int *warnings)
{
    SEAM_CHECK(!plan, plan);
    return batch_finish(
        plan, stream, status, [&] { return plan->core->read_status(plan->st); },
        [&](size_t b, int h) -> FNFT_INT {
            if (warnings) warnings[b] = ((h & 8) && !(h & 64)) ? 1 : 0;
            // the drop-in, in its order: a bound state with Im <= 0 (bit 6) fails before anything runs; then
            // fnft__nse_finvscatter with FNFT_EC_OTHER (bits 4, 5) and the discrete part on equal bound states (bit 7),
            // both returned as subroutine failures
            if (h & 64) return FNFT_EC_SANITY_CHECK_FAILED;
            if (h & 48) return -FNFT_EC_OTHER;
            if (h & 128) return -FNFT_EC_SANITY_CHECK_FAILED;
            return FNFT_SUCCESS;
        });
}

// ---- batched, device-resident discrete spectrum of fnft_nsev (NEWTON) ----------------------------------------------
// Size and option checks follow fnft_nsev (fnft_nsev_host.c) in its order, with its codes and message texts, and run
// before any HIP call.  Both create entries make the same handle (core: NftDiscSpecPlan, nft_discspec_plan.h); each
// keeps its own list of checks, and they share the list's end -- the message of its refusal, or NULL:
static const char *discspec_create_refused(const fnft_nsev_opts_t &o, FNFT_UINT K, FNFT_UINT batch)
{
    if (o.richardson_extrapolation_flag != 0)   // fnft_amd_discspec_plan_set_richardson switches it on
        return "Not yet implemented (batched discrete spectrum: Richardson extrapolation).";
    if (K > NftDiscSpecBatch<HipBackend>::kMaxK || batch > NftDiscSpecBatch<HipBackend>::kMaxGroups / K)
        return "Not yet implemented (batched discrete spectrum: K > 65535 or batch*K > 2^31 - 1).";
    return nullptr;
}
static NftDsOpts discspec_opts(const fnft_nsev_opts_t &o)
{
    NftDsOpts d;
    d.bsfilt = (int)o.bound_state_filtering; d.bsloc = (int)o.bound_state_localization; d.niter = o.niter;
    d.Dsub = o.Dsub; d.dstype = (int)o.discspec_type; d.nse_disc = (int)o.discretization; d.richardson = 0;
    return d;
}

FNFT_INT fnft_amd_discspec_plan_create(fnft_amd_discspec_plan_t **plan, FNFT_UINT D, FNFT_UINT K, FNFT_UINT batch,
                                       fnft_nsev_opts_t const *opts, int device)
{
    SEAM_CHECK(!plan, plan);
    SEAM_CHECK(D < 2, D);
    SEAM_CHECK(K == 0, K);
    SEAM_CHECK(batch == 0, batch);
    fnft_nsev_opts_t o = opts ? *opts : fnft_nsev_default_opts();
    if (!opts) o.bound_state_localization = fnft_nsev_bsloc_NEWTON;
    const int disc = (int)o.discretization, loc = (int)o.bound_state_localization;
    const bool slow = disc == (int)fnft_nse_discretization_BO
                      || (disc >= (int)fnft_nse_discretization_CF4_2 && disc <= (int)fnft_nse_discretization_TES4);
    SEAM_CHECK(slow && loc != (int)fnft_nsev_bsloc_NEWTON, opts->bound_state_localization);   // fnft_nsev.c:183-220
    SEAM_CHECK(!slow && nft_nse_to_akns(disc) < 0, opts->discretization);
    if (slow)
        return fnft_amd__raise(FNFT_EC_NOT_YET_IMPLEMENTED, __func__, __LINE__,
                               "Not yet implemented (discretization). GPU path covers the fast (polynomial) discretizations.");
    SEAM_CHECK(loc < 0 || loc > 2, opts->bound_state_localization);
    SEAM_CHECK((int)o.bound_state_filtering < 0 || (int)o.bound_state_filtering > 2, opts->bound_state_filtering);
    SEAM_CHECK((int)o.discspec_type < 0 || (int)o.discspec_type > 2, opts->discspec_type);
    if (loc != (int)fnft_nsev_bsloc_NEWTON)
        return fnft_amd__raise(FNFT_EC_NOT_YET_IMPLEMENTED, __func__, __LINE__,
                               "Not yet implemented (batched discrete spectrum: FAST_EIGENVALUE and SUBSAMPLE_AND_REFINE).");
    if (const char *msg = discspec_create_refused(o, K, batch))
        return fnft_amd__raise(FNFT_EC_NOT_YET_IMPLEMENTED, __func__, __LINE__, msg);
    NftDsOpts d = discspec_opts(o);   // bsloc 1: a guess plan
    d.Dsub = 0;
    return batch_init(plan, batch_new<fnft_amd_discspec_plan>((size_t)D, (size_t)K, (size_t)batch, d), device);
}

void fnft_amd_discspec_plan_destroy(fnft_amd_discspec_plan_t *plan) { batch_destroy(plan); }

FNFT_UINT fnft_amd_discspec_plan_workspace_bytes(const fnft_amd_discspec_plan_t *plan)
{
    return plan ? plan->core->workspace_bytes() : 0;
}

// on a plan of either creator (NftDiscSpecPlan::enable_richardson)
FNFT_INT fnft_amd_discspec_plan_set_richardson(fnft_amd_discspec_plan_t *plan, int enabled)
{
    SEAM_CHECK(!plan, plan);
    SEAM_CHECK(plan->core->D < 3, D);
    return plan_set_richardson(plan, enabled);
}

// one call of either kind of plan; d_guesses NULL: a guess-free plan
static FNFT_INT discspec_run(fnft_amd_discspec_plan_t *plan, const void *d_q, const FNFT_REAL *T, const void *d_guesses,
                             void *d_bound_states, void *d_normconsts_or_residues, void *d_K_out, void *stream,
                             const char *func, int line)
{
    PlanCall call(plan->mtx, plan->device, plan->be, &plan->last_stream, stream);
    if (!call.ok) return FNFT_EC_OTHER;
    plan->last_K = (const unsigned long long *)d_K_out;
    const int rc = plan->core->run((const cplx *)d_q, T, (const cplx *)d_guesses, (cplx *)d_bound_states,
                                   (cplx *)d_normconsts_or_residues, (unsigned long long *)d_K_out);
    return batch_run_result(plan->be, rc, func, line);
}

FNFT_INT fnft_amd_nsev_discspec_device(fnft_amd_discspec_plan_t *plan, const void *d_q, const FNFT_REAL *T,
                                       const void *d_guesses, void *d_bound_states, void *d_normconsts_or_residues,
                                       void *d_K_out, void *stream)
{
    SEAM_CHECK(!plan, plan);
    SEAM_CHECK(!d_q, q);
    SEAM_CHECK(T == NULL || T[0] >= T[1], T);
    SEAM_CHECK(!d_guesses, guesses);
    SEAM_CHECK(!d_bound_states, bound_states);
    SEAM_CHECK(!d_K_out, K_out);
    if (plan->core->guess_free()) return inv_subroutine(__func__, __LINE__, seam_invalid(__func__, __LINE__, "plan"));
    return discspec_run(plan, d_q, T, d_guesses, d_bound_states, d_normconsts_or_residues, d_K_out, stream, __func__,
                        __LINE__);
}

FNFT_INT fnft_amd_discspec_plan_finish(fnft_amd_discspec_plan_t *plan, void *stream, FNFT_INT *status,
                                       FNFT_UINT *K_out)
{
    SEAM_CHECK(!plan, plan);
    return batch_finish(
        plan, stream, status,
        [&] { return plan->core->read(plan->st, plan->kout, plan->wn, plan->last_K); },
        [&](size_t b, int h) -> FNFT_INT {
            if (K_out) K_out[b] = (FNFT_UINT)plan->kout[b];
            if (h & 8) return -FNFT_EC_OTHER;   // guess-free plans: the root finder did not converge (poly_roots_fasteigen)
            // the drop-in on this signal alone, in its order: the MODAL step-size check of the transform it runs first
            // (fnft__akns_fscatter.c:122-126), an empty bounding box, a' = 0 in the refinement or the residues -- each
            // passed on as a subroutine failure (negative)
            if (h & 1) return -FNFT_EC_OTHER;
            if (h & 4) return -FNFT_EC_INVALID_ARGUMENT;
            if (h & 2) return -FNFT_EC_DIV_BY_ZERO;
            return FNFT_SUCCESS;
        });
}

// ---- the same without guesses: FAST_EIGENVALUE and SUBSAMPLE_AND_REFINE (nft_discspec_search.h) --------------------
FNFT_UINT fnft_amd_discspec_search_plan_roots(FNFT_UINT D, fnft_nsev_opts_t const *opts, FNFT_UINT *Dsub)
{
    const fnft_nsev_opts_t o = opts ? *opts : fnft_nsev_default_opts();
    size_t ds = 0, nskip = 1, roots = 0;
    NftDiscSpecSearch<HipBackend>::sizes((size_t)D, discspec_opts(o), &ds, &nskip, &roots);
    if (Dsub) *Dsub = (FNFT_UINT)ds;
    return (FNFT_UINT)roots;
}

FNFT_INT fnft_amd_discspec_search_plan_create(fnft_amd_discspec_plan_t **plan, FNFT_UINT D, FNFT_UINT K, FNFT_UINT batch,
                                              fnft_nsev_opts_t const *opts, int device)
{
    SEAM_CHECK(!plan, plan);
    SEAM_CHECK(D < 2, D);
    SEAM_CHECK(K == 0, K);
    SEAM_CHECK(batch == 0, batch);
    const fnft_nsev_opts_t o = opts ? *opts : fnft_nsev_default_opts();
    const int disc = (int)o.discretization, loc = (int)o.bound_state_localization;
    const bool slow = disc == (int)fnft_nse_discretization_BO
                      || (disc >= (int)fnft_nse_discretization_CF4_2 && disc <= (int)fnft_nse_discretization_TES4);
    SEAM_CHECK(!slow && nft_nse_to_akns(disc) < 0, opts->discretization);
    SEAM_CHECK(loc < 0 || loc > 2, opts->bound_state_localization);
    SEAM_CHECK(loc == (int)fnft_nsev_bsloc_NEWTON, opts->bound_state_localization);   // fnft_amd_discspec_plan_create
    SEAM_CHECK((int)o.bound_state_filtering < 0 || (int)o.bound_state_filtering > 2, opts->bound_state_filtering);
    SEAM_CHECK((int)o.discspec_type < 0 || (int)o.discspec_type > 2, opts->discspec_type);
    if (slow)
        return fnft_amd__raise(FNFT_EC_NOT_YET_IMPLEMENTED, __func__, __LINE__,
                               "Not yet implemented (discretization). GPU path covers the fast (polynomial) discretizations.");
    if (const char *msg = discspec_create_refused(o, K, batch))
        return fnft_amd__raise(FNFT_EC_NOT_YET_IMPLEMENTED, __func__, __LINE__, msg);
    const NftDsOpts d = discspec_opts(o);
    size_t ds = 0, nskip = 1, roots = 0;
    NftDiscSpecSearch<HipBackend>::sizes((size_t)D, d, &ds, &nskip, &roots);
    if (roots > NftDiscSpecSearch<HipBackend>::kMaxRoots)
        return fnft_amd__raise(FNFT_EC_NOT_YET_IMPLEMENTED, __func__, __LINE__,
                               "Not yet implemented (batched discrete spectrum: more than 16384 roots per signal).");
    return batch_init(plan, batch_new<fnft_amd_discspec_plan>((size_t)D, (size_t)K, (size_t)batch, d), device);
}

FNFT_INT fnft_amd_nsev_discspec_search_device(fnft_amd_discspec_plan_t *plan, const void *d_q, const FNFT_REAL *T,
                                              void *d_bound_states, void *d_normconsts_or_residues, void *d_K_out,
                                              void *stream)
{
    SEAM_CHECK(!plan, plan);
    SEAM_CHECK(!d_q, q);
    SEAM_CHECK(T == NULL || T[0] >= T[1], T);
    SEAM_CHECK(!d_bound_states, bound_states);
    SEAM_CHECK(!d_K_out, K_out);
    if (!plan->core->guess_free()) return inv_subroutine(__func__, __LINE__, seam_invalid(__func__, __LINE__, "plan"));
    return discspec_run(plan, d_q, T, nullptr, d_bound_states, d_normconsts_or_residues, d_K_out, stream, __func__,
                        __LINE__);
}

// per-launch timers of the plan's calls, as fnft_amd_plan_set_launch_timing and its two readers
void fnft_amd_discspec_plan_set_launch_timing(fnft_amd_discspec_plan_t *plan, int enabled)
{
    if (!plan) return;
    std::lock_guard<std::mutex> lk(plan->mtx);
    plan->be.launch_timing = enabled != 0;
    plan->be.launches_used = 0;
}

FNFT_UINT fnft_amd_discspec_plan_launch_count(const fnft_amd_discspec_plan_t *plan)
{
    if (!plan) return 0;
    std::lock_guard<std::mutex> lk(const_cast<fnft_amd_discspec_plan_t *>(plan)->mtx);   // a call appends to the list
    return plan->be.launches_used;
}

double fnft_amd_discspec_plan_launch_ms(const fnft_amd_discspec_plan_t *plan, FNFT_UINT i, char *name, FNFT_UINT name_cap)
{
    if (!plan) return -1.0;
    std::lock_guard<std::mutex> lk(const_cast<fnft_amd_discspec_plan_t *>(plan)->mtx);
    return launch_ms_of(plan->be, i, name, name_cap);
}

FNFT_INT fnft_amd_discspec_plan_warnings(const fnft_amd_discspec_plan_t *plan, int *warnings)
{
    SEAM_CHECK(!plan, plan);
    SEAM_CHECK(!warnings, warnings);
    for (size_t b = 0; b < plan->core->batch; b++) warnings[b] = (b < plan->wn.size()) ? plan->wn[b] : 0;
    return FNFT_SUCCESS;
}

// ---- batched, device-resident continuous spectrum of fnft_nsev under the slow discretizations ----------------------
// Size and option checks run before any HIP call, with fnft_nsev's codes (fnft_nsev_host.c) in its order.
FNFT_INT fnft_amd_slow_plan_create(fnft_amd_slow_plan_t **plan, FNFT_UINT D, FNFT_UINT M, FNFT_UINT batch,
                                   fnft_nsev_opts_t const *opts, int device)
{
    SEAM_CHECK(!plan, plan);
    SEAM_CHECK(D < 2, D);
    SEAM_CHECK(M < 2, M);
    SEAM_CHECK(batch == 0, batch);
    fnft_nsev_opts_t o = opts ? *opts : fnft_nsev_default_opts();
    if (!opts) o.discretization = fnft_nse_discretization_BO;
    const int disc = (int)o.discretization;
    NftSlowOpts so;
    so.nse_disc = disc;
    so.cstype = (int)o.contspec_type;
    so.richardson = o.richardson_extrapolation_flag == 1 ? 1 : 0;
    if (nft_slow_scheme(disc) < 0) {
        SEAM_CHECK(nft_nse_to_akns(disc) < 0, opts->discretization);
        return fnft_amd__raise(FNFT_EC_INVALID_ARGUMENT, __func__, __LINE__,
                               "Invalid argument opts->discretization. A fast (polynomial) discretization: use "
                               "fnft_amd_plan_create.");
    }
    if (so.cstype < 0 || so.cstype > 2)   // fnft_nsev_host.c:227-233: raised inside nsev_compute_contspec, wrapped twice
        return inv_subroutine(__func__, __LINE__,
                              inv_subroutine(__func__, __LINE__, seam_invalid(__func__, __LINE__, "opts->contspec_type")));
    const int scheme = nft_slow_scheme(disc);
    SEAM_CHECK(scheme >= 1 && scheme <= 4 && D <= 2, D);   // the resampler needs more than two samples, fnft__misc.c:331-332
    auto h = batch_new<fnft_amd_slow_plan>((size_t)D, (size_t)M, (size_t)batch, so);
    if (h && h->core->too_large())
        return fnft_amd__raise(FNFT_EC_NOT_YET_IMPLEMENTED, __func__, __LINE__,
                               "Not yet implemented (slow discretizations: more than 2^31 - 1 workgroups).");
    return batch_init(plan, std::move(h), device);
}

void fnft_amd_slow_plan_destroy(fnft_amd_slow_plan_t *plan) { batch_destroy(plan); }

FNFT_UINT fnft_amd_slow_plan_chunks(FNFT_UINT D, FNFT_UINT M, FNFT_UINT batch, FNFT_UINT *points_per_chunk)
{
    if (D < 2 || M < 2 || batch == 0) return 0;
    size_t L = 0;
    const size_t nc = nft_slow_chunks((size_t)D, (size_t)M, (size_t)batch, &L);
    if (points_per_chunk) *points_per_chunk = (FNFT_UINT)L;
    return (FNFT_UINT)nc;
}

FNFT_UINT fnft_amd_slow_plan_workspace_bytes(const fnft_amd_slow_plan_t *plan)
{
    return plan ? plan->core->workspace_bytes() : 0;
}

FNFT_INT fnft_amd_nsev_slow_device(fnft_amd_slow_plan_t *plan, const void *d_q, const FNFT_REAL *T, void *d_contspec,
                                   const FNFT_REAL *XI, FNFT_INT kappa, void *stream)
{
    SEAM_CHECK(!plan, plan);
    SEAM_CHECK(!d_q, q);
    SEAM_CHECK(T == NULL || !(T[0] < T[1]), T);
    SEAM_CHECK(!d_contspec, contspec);
    SEAM_CHECK(XI == NULL || !(XI[0] < XI[1]), XI);
    SEAM_CHECK(kappa != +1 && kappa != -1, kappa);
    PlanCall call(plan->mtx, plan->device, plan->be, &plan->last_stream, stream);
    if (!call.ok) return FNFT_EC_OTHER;
    const int rc = plan->core->run((const cplx *)d_q, T, (cplx *)d_contspec, XI, (int)kappa);
    return batch_run_result(plan->be, rc, __func__, __LINE__);
}

FNFT_INT fnft_amd_slow_plan_finish(fnft_amd_slow_plan_t *plan, void *stream, FNFT_INT *status, int *warnings)
{
    SEAM_CHECK(!plan, plan);
    return batch_finish(
        plan, stream, status, [&] { return plan->core->read(plan->st, plan->wn); },
        [&](size_t b, int h) -> FNFT_INT {
            if (warnings) warnings[b] = (plan->wn[b] & 4) ? 1 : 0;
            // src/fnft_nsev.c:850-853 through the two callers that wrap it, as the fast plan reports it
            return (h & 1) ? -FNFT_EC_DIV_BY_ZERO : FNFT_SUCCESS;
        });
}

FNFT_INT fnft_amd_poly_chirpz(const FNFT_UINT deg, FNFT_COMPLEX const *const p, const double *A,
                              const double *W, const FNFT_UINT M, FNFT_COMPLEX *const result)
{
    SEAM_CHECK(!p, p);
    SEAM_CHECK(M == 0, M);
    SEAM_CHECK(!result, result);
    SEAM_CHECK(!A || !W, A);
    HostCall call(HostCall::kNoLock);
    if (!call.ok) return FNFT_EC_OTHER;
    return call.done(Plan::chirpz_host(call.be, deg, p, {A[0], A[1]}, {W[0], W[1]}, M, result));
}

FNFT_INT fnft__poly_chirpz(const FNFT_UINT deg, FNFT_COMPLEX const *const p, const FNFT_COMPLEX A,
                           const FNFT_COMPLEX W, const FNFT_UINT M, FNFT_COMPLEX *const result)
{
    const double a[2] = {A.real(), A.imag()}, w[2] = {W.real(), W.imag()};
    return fnft_amd_poly_chirpz(deg, p, a, w, M, result);
}

// include/private/fnft__poly_eval.h:43-44, :66-68 (src/private/fnft__poly_eval.c:25-53, :55-91): p at the nz points z, in
// place; the derivative goes to deriv.  KPolyEval / KPolyJoin on the current device.
static FNFT_INT poly_eval_host(const FNFT_UINT deg, FNFT_COMPLEX const *const p, const FNFT_UINT nz, FNFT_COMPLEX *const z,
                               FNFT_COMPLEX *const deriv)
{
    HostCall call;
    if (!call.ok) return FNFT_EC_OTHER;
    HipBackend &be = call.be;
    DevArena<HipBackend> tmp(be);
    cplx *dp = nullptr, *dz = nullptr, *dv = nullptr, *dd = nullptr;
    if (!tmp.get(dp, deg + 1) || !tmp.get(dz, nz) || !tmp.get(dv, nz) || (deriv && !tmp.get(dd, nz)))
        return call.done(FNFT_EC_NOMEM);
    be.h2d(dp, p, (deg + 1) * sizeof(cplx));
    be.h2d(dz, z, nz * sizeof(cplx));
    int rc = polyeval_device(be, deg, 1, 1, dp, deg + 1, deg + 1, nz, dz, 0, dv, dd);
    if (rc == NFT_SUCCESS) {
        be.d2h(z, dv, nz * sizeof(cplx));
        if (deriv) be.d2h(deriv, dd, nz * sizeof(cplx));
        rc = be.sync();
    }
    return call.done(rc);
}

FNFT_INT fnft__poly_eval(const FNFT_UINT deg, FNFT_COMPLEX const *const p, const FNFT_UINT nz, FNFT_COMPLEX *const z)
{
    SEAM_CHECK(!p, p);   // :32-35
    SEAM_CHECK(!z, z);
    if (nz == 0) return FNFT_SUCCESS;
    return poly_eval_host(deg, p, nz, z, nullptr);
}

FNFT_INT fnft__poly_evalderiv(const FNFT_UINT deg, FNFT_COMPLEX const *const p, const FNFT_UINT nz, FNFT_COMPLEX *const z,
                              FNFT_COMPLEX *const deriv)
{
    SEAM_CHECK(!p, p);   // :63-66
    SEAM_CHECK(!z, z);
    if (nz == 0) return FNFT_SUCCESS;
    SEAM_CHECK(!deriv, deriv);   // the reference would write through it
    return poly_eval_host(deg, p, nz, z, deriv);
}

// The same on device arrays, batched: npoly polynomials per signal (d_p + b*bstride + j*pstride, deg+1 coefficients,
// highest power first) at nz points per signal (d_z + b*zstride; zstride 0: one list for all signals); d_val and d_deriv
// (may be NULL) are [batch][npoly][nz].  On `stream` of the current device; waits for it once (pooled scratch).
FNFT_INT fnft_amd_poly_eval_device(FNFT_UINT deg, FNFT_UINT npoly, FNFT_UINT batch, const void *d_p, FNFT_UINT pstride,
                                   FNFT_UINT bstride, FNFT_UINT nz, const void *d_z, FNFT_UINT zstride, void *d_val,
                                   void *d_deriv, void *stream)
{
    if (!d_p || !d_z || !d_val || npoly == 0 || batch == 0 || pstride < deg + 1 || (zstride != 0 && zstride < nz))
        return FNFT_EC_INVALID_ARGUMENT;
    if (batch > 1 && bstride < deg + 1) return FNFT_EC_INVALID_ARGUMENT;
    if (nz == 0) return FNFT_SUCCESS;
    HostCall call(HostCall::kLock, stream);
    if (!call.ok) return FNFT_EC_OTHER;
    return call.done(polyeval_device(call.be, deg, npoly, batch, (const cplx *)d_p, pstride, bstride, nz, (const cplx *)d_z,
                                     zstride, (cplx *)d_val, (cplx *)d_deriv));
}

// include/private/fnft__misc.h:241-242 (src/private/fnft__misc.c:326-407): band-limited shift by delta
FNFT_INT fnft__misc_resample(const FNFT_UINT D, const FNFT_REAL eps_t, FNFT_COMPLEX const *const q,
                             const FNFT_REAL delta, FNFT_COMPLEX *const q_new)
{
    // argument checks of the reference, :331-338
    SEAM_CHECK(D <= 2, D);
    SEAM_CHECK(!q, q);
    SEAM_CHECK(!q_new, q_new);
    SEAM_CHECK(eps_t == 0.0, eps_t);
    HostCall call;
    if (!call.ok) return FNFT_EC_OTHER;
    int warn = 0;
    const FNFT_INT rc = call.done(Plan::resample_host(call.be, D, eps_t, q, delta, q_new, &warn));
    if (rc == FNFT_SUCCESS && warn) fnft_amd__warn(kNotBandlimitedMsg, "fnft__misc_resample", __LINE__);
    return rc;
}

// include/private/fnft__poly_roots_fasteigen.h (src/private/fnft__poly_roots_fasteigen.c:29-48): all roots of
// p[0] z^deg + ... + p[deg].  The reference calls eiscor's QR (Fortran); here the Ehrlich-Aberth kernels.
FNFT_INT fnft__poly_roots_fasteigen(const FNFT_UINT deg, FNFT_COMPLEX const *const p, FNFT_COMPLEX *const roots)
{
    SEAM_CHECK(!p, p);
    SEAM_CHECK(!roots, roots);
    if (deg == 0) return FNFT_SUCCESS;
    HostCall call;
    if (!call.ok) return FNFT_EC_OTHER;
    HipBackend &be = call.be;
    NftDiscSpec<HipBackend> ds(be);
    DevArena<HipBackend> tmp(be);
    cplx *d_coef = nullptr;
    if (!tmp.get(d_coef, deg + 1)) return call.done(FNFT_EC_NOMEM);
    be.h2d(d_coef, p, (deg + 1) * sizeof(cplx));
    std::vector<std::complex<double>> z;
    const int rc = ds.roots(d_coef, deg, z);
    if (rc != NFT_SUCCESS || be.failed) return call.done(-abs(rc));   // E_SUBROUTINE, :44-47
    for (size_t i = 0; i < deg; i++) roots[i] = z[i];
    return FNFT_SUCCESS;
}

// TEST SEAM ("Test seams"; not declared in include/fnft_amd.h): the batched root finder of the guess-free
// discrete spectrum alone, NftDiscSpecSearch::roots, on caller-supplied polynomials -- what emu_aberthb_roots of
// tests/emu/emu_discspec_search.cpp is over the emulator.  Every array in host memory.  coef: batch polynomials of
// degree n, n + 1 coefficients each, highest power first; each becomes entry 11 of a 4*(n + 1) block, as roots(tm)
// expects.  z: batch*n roots; per signal: mdeg, the degree the iteration ran on (without zero end coefficients), the
// status word (bit 3: not converged), the warning word (bit 1: sweep limit) and the sweeps of its AbState; sizes (may
// be NULL): {segments of the plan}
FNFT_INT fnft_amd__aberthb_roots(FNFT_UINT n, FNFT_UINT batch, FNFT_COMPLEX const *coef, FNFT_COMPLEX *z, int *mdeg,
                                 int *status, int *warn, int *sweeps, FNFT_UINT *sizes)
{
    if (n < 2 || batch == 0 || !coef || !z || !mdeg || !status || !warn || !sweeps) return FNFT_EC_INVALID_ARGUMENT;
    HostCall call;
    if (!call.ok) return FNFT_EC_OTHER;
    HipBackend &be = call.be;
    NftDsOpts o;
    o.bsfilt = 2; o.bsloc = 0; o.niter = 0; o.Dsub = 0; o.dstype = 0; o.nse_disc = 4; o.richardson = 0;   // 2SPLIT2A: n = D
    NftDiscSpecSearch<HipBackend> ds(be, n, 1, batch, o);
    int rc = ds.init();
    if (rc == NFT_SUCCESS && be.failed) rc = NFT_EC_NOMEM;
    DevArena<HipBackend> tmp(be);
    cplx *tm = nullptr;
    const size_t stride = 4 * (n + 1);
    if (rc == NFT_SUCCESS && !tmp.get(tm, batch * stride)) rc = NFT_EC_NOMEM;
    if (rc == NFT_SUCCESS) {
        std::vector<cplx> h(batch * stride, cmake(0.0, 0.0));
        for (size_t b = 0; b < batch; b++) std::memcpy(h.data() + b * stride, coef + b * (n + 1), (n + 1) * sizeof(cplx));
        be.h2d(tm, h.data(), h.size() * sizeof(cplx));
        be.memset0(ds.sstatus, batch * sizeof(int));
        be.memset0(ds.warn, batch * sizeof(int));
        ds.roots(tm);
        std::vector<AbState> st(batch);
        std::vector<cplx> zb[2] = {std::vector<cplx>(batch * n), std::vector<cplx>(batch * n)};
        be.d2h(st.data(), ds.A.state, batch * sizeof(AbState));
        be.d2h(zb[0].data(), ds.A.zbuf[0], batch * n * sizeof(cplx));
        be.d2h(zb[1].data(), ds.A.zbuf[1], batch * n * sizeof(cplx));
        be.d2h(status, ds.sstatus, batch * sizeof(int));
        be.d2h(warn, ds.warn, batch * sizeof(int));
        rc = be.sync();
        for (size_t b = 0; b < batch && rc == NFT_SUCCESS; b++) {
            std::memcpy(z + b * n, zb[st[b].zin & 1].data() + b * n, n * sizeof(cplx));
            mdeg[b] = st[b].m;
            sweeps[b] = st[b].sweeps;
        }
        if (sizes) sizes[0] = (FNFT_UINT)ds.S;
    }
    return call.done(rc);
}

// include/private/fnft__nse_scatter.h:76-80 (src/private/fnft__nse_scatter_bound_states.c:29-667) for the
// Boffetta-Osborne scheme (the one fnft_nsev uses for Newton refinement and norming constants of every
// 2SPLIT discretization): a, a' and b = phi/psi at K points lambda; q holds the D samples, r is not read
// (r = -conj(q)).  Chunk-parallel on the GPU (body_bs_*).
FNFT_INT fnft__nse_scatter_bound_states(const FNFT_UINT D, FNFT_COMPLEX const *const q, FNFT_COMPLEX *r,
                                        FNFT_REAL const *const T, FNFT_UINT K, FNFT_COMPLEX *bound_states,
                                        FNFT_COMPLEX *a_vals, FNFT_COMPLEX *aprime_vals, FNFT_COMPLEX *b,
                                        fnft_nse_discretization_t discretization, FNFT_UINT skip_b_flag)
{
    (void)r;
    // argument checks in the reference's order, :53-66
    SEAM_CHECK(D == 0, D);
    SEAM_CHECK(!q, q);
    SEAM_CHECK(!T, eps_t);
    SEAM_CHECK(K == 0, K);
    SEAM_CHECK(!bound_states, bound_states);
    SEAM_CHECK(!a_vals, a);
    SEAM_CHECK(!aprime_vals, a_prime);
    SEAM_CHECK(!skip_b_flag && !b, b);
    const bool cf42 = discretization == fnft_nse_discretization_CF4_2;
    if (discretization != fnft_nse_discretization_BO && !cf42) return FNFT_EC_NOT_YET_IMPLEMENTED;
    if (D < 2 || !(T[0] < T[1])) return FNFT_EC_INVALID_ARGUMENT;
    if (cf42 && (D % 2 != 0 || D < 4)) return FNFT_EC_ASSERTION_FAILED;   // :188-191
    HostCall call;
    if (!call.ok) return FNFT_EC_OTHER;
    HipBackend &be = call.be;
    NftDiscSpec<HipBackend> ds(be);
    NftDiscSpec<HipBackend>::Prepared P(be);
    int rc;
    if (cf42) {
        // CF4_2 (the scatterer fnft_nsev uses with 4SPLIT4A/B, :188-197): q holds the D preprocessed samples, two per
        // grid point; the grid has D/2 points on T
        P.ups = 2; P.deg0 = 4;
        P.Deff = D; P.Dsub = D / 2;
        P.T[0] = T[0]; P.T[1] = T[1];
        P.eps_t = (T[1] - T[0]) / (double)(D / 2 - 1);
        rc = P.mem.get(P.d_in, D) ? NFT_SUCCESS : NFT_EC_NOMEM;
        if (rc == NFT_SUCCESS) {
            be.h2d(P.d_in, q, D * sizeof(cplx));
            P.d_qpre = P.d_in;
        }
    } else {
        // any 2SPLIT scheme: upsampling factor 1, the slow scatterer is BO (src/fnft_nsev.c:675-680)
        rc = ds.prepare(D, (const std::complex<double> *)q, T, D, (int)fnft_nse_discretization_2SPLIT4B, P, false);
    }
    if (rc == NFT_SUCCESS)
        rc = ds.scatter(P, K, (const std::complex<double> *)bound_states, (std::complex<double> *)a_vals,
                        (std::complex<double> *)aprime_vals, (std::complex<double> *)b, skip_b_flag != 0);
    return call.done(rc);
}

// include/private/fnft__poly_roots_fftgridsearch.h (src/private/fnft__poly_roots_fftgridsearch.c:35-151 and :159-217):
// roots of a polynomial on the arc PHI of the unit circle.  *M_ptr: grid points in, estimates out; roots: *M_ptr
// entries.  The chirp z-transforms, the candidate test and the ordered compaction run on the GPU.
static FNFT_INT gridsearch_common(const size_t deg, const std::complex<double> *p, size_t *M_ptr, const double *PHI,
                                  std::complex<double> *roots, bool paraherm)
{
    HostCall call;
    if (!call.ok) return FNFT_EC_OTHER;
    HipBackend &be = call.be;
    const size_t M = *M_ptr;
    const double eps = (PHI[1] - PHI[0]) / (double)(M - 1);
    const std::complex<double> W(std::cos(eps), std::sin(eps));
    const size_t nblk = (M + 255) / 256, rings = paraherm ? 1 : 3;
    DevArena<HipBackend> tmp(be);
    cplx *vals = nullptr, *cand = nullptr, *out = nullptr;
    int *keep = nullptr, *bcnt = nullptr, *boff = nullptr, *dstatus = nullptr;
    // no early return on a failed request: the back end's failure flag decides the code below, as for any other fault
    int rc = (tmp.get(vals, rings * M) && tmp.get(cand, M) && tmp.get(out, M) && tmp.get(keep, M) && tmp.get(bcnt, nblk)
              && tmp.get(boff, nblk) && tmp.get(dstatus, 4)) ? FNFT_SUCCESS : FNFT_EC_NOMEM;
    size_t nroots = 0;
    if (rc == FNFT_SUCCESS) {
        be.memset0(dstatus, 4 * sizeof(int));
        for (size_t k = 0; k < rings && rc == FNFT_SUCCESS; k++) {
            const double scl = paraherm ? 1.0 : 1.0 + ((double)k - 1.0) * eps;      // rings k = -1, 0, 1 (:66-72)
            const std::complex<double> A = scl * std::complex<double>(std::cos(PHI[0]), -std::sin(PHI[0]));
            rc = Plan::chirpz_host(be, deg, p, A, W, M, nullptr, vals + k * M);
        }
    }
    if (rc == FNFT_SUCCESS) {
        GridSearchParams G;
        std::memset(&G, 0, sizeof(G));
        G.vals = vals; G.M = (long long)M; G.phi0 = PHI[0]; G.eps = eps; G.N1 = (long long)(deg / 2);
        G.keep = keep; G.cand = cand; G.blockcnt = bcnt; G.blockoff = boff; G.out = out; G.status = dstatus;
        if (paraherm) be.run<KGridMarkPh>((int)nblk, 1, G);
        else be.run<KGridMark>((int)nblk, 1, G);
        be.run<KCompactCount>((int)nblk, 1, G);
        std::vector<int> hc(nblk), ho(nblk);
        int hst[4] = {0, 0, 0, 0};
        be.d2h(hc.data(), bcnt, nblk * sizeof(int));
        be.d2h(hst, dstatus, sizeof(hst));
        rc = be.sync();
        if (rc == FNFT_SUCCESS && (hst[0] & 2)) rc = FNFT_EC_DIV_BY_ZERO;
        if (rc == FNFT_SUCCESS) {
            for (size_t b = 0; b < nblk; b++) { ho[b] = (int)nroots; nroots += (size_t)hc[b]; }
            be.h2d(boff, ho.data(), nblk * sizeof(int));
            be.run<KCompactScatter>((int)nblk, 1, G);
            if (nroots) be.d2h(roots, out, nroots * sizeof(cplx));
            rc = be.sync();
        }
    }
    rc = call.done(rc);
    if (rc == FNFT_SUCCESS) *M_ptr = nroots;
    return rc;
}
FNFT_INT fnft__poly_roots_fftgridsearch(const FNFT_UINT deg, FNFT_COMPLEX const *const p, FNFT_UINT *const M_ptr,
                                        FNFT_REAL const *const PHI, FNFT_COMPLEX *const roots)
{
    // argument checks in the reference's order, :46-57
    SEAM_CHECK(deg < 2, deg);
    SEAM_CHECK(!p, p);
    SEAM_CHECK(!M_ptr || *M_ptr < 2, M_ptr);
    SEAM_CHECK(!PHI || !(PHI[0] < PHI[1]) || PHI[0] == -INFINITY || PHI[1] == INFINITY, PHI);
    SEAM_CHECK(!roots, roots);
    return gridsearch_common(deg, p, M_ptr, PHI, roots, false);
}
FNFT_INT fnft__poly_roots_fftgridsearch_paraherm(const FNFT_UINT deg, FNFT_COMPLEX const *const p, FNFT_UINT *const M_ptr,
                                                 FNFT_REAL const *const PHI, FNFT_COMPLEX *const roots)
{
    // :170-180: the degree must be even
    SEAM_CHECK(deg % 2 == 1 || deg < 2, deg);
    SEAM_CHECK(!p, p);
    SEAM_CHECK(!M_ptr || *M_ptr < 2, M_ptr);
    SEAM_CHECK(!PHI || !(PHI[0] < PHI[1]) || PHI[0] == -INFINITY || PHI[1] == INFINITY, PHI);
    SEAM_CHECK(!roots, roots);
    return gridsearch_common(deg, p, M_ptr, PHI, roots, true);
}

// include/private/fnft__nse_scatter.h:119-123 (src/private/fnft__nse_scatter_matrix.c:33-86 ->
// fnft__akns_scatter_matrix.c, BO scheme): S(lambda) = U_{D-1} ... U_0 and dS/dlambda for K values of lambda -- the slow
// scatterer the periodic problem and Newton refinements call.  Chunk-parallel like the bound-state scatterer.
FNFT_INT fnft__nse_scatter_matrix(const FNFT_UINT D, FNFT_COMPLEX const *const q, FNFT_COMPLEX *r, const FNFT_REAL eps_t,
                                  const FNFT_INT kappa, const FNFT_UINT K, FNFT_COMPLEX const *const lambda,
                                  FNFT_COMPLEX *const result, fnft_nse_discretization_t discretization,
                                  const FNFT_UINT derivative_flag)
{
    // argument checks in the reference's order, :46-59
    if (D == 0 || !q || !(eps_t > 0) || (kappa != 1 && kappa != -1) || K == 0 || !lambda || !result)
        return FNFT_EC_INVALID_ARGUMENT;
    // BO, and CF4_2 (two preprocessed samples per step, each advanced with lambda/2 and the whole step eps_t; the
    // derivative picks up the factor 1/2 -- BsParams::lscale, applied by the chunk kernel:
    // src/private/fnft__akns_scatter_matrix.c:122-130,201-208)
    const bool cf42 = discretization == fnft_nse_discretization_CF4_2;
    if (discretization != fnft_nse_discretization_BO && !cf42) return FNFT_EC_NOT_YET_IMPLEMENTED;
    if (cf42 && D % 2 != 0) return FNFT_EC_ASSERTION_FAILED;
    HostCall call;
    if (!call.ok) return FNFT_EC_OTHER;
    HipBackend &be = call.be;
    BsParams B;
    std::memset(&B, 0, sizeof(B));
    const size_t L = nft_bs_chunk_len(D);
    const size_t nchunk = (D + L - 1) / L;
    const size_t w = derivative_flag ? 8 : 4;
    DevArena<HipBackend> tmp(be);
    cplx *dq = nullptr, *dr = nullptr, *dl = nullptr, *cm = nullptr, *ds = nullptr;
    // no early return on a failed request: the back end's failure flag decides the code below, as for any other fault
    int rc = (tmp.get(dq, D) && (!r || tmp.get(dr, D)) && tmp.get(dl, K) && tmp.get(cm, K * nchunk * 8)
              && tmp.get(ds, K * w)) ? FNFT_SUCCESS : FNFT_EC_NOMEM;
    if (rc == FNFT_SUCCESS) {
        be.h2d(dq, q, D * sizeof(cplx));
        if (r) be.h2d(dr, r, D * sizeof(cplx));
        be.h2d(dl, lambda, K * sizeof(cplx));
        B.q = dq; B.r = dr; B.kappa = (int)kappa; B.D = (long long)D; B.ups = cf42 ? 2 : 1; B.lscale = cf42 ? 0.5 : 1.0;
        B.eps = eps_t;
        B.K = (int)K; B.lam = dl; B.L = (int)L; B.nchunk = (int)nchunk; B.cm = cm; B.smat = ds;
        B.with_deriv = derivative_flag ? 1 : 0;
        for (size_t k0 = 0; k0 < K; k0 += 32768) {   // grid.y limit
            const size_t kn = std::min<size_t>(32768, K - k0);
            BsParams Bk = B;
            Bk.K = (int)kn; Bk.lam = dl + k0; Bk.cm = cm + k0 * nchunk * 8; Bk.smat = ds + k0 * w;
            be.run<KBsChunk<false>>((int)((nchunk + 63) / 64), (int)kn, Bk);
            be.run<KBsMatrix>((int)kn, 1, Bk);
        }
        be.d2h(result, ds, K * w * sizeof(cplx));
        rc = be.sync();
    }
    return call.done(rc);
}

FNFT_UINT fnft__akns_fscatter_numel(FNFT_UINT D, fnft__akns_discretization_t discretization)
{
    const int deg = nft_akns_degree((int)discretization);
    return deg == 0 ? 0 : fnft__poly_fmult2x2_numel((FNFT_UINT)deg, D);
}

FNFT_INT fnft__akns_fscatter(const FNFT_UINT D, FNFT_COMPLEX const *const q,
                             FNFT_COMPLEX const *const r, const FNFT_REAL eps_t,
                             FNFT_COMPLEX *const result, FNFT_UINT *const deg_ptr,
                             FNFT_INT *const W_ptr, fnft__akns_discretization_t discretization)
{
    // argument checks in the reference's order, src/private/fnft__akns_fscatter.c:80-97
    SEAM_CHECK(D == 0, D);
    SEAM_CHECK(!q, q);
    SEAM_CHECK(!r, r);
    SEAM_CHECK(!(eps_t > 0.0), eps_t);
    SEAM_CHECK(!result, result);
    SEAM_CHECK(!deg_ptr, deg_ptr);
    SEAM_CHECK(nft_akns_degree((int)discretization) == 0, discretization);
    HostCall call(HostCall::kNoLock);
    if (!call.ok) return FNFT_EC_OTHER;
    return call.done(api_akns_fscatter(call.be, D, q, r, eps_t, 1, result, deg_ptr, W_ptr, (int)discretization));
}

FNFT_UINT fnft__nse_fscatter_numel(FNFT_UINT D, fnft_nse_discretization_t discretization)
{
    const int a = nft_nse_to_akns((int)discretization);
    return a < 0 ? 0 : fnft__akns_fscatter_numel(D, (fnft__akns_discretization_t)a);
}

FNFT_INT fnft__nse_fscatter(const FNFT_UINT D, FNFT_COMPLEX const *const q, const FNFT_REAL eps_t,
                            const FNFT_INT kappa, FNFT_COMPLEX *const result,
                            FNFT_UINT *const deg_ptr, FNFT_INT *const W_ptr,
                            fnft_nse_discretization_t discretization)
{
    // src/private/fnft__nse_fscatter.c:55-69
    if (D == 0 || !q || !(eps_t > 0.0) || (kappa != 1 && kappa != -1) || !result || !deg_ptr)
        return FNFT_EC_INVALID_ARGUMENT;
    const int a = nft_nse_to_akns((int)discretization);
    if (a < 0) return FNFT_EC_INVALID_ARGUMENT;
    HostCall call(HostCall::kNoLock);
    if (!call.ok) return FNFT_EC_OTHER;
    return call.done(api_akns_fscatter(call.be, D, q, nullptr, eps_t, kappa, result, deg_ptr, W_ptr, a));
}

// 4SPLIT4A / 4SPLIT4B of the KdV seams: per-sample formulas and degrees of 2SPLIT4A / 2SPLIT4B on the samples as they
// are (src/private/fnft__kdv_discretization.c:139-143; kdv_fscatter does not resample)
static int kdv_alias(int kd)
{
    if (kd == (int)fnft_kdv_discretization_4SPLIT4A) return (int)fnft_kdv_discretization_2SPLIT4A;
    if (kd == (int)fnft_kdv_discretization_4SPLIT4B) return (int)fnft_kdv_discretization_2SPLIT4B;
    return kd;
}

FNFT_UINT fnft__kdv_fscatter_numel(FNFT_UINT D, fnft_kdv_discretization_t discretization)
{
    const int kd = kdv_alias((int)discretization);
    if (kd < 0 || kd > (int)fnft_kdv_discretization_2SPLIT8B) return 0;
    return fnft__poly_fmult2x2_numel((FNFT_UINT)nft_akns_degree(kd + 1), D);
}

// src/private/fnft__kdv_fscatter.c:45-83
FNFT_INT fnft__kdv_fscatter(const FNFT_UINT D, FNFT_COMPLEX const *const u, const FNFT_REAL eps_t,
                            FNFT_COMPLEX *const result, FNFT_UINT *const deg_ptr, FNFT_INT *const W_ptr,
                            fnft_kdv_discretization_t discretization)
{
    SEAM_CHECK(D == 0, D);
    SEAM_CHECK(!u, u);
    SEAM_CHECK(!(eps_t > 0.0), eps_t);
    SEAM_CHECK(!result, result);
    SEAM_CHECK(!deg_ptr, deg_ptr);
    const int kd = kdv_alias((int)discretization);
    if (kd < 0 || kd > (int)fnft_kdv_discretization_2SPLIT8B) return FNFT_EC_INVALID_ARGUMENT;
    HostCall call(HostCall::kNoLock);
    if (!call.ok) return FNFT_EC_OTHER;
    return call.done(api_kdv_fscatter(call.be, D, (const std::complex<double> *)u, eps_t, (std::complex<double> *)result,
                                      deg_ptr, W_ptr, kd + 1));
}

// internal entry used by fnft_kdvv_host.c: host buffers in and out, plans cached per (D, M, scheme)
FNFT_INT fnft_amd__kdvv_contspec_host(FNFT_UINT D, const FNFT_COMPLEX *u, const FNFT_REAL *T, FNFT_UINT M,
                                      FNFT_COMPLEX *contspec, const FNFT_REAL *XI, int discretization)
{
    HostCall call;
    if (!call.ok) return FNFT_EC_OTHER;
    fnft_amd_plan *P = nullptr;
    const FNFT_INT rc = call.hs->kdvv.get(std::make_tuple((size_t)D, (size_t)M, discretization), &P, [&](fnft_amd_plan **h) {
        return fnft_amd_kdvv_plan_create(h, D, M, 1, (fnft_kdv_discretization_t)discretization, call.dev);
    });
    if (rc != FNFT_SUCCESS) return call.done(rc);
    {   // the potential is in host memory: look at it here instead of asking the device
        bool real = true;
        const std::complex<double> *uh = (const std::complex<double> *)u;
        for (size_t i = 0; i < D && real; i++) real = (uh[i].imag() == 0.0);
        P->real_mode = real ? 1 : 0;
    }
    return staged_run(call, u, D, contspec, M, [&](cplx *du, cplx *dcs) {
        const FNFT_INT r = fnft_amd_kdvv_contspec_device(P, du, dcs, T, XI, nullptr);
        return r == FNFT_SUCCESS ? fnft_amd_plan_finish(P, nullptr) : r;
    });
}

// internal entry used by fnft_nsev_host.c: discrete spectrum (kappa = +1), host buffers.
// *K_ptr: capacity of bound_states in, number of bound states out.  *warn: more were found than fit.
FNFT_INT fnft_amd__nsev_discspec_host(FNFT_UINT D, const FNFT_COMPLEX *q, const FNFT_REAL *T, int bsfilt,
                                      int bsloc, FNFT_UINT niter, FNFT_UINT Dsub, int dstype, int discretization,
                                      int richardson, FNFT_UINT *K_ptr, FNFT_COMPLEX *bound_states,
                                      FNFT_COMPLEX *normconsts_or_residues, int *warn)
{
    HostCall call;
    if (!call.ok) return FNFT_EC_OTHER;
    NftDiscSpec<HipBackend> ds(call.be);
    NftDsOpts o;
    o.bsfilt = bsfilt; o.bsloc = bsloc; o.niter = niter; o.Dsub = Dsub; o.dstype = dstype;
    o.nse_disc = discretization; o.richardson = richardson;
    size_t K = *K_ptr;
    const FNFT_INT rc = call.done(ds.run(D, (const std::complex<double> *)q, T, o, &K, (std::complex<double> *)bound_states,
                                         (std::complex<double> *)normconsts_or_residues));
    if (warn) *warn = (ds.warn_more_than_K ? 1 : 0) | (ds.warn_roots_unconverged ? 2 : 0);
    if (rc == NFT_SUCCESS) *K_ptr = K;
    return rc;
}

// ---- internal entry used by the C driver (fnft_nsev_host.c) ------------------------------------
// Host buffers in, host buffers out; plans are cached per (D, M, discretization, nskip).
// nskip > 1 (4SPLIT4A/B only): the transform of every nskip-th step of the D samples, as
// fnft__nse_discretization_preprocess_signal forms it for Richardson extrapolation.
FNFT_INT fnft_amd__nsev_contspec_host(FNFT_UINT D, const FNFT_COMPLEX *q, const FNFT_REAL *T,
                                      FNFT_UINT M, FNFT_COMPLEX *contspec, const FNFT_REAL *XI,
                                      FNFT_INT kappa, int discretization, int contspec_type,
                                      FNFT_INT normalization_flag, FNFT_UINT nskip)
{
    HostCall call;
    if (!call.ok) return FNFT_EC_OTHER;
    fnft_amd_plan *P = nullptr;
    const FNFT_INT rc = call.hs->nsev.get(
        std::make_tuple((size_t)D, (size_t)M, discretization, (size_t)nskip), &P, [&](fnft_amd_plan **h) {
            return fnft_amd_plan_create_sub(h, D, M, 1, (fnft_nse_discretization_t)discretization, call.dev, nskip);
        });
    if (rc != FNFT_SUCCESS) return call.done(rc);
    const size_t cs_len = M * (contspec_type == 0 ? 1 : (contspec_type == 1 ? 2 : 3));
    return staged_run(call, q, D, contspec, cs_len, [&](cplx *dq, cplx *dcs) {
        FNFT_INT r = fnft_amd_nsev_contspec_device(P, dq, contspec ? dcs : nullptr, T, XI, kappa,
                                                   (fnft_nsev_cstype_t)contspec_type, normalization_flag, nullptr);
        if (r == FNFT_SUCCESS) r = fnft_amd_plan_finish(P, nullptr);
        // the resampler of the 4SPLIT4A/B front end warns when the spectrum has not decayed (fnft__misc.c:371-381)
        if (fnft_amd_plan_last_warnings(P) & 1) fnft_amd__warn(kNotBandlimitedMsg, "fnft__misc_resample", __LINE__);
        return r;
    });
}

// Everything the host-pointer entry points keep on `device` between calls goes back to the driver: cached plans, the
// resident layer-peeling state of fnft__nse_finvscatter / fnft_nsev_inverse, and the cache of released device blocks.
// device < 0: every device.  Device-resident plans the caller created are not touched.
void fnft_amd_release_cached(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) return;
    for (int d = 0; d < ndev; d++) {
        if (device >= 0 && d != device) continue;
        HostState &hs = host_state(d);
        std::lock_guard<std::mutex> host_lk(hs.mtx);
        hs.nsev.clear();
        hs.kdvv.clear();
        DeviceGuard dg(d);
        if (dg.ok) {
            (void)hipDeviceSynchronize();
            hs.peeler.lp.destroy();
        }
        DevPool &P = pool();
        std::lock_guard<std::mutex> lk(P.m);
        P.trim_locked(d);
    }
}

}  // extern "C"
