// emu_alloc_balance.cpp -- every plan class over a back end that counts: what init() requests, what the plan's arena
// (fnft_amd/csrc/nft_arena.h) reports, and that everything is handed back exactly once when the plan goes out of scope,
// after a successful init() and after one that ran out of memory at its n-th request (TEST INFRASTRUCTURE ONLY, its own
// shared object; see emu_backend.h).  No kernel executes (schedule-only mode).
#include <set>

#include "emu_backend.h"

thread_local fa_emu_ctx *fa_emu = nullptr;

#include "../../fnft_amd/csrc/nft_discspec_plan.h"
#include "../../fnft_amd/csrc/nft_nsev_inverse.h"
#include "../../fnft_amd/csrc/nft_nsev_slow.h"

struct CountingBackend : EmuBackend {
    std::set<void *> live;
    size_t requested = 0;      // bytes of the requests that were served
    long nalloc = 0;           // requests so far, served or not
    long fail_at = -1;         // the request (counted from 0) that finds no memory
    int bad_free = 0;          // blocks handed back that are not live: unknown, null or freed twice
    void *alloc(size_t b)
    {
        if (nalloc++ == fail_at) return nullptr;
        void *p = EmuBackend::alloc(b);
        if (p) { live.insert(p); requested += b; }
        return p;
    }
    void free(void *p)
    {
        if (live.erase(p) != 1) { bad_free++; return; }
        EmuBackend::free(p);
    }
};

// the options of kind 7 (those of kind 2 with a[4] as the localization): FULL, niter 10, the default Dsub, BOTH
static NftDsOpts ds_plan_opts(const long long *a)
{
    NftDsOpts o;
    o.bsfilt = 2; o.bsloc = (int)a[4]; o.niter = 10; o.Dsub = 0; o.dstype = 2; o.nse_disc = (int)a[3]; o.richardson = 0;
    return o;
}

// init() of one plan or part; *class_bytes: its own count while it is alive (a part: the count of the arena it was given);
// *inner_bytes: kind 6, the count of the plan without the tables it borrows; kind 7, what a failing enable_richardson()
// left wrong (0: nothing)
static int init_one(CountingBackend &be, int kind, const long long *a, size_t *class_bytes, size_t *inner_bytes)
{
    typedef CountingBackend BE;
    switch (kind) {
    case 0: {   // NftPlan: a = {D of the tree, M, batch, akns, deg0, Din, ups, kdv}
        NftPlan<BE> pl(be, (size_t)a[0], (size_t)a[1], (size_t)a[2], (int)a[3], (int)a[4]);
        pl.set_front((size_t)a[5], 1, (int)a[6]);
        pl.kdv = a[7] != 0;
        const int rc = pl.init();
        *class_bytes = pl.mem.bytes;
        return rc;
    }
    case 1: {   // NftSlowPlan: a = {D, M, batch, nse_disc, cstype, richardson}
        NftSlowOpts o;
        o.nse_disc = (int)a[3]; o.cstype = (int)a[4]; o.richardson = (int)a[5];
        NftSlowPlan<BE> sp(be, (size_t)a[0], (size_t)a[1], (size_t)a[2], o);
        const int rc = sp.init();
        *class_bytes = sp.workspace_bytes();
        return rc;
    }
    case 2: {   // NftDiscSpecBatch: a = {D, K, batch, nse_disc}
        NftDsOpts o;
        o.bsfilt = 2; o.bsloc = 1; o.niter = 10; o.Dsub = 0; o.dstype = 2; o.nse_disc = (int)a[3]; o.richardson = 0;
        NftDiscSpecBatch<BE> ds(be, (size_t)a[0], (size_t)a[1], (size_t)a[2], o);
        const int rc = ds.init();
        *class_bytes = ds.workspace_bytes();
        return rc;
    }
    case 3: {   // NftInverseBatch: a = {D, M, batch, cstype, oversampling, modal, K, ds_mode, residues}
        NftInverseBatch<BE> inv(be, (size_t)a[0], (size_t)a[1], (size_t)a[2], (int)a[3], (size_t)a[4], (int)a[5],
                                (size_t)a[6], (int)a[7], (int)a[8]);
        const int rc = inv.init();
        *class_bytes = inv.workspace_bytes();
        return rc;
    }
    case 4: {   // NftResampler alone: a = {Din, batch}
        DevArena<BE> mem(be);
        NftTwiddles<BE> tw;
        NftResampler<BE> rs(be, tw);
        const int rc = tw.init(mem) ? rs.init(mem, (size_t)a[0], (size_t)a[1]) : NFT_EC_NOMEM;
        *class_bytes = mem.bytes;
        return rc;
    }
    case 5: {   // NftAnyDft alone: a = {nmax, jobs}
        DevArena<BE> mem(be);
        NftTwiddles<BE> tw;
        NftAnyDft<BE> ft(be, tw);
        const int rc = tw.init(mem) ? ft.init(mem, (size_t)a[0], (size_t)a[1]) : NFT_EC_NOMEM;
        *class_bytes = mem.bytes;
        return rc;
    }
    case 6: {   // NftPlan on borrowed tables: a as for kind 0
        DevArena<BE> mem(be);
        NftTwiddles<BE> tw;
        if (!tw.init(mem, a[7] != 0)) return NFT_EC_NOMEM;
        NftPlan<BE> pl(be, (size_t)a[0], (size_t)a[1], (size_t)a[2], (int)a[3], (int)a[4], &tw);
        pl.set_front((size_t)a[5], 1, (int)a[6]);
        pl.kdv = a[7] != 0;
        const int rc = pl.init();
        *inner_bytes = pl.mem.bytes;
        *class_bytes = mem.bytes + pl.mem.bytes;
        return rc;
    }
    case 7: {   // NftDiscSpecPlan: a = {D, K, batch, nse_disc, bsloc, Richardson}
        NftDiscSpecPlan<BE> pl(be, (size_t)a[0], (size_t)a[1], (size_t)a[2], ds_plan_opts(a));
        int rc = pl.init();
        if (rc == NFT_SUCCESS && a[5]) {
            const size_t before = be.live.size();
            rc = pl.enable_richardson();
            if (rc != NFT_SUCCESS) {   // blocks it left behind while the plan lives; 2^20: the plan no longer runs as it did
                cplx *dummy = (cplx *)pl.fine_status();   // schedule-only: no kernel reads the caller's arrays
                const double T[2] = {-1.0, 1.0};
                const bool runs = !pl.rich_on && !pl.rich_ready()
                                  && pl.run(dummy, T, dummy, dummy, dummy, (unsigned long long *)dummy) == NFT_SUCCESS;
                *inner_bytes = (be.live.size() - before) + (runs ? 0 : (size_t)1 << 20);
            }
        }
        *class_bytes = pl.workspace_bytes();
        return rc;
    }
    default: return -1;
    }
}

extern "C" {

// out = {requests made, blocks live after the plan is gone, bytes requested and served, the plan's own byte count,
// bad frees, kind 6: the plan's count without the borrowed tables, kind 7: what a failing enable_richardson() left wrong};
// returns init()'s code (kind 7 with Richardson: enable_richardson()'s after a successful init())
int emu_alloc_balance(int kind, const long long *a, long fail_at, unsigned long long *out)
{
    CountingBackend be;
    be.fail_at = fail_at;
    std::vector<std::string> names;
    emu_schedule = &names;
    size_t class_bytes = 0, inner_bytes = 0;
    const int rc = init_one(be, kind, a, &class_bytes, &inner_bytes);
    emu_schedule = nullptr;
    out[0] = (unsigned long long)be.nalloc;
    out[1] = be.live.size();
    out[2] = be.requested;
    out[3] = class_bytes;
    out[4] = (unsigned long long)be.bad_free;
    out[5] = inner_bytes;
    for (void *p : be.live) std::free(p);
    return rc;
}

// Schedule of one run() of a batched plan class without executing it (schedule-only mode, as emu_tree_schedule of
// emu_main.cpp): kind and a as in init_one (kinds 1 .. 3 and 7); the names of every kernel that init() and run() launch,
// '\n'-separated, into out[cap].  Nothing executes, so one dummy address stands for every device array of the caller.
// Returns the plan's rc, or -1 if out is too small.
int emu_plan_schedule(int kind, const long long *a, char *out, size_t cap)
{
    EmuBackend be;
    std::vector<std::string> names;
    emu_schedule = &names;
    cplx *dummy = (cplx *)be.alloc(16);
    const double T[2] = {-1.0, 1.0}, XI[2] = {-0.5, 0.7};
    int rc = NFT_EC_INVALID_ARGUMENT;
    if (kind == 1) {
        NftSlowOpts o;
        o.nse_disc = (int)a[3]; o.cstype = (int)a[4]; o.richardson = (int)a[5];
        NftSlowPlan<EmuBackend> sp(be, (size_t)a[0], (size_t)a[1], (size_t)a[2], o);
        rc = sp.init();
        if (rc == NFT_SUCCESS) rc = sp.run(dummy, T, dummy, XI, +1);
    } else if (kind == 2) {
        NftDsOpts o;
        o.bsfilt = 2; o.bsloc = 1; o.niter = 10; o.Dsub = 0; o.dstype = 2; o.nse_disc = (int)a[3]; o.richardson = 0;
        NftDiscSpecBatch<EmuBackend> ds(be, (size_t)a[0], (size_t)a[1], (size_t)a[2], o);
        rc = ds.init();
        if (rc == NFT_SUCCESS) rc = ds.run(dummy, T, dummy, dummy, dummy, (unsigned long long *)dummy);
    } else if (kind == 7) {
        NftDiscSpecPlan<EmuBackend> pl(be, (size_t)a[0], (size_t)a[1], (size_t)a[2], ds_plan_opts(a));
        rc = pl.init();
        if (rc == NFT_SUCCESS && a[5]) rc = pl.enable_richardson();
        if (rc == NFT_SUCCESS)
            rc = pl.run(dummy, T, pl.guess_free() ? nullptr : dummy, dummy, dummy, (unsigned long long *)dummy);
    } else if (kind == 3) {
        NftInverseBatch<EmuBackend> inv(be, (size_t)a[0], (size_t)a[1], (size_t)a[2], (int)a[3], (size_t)a[4], (int)a[5],
                                        (size_t)a[6], (int)a[7], (int)a[8]);
        rc = inv.init();
        const double eps_t = (T[1] - T[0]) / (double)(a[0] - 1);
        if (rc == NFT_SUCCESS)
            rc = a[6] ? inv.run_discrete(dummy, XI, dummy, dummy, dummy, T, eps_t, +1, 0.0)
                      : inv.run(dummy, XI, dummy, eps_t, +1, 0.0);
    }
    be.free(dummy);
    emu_schedule = nullptr;
    std::string s;
    for (const auto &n : names) s += n + "\n";
    if (s.size() + 1 > cap) return -1;
    std::memcpy(out, s.c_str(), s.size() + 1);
    return rc;
}

}  // extern "C"
