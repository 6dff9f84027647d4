// emu_alloc_balance.cpp -- every plan class over a back end that counts: what init() requests, what the plan's arena
// (fnft_amd/csrc/nft_arena.h) reports, and that everything is handed back exactly once when the plan goes out of scope,
// after a successful init() and after one that ran out of memory at its n-th request (TEST INFRASTRUCTURE ONLY, its own
// shared object; see emu_backend.h).  No kernel executes (schedule-only mode).
#include <set>

#include "emu_backend.h"

thread_local fa_emu_ctx *fa_emu = nullptr;

#include "../../fnft_amd/csrc/nft_discspec_batch.h"
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

// init() of one plan; *class_bytes: the plan's own count while it is alive
static int init_one(CountingBackend &be, int kind, const long long *a, size_t *class_bytes)
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
    default: return -1;
    }
}

extern "C" {

// out = {requests made, blocks live after the plan is gone, bytes requested and served, the plan's own byte count,
// bad frees}; returns init()'s code
int emu_alloc_balance(int kind, const long long *a, long fail_at, unsigned long long *out)
{
    CountingBackend be;
    be.fail_at = fail_at;
    std::vector<std::string> names;
    emu_schedule = &names;
    size_t class_bytes = 0;
    const int rc = init_one(be, kind, a, &class_bytes);
    emu_schedule = nullptr;
    out[0] = (unsigned long long)be.nalloc;
    out[1] = be.live.size();
    out[2] = be.requested;
    out[3] = class_bytes;
    out[4] = (unsigned long long)be.bad_free;
    for (void *p : be.live) std::free(p);
    return rc;
}

}  // extern "C"
