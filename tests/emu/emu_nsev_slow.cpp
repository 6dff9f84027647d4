// emu_nsev_slow.cpp -- the slow-discretization plan (fnft_amd/csrc/nft_nsev_slow.h and the body_slow_* kernels) in the
// CPU lane emulator (TEST INFRASTRUCTURE ONLY, its own shared object; see emu_backend.h).
#include "emu_backend.h"

thread_local fa_emu_ctx *fa_emu = nullptr;

#include "../../fnft_amd/csrc/nft_nsev_slow.h"

extern "C" {

// every array in host memory; status: bit 0 a(xi) == 0; warn: bit 2 not band-limited
int emu_nsev_slow(size_t D, size_t M, size_t batch, int nse_disc, int cstype, int richardson, const cplx *q,
                  const double *T, const double *XI, int kappa, cplx *out, int *status, int *warn)
{
    EmuBackend be;
    NftSlowOpts o;
    o.nse_disc = nse_disc; o.cstype = cstype; o.richardson = richardson;
    NftSlowPlan<EmuBackend> sp(be, D, M, batch, o);
    int rc = sp.init();
    if (rc == NFT_SUCCESS) rc = sp.run(q, T, out, XI, kappa);
    if (rc == NFT_SUCCESS) {
        std::vector<int> st, wn;
        rc = sp.read(st, wn);
        for (size_t b = 0; b < batch; b++) { status[b] = st[b]; warn[b] = wn[b]; }
    }
    return rc;
}

}  // extern "C"
