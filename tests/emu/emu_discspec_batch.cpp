// emu_discspec_batch.cpp -- the batched discrete spectrum (fnft_amd/csrc/nft_discspec_batch.h and the body_ds_*
// kernels) in the CPU lane emulator (TEST INFRASTRUCTURE ONLY, its own shared object; see emu_backend.h).
#include "emu_backend.h"

thread_local fa_emu_ctx *fa_emu = nullptr;

#include "../../fnft_amd/csrc/nft_discspec_batch.h"

extern "C" {

// every array in host memory; status: the device status words (bit 0 MODAL step check, bit 1 a' = 0, bit 2 empty box)
int emu_discspec_batch(size_t D, size_t K, size_t batch, int nse_disc, size_t niter, int bsfilt, int dstype,
                       const cplx *q, const double *T, const cplx *guesses, cplx *bound_states, cplx *normconsts,
                       unsigned long long *K_out, int *status)
{
    EmuBackend be;
    NftDsOpts o;
    o.bsfilt = bsfilt; o.bsloc = 1; o.niter = niter; o.Dsub = 0; o.dstype = dstype; o.nse_disc = nse_disc;
    o.richardson = 0;
    NftDiscSpecBatch<EmuBackend> ds(be, D, K, batch, o);
    int rc = ds.init();
    if (rc == NFT_SUCCESS) rc = ds.run(q, T, guesses, bound_states, normconsts, K_out);
    if (rc == NFT_SUCCESS) {
        std::vector<int> st;
        std::vector<unsigned long long> ko;
        rc = ds.read(st, ko, K_out);
        for (size_t b = 0; b < batch; b++) status[b] = st[b];
    }
    return rc;
}

// LDS bytes of the kernels and the sample count up to which a signal is staged in LDS
size_t emu_discspec_lds_bytes(int which)
{
    switch (which) {
    case 0: return KDsNewton<false>::lds_bytes();
    case 1: return KDsNewton<true>::lds_bytes();
    case 2: return KDsNorm<false>::lds_bytes();
    case 3: return KDsNorm<true>::lds_bytes();
    default: return (size_t)kDsLdsSamples;
    }
}

}  // extern "C"
