// emu_richardson.cpp -- builds tests/emu/libfnft_emu_richardson.so: Richardson extrapolation of the batched nsev plans
// (NftPlan::enable_richardson / run_richardson, nft_discspec_plan.h, KRichCombineCs, KRichMatchDs) in the CPU lane
// emulator (TEST INFRASTRUCTURE ONLY; see emu_backend.h).
#include "emu_backend.h"

thread_local fa_emu_ctx *fa_emu = nullptr;

#include "../../fnft_amd/csrc/nft_discspec_plan.h"

extern "C" {

// The tree plan as fnft_amd_nsev_contspec_device drives it, with fnft_amd_plan_set_richardson(plan, richardson) before
// the call: contspec receives batch * parts * M values; returns what fnft_amd_plan_finish returns.
int emu_rich_contspec(size_t D, size_t M, size_t batch, int disc, int kappa, int cstype, int richardson, const cplx *q,
                      const double *T, const double *XI, cplx *contspec)
{
    EmuBackend be;
    using P = NftPlan<EmuBackend>;
    const int akns = nft_nse_to_akns(disc);
    if (akns < 0) return NFT_EC_INVALID_ARGUMENT;
    const int ups = nft_nse_upsampling(disc);
    P pl(be, (size_t)ups * D, M, batch, akns, nft_akns_degree(akns));
    pl.set_front(D, 1, ups);
    int rc = pl.init();
    if (rc == NFT_SUCCESS && richardson) rc = pl.enable_richardson();
    if (rc != NFT_SUCCESS) return rc;
    double Tsub[2];
    rc = pl.run_front(q, T, kappa, Tsub);
    if (rc == NFT_SUCCESS) rc = pl.run_tree();
    if (rc == NFT_SUCCESS) {
        P::Contspec cs;
        cs.T[0] = Tsub[0]; cs.T[1] = Tsub[1]; cs.XI[0] = XI[0]; cs.XI[1] = XI[1];
        cs.nse_disc = disc; cs.cstype = cstype; cs.normalization_flag = 1;
        rc = pl.run_contspec(contspec, cs);
        if (rc == NFT_SUCCESS && pl.rich_on) rc = pl.run_richardson(q, T, kappa, contspec, cs);
    }
    if (rc != NFT_SUCCESS) return rc;
    return pl.read_status();
}

// The discrete-spectrum plan (NftDiscSpecPlan) as fnft_amd_nsev_discspec_device / fnft_amd_nsev_discspec_search_device
// drive it, with fnft_amd_discspec_plan_set_richardson(plan, richardson) before the call.  bsloc 1: a guess plan; 0, 2:
// a guess-free plan (guesses NULL, Dsub as in the options; one segment per sweep).  Every array in host memory, status:
// the device status words
int emu_rich_discspec(size_t D, size_t K, size_t batch, int nse_disc, int bsloc, size_t niter, size_t Dsub, int bsfilt,
                      int dstype, int richardson, const cplx *q, const double *T, const cplx *guesses, cplx *bound_states,
                      cplx *normconsts, unsigned long long *K_out, int *status)
{
    EmuBackendOneSegment be;
    NftDsOpts o;
    o.bsfilt = bsfilt; o.bsloc = bsloc; o.niter = niter; o.Dsub = Dsub; o.dstype = dstype; o.nse_disc = nse_disc;
    o.richardson = 0;
    NftDiscSpecPlan<EmuBackendOneSegment> ds(be, D, K, batch, o);
    int rc = ds.init();
    if (rc == NFT_SUCCESS && richardson) rc = ds.enable_richardson();
    if (rc == NFT_SUCCESS) rc = ds.run(q, T, guesses, bound_states, normconsts, K_out);
    if (rc == NFT_SUCCESS) {
        std::vector<int> st, wn;
        std::vector<unsigned long long> ko;
        rc = ds.read(st, ko, wn, K_out);
        for (size_t b = 0; b < batch; b++) status[b] = st[b];
    }
    return rc;
}

// KRichMatchDs alone on the caller's arrays: nc, nc_s in the BOTH layout (2K per signal) or NULL; res: K per signal
int emu_rich_match(size_t K, size_t batch, double thr, double sn, double sd, cplx *bs, const cplx *bs_s,
                   const unsigned long long *K_out, const unsigned long long *Ks_out, const cplx *nc, const cplx *nc_s,
                   cplx *res, int *status, const int *status_s)
{
    EmuBackend be;
    RichDsParams R;
    std::memset(&R, 0, sizeof(R));
    R.bs = bs; R.bs_s = bs_s; R.K_out = K_out; R.Ks_out = Ks_out;
    R.nc = nc; R.nc_s = nc_s; R.res = res;
    R.res_stride = (long long)K; R.res_off = 0;
    R.K = (int)K;
    R.thr = thr; R.sn = sn; R.sd = sd;
    R.status = status; R.status_s = status_s;
    be.run<KRichMatchDs>((int)batch, 1, R);
    return (int)kRichTile;
}

// the kernel names of FA_ALL_UNITS (which = 0), FA_EXT_UNITS (1) or FA_EXT2_UNITS (2), '\n'-separated; their number
int emu_rich_kernel_list(int which, char *out, size_t cap)
{
    std::vector<std::string> v;
#define FA_EMU_NAME(...) v.push_back(emu_kernel_name<__VA_ARGS__>());
    if (which == 2) { FA_EXT2_UNITS(FA_EMU_NAME) }
    else if (which == 1) { FA_EXT_UNITS(FA_EMU_NAME) }
    else { FA_ALL_UNITS(FA_EMU_NAME) }
#undef FA_EMU_NAME
    std::string s;
    for (const auto &n : v) s += n + "\n";
    if (s.size() + 1 > cap) return -1;
    std::memcpy(out, s.c_str(), s.size() + 1);
    return (int)v.size();
}

}  // extern "C"
