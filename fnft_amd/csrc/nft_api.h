// nft_api.h -- host-pointer entry points (the reference's private-layer signatures) expressed
// over NftPlan<BE>.  Instantiated with the HIP back end in hip_backend.hip (product) and with
// the lane emulator in tests/emu (tests only).
#pragma once
#include "nft_plan.h"

// the root of the tree to the caller: export, read back W, coefficients times 2^W if the caller takes no exponent.
// use_status: wait through pl.read_status() (the scatterers: its bits are theirs to raise), else a plain sync
template <class BE>
int api_export_result(NftPlan<BE> &pl, std::complex<double> *result, size_t *deg_ptr, int32_t *W_ptr, bool use_status)
{
    BE &be = pl.be;
    pl.export_tm();
    const size_t cnt = 4 * (pl.res_deg + 1);
    be.d2h(result, pl.tm_out, cnt * sizeof(cplx));
    int W = 0;
    be.d2h(&W, pl.wexp[pl.cur], sizeof(int));
    int rc = use_status ? pl.read_status() : be.sync();
    if (rc == -NFT_EC_OTHER) rc = NFT_EC_OTHER;  // raised by the scatterer itself
    if (rc != NFT_SUCCESS) return rc;
    *deg_ptr = pl.res_deg;
    if (W_ptr) {
        *W_ptr = W;
    } else {  // caller asked for un-normalised coefficients
        const double s = std::ldexp(1.0, W);
        for (size_t i = 0; i < cnt; i++) result[i] *= s;
    }
    return NFT_SUCCESS;
}

// what a host-pointer entry returns while its plan is still alive: a call that failed half-way waits for what it has
// enqueued, so that the plan's arena hands its blocks back from an idle stream
template <class BE> int api_return(BE &be, int rc)
{
    if (rc != NFT_SUCCESS) (void)be.sync();
    return rc;
}

// fnft__poly_fmult2x2, src/private/fnft__poly_fmult.c:381-546 (host buffers in and out)
template <class BE>
int api_poly_fmult2x2(BE &be, size_t *d, size_t n, std::complex<double> *p,
                      std::complex<double> *result, int32_t *W_ptr)
{
    if (!d || !p || !result || n == 0 || *d == 0) return NFT_EC_INVALID_ARGUMENT;
    const size_t deg = *d;
    if (deg > 0x7fffffff) return NFT_EC_INVALID_ARGUMENT;
    NftPlan<BE> pl(be, n, 0, 1, -1, (int)deg);
    int rc = pl.init();
    if (rc == NFT_SUCCESS) rc = pl.load_level0_from_host(p);
    if (rc == NFT_SUCCESS) rc = pl.run_tree();
    if (rc == NFT_SUCCESS) rc = api_export_result(pl, result, d, W_ptr, false);
    return api_return(be, rc);
}

// fnft__akns_fscatter, src/private/fnft__akns_fscatter.c:64-925 (r may be NULL: r = -kappa q*)
template <class BE>
int api_akns_fscatter(BE &be, size_t D, const std::complex<double> *q, const std::complex<double> *r,
                      double eps_t, int kappa, std::complex<double> *result, size_t *deg_ptr,
                      int32_t *W_ptr, int akns_disc)
{
    const int deg0 = nft_akns_degree(akns_disc);
    if (deg0 == 0) return NFT_EC_INVALID_ARGUMENT;
    NftPlan<BE> pl(be, D, 0, 1, akns_disc, deg0);
    int rc = pl.init();
    if (rc != NFT_SUCCESS) return api_return(be, rc);
    cplx *dq = nullptr, *dr = nullptr;
    if (!pl.mem.get(dq, D) || (r && !pl.mem.get(dr, D))) return api_return(be, NFT_EC_NOMEM);
    be.h2d(dq, q, D * sizeof(cplx));
    if (r) be.h2d(dr, r, D * sizeof(cplx));
    rc = pl.run_coeffs(dq, dr, eps_t, kappa);
    if (rc == NFT_SUCCESS) rc = pl.run_tree();
    if (rc == NFT_SUCCESS) rc = api_export_result(pl, result, deg_ptr, W_ptr, true);
    return api_return(be, rc);
}

// fnft__kdv_fscatter, src/private/fnft__kdv_fscatter.c:45-83: r = -1 for every sample; a real potential takes the
// real-coefficient tree (nft_real.h)
template <class BE>
int api_kdv_fscatter(BE &be, size_t D, const std::complex<double> *u, double eps_t, std::complex<double> *result,
                     size_t *deg_ptr, int32_t *W_ptr, int akns_disc)
{
    const int deg0 = nft_akns_degree(akns_disc);
    if (deg0 == 0) return NFT_EC_INVALID_ARGUMENT;
    bool real = true;
    for (size_t i = 0; i < D && real; i++) real = (u[i].imag() == 0.0);
    NftPlan<BE> pl(be, D, 0, 1, akns_disc, deg0);
    pl.kdv = true;
    pl.want_real = real;
    int rc = pl.init();
    if (rc != NFT_SUCCESS) return api_return(be, rc);
    cplx *dq = nullptr;
    if (!pl.mem.get(dq, D)) return api_return(be, NFT_EC_NOMEM);
    be.h2d(dq, u, D * sizeof(cplx));
    rc = pl.run_coeffs(dq, pl.rneg, eps_t, 1);
    if (rc == NFT_SUCCESS) rc = pl.run_tree();
    if (rc == NFT_SUCCESS) rc = api_export_result(pl, result, deg_ptr, W_ptr, true);
    return api_return(be, rc);
}
