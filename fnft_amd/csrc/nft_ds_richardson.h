// nft_ds_richardson.h -- Richardson extrapolation of the batched, device-resident discrete spectrum: the stage that
// follows a finished fine pass of NftDiscSpecBatch (the guess plan) or NftDiscSpecSearch (the guess-free plan, which ends
// in the same refinement).  Per signal it computes what NftDiscSpec::run does with o.richardson set (nft_discspec.h;
// reference: src/fnft_nsev.c:340-364, :376-392, :406-441):
//   coarse pass: a second NftDiscSpecBatch over every nskip-th sample (gathered; 4SPLIT4A/B: resampled from all D
//   samples), Newton from the fine bound states as guesses, the fine counts as live guesses, same niter and filter
//   -> KRichMatchDs: every fine bound state and its nearest coarse one, one Richardson step on the eigenvalue and, for
//   residues, on a' = norming constant / residue
// NORMING_CONSTANTS: the coarse pass computes none (the reference extrapolates eigenvalues and residues only).
// RESIDUES: both passes produce the BOTH layout -- the fine pass runs with fine_dstype() into fine_nc(), a buffer of the
// stage -- and the match kernel writes the caller's residues.
// Nothing is read back and nothing allocated in run(); init() allocates everything.  Back-end independent.
#pragma once
#include <memory>

#include "nft_discspec_batch.h"

template <class BE> class NftDsRichardson {
public:
    BE &be;
    DevArena<BE> mem;
    const size_t D, K, batch;
    const NftDsOpts o;                // the plan's options; a guess-free plan's coarse pass is a Newton pass all the same
    size_t Dsub = 0, nskip = 1;
    std::unique_ptr<NftDiscSpecBatch<BE>> coarse;
    cplx *bs_s = nullptr, *nc_s = nullptr;   // coarse bound states (batch*K), norming constants and residues (batch*2K)
    cplx *nc_f = nullptr;                    // RESIDUES: the fine pass's BOTH layout (batch*2K)
    unsigned long long *K_s = nullptr;

    NftDsRichardson(BE &be_, size_t D_, size_t K_, size_t batch_, const NftDsOpts &o_)
        : be(be_), mem(be_), D(D_), K(K_), batch(batch_), o(o_)
    {
        // NftDiscSpec::prepare with Dsub_wish = D/2
        Dsub = D / 2;
        if (Dsub < 2) Dsub = 2;
        if (Dsub > D) Dsub = D;
        nskip = (size_t)std::llround((double)D / (double)Dsub);
        Dsub = (size_t)std::llround((double)D / (double)nskip);
    }

    int init()
    {
        if (D < 3) return NFT_EC_INVALID_ARGUMENT;   // the stride rounds to 1: the combination would divide by zero
        NftDsOpts co = o;
        co.bsloc = 1;
        co.dstype = (o.dstype == 0) ? 0 : 2;
        coarse.reset(new NftDiscSpecBatch<BE>(be, Dsub, K, batch, co));
        coarse->set_front(D, nskip);
        const int rc = coarse->init();
        if (rc != NFT_SUCCESS) return rc;
        bool ok = mem.get(bs_s, batch * K) && mem.get(K_s, batch);
        if (ok && o.dstype != 0) ok = mem.get(nc_s, batch * 2 * K);
        if (ok && o.dstype == 1) ok = mem.get(nc_f, batch * 2 * K);
        return ok ? NFT_SUCCESS : NFT_EC_NOMEM;
    }

    size_t workspace_bytes() const { return mem.bytes + (coarse ? coarse->workspace_bytes() : 0); }

    // what the fine pass is run with in place of the caller's d_nc and the options' output type
    int fine_dstype() const { return (o.dstype == 1) ? 2 : o.dstype; }
    cplx *fine_nc(cplx *d_nc) const { return (d_nc && o.dstype == 1) ? nc_f : d_nc; }

    // after the fine pass (d_bs, fine_nc(d_nc), d_K; its status words d_status): enqueues the coarse pass and the match
    int run(const cplx *d_q, const double T[2], cplx *d_bs, cplx *d_nc, unsigned long long *d_K, int *d_status)
    {
        const bool res = d_nc && o.dstype != 0;
        const int rc = coarse->run(d_q, T, d_bs, bs_s, res ? nc_s : nullptr, K_s, d_K);
        if (rc != NFT_SUCCESS) return rc;
        const double eps_t = (T[1] - T[0]) / (double)(D - 1);
        const double Ts1 = T[0] + (double)((Dsub - 1) * nskip) * eps_t;
        const double eps_s = (Ts1 - T[0]) / (double)(Dsub - 1);
        RichDsParams R;
        std::memset(&R, 0, sizeof(R));
        R.bs = d_bs; R.bs_s = bs_s;
        R.K_out = d_K; R.Ks_out = K_s;
        if (res) {
            R.nc = fine_nc(d_nc);
            R.nc_s = nc_s;
            R.res = d_nc;
            R.res_stride = (long long)((o.dstype == 2) ? 2 * K : K);
            R.res_off = (long long)((o.dstype == 2) ? K : 0);
        }
        R.K = (int)K;
        R.thr = eps_t;
        R.sn = std::pow(eps_s / eps_t, (double)nft_nse_method_order(o.nse_disc));
        R.sd = R.sn - 1.0;
        R.status = d_status;
        R.status_s = coarse->status;
        be.template run<KRichMatchDs>((int)batch, 1, R);
        return NFT_SUCCESS;
    }

    // a guess plan's call with the stage: the fine pass, then run()
    int run_after(NftDiscSpecBatch<BE> &fine, const cplx *d_q, const double T[2], const cplx *d_guess, cplx *d_bs,
                  cplx *d_nc, unsigned long long *d_K)
    {
        const int rc = fine.run(d_q, T, d_guess, d_bs, fine_nc(d_nc), d_K, nullptr, fine_dstype());
        if (rc != NFT_SUCCESS) return rc;
        return run(d_q, T, d_bs, d_nc, d_K, fine.status);
    }
};
