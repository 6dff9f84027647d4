// nft_discspec_plan.h -- the core of fnft_amd_discspec_plan.  NftDiscSpecPlan owns the fine pass -- NftDiscSpecBatch
// (o.bsloc == 1: the caller's guesses) or NftDiscSpecSearch (0, 2: guess-free; it ends in the same refinement) -- and the
// optional Richardson stage, and its run() is the only place that orders a call: fine pass, then stage.
// NftDsRichardson is the stage.  Per signal it computes what NftDiscSpec::run does with o.richardson set (nft_discspec.h;
// reference: src/fnft_nsev.c:340-364, :376-392, :406-441):
//   coarse pass: a second NftDiscSpecBatch over every nskip-th sample (gathered; 4SPLIT4A/B: resampled from all D
//   samples), Newton from the fine bound states as guesses, the fine counts as live guesses, same niter and filter
//   -> KRichMatchDs: every fine bound state and its nearest coarse one, one Richardson step on the eigenvalue and, for
//   residues, on a' = norming constant / residue
// NORMING_CONSTANTS: the coarse pass computes none (the reference extrapolates eigenvalues and residues only).
// RESIDUES: both passes produce the BOTH layout -- the fine pass runs with fine_dstype() into fine_nc(), a buffer of the
// stage -- and the match kernel writes the caller's residues.
// Nothing is read back and nothing allocated in run().  Back-end independent: the HIP back end or the lane emulator.
#pragma once
#include "nft_discspec_search.h"

template <class BE> class NftDsRichardson {
public:
    BE &be;
    DevArena<BE> mem;
    const size_t D, K, batch;
    const NftDsOpts o;                // the plan's options; a guess-free plan's coarse pass is a Newton pass all the same
    const NftSubGrid g;               // NftDiscSpec::prepare with Dsub_wish = D/2
    std::unique_ptr<NftDiscSpecBatch<BE>> coarse;
    cplx *bs_s = nullptr, *nc_s = nullptr;   // coarse bound states (batch*K), norming constants and residues (batch*2K)
    cplx *nc_f = nullptr;                    // RESIDUES: the fine pass's BOTH layout (batch*2K)
    unsigned long long *K_s = nullptr;

    NftDsRichardson(BE &be_, size_t D_, size_t K_, size_t batch_, const NftDsOpts &o_)
        : be(be_), mem(be_), D(D_), K(K_), batch(batch_), o(o_), g(nft_sub_grid(D_, D_ / 2)) {}

    int init()
    {
        if (D < 3) return NFT_EC_INVALID_ARGUMENT;   // the stride rounds to 1: the combination would divide by zero
        NftDsOpts co = o;
        co.bsloc = 1;
        co.dstype = (o.dstype == 0) ? 0 : 2;
        coarse.reset(new NftDiscSpecBatch<BE>(be, g.Dsub, K, batch, co));
        coarse->set_front(D, g.nskip);
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
        double Ts1, eps_s;
        nft_sub_interval(T, D, g.Dsub, g.nskip, &Ts1, &eps_s);
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
};

template <class BE> class NftDiscSpecPlan {
public:
    BE &be;
    const size_t D, K, batch;
    const NftDsOpts o;
    std::unique_ptr<NftDiscSpecBatch<BE>> guess;     // at most one of the two: the fine pass
    std::unique_ptr<NftDiscSpecSearch<BE>> search;
    std::unique_ptr<NftDsRichardson<BE>> rich;       // after the fine pass: its coarse pass reads the fine one's outputs
    bool rich_on = false;

    // sizes things and nothing else: no device call, no device memory
    NftDiscSpecPlan(BE &be_, size_t D_, size_t K_, size_t batch_, const NftDsOpts &o_)
        : be(be_), D(D_), K(K_), batch(batch_), o(o_),
          guess(o_.bsloc == 1 ? new NftDiscSpecBatch<BE>(be_, D_, K_, batch_, o_) : nullptr),
          search(o_.bsloc == 1 ? nullptr : new NftDiscSpecSearch<BE>(be_, D_, K_, batch_, o_)) {}

    bool guess_free() const { return !guess; }
    int init() { return guess ? guess->init() : search->init(); }

    size_t workspace_bytes() const
    {
        return (guess ? guess->workspace_bytes() : search->workspace_bytes()) + (rich ? rich->workspace_bytes() : 0);
    }

    // As NftPlan::enable_richardson: the caller has waited for the plan's stream; the first call allocates the coarse pass,
    // a failing one leaves no block behind and the plan as it was; rich_on = false switches off and keeps the workspace
    bool rich_ready() const { return (bool)rich; }
    int enable_richardson()
    {
        if (rich) { rich_on = true; return NFT_SUCCESS; }
        std::unique_ptr<NftDsRichardson<BE>> r(new (std::nothrow) NftDsRichardson<BE>(be, D, K, batch, o));
        if (!r) return NFT_EC_NOMEM;
        const int rc = r->init();
        if (rc == NFT_SUCCESS) { rich = std::move(r); rich_on = true; }
        else (void)be.sync();   // what init enqueued, before the stage's blocks go back
        return rc;
    }

    // the fine pass's status words: what read() reports and the stage ORs the coarse bits into
    int *fine_status() const { return guess ? guess->status : search->refine->status; }

    // enqueues everything; waits for nothing.  d_guess: K guesses per signal, NULL on a guess-free plan; d_nc may be NULL
    int run(const cplx *d_q, const double T[2], const cplx *d_guess, cplx *d_bs, cplx *d_nc, unsigned long long *d_K)
    {
        cplx *const nc = rich_on ? rich->fine_nc(d_nc) : d_nc;
        const int dstype = rich_on ? rich->fine_dstype() : -1;
        const int rc = guess ? guess->run(d_q, T, d_guess, d_bs, nc, d_K, nullptr, dstype)
                             : search->run(d_q, T, d_bs, nc, d_K, dstype);
        if (rc != NFT_SUCCESS || !rich_on) return rc;
        return rich->run(d_q, T, d_bs, d_nc, d_K, fine_status());
    }

    // waits for the stream; st: the status words, kout: the counts (d_K of the last call), wn: the guess-free plan's
    // warning bits, all zero on a guess plan
    int read(std::vector<int> &st, std::vector<unsigned long long> &kout, std::vector<int> &wn,
             const unsigned long long *d_K)
    {
        if (search) return search->read(st, kout, wn, d_K);
        wn.assign(batch, 0);
        return guess->read(st, kout, d_K);
    }
};
