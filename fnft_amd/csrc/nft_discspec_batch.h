// nft_discspec_batch.h -- batched, device-resident discrete spectrum of fnft_nsev (NEWTON localization, kappa = +1):
// `batch` signals of D samples with K eigenvalue guesses each, every array on the device, nothing read back between
// the stages.  Per signal it computes what NftDiscSpec::base() with bsloc == 1 computes (nft_discspec.h; reference:
// src/fnft_nsev.c:971-1038 Newton refinement, misc_filter / misc_merge, :895-968 norming constants / residues), with
// one workgroup per (signal, eigenvalue) instead of a host loop over chunk kernels (nft_kernels.h: body_ds_*).
//   box kernel -> Newton kernel (all iterations on chip) -> filter + merge kernel -> norming kernel
// 4SPLIT4A/B refine on the resampled signal of that scheme's front end (NftResampler::run_4split4, qpre).
// set_front(Din, nskip): the D samples are every nskip-th of Din input samples (the coarse pass of the Richardson
// extrapolation, nft_discspec_plan.h) -- gathered (KDsGather) or, for 4SPLIT4A/B, resampled from all Din samples.
// Back-end independent like NftDiscSpec: hip_backend.hip instantiates it with the HIP back end, tests/emu with the
// lane emulator.
#pragma once
#include "nft_discspec.h"

template <class BE> class NftDiscSpecBatch {
public:
    BE &be;
    DevArena<BE> mem;                 // owns lam, box, status, phi and the front end's tables and arrays
    const size_t D, K, batch;
    const NftDsOpts o;
    int ups = 1, deg0 = 0, akns = -1;
    size_t Dq = 0;                    // preprocessed samples per signal
    size_t Din = 0, nskip = 1;        // set_front: input samples per signal (0: D) and their stride
    int G = 1;                        // samples per lane
    NftTwiddles<BE> tw;
    NftResampler<BE> rs;              // 4SPLIT4A/B: the front end's shifted copies, combined into qpre (batch * Dq)
    cplx *qpre = nullptr;             // also the gathered samples of a strided front with upsampling factor 1
    cplx *lam = nullptr;              // batch*K refined eigenvalues
    double *box = nullptr;            // batch*4
    int *status = nullptr;            // batch
    cplx *phi = nullptr;              // slab * K * sphi
    size_t slab = 0, sphi = 0;        // signals per launch of the norming kernel; phi values per (signal, eigenvalue)
    static constexpr size_t kMaxK = 65535;                      // the merge is one lane's O(K^2) loop per signal
    static constexpr size_t kMaxGroups = 0x7fffffff;            // batch*K workgroups on grid.x
    static constexpr size_t kPhiBytes = (size_t)256 << 20;      // phi workspace of one norming launch

    NftDiscSpecBatch(BE &be_, size_t D_, size_t K_, size_t batch_, const NftDsOpts &o_)
        : be(be_), mem(be_), D(D_), K(K_), batch(batch_), o(o_), rs(be_, tw)
    {
        akns = nft_nse_to_akns(o.nse_disc);
        ups = nft_nse_upsampling(o.nse_disc);
        deg0 = akns >= 0 ? nft_akns_degree(akns) : 0;
        Dq = D * (size_t)ups;
        size_t g = (Dq + kDsLanes - 1) / kDsLanes;
        g = (g + (size_t)ups - 1) / (size_t)ups * (size_t)ups;
        G = (int)g;
        sphi = ((size_t)G / (size_t)ups + 1) * (size_t)kDsLanes * 2;
    }

    // call before init(): this plan's D = nft_sub_count(Din_, nskip_) samples are every nskip_-th of Din_
    void set_front(size_t Din_, size_t nskip_) { Din = Din_; nskip = nskip_; }

    int init()
    {
        if (akns < 0 || deg0 == 0 || D < 2 || K == 0 || batch == 0) return NFT_EC_INVALID_ARGUMENT;
        if (Din == 0) { Din = D; nskip = 1; }
        if (nskip < 1 || D != nft_sub_count(Din, nskip) || (D - 1) * nskip >= Din) return NFT_EC_INVALID_ARGUMENT;
        if (K > kMaxK || batch > kMaxGroups / K || Dq > (size_t)0x7fffffff * (size_t)kDsLanes)
            return NFT_EC_NOT_YET_IMPLEMENTED;
        if (ups == 2) {
            if (Din <= 2) return NFT_EC_INVALID_ARGUMENT;
            if (nft_tree_too_large(Dq, deg0)) return NFT_EC_NOT_YET_IMPLEMENTED;   // the limit of the scheme's tree plan, kept
            const int rc = rs.init(mem, Din, batch);
            if (rc != NFT_SUCCESS) return rc;
            // the tables last: their upload waits for the cleared status word
            if (!(mem.get(qpre, batch * Dq) && tw.init(mem))) return NFT_EC_NOMEM;
        } else if (nskip > 1) {
            if (!mem.get(qpre, batch * D)) return NFT_EC_NOMEM;
        }
        const size_t per_signal = K * sphi * sizeof(cplx);
        slab = kPhiBytes / per_signal;
        if (slab < 1) slab = 1;
        if (slab > batch) slab = batch;
        const bool ok = mem.get(lam, batch * K) && mem.get(box, batch * 4) && mem.get(status, batch)
                        && mem.get(phi, slab * K * sphi);
        return ok ? NFT_SUCCESS : NFT_EC_NOMEM;
    }

    // the workspace back before the plan goes out of scope (the destructor does the same); init() again before reuse
    void destroy() { mem.clear(); }

    size_t workspace_bytes() const { return mem.bytes; }

    // enqueues everything; waits for nothing.  d_q, T: the Din input samples per signal and their interval.  d_nc may be
    // NULL (no norming constants / residues); d_nguess: live guesses per signal (the guess-free plan's candidates,
    // nft_discspec_search.h; the fine counts of the Richardson stage), NULL: K each; dstype: the output layout of d_nc in
    // place of the options' (the Richardson stage needs BOTH where the caller asked for residues), -1: the options'
    int run(const cplx *d_q, const double T[2], const cplx *d_guess, cplx *d_bs, cplx *d_nc,
            unsigned long long *d_K, const unsigned long long *d_nguess = nullptr, int dstype = -1)
    {
        // grid and step as NftDiscSpec::prepare forms them (without set_front the full signal: Dsub = D, nskip = 1)
        double T1, eps_t;
        nft_sub_interval(T, Din, D, nskip, &T1, &eps_t);
        be.memset0(status, batch * sizeof(int));
        if (ups == 2) {
            const int rc = rs.run_4split4(d_q, nskip, D, qpre, rs.ft.status);   // the band check's bit: read by nobody
            if (rc != NFT_SUCCESS) return rc;
        } else if (nskip > 1) {
            GatherParams Gp;
            Gp.q = d_q; Gp.out = qpre;
            Gp.D = (long long)Din; Gp.Dsub = (long long)D; Gp.nskip = (long long)nskip; Gp.batch = (long long)batch;
            be.template run<KDsGather>((int)((batch * D + 255) / 256), 1, Gp);
        }
        DsBatchParams P;
        std::memset(&P, 0, sizeof(P));
        P.q = (ups == 2 || nskip > 1) ? qpre : d_q;
        P.D = (long long)Dq;
        P.ups = ups;
        P.G = G;
        P.lscale = (ups == 2) ? 0.5 : 1.0;
        P.T0 = T[0]; P.T1 = T1; P.eps = eps_t;
        P.K = (int)K;
        P.batch = (long long)batch;
        P.guess = d_guess;
        P.nguess = d_nguess;
        P.lam = lam;
        P.src = (o.niter > 0) ? lam : d_guess;
        P.box = box;
        P.re_bound = 0.9 * 3.14159265358979323846 / std::fabs(2.0 / (double)deg0 * eps_t);
        P.bsfilt = o.bsfilt;
        P.niter = (int)std::min<size_t>(o.niter, 0x7fffffff);
        P.dstype = (dstype >= 0) ? dstype : o.dstype;
        P.modal = (o.nse_disc == 0) ? 1 : 0;
        P.status = status;
        P.bs = d_bs;
        P.nc = d_nc;
        P.K_out = d_K;
        P.phi = phi;
        P.sphi = (long long)sphi;
        const bool ldsq = Dq <= (size_t)kDsLdsSamples;
        be.template run<KDsBox>((int)batch, 1, P);
        if (o.niter > 0) {
            if (ldsq) be.template run<KDsNewton<true>>((int)(batch * K), 1, P);
            else be.template run<KDsNewton<false>>((int)(batch * K), 1, P);
        }
        be.template run<KDsFilter>((int)((batch + 255) / 256), 1, P);
        if (d_nc) {
            for (size_t b0 = 0; b0 < batch; b0 += slab) {
                const size_t nb = std::min(slab, batch - b0);
                P.b0 = (long long)b0;
                if (ldsq) be.template run<KDsNorm<true>>((int)(nb * K), 1, P);
                else be.template run<KDsNorm<false>>((int)(nb * K), 1, P);
            }
        }
        return NFT_SUCCESS;
    }

    // waits for the stream; st: the status words, kout: the counts (d_K of the last call)
    int read(std::vector<int> &st, std::vector<unsigned long long> &kout, const unsigned long long *d_K)
    {
        st.assign(batch, 0);
        kout.assign(batch, 0);
        be.d2h(st.data(), status, batch * sizeof(int));
        if (d_K) be.d2h(kout.data(), d_K, batch * sizeof(unsigned long long));
        return be.sync();
    }
};
