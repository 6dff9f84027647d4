// nft_discspec_search.h -- batched, device-resident discrete spectrum of fnft_nsev WITHOUT guesses (FAST_EIGENVALUE and
// SUBSAMPLE_AND_REFINE localization, kappa = +1): `batch` signals of D samples, room for K bound states each, every
// array on the device, nothing read back between the stages.  Per signal it computes what NftDiscSpec::run() computes
// (nft_discspec.h; reference: src/fnft_nsev.c:276-309, :683-706):
//   gather / resampling front end -> product tree (one batched NftPlan) -> start values -> fixed schedule of
//   Ehrlich-Aberth sweeps + two polish sweeps -> z -> lambda, box test, merge, truncation to K (candidates)
//   -> NftDiscSpecBatch with the candidates as guesses: box, Newton (SUBSAMPLE_AND_REFINE only), filter, norming
// The host cannot know when a signal's iteration has converged, so it always enqueues kAbSweeps sweeps; the device
// keeps every signal's state (AbState) and the workgroups of a finished signal return at once (nft_kernels.h:
// body_aberthb_*).  Back-end independent like NftDiscSpecBatch: hip_backend.hip instantiates it with the HIP back
// end, tests/emu with the lane emulator.
#pragma once
#include "nft_discspec_batch.h"

template <class BE> class NftDiscSpecSearch {
public:
    BE &be;
    DevArena<BE> mem;
    const size_t D, K, batch;
    const NftDsOpts o;                // bsloc 0 (FAST_EIGENVALUE) or 2 (SUBSAMPLE_AND_REFINE)
    int ups = 1, deg0 = 0, akns = -1;
    size_t Dsub = 0, nskip = 1;       // subsampled length actually used and its stride (D and 1 for FAST_EIGENVALUE)
    size_t n = 0;                     // roots per signal
    int S = 1, gxn = 1;
    std::unique_ptr<NftPlan<BE>> tree;
    std::unique_ptr<NftDiscSpecBatch<BE>> refine;
    cplx *qsub = nullptr;             // batch*Dsub gathered samples (ups == 1, nskip > 1)
    AberthBatchParams A;
    double *sbox = nullptr;           // batch*4: box of the signal the roots belong to
    int *sstatus = nullptr, *warn = nullptr;
    static constexpr size_t kMaxRoots = 16384;

    // Dsub as NftDiscSpec::run / prepare form it; *roots = 0: sizes no plan can have
    static void sizes(size_t D, const NftDsOpts &o, size_t *Dsub_out, size_t *nskip_out, size_t *roots)
    {
        *Dsub_out = 0; *nskip_out = 1; *roots = 0;
        const int akns = nft_nse_to_akns(o.nse_disc);
        if (akns < 0 || D < 2 || (o.bsloc != 0 && o.bsloc != 2)) return;
        size_t Dsub = D, nskip = 1;
        if (o.bsloc == 2) {
            Dsub = o.Dsub;
            if (Dsub == 0) Dsub = (size_t)std::sqrt((double)D * std::log2((double)D) * std::log2((double)D));
            const NftSubGrid g = nft_sub_grid(D, Dsub);
            Dsub = g.Dsub; nskip = g.nskip;
        }
        *Dsub_out = Dsub;
        *nskip_out = nskip;
        *roots = Dsub * (size_t)nft_nse_upsampling(o.nse_disc) * (size_t)nft_akns_degree(akns);
    }

    NftDiscSpecSearch(BE &be_, size_t D_, size_t K_, size_t batch_, const NftDsOpts &o_)
        : be(be_), mem(be_), D(D_), K(K_), batch(batch_), o(o_)
    {
        akns = nft_nse_to_akns(o.nse_disc);
        ups = nft_nse_upsampling(o.nse_disc);
        deg0 = akns >= 0 ? nft_akns_degree(akns) : 0;
        sizes(D, o, &Dsub, &nskip, &n);
        std::memset(&A, 0, sizeof(A));
    }

    int init()
    {
        if (n == 0 || K == 0 || batch == 0) return NFT_EC_INVALID_ARGUMENT;
        if (n > kMaxRoots || batch > (size_t)0x7fffffff / ((n + 255) / 256)) return NFT_EC_NOT_YET_IMPLEMENTED;
        if (ups == 2 && Dsub < 2) return NFT_EC_INVALID_ARGUMENT;
        NftDsOpts ro = o;
        ro.bsloc = 1;
        if (o.bsloc == 0) ro.niter = 0;   // FAST_EIGENVALUE: filter and norming constants only
        refine.reset(new NftDiscSpecBatch<BE>(be, D, K, batch, ro));
        int rc = refine->init();
        if (rc != NFT_SUCCESS) return rc;
        tree.reset(new NftPlan<BE>(be, Dsub * (size_t)ups, 0, batch, akns, deg0));
        if (ups == 2) tree->set_front(D, nskip, ups);
        rc = tree->init();
        if (rc != NFT_SUCCESS) return rc;
        // segments of the two O(n^2) kernels: the chip filled by the whole batch, the same for every sweep and for every
        // signal (one whose degree drops below 128 through zero end coefficients runs unsegmented, aberthb_params)
        gxn = (int)((n + 255) / 256);
        size_t s = (BE::kTargetWorkgroups + (size_t)gxn * batch - 1) / ((size_t)gxn * batch);
        if (s > (size_t)kAbSegCap) s = (size_t)kAbSegCap;
        if (n < 128 || s < 1) s = 1;
        S = (int)s;
        const size_t bn = batch * n;
        bool ok = mem.get(A.zbuf[0], bn) && mem.get(A.zbuf[1], bn) && mem.get(A.ibuf[0], bn) && mem.get(A.ibuf[1], bn)
                  && mem.get(A.hit, bn) && mem.get(A.pp, s * bn) && mem.get(A.pd, s * bn) && mem.get(A.ps, s * bn)
                  && mem.get(A.pe, s * bn) && mem.get(A.state, batch) && mem.get(sbox, batch * 4)
                  && mem.get(sstatus, batch) && mem.get(warn, batch) && mem.get(A.cand, batch * K)
                  && mem.get(A.ncand, batch);
        if (ok && n + 1 > (size_t)kAbStartLds) ok = mem.get(A.la, batch * (n + 1)) && mem.get(A.hull, batch * (n + 1));
        if (ok && ups == 1 && nskip > 1) ok = mem.get(qsub, batch * Dsub);
        if (!ok) return NFT_EC_NOMEM;
        A.n = (long long)n;
        A.tm_stride = (long long)(4 * (n + 1));
        A.batch = (long long)batch;
        A.gxn = gxn;
        A.S = S;
        A.status = sstatus;
        A.warn = warn;
        A.box = sbox;
        A.bsfilt = o.bsfilt;
        A.K = (int)K;
        return NFT_SUCCESS;
    }

    void destroy() { tree.reset(); refine.reset(); mem.clear(); }

    size_t workspace_bytes() const
    {
        return mem.bytes + (tree ? tree->mem.bytes : 0) + (refine ? refine->workspace_bytes() : 0);
    }

    // enqueues everything; waits for nothing.  d_nc may be NULL; dstype: the layout of d_nc in place of the options'
    // (NftDiscSpecBatch::run), -1: the options'
    int run(const cplx *d_q, const double T[2], cplx *d_bs, cplx *d_nc, unsigned long long *d_K, int dstype = -1)
    {
        // grid of the subsampled signal, NftDiscSpec::prepare
        double Ts1, eps_s;
        nft_sub_interval(T, D, Dsub, nskip, &Ts1, &eps_s);
        be.memset0(sstatus, batch * sizeof(int));
        be.memset0(warn, batch * sizeof(int));
        const cplx *qs = d_q;     // preprocessed samples of the signal the roots belong to
        double Tsub[2];
        int rc;
        if (ups == 1) {
            if (nskip > 1) {
                GatherParams G;
                G.q = d_q; G.out = qsub;
                G.D = (long long)D; G.Dsub = (long long)Dsub; G.nskip = (long long)nskip; G.batch = (long long)batch;
                be.template run<KDsGather>((int)((batch * Dsub + 255) / 256), 1, G);
                qs = qsub;
            }
            const double Tf[2] = {T[0], Ts1};
            rc = tree->run_front(qs, Tf, +1, Tsub);
        } else {
            rc = tree->run_front(d_q, T, +1, Tsub);   // resampling with nskip, then level 0
            qs = tree->qpre;
        }
        if (rc == NFT_SUCCESS) rc = tree->run_tree();
        if (rc != NFT_SUCCESS) return rc;
        tree->export_tm();
        {   // box of that signal and its MODAL step-size check (fnft__akns_fscatter.c:122-126), as body_ds_box forms them
            DsBatchParams P;
            std::memset(&P, 0, sizeof(P));
            P.q = qs;
            P.D = (long long)(Dsub * (size_t)ups);
            P.ups = ups;
            P.T0 = T[0]; P.T1 = Ts1; P.eps = eps_s;
            P.batch = (long long)batch;
            P.box = sbox;
            P.re_bound = 0.9 * 3.14159265358979323846 / std::fabs(2.0 / (double)deg0 * eps_s);
            P.bsfilt = o.bsfilt;
            P.niter = 0;              // the drop-in tests this box for emptiness only before a Newton refinement
            P.modal = (o.nse_disc == 0) ? 1 : 0;
            P.status = sstatus;
            be.template run<KDsBox>((int)batch, 1, P);
        }
        A.den = 2.0 * eps_s / (double)(deg0 * ups);
        roots(tree->tm_out);
        be.template run<KDsCandidates>((int)batch, 1, A);
        return refine->run(d_q, T, A.cand, d_bs, d_nc, d_K, A.ncand, dstype);
    }

    // all roots of entry 11 of every signal's transfer matrix (tm: batch * 4 * (n + 1) coefficients): start values, the
    // fixed schedule of sweeps, the polish sweeps.  Signal b's roots end in zbuf[state[b].zin] + b*n
    void roots(const cplx *tm)
    {
        A.tm = tm;
        const int gx = (int)(batch * (size_t)gxn);
        be.template run<KAberthBStart>((int)batch, 1, A);
        for (int it = 0; it < kAbSweeps; it++) {
            be.template run<KAberthBNewton>(gx, S, A);
            be.template run<KAberthBSum>(gx, S, A);
            be.template run<KAberthBApply>(gx, 1, A);
            A.stage = (it == kAbSweeps - 1) ? 1 : 0;
            be.template run<KAberthBStep>((int)batch, 1, A);
        }
        for (int it = 0; it < 2; it++) {   // polish, NftDiscSpec::roots
            be.template run<KAberthBNewton>(gx, S, A);
            be.template run<KAberthBApply>(gx, 1, A);
            if (it == 0) {
                A.stage = 2;
                be.template run<KAberthBStep>((int)batch, 1, A);
            }
        }
    }

    // waits for the stream; st: the status words (NftDiscSpecBatch's bits, bit 3: root finder failed), kout: the counts,
    // wn: the warning bits
    int read(std::vector<int> &st, std::vector<unsigned long long> &kout, std::vector<int> &wn,
             const unsigned long long *d_K)
    {
        std::vector<int> s2(batch, 0);
        wn.assign(batch, 0);
        be.d2h(s2.data(), sstatus, batch * sizeof(int));
        be.d2h(wn.data(), warn, batch * sizeof(int));
        const int rc = refine->read(st, kout, d_K);
        for (size_t b = 0; b < batch; b++) st[b] |= s2[b];
        return rc;
    }
};
