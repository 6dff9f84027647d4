// nft_nsev_inverse.h -- device side of fnft_nsev_inverse (src/fnft_nsev_inverse.c:121-1033) and of
// fnft__poly_specfact (src/private/fnft__poly_specfact.c:25-140).  The host keeps the reference's control flow;
// what runs on the GPU: every DFT (chirp kernels in DFT mode: any length, so the reference's 2-3-5-smooth lengths are
// kept), every element-wise stage with transcendentals (body_inv_op), the layer peeling's polynomial products
// (fnft__nse_finvscatter), the multi-soliton recursion, the eigenfunctions of the seed potential (the chunk-parallel
// scatterer of the discrete spectrum on the half-step signal) and the Darboux steps.
#pragma once
#include <algorithm>
#include <complex>
#include <cstring>
#include <map>
#include <memory>
#include <new>
#include <vector>

#include "nft_plan.h"
#include "nft_discspec.h"

// kiss_fft_next_fast_size (fft_wrapper_next_fft_length): smallest m >= n with only the factors 2, 3, 5
inline size_t nft_next_fast_size(size_t n)
{
    for (;; n++) {
        size_t m = n;
        while (m % 2 == 0) m /= 2;
        while (m % 3 == 0) m /= 3;
        while (m % 5 == 0) m /= 5;
        if (m <= 1) return n;
    }
}

// Layer peeling with every array on the device (src/private/fnft__nse_finvscatter.c:66-232): the recursion of
// (steps 1-4 below) issued from the host without a single synchronisation -- blocks of up to kLeaf samples by the
// one-wave leaf kernel (body_peel_leaf), the 2x2 polynomial products above that by resident plans (one per degree,
// n = 2 matrices: the tree's general pair kernels), factors and results moved between the caller's strided arrays
// and the plans' layout by two small kernels.  Work arrays: one set per recursion depth (depth-first order on one
// stream, so siblings reuse them).
// batch > 1: that many independent signals peeled together -- every launch covers the whole batch (grid.y = signal for
// the leaf and the one-launch products, plans created with `batch` signals of two matrices each), every array holds the
// signals at a fixed distance (the *b arguments), and the status word is one int per signal.
template <class BE> class NftLayerPeelingDev {
public:
    static constexpr size_t kLeaf = 256;
    static constexpr size_t kOneLaunchMaxDeg = 1024;   // products up to this degree: KPeelProduct
    BE &be;
    DevArena<BE> mem;            // owns the status words, the work arrays and, unless borrowed, the twiddle tables
    NftTwiddles<BE> own_tw;      // allocated with the first product above the leaf
    const NftTwiddles<BE> &tw;   // the one table set of the peeler and of its per-degree trees
    double eps_t;
    int kappa, modal;
    size_t batch = 1;
    int rc = NFT_SUCCESS;
    int *d_status = nullptr;     // max(4, batch) ints: signal s's status at d_status[s]
    std::map<size_t, std::unique_ptr<NftPlan<BE>>> plans;
    struct Work { cplx *T2i = nullptr, *T1 = nullptr, *T1i = nullptr; };
    std::vector<Work> work;

    // borrowed: the tables of the class the peeler is a part of, initialised before prepare() / peel()
    NftLayerPeelingDev(BE &b, double eps, int kap, int is_modal, const NftTwiddles<BE> *borrowed = nullptr)
        : be(b), mem(b), tw(borrowed ? *borrowed : own_tw), eps_t(eps), kappa(kap), modal(is_modal) {}
    size_t status_words() const { return std::max<size_t>(4, batch); }
    // everything back, the object stays usable: the resident peeler of the host-pointer entries is emptied and reused
    void destroy()
    {
        plans.clear();
        work.clear();
        work_deg = 0;
        mem.clear();
        own_tw = NftTwiddles<BE>();
        d_status = nullptr;
    }
    size_t workspace_bytes() const
    {
        size_t b = mem.bytes;
        for (const auto &kv : plans) b += kv.second->mem.bytes;
        return b;
    }
    // status word, work arrays for a transfer matrix of degree deg (kept and reused by later calls of the same or a
    // smaller size: depth 0 is always the largest)
    size_t work_deg = 0;
    int init(size_t deg)
    {
        rc = NFT_SUCCESS;
        if (!d_status && !mem.get(d_status, status_words())) return NFT_EC_NOMEM;
        be.memset0(d_status, status_words() * sizeof(int));
        if (deg > work_deg) {
            for (auto &w : work) { mem.give_back(w.T2i); mem.give_back(w.T1); mem.give_back(w.T1i); }
            work.clear();
            work_deg = 0;
            for (size_t d = deg; d > kLeaf; d /= 2) {
                Work w;
                const bool ok = mem.get(w.T2i, batch * 4 * (d + 1)) && mem.get(w.T1, batch * 4 * (2 * d + 1))
                                && mem.get(w.T1i, batch * 4 * (d / 2 + 1));
                work.push_back(w);   // an incomplete set too: the next call gives it back
                if (!ok) return NFT_EC_NOMEM;
                // the upper half of T2i (coefficients 0 .. d/2 - 1 of every entry) is never written: zero once
                be.memset0(w.T2i, batch * 4 * (d + 1) * sizeof(cplx));
            }
            work_deg = deg;
        }
        return NFT_SUCCESS;
    }
    bool tables()
    {
        if (tw.ready() || (&tw == &own_tw && own_tw.init(mem))) return true;
        rc = NFT_EC_NOMEM;
        return false;
    }
    NftPlan<BE> *plan_for(size_t deg)
    {
        auto it = plans.find(deg);
        if (it != plans.end()) return it->second.get();
        if (!tables()) return nullptr;
        std::unique_ptr<NftPlan<BE>> pl(new (std::nothrow) NftPlan<BE>(be, 2, 0, batch, -1, (int)deg, &tw));
        if (!pl) { rc = NFT_EC_NOMEM; return nullptr; }
        const int r = pl->init();
        if (r != NFT_SUCCESS) { rc = r; return nullptr; }
        return (plans[deg] = std::move(pl)).get();
    }
    // every plan and work array a peeling of degree deg will use (the batched call allocates nothing while it runs)
    int prepare(size_t deg)
    {
        const int r = init(deg);
        if (r != NFT_SUCCESS) return r;
        if (deg > kLeaf && !tables()) return rc;
        for (size_t d = deg; d > kLeaf; d /= 2)
            if (d != 256 && d != 512 && d != kOneLaunchMaxDeg && !plan_for(d)) return rc;
        return NFT_SUCCESS;
    }
    // C (four entries of 2 deg + 1 coefficients at stride Cs) = A * B (four entries of deg + 1 at strides As, Bs);
    // Ab, Bb, Cb: distances between the signals of the batch
    void prod(size_t deg, const cplx *A, size_t As, size_t Ab, const cplx *B, size_t Bs, size_t Bb, cplx *C, size_t Cs,
              size_t Cb)
    {
        if (rc != NFT_SUCCESS) return;
        if (deg == 256 || deg == 512 || deg == kOneLaunchMaxDeg) {   // one launch, entries transformed concurrently
            if (!tables()) return;
            PeelProdParams Q;
            std::memset(&Q, 0, sizeof(Q));
            Q.A = A; Q.B = B; Q.As = (long long)As; Q.Bs = (long long)Bs; Q.C = C; Q.Cs = (long long)Cs;
            Q.tw = tw.tw_table(2 * deg);
            Q.Ab = (long long)Ab; Q.Bb = (long long)Bb; Q.Cb = (long long)Cb;
            const int gy = (int)batch;
            if (deg == 256) be.template run<KPeelProduct<512>>(1, gy, Q);
            else if (deg == 512) be.template run<KPeelProduct<1024>>(1, gy, Q);
            else be.template run<KPeelProduct<2048>>(1, gy, Q);
            return;
        }
        NftPlan<BE> *pl = plan_for(deg);
        if (!pl) return;
        PeelIoParams P;
        std::memset(&P, 0, sizeof(P));
        P.A = A; P.B = B; P.As = (long long)As; P.Bs = (long long)Bs; P.d = (long long)deg;
        P.body = pl->body[0]; P.tail = pl->tail[0]; P.scale = pl->scale[0]; P.wexp = pl->wexp[0];
        P.batch = (long long)batch; P.Ab = (long long)Ab; P.Bb = (long long)Bb; P.n0 = (long long)pl->n0;
        be.template run<KPeelImport>((int)((batch * 8 * (deg + 1) + 255) / 256), 1, P);
        pl->cur = 0;
        pl->ne = 4;
        pl->start_n = pl->n0;
        pl->start_d = deg;
        const int r = pl->run_tree();
        if (r != NFT_SUCCESS) { rc = r; return; }
        pl->export_tm(C, Cs, true, Cb); // result layout, un-normalised, straight into the caller's strided array
    }
    // T: four entries of deg+1 coefficients at stride Ts; Ti (may be NULL): the inverse up to a power of z, four
    // entries of deg+1 at stride Tis; q: deg samples.  All device pointers; Tb, Tib, qb: distances between the signals
    void peel(size_t deg, const cplx *T, size_t Ts, size_t Tb, cplx *Ti, size_t Tis, size_t Tib, cplx *q, size_t qb,
              size_t depth = 0)
    {
        if (rc != NFT_SUCCESS) return;
        if (deg <= kLeaf) {
            PeelLeafParams L;
            std::memset(&L, 0, sizeof(L));
            L.T = T; L.Ts = (long long)Ts; L.d = (int)deg; L.Ti = Ti; L.Tis = (long long)Tis; L.q = q;
            L.eps_t = eps_t; L.kappa = kappa; L.modal = modal; L.status = d_status;
            L.Tb = (long long)Tb; L.Tib = (long long)Tib; L.qb = (long long)qb; L.sb = 1;
            be.template run<KPeelLeaf>(1, (int)batch, L);
            return;
        }
        const size_t h = deg / 2;
        size_t slot = 0;                                                      // work[0] serves degree work_deg
        for (size_t d = work_deg; d > deg; d /= 2) slot++;
        (void)depth;
        Work &w = work[slot];
        const size_t b2i = 4 * (deg + 1), b1 = 4 * (2 * deg + 1), b1i = 4 * (h + 1);   // per signal
        // w.T2i: the child below fills coefficients h .. deg of every entry; 0 .. h-1 are zero since init()
        peel(h, T + h, Ts, Tb, w.T2i + h, deg + 1, b2i, q + h, qb, depth + 1);                    // step 1, :107-116
        prod(deg, w.T2i, deg + 1, b2i, T, Ts, Tb, w.T1, 2 * deg + 1, b1);                        // step 2, :120-127
        peel(h, w.T1 + deg, 2 * deg + 1, b1, w.T1i, h + 1, b1i, q, qb, depth + 1);               // step 3, :131-140
        if (Ti) prod(h, w.T1i, h + 1, b1i, w.T2i + h, deg + 1, b2i, Ti, Tis, Tib);              // step 4, :144-156
    }
    // host-pointer driver: tm (4*(deg+1)) -> q[deg]
    int run_host(size_t deg, const std::complex<double> *tm, std::complex<double> *q)
    {
        int r = init(deg);
        if (r != NFT_SUCCESS) return r;
        DevArena<BE> tmp(be);
        cplx *dT = nullptr, *dq = nullptr;
        if (!(tmp.get(dT, 4 * (deg + 1)) && tmp.get(dq, deg))) return NFT_EC_NOMEM;
        be.h2d(dT, tm, 4 * (deg + 1) * sizeof(cplx));
        peel(deg, dT, deg + 1, 0, nullptr, 0, 0, dq, 0);
        r = rc;
        if (r == NFT_SUCCESS) {
            int hst[4] = {0, 0, 0, 0};
            be.d2h(q, dq, deg * sizeof(cplx));
            be.d2h(hst, d_status, sizeof(hst));
            r = be.sync();
            if (r == NFT_SUCCESS && (hst[0] & 48)) r = NFT_EC_OTHER;      // :173-176 (bit 5: a leaf gave up waiting)
        }
        return r;      // plans and work arrays stay for the next call (destroy() releases them)
    }
};

template <class BE> class NftInverseDev {
public:
    typedef std::complex<double> cd;
    BE &be;
    DevArena<BE> mem;            // owns the tables and the workspace below; the entry points' temporaries have their own
    NftTwiddles<BE> tw;
    NftAnyDft<BE> ft;
    int *dstatus = nullptr;      // the DFTs' status word, shared with the element-wise stages (bit 3: specfact)
    double *dacc = nullptr;
    size_t acc_cap = 0;

    explicit NftInverseDev(BE &b) : be(b), mem(b), ft(b, tw) {}

    // workspace for DFTs of up to nmax points
    int init(size_t nmax)
    {
        if (!tw.init(mem)) return NFT_EC_NOMEM;
        const int rc = ft.init(mem, nmax, 1);
        if (rc != NFT_SUCCESS) return rc;
        dstatus = ft.status;
        acc_cap = (nmax + 255) / 256;
        return mem.get(dacc, acc_cap) ? NFT_SUCCESS : NFT_EC_NOMEM;
    }
    int dft(const cplx *d_in, cplx *d_out, size_t n, int sign) { return ft.dft(d_in, d_out, n, 1, 1, sign); }
    void op(int code, size_t n, const cplx *a, const cplx *b, cplx *out, cplx *out2 = nullptr, double s0 = 0, double s1 = 0,
            double s2 = 0, long long i0 = 0, int kappa = 0, int K = 0, const cplx *bs = nullptr)
    {
        InvOpParams P;
        std::memset(&P, 0, sizeof(P));
        P.op = code; P.n = (long long)n; P.a = a; P.b = b; P.out = out; P.out2 = out2;
        P.s0 = s0; P.s1 = s1; P.s2 = s2; P.i0 = i0; P.kappa = kappa; P.K = K; P.bs = bs;
        P.status = dstatus; P.accum = dacc;
        be.template run<KInvOp>((int)((n + 255) / 256), 1, P);
    }

    // fnft__poly_specfact.c:25-140 on device arrays: d_poly deg+1 coefficients -> d_result deg+1 coefficients;
    // w3: three work arrays of next_fast_size((deg+1)*oversampling) elements.  *warn: ill-posed problem (:109-110)
    static size_t specfact_len(size_t deg, size_t oversampling) { return nft_next_fast_size((deg + 1) * oversampling); }
    int specfact(size_t deg, const cplx *d_poly, cplx *d_result, size_t oversampling, int kappa, cplx *w_in, cplx *w_out,
                 cplx *w_x, int *warn)
    {
        const size_t Mf = specfact_len(deg, oversampling);
        be.memset0(dstatus, 4 * sizeof(int));
        op(INV_PAD, Mf, d_poly, nullptr, w_in, nullptr, 0, 0, 0, (long long)deg);
        int rc = dft(w_in, w_out, Mf, -1);
        if (rc != NFT_SUCCESS) return rc;
        op(INV_SPEC_X, Mf, w_out, nullptr, w_x, nullptr, 0, 0, 0, 0, kappa);
        rc = dft(w_x, w_in, Mf, -1);                     // Hilbert transform of x, :112-125
        if (rc != NFT_SUCCESS) return rc;
        op(INV_HILBERT, Mf, w_in, nullptr, w_in);
        rc = dft(w_in, w_out, Mf, +1);
        if (rc != NFT_SUCCESS) return rc;
        op(INV_SPEC_RESP, Mf, w_x, w_out, w_in);         // exp(x - i y)/M, :129-130
        rc = dft(w_in, w_out, Mf, +1);
        if (rc != NFT_SUCCESS) return rc;
        op(INV_REV_CONJ, deg + 1, w_out, nullptr, d_result, nullptr, 0, 0, 0, (long long)deg);
        int hst[4] = {0, 0, 0, 0};
        be.d2h(hst, dstatus, sizeof(hst));
        rc = be.sync();
        if (warn) *warn = (hst[0] & 8) ? 1 : 0;
        return rc;
    }
    // host-pointer form (the exported fnft__poly_specfact)
    int specfact_host(size_t deg, const cd *poly, cd *result, size_t oversampling, int kappa, int *warn)
    {
        const size_t Mf = specfact_len(deg, oversampling);
        int rc = init(Mf);
        if (rc != NFT_SUCCESS) return rc;
        DevArena<BE> tmp(be);
        cplx *dp = nullptr, *dr = nullptr, *w0 = nullptr, *w1 = nullptr, *w2 = nullptr;
        if (!(tmp.get(dp, deg + 1) && tmp.get(dr, deg + 1) && tmp.get(w0, Mf) && tmp.get(w1, Mf) && tmp.get(w2, Mf)))
            return NFT_EC_NOMEM;
        be.h2d(dp, poly, (deg + 1) * sizeof(cplx));
        rc = specfact(deg, dp, dr, oversampling, kappa, w0, w1, w2, warn);
        if (rc == NFT_SUCCESS) {
            be.d2h(result, dr, (deg + 1) * sizeof(cplx));
            rc = be.sync();
        }
        return rc;
    }

    // ---- continuous part: transfer matrix from the given representation, :302-676 ------------------------------
    // contspec (M values, host) is modified as the reference modifies its argument; tm: 4*(deg+1) host values.
    // cstype 0 rho, 1 b(xi), 2 B(tau); method 0/1 A = 1 (:302-369), 2 iteration (:375-508).  pf: the phase factor
    // the host formed (fnft__nse_discretization.c:240-258 / :319-379)
    int transfer_matrix(size_t M, cd *contspec, const double *XI, size_t K, const cd *bound_states, size_t D,
                        const double *T, size_t deg, cd *tm, int kappa, int cstype, int method, size_t max_iter,
                        size_t oversampling, double pf, int *warn_specfact, int *warn_maxiter)
    {
        *warn_specfact = 0;
        *warn_maxiter = 0;
        const size_t os = (cstype == 0) ? 32 : oversampling;
        const bool need_sf = (cstype != 0) || method == 2;
        const size_t sf_deg = (cstype == 1) ? deg : D - 1;
        const size_t Mf = need_sf ? specfact_len(sf_deg, os) : 0;
        int rc = init(std::max(M, Mf));
        if (rc != NFT_SUCCESS) return rc;
        const double eps_t = (T[1] - T[0]) / (double)(D - 1);
        DevArena<BE> tmp(be);
        cplx *dc = nullptr, *dr = nullptr, *db = nullptr, *da = nullptr, *dbs = nullptr;
        cplx *w0 = nullptr, *w1 = nullptr, *w2 = nullptr;
        bool ok = tmp.get(dc, M) && tmp.get(dr, M) && tmp.get(db, std::max(M, deg + 1)) && tmp.get(da, deg + 1)
                  && tmp.get(dbs, K ? K : 1);
        if (need_sf) ok = ok && tmp.get(w0, Mf) && tmp.get(w1, Mf) && tmp.get(w2, Mf);
        std::vector<cd> hb, ha;
        for (size_t i = 0; i < 4 * (deg + 1); i++) tm[i] = 0.0;
        if (!ok) return NFT_EC_NOMEM;
        if (rc == NFT_SUCCESS && cstype != 2) {
            // :251-296 (and :1013-1033 for the reflection coefficient): phases off, FFT order
            const double eps_xi = (XI[1] - XI[0]) / (double)(M - 1);
            be.h2d(dc, contspec, M * sizeof(cplx));
            const size_t Kp = (cstype == 0) ? K : 0;
            if (Kp) be.h2d(dbs, bound_states, Kp * sizeof(cplx));
            op(INV_PREP, M, dc, nullptr, dc, dr, XI[0], eps_xi, pf, 0, 0, (int)Kp, dbs);
            be.d2h(contspec, dc, M * sizeof(cplx));
            rc = be.sync();
        }
        if (rc == NFT_SUCCESS && (cstype == 1 || (cstype == 0 && method != 2))) {
            rc = dft(dr, db, M, -1);                                       // B(z) from an M-point FFT, :340 / :594
            hb.resize(M);
            if (rc == NFT_SUCCESS) { be.d2h(hb.data(), db, M * sizeof(cplx)); rc = be.sync(); }
            if (rc == NFT_SUCCESS) {
                const size_t i0 = (deg <= M - 1) ? 0 : deg - (M - 1);
                const double invM = 1.0 / (double)M;
                for (size_t i = i0; i <= deg; i++) {
                    tm[1 * (deg + 1) + i] = -(double)kappa * std::conj(hb[M - 1 - deg + i] * invM);
                    tm[2 * (deg + 1) + i] = hb[deg - i] * invM;
                }
                if (cstype == 0) {                                         // A(z) = 1, :363-364
                    tm[deg] = 1.0;
                    tm[3 * (deg + 1)] = 1.0;
                } else {                                                   // A by spectral factorization, :615-620
                    be.h2d(db, tm + 2 * (deg + 1), (deg + 1) * sizeof(cplx));
                    rc = specfact(deg, db, da, os, kappa, w0, w1, w2, warn_specfact);
                    if (rc == NFT_SUCCESS) { be.d2h(tm, da, (deg + 1) * sizeof(cplx)); rc = be.sync(); }
                    for (size_t i = 0; i <= deg; i++) tm[3 * (deg + 1) + i] = tm[deg - i];
                }
            }
        } else if (rc == NFT_SUCCESS && cstype == 0) {
            // Algorithm 1 of arXiv:1607.01305v2, :375-508 (M = D = deg, defocusing; checked by the host)
            double prev_change = INFINITY, prev_diff = INFINITY;
            size_t iter = 0;
            std::vector<double> part((D + 255) / 256);
            for (; iter < max_iter && rc == NFT_SUCCESS; iter++) {
                op(INV_ITER_FIN, D, dr, nullptr, db, nullptr, 0, 0, 0, 0, kappa);
                rc = dft(db, w0, D, -1);
                if (rc != NFT_SUCCESS) break;
                op(INV_REVERSE, D, w0, nullptr, db);                                  // b_coeffs
                int w = 0;
                rc = specfact(D - 1, db, da, 32, kappa, w0, w1, w2, &w);               // a_coeffs
                if (rc != NFT_SUCCESS) break;
                *warn_specfact |= w;
                op(INV_REVERSE, D, da, nullptr, w0);
                rc = dft(w0, w1, D, +1);
                if (rc != NFT_SUCCESS) break;
                op(INV_ITER_PHASE, D, w1, dc, dr);
                be.d2h(part.data(), dacc, part.size() * sizeof(double));
                rc = be.sync();
                if (rc != NFT_SUCCESS) break;
                double cur = 0.0;
                for (double v : part) cur += v;
                cur /= (double)D;
                const double diff = std::fabs(cur - prev_change);
                if (diff < 10.0 * 2.220446049250313e-16) break;
                prev_change = cur;
                if (diff > 0.9 * prev_diff) break;
                prev_diff = diff;
            }
            if (iter == max_iter) *warn_maxiter = 1;
            if (rc == NFT_SUCCESS) {
                ha.resize(D); hb.resize(D);
                be.d2h(ha.data(), da, D * sizeof(cplx));
                be.d2h(hb.data(), db, D * sizeof(cplx));
                rc = be.sync();
            }
            if (rc == NFT_SUCCESS)
                for (size_t i = 0; i < D; i++) {
                    tm[1 + i] = ha[i];
                    tm[1 * (deg + 1) + i] = -(double)kappa * std::conj(hb[D - 1 - i]);
                    tm[2 * (deg + 1) + 1 + i] = hb[i];
                    tm[3 * (deg + 1) + i] = ha[D - 1 - i];
                }
        } else if (rc == NFT_SUCCESS) {
            // B(tau), :632-676 (degree1step = 1 for both admissible discretizations)
            be.h2d(dc, contspec, D * sizeof(cplx));
            op(INV_BTAU, D, dc, nullptr, db, nullptr, eps_t);
            rc = specfact(D - 1, db, da, os, kappa, w0, w1, w2, warn_specfact);
            if (rc == NFT_SUCCESS) {
                ha.resize(D); hb.resize(D);
                be.d2h(ha.data(), da, D * sizeof(cplx));
                be.d2h(hb.data(), db, D * sizeof(cplx));
                rc = be.sync();
            }
            if (rc == NFT_SUCCESS)
                for (size_t i = 0; i < D; i++) {
                    tm[1 + i] = ha[i];
                    tm[2 * (deg + 1) + 1 + i] = hb[i];
                    tm[1 * (deg + 1) + i] = -(double)kappa * std::conj(hb[D - 1 - i]);
                    tm[3 * (deg + 1) + i] = ha[D - 1 - i];
                }
        }
        return rc;
    }

    // ---- discrete part, :680-903 ------------------------------------------------------------------------------
    // bs / nc: sorted bound states and NORMING CONSTANTS (the host converted residues); mode 0: pure solitons
    // (:797-842), 1: Darboux steps on the seed q (:843-889)
    int add_discrete(size_t K, const cd *bs, const cd *nc, size_t D, cd *q, const double *T, int mode)
    {
        const double eps_t = (T[1] - T[0]) / (double)(D - 1);
        InvDsParams P;
        std::memset(&P, 0, sizeof(P));
        DevArena<BE> tmp(be);
        cplx *dbs = nullptr, *dnc = nullptr, *dq = nullptr, *work = nullptr;
        if (!(tmp.get(dbs, K) && tmp.get(dnc, K) && tmp.get(dq, D) && tmp.get(work, (mode ? 2 : 1) * K * D)))
            return NFT_EC_NOMEM;
        cplx *dq2 = nullptr, *cm = nullptr, *bnd = nullptr, *bndp = nullptr, *PHI = nullptr, *PSI = nullptr, *dout = nullptr;
        be.h2d(dbs, bs, K * sizeof(cplx));
        be.h2d(dnc, nc, K * sizeof(cplx));
        P.D = (long long)D; P.K = (int)K; P.bs = dbs; P.nc = dnc; P.T0 = T[0]; P.eps_t = eps_t;
        P.q = dq; P.work = work;
        size_t zc = 0;                                    // :726-733: first sample with t >= 0 (0 if none)
        for (size_t i = 0; i < D; i++)
            if (T[0] + eps_t * (double)i >= 0.0) { zc = i; break; }
        P.zc = (long long)zc;
        if (mode == 0) {
            be.template run<KInvSolitons>((int)((D + 255) / 256), 1, P);
        } else {
            // eigenfunctions of the seed on the half-step signal (nft_bs_eigenfunctions)
            const size_t D2 = 2 * (D - 1);
            BsParams B;
            std::memset(&B, 0, sizeof(B));
            const size_t L = nft_bs_chunk_len(D2);
            const size_t nchunk = (D2 + L - 1) / L;
            if (!(tmp.get(dq2, D2) && tmp.get(cm, K * nchunk * 8) && tmp.get(bnd, K * (nchunk + 1) * 2)
                  && tmp.get(bndp, K * (nchunk + 1) * 2) && tmp.get(PHI, K * D * 2) && tmp.get(PSI, K * D * 2)
                  && tmp.get(dout, 3 * K)))
                return NFT_EC_NOMEM;
            be.h2d(dq, q, D * sizeof(cplx));
            InvOpParams O;
            std::memset(&O, 0, sizeof(O));
            O.op = INV_DOUBLE_Q; O.n = (long long)D2; O.a = dq; O.out = dq2;
            be.template run<KInvOp>((int)((D2 + 255) / 256), 1, O);
            B.q = dq2; B.D = (long long)D2;
            B.K = (int)K; B.lam = dbs; B.L = (int)L; B.nchunk = (int)nchunk;
            B.cm = cm; B.bnd = bnd; B.bndp = bndp; B.PHI = PHI; B.PSI = PSI;
            B.a = dout; B.aprime = dout + K; B.b = dout + 2 * K;
            nft_bs_eigenfunctions(be, (int)((nchunk + 63) / 64), (int)K, B, T, eps_t);
            P.PHI = PHI; P.PSI = PSI;
            be.template run<KInvCdt>((int)((D + 255) / 256), 1, P);
        }
        be.d2h(q, dq, D * sizeof(cplx));
        return be.sync();
    }
};

// Batched discrete part of fnft_nsev_inverse (src/fnft_nsev_inverse.c:680-903): K bound states and norming constants
// (or residues) per signal, for `batch` signals of D samples, one launch per stage for the whole batch.  Per signal the
// arithmetic is that of the host-pointer driver (fnft_amd__inverse_add_discrete, NftInverseDev::add_discrete): the same
// kernels, with the host's bookkeeping -- the check Im lambda > 0, the sort, the check for equal neighbours and the
// conversion of residues -- in KInvDsPrep, one lane per signal.  mode 0: pure solitons (:797-842); 1: Darboux steps on
// the seed in q (:843-889), which is the plan's continuous part (seed_cs) or the caller's q.  Every array is allocated
// by init(); signal s of an array of n values per signal starts at s*n.
template <class BE> class NftInverseDiscBatch {
public:
    static constexpr size_t kMaxGridY = 65535;   // grid.y of one launch: larger batches go in slices of whole signals
    BE &be;
    DevArena<BE> mem;            // owns every array below
    const size_t D, B, K;
    const int mode;
    const bool residues, seed_cs;
    size_t L = 0, nchunk = 0, Lr = 0, nchunk_r = 0, ncm = 0;
    cplx *bs = nullptr, *nc = nullptr, *work = nullptr;                                  // sorted copies; rho_k or S1, S2
    cplx *q2 = nullptr, *cm = nullptr, *bnd = nullptr, *bndp = nullptr, *PHI = nullptr, *PSI = nullptr, *aout = nullptr;

    NftInverseDiscBatch(BE &b, size_t D_, size_t B_, size_t K_, int mode_, bool residues_, bool seed_cs_)
        : be(b), mem(b), D(D_), B(B_), K(K_), mode(mode_), residues(residues_), seed_cs(seed_cs_) {}
    size_t work_per_signal() const { return (mode ? 2 : 1) * K * D; }
    int init()
    {
        bool ok = mem.get(bs, B * K) && mem.get(nc, B * K) && mem.get(work, B * work_per_signal());
        if (mode == 1) {
            const size_t D2 = 2 * (D - 1);
            L = nft_bs_chunk_len(D2);
            nchunk = (D2 + L - 1) / L;
            ncm = nchunk;
            if (residues && seed_cs) {          // a(lambda_k) of the seed, BO scheme on its D samples
                Lr = nft_bs_chunk_len(D);
                nchunk_r = (D + Lr - 1) / Lr;
                ncm = std::max(ncm, nchunk_r);
            }
            ok = ok && mem.get(q2, B * D2) && mem.get(cm, B * K * ncm * 8) && mem.get(bnd, B * K * (ncm + 1) * 2)
                 && mem.get(bndp, B * K * (ncm + 1) * 2) && mem.get(PHI, B * K * D * 2) && mem.get(PSI, B * K * D * 2)
                 && mem.get(aout, 2 * B * K);
        }
        return ok ? NFT_SUCCESS : NFT_EC_NOMEM;
    }
    // stage 0 of KInvDsPrep: d_bs, d_nc are the caller's arrays; status: one word per signal
    void check_and_sort(const cplx *d_bs, const cplx *d_nc, int *status)
    {
        InvDsPrepParams P;
        std::memset(&P, 0, sizeof(P));
        P.B = (long long)B; P.K = (int)K; P.stage = 0; P.residues = (residues && !seed_cs) ? 1 : 0;
        P.bs_in = d_bs; P.nc_in = d_nc; P.bs = bs; P.nc = nc; P.status = status;
        be.template run<KInvDsPrep>((int)((B + 63) / 64), 1, P);
    }
    // the scatterer's parameters for signals s0 .. s0 + ns - 1 of the batch (strides: see BsParams)
    BsParams bs_params(const cplx *q, size_t Dq, size_t s0) const
    {
        BsParams P;
        std::memset(&P, 0, sizeof(P));
        P.K = (int)K;
        P.q = q + s0 * Dq; P.lam = bs + s0 * K;
        P.cm = cm + s0 * K * ncm * 8; P.bnd = bnd + s0 * K * (ncm + 1) * 2; P.bndp = bndp + s0 * K * (ncm + 1) * 2;
        P.PHI = PHI + s0 * K * D * 2; P.PSI = PSI + s0 * K * D * 2;
        P.a = aout + s0 * K; P.aprime = aout + B * K + s0 * K;
        P.sq = (long long)Dq; P.slam = (long long)K; P.scm = (long long)(K * ncm * 8);
        P.sbnd = (long long)(K * (ncm + 1) * 2); P.sphi = (long long)(K * D * 2); P.sab = (long long)K;
        return P;
    }
    InvDsParams ds_params(cplx *q, double T0, double eps_t, size_t zc, size_t s0) const
    {
        InvDsParams P;
        std::memset(&P, 0, sizeof(P));
        P.D = (long long)D; P.K = (int)K; P.T0 = T0; P.eps_t = eps_t; P.zc = (long long)zc;
        P.bs = bs + s0 * K; P.nc = nc + s0 * K; P.q = q + s0 * D; P.work = work + s0 * work_per_signal();
        if (mode == 1) { P.PHI = PHI + s0 * K * D * 2; P.PSI = PSI + s0 * K * D * 2; }
        P.sbs = (long long)K; P.sq = (long long)D; P.swork = (long long)work_per_signal();
        P.sphi = (long long)(K * D * 2);
        return P;
    }
    // d_q: the seed on entry (mode 1), the signals on exit; T: host, shared by the batch.  check_and_sort() has run.
    void run(cplx *d_q, const double *T, int *status)
    {
        const double eps_t = (T[1] - T[0]) / (double)(D - 1);
        size_t zc = 0;                                    // :726-733: first sample with t >= 0 (0 if none)
        for (size_t i = 0; i < D; i++)
            if (T[0] + eps_t * (double)i >= 0.0) { zc = i; break; }
        const size_t per_y = kMaxGridY / K;               // signals per slice of a launch with grid.y = signal*K + k
        if (residues && seed_cs) {
            // :771-795 with a continuous part: a(lambda_k) of the seed by the slow scatterer, BO scheme
            // (NftDiscSpec::prepare(2SPLIT4B, need_tree = false) and scatter(skip_b = true) on the drop-in's path)
            const double eps_in = (T[1] - T[0]) / (double)(D - 1);
            const double T1 = T[0] + (double)(D - 1) * eps_in;
            for (size_t s0 = 0; s0 < B; s0 += per_y) {
                const size_t ns = std::min(per_y, B - s0);
                BsParams P = bs_params(d_q, D, s0);
                P.D = (long long)D; P.ups = 1; P.lscale = 1.0;
                P.T0 = T[0]; P.T1 = T1; P.eps = (T1 - T[0]) / (double)(D - 1);
                P.L = (int)Lr; P.nchunk = (int)nchunk_r;
                nft_bs_forward(be, (int)((nchunk_r + 63) / 64), (int)(ns * K), P);
            }
            InvDsPrepParams R;
            std::memset(&R, 0, sizeof(R));
            R.B = (long long)B; R.K = (int)K; R.stage = 1; R.bs = bs; R.nc = nc; R.acs = aout; R.status = status;
            be.template run<KInvDsPrep>((int)((B + 63) / 64), 1, R);
        }
        const int gx = (int)((D + 255) / 256);
        if (mode == 0) {
            for (size_t s0 = 0; s0 < B; s0 += kMaxGridY)
                be.template run<KInvSolitons>(gx, (int)std::min(kMaxGridY, B - s0), ds_params(d_q, T[0], eps_t, zc, s0));
            return;
        }
        // eigenfunctions of the seed on the half-step signal (nft_bs_eigenfunctions)
        const size_t D2 = 2 * (D - 1);
        for (size_t s0 = 0; s0 < B; s0 += kMaxGridY) {
            InvOpParams O;
            std::memset(&O, 0, sizeof(O));
            O.op = INV_DOUBLE_Q; O.n = (long long)D2; O.a = d_q + s0 * D; O.out = q2 + s0 * D2;
            O.sa = (long long)D; O.sout = (long long)D2;
            be.template run<KInvOp>((int)((D2 + 255) / 256), (int)std::min(kMaxGridY, B - s0), O);
        }
        for (size_t s0 = 0; s0 < B; s0 += per_y) {
            const size_t ns = std::min(per_y, B - s0);
            BsParams P = bs_params(q2, D2, s0);
            P.D = (long long)D2;
            P.L = (int)L; P.nchunk = (int)nchunk;
            nft_bs_eigenfunctions(be, (int)((nchunk + 63) / 64), (int)(ns * K), P, T, eps_t);
        }
        for (size_t s0 = 0; s0 < B; s0 += kMaxGridY)
            be.template run<KInvCdt>(gx, (int)std::min(kMaxGridY, B - s0), ds_params(d_q, T[0], eps_t, zc, s0));
    }
};

// Batched, device-resident continuous part of fnft_nsev_inverse (K = 0): `batch` signals of one size and one set of
// options per call, every launch covering the whole batch, nothing copied to or from the host and no allocation while
// a call runs.  Per signal the arithmetic is that of the host-pointer driver above (NftInverseDev::transfer_matrix,
// then NftLayerPeelingDev::run_host): the same kernels, with the transfer matrix formed on the device (INV_TM_B /
// INV_TM_AB) instead of on the host.  Every array holds the signals back to back.
// K > 0: a discrete stage (NftInverseDiscBatch) follows; M = 0 then means no continuous part at all.
template <class BE> class NftInverseBatch {
public:
    BE &be;
    const size_t D, M, B;
    const int cstype;            // 0 rho, 1 b(xi), 2 B(tau)
    const size_t os;             // oversampling factor of the spectral factorization
    const size_t K;              // bound states per signal
    const int ds_mode, ds_residues;
    DevArena<BE> mem;            // owns the tables and the arrays of the continuous part below
    NftTwiddles<BE> tw;          // one set: the DFTs', the peeler's and its trees'
    NftAnyDft<BE> ft;
    NftLayerPeelingDev<BE> lp;
    std::unique_ptr<NftInverseDiscBatch<BE>> ds;
    size_t Mf = 0;
    cplx *dc = nullptr, *dr = nullptr, *db = nullptr, *da = nullptr, *dtm = nullptr;
    cplx *w0 = nullptr, *w1 = nullptr, *w2 = nullptr;

    NftInverseBatch(BE &b, size_t D_, size_t M_, size_t B_, int cstype_, size_t os_, int modal, size_t K_ = 0,
                    int ds_mode_ = 0, int ds_residues_ = 0)
        : be(b), D(D_), M(M_), B(B_), cstype(cstype_), os(os_), K(K_), ds_mode(ds_mode_), ds_residues(ds_residues_),
          mem(b), ft(b, tw), lp(b, 1.0, 1, modal, &tw)
    {
        lp.batch = B;
    }
    size_t workspace_bytes() const
    {
        return mem.bytes + lp.workspace_bytes() + (ds ? ds->mem.bytes : 0);
    }
    int init()
    {
        if (M > 0) {
            const int r = init_continuous();
            if (r != NFT_SUCCESS) return r;
        } else {
            const int r = lp.init(0);                 // the status words only
            if (r != NFT_SUCCESS) return r;
        }
        if (K > 0) {
            ds.reset(new (std::nothrow) NftInverseDiscBatch<BE>(be, D, B, K, ds_mode, ds_residues != 0, M > 0));
            if (!ds) return NFT_EC_NOMEM;
            const int r = ds->init();
            if (r != NFT_SUCCESS) return r;
        }
        return be.sync();
    }
    int init_continuous()
    {
        const size_t deg = D;
        if (cstype != 0) Mf = NftInverseDev<BE>::specfact_len(cstype == 1 ? deg : D - 1, os);
        if (!tw.init(mem)) return NFT_EC_NOMEM;
        const int r = ft.init(mem, std::max(cstype == 2 ? D : M, Mf), B);
        if (r != NFT_SUCCESS) return r;
        bool ok = mem.get(dtm, B * 4 * (deg + 1));
        if (cstype != 2) ok = ok && mem.get(dc, B * M) && mem.get(dr, B * M) && mem.get(db, B * M);
        else ok = ok && mem.get(db, B * D) && mem.get(da, B * D);
        if (cstype != 0) ok = ok && mem.get(w0, B * Mf) && mem.get(w1, B * Mf) && mem.get(w2, B * Mf);
        if (!ok) return NFT_EC_NOMEM;
        return lp.prepare(deg);
    }
    // out[s*n + k] = sum_j in[s*n + j] exp(sign 2 pi i j k / n) for every signal s
    int dft(const cplx *d_in, cplx *d_out, size_t n, int sign) { return ft.dft(d_in, d_out, n, B, 1, sign); }
    // body_inv_op over n elements of every signal; sa, sb, so: distances between the signals of a, b, out
    void op(int code, size_t n, const cplx *a, size_t sa, const cplx *b, size_t sb, cplx *out, size_t so,
            cplx *out2 = nullptr, size_t so2 = 0, double s0 = 0, double s1 = 0, double s2 = 0, long long i0 = 0,
            int kappa = 0, long long i1 = 0, const cplx *bs = nullptr)
    {
        InvOpParams P;
        std::memset(&P, 0, sizeof(P));
        P.op = code; P.n = (long long)n; P.a = a; P.b = b; P.out = out; P.out2 = out2;
        P.s0 = s0; P.s1 = s1; P.s2 = s2; P.i0 = i0; P.i1 = i1; P.kappa = kappa;
        P.sa = (long long)sa; P.sb = (long long)sb; P.sout = (long long)so; P.sout2 = (long long)so2;
        if (bs) { P.K = (int)K; P.bs = bs; P.sbs = (long long)K; }   // INV_PREP: Blaschke factors
        P.status = lp.d_status; P.sst = 1;
        be.template run<KInvOp>((int)((n + 255) / 256), (int)B, P);
    }
    // NftInverseDev::specfact for every signal: poly (deg+1 coefficients at distance pb) -> result (distance rb)
    int specfact(size_t deg, const cplx *poly, size_t pb, cplx *result, size_t rb, int kappa)
    {
        op(INV_PAD, Mf, poly, pb, nullptr, 0, w0, Mf, nullptr, 0, 0, 0, 0, (long long)deg);
        int rc = dft(w0, w1, Mf, -1);
        if (rc != NFT_SUCCESS) return rc;
        op(INV_SPEC_X, Mf, w1, Mf, nullptr, 0, w2, Mf, nullptr, 0, 0, 0, 0, 0, kappa);
        rc = dft(w2, w0, Mf, -1);
        if (rc != NFT_SUCCESS) return rc;
        op(INV_HILBERT, Mf, w0, Mf, nullptr, 0, w0, Mf);
        rc = dft(w0, w1, Mf, +1);
        if (rc != NFT_SUCCESS) return rc;
        op(INV_SPEC_RESP, Mf, w2, Mf, w1, Mf, w0, Mf);
        rc = dft(w0, w1, Mf, +1);
        if (rc != NFT_SUCCESS) return rc;
        op(INV_REV_CONJ, deg + 1, w1, Mf, nullptr, 0, result, rb, nullptr, 0, 0, 0, 0, (long long)deg);
        return NFT_SUCCESS;
    }
    // d_cs: B*M values (B(tau): B*D), d_q: B*D samples.  pf, eps_t: formed by the caller as the host driver forms
    // them.  Enqueued on be.stream; the per-signal status words are read by the caller after the stream is done.
    int run(const cplx *d_cs, const double *XI, cplx *d_q, double eps_t, int kappa, double pf)
    {
        reset(eps_t, kappa);
        return continuous(d_cs, XI, d_q, eps_t, kappa, pf, nullptr);
    }
    // K > 0: d_bs, d_nc: batch*K bound states and norming constants / residues (the caller's, read only); d_cs and XI
    // unused if M = 0; d_q: the seed on entry if the plan has no continuous part and mode 1; T: host
    int run_discrete(const cplx *d_cs, const double *XI, const cplx *d_bs, const cplx *d_nc, cplx *d_q, const double *T,
                     double eps_t, int kappa, double pf)
    {
        reset(eps_t, kappa);
        ds->check_and_sort(d_bs, d_nc, lp.d_status);
        if (M > 0) {
            // the Blaschke factors of the reflection coefficient take the bound states in the caller's order, as the
            // drop-in uploads them (:1013-1033); the Darboux steps the sorted ones
            const int rc = continuous(d_cs, XI, d_q, eps_t, kappa, pf, cstype == 0 ? d_bs : nullptr);
            if (rc != NFT_SUCCESS) return rc;
        }
        ds->run(d_q, T, lp.d_status);
        return NFT_SUCCESS;
    }
    void reset(double eps_t, int kappa)
    {
        lp.rc = NFT_SUCCESS;
        lp.eps_t = eps_t;
        lp.kappa = kappa;
        be.memset0(lp.d_status, lp.status_words() * sizeof(int));
    }
    int continuous(const cplx *d_cs, const double *XI, cplx *d_q, double eps_t, int kappa, double pf, const cplx *d_bs)
    {
        const size_t deg = D, per = 4 * (deg + 1);
        int rc = NFT_SUCCESS;
        if (cstype != 2) {
            const double eps_xi = (XI[1] - XI[0]) / (double)(M - 1);
            op(INV_PREP, M, d_cs, M, nullptr, 0, dc, M, dr, M, XI[0], eps_xi, pf, 0, 0, 0, d_bs);
            rc = dft(dr, db, M, -1);                                                  // B(z), :340 / :594
            if (rc != NFT_SUCCESS) return rc;
            const long long i0 = (deg <= M - 1) ? 0 : (long long)(deg - (M - 1));
            op(INV_TM_B, per, db, M, nullptr, 0, dtm, per, nullptr, 0, 1.0 / (double)M, cstype == 0 ? 1.0 : 0.0, 0, i0,
               kappa, (long long)M);
            if (cstype == 1) {                                                        // A, :615-620
                rc = specfact(deg, dtm + 2 * (deg + 1), per, dtm, per, kappa);
                if (rc != NFT_SUCCESS) return rc;
                op(INV_REVERSE, deg + 1, dtm, per, nullptr, 0, dtm + 3 * (deg + 1), per);
            }
        } else {                                                                      // :632-676
            op(INV_BTAU, D, d_cs, D, nullptr, 0, db, D, nullptr, 0, eps_t);
            rc = specfact(D - 1, db, D, da, D, kappa);
            if (rc != NFT_SUCCESS) return rc;
            op(INV_TM_AB, per, da, D, db, D, dtm, per, nullptr, 0, 0, 0, 0, 0, kappa);
        }
        lp.peel(deg, dtm, deg + 1, per, nullptr, 0, 0, d_q, D);
        return lp.rc;
    }
    // after the stream is done: status word of every signal (bit 3 ill-posed factorization, bits 4, 5 the leaf's;
    // K > 0: bit 6 a bound state with Im <= 0, bit 7 equal bound states)
    int read_status(std::vector<int> &st)
    {
        st.assign(B, 0);
        be.d2h(st.data(), lp.d_status, B * sizeof(int));
        return be.sync();
    }
};
