// nft_nsev_slow.h -- batched, device-resident continuous spectrum of fnft_nsev under the slow discretizations (BO,
// CF4_2, CF4_3, CF5_3, CF6_4, ES4, TES4): `batch` signals of D samples on one xi-grid of M points, every array on the
// device, nothing read back.  Per signal it computes what the reference's fnft_nsev writes to contspec (src/fnft_nsev.c:
// 133-453, nsev_compute_contspec :763-891):
//   band-limited shifts (NftResampler, CF4_2 ... CF6_4) -> record kernel -> scatter kernel over
//   (xi tile, chunk, signal) -> [reduce kernel: chunk maps in groups, from 64 chunks on] -> combine kernel (chunk or
//   group maps, phase factors, Richardson extrapolation, status)
// With Richardson extrapolation the first three stages run a second time on every nskip-th sample inside the same call.
// Back-end independent like NftDiscSpecBatch: hip_backend.hip instantiates it with the HIP back end, tests/emu with the
// lane emulator.
#pragma once
#include "nft_discspec.h"

struct NftSlowOpts {
    int nse_disc = 1;      // fnft_nse_discretization_t ordinal: 1 BO, 22 CF4_2 ... 27 TES4
    int cstype = 0;        // 0 rho, 1 a b, 2 rho a b
    int richardson = 0;
};

// scheme index of the kernels (SlowParams::scheme), -1: not a slow discretization
inline int nft_slow_scheme(int nse_disc)
{
    if (nse_disc == 1) return 0;
    return (nse_disc >= 22 && nse_disc <= 27) ? nse_disc - 21 : -1;
}
inline int nft_slow_upsampling(int scheme) { const int u[7] = {1, 2, 3, 3, 4, 3, 3}; return u[scheme]; }
inline int nft_slow_order(int scheme) { const int o[7] = {2, 4, 4, 5, 6, 4, 4}; return o[scheme]; }

// Chunks of the sample axis.  One lane owns one xi; batch * ceil(M/64) waves of 64 lanes fill the card only for large
// M * batch, so the G grid points are cut into chunks until about two waves per SIMD are in flight (256 CUs x 4 SIMDs
// x 2 = 2048 waves), with at least 16 grid points per chunk.  For few xi and a long signal that is up to 2048 chunks:
// a wave whose 64 lanes hold 16 xi still occupies its SIMD, so every SIMD needs a chunk of its own.  L: grid points
// per chunk; returns the number of chunks.
inline size_t nft_slow_chunks(size_t G, size_t M, size_t batch, size_t *L)
{
    const size_t waves = batch * ((M + 63) / 64);
    size_t nc = (size_t)2048 / waves;
    if (nc > G / 16) nc = G / 16;
    if (nc < 1) nc = 1;
    *L = (G + nc - 1) / nc;
    return (G + *L - 1) / *L;
}
// from this many chunks on, their maps are multiplied in groups of about sqrt(nchunk) first (KSlowReduce)
constexpr size_t kSlowReduceFrom = 64;
inline size_t nft_slow_group(size_t nchunk)
{
    if (nchunk < kSlowReduceFrom) return 1;
    size_t g = 1;
    while (g * g < nchunk) g++;
    return g;
}

// resampling weights (12) and lambda weights (4) of a scheme, src/private/fnft__akns_discretization.c:243-381 and
// fnft__akns_scatter_matrix.c:101-109,116-158, in double exactly as the reference forms them; returns the shift of the
// two resampled copies in steps (0: no resampling)
inline double nft_slow_weights(int scheme, std::complex<double> *w)
{
    typedef std::complex<double> Z;
    for (int i = 0; i < 16; i++) w[i] = Z(0.0, 0.0);
    int rows = 1, cols = 1;
    double shift = 0.0;
    switch (scheme) {
    case 1: {
        const double s = std::sqrt(3.0) / 6.0;
        w[0] = 0.25 + s; w[1] = 0.25 - s; w[2] = 0.25 - s; w[3] = 0.25 + s;
        rows = 2; cols = 2; shift = s;
        break;
    }
    case 2: {
        const double f[3][3] = {{11.0 / 40.0, 20.0 / 87.0, 7.0 / 50.0}, {9.0 / 20.0, 0.0, -7.0 / 25.0},
                                {11.0 / 40.0, -20.0 / 87.0, 7.0 / 50.0}};
        const double wm[3] = {5.0 / 18.0, 4.0 / 9.0, 5.0 / 18.0};
        const double xm[3] = {2.0 * std::sqrt(3.0 / 20.0), 0.0, -2.0 * std::sqrt(3.0 / 20.0)};
        for (int m = 0; m < 3; m++)
            for (int i = 0; i < 3; i++) {
                Z a(0.0, 0.0);
                for (int n = 0; n < 3; n++) {
                    double P = 1.0;   // Legendre polynomial of degree n at xm[m], by the reference's recursion
                    if (n == 1) P = xm[m];
                    if (n == 2) P = (2.0 * 2 - 1) * xm[m] * xm[m] / 2 - (2 - 1.0) * 1.0 / 2;
                    a = a + (double)(2 * n + 1) * P * f[i][n];
                }
                w[i * 3 + m] = a * wm[m];
            }
        rows = 3; cols = 3; shift = std::sqrt(3.0 / 20.0);
        break;
    }
    case 3: {
        const double s15 = std::sqrt(15.0);
        w[0] = Z((145.0 + 37.0 * s15) / 900.0, (5.0 + 3.0 * s15) / 300.0);
        w[1] = Z(-1.0 / 45.0, 1.0 / 15.0);
        w[2] = Z((145.0 - 37.0 * s15) / 900.0, (5.0 - 3.0 * s15) / 300.0);
        w[3] = Z(-2.0 / 45.0, -s15 / 50.0);
        w[4] = 22.0 / 45.0;
        w[5] = std::conj(w[3]); w[6] = std::conj(w[2]); w[7] = std::conj(w[1]); w[8] = std::conj(w[0]);
        rows = 3; cols = 3; shift = s15 / 10.0;
        break;
    }
    case 4: {
        const Z c[6] = {Z(0.245985577298764, 0.038734389227165), Z(-0.046806149832549, 0.012442141491185),
                        Z(0.010894359342569, -0.004575808769067), Z(0.062868370946917, -0.048761268117765),
                        Z(0.269028372054771, -0.012442141491185), Z(-0.041970529810473, 0.014602687659668)};
        for (int i = 0; i < 6; i++) { w[i] = c[i]; w[11 - i] = c[i]; }
        rows = 4; cols = 3; shift = std::sqrt(15.0) / 10.0;
        break;
    }
    default:
        w[0] = 1.0;
        break;
    }
    for (int i = 0; i < rows; i++) {
        Z l(0.0, 0.0);
        for (int j = 0; j < cols; j++) l = l + w[i * cols + j];
        w[12 + i] = (scheme == 0) ? Z(1.0, 0.0) : l;
    }
    if (scheme == 1) w[13] = w[12];   // :128-129: both positions take l_weights[0]
    return shift;
}

template <class BE> class NftSlowPlan {
public:
    BE &be;
    DevArena<BE> mem;                 // owns every device buffer below
    const size_t D, M, batch;
    const NftSlowOpts o;
    int scheme = -1, ups = 1, fam = 0;
    bool realk = false;
    double shift = 0.0;               // of the resampled copies, in kept steps
    size_t nskip2 = 1, D2 = 0;        // Richardson pass: stride and kept grid points
    size_t L = 1, nchunk = 1, nchunk2 = 0, ntile = 1;
    size_t per = 1;                   // record values per grid point
    NftTwiddles<BE> tw;
    NftResampler<BE> rs;              // CF4_2 ... CF6_4 from kSlowDirectBelow samples on (resample): the shifted copies
    bool resample = false;
    cplx *wtab = nullptr, *rec = nullptr, *rec2 = nullptr, *cm = nullptr, *cm2 = nullptr, *cmr = nullptr, *cmr2 = nullptr;
    size_t gsize = 1;                 // chunk maps per group of the reduce stage (1: none)
    int *status = nullptr, *warn = nullptr;
    static constexpr size_t kMaxGroups = 0x7fffffff;

    NftSlowPlan(BE &be_, size_t D_, size_t M_, size_t batch_, const NftSlowOpts &o_)
        : be(be_), mem(be_), D(D_), M(M_), batch(batch_), o(o_), rs(be_, tw)
    {
        scheme = nft_slow_scheme(o.nse_disc);
        if (scheme < 0) return;
        ups = nft_slow_upsampling(scheme);
        fam = scheme <= 4 ? 0 : scheme - 4;
        realk = scheme <= 2;
        per = fam == 0 ? (size_t)ups * kSlowRecCf : (fam == 1 ? (size_t)kSlowRecEs : (size_t)kSlowRecTes);
        ntile = (M + kSlowLanes - 1) / kSlowLanes;
        nchunk = nft_slow_chunks(D, M, batch, &L);
        gsize = nft_slow_group(nchunk);
        if (o.richardson) {   // nft_sub_grid for Dsub = D/2, fnft_nsev.c:376
            const NftSubGrid g = nft_sub_grid(D, D / 2);
            nskip2 = g.nskip; D2 = g.Dsub;
            nchunk2 = (D2 + L - 1) / L;
        }
    }

    // beyond what the kernels' 32-bit grids (scatter: tiles * chunks * batch workgroups; the others: 256 items per
    // workgroup) and chunk indices cover
    bool too_large() const
    {
        const size_t lim = kMaxGroups;
        if (D > lim || M > lim || batch > lim) return true;
        if (batch > lim / nchunk / ntile) return true;      // scatter; reduce and combine have at most M/256 per tile
        return batch * D / 256 >= lim;                      // record kernel
    }

    int init()
    {
        if (scheme < 0 || D < 2 || M < 2 || batch == 0) return NFT_EC_INVALID_ARGUMENT;
        if (scheme >= 1 && scheme <= 4 && D <= 2) return NFT_EC_INVALID_ARGUMENT;   // fnft__misc.c:331-332
        if (too_large()) return NFT_EC_NOT_YET_IMPLEMENTED;
        std::complex<double> w[16];
        shift = nft_slow_weights(scheme, w);
        if (shift != 0.0 && D >= (size_t)kSlowDirectBelow) {   // shorter signals: the prep kernel sums the shifts directly
            if (nft_tree_too_large(2 * D, 2)) return NFT_EC_NOT_YET_IMPLEMENTED;   // the limit of 4SPLIT4B's tree plan, kept
            const int rc = rs.init(mem, D, batch);
            if (rc != NFT_SUCCESS) return rc;
            if (!tw.init(mem)) return NFT_EC_NOMEM;   // last: the upload waits for the cleared status word
            resample = true;
        }
        bool ok = mem.get(wtab, 16) && mem.get(rec, batch * D * per) && mem.get(cm, batch * nchunk * 4 * M)
                  && mem.get(status, batch) && mem.get(warn, batch);
        if (gsize > 1) ok = ok && mem.get(cmr, batch * groups(nchunk) * 4 * M);
        if (o.richardson) ok = ok && mem.get(rec2, batch * D2 * per) && mem.get(cm2, batch * nchunk2 * 4 * M);
        if (o.richardson && gsize > 1) ok = ok && mem.get(cmr2, batch * groups(nchunk2) * 4 * M);
        if (!ok) return NFT_EC_NOMEM;
        be.h2d(wtab, w, sizeof(w));
        return NFT_SUCCESS;
    }

    size_t groups(size_t nc) const { return (nc + gsize - 1) / gsize; }

    // the workspace back before the plan goes out of scope (the destructor does the same); init() again before reuse
    void destroy() { resample = false; mem.clear(); }

    size_t workspace_bytes() const { return mem.bytes; }

    // records and chunk maps of one pass: Dk kept grid points, every nskip-th sample, interval Tk
    int pass(SlowParams P, const cplx *d_q, size_t Dk, size_t nskip, const double Tk[2], double eps_in, bool first,
             cplx *rec_k, cplx *cm_k, size_t nchunk_k, cplx *cmr_k)
    {
        if (resample) {
            ResampleParams R;
            const int rc = rs.run(d_q, shift * (double)nskip / (double)D, warn, 1, first, R);
            if (rc != NFT_SUCCESS) return rc;
            P.Q12 = rs.Q12;
        }
        P.dsteps = shift * (double)nskip;
        P.rec = rec_k;
        P.Dsub = (long long)Dk;
        P.nskip = (long long)nskip;
        P.srec = (long long)(Dk * per);
        P.eps = (Tk[1] - Tk[0]) / (double)(Dk - 1);
        P.eps_fd = eps_in * (double)nskip;
        P.nchunk = (int)nchunk_k;
        P.cm = cm_k;
        be.template run<KSlowPrep>((int)((batch * Dk + 255) / 256), 1, P);
        if (!dispatch_slow_scatter(be, (int)(ntile * nchunk_k * batch), P, fam, realk)) return NFT_EC_NOT_YET_IMPLEMENTED;
        if (cmr_k) {
            P.cmr = cmr_k;
            P.gsize = (int)gsize;
            P.ngroup = (int)groups(nchunk_k);
            be.template run<KSlowReduce>((int)((batch * groups(nchunk_k) * M + 255) / 256), 1, P);
        }
        return NFT_SUCCESS;
    }

    // phase factors of rho, a, b (fnft__nse_discretization.c:240-375 with boundary_coeff 1/2)
    static void phase_factors(const double Tk[2], double eps, double *pf)
    {
        pf[0] = -2.0 * (Tk[1] + eps * 0.5);
        pf[1] = (Tk[1] + eps * 0.5) - (Tk[0] - eps * 0.5);
        pf[2] = -(Tk[1] + eps * 0.5) - (Tk[0] - eps * 0.5);
    }

    // enqueues everything; waits for nothing
    int run(const cplx *d_q, const double T[2], cplx *d_out, const double XI[2], int kappa)
    {
        const double eps_t = (T[1] - T[0]) / (double)(D - 1);
        be.memset0(status, batch * sizeof(int));
        be.memset0(warn, batch * sizeof(int));
        SlowParams P;
        std::memset(&P, 0, sizeof(P));
        P.q = d_q;
        P.wtab = wtab;
        P.D = (long long)D;
        P.batch = (int)batch;
        P.kappa = kappa;
        P.scheme = scheme;
        P.npos = ups;
        P.M = (long long)M;
        P.xi0 = XI[0];
        P.dxi = (XI[1] - XI[0]) / (double)(M - 1);
        P.L = (long long)L;
        P.ntile = (int)ntile;
        int rc = pass(P, d_q, D, 1, T, eps_t, true, rec, cm, nchunk, cmr);
        if (rc != NFT_SUCCESS) return rc;
        phase_factors(T, eps_t, P.pf);
        if (o.richardson) {
            double Tsub[2] = {T[0], 0.0}, eps_sub;
            nft_sub_interval(T, D, D2, nskip2, &Tsub[1], &eps_sub);
            rc = pass(P, d_q, D2, nskip2, Tsub, eps_t, false, rec2, cm2, nchunk2, cmr2);
            if (rc != NFT_SUCCESS) return rc;
            phase_factors(Tsub, eps_sub, P.pf2);
            P.cm2 = cmr2 ? cmr2 : cm2;
            P.nchunk2 = (int)(cmr2 ? groups(nchunk2) : nchunk2);
            P.scl_num = std::pow(eps_sub / eps_t, (double)nft_slow_order(scheme));
            P.scl_den = P.scl_num - 1.0;
            P.xi_lim = 0.9 * 3.14159265358979323846 / (2.0 * eps_sub);
        }
        P.cm = cmr ? cmr : cm;
        P.nchunk = (int)(cmr ? groups(nchunk) : nchunk);
        P.cstype = o.cstype;
        P.out = d_out;
        P.status = status;
        be.template run<KSlowCombine>((int)((batch * M + 255) / 256), 1, P);
        return NFT_SUCCESS;
    }

    // waits for the stream; st: bit 0 a(xi) == 0, wn: bit 2 the resampler's "not band-limited"
    int read(std::vector<int> &st, std::vector<int> &wn)
    {
        st.assign(batch, 0);
        wn.assign(batch, 0);
        be.d2h(st.data(), status, batch * sizeof(int));
        be.d2h(wn.data(), warn, batch * sizeof(int));
        return be.sync();
    }
};
