// emu_main.cpp -- builds tests/emu/libfnft_emu.so: the kernel bodies of fnft_amd/csrc compiled
// for the CPU lane emulator (TEST INFRASTRUCTURE ONLY; see emu_backend.h).
#include "emu_backend.h"

thread_local fa_emu_ctx *fa_emu = nullptr;

#include "../../fnft_amd/csrc/nft_api.h"
#include "../../fnft_amd/csrc/nft_discspec.h"

// ---- stand-alone checks of fft_wg in every tiling the kernels use -----------------------------
struct FftTestParams {
    const cplx *in;   // B sequences of N, sequence c at in[c*N + idx]
    cplx *out;
    const cplx *tw;
    int sign;
};
template <int N, int R, int B, bool DB, int T> struct KFftTest {
    using Params = FftTestParams;
    static constexpr int THREADS = T;
    static constexpr size_t lds_bytes() { return (N > R) ? (size_t)(DB ? 2 : 1) * N * B * sizeof(cplx) : 0; }
    static void body(const Params &p)
    {
        cplx *lds = (cplx *)FA_LDS_PTR;
        const int tid = FA_TID;
        const int c = tid % B, v = tid / B;
        cplx x[R];
        for (int i = 0; i < R; i++) x[i] = p.in[(size_t)c * N + v + (N / R) * i];
        int parity = 0;
        // two transforms back to back exercise the buffer-parity hand-over
        if (p.sign < 0) {
            fft_wg<N, R, B, -1, DB>(x, lds, v, c, p.tw, parity);
        } else {
            fft_wg<N, R, B, -1, DB>(x, lds, v, c, p.tw, parity);
            fft_wg<N, R, B, +1, DB>(x, lds, v, c, p.tw, parity);
        }
        for (int i = 0; i < R; i++) p.out[(size_t)c * N + v + (N / R) * i] = x[i];
    }
};

static std::vector<cplx> host_tw(size_t N)
{
    std::vector<cplx> t(N);
    const long double tau = 6.283185307179586476925286766559005768L;
    for (size_t j = 0; j < N; j++) {
        const long double a = -tau * (long double)j / (long double)N;
        t[j] = cmake((double)cosl(a), (double)sinl(a));
    }
    return t;
}

template <int N> static int fft_pair_cfg(int sign, const cplx *in, cplx *out)
{
    EmuBackend be;
    using C = PairCfg<N>;
    auto tw = host_tw(N);
    FftTestParams p{in, out, tw.data(), sign};
    be.run<KFftTest<N, C::R, C::B, true, C::THREADS>>(1, 1, p);
    return C::B;
}
template <int N1> static int fft_col_cfg(int sign, const cplx *in, cplx *out)
{
    EmuBackend be;
    using C = ColCfg<N1>;
    auto tw = host_tw(N1);
    FftTestParams p{in, out, tw.data(), sign};
    be.run<KFftTest<N1, C::R, C::BC, C::DB, C::THREADS>>(1, 1, p);
    return C::BC;
}

extern "C" {

// returns the batch size B of the configuration (0: not instantiated); if in == NULL only reports B
int emu_fft_pair_cfg(int N, int sign, const cplx *in, cplx *out)
{
    switch (N) {
#define X(n) case n: return in ? fft_pair_cfg<n>(sign, in, out) : PairCfg<n>::B;
        X(8) X(16) X(32) X(64) X(128) X(256) X(512) X(1024) X(2048) X(4096)
#undef X
    default: return 0;
    }
}
int emu_fft_col_cfg(int N1, int sign, const cplx *in, cplx *out)
{
    switch (N1) {
#define X(n) case n: return in ? fft_col_cfg<n>(sign, in, out) : ColCfg<n>::BC;
        FA_FOR_EACH_N1(X)
#undef X
    default: return 0;
    }
}

int emu_poly_fmult2x2(size_t *d, size_t n, std::complex<double> *p, std::complex<double> *result,
                      int32_t *W_ptr)
{
    EmuBackend be;
    return api_poly_fmult2x2(be, d, n, p, result, W_ptr);
}

int emu_akns_fscatter(size_t D, const std::complex<double> *q, const std::complex<double> *r,
                      double eps_t, int kappa, std::complex<double> *result, size_t *deg_ptr,
                      int32_t *W_ptr, int akns_disc)
{
    EmuBackend be;
    return api_akns_fscatter(be, D, q, r, eps_t, kappa, result, deg_ptr, W_ptr, akns_disc);
}

int emu_poly_chirpz(size_t deg, const std::complex<double> *p, const double *A, const double *W,
                    size_t M, std::complex<double> *result)
{
    EmuBackend be;
    return NftPlan<EmuBackend>::chirpz_host(be, deg, p, {A[0], A[1]}, {W[0], W[1]}, M, result);
}

// fnft_nsev continuous spectrum, host buffers
int emu_nsev_contspec(size_t D, const std::complex<double> *q, const double *T, size_t M,
                      std::complex<double> *contspec, const double *XI, int kappa, int nse_disc,
                      int cstype, int normalization_flag)
{
    EmuBackend be;
    const int akns = nft_nse_to_akns(nse_disc);
    if (akns < 0) return NFT_EC_INVALID_ARGUMENT;
    const int ups = nft_nse_upsampling(nse_disc);
    NftPlan<EmuBackend> pl(be, (size_t)ups * D, M, 1, akns, nft_akns_degree(akns));
    pl.set_front(D, 1, ups);
    int rc = pl.init();
    if (rc != NFT_SUCCESS) return rc;
    const size_t cs_len = M * (cstype == 0 ? 1 : (cstype == 1 ? 2 : 3));
    cplx *dq = (cplx *)be.alloc(D * sizeof(cplx));
    cplx *dcs = (cplx *)be.alloc(cs_len * sizeof(cplx));
    be.h2d(dq, q, D * sizeof(cplx));
    double Tsub[2];
    rc = pl.run_front(dq, T, kappa, Tsub);
    if (rc == NFT_SUCCESS) rc = pl.run_tree();
    if (rc == NFT_SUCCESS) {
        NftPlan<EmuBackend>::Contspec cs;
        cs.T[0] = Tsub[0]; cs.T[1] = Tsub[1]; cs.XI[0] = XI[0]; cs.XI[1] = XI[1];
        cs.nse_disc = nse_disc; cs.cstype = cstype; cs.normalization_flag = normalization_flag;
        rc = pl.run_contspec(dcs, cs);
    }
    if (rc == NFT_SUCCESS) rc = pl.read_status();
    if (rc == NFT_SUCCESS) be.d2h(contspec, dcs, cs_len * sizeof(cplx));
    be.free(dq);
    be.free(dcs);
    return rc;
}

// fnft_kdvv reflection coefficient, host buffers (kdv_disc 0..17)
// real != 0: the real-coefficient path (nft_real.h; u must be real)
int emu_kdvv_contspec(size_t D, const std::complex<double> *u, const double *T, size_t M,
                      std::complex<double> *contspec, const double *XI, int kdv_disc, int real)
{
    EmuBackend be;
    const int akns = kdv_disc + 1;
    NftPlan<EmuBackend> pl(be, D, M, 1, akns, nft_akns_degree(akns));
    pl.kdv = true;
    pl.want_real = real != 0;
    int rc = pl.init();
    if (rc != NFT_SUCCESS) return rc;
    cplx *du = (cplx *)be.alloc(D * sizeof(cplx));
    cplx *dcs = (cplx *)be.alloc(M * sizeof(cplx));
    be.h2d(du, u, D * sizeof(cplx));
    double Tsub[2];
    rc = pl.run_front(du, T, 1, Tsub);
    if (rc == NFT_SUCCESS) rc = pl.run_tree();
    if (rc == NFT_SUCCESS) rc = pl.run_contspec_kdv(dcs, T, XI, kdv_disc == 2);
    if (rc == NFT_SUCCESS) rc = pl.read_status();
    if (rc == NFT_SUCCESS) be.d2h(contspec, dcs, M * sizeof(cplx));
    be.free(du);
    be.free(dcs);
    return rc;
}

// discrete spectrum of fnft_nsev, host buffers (capacity *K_ptr in, count out)
int emu_nsev_discspec(size_t D, const std::complex<double> *q, const double *T, int bsfilt, int bsloc,
                      size_t niter, size_t Dsub, int dstype, int nse_disc, int richardson, size_t *K_ptr,
                      std::complex<double> *bound_states, std::complex<double> *nc)
{
    EmuBackend be;
    NftDiscSpec<EmuBackend> ds(be);
    NftDsOpts o;
    o.bsfilt = bsfilt; o.bsloc = bsloc; o.niter = niter; o.Dsub = Dsub; o.dstype = dstype;
    o.nse_disc = nse_disc; o.richardson = richardson;
    return ds.run(D, q, T, o, K_ptr, bound_states, nc);
}

// all roots of a polynomial (fnft__poly_roots_fasteigen seam): the Ehrlich-Aberth kernels in the emulator.
// *last_corr: largest relative correction of the last sweep
int emu_poly_roots(size_t deg, const std::complex<double> *p, std::complex<double> *roots, double *last_corr)
{
    EmuBackend be;
    NftDiscSpec<EmuBackend> ds(be);
    cplx *d_coef = (cplx *)be.alloc((deg + 1) * sizeof(cplx));
    be.h2d(d_coef, p, (deg + 1) * sizeof(cplx));
    std::vector<std::complex<double>> z;
    const int rc = ds.roots(d_coef, deg, z);
    be.free(d_coef);
    if (last_corr) *last_corr = ds.last_root_corr;
    for (size_t i = 0; i < z.size() && i < deg; i++) roots[i] = z[i];
    return rc;
}

// Schedule of the product tree without executing it (schedule-only mode of EmuBackend): the names of every kernel
// the plan launches, '\n'-separated, into out[cap].  Returns the plan's rc, or -1 if out is too small.
//   entry 0: fnft__poly_fmult2x2, D matrices of degree `disc` (general form)
//   entry 1: fnft_amd_plan / fnft_nsev, D samples per signal, `batch` signals, nse discretization `disc`
//   entry 2: fnft__akns_fscatter with an explicit r (general form), akns discretization `disc`
//   entry 3: fnft__kdv_fscatter, kdv discretization `disc`; real != 0: a real potential (real-coefficient tree)
int emu_tree_schedule(int entry, size_t D, int disc, size_t batch, int real, char *out, size_t cap)
{
    EmuBackend be;
    std::vector<std::string> names;
    emu_schedule = &names;
    int akns = -1, deg0 = disc, ups = 1;
    size_t Dtree = D;
    if (entry == 1) {
        akns = nft_nse_to_akns(disc);
        ups = nft_nse_upsampling(disc);
        Dtree = (ups == 1) ? D : 2 * nft_sub_count(D, 1);
    } else if (entry == 2) {
        akns = disc;
    } else if (entry == 3) {
        akns = disc + 1;
    }
    if (entry != 0) deg0 = akns >= 0 ? nft_akns_degree(akns) : 0;
    int rc = NFT_EC_INVALID_ARGUMENT;
    if (deg0 > 0 && D > 0 && batch > 0) {
        NftPlan<EmuBackend> pl(be, Dtree, 0, entry == 1 ? batch : 1, akns, deg0);
        if (entry == 1) pl.set_front(D, 1, ups);
        pl.kdv = entry == 3;
        pl.want_real = entry == 3 && real != 0;
        rc = pl.init();
        // any non-null address: the kernels that would read it are not executed
        cplx *dummy = (cplx *)be.alloc(16);
        const double T[2] = {-1.0, 1.0};
        double Tsub[2];
        if (rc == NFT_SUCCESS) {
            switch (entry) {
            case 0: rc = pl.load_level0_from_device(dummy); break;
            case 1: rc = pl.run_front(dummy, T, 1, Tsub); break;
            case 2: rc = pl.run_coeffs(dummy, dummy, 1e-3, 1); break;
            case 3: rc = pl.run_coeffs(dummy, pl.rneg, 1e-3, 1); break;
            default: rc = NFT_EC_INVALID_ARGUMENT;
            }
        }
        if (rc == NFT_SUCCESS) rc = pl.run_tree();
        if (rc == NFT_SUCCESS) pl.export_tm();
        be.free(dummy);
    }
    emu_schedule = nullptr;
    std::string s;
    for (const auto &n : names) s += n + "\n";
    if (s.size() + 1 > cap) return -1;
    std::memcpy(out, s.c_str(), s.size() + 1);
    return rc;
}

// Schedule of the chirp z-transform entry points without executing them (schedule-only mode, as emu_tree_schedule):
// the names of every kernel launched, '\n'-separated, into out[cap].  Returns the entry's rc, or -1 if out is too small.
//   entry 0: fnft__poly_chirpz, a polynomial of degree n, M outputs (chirpz_host)
//   entry 1: fnft__misc_resample, n samples (resample_host)
//   entry 2: fnft_amd_plan / fnft_nsev, n samples per signal, `batch` signals, nse discretization `disc`, M points,
//            contspec type `cstype` (run_front, run_tree, run_contspec)
//   entry 3: fnft_amd_nsev_contspec_from_tm_device on a plan of n samples (run_contspec_tm)
//   entry 4: fnft_amd_kdvv_contspec_device, kdv discretization `disc`; real != 0: the real-coefficient tree
//            (run_front, run_tree, run_contspec_kdv)
int emu_chirp_schedule(int entry, size_t n, size_t M, int disc, size_t batch, int cstype, int real, char *out,
                       size_t cap)
{
    EmuBackend be;
    using P = NftPlan<EmuBackend>;
    std::vector<std::string> names;
    emu_schedule = &names;
    int rc = NFT_EC_INVALID_ARGUMENT;
    const double T[2] = {-1.0, 1.0}, XI[2] = {-0.5, 0.7};
    // any non-null address: the kernels that would read or write it are not executed (calloc maps lazily)
    cplx *dummy = (cplx *)be.alloc(16);
    if (entry == 0 && M > 0) {
        std::complex<double> *p = (std::complex<double> *)std::calloc(n + 1, sizeof(cplx));
        rc = p ? P::chirpz_host(be, n, p, {1.0, 0.0}, {std::cos(1e-3), std::sin(1e-3)}, M, nullptr, dummy)
               : NFT_EC_NOMEM;
        std::free(p);
    } else if (entry == 1 && n > 2) {
        std::complex<double> *q = (std::complex<double> *)std::calloc(2 * n, sizeof(cplx));
        rc = q ? P::resample_host(be, n, 0.1, q, 0.03, q + n) : NFT_EC_NOMEM;
        std::free(q);
    } else if ((entry == 2 || entry == 3) && n > 1 && M > 0 && batch > 0) {
        const int akns = nft_nse_to_akns(disc);
        const int ups = nft_nse_upsampling(disc);
        if (akns >= 0) {
            const size_t Dtree = (ups == 1) ? n : 2 * nft_sub_count(n, 1);
            P pl(be, Dtree, M, batch, akns, nft_akns_degree(akns));
            pl.set_front(n, 1, ups);
            rc = pl.init();
            double Tsub[2];
            P::Contspec cs;
            cs.XI[0] = XI[0]; cs.XI[1] = XI[1];
            cs.nse_disc = disc; cs.cstype = cstype; cs.normalization_flag = 1;
            if (entry == 2) {
                if (rc == NFT_SUCCESS) rc = pl.run_front(dummy, T, 1, Tsub);
                if (rc == NFT_SUCCESS) rc = pl.run_tree();
                cs.T[0] = Tsub[0]; cs.T[1] = Tsub[1];
                if (rc == NFT_SUCCESS) rc = pl.run_contspec(dummy, cs);
            } else {
                cs.T[0] = T[0]; cs.T[1] = T[1];
                if (rc == NFT_SUCCESS) rc = pl.run_contspec_tm(dummy, cs, dummy, 3);
            }
        }
    } else if (entry == 4 && n > 1 && M > 0 && batch > 0 && disc >= 0) {
        const int akns = disc + 1;
        P pl(be, n, M, batch, akns, nft_akns_degree(akns));
        pl.kdv = true;
        pl.want_real = real != 0;
        rc = pl.init();
        double Tsub[2];
        if (rc == NFT_SUCCESS) rc = pl.run_front(dummy, T, 1, Tsub);
        if (rc == NFT_SUCCESS) rc = pl.run_tree();
        if (rc == NFT_SUCCESS) rc = pl.run_contspec_kdv(dummy, T, XI, disc == 2);
    }
    be.free(dummy);
    emu_schedule = nullptr;
    std::string s;
    for (const auto &nm : names) s += nm + "\n";
    if (s.size() + 1 > cap) return -1;
    std::memcpy(out, s.c_str(), s.size() + 1);
    return rc;
}

// Every kernel instantiation of the library (the units of fnft_amd/csrc/nft_kernel_list.h, which the hip_kernels_*.hip
// files instantiate and the dispatch switches read), named as the schedules above name them, '\n'-separated, into
// out[cap].  Returns the number of names, or -1 if out is too small.
int emu_kernel_list(char *out, size_t cap)
{
    std::string s;
    int n = 0;
#define FA_EMU_NAME(...) s += emu_kernel_name<__VA_ARGS__>() + "\n"; n++;
    FA_ALL_UNITS(FA_EMU_NAME)
#undef FA_EMU_NAME
    if (s.size() + 1 > cap) return -1;
    std::memcpy(out, s.c_str(), s.size() + 1);
    return n;
}

}  // extern "C"
