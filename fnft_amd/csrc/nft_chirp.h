// nft_chirp.h -- the chirp z-transform's launches and the two parts built on them, for whoever needs one: the DFT of any
// length (chirp kernels in DFT mode) and the band-limited resampler (fnft__misc_resample for a batch).  Each part borrows
// the twiddle tables of its owner and takes its workspace from the owner's arena.
//   poly_chirpz      src/private/fnft__poly_chirpz.c:33-105
//   misc_resample    src/private/fnft__misc.c:326-407
#pragma once
#include <complex>
#include <cstring>

#include "nft_twiddles.h"

// return codes (include/fnft_errwarn.h:44-94)
enum {
    NFT_SUCCESS = 0, NFT_EC_NOMEM = 1, NFT_EC_INVALID_ARGUMENT = 2, NFT_EC_DIV_BY_ZERO = 3,
    NFT_EC_OTHER = 5, NFT_EC_NOT_YET_IMPLEMENTED = 6
};

constexpr size_t kMaxSplitChirp = (size_t)kRowChirp * 8192;  // chirp length up to 2^25 (any-length DFTs up to 2^24 points)

// log of a complex number through libm's clog -- the routine glibc's cpow() (which the reference
// calls for every chirp factor, src/private/fnft__poly_chirpz.c:69,77,81,95) is built on.  It keeps
// the tiny real part log|z| of a z that is on the unit circle only up to rounding; the generic
// std::log(std::complex) of some C++ runtimes returns log(hypot) = 0 there, which changes
// |z|^(n^2/2) by up to 1e-9 at n = 2^16.
inline std::complex<double> nft_clog(std::complex<double> z)
{
    __complex__ double zz;
    __real__ zz = z.real();
    __imag__ zz = z.imag();
    const __complex__ double r = __builtin_clog(zz);
    return std::complex<double>(__real__ r, __imag__ r);
}

// smallest chirp length for a transform whose input and output points add up to n: a power of two, two rows at least
inline size_t nft_chirp_len(size_t n)
{
    const size_t L = nft_nextpow2(n);
    return (L < 2 * (size_t)kRowChirp) ? 2 * (size_t)kRowChirp : L;
}

template <class BE> void fill_chirp_geometry(const NftTwiddles<BE> &tw, ChirpParams &C, size_t L)
{
    C.N2 = kRowChirp;
    C.N1 = (int)(L / kRowChirp);
    C.btw = tw.big_tw(L);
    C.tw1 = tw.tw_table((size_t)C.N1);
    C.tw2 = tw.tw_table(kRowChirp);
    C.jobs_per_group = 2;
}

template <class BE> int run_chirp(BE &be, const ChirpParams &C)
{
    if (!dispatch_chirp_col_fwd(be, C)) return NFT_EC_NOT_YET_IMPLEMENTED;
    const int njobs = C.batch * C.npoly;
    be.template run<KChirpRows>(C.N1, (njobs + C.jobs_per_group - 1) / C.jobs_per_group, C);
    if (!dispatch_chirp_col_inv(be, C)) return NFT_EC_NOT_YET_IMPLEMENTED;
    return NFT_SUCCESS;
}

// DFTs of any length up to nmax points, jobs_max at a time: out[k] = sum_j in[j] exp(sign 2 pi i j k / n), un-normalised
// (fft_wrapper_execute_plan), by the chirp kernels in DFT mode
template <class BE> class NftAnyDft {
public:
    BE &be;
    const NftTwiddles<BE> &tw;
    cplx *Y = nullptr, *V = nullptr;
    int *status = nullptr;       // status word of the chirp kernels (DFT mode sets no bit)
    size_t Lcap = 0, jobs = 0;

    NftAnyDft(BE &b, const NftTwiddles<BE> &t) : be(b), tw(t) {}
    static size_t len(size_t n) { return nft_chirp_len(2 * n - 1); }
    // shared_status: the owner's status word (4 ints) instead of one of its own
    int init(DevArena<BE> &mem, size_t nmax, size_t jobs_max, int *shared_status = nullptr)
    {
        const size_t L = len(nmax);
        if (L > kMaxSplitChirp) return NFT_EC_NOT_YET_IMPLEMENTED;
        if (!(mem.get(Y, jobs_max * L) && mem.get(V, L))) return NFT_EC_NOMEM;
        status = shared_status;
        if (!status) {
            if (!mem.get(status, 4)) return NFT_EC_NOMEM;
            be.memset0(status, 4 * sizeof(int));
        }
        Lcap = L; jobs = jobs_max;
        return NFT_SUCCESS;
    }
    // batch * npoly transforms of n points each, back to back in d_in and in d_out
    int dft(const cplx *d_in, cplx *d_out, size_t n, size_t batch, int npoly, int sign)
    {
        const size_t L = len(n);
        if (L > Lcap || batch * (size_t)npoly > jobs) return NFT_EC_OTHER;
        ChirpParams C;
        std::memset(&C, 0, sizeof(C));
        C.poly = d_in; C.deg = (long long)n - 1; C.M = (long long)n;
        C.batch = (int)batch; C.npoly = npoly;
        C.Ybuf = Y; C.Vbuf = V; C.Hbuf = d_out;
        fill_chirp_geometry(tw, C, L);
        C.status = status; C.cstype = -1;
        C.dft_len = (long long)n; C.dft_sign = sign;
        return run_chirp(be, C);
    }
};

// fnft__misc_resample for every signal of a batch and the two shifts -/+ delta: forward DFT, band check, phase ramps,
// inverse DFTs.  Leaves the shifted copies times Din in Q12 (signal b: rows 2b and 2b + 1).
template <class BE> class NftResampler {
public:
    BE &be;
    NftAnyDft<BE> ft;
    size_t Din = 0, batch = 0;
    cplx *X = nullptr, *X12 = nullptr, *Q12 = nullptr;
    NftResampler(BE &b, const NftTwiddles<BE> &t) : be(b), ft(b, t) {}
    int init(DevArena<BE> &mem, size_t Din_, size_t batch_, int *shared_status = nullptr)
    {
        if (Din_ <= 2) return NFT_EC_INVALID_ARGUMENT;   // fnft__misc.c:331-332
        if (NftAnyDft<BE>::len(Din_) > kMaxSplitChirp) return NFT_EC_NOT_YET_IMPLEMENTED;
        Din = Din_; batch = batch_;
        if (!(mem.get(X, batch * Din) && mem.get(X12, batch * 2 * Din) && mem.get(Q12, batch * 2 * Din)))
            return NFT_EC_NOMEM;
        return ft.init(mem, Din, 2 * batch, shared_status);
    }
    // delta_over_span: delta / (Din * eps_t), formed by the caller.  fwd: transform the signal first and check its band
    // (bit 2 of wstat[b * wstride]); without it the spectrum of the last call with the same signal is used again.
    int run(const void *d_q, double delta_over_span, int *wstat, long long wstride, bool fwd, ResampleParams &R)
    {
        if (fwd) {   // forward DFT of every signal (fnft__misc.c:366-370)
            const int rc = ft.dft((const cplx *)d_q, X, Din, batch, 1, -1);
            if (rc != NFT_SUCCESS) return rc;
        }
        // phase ramps for the two shifts (fnft__misc.c:383-393)
        R.X = X; R.X12 = X12; R.Q12 = Q12; R.qpre = nullptr;
        R.Din = (long long)Din; R.Dsub = 0; R.nskip = 1;
        R.batch = (int)batch;
        R.delta_over_span = delta_over_span;
        R.w0 = R.w1 = 0.0;
        R.status = wstat;
        R.sstat = wstride;
        if (fwd) be.template run<KBandCheck>((int)batch, 1, R);     // fnft__misc.c:371-381 (warning only)
        be.template run<KResamplePhase>((int)((batch * Din + 255) / 256), 1, R);
        return ft.dft(X12, Q12, Din, batch, 2, +1);                 // inverse DFTs (:395-399)
    }
    // the front end of 4SPLIT4A/B (fnft__nse_discretization.c:474-503): shifts -/+ sqrt(3)/6 of the kept step (:482-485),
    // then the weighted pairs (:493-499), two samples per kept step into qpre (batch * 2 * Dsub)
    int run_4split4(const void *d_q, size_t nskip, size_t Dsub, cplx *qpre, int *wstat)
    {
        const double scl = std::sqrt(3.0) / 6.0;
        ResampleParams R;
        const int rc = run(d_q, scl * (double)nskip / (double)Din, wstat, 0, true, R);
        if (rc != NFT_SUCCESS) return rc;
        R.qpre = qpre; R.Dsub = (long long)Dsub; R.nskip = (long long)nskip;
        R.w0 = 0.25 + scl; R.w1 = 0.25 - scl;
        be.template run<KResampleCombine>((int)((batch * Dsub + 255) / 256), 1, R);
        return NFT_SUCCESS;
    }
};
