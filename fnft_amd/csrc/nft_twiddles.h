// nft_twiddles.h -- the twiddle tables of every transform (product tree, chirp z-transform, any-length DFT, layer
// peeling's products), as a part of its own: the outermost host class owns one set, allocated from ITS arena, and every
// part and tree inside it borrows the set as `const NftTwiddles &`.  The host copies are computed once per process.
#pragma once
#include <cmath>
#include <vector>

#include "nft_arena.h"
#include "nft_dispatch.h"

inline size_t nft_nextpow2(size_t n)
{
    size_t r = 1;
    while (r < n) r *= 2;
    return r;
}
inline int nft_log2(size_t n)
{
    int l = 0;
    while (((size_t)1 << l) < n) l++;
    return l;
}

constexpr int kFineLog2 = 12;           // master twiddle: NMAX = 2^24
constexpr int kMaxTwTable = 16384;      // per-length tables up to this length (longest column transform; the real path's
                                        // quarter-step tables of 4*N1 entries)
// fine tables of the two master twiddle pairs: 2^12 entries exp(-2 pi i j/2^24), then 2^13 entries exp(-2 pi i j/2^26)
constexpr size_t kTwLoEntries = ((size_t)1 << kFineLog2) + ((size_t)1 << (kFineLog2 + 1));
constexpr int kTw3MaxLog = 12;

template <class BE> class NftTwiddles {
public:
    cplx *twtab = nullptr;   // concatenated tables for N = 2,4,...,kMaxTwTable
    cplx *twlo = nullptr;    // exp(-2 pi i j / 2^24), j < 4096
    // lengths 3*2^b (column transforms of the real path, nft_real.h): tables for L = 3, 6, ..., 3*2^kTw3MaxLog back to
    // back (offset L - 3), and the fine table exp(-2 pi i j/(3*2^22)), j < 4096, of the master pair for 3*2^22
    cplx *tw3tab = nullptr, *twlo3 = nullptr;

    // the tables from the owner's arena, uploaded; with3: the lengths 3*2^b too (KdV).  false: no memory
    bool init(DevArena<BE> &mem, bool with3 = false)
    {
        bool ok = mem.get(twtab, (size_t)2 * kMaxTwTable) && mem.get(twlo, kTwLoEntries);
        if (with3) ok = ok && mem.get(tw3tab, (size_t)3 << (kTw3MaxLog + 1)) && mem.get(twlo3, (size_t)1 << kFineLog2);
        if (!ok) return false;
        const HostTables &H = host_tables();
        mem.be.h2d(twtab, H.tw.data(), H.tw.size() * sizeof(cplx));
        mem.be.h2d(twlo, H.lo.data(), H.lo.size() * sizeof(cplx));
        if (with3) {
            mem.be.h2d(tw3tab, H.tw3.data(), H.tw3.size() * sizeof(cplx));
            mem.be.h2d(twlo3, H.lo3.data(), H.lo3.size() * sizeof(cplx));
        }
        return true;
    }
    bool ready() const { return twtab != nullptr; }

    const cplx *tw_table(size_t N) const
    {   // tables are stored back to back: N=2 at offset 0, N=4 at 2, N=8 at 6, ... offset = N-2
        return twtab + (N - 2);
    }
    const cplx *tw3_table(size_t L) const { return tw3tab + (L - 3); }
    BigTwiddle big_tw3(size_t N) const   // N = 3*2^a <= 3*2^22
    {
        BigTwiddle t;
        t.hi = tw3_table((size_t)3 << 10);   // exp(-2 pi i jh/3072)
        t.lo = twlo3;
        t.fine_log2 = kFineLog2;
        t.shift = 22 - nft_log2(N / 3);
        return t;
    }
    BigTwiddle big_tw(size_t N) const
    {
        BigTwiddle t;
        if (N > ((size_t)1 << (2 * kFineLog2))) {   // 2^24 < N <= 2^26: the pair with 2^13-entry tables
            t.hi = tw_table((size_t)1 << (kFineLog2 + 1));
            t.lo = twlo + ((size_t)1 << kFineLog2);
            t.fine_log2 = kFineLog2 + 1;
            t.shift = 2 * (kFineLog2 + 1) - nft_log2(N);
            return t;
        }
        t.hi = tw_table((size_t)1 << kFineLog2);   // exp(-2 pi i jh / 2^FINE)
        t.lo = twlo;
        t.fine_log2 = kFineLog2;
        t.shift = 2 * kFineLog2 - nft_log2(N);
        return t;
    }

    // host copies of the tables, computed once per process (long-double sines: ~2 ms per plan otherwise)
    struct HostTables {
        std::vector<cplx> tw, lo, tw3, lo3;
        HostTables()
        {
            const long double tau = 6.283185307179586476925286766559005768L;
            tw.resize((size_t)2 * kMaxTwTable);
            for (size_t N = 2; N <= (size_t)kMaxTwTable; N *= 2)
                for (size_t j = 0; j < N; j++) {
                    const long double a = -tau * (long double)j / (long double)N;
                    tw[N - 2 + j] = cmake((double)cosl(a), (double)sinl(a));
                }
            lo.resize(kTwLoEntries);
            const long double nmax = (long double)((size_t)1 << (2 * kFineLog2));
            for (size_t j = 0; j < ((size_t)1 << kFineLog2); j++) {
                const long double a = -tau * (long double)j / nmax;
                lo[j] = cmake((double)cosl(a), (double)sinl(a));
            }
            for (size_t j = 0; j < ((size_t)1 << (kFineLog2 + 1)); j++) {
                const long double a = -tau * (long double)j / (4.0L * nmax);
                lo[((size_t)1 << kFineLog2) + j] = cmake((double)cosl(a), (double)sinl(a));
            }
            tw3.resize((size_t)3 << (kTw3MaxLog + 1));
            for (int b = 0; b <= kTw3MaxLog; b++) {
                const size_t Lb = (size_t)3 << b;
                for (size_t j = 0; j < Lb; j++) {
                    const long double a = -tau * (long double)j / (long double)Lb;
                    tw3[Lb - 3 + j] = cmake((double)cosl(a), (double)sinl(a));
                }
            }
            lo3.resize((size_t)1 << kFineLog2);
            const long double nmax3 = 3.0L * (long double)((size_t)1 << 22);
            for (size_t j = 0; j < lo3.size(); j++) {
                const long double a = -tau * (long double)j / nmax3;
                lo3[j] = cmake((double)cosl(a), (double)sinl(a));
            }
        }
    };
    static const HostTables &host_tables()
    {
        static const HostTables t;
        return t;
    }
};
