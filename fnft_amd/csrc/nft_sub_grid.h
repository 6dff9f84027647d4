// nft_sub_grid.h -- the subsampled grid of fnft__nse_discretization_preprocess_signal (fnft__nse_discretization.c:
// 419-430), stated once for every pass over every nskip-th sample (SUBSAMPLE_AND_REFINE, the coarse passes of the
// Richardson extrapolation): a fine and a coarse pass agree about the grid because both ask here.  No dependency beyond
// <cmath>; the C drivers (fnft_nsev_host.c, fnft_nsep_host.c) keep their transcriptions of the reference.
#pragma once
#include <cmath>
#include <cstddef>

// samples kept when every nskip-th of D is used (also: the stride that comes closest to Dsub kept samples)
inline size_t nft_sub_count(size_t D, size_t nskip) { return (size_t)std::llround((double)D / (double)nskip); }

struct NftSubGrid { size_t Dsub, nskip; };
// Dsub_wish clamped to [2, D], the stride nearest to it, and the samples that stride keeps
inline NftSubGrid nft_sub_grid(size_t D, size_t Dsub_wish)
{
    size_t Dsub = Dsub_wish;
    if (Dsub < 2) Dsub = 2;
    if (Dsub > D) Dsub = D;
    const size_t nskip = nft_sub_count(D, Dsub);
    return NftSubGrid{nft_sub_count(D, nskip), nskip};
}

// T: the interval of the D input samples.  *T1: the time of the last kept sample, *eps_sub: the step of the kept ones
inline void nft_sub_interval(const double T[2], size_t D, size_t Dsub, size_t nskip, double *T1, double *eps_sub)
{
    const double eps_in = (T[1] - T[0]) / (double)(D - 1);
    *T1 = T[0] + (double)((Dsub - 1) * nskip) * eps_in;
    *eps_sub = (*T1 - T[0]) / (double)(Dsub - 1);
}
