// emu_discspec_search.cpp -- the guess-free batched discrete spectrum (fnft_amd/csrc/nft_discspec_search.h and the
// body_aberthb_* / body_ds_candidates kernels) in the CPU lane emulator (TEST INFRASTRUCTURE ONLY, its own shared
// object; see emu_backend.h).
#include "emu_backend.h"

thread_local fa_emu_ctx *fa_emu = nullptr;

#include "../../fnft_amd/csrc/nft_discspec_search.h"

template <class BE>
static int run_search(size_t D, size_t K, size_t batch, const NftDsOpts &o, const cplx *q, const double *T, cplx *bound_states,
                      cplx *normconsts, unsigned long long *K_out, int *status, int *warn, size_t *sizes)
{
    BE be;
    NftDiscSpecSearch<BE> ds(be, D, K, batch, o);
    int rc = ds.init();
    if (rc == NFT_SUCCESS) rc = ds.run(q, T, bound_states, normconsts, K_out);
    if (rc == NFT_SUCCESS) {
        std::vector<int> st, wn;
        std::vector<unsigned long long> ko;
        rc = ds.read(st, ko, wn, K_out);
        for (size_t b = 0; b < batch; b++) { status[b] = st[b]; warn[b] = wn[b]; }
    }
    if (sizes) { sizes[0] = ds.Dsub; sizes[1] = ds.n; sizes[2] = (size_t)ds.S; }
    return rc;
}

extern "C" {

// every array in host memory; status: the device status words (NftDiscSpecBatch's bits, bit 3: root finder failed),
// warn: bit 0 truncated to K, bit 1 sweep limit; sizes (may be NULL): {Dsub, roots per signal, segments}
// segmented != 0: several segments per sweep (the emulator's kTargetWorkgroups), else one
int emu_discspec_search(size_t D, size_t K, size_t batch, int nse_disc, int bsloc, size_t niter, size_t Dsub, int bsfilt,
                        int dstype, int segmented, const cplx *q, const double *T, cplx *bound_states, cplx *normconsts,
                        unsigned long long *K_out, int *status, int *warn, size_t *sizes)
{
    NftDsOpts o;
    o.bsfilt = bsfilt; o.bsloc = bsloc; o.niter = niter; o.Dsub = Dsub; o.dstype = dstype; o.nse_disc = nse_disc;
    o.richardson = 0;
    if (segmented)
        return run_search<EmuBackend>(D, K, batch, o, q, T, bound_states, normconsts, K_out, status, warn, sizes);
    return run_search<EmuBackendOneSegment>(D, K, batch, o, q, T, bound_states, normconsts, K_out, status, warn, sizes);
}

// the root finder alone on caller-supplied polynomials: entry 11 of signal b (n + 1 coefficients, highest power first)
// at tm + b*4*(n + 1).  z: batch*n roots; per signal, as fnft_amd__aberthb_roots of hip_backend.hip reports them: mdeg,
// the degree the iteration ran on (without zero end coefficients), the status word (bit 3: not converged), the warning
// word (bit 1: sweep limit) and the sweeps of its AbState; sizes (may be NULL): {segments of the plan}
int emu_aberthb_roots(size_t n, size_t batch, const cplx *tm, cplx *z, int *mdeg, int *status, int *warn, int *sweeps,
                      size_t *sizes)
{
    EmuBackend be;
    NftDsOpts o;
    o.bsfilt = 2; o.bsloc = 0; o.niter = 0; o.Dsub = 0; o.dstype = 0; o.nse_disc = 4; o.richardson = 0;   // 2SPLIT2A: n = D
    NftDiscSpecSearch<EmuBackend> ds(be, n, 1, batch, o);
    int rc = ds.init();
    if (rc != NFT_SUCCESS) return rc;
    be.memset0(ds.sstatus, batch * sizeof(int));
    be.memset0(ds.warn, batch * sizeof(int));
    ds.roots(tm);
    for (size_t b = 0; b < batch; b++) {
        const AbState &s = ds.A.state[b];
        std::memcpy(z + b * n, ds.A.zbuf[s.zin] + b * n, n * sizeof(cplx));
        mdeg[b] = s.m;
        status[b] = ds.sstatus[b];
        warn[b] = ds.warn[b];
        sweeps[b] = s.sweeps;
    }
    if (sizes) sizes[0] = (size_t)ds.S;
    return rc;
}

// LDS bytes of the new kernels
size_t emu_discspec_search_lds_bytes(int which)
{
    switch (which) {
    case 0: return KAberthBStart::lds_bytes();
    case 1: return KAberthBNewton::lds_bytes();
    case 2: return KAberthBSum::lds_bytes();
    default: return KDsCandidates::lds_bytes();
    }
}

}  // extern "C"

#ifdef EMU_SEARCH_MAIN
// stand-alone run (host sanitizers): two sech pulses, SUBSAMPLE_AND_REFINE under 2SPLIT2A
#include <cstdio>
int main()
{
    const size_t D = 64, K = 4, B = 2;
    std::vector<cplx> q(B * D), bs(B * K), nc(B * 2 * K);
    std::vector<unsigned long long> ko(B);
    std::vector<int> st(B), wn(B);
    const double T[2] = {-10.0, 10.0};
    for (size_t b = 0; b < B; b++)
        for (size_t i = 0; i < D; i++) {
            const double t = T[0] + (T[1] - T[0]) * (double)i / (double)(D - 1);
            q[b * D + i] = cmake(0.0, (1.2 + (double)b) / std::cosh(t));
        }
    size_t sz[3];
    const int rc = emu_discspec_search(D, K, B, 4, 2, 10, 0, 2, 2, 1, q.data(), T, bs.data(), nc.data(), ko.data(), st.data(),
                                       wn.data(), sz);
    std::printf("rc %d Dsub %zu roots %zu S %zu\n", rc, sz[0], sz[1], sz[2]);
    for (size_t b = 0; b < B; b++) {
        std::printf("signal %zu: K_out %llu status %d warn %d:", b, ko[b], st[b], wn[b]);
        for (size_t i = 0; i < ko[b] && i < K; i++) std::printf(" (%.12g, %.12g)", bs[b * K + i].x, bs[b * K + i].y);
        std::printf("\n");
    }
    return (rc == 0 && ko[0] == 1 && ko[1] == 2) ? 0 : 1;
}
#endif
