// nft_plan.h -- back-end independent host logic of the fnft_nsev continuous-spectrum path:
// workspace layout in HBM, level schedule of the product tree, chirp z-transform set-up.  The twiddle tables, the chirp
// launches and the resampler of the 4SPLIT4A/B front end are parts of their own (nft_twiddles.h, nft_chirp.h).
//
// Mirrors the control flow of the reference (file:line relative to the FNFT source tree):
//   fnft_nsev_base           src/fnft_nsev.c:458-565
//   nse_fscatter             src/private/fnft__nse_fscatter.c:44-91
//   akns_fscatter            src/private/fnft__akns_fscatter.c:64-925
//   poly_fmult2x2            src/private/fnft__poly_fmult.c:381-546
//   nsev_compute_contspec    src/fnft_nsev.c:744-891
//   poly_chirpz              src/private/fnft__poly_chirpz.c:33-105
//
// BE (back end) supplies device memory, copies, kernel launches and stage timers; see
// hip_backend.hip (product) and tests/emu/emu_backend.h (CPU lane emulator, tests only).
// Every device buffer of a plan comes from its arena `mem` (nft_arena.h) and goes back when the plan is destroyed.
#pragma once
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "nft_chirp.h"
#include "nft_schemes.h"
#include "nft_sub_grid.h"

// fnft__akns_discretization.c:29-67 restricted to what the coefficient kernel implements
inline int nft_akns_degree(int akns_disc)
{
    switch (akns_disc) {
    case 0: case 1: case 2: case 3: case 4: case 5: return 1;   // MODAL,1A,1B,2A,2B,2S
    case 8: case 10: return 2;                                   // 3S, 4B
    case 6: case 7: return 3;                                    // 3A, 3B
    case 9: return 4;                                            // 4A
    case 14: return 6;                                           // 6B
    case 13: case 18: return 12;                                 // 6A, 8B
    case 11: case 12: return 15;                                 // 5A, 5B
    case 17: return 24;                                          // 8A
    case 15: case 16: return 105;                                // 7A, 7B
    default: return 0;
    }
}
// fnft__nse_discretization.c:108-200 (upsampling-factor-1 splitting schemes); -1 otherwise
inline int nft_nse_to_akns(int nse_disc)
{
    switch (nse_disc) {
    case 0: return 0;    // 2SPLIT2_MODAL
    case 2: return 1;    // 2SPLIT1A
    case 3: return 2;    // 2SPLIT1B
    case 4: return 3;    // 2SPLIT2A
    case 5: return 4;    // 2SPLIT2B
    case 6: return 5;    // 2SPLIT2S
    case 7: return 6;    // 2SPLIT3A
    case 8: return 7;    // 2SPLIT3B
    case 9: return 8;    // 2SPLIT3S
    case 10: return 9;   // 2SPLIT4A
    case 11: return 10;  // 2SPLIT4B
    case 12: case 13: case 14: case 15: case 16: case 17: case 18: case 19:
        return nse_disc - 1;   // 2SPLIT5A .. 2SPLIT8B -> akns 11 .. 18
    case 20: return 9;   // 4SPLIT4A: per-sample formulas of 2SPLIT4A (fnft__akns_fscatter.c:362-363)
    case 21: return 10;  // 4SPLIT4B: ... of 2SPLIT4B (:402-403)
    default: return -1;
    }
}

// fnft__akns_discretization.c:114-152: preprocessed samples per step
inline int nft_nse_upsampling(int nse_disc) { return (nse_disc == 20 || nse_disc == 21) ? 2 : 1; }
// fnft__akns_discretization.c:157-192: order used by Richardson extrapolation
inline int nft_nse_method_order(int nse_disc) { return (nse_disc == 20 || nse_disc == 21) ? 4 : 2; }

// transform length used for a product of two degree-d polynomials
inline size_t nft_product_len(size_t d)
{
    const size_t p = nft_nextpow2(2 * d);
    return (p == 2 * d) ? p : nft_nextpow2(2 * d + 1);
}

constexpr size_t kMaxSplitTree = (size_t)kRowTree * 8192;    // largest column transform: 8192 (N up to 2^24)
inline bool nft_tree_too_large(size_t D, int deg0)   // the top product of D matrices of degree deg0: beyond the split limit
{
    const size_t Dpad = nft_nextpow2(D);
    return Dpad > 1 && nft_product_len(Dpad / 2 * (size_t)deg0) > kMaxSplitTree;
}

// ---- polynomials at arbitrary points (KPolyEval, KPolyJoin) ------------------------------------------------------------
// Segments of the coefficient range: a call with few points and a long polynomial must still fill the chip.  One
// workgroup takes 256 points of one polynomial; with G such workgroups, S = ceil(target / G) segments give the launch
// `target` workgroups, as long as a segment keeps kPolyEvalMinSeg powers (two tiles: below that the tile loads and the
// join cost more than the segment saves).  L = powers per segment, a multiple of the 8 chains.  force_S > 0: the tests'
// choice of S (the last segment may be ragged or, for deg < L, the only one that holds coefficients).
constexpr long long kPolyEvalMinSeg = 2 * kPolyEvalTile;
struct PolyEvalSegs {
    int S;
    long long L;
    bool ok;   // the grid fits the launch limits
};
inline PolyEvalSegs polyeval_segments(size_t deg, size_t nz, size_t jobs, size_t target, int force_S)
{
    const unsigned long long G = (unsigned long long)jobs * ((nz + 255) / 256);
    const long long np = (long long)deg + 1;
    long long S = force_S;
    if (S <= 0) {
        S = (long long)(((unsigned long long)target + G - 1) / (G ? G : 1));
        const long long smax = (np + kPolyEvalMinSeg - 1) / kPolyEvalMinSeg;
        if (S > smax) S = smax;
        if (S < 1) S = 1;
    }
    long long L = ((np + S - 1) / S + 7) / 8 * 8;
    if (force_S <= 0) S = (np + L - 1) / L;   // no segment without a coefficient
    return PolyEvalSegs{(int)S, L, G >= 1 && G <= 0x7fffffffull && S <= 65535};
}
// Partials (per array) a plan keeps for calls of up to nz points: those of the most segments a call of nz OR FEWER points
// can get -- S grows as the points fill fewer workgroups, and is largest where they fill one per polynomial.  Monotone
// in nz, so a later call with the same or a smaller nz fits what an earlier one allocated.
inline size_t polyeval_partials(size_t deg, size_t nz, size_t jobs, size_t target, int force_S)
{
    return (size_t)polyeval_segments(deg, 1, jobs, target, force_S).S * jobs * nz;
}
// the two launches; P.S, P.L, P.pp, P.pd are set by the caller (polyeval_segments, S*jobs*nz partials each)
template <class BE> void polyeval_launch(BE &be, const PolyEvalParams &P)
{
    const int gx = (int)((long long)P.batch * P.npoly * ((P.nz + 255) / 256));
    if (P.der) be.template run<KPolyEval<true>>(gx, P.S, P);
    else be.template run<KPolyEval<false>>(gx, P.S, P);
    be.template run<KPolyJoin>(gx, 1, P);
}
// fnft__poly_eval / fnft__poly_evalderiv on device arrays (fnft_amd_poly_eval_device): the partials come from a
// temporary arena, so the stream is waited for once before they go back
template <class BE>
int polyeval_device(BE &be, size_t deg, size_t npoly, size_t batch, const cplx *d_p, size_t pstride, size_t bstride,
                    size_t nz, const cplx *d_z, size_t zstride, cplx *d_val, cplx *d_deriv, int force_S = 0)
{
    const PolyEvalSegs sg = polyeval_segments(deg, nz, batch * npoly, BE::kTargetWorkgroups, force_S);
    if (!sg.ok || batch > 0x7fffffff || npoly > 0x7fffffff) return NFT_EC_NOT_YET_IMPLEMENTED;
    DevArena<BE> tmp(be);
    PolyEvalParams P;
    std::memset(&P, 0, sizeof(P));
    const size_t part = (size_t)sg.S * batch * npoly * nz;
    if (!tmp.get(P.pp, part) || (d_deriv && !tmp.get(P.pd, part))) return NFT_EC_NOMEM;
    P.coef = d_p; P.pstride = (long long)pstride; P.bstride = (long long)bstride;
    P.deg = (long long)deg; P.npoly = (int)npoly; P.batch = (int)batch;
    P.z = d_z; P.zstride = (long long)zstride; P.nz = (long long)nz;
    P.val = d_val; P.der = d_deriv;
    P.S = sg.S; P.L = sg.L;
    polyeval_launch(be, P);
    return be.sync();   // before tmp hands the partials back to the pool
}

template <class BE> class NftPlan {
public:
    BE &be;
    DevArena<BE> mem;        // owns every device buffer below; mem.bytes is the plan's workspace size
    size_t D, M, batch;
    int akns_disc, deg0;
    NftTwiddles<BE> own_tw;          // allocated by init() unless the plan borrows its owner's
    const NftTwiddles<BE> &tw;
    NftResampler<BE> rs;             // ups == 2: the band-limited shifts of the 4SPLIT4A/B front end
    size_t Dpad, plane, n0;

    // device buffers
    cplx *body[2] = {nullptr, nullptr};
    cplx *tail[2] = {nullptr, nullptr};
    double *scale[2] = {nullptr, nullptr};
    unsigned *max2[2] = {nullptr, nullptr};  // ping-pong across split levels, kMax2Slots per matrix
    int *wexp[2] = {nullptr, nullptr};  // per matrix, ping-pong with body/tail/scale
    int *status = nullptr;
    int *wuser = nullptr;   // exponents of caller-supplied transfer matrices (run_contspec_tm)
    // fnft_amd_nsev_eval_device (run_eval): segment partials, grown lazily like wuser, and whether tm_out already holds the
    // matrix of the last tree run (export_tm() without a destination; run_tree clears it)
    cplx *evpp = nullptr, *evpd = nullptr;
    size_t evpp_n = 0, evpd_n = 0;
    bool tm_current = false;
    // monomial program of the order 5..8 schemes (nft_schemes.h), device copies
    double *prog_bfrac = nullptr, *prog_mw = nullptr;
    int *prog_ptr = nullptr;
    unsigned char *prog_fac = nullptr;
    int prog_nB = 0, prog_maxf = 0;
    // KdV (fnft_kdvv): r = -1 for every sample (fnft__kdv_fscatter.c:74-75), general 2x2 tree
    bool kdv = false;
    cplx *rneg = nullptr;
    // real-coefficient path (nft_real.h): r = -1 and a real potential make every coefficient real.  want_real is the
    // caller's request for the NEXT run_front / run_coeffs (hip_backend.hip decides per call); real_run says which layout
    // the current level arrays hold
    bool want_real = false;
    bool real_run = false;
    // 4SPLIT4A/B front end (set_front): Din input samples per signal, every nskip-th step kept,
    // ups preprocessed samples per kept step; D = ups * Dsub matrices enter the tree
    size_t Din = 0, nskip = 1;
    int ups = 1;
    cplx *qpre = nullptr;
    cplx *Y = nullptr, *Z = nullptr, *Z2 = nullptr;   // Z ping-pongs: spectral doubling reads the previous level's Z
    cplx *chY = nullptr, *chV = nullptr;
    cplx *chVS = nullptr;                 // cached spectrum of the chirp filter
    double vs_key[4] = {0, 0, 0, 0};      // log W (re, im), M, deg+1 it was computed for
    bool vs_valid = false;
    cplx *tm_out = nullptr;
    size_t Lc = 0;           // chirp transform length
    int cur = 0;             // index of the body/tail/scale set holding the current level
    bool tree_valid = false;
    // The last split level leaves two things undone.
    // (1) Its maxima stay unreduced (64 slots per matrix): turning them into the pending scale and the final exponent is
    // a one-wave job (KFinalizeScales, 6 us as a launch of its own between the tree and the evaluation) that a kernel of
    // the chirp transform does on the way (ChirpParams::fin_*: every workgroup reduces the slots of its signal for
    // itself, one of them stores scale and exponent).  final_pending says that this is still to be done.
    // (2) Where the chirp transform can take the root straight from the row kernel's output (root_fusable), the level's
    // inverse column pass is not launched either: the chirp transform's first kernel does it in registers
    // (ChirpParams::root_fused, hand_final_to), and the root's coefficients -- body[cur], tail[cur] -- do not exist in
    // HBM.  root_pending says so; root_G and root_inv are the pass as the tree would have launched it.  Z is scratch of
    // the tree run that produced it, so a new run_tree drops a pending root.
    // Every reader of the root other than the fused chirp kernel (export, and through it the discrete spectrum, the
    // block matrices and the inverse plans' trees; the chirp transform on a shape that is not eligible) calls
    // ensure_root() first: the kept pass, then the finalize unless a chirp kernel has done it already.
    bool final_pending = false;
    TreeLevel final_L;
    size_t final_n = 0;
    bool root_pending = false;
    BigLevel root_G;
    bool (*root_inv)(BE &, const BigLevel &) = nullptr;
    void defer_final(const TreeLevel &L, size_t n_out) { final_L = L; final_n = n_out; final_pending = true; }
    void ensure_final()
    {
        if (!final_pending) return;
        be.template run<KFinalizeScales>((int)final_n, 1, final_L);
        final_pending = false;
    }
    void ensure_root()
    {
        if (root_pending) {
            root_pending = false;
            root_inv(be, root_G);   // dispatched once already when the level was run: the length is instantiated
        }
        ensure_final();
    }
    size_t res_deg = 0;      // degree of the transfer matrix of the last tree run
    size_t start_n = 0, start_d = 0;  // matrices (all signals) / degree the tree run starts from
    bool leaf_pending = false;    // run_coeffs left the leaf to the first launch of run_tree
    LeafParams leaf_lp;
    int ne = 4;              // stored entries per matrix in the current tree run
    int kappa_run = 1;
    unsigned long long *dbg_stamps = nullptr;   // -DFNFT_AMD_STAMPS builds: 16 u64 per wave of the row kernel
    int stamp_level = -1;                        // split level (0 = first) whose row kernel is stamped
    int last_warn = 0;       // bit 0: the resampler found the signal not band-limited (set by read_status)
    int tune_stagger = 0;    // row kernel start delay of the second half of a one-round grid (BigLevel::stagger)
    int tune_fuse_root = 1;  // 0: the tree always runs its last inverse column pass itself (A/B runs of ChirpParams::root_fused)
    int dbg_flags = 0;       // timing ablation: only builds with -DFNFT_AMD_ABLATION ever set it (hip_backend.hip)
    // Richardson extrapolation of the continuous spectrum (enable_richardson, run_richardson): a child plan over every
    // rich_g.nskip-th sample on the same back end, fed by KDsGather through rich_q (upsampling factor 1) or with the
    // caller's samples and the stride (4SPLIT4A/B: the resampler sees all of them); its spectrum goes to rich_cs
    std::unique_ptr<NftPlan> rich_child;
    cplx *rich_q = nullptr, *rich_cs = nullptr;
    NftSubGrid rich_g{0, 1};
    bool rich_on = false;

    // borrowed: the twiddle tables of the class this plan is a part of (KdV plans: with the lengths 3*2^b); without it the
    // plan allocates its own
    NftPlan(BE &be_, size_t D_, size_t M_, size_t batch_, int akns_disc_, int deg0_, const NftTwiddles<BE> *borrowed = nullptr)
        : be(be_), mem(be_), D(D_), M(M_), batch(batch_), akns_disc(akns_disc_), deg0(deg0_), tw(borrowed ? *borrowed : own_tw),
          rs(be_, tw)
    {
        Dpad = nft_nextpow2(D);
        n0 = batch * Dpad;
        plane = n0 * (size_t)deg0;
    }

    static size_t sub_count(size_t Din_, size_t nskip_) { return nft_sub_count(Din_, nskip_); }   // its name on the tree plan
    // call before init(): this plan was constructed with D = ups_ * nft_sub_count(Din_, nskip_)
    void set_front(size_t Din_, size_t nskip_, int ups_) { Din = Din_; nskip = nskip_; ups = ups_; }
    // largest pair product done by one workgroup.  General (4-entry) form: 2048 -- a 4096-point pair needs 8 + 4
    // transforms of 16 points per lane in one workgroup (616 B of scratch per lane, 75 us for ONE pair); as a split
    // transform of 4 columns x 1024-point rows it is three small launches (~30 us for one pair, rows over 4 CUs)
    size_t fused_max_len() const { return (ne == 4) ? (size_t)2048 : (size_t)kFusedMaxN; }

    int init()
    {
        if (D < 1 || batch < 1 || deg0 < 1) return NFT_EC_INVALID_ARGUMENT;
        if (Din == 0) Din = D;
        if (ups == 1 && (nskip != 1 || Din != D)) return NFT_EC_NOT_YET_IMPLEMENTED;
        if (ups == 2 && (Din <= 2 || D != 2 * nft_sub_count(Din, nskip))) return NFT_EC_INVALID_ARGUMENT;
        // largest product transform of the tree and chirp length must be within the split limits
        if (nft_tree_too_large(D, deg0)) return NFT_EC_NOT_YET_IMPLEMENTED;
        bool ok = true;
        for (int i = 0; i < 2; i++) {
            ok = ok && mem.get(body[i], 4 * plane) && mem.get(tail[i], 4 * n0) && mem.get(scale[i], n0)
                 && mem.get(wexp[i], n0);
        }
        {   // split levels hold at most n0*deg0/2048 matrices, kMax2Slots slots each
            const size_t nm = n0 * (size_t)deg0 / 32 + 4 * (size_t)kMax2Slots;
            ok = ok && mem.get(max2[0], nm) && mem.get(max2[1], nm) && mem.get(status, 4);
            if (ok) be.memset0(status, 4 * sizeof(int));
        }
        {   // scratch of the split transforms: 4*n_in polynomials of N forward, 4*n_out inverse,
            // maximised over the levels that use them (N can exceed 2d when d is not 2^k)
            size_t needY = 0, needZ = 0, n = n0, d = (size_t)deg0;
            while (n / batch > 1) {
                const size_t N = nft_product_len(d);
                if (d > (size_t)kSchoolMaxDeg && N > fused_max_len()) {
                    if (4 * n * N > needY) needY = 4 * n * N;
                    if (2 * n * N > needZ) needZ = 2 * n * N;
                }
                n /= 2;
                d *= 2;
            }
            if (needY) ok = ok && mem.get(Y, needY) && mem.get(Z, needZ) && mem.get(Z2, needZ);
        }
        if (M > 0) {
            Lc = nft_chirp_len(D * (size_t)deg0 + 1 + M - 1);
            if (Lc > kMaxSplitChirp) return NFT_EC_NOT_YET_IMPLEMENTED;
            ok = ok && mem.get(chY, batch * 2 * Lc) && mem.get(chV, Lc) && mem.get(chVS, Lc);
        }
        ok = ok && mem.get(tm_out, batch * 4 * (D * (size_t)deg0 + 1));
        if (&tw == &own_tw) ok = ok && own_tw.init(mem, kdv);
        else if (!tw.ready() || (kdv && !tw.tw3tab)) return NFT_EC_INVALID_ARGUMENT;
        if (kdv) {
            ok = ok && mem.get(rneg, batch * D);
            if (ok) {
                std::vector<cplx> h(batch * D, cmake(-1.0, 0.0));
                be.h2d(rneg, h.data(), h.size() * sizeof(cplx));
            }
        }
        if (ups == 2) {
            ok = ok && mem.get(qpre, batch * D);
            const int rc = ok ? rs.init(mem, Din, batch, status) : NFT_EC_NOMEM;
            if (rc != NFT_SUCCESS) return rc;
        }
        CoeffProgramHost prog;
        const bool has_prog = akns_disc >= 11 && akns_disc <= 18;   // 2SPLIT5A .. 2SPLIT8B
        if (has_prog) {
            if (!nft_build_coeff_program(akns_disc, deg0, prog)) return NFT_EC_NOT_YET_IMPLEMENTED;
            ok = ok && mem.get(prog_bfrac, prog.bfrac.size()) && mem.get(prog_mw, prog.mw.size())
                 && mem.get(prog_ptr, prog.tgt_ptr.size()) && mem.get(prog_fac, prog.mfac.size());
        }
        if (!ok) return NFT_EC_NOMEM;
        if (has_prog) {
            be.h2d(prog_bfrac, prog.bfrac.data(), prog.bfrac.size() * sizeof(double));
            be.h2d(prog_mw, prog.mw.data(), prog.mw.size() * sizeof(double));
            be.h2d(prog_ptr, prog.tgt_ptr.data(), prog.tgt_ptr.size() * sizeof(int));
            be.h2d(prog_fac, prog.mfac.data(), prog.mfac.size());
            prog_nB = (int)prog.bfrac.size();
            prog_maxf = prog.maxf;
        }
        if (&tw != &own_tw) (void)be.sync();   // no upload of own tables has waited for the cleared status word: wait here
        return NFT_SUCCESS;
    }

    // the workspace back before the plan goes out of scope (the destructor does the same); the plan is not usable after
    void destroy() { rich_child.reset(); mem.clear(); }

    size_t workspace_bytes() const { return mem.bytes + (rich_child ? rich_child->mem.bytes : 0); }

    // ---- front end: fnft__nse_discretization_preprocess_signal (:386-656) + level 0 ------------
    // T: interval of the Din input samples.  Tsub: interval of the kept steps (fnft_nsev.c:381-384),
    // to be handed to run_contspec.
    int run_front(const void *d_q, const double T[2], int kappa, double Tsub[2])
    {
        const double eps_in = (T[1] - T[0]) / (double)(Din - 1);
        if (ups == 1) {
            Tsub[0] = T[0];
            Tsub[1] = T[1];
            return run_coeffs(d_q, kdv ? rneg : nullptr, eps_in, kappa);
        }
        const size_t Dsub = D / 2;
        double eps_t;
        Tsub[0] = T[0];
        nft_sub_interval(T, Din, Dsub, nskip, &Tsub[1], &eps_t);
        const int rc = rs.run_4split4(d_q, nskip, Dsub, qpre, status);
        if (rc != NFT_SUCCESS) return rc;
        return run_coeffs(qpre, nullptr, eps_t, kappa, false);
    }

    // ---- level 0 from samples (fnft__akns_fscatter.c:116-917) --------------------------------
    int run_coeffs(const void *d_q, const void *d_r, double eps_t, int kappa, bool clear_status = true)
    {
        (void)clear_status;   // the status word is cleared by whoever reads it (read_status), not per transform
        CoeffParams p;
        p.q = (const cplx *)d_q;
        p.r = (const cplx *)d_r;
        p.body = body[0];
        p.tail = tail[0];
        p.scale = scale[0];
        p.wexp = wexp[0];
        p.status = status;
        p.plane = plane;
        p.eps_t = eps_t;
        p.D = (int)D;
        p.Dpad = (int)Dpad;
        p.batch = (int)batch;
        p.kappa = kappa;
        p.disc = akns_disc;
        p.deg = deg0;
        real_run = want_real && kdv && d_r == rneg;
        p.real_out = real_run ? 1 : 0;
        cur = 0;
        kappa_run = kappa;
        // leaf kernel: coefficients and the first levels fused (nft_kernels.h body_leaf)
        const int spt = leaf_spt(deg0);
        const bool leaf = spt > 1 && Dpad >= (size_t)spt;
        // NSE symmetry, only the first column stored and transformed (ne = 2): the symmetric form needs
        // r = -kappa*conj(q) (no explicit r) and starts above the direct-product levels, which the leaf kernel guarantees
        ne = (leaf && d_r == nullptr && (size_t)deg0 * spt > (size_t)kSchoolMaxDeg) ? 2 : 4;
        p.ne = ne;
        leaf_pending = false;
        if (leaf) {
            LeafParams lp;
            lp.c = p;
            lp.spt = spt;
            start_n = n0 / (size_t)spt;
            start_d = (size_t)deg0 * (size_t)spt;
            // symmetric form with d = 8: the leaf is computed inside the first multi-level launch (body_leaf_multi)
            if (ne == 2 && start_d == 8 && dbg_flags == 0 && start_n / batch >= 4) {
                leaf_lp = lp;
                leaf_pending = true;
                return NFT_SUCCESS;
            }
            if (!dispatch_leaf(be, lp)) return NFT_EC_NOT_YET_IMPLEMENTED;
            return NFT_SUCCESS;
        }
        const int rl_spt = real_run ? rleaf_strang_samples(akns_disc) : 0;
        if (rl_spt > 1 && Dpad >= (size_t)rl_spt) {
            // even-order splitting schemes on the real path: coefficients from their elementary factors AND the ordered
            // product of rl_spt consecutive samples by direct multiplication (body_rleaf_strang, nft_real.h)
            ne = 4;
            LeafParams lp;
            lp.c = p;
            lp.c.ne = 4;
            lp.spt = rl_spt;
            if (!dispatch_rleaf_strang(be, lp)) return NFT_EC_NOT_YET_IMPLEMENTED;
            start_n = n0 / (size_t)rl_spt;
            start_d = (size_t)deg0 * (size_t)rl_spt;
            return NFT_SUCCESS;
        }
        if (real_run && dispatch_rcoeffs_strang(be, p)) {
            // ... (short signals) coefficients only, composed from their elementary factors
            ne = 4;
        } else if (prog_ptr != nullptr) {
            // schemes of order 5..8: generated coefficient program; the symmetric form can start at
            // level 0 because every level is an FFT level (deg0 > kSchoolMaxDeg)
            ne = (d_r == nullptr) ? 2 : 4;
            CoeffProgParams pp;
            pp.c = p;
            pp.c.ne = ne;
            pp.bfrac = prog_bfrac; pp.tgt_ptr = prog_ptr; pp.mw = prog_mw; pp.mfac = prog_fac;
            pp.nB = prog_nB; pp.maxf = prog_maxf;
            be.template run<KCoeffsProg>((int)((n0 + 63) / 64), 1, pp);
        } else if (!dispatch_coeffs(be, p)) return NFT_EC_NOT_YET_IMPLEMENTED;
        start_n = n0;
        start_d = (size_t)deg0;
        return NFT_SUCCESS;
    }

    // ---- level 0 from explicit coefficient matrices in the reference layout (host) ------------
    // p_host: [4][n*(deg0+1)], n = D matrices (fnft__poly_fmult.c:398-401)
    int load_level0_from_host(const std::complex<double> *p_host)
    {
        std::vector<cplx> hb(4 * plane), ht(4 * n0);
        std::vector<double> hs(n0, 1.0);
        const size_t w = (size_t)deg0 + 1;
        for (int e = 0; e < 4; e++)
            for (size_t j = 0; j < Dpad; j++) {
                for (size_t k = 0; k < w; k++) {
                    cplx v = cmake(0.0, 0.0);
                    if (j < D) {
                        const std::complex<double> z = p_host[(size_t)e * D * w + j * w + k];
                        v = cmake(z.real(), z.imag());
                    } else if (k == 0 && (e == 0 || e == 3)) {
                        v = cmake(1.0, 0.0);  // identity pad z^deg * I, fnft__poly_fmult.c:422-438
                    }
                    if (k < (size_t)deg0) hb[(size_t)e * plane + j * deg0 + k] = v;
                    else ht[(size_t)e * n0 + j] = v;
                }
            }
        be.h2d(body[0], hb.data(), hb.size() * sizeof(cplx));
        be.h2d(tail[0], ht.data(), ht.size() * sizeof(cplx));
        be.h2d(scale[0], hs.data(), hs.size() * sizeof(double));
        be.memset0(wexp[0], n0 * sizeof(int));
        cur = 0;
        ne = 4;
        real_run = false;
        start_n = n0;
        start_d = (size_t)deg0;
        return NFT_SUCCESS;
    }

    // ---- product tree (fnft__poly_fmult.c:460-519) ---------------------------------------------
    // ---- level 0 from coefficient matrices in DEVICE memory (reference layout, D matrices of degree deg0) ------
    int load_level0_from_device(const void *d_p)
    {
        ImportParams I;
        I.p = (const cplx *)d_p;
        I.body = body[0]; I.tail = tail[0]; I.scale = scale[0]; I.wexp = wexp[0];
        I.plane = plane;
        I.n = (long long)D; I.npad = (long long)Dpad; I.deg = (long long)deg0;
        const long long tot = 4 * I.npad * (I.deg + 1);
        be.template run<KImportLevel0>((int)((tot + 255) / 256), 1, I);
        cur = 0;
        ne = 4;
        real_run = false;
        start_n = n0;
        start_d = (size_t)deg0;
        return NFT_SUCCESS;
    }

    // what one level of the tree hands on to the next
    struct TreeWalk {
        bool y_from_bridge = false;   // the previous level bridged: Y holds this level's forward column step
        bool in_pending = false;      // the previous level was split: its rescale is still pending
        int zcur = 0, mcur = 0;       // which of Z / Z2 and of the max2 pair the level reads
    };
    // the level of n matrices of degree d, all signals; the branch that runs it adds its twiddle tables
    TreeLevel tree_level(const TreeWalk &w, size_t n, size_t d, int ne_level, int dbg) const
    {
        TreeLevel L;
        L.body_in = body[cur]; L.tail_in = tail[cur]; L.scale_in = scale[cur];
        L.body_out = body[cur ^ 1]; L.tail_out = tail[cur ^ 1]; L.scale_out = scale[cur ^ 1];
        L.max2_out = max2[w.mcur ^ 1];
        L.max2_in = max2[w.mcur];
        L.in_pending = w.in_pending ? 1 : 0;
        L.wexp_in = wexp[cur];
        L.wexp_out = wexp[cur ^ 1];
        L.plane = plane;
        L.n_in = (int)n;
        L.d = (int)d;
        L.pairs_per_signal = (int)(n / 2 / batch);
        L.ne = ne_level;
        L.kappa = kappa_run;
        L.dbg = dbg;
        return L;
    }
    // the launches of a split level G: the forward column step unless the previous level bridged into Y (or the row
    // kernel does it on the fly, y_direct), the rows, then the bridge straight into the next level's column step when
    // that level is split too (next_split), else the inverse column step
    typedef bool (*ColStep)(BE &, const BigLevel &);
    bool run_split_level(TreeWalk &w, const BigLevel &G, ColStep fwd, ColStep bridge, ColStep inv, bool next_split)
    {
        bool ok = true;
        if (!w.y_from_bridge && !G.y_direct) ok = fwd(be, G);
        if (ok) run_mid(be, G);
        const bool last_level = G.L.pairs_per_signal <= 1;
        if (ok && !next_split && last_level && root_fusable(G)) {
            root_G = G;
            root_inv = inv;
            root_pending = true;
        } else if (ok) {
            ok = next_split ? bridge(be, G) : inv(be, G);
        }
        w.zcur ^= 1;
        w.y_from_bridge = ok && next_split;
        // the consumer of the next level finalizes this one; the last level needs a kernel
        if (ok && last_level) defer_final(G.L, (size_t)G.L.n_in / 2);
        w.in_pending = !last_level;
        w.mcur ^= 1;
        return ok;
    }
    // The chirp transform of this plan can take the root of the last split level G from the row kernel's output
    // (chirp_col_fwd_root, nft_kernels.h): complex symmetric form, one matrix per signal, no padding (deg = deg_tot = N,
    // so N = 2d and coefficient kk is chirp element N - kk), and a chirp of length 2N -- M <= D*deg0 -- whose rows are
    // twice the tree's, so that both have the same column length.  Plans of fewer than kRootFusedMinM spectral points keep
    // the root's last pass inside the tree: a conservative cut -- those are the plans that are made for their transfer
    // matrix (a few points to check, then the export; tests/test_gpu_tree_paths.py pins KColInv<N1> in the transform of
    // its M = 64 plans), and the saving does not depend on M.
    static constexpr size_t kRootFusedMinM = 512;
    bool root_fusable(const BigLevel &G) const
    {
        if (kRowChirp != 2 * kRowTree) return false;
        const size_t N = (size_t)G.N1 * (size_t)G.N2;
        return tune_fuse_root != 0 && dbg_flags == 0 && !real_run && ne == 2 && G.L.ne == 2 && M >= kRootFusedMinM && chY != nullptr
               && G.N1 < kRootFusedMaxN1 && G.N2 == kRowTree && Lc == 2 * N && N == 2 * (size_t)G.L.d && D == Dpad && N == D * (size_t)deg0
               && (size_t)(G.L.n_in / 2) == batch;
    }

    // the same tree on real coefficients (nft_real.h): folded transforms of length M = nft_real_len(d)
    int run_tree_real()
    {
        size_t n = start_n, d = start_d;
        TreeWalk w;
        // degrees 3*2^a: the split levels take columns of 3*K rows of kRowGen points -- transform length M = d exactly
        // (nft_real.h) -- when the last level's column length is instantiated
        bool r3 = false;
        if (tw.tw3tab) {
            size_t odd = start_d;
            while (odd % 2 == 0) odd /= 2;
            const size_t dtop = start_d * (start_n / batch) / 2;   // degree of the last level's factors
            r3 = (odd == 3) && dtop % (size_t)kRowGen == 0 && dtop / (size_t)kRowGen <= (size_t)3 * kR3MaxK;
        }
        while (n / batch > 1) {
            TreeLevel L = tree_level(w, n, d, 4, 0);
            const size_t M = nft_real_len(d);
            bool ok;
            if (d <= (size_t)kSchoolMaxDeg) {
                ok = dispatch_rpair_school(be, L);
            } else if (r3 && d % (size_t)kRowGen == 0 && d / (size_t)kRowGen >= 3) {
                BigLevel G;
                std::memset(&G, 0, sizeof(G));
                G.L = L;
                G.Y = Y;
                G.Z = w.zcur ? Z2 : Z;
                G.N2 = kRowGen;
                G.N1 = (int)(d / (size_t)kRowGen);   // 3*K
                const size_t K = (size_t)G.N1 / 3;
                G.btw = tw.big_tw3(4 * d);              // row twiddle w_{4M}^{(4 k1 - 1) n2}, M = d
                G.rtwist = 1;
                G.row_mod = 4ull * (unsigned long long)d;
                G.tw1 = tw.tw_table(K >= 2 ? K : 2);
                G.tw2 = tw.tw_table((size_t)G.N2);
                G.tw1x2 = tw.tw_table(2 * K);
                G.tw3 = tw.tw3_table((size_t)G.N1);
                G.tw3x2 = tw.tw3_table((size_t)2 * G.N1);
                G.twq = tw.tw3_table((size_t)4 * G.N1);
                G.twq2 = ((size_t)8 * G.N1 <= ((size_t)3 << kTw3MaxLog)) ? tw.tw3_table((size_t)8 * G.N1) : nullptr;
                G.y_unscaled = w.y_from_bridge ? 1 : 0;
                const bool next_split = (n / 2 / batch > 1) && K <= (size_t)kR3BridgeMaxK;
                ok = run_split_level(w, G, dispatch_r3col_fwd<BE>, dispatch_r3bridge<BE>, dispatch_r3col_inv<BE>,
                                     next_split);
            } else if (M <= (size_t)kRealFusedMaxM) {
                L.tw = tw.tw_table(M);
                L.twx = tw.tw_table(4 * M);
                ok = dispatch_rpair(be, L, (int)M);
            } else {
                BigLevel G;
                std::memset(&G, 0, sizeof(G));
                G.L = L;
                G.Y = Y;
                G.Z = w.zcur ? Z2 : Z;
                G.N2 = row_len_gen(M);
                G.N1 = (int)(M / (size_t)G.N2);
                if (4 * (size_t)G.N1 > (size_t)kMaxTwTable) return NFT_EC_NOT_YET_IMPLEMENTED;
                G.btw = tw.big_tw(4 * M);   // row twiddle w_{4M}^{(4 k1 - 1) n2}
                G.rtwist = 1;
                G.tw1 = tw.tw_table((size_t)G.N1);
                G.tw2 = tw.tw_table((size_t)G.N2);
                G.tw1x2 = tw.tw_table((size_t)2 * G.N1);
                G.twq = tw.tw_table((size_t)4 * G.N1);
                G.twq2 = (8 * (size_t)G.N1 <= (size_t)kMaxTwTable) ? tw.tw_table((size_t)8 * G.N1) : nullptr;
                G.y_unscaled = w.y_from_bridge ? 1 : 0;
                const bool next_split = (n / 2 / batch > 1) && G.N1 <= kRBridgeMaxN1
                                        && row_len_gen(2 * M) == G.N2;
                ok = run_split_level(w, G, dispatch_rcol_fwd<BE>, dispatch_rbridge<BE>, dispatch_rcol_inv<BE>,
                                     next_split);
            }
            if (!ok) return NFT_EC_NOT_YET_IMPLEMENTED;
            cur ^= 1;
            n /= 2;
            d *= 2;
        }
        res_deg = D * (size_t)deg0;
        tree_valid = true;
        return NFT_SUCCESS;
    }

    int run_tree()
    {
        final_pending = false;   // an unconsumed root of an earlier run is dropped
        root_pending = false;
        tm_current = false;
        if (real_run) return run_tree_real();
        size_t n = start_n;     // matrices at the current level, all signals
        size_t d = start_d;
        TreeWalk w;
        int split_idx = 0;
        while (n / batch > 1) {
            TreeLevel L = tree_level(w, n, d, ne, dbg_flags);
            const size_t N = nft_product_len(d);
            L.tw = (N <= (size_t)kMaxTwTable) ? tw.tw_table(N) : nullptr;
            bool ok;
            // consecutive fused levels of the symmetric form in one launch: as many as fit (<= 3)
            int stages = 1;
            if (ne == 2 && d > (size_t)kSchoolMaxDeg && N == 2 * d && N >= 16 && dbg_flags == 0) {
                while (stages < 3 && (N << stages) <= (size_t)kFusedMaxN && ((n / batch) >> (stages + 1)) >= 1) stages++;
            }
            if (leaf_pending && stages < 2) {   // cannot happen (start_n/batch >= 4), but never skip the leaf
                if (!dispatch_leaf(be, leaf_lp)) return NFT_EC_NOT_YET_IMPLEMENTED;
                leaf_pending = false;
            }
            if (stages > 1) {
                for (int s = 0; s < stages; s++) L.twm[s] = tw.tw_table(N << s);
                if (leaf_pending) {
                    LeafMultiParams Q;
                    Q.lp = leaf_lp;
                    Q.L = L;
                    ok = dispatch_leaf_multi(be, Q, stages);
                    leaf_pending = false;
                } else {
                    ok = dispatch_multi(be, L, (int)N, stages);
                }
                if (!ok) return NFT_EC_NOT_YET_IMPLEMENTED;
                cur ^= 1;
                n >>= stages;
                d <<= stages;
                continue;
            }
            if (d <= (size_t)kSchoolMaxDeg) {
                ok = dispatch_pair_school(be, L);
            } else if (N <= fused_max_len()) {
                ok = dispatch_pair_fft(be, L, (int)N);
            } else {
                BigLevel G;
                G.L = L;
                G.Y = Y;
                G.Z = w.zcur ? Z2 : Z;
                G.Zprev = w.zcur ? Z : Z2;
                G.y_split = w.y_from_bridge ? 1 : 0;   // every bridge doubles: Y holds the odd rows only
                G.N2 = (ne == 4) ? row_len_gen(N) : kRowTree;
                G.N1 = (int)(N / (size_t)G.N2);
                G.btw = tw.big_tw(N);
                G.tw1 = (G.N1 >= 2) ? tw.tw_table((size_t)G.N1) : nullptr;
                G.tw2 = tw.tw_table((size_t)G.N2);
                G.tw1x2 = tw.tw_table((size_t)2 * G.N1);
                G.btw2 = tw.big_tw(2 * N);
                G.y_unscaled = w.y_from_bridge ? 1 : 0;
                // first split level of the symmetric form: a length-4 column transform of two non-zero rows is done
                // by the row kernel on the fly (saves the column launch and its 32 + 64 MB)
                G.y_direct = (!w.y_from_bridge && G.N1 == 4 && N == 2 * d && dbg_flags == 0 && ne == 2) ? 1 : 0;
                G.stagger = (n / 2 * (size_t)G.N1 == 512) ? tune_stagger : 0;   // exactly one round of workgroups
                G.stamps = (dbg_stamps && split_idx == stamp_level) ? dbg_stamps : nullptr;
                split_idx++;
                // the bridge doubles the spectrum (body_col_bridge2; N = 2d and N > 2d alike)
                const bool next_split = (n / 2 / batch > 1) && G.N1 <= 4096 && nft_product_len(2 * d) == 2 * N
                                        && ((ne == 4) ? row_len_gen(2 * N) : kRowTree) == G.N2;
                ok = run_split_level(w, G, dispatch_col_fwd<BE>, dispatch_col_bridge2<BE>, dispatch_col_inv<BE>,
                                     next_split);
            }
            if (!ok) return NFT_EC_NOT_YET_IMPLEMENTED;
            cur ^= 1;
            n /= 2;
            d *= 2;
        }
        res_deg = D * (size_t)deg0;
        tree_valid = true;
        return NFT_SUCCESS;
    }

    // ---- result in the reference layout (fnft__poly_fmult.c:522-538) ---------------------------
    // dst / stride / unscale: the result straight into a caller's strided device array, times 2^W (layer peeling);
    // bstride: distance between the signals of a batch in dst
    void export_tm(cplx *dst = nullptr, size_t stride = 0, bool unscale = false, size_t bstride = 0)
    {
        ensure_root();
        ExportParams E;
        E.body = body[cur]; E.tail = tail[cur]; E.scale = scale[cur];
        E.out = dst ? dst : tm_out;
        E.out_stride = dst ? (long long)stride : 0;
        E.out_bstride = dst ? (long long)bstride : 0;
        E.W = unscale ? wexp[cur] : nullptr;
        E.plane = plane;
        E.deg_tot = (long long)(Dpad * (size_t)deg0);
        E.deg = (long long)res_deg;
        E.batch = (int)batch;
        E.ne = ne;
        E.kappa = kappa_run;
        E.real_layout = real_run ? 1 : 0;
        const long long tot = 4 * (E.deg + 1) * E.batch;
        be.template run<KExportTm>((int)((tot + 255) / 256), 1, E);
        if (!dst) tm_current = true;
    }

    // ---- a(lambda), b(lambda) and their derivatives at arbitrary lambda (fnft_amd_nsev_eval_device) ---------------------
    // Entries 11 and 21 of the last tree run's matrix by KPolyEval / KPolyJoin at z = exp(2i lambda eps_t/(deg0*ups))
    // (fnft__akns_discretization.c:204-219), times 2^W exp(i lambda pf) with the phase factors of run_contspec_impl
    // (fnft__nse_discretization.c:240-379).  T: the interval of the plan's input samples.  d_out per signal:
    // [a(n) | b(n)], with derivative [a | b | da/dlambda | db/dlambda].  lambda_stride 0: one list for all signals.
    int run_eval(const double T[2], int nse_disc, const cplx *d_lambda, size_t n, size_t lambda_stride, bool derivative,
                 cplx *d_out, int force_S = 0)
    {
        if (!tree_valid || kdv) return NFT_EC_INVALID_ARGUMENT;
        const PolyEvalSegs sg = polyeval_segments(res_deg, n, batch * 2, BE::kTargetWorkgroups, force_S);
        if (!sg.ok) return NFT_EC_NOT_YET_IMPLEMENTED;
        const size_t part = polyeval_partials(res_deg, n, batch * 2, BE::kTargetWorkgroups, force_S);   // >= S * batch * 2 * n
        if (part > evpp_n || (derivative && part > evpd_n)) be.sync();   // queued kernels may still use what goes back
        if (part > evpp_n) {
            mem.give_back(evpp);
            evpp_n = 0;
            if (!mem.get(evpp, part)) return NFT_EC_NOMEM;
            evpp_n = part;
        }
        if (derivative && part > evpd_n) {
            mem.give_back(evpd);
            evpd_n = 0;
            if (!mem.get(evpd, part)) return NFT_EC_NOMEM;
            evpd_n = part;
        }
        if (!tm_current) export_tm();   // ensure_root() and the export, once per tree run
        const double deg1 = (double)(deg0 * ups);
        const size_t Dg = D / (size_t)ups;
        // the interval of the kept steps as run_front hands it to run_contspec (nskip = 1 here)
        const double T1 = (ups == 1) ? T[1] : T[0] + (double)(Dg - 1) * ((T[1] - T[0]) / (double)(Din - 1));
        const double eps_t = (T1 - T[0]) / (double)(Dg - 1);
        const double bc = 0.5;
        const bool shifted = (nse_disc == 0 /*MODAL*/ || nse_disc == 4 /*2SPLIT2A*/);
        PolyEvalParams P;
        std::memset(&P, 0, sizeof(P));
        P.coef = tm_out;
        P.pstride = (long long)(2 * (res_deg + 1));   // [r11|r12|r21|r22]: entries 11 and 21
        P.bstride = (long long)(4 * (res_deg + 1));
        P.deg = (long long)res_deg; P.npoly = 2; P.batch = (int)batch;
        P.z = d_lambda; P.zstride = (long long)lambda_stride; P.nz = (long long)n;
        P.val = d_out; P.der = derivative ? d_out : nullptr;
        P.S = sg.S; P.L = sg.L; P.pp = evpp; P.pd = evpd;
        P.nse = 1; P.eps_t = eps_t; P.deg1 = deg1; P.W = wexp[cur];
        P.pf[0] = -eps_t * (double)Dg + (T1 + eps_t * bc) - (T[0] - eps_t * bc);
        P.pf[1] = -eps_t * (double)Dg - (T1 + eps_t * bc) - (T[0] - eps_t * bc) + (shifted ? eps_t / deg1 : 0.0);
        polyeval_launch(be, P);
        return NFT_SUCCESS;
    }

    // ---- chirp z + epilogue (fnft_nsev.c:744-891) ----------------------------------------------
    struct Contspec {
        double T[2], XI[2];
        int nse_disc;
        int cstype;
        int normalization_flag;
    };

    int run_contspec(void *d_contspec, const Contspec &cs) { return run_contspec_impl(d_contspec, cs, nullptr, 0); }

    // nsev_compute_contspec (src/fnft_nsev.c:744-891) on a transfer matrix the CALLER supplies: d_tm holds, per
    // signal, [r11|r12|r21|r22] of deg+1 = D*deg0+1 coefficients each (highest power first, the layout of
    // fnft__poly_fmult2x2 / fnft_amd_plan_get_transfer_matrix_device), true matrix = stored * 2^W.
    int run_contspec_tm(void *d_contspec, const Contspec &cs, const void *d_tm, int W)
    {
        if (!d_tm) return NFT_EC_INVALID_ARGUMENT;
        if (!wuser && !mem.get(wuser, batch)) return NFT_EC_NOMEM;
        std::vector<int> hw(batch, W);
        be.h2d(wuser, hw.data(), batch * sizeof(int));
        return run_contspec_impl(d_contspec, cs, (const cplx *)d_tm, 1);
    }

    int run_contspec_impl(void *d_contspec, const Contspec &cs, const cplx *d_tm, int from_tm)
    {
        // step size and phase factors refer to D_given = D/upsampling (fnft_nsev.c:766-774);
        // lambda -> z uses degree*upsampling (fnft__akns_discretization.c:204-219)
        const double deg1 = (double)(deg0 * ups);
        const size_t Dg = D / (size_t)ups;
        const double eps_t = (cs.T[1] - cs.T[0]) / (double)(Dg - 1);
        const double eps_xi = (cs.XI[1] - cs.XI[0]) / (double)(M - 1);
        // lambda -> z, fnft__akns_discretization.c:204-219 called from fnft_nsev.c:822-827
        const double phiV = 2.0 * eps_xi * eps_t / deg1;
        const double phiA = 2.0 * (-cs.XI[0]) * eps_t / deg1;
        const std::complex<double> V(std::cos(phiV), std::sin(phiV));
        const std::complex<double> A(std::cos(phiA), std::sin(phiA));
        const std::complex<double> lV = nft_clog(V), lA = nft_clog(A);

        ChirpParams C;
        std::memset(&C, 0, sizeof(C));
        C.body = body[cur]; C.tail = tail[cur]; C.scale = scale[cur];
        C.poly = from_tm ? d_tm : nullptr;
        C.poly_tm = from_tm;
        C.plane = plane;
        C.deg_tot = (long long)(Dpad * (size_t)deg0);
        C.deg = from_tm ? (long long)(D * (size_t)deg0) : (long long)res_deg;
        C.batch = (int)batch;
        C.npoly = 2;
        C.ne = from_tm ? 4 : ne;
        C.entry[0] = 0;                    // H11, fnft_nsev.c:829
        C.entry[1] = (C.ne == 4) ? 2 : 1;  // H21, fnft_nsev.c:832 (plane 1 in the symmetric form)
        C.logA[0] = lA.real(); C.logA[1] = lA.imag();
        C.logW[0] = lV.real(); C.logW[1] = lV.imag();
        C.M = (long long)M;
        C.Ybuf = chY; C.Vbuf = chV; C.Hbuf = nullptr;
        fill_chirp_geometry(tw, C, Lc);
        C.contspec = (cplx *)d_contspec;
        C.W = from_tm ? wuser : wexp[cur];
        C.status = status;
        C.xi0 = cs.XI[0];
        C.eps_xi = eps_xi;
        // phase factors, fnft__nse_discretization.c:240-379, boundary coefficient 0.5
        const double bc = 0.5;
        const bool shifted = (cs.nse_disc == 0 /*MODAL*/ || cs.nse_disc == 4 /*2SPLIT2A*/);
        C.pf_rho = -2.0 * (cs.T[1] + eps_t * bc) + (shifted ? eps_t / deg1 : 0.0);
        C.pf_a = -eps_t * (double)Dg + (cs.T[1] + eps_t * bc) - (cs.T[0] - eps_t * bc);
        C.pf_b = -eps_t * (double)Dg - (cs.T[1] + eps_t * bc) - (cs.T[0] - eps_t * bc)
                 + (shifted ? eps_t / deg1 : 0.0);
        C.cstype = cs.cstype;
        C.use_W = 1;  // W is the exponent actually taken out, whatever normalization_flag says
        if (!from_tm) hand_final_to(C);
        return run_chirp_cached(C);
    }

    // fnft_kdvv.c:126-209 (tf2contspec_negxi): entries 12 and 22 on the grid -(XI0 + m*eps_xi)
    int run_contspec_kdv(void *d_contspec, const double T[2], const double XI[2], bool scheme_2A)
    {
        const double deg1 = (double)deg0;
        const double eps_t = (T[1] - T[0]) / (double)(D - 1);
        const double eps_xi = (XI[1] - XI[0]) / (double)(M - 1);
        const double phiV = -2.0 * eps_xi * eps_t / deg1;   // :159
        const double phiA = 2.0 * XI[0] * eps_t / deg1;     // :160
        const std::complex<double> V(std::cos(phiV), std::sin(phiV));
        const std::complex<double> A(std::cos(phiA), std::sin(phiA));
        const std::complex<double> lV = nft_clog(V), lA = nft_clog(A);
        ChirpParams C;
        std::memset(&C, 0, sizeof(C));
        C.body = body[cur]; C.tail = tail[cur]; C.scale = scale[cur];
        C.plane = plane;
        C.deg_tot = (long long)(Dpad * (size_t)deg0);
        C.deg = (long long)res_deg;
        C.batch = (int)batch;
        C.npoly = 2;
        C.ne = ne;
        if (ne != 4) return NFT_EC_OTHER;   // explicit r: the general form
        C.entry[0] = 1;   // H12, :165
        C.entry[1] = 3;   // H22, :172
        C.logA[0] = lA.real(); C.logA[1] = lA.imag();
        C.logW[0] = lV.real(); C.logW[1] = lV.imag();
        C.M = (long long)M;
        C.Ybuf = chY; C.Vbuf = chV;
        fill_chirp_geometry(tw, C, Lc);
        C.contspec = (cplx *)d_contspec;
        C.W = wexp[cur];
        C.status = status;
        C.xi0 = -XI[0];
        C.eps_xi = -eps_xi;
        C.pf_rho = 2.0 * (T[1] + 0.5 * eps_t);          // :199, boundary coefficient 0.5
        C.pf_a = scheme_2A ? -eps_t / deg1 : 0.0;       // :186-195
        C.cstype = 10;
        C.real_layout = real_run ? 1 : 0;
        hand_final_to(C);
        return run_chirp_cached(C);
    }

    // ---- Richardson extrapolation of the continuous spectrum (src/fnft_nsev.c:316-406, fnft_nsev_host.c) -----------------
    // The workspace of the coarse pass, once; the caller has waited for the plan's stream.  The coarse grid is that of
    // nft_sub_grid for Dsub = D/2.
    bool rich_ready() const { return (bool)rich_child; }
    int enable_richardson()
    {
        if (rich_child) { rich_on = true; return NFT_SUCCESS; }
        if (kdv || M == 0 || Din < 3) return NFT_EC_INVALID_ARGUMENT;
        if (nskip > 1) return NFT_EC_NOT_YET_IMPLEMENTED;
        rich_g = nft_sub_grid(Din, Din / 2);
        std::unique_ptr<NftPlan> ch(new NftPlan(be, rich_g.Dsub * (size_t)ups, M, batch, akns_disc, deg0, &tw));
        if (ups == 2) ch->set_front(Din, rich_g.nskip, ups);
        const int rc = ch->init();
        cplx *q = nullptr, *cs = nullptr;
        if (rc != NFT_SUCCESS || (ups == 1 && !mem.get(q, batch * rich_g.Dsub)) || !mem.get(cs, batch * 3 * M)) {
            (void)be.sync();   // what init enqueued, before the child's blocks go back
            mem.give_back(q);
            return rc != NFT_SUCCESS ? rc : NFT_EC_NOMEM;
        }
        rich_q = q;
        rich_cs = cs;
        rich_child = std::move(ch);
        rich_on = true;
        return NFT_SUCCESS;
    }

    // after run_front / run_tree / run_contspec of the same call (d_q, T: the input samples and their interval; cs: what
    // run_contspec was given): the coarse pass on the child, then contspec = (sn*contspec - coarse)/sd where
    // |xi| < 0.9 pi / (2 eps_t_sub), fnft_nsev_host.c (fnft_nsev) in its order
    int run_richardson(const void *d_q, const double T[2], int kappa, void *d_contspec, const Contspec &cs)
    {
        NftPlan &ch = *rich_child;
        const double eps_t = (T[1] - T[0]) / (double)(Din - 1);
        double Tc[2] = {T[0], 0.0}, eps_sub;
        nft_sub_interval(T, Din, rich_g.Dsub, rich_g.nskip, &Tc[1], &eps_sub);
        double Tsub[2];
        int rc;
        if (ups == 1) {
            GatherParams G;
            G.q = (const cplx *)d_q; G.out = rich_q;
            G.D = (long long)Din; G.Dsub = (long long)rich_g.Dsub; G.nskip = (long long)rich_g.nskip; G.batch = (long long)batch;
            be.template run<KDsGather>((int)((batch * rich_g.Dsub + 255) / 256), 1, G);
            rc = ch.run_front(rich_q, Tc, kappa, Tsub);
        } else {
            rc = ch.run_front(d_q, T, kappa, Tsub);   // resampling of all Din samples, every rich_g.nskip-th step kept
        }
        if (rc == NFT_SUCCESS) rc = ch.run_tree();
        if (rc != NFT_SUCCESS) return rc;
        Contspec cc = cs;
        cc.T[0] = Tsub[0]; cc.T[1] = Tsub[1];
        rc = ch.run_contspec(rich_cs, cc);
        if (rc != NFT_SUCCESS) return rc;
        RichCsParams R;
        std::memset(&R, 0, sizeof(R));
        R.c = (cplx *)d_contspec; R.cs = rich_cs;
        R.M = (long long)M; R.batch = (long long)batch;
        R.parts = (cs.cstype == 0) ? 1 : (cs.cstype == 1 ? 2 : 3);
        R.xi0 = cs.XI[0];
        R.dxi = (cs.XI[1] - cs.XI[0]) / (double)(M - 1);
        R.bound = 0.9 * std::acos(-1.0) / (2.0 * eps_sub);
        R.sn = std::pow(eps_sub / eps_t, (double)nft_nse_method_order(cs.nse_disc));
        R.sd = R.sn - 1.0;
        be.template run<KRichCombineCs>((int)((batch * M + 255) / 256), 1, R);
        return NFT_SUCCESS;
    }

    // the root's pending finalize rides on a kernel of the chirp transform (one matrix per signal at the root): on the row
    // kernel, with the root's last inverse column pass on the first column kernel, when that pass is still pending
    // (root_fusable said that this plan's chirp transform can take it; the checks here are about THIS transform); on the
    // first column kernel otherwise
    void hand_final_to(ChirpParams &C)
    {
        if (root_pending && final_pending && final_n == batch && C.poly == nullptr && !C.real_layout && C.ne == 2
            && C.npoly == 2 && C.dft_len == 0 && C.N1 == root_G.N1 && C.N2 == 2 * root_G.N2 && C.deg == C.deg_tot
            && C.deg == (long long)root_G.N1 * root_G.N2) {
            C.root_fused = 1;
            C.root_N2 = root_G.N2;
            C.root_Z = root_G.Z;
            C.root_L = root_G.L;
            C.fin_max2 = final_L.max2_out;
            C.fin_scale = final_L.scale_out;
            C.fin_wexp = final_L.wexp_out;
            final_pending = false;   // the coefficients stay pending: ensure_root() makes them for whoever asks
            return;
        }
        if (root_pending) {
            root_pending = false;
            root_inv(be, root_G);
        }
        if (!final_pending) return;
        if (final_n != batch) { ensure_final(); return; }
        C.fin_max2 = final_L.max2_out;
        C.fin_scale = final_L.scale_out;
        C.fin_wexp = final_L.wexp_out;
        final_pending = false;
    }

    // the spectrum of the chirp filter only depends on W, M, the degree and the transform length:
    // repeated transforms on the same grids (T, XI fixed) reuse it
    int run_chirp_cached(ChirpParams &C)
    {
        const double key[4] = {C.logW[0], C.logW[1], (double)C.M, (double)(C.deg + 1)};
        const bool hit = vs_valid && std::memcmp(key, vs_key, sizeof(key)) == 0;
        C.VS = chVS;
        C.v_mode = hit ? 2 : 1;
        const int rc = run_chirp(be, C);
        if (rc == NFT_SUCCESS) { std::memcpy(vs_key, key, sizeof(key)); vs_valid = true; }
        return rc;
    }

    // stand-alone chirp z-transform of one host polynomial (fnft__poly_chirpz.c:33-105): no plan, tables and workspace
    // from a temporary arena.  d_out != NULL: the M values stay on the device (d_out), `result` is not touched
    static int chirpz_host(BE &be, size_t deg, const std::complex<double> *p, std::complex<double> A,
                           std::complex<double> Wc, size_t Mo, std::complex<double> *result, cplx *d_out = nullptr)
    {
        DevArena<BE> tmp(be);
        NftTwiddles<BE> tabs;
        const size_t L = nft_chirp_len(deg + 1 + Mo - 1);
        if (L > kMaxSplitChirp) return NFT_EC_NOT_YET_IMPLEMENTED;
        cplx *dp = nullptr, *dY = nullptr, *dV = nullptr, *dH = nullptr;
        int *dstatus = nullptr;
        const bool ok = tabs.init(tmp) && tmp.get(dp, deg + 1) && tmp.get(dY, L) && tmp.get(dV, L) && tmp.get(dH, Mo)
                        && tmp.get(dstatus, 4);
        if (!ok) return NFT_EC_NOMEM;
        be.h2d(dp, p, (deg + 1) * sizeof(cplx));
        be.memset0(dstatus, 4 * sizeof(int));
        const std::complex<double> lA = nft_clog(A), lW = nft_clog(Wc);
        ChirpParams C;
        std::memset(&C, 0, sizeof(C));
        C.poly = dp; C.deg = (long long)deg; C.M = (long long)Mo;
        C.batch = 1; C.npoly = 1;
        C.logA[0] = lA.real(); C.logA[1] = lA.imag();
        C.logW[0] = lW.real(); C.logW[1] = lW.imag();
        C.Ybuf = dY; C.Vbuf = dV; C.Hbuf = d_out ? d_out : dH;
        fill_chirp_geometry(tabs, C, L);
        C.status = dstatus; C.cstype = -1;
        int rc = run_chirp(be, C);
        if (rc == NFT_SUCCESS) {
            if (!d_out) be.d2h(result, dH, Mo * sizeof(cplx));
            rc = be.sync();
        }
        return rc;
    }

    // stand-alone band-limited shift of one host signal by delta (fnft__misc.c:326-407), 1/D included: a batch-1
    // resampler over a temporary arena
    static int resample_host(BE &be, size_t Dn, double eps_t, const std::complex<double> *q, double delta,
                             std::complex<double> *q_new, int *warn_not_bandlimited = nullptr)
    {
        DevArena<BE> tmp(be);
        NftTwiddles<BE> tabs;
        NftResampler<BE> one(be, tabs);
        cplx *dq = nullptr;
        int rc = one.init(tmp, Dn, 1);
        if (rc == NFT_SUCCESS && !(tabs.init(tmp) && tmp.get(dq, Dn))) rc = NFT_EC_NOMEM;
        if (rc != NFT_SUCCESS) return rc;
        be.h2d(dq, q, Dn * sizeof(cplx));
        ResampleParams R;
        rc = one.run(dq, delta / ((double)Dn * eps_t), one.ft.status, 0, true, R);   // freq[i]*delta, :383-393
        if (rc == NFT_SUCCESS) {
            int hst[4] = {0, 0, 0, 0};
            be.d2h(hst, one.ft.status, sizeof(hst));
            be.d2h(q_new, one.Q12 + Dn, Dn * sizeof(cplx));      // the +delta copy
            rc = be.sync();
            if (warn_not_bandlimited) *warn_not_bandlimited = (hst[0] & 4) ? 1 : 0;
            const double inv = 1.0 / (double)Dn;                // :395-399
            if (rc == NFT_SUCCESS)
                for (size_t i = 0; i < Dn; i++) q_new[i] *= inv;
        }
        return rc;
    }

    // device-side status word -> return code (after the stream has been waited for)
    int read_status()
    {
        int h[4] = {0, 0, 0, 0}, hc[4] = {0, 0, 0, 0};
        be.d2h(h, status, sizeof(h));
        if (rich_child) be.d2h(hc, rich_child->status, sizeof(hc));
        const int rc = be.sync();
        if (rc != NFT_SUCCESS) return rc;
        // sticky bits of every transform since the last read; cleared here (off the transforms' critical path)
        be.memset0(status, 4 * sizeof(int));
        if (rich_child) be.memset0(rich_child->status, 4 * sizeof(int));
        last_warn = ((h[0] | hc[0]) & 4) ? 1 : 0;  // fnft__misc.c:371-381: not an error
        if (h[0] & 8) return NFT_EC_INVALID_ARGUMENT;   // real-coefficient path on a potential that is not real
        if (h[0] & 1) return -NFT_EC_OTHER;        // fnft__akns_fscatter.c:122-126 via CHECK_RETCODE
        if (h[0] & 2) return -NFT_EC_DIV_BY_ZERO;  // fnft_nsev.c:850-853 via CHECK_RETCODE
        // the coarse pass of the Richardson extrapolation: its step-size check and its division, after the fine pass's
        if (hc[0] & 1) return -NFT_EC_OTHER;
        if (hc[0] & 2) return -NFT_EC_DIV_BY_ZERO;
        return NFT_SUCCESS;
    }
};
