// emu_handover.cpp -- builds tests/emu/libfnft_emu_handover.so: fnft_amd_plan's transform (run_front, run_tree,
// run_contspec, run_contspec_tm, export_tm) in the CPU lane emulator with the tree -> chirp hand-over of the root
// switched on or off, executing AND recording the launches (TEST INFRASTRUCTURE ONLY; see emu_backend.h).
#include "emu_backend.h"

thread_local fa_emu_ctx *fa_emu = nullptr;

#include "../../fnft_amd/csrc/nft_plan.h"

// the emulator's back end that also keeps the name of every launch, in order
struct NamedBackend : EmuBackend {
    std::vector<std::string> names;
    template <class K> void run(int gx, int gy, const typename K::Params &p)
    {
        names.push_back(emu_kernel_name<K>());
        EmuBackend::run<K>(gx, gy, p);
    }
};

extern "C" {

// `batch` signals of D samples, nse discretization `disc`, M points, contspec type `cstype` (cs_len = M, 2M, 3M
// complex numbers per signal).
//   mode 0: run_front, run_tree, run_contspec, export_tm -- everything executed; q: batch*D, XI: 2; contspec
//           (batch*cs_len), tm (batch*4*(deg+1), the layout of fnft_amd_plan_get_transfer_matrix) and W (batch) are filled
//   mode 1: run_front, run_tree, export_tm in schedule-only mode (nothing executed, the outputs untouched)
//   mode 2: another signal on the same plan.  q: two signal sets (2*batch*D), XI: two grids (4).  Three transforms
//           (run_front, run_tree, run_contspec) on ONE plan -- set 0 on grid 0, set 1 on grid 0 (the filter spectrum is
//           cached: v_mode 2), set 1 on grid 1 (a miss) -- then export_tm; contspec holds the three outputs
//           (3*batch*cs_len), tm and W are those of the last transform
//   mode 3: a caller's matrix in between.  One transform of q, then run_contspec_tm on tm_in (batch*4*(deg+1)) with
//           exponent W_in on the same grids, then export_tm; contspec holds both outputs (2*batch*cs_len), tm and W are
//           the plan's own
//   mode 4: run_contspec_tm on tm_in / W_in alone, on a plan that never ran its tree; contspec (batch*cs_len) is filled
// fuse: NftPlan::tune_fuse_root.  names: the launches, '\n'-separated, with a line "--contspec" in front of the launches
// of every run_contspec / run_contspec_tm and "--export" in front of export_tm's.  Returns the plan's rc, or -1 if names
// does not fit cap.
int emu_handover(size_t D, size_t M, size_t batch, int disc, int kappa, int cstype, int fuse, int mode, const cplx *q,
                 const double *T, const double *XI, const cplx *tm_in, int W_in, cplx *contspec, cplx *tm, int *W,
                 char *names, size_t cap)
{
    NamedBackend be;
    using P = NftPlan<NamedBackend>;
    const int akns = nft_nse_to_akns(disc);
    if (akns < 0 || cstype < 0 || cstype > 2 || mode < 0 || mode > 4) return NFT_EC_INVALID_ARGUMENT;
    const int ups = nft_nse_upsampling(disc);
    std::vector<std::string> discard;
    if (mode == 1) emu_schedule = &discard;
    int rc;
    {
        P pl(be, (size_t)ups * D, M, batch, akns, nft_akns_degree(akns));
        pl.set_front(D, 1, ups);
        pl.tune_fuse_root = fuse;
        rc = pl.init();
        const size_t cs_len = (size_t)(cstype + 1) * M;
        const size_t nset = mode == 2 ? 2 : 1, nout = mode == 2 ? 3 : mode == 3 ? 2 : 1;
        const size_t tm_len = batch * 4 * (D * (size_t)ups * (size_t)nft_akns_degree(akns) + 1);
        cplx *dq = (cplx *)be.alloc(nset * batch * D * sizeof(cplx));
        cplx *dcs = (cplx *)be.alloc(nout * batch * cs_len * sizeof(cplx));
        cplx *dtm = (mode >= 3) ? (cplx *)be.alloc(tm_len * sizeof(cplx)) : nullptr;
        if (mode != 1 && mode != 4) be.h2d(dq, q, nset * batch * D * sizeof(cplx));
        if (dtm) be.h2d(dtm, tm_in, tm_len * sizeof(cplx));
        P::Contspec cs;
        cs.nse_disc = disc; cs.cstype = cstype; cs.normalization_flag = 1;
        // the transforms: (signal set, grid) of each
        const int seq[3][2] = {{0, 0}, {1, 0}, {1, 1}};
        const size_t ntrans = mode == 4 ? 0 : mode == 2 ? 3 : 1;
        for (size_t t = 0; t < ntrans && rc == NFT_SUCCESS; t++) {
            double Tsub[2];
            rc = pl.run_front(dq + (size_t)seq[t][0] * batch * D, T, kappa, Tsub);
            if (rc == NFT_SUCCESS) rc = pl.run_tree();
            if (rc == NFT_SUCCESS && mode != 1) {
                be.names.push_back("--contspec");
                cs.T[0] = Tsub[0]; cs.T[1] = Tsub[1];
                cs.XI[0] = XI[2 * seq[t][1]]; cs.XI[1] = XI[2 * seq[t][1] + 1];
                rc = pl.run_contspec(dcs + t * batch * cs_len, cs);
            }
        }
        if (rc == NFT_SUCCESS && mode >= 3) {
            be.names.push_back("--contspec");
            cs.T[0] = T[0]; cs.T[1] = T[1]; cs.XI[0] = XI[0]; cs.XI[1] = XI[1];
            rc = pl.run_contspec_tm(dcs + (nout - 1) * batch * cs_len, cs, dtm, W_in);
        }
        if (rc == NFT_SUCCESS && mode != 4) {
            be.names.push_back("--export");
            pl.export_tm();
        }
        if (rc == NFT_SUCCESS && mode != 1) rc = pl.read_status();
        if (rc == NFT_SUCCESS && mode != 1) {
            be.d2h(contspec, dcs, nout * batch * cs_len * sizeof(cplx));
            if (mode != 4) {
                be.d2h(tm, pl.tm_out, batch * 4 * (pl.res_deg + 1) * sizeof(cplx));
                be.d2h(W, pl.wexp[pl.cur], batch * sizeof(int));
            }
        }
        be.free(dq);
        be.free(dcs);
        if (dtm) be.free(dtm);
    }
    emu_schedule = nullptr;
    std::string s;
    for (const auto &n : be.names) s += n + "\n";
    if (s.size() + 1 > cap) return -1;
    std::memcpy(names, s.c_str(), s.size() + 1);
    return rc;
}

}  // extern "C"
