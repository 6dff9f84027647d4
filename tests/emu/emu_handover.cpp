// emu_handover.cpp -- builds tests/emu/libfnft_emu_handover.so: fnft_amd_plan's transform (run_front, run_tree,
// run_contspec, export_tm) in the CPU lane emulator with the tree -> chirp hand-over of the root switched on or off,
// executing AND recording the launches (TEST INFRASTRUCTURE ONLY; see emu_backend.h).
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

// `batch` signals of D samples (q: batch*D), nse discretization `disc`, M points, contspec type BOTH.
//   mode 0: run_front, run_tree, run_contspec, export_tm -- everything executed; contspec (batch*3*M), tm (batch*4*(deg+1),
//           the layout of fnft_amd_plan_get_transfer_matrix) and W (batch) are filled
//   mode 1: run_front, run_tree, export_tm in schedule-only mode (nothing executed, the outputs untouched)
// fuse: NftPlan::tune_fuse_root.  names: the launches, '\n'-separated, with the lines "--contspec" and "--export" in front
// of the launches of those two steps.  Returns the plan's rc, or -1 if names does not fit cap.
int emu_handover(size_t D, size_t M, size_t batch, int disc, int kappa, int fuse, int mode, const cplx *q,
                 const double *T, const double *XI, cplx *contspec, cplx *tm, int *W, char *names, size_t cap)
{
    NamedBackend be;
    using P = NftPlan<NamedBackend>;
    const int akns = nft_nse_to_akns(disc);
    if (akns < 0) return NFT_EC_INVALID_ARGUMENT;
    const int ups = nft_nse_upsampling(disc);
    std::vector<std::string> discard;
    if (mode == 1) emu_schedule = &discard;
    int rc;
    {
        P pl(be, (size_t)ups * D, M, batch, akns, nft_akns_degree(akns));
        pl.set_front(D, 1, ups);
        pl.tune_fuse_root = fuse;
        rc = pl.init();
        const size_t cs_len = 3 * M;
        cplx *dq = (cplx *)be.alloc(batch * D * sizeof(cplx));
        cplx *dcs = (cplx *)be.alloc(batch * cs_len * sizeof(cplx));
        if (mode == 0) be.h2d(dq, q, batch * D * sizeof(cplx));
        double Tsub[2];
        if (rc == NFT_SUCCESS) rc = pl.run_front(dq, T, kappa, Tsub);
        if (rc == NFT_SUCCESS) rc = pl.run_tree();
        if (rc == NFT_SUCCESS && mode == 0) {
            be.names.push_back("--contspec");
            P::Contspec cs;
            cs.T[0] = Tsub[0]; cs.T[1] = Tsub[1]; cs.XI[0] = XI[0]; cs.XI[1] = XI[1];
            cs.nse_disc = disc; cs.cstype = 2; cs.normalization_flag = 1;
            rc = pl.run_contspec(dcs, cs);
        }
        if (rc == NFT_SUCCESS) {
            be.names.push_back("--export");
            pl.export_tm();
        }
        if (rc == NFT_SUCCESS && mode == 0) rc = pl.read_status();
        if (rc == NFT_SUCCESS && mode == 0) {
            be.d2h(contspec, dcs, batch * cs_len * sizeof(cplx));
            be.d2h(tm, pl.tm_out, batch * 4 * (pl.res_deg + 1) * sizeof(cplx));
            be.d2h(W, pl.wexp[pl.cur], batch * sizeof(int));
        }
        be.free(dq);
        be.free(dcs);
    }
    emu_schedule = nullptr;
    std::string s;
    for (const auto &n : be.names) s += n + "\n";
    if (s.size() + 1 > cap) return -1;
    std::memcpy(names, s.c_str(), s.size() + 1);
    return rc;
}

}  // extern "C"
