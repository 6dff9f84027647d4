// emu_polyeval.cpp -- builds tests/emu/libfnft_emu_polyeval.so: the polynomial evaluation kernels (KPolyEval, KPolyJoin)
// and fnft_amd_nsev_eval_device's plan logic (NftPlan::run_eval) in the CPU lane emulator, executing AND recording the
// launches (TEST INFRASTRUCTURE ONLY; see emu_backend.h).
#include "emu_backend.h"

thread_local fa_emu_ctx *fa_emu = nullptr;

#include "../../fnft_amd/csrc/nft_plan.h"

struct NamedBackend : EmuBackend {
    std::vector<std::string> names;
    template <class K> void run(int gx, int gy, const typename K::Params &p)
    {
        names.push_back(emu_kernel_name<K>());
        EmuBackend::run<K>(gx, gy, p);
    }
};

static int put_names(const std::vector<std::string> &v, char *names, size_t cap)
{
    std::string s;
    for (const auto &n : v) s += n + "\n";
    if (s.size() + 1 > cap) return -1;
    std::memcpy(names, s.c_str(), s.size() + 1);
    return 0;
}

extern "C" {

// polyeval_device on host arrays (the emulator's "device" memory is the heap): the arguments of
// fnft_amd_poly_eval_device, force_S > 0 the number of segments (0: the host logic's choice).  seg receives S and L.
int emu_polyeval(size_t deg, size_t npoly, size_t batch, const cplx *p, size_t pstride, size_t bstride, size_t nz,
                 const cplx *z, size_t zstride, cplx *val, cplx *deriv, int force_S, long long *seg)
{
    EmuBackend be;
    const PolyEvalSegs sg = polyeval_segments(deg, nz, batch * npoly, EmuBackend::kTargetWorkgroups, force_S);
    seg[0] = sg.S;
    seg[1] = sg.L;
    return polyeval_device(be, deg, npoly, batch, p, pstride, bstride, nz, z, zstride, val, deriv, force_S);
}

// polyeval_segments and polyeval_partials for a back end whose launches aim at `target` workgroups (the HIP back end:
// 2048): out = {S, L, partials per array a plan keeps for calls of up to nz points}
void emu_polyeval_sizes(size_t deg, size_t nz, size_t jobs, size_t target, long long *out)
{
    const PolyEvalSegs sg = polyeval_segments(deg, nz, jobs, target, 0);
    out[0] = sg.S;
    out[1] = sg.L;
    out[2] = (long long)polyeval_partials(deg, nz, jobs, target, 0);
}

// One transform of `batch` signals of D samples (run_front, run_tree, run_contspec of type AB when M > 0), then
// run_eval `reps` times at the n points per signal of lam (lam_stride as in fnft_amd_nsev_eval_device), then export_tm.
// out: batch * (deriv ? 4 : 2) * n; contspec: batch * 2 * M (M > 0); tm: batch * 4 * (deg + 1), W: batch -- the plan's own
// exported matrix.  names: the launches, with "--contspec", "--eval" (one per repetition) and "--export" lines in front
// of the respective parts.
int emu_nsev_eval(size_t D, size_t M, size_t batch, int disc, int kappa, const cplx *q, const double *T,
                  const double *XI, const cplx *lam, size_t n, size_t lam_stride, int deriv, int force_S, int reps,
                  cplx *out, cplx *contspec, cplx *tm, int *W, char *names, size_t cap)
{
    NamedBackend be;
    using P = NftPlan<NamedBackend>;
    const int akns = nft_nse_to_akns(disc);
    if (akns < 0) return NFT_EC_INVALID_ARGUMENT;
    const int ups = nft_nse_upsampling(disc);
    int rc;
    {
        P pl(be, (size_t)ups * D, M, batch, akns, nft_akns_degree(akns));
        pl.set_front(D, 1, ups);
        rc = pl.init();
        double Tsub[2];
        if (rc == NFT_SUCCESS) rc = pl.run_front(q, T, kappa, Tsub);
        if (rc == NFT_SUCCESS) rc = pl.run_tree();
        if (rc == NFT_SUCCESS && M > 0) {
            be.names.push_back("--contspec");
            P::Contspec cs;
            cs.nse_disc = disc; cs.cstype = 1; cs.normalization_flag = 1;
            cs.T[0] = Tsub[0]; cs.T[1] = Tsub[1]; cs.XI[0] = XI[0]; cs.XI[1] = XI[1];
            rc = pl.run_contspec(contspec, cs);
        }
        for (int r = 0; r < reps && rc == NFT_SUCCESS; r++) {
            be.names.push_back("--eval");
            rc = pl.run_eval(T, disc, lam, n, lam_stride, deriv != 0, out, force_S);
        }
        if (rc == NFT_SUCCESS) {
            be.names.push_back("--export");
            pl.export_tm();
            rc = pl.read_status();
        }
        if (rc == NFT_SUCCESS) {
            be.d2h(tm, pl.tm_out, batch * 4 * (pl.res_deg + 1) * sizeof(cplx));
            be.d2h(W, pl.wexp[pl.cur], batch * sizeof(int));
        }
    }
    if (put_names(be.names, names, cap) != 0) return -1;
    return rc;
}

// the names of FA_EXT_UNITS (nft_kernel_list.h; which = 1) or of FA_ALL_UNITS (which = 0, what emu_main.cpp's
// emu_kernel_list prints), '\n'-separated; returns their number
int emu_ext_kernel_list(int which, char *out, size_t cap)
{
    std::vector<std::string> v;
#define FA_EMU_NAME(...) v.push_back(emu_kernel_name<__VA_ARGS__>());
    if (which) { FA_EXT_UNITS(FA_EMU_NAME) }
    else { FA_ALL_UNITS(FA_EMU_NAME) }
#undef FA_EMU_NAME
    if (put_names(v, out, cap) != 0) return -1;
    return (int)v.size();
}

}  // extern "C"
