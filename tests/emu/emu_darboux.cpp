// emu_darboux.cpp -- builds tests/emu/libfnft_emu_darboux.so: the batched discrete part of the inverse transform
// (NftInverseDiscBatch: KInvDsPrep, KInvSolitons, the eigenfunction launches of nft_bs_eigenfunctions, KInvCdt) in the CPU
// lane emulator, executing AND recording the launches (TEST INFRASTRUCTURE ONLY; see emu_backend.h).
#include "emu_backend.h"

thread_local fa_emu_ctx *fa_emu = nullptr;

#include "../../fnft_amd/csrc/nft_nsev_inverse.h"

struct NamedBackend : EmuBackend {
    std::vector<std::string> names;
    template <class K> void run(int gx, int gy, const typename K::Params &p)
    {
        names.push_back(emu_kernel_name<K>());
        EmuBackend::run<K>(gx, gy, p);
    }
};

extern "C" {

// init, check_and_sort and run on host arrays (the emulator's "device" memory is the heap): bs, nc: B*K values as the
// caller passes them; q: B*D samples, the seed on entry in mode 1; status: B words, zeroed here; names: the launches
int emu_darboux(size_t D, size_t B, size_t K, int mode, int residues, const cplx *bs, const cplx *nc, cplx *q,
                const double *T, int *status, char *names, size_t cap)
{
    NamedBackend be;
    int rc;
    {
        NftInverseDiscBatch<NamedBackend> ds(be, D, B, K, mode, residues != 0, false);
        rc = ds.init();
        if (rc == NFT_SUCCESS) {
            std::memset(status, 0, B * sizeof(int));
            ds.check_and_sort(bs, nc, status);
            ds.run(q, T, status);
        }
    }
    std::string s;
    for (const auto &n : be.names) s += n + "\n";
    if (s.size() + 1 > cap) return -1;
    std::memcpy(names, s.c_str(), s.size() + 1);
    return rc;
}

}  // extern "C"
