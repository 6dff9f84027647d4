// hip_kernels_realcol.hip -- kernel instantiations of group "realcol" (see hip_be.h); written by gen_kernel_units.py, gfx950 only.
#define FA_HIP_RUN_IMPL
#include "hip_be.h"

FA_INST(KRColFwd<4>)
FA_INST(KRColFwd<4096>)
FA_INST(KRColInv<4>)
FA_INST(KRColInv<8>)
FA_INST(KRColInv<16>)
FA_INST(KRColInv<32>)
FA_INST(KRColInv<64>)
FA_INST(KRColInv<128>)
FA_INST(KRColInv<256>)
FA_INST(KRColInv<512>)
FA_INST(KRColInv<1024>)
FA_INST(KRColInv<2048>)
FA_INST(KRColInv<4096>)
