// hip_kernels_slow.hip -- kernel instantiations of group "slow" (see hip_be.h); written by gen_kernel_units.py, gfx950 only.
#define FA_HIP_RUN_IMPL
#include "hip_be.h"

FA_INST(KSlowPrep)
FA_INST(KSlowScatter<0, true>)
FA_INST(KSlowScatter<0, false>)
FA_INST(KSlowScatter<1, false>)
FA_INST(KSlowScatter<2, false>)
FA_INST(KSlowReduce)
FA_INST(KSlowCombine)
