// hip_kernels_discbatch.hip -- kernel instantiations of group "discbatch" (see hip_be.h); written by gen_kernel_units.py, gfx950 only.
#define FA_HIP_RUN_IMPL
#include "hip_be.h"

FA_INST(KDsBox)
FA_INST(KDsNewton<false>)
FA_INST(KDsNewton<true>)
FA_INST(KDsFilter)
FA_INST(KDsNorm<false>)
FA_INST(KDsNorm<true>)
