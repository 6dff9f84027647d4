// hip_kernels_discroots.hip -- kernel instantiations of group "discroots" (see hip_be.h); written by gen_kernel_units.py, gfx950 only.
#define FA_HIP_RUN_IMPL
#include "hip_be.h"

FA_INST(KDsGather)
FA_INST(KAberthBStart)
FA_INST(KAberthBNewton)
FA_INST(KAberthBSum)
FA_INST(KAberthBApply)
FA_INST(KAberthBStep)
FA_INST(KDsCandidates)
