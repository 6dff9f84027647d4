#define FA_HIP_RUN_IMPL
#include "hip_be.h"
FA_UNIT_richardson(FA_INST)   // nft_kernel_list.h
