// nsf_flow_inv.hip -- inverse (sampling) instantiations of the fused flow kernel.
#include "nsf_flow_kernel.h"

template int dispatch_flow<true>(const sbi_amd_nsf_config*, const float*, const float*, const float*, const float*,
                                 int64_t, int64_t, float*, float*, float*, float*, float*, void*, bool);
