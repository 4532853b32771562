// mnle_k8.hip -- num_bins = 8 instantiations of the MNLE kernels (separate translation unit: parallel build)
#include "mnle_kernel.h"
template int mnle_dispatch_k<8>(const MnlePlan&, const MnleCall&, hipStream_t);
