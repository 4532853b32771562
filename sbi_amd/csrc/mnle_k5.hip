// mnle_k5.hip -- num_bins = 5 instantiations of the MNLE kernels (separate translation unit: parallel build)
#include "mnle_kernel.h"
template int mnle_dispatch_k<5>(const MnlePlan&, const MnleCall&, hipStream_t);
