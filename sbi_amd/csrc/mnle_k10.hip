// mnle_k10.hip -- num_bins = 10 instantiations of the MNLE kernels (separate translation unit: parallel build)
#include "mnle_kernel.h"
template int mnle_dispatch_k<10>(const MnlePlan&, const MnleCall&, hipStream_t);
