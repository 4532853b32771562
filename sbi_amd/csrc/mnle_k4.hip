// mnle_k4.hip -- num_bins = 4 instantiations of the MNLE kernels (separate translation unit: parallel build)
#include "mnle_kernel.h"
template int mnle_dispatch_k<4>(const MnlePlan&, const MnleCall&, hipStream_t);
