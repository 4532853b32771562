// mnle_k16.hip -- num_bins = 16 instantiations of the MNLE kernels (separate translation unit: parallel build)
#include "mnle_kernel.h"
template int mnle_dispatch_k<16>(const MnlePlan&, const MnleCall&, hipStream_t);
