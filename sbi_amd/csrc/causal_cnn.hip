// causal_cnn.hip -- C ABI of CausalCNNEmbedding's causal stack (include/sbi_amd_causal_cnn.h); kernels in
// causal_cnn_kernel.h.
#include <mutex>
#include "causal_cnn_kernel.h"

// The dynamic-LDS limit sticks to (device, kernel): raise it only when a launch needs more than any launch before it.
#define CC_CACHED_DEVICES 64
static int cc_set_lds(int which, const void* kern, int lds_bytes) {
  static std::mutex lock;
  static int have[CC_CACHED_DEVICES][2];
  int dev = -1;
  const bool cached = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < CC_CACHED_DEVICES;
  std::lock_guard<std::mutex> guard(lock);
  if (cached && have[dev][which] >= lds_bytes) return 0;
  const int e = (int)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (!e && cached) have[dev][which] = lds_bytes;
  return e;
}

extern "C" int64_t sbi_amd_ccnn_param_count(const sbi_amd_ccnn_config* cfg, int64_t* offsets) {
  CcPlan pl;
  const int rc = cc_plan_sizes(cfg, &pl);     // the count does not depend on the LDS budget
  if (rc) return rc;
  if (offsets)
    for (int l = 0; l < pl.L; ++l) {
      offsets[2 * l] = pl.p_w[l];
      offsets[2 * l + 1] = pl.p_b[l];
    }
  return pl.P;
}

extern "C" int sbi_amd_ccnn_plan(const sbi_amd_ccnn_config* cfg, int64_t B, int32_t* tile_steps, int32_t* lds_bytes,
                                 int32_t* fwd_lds_bytes) {
  if (!cfg || B < 1) return SBI_AMD_E_BADARG;
  CcPlan pl;
  int rc = cc_build_plan(cfg, &pl);
  if (rc && rc != SBI_AMD_E_LDS) return rc;
  const int rb = cc_check_batch(pl, B);
  if (rb) return rb;
  if (tile_steps) *tile_steps = pl.TS;
  if (lds_bytes) *lds_bytes = pl.bwd_floats * 4;
  if (fwd_lds_bytes) *fwd_lds_bytes = pl.fwd_floats * 4;
  return rc;
}

extern "C" int64_t sbi_amd_ccnn_workspace_bytes(const sbi_amd_ccnn_config* cfg, int64_t B) {
  CcPlan pl;
  int rc = cc_build_plan(cfg, &pl);
  if (rc) return rc;
  rc = cc_check_batch(pl, B);
  if (rc) return rc;
  return (int64_t)CC_GROUPS * pl.P * 4;
}

extern "C" int sbi_amd_ccnn_forward(const sbi_amd_ccnn_config* cfg, const float* params, const float* x, int64_t B,
                                    float* pooled, void* stream) {
  CcPlan pl;
  int rc = cc_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!params || !x || !pooled) return SBI_AMD_E_BADARG;
  rc = cc_check_batch(pl, B);
  if (rc) return rc;
  const int lds_bytes = pl.fwd_floats * 4;
  const int e = cc_set_lds(0, (const void*)cc_forward_kernel, lds_bytes);
  if (e) return e;
  CcArgs a = {};
  a.params = params; a.x = x; a.pooled = pooled; a.units = (long long)B * pl.nseg;
  const unsigned groups = (unsigned)(a.units < CC_FWD_GROUPS ? a.units : CC_FWD_GROUPS);
  hipLaunchKernelGGL(cc_forward_kernel, dim3(groups), dim3(CC_THREADS), lds_bytes, (hipStream_t)stream, pl, a);
  return (int)hipGetLastError();
}

extern "C" int sbi_amd_ccnn_backward(const sbi_amd_ccnn_config* cfg, const float* params, const float* x, int64_t B,
                                     const float* grad_pooled, float* grad_params, void* workspace, void* stream) {
  CcPlan pl;
  int rc = cc_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!params || !x || !grad_pooled || !grad_params || !workspace) return SBI_AMD_E_BADARG;
  rc = cc_check_batch(pl, B);
  if (rc) return rc;
  const int lds_bytes = pl.bwd_floats * 4;
  const int e = cc_set_lds(1, (const void*)cc_backward_kernel, lds_bytes);
  if (e) return e;
  CcArgs a = {};
  a.params = params; a.x = x; a.gpool = grad_pooled; a.partial = (float*)workspace; a.units = (long long)B * pl.nseg;
  const int groups = (int)(a.units < CC_GROUPS ? a.units : CC_GROUPS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_backward_kernel, dim3((unsigned)groups), dim3(CC_BWD_THREADS), lds_bytes, s, pl, a);
  hipLaunchKernelGGL(cc_reduce_kernel, dim3((unsigned)((pl.P + 255) / 256)), dim3(256), 0, s,
                     (const float*)workspace, groups, pl.P, grad_params);
  return (int)hipGetLastError();
}
