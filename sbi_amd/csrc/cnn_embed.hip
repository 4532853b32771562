// cnn_embed.hip -- C ABI of CNNEmbedding's convolution stack (include/sbi_amd_cnn.h); kernels in cnn_embed_kernel.h.
#include <mutex>
#include "cnn_embed_kernel.h"

// The dynamic-LDS limit sticks to (device, kernel): raise it only when a launch needs more than any launch before it.
#define CN_CACHED_DEVICES 64
static int cn_set_lds(int which, const void* kern, int lds_bytes) {
  static std::mutex lock;
  static int have[CN_CACHED_DEVICES][12];
  int dev = -1;
  const bool cached = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < CN_CACHED_DEVICES;
  std::lock_guard<std::mutex> guard(lock);
  if (cached && have[dev][which] >= lds_bytes) return 0;
  const int e = (int)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (!e && cached) have[dev][which] = lds_bytes;
  return e;
}

static bool cn_batch_ok(int64_t B) { return B >= 1 && B <= CN_MAX_BATCH; }

static int32_t cn_saturate(long long v) { return (int32_t)(v > 0x7fffffffll ? 0x7fffffffll : v); }

extern "C" int64_t sbi_amd_cnn_param_count(const sbi_amd_cnn_config* cfg, int64_t* offsets) {
  CnPlan pl;
  const int rc = cn_plan_sizes(cfg, &pl);     // the count does not depend on the LDS budget
  if (rc) return rc;
  if (offsets)
    for (int l = 0; l < pl.L; ++l) {
      offsets[2 * l] = pl.ly[l].off_w;
      offsets[2 * l + 1] = pl.ly[l].off_b;
    }
  return pl.P;
}

extern "C" int64_t sbi_amd_cnn_feature_count(const sbi_amd_cnn_config* cfg) {
  CnPlan pl;
  const int rc = cn_plan_sizes(cfg, &pl);
  if (rc) return rc;
  return pl.F64;
}

extern "C" int sbi_amd_cnn_plan(const sbi_amd_cnn_config* cfg, int64_t B, int32_t* lds_bytes, int32_t* fwd_lds_bytes) {
  if (!cfg || B < 1) return SBI_AMD_E_BADARG;
  CnPlan pl;
  const int rc = cn_plan_sizes(cfg, &pl);
  if (rc) return rc;
  if (!cn_batch_ok(B)) return SBI_AMD_E_UNSUPPORTED;
  if (lds_bytes) *lds_bytes = cn_saturate(pl.bwd_floats * 4);
  if (fwd_lds_bytes) *fwd_lds_bytes = cn_saturate(pl.fwd_floats * 4);
  return pl.bwd_floats * 4 <= CN_LDS_BUDGET ? 0 : SBI_AMD_E_LDS;
}

extern "C" int64_t sbi_amd_cnn_workspace_bytes(const sbi_amd_cnn_config* cfg, int64_t B) {
  CnPlan pl;
  const int rc = cn_build_plan(cfg, &pl);
  if (rc) return rc;
  if (B < 1) return SBI_AMD_E_BADARG;
  if (!cn_batch_ok(B)) return SBI_AMD_E_UNSUPPORTED;
  return (int64_t)cn_groups(B) * pl.P * 4;
}

template <int PH, int PW>
static int cn_launch(int which, bool backward, const CnPlan& pl, const CnArgs& a, float* grad_params,
                     hipStream_t stream) {
  const int groups = cn_groups(a.B);
  if (!backward) {
    const int lds_bytes = (int)pl.fwd_floats * 4;
    const int e = cn_set_lds(which, (const void*)cn_forward_kernel<PH, PW>, lds_bytes);
    if (e) return e;
    hipLaunchKernelGGL((cn_forward_kernel<PH, PW>), dim3((unsigned)groups), dim3(CN_THREADS), lds_bytes, stream, pl, a);
    return (int)hipGetLastError();
  }
  const int lds_bytes = (int)pl.bwd_floats * 4;
  const int e = cn_set_lds(6 + which, (const void*)cn_backward_kernel<PH, PW>, lds_bytes);
  if (e) return e;
  hipLaunchKernelGGL((cn_backward_kernel<PH, PW>), dim3((unsigned)groups), dim3(CN_THREADS), lds_bytes, stream, pl, a);
  hipLaunchKernelGGL(cn_reduce_kernel, dim3((unsigned)((pl.P + 255) / 256)), dim3(256), 0, stream,
                     (const float*)a.partial, groups, pl.P, grad_params);
  return (int)hipGetLastError();
}

// one instantiation per pool window: (1, pk) in 1-D, (pk, pk) in 2-D
static int cn_dispatch(bool backward, const CnPlan& pl, const CnArgs& a, float* grad_params, hipStream_t stream) {
  if (pl.PH == 1) {
    if (pl.PW == 2) return cn_launch<1, 2>(0, backward, pl, a, grad_params, stream);
    if (pl.PW == 3) return cn_launch<1, 3>(1, backward, pl, a, grad_params, stream);
    return cn_launch<1, 4>(2, backward, pl, a, grad_params, stream);
  }
  if (pl.PW == 2) return cn_launch<2, 2>(3, backward, pl, a, grad_params, stream);
  if (pl.PW == 3) return cn_launch<3, 3>(4, backward, pl, a, grad_params, stream);
  return cn_launch<4, 4>(5, backward, pl, a, grad_params, stream);
}

extern "C" int sbi_amd_cnn_forward(const sbi_amd_cnn_config* cfg, const float* params, const float* x, int64_t B,
                                   float* features, void* stream) {
  CnPlan pl;
  const int rc = cn_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!params || !x || !features || B < 1) return SBI_AMD_E_BADARG;
  if (!cn_batch_ok(B)) return SBI_AMD_E_UNSUPPORTED;
  CnArgs a = {};
  a.params = params; a.x = x; a.features = features; a.B = B;
  return cn_dispatch(false, pl, a, nullptr, (hipStream_t)stream);
}

extern "C" int sbi_amd_cnn_backward(const sbi_amd_cnn_config* cfg, const float* params, const float* x, int64_t B,
                                    const float* grad_features, float* grad_params, void* workspace, void* stream) {
  CnPlan pl;
  const int rc = cn_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!params || !x || !grad_features || !grad_params || !workspace || B < 1) return SBI_AMD_E_BADARG;
  if (!cn_batch_ok(B)) return SBI_AMD_E_UNSUPPORTED;
  CnArgs a = {};
  a.params = params; a.x = x; a.grad_features = grad_features; a.partial = (float*)workspace; a.B = B;
  return cn_dispatch(true, pl, a, grad_params, (hipStream_t)stream);
}
