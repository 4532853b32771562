// sc_embed.hip -- C ABI of SpectralConvEmbedding (include/sbi_amd_sc.h); kernels in sc_embed_kernel.h.
#include <mutex>
#include "sc_embed_kernel.h"

// The dynamic-LDS limit sticks to (device, kernel): raise it only when a launch needs more than any launch before it.
#define SC_CACHED_DEVICES 64
static int sc_set_lds(int which, const void* kern, int lds_bytes) {
  static std::mutex lock;
  static int have[SC_CACHED_DEVICES][2];
  int dev = -1;
  const bool cached = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < SC_CACHED_DEVICES;
  std::lock_guard<std::mutex> guard(lock);
  if (cached && have[dev][which] >= lds_bytes) return 0;
  const int e = (int)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (!e && cached) have[dev][which] = lds_bytes;
  return e;
}

extern "C" int64_t sbi_amd_sc_param_count(const sbi_amd_sc_config* cfg, int64_t* offsets) {
  ScPlan pl;
  const int rc = sc_plan_sizes(cfg, &pl);
  if (rc) return rc;
  if (offsets) {
    int n = 0;
    offsets[n++] = pl.p_fc0w;
    offsets[n++] = pl.p_fc0b;
    for (int l = 0; l < pl.L; ++l) offsets[n++] = pl.p_conv[l];
    for (int l = 0; l < pl.L; ++l) {
      offsets[n++] = pl.p_ww[l];
      offsets[n++] = pl.p_wb[l];
    }
    offsets[n++] = pl.p_last;
    offsets[n++] = pl.p_flw;
    offsets[n++] = pl.p_flb;
  }
  return pl.P;
}

extern "C" int sbi_amd_sc_plan(const sbi_amd_sc_config* cfg, int64_t B, int32_t* lds_bytes, int32_t* fwd_lds_bytes,
                               int32_t* parts) {
  if (!cfg || B < 1) return SBI_AMD_E_BADARG;
  ScPlan pl;
  const int rc = sc_build_plan(cfg, &pl);
  if (rc && rc != SBI_AMD_E_LDS) return rc;
  const int rb = sc_check_batch(pl, B);
  if (rb) return rb;
  if (lds_bytes) *lds_bytes = pl.bwd_floats * 4;
  if (fwd_lds_bytes) *fwd_lds_bytes = pl.fwd_floats * 4;
  if (parts) *parts = pl.parts;
  return rc;
}

extern "C" int64_t sbi_amd_sc_workspace_bytes(const sbi_amd_sc_config* cfg, int64_t B) {
  ScPlan pl;
  int rc = sc_build_plan(cfg, &pl);
  if (rc) return rc;
  rc = sc_check_batch(pl, B);
  if (rc) return rc;
  return (B < SC_GROUPS ? B : SC_GROUPS) * (int64_t)pl.P * 4;
}

static int sc_check_views(const ScPlan& pl, const float* x, int64_t xbs, int64_t xcs, const float* pos, int64_t pbs) {
  if (!x || xbs < 0 || xcs < 0 || pbs < 0) return SBI_AMD_E_BADARG;
  if (pl.pos ? !pos : pos != nullptr) return SBI_AMD_E_BADARG;
  return 0;
}

extern "C" int sbi_amd_sc_forward(const sbi_amd_sc_config* cfg, const float* params, const float* x,
                                  int64_t x_batch_stride, int64_t x_channel_stride, const float* positions,
                                  int64_t pos_batch_stride, int64_t B, float* out, void* stream) {
  ScPlan pl;
  int rc = sc_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!params || !out) return SBI_AMD_E_BADARG;
  rc = sc_check_views(pl, x, x_batch_stride, x_channel_stride, positions, pos_batch_stride);
  if (rc) return rc;
  rc = sc_check_batch(pl, B);
  if (rc) return rc;
  const int lds_bytes = pl.fwd_floats * 4;
  const int e = sc_set_lds(0, (const void*)sc_forward_kernel, lds_bytes);
  if (e) return e;
  ScArgs a = {};
  a.params = params; a.x = x; a.pos = positions; a.xbs = x_batch_stride; a.xcs = x_channel_stride;
  a.pbs = pos_batch_stride; a.out = out; a.B = B;
  const unsigned groups = (unsigned)(B < SC_GROUPS ? B : SC_GROUPS);      // two resident workgroups per CU
  hipLaunchKernelGGL(sc_forward_kernel, dim3(groups), dim3(SC_THREADS), lds_bytes, (hipStream_t)stream, pl, a);
  return (int)hipGetLastError();
}

extern "C" int sbi_amd_sc_backward(const sbi_amd_sc_config* cfg, const float* params, const float* x,
                                   int64_t x_batch_stride, int64_t x_channel_stride, const float* positions,
                                   int64_t pos_batch_stride, int64_t B, const float* grad_out, float* grad_params,
                                   void* workspace, void* stream) {
  ScPlan pl;
  int rc = sc_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!params || !grad_out || !grad_params || !workspace) return SBI_AMD_E_BADARG;
  rc = sc_check_views(pl, x, x_batch_stride, x_channel_stride, positions, pos_batch_stride);
  if (rc) return rc;
  rc = sc_check_batch(pl, B);
  if (rc) return rc;
  const int lds_bytes = pl.bwd_floats * 4;
  const int e = sc_set_lds(1, (const void*)sc_backward_kernel, lds_bytes);
  if (e) return e;
  ScArgs a = {};
  a.params = params; a.x = x; a.pos = positions; a.xbs = x_batch_stride; a.xcs = x_channel_stride;
  a.pbs = pos_batch_stride; a.gout = grad_out; a.partial = (float*)workspace; a.B = B;
  const int groups = (int)(B < SC_GROUPS ? B : SC_GROUPS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sc_backward_kernel, dim3((unsigned)groups), dim3(SC_THREADS), lds_bytes, s, pl, a);
  hipLaunchKernelGGL(sc_reduce_kernel, dim3((unsigned)((pl.P + 255) / 256)), dim3(256), 0, s,
                     (const float*)workspace, groups, pl.P, grad_params);
  return (int)hipGetLastError();
}
