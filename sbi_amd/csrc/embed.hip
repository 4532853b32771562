// embed.hip -- C ABI of the embedding nets (include/sbi_amd_embed.h); kernels in embed_kernel.h.
#include <mutex>
#include "embed_kernel.h"

// The dynamic-LDS limit sticks to (device, kernel): raise it only when a launch needs more than any launch before it.
#define EM_CACHED_DEVICES 64
static int em_set_lds(int which, const void* kern, int lds_bytes) {
  static std::mutex lock;
  static int have[EM_CACHED_DEVICES][4];
  int dev = -1;
  const bool cached = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < EM_CACHED_DEVICES;
  std::lock_guard<std::mutex> guard(lock);
  if (cached && have[dev][which] >= lds_bytes) return 0;
  const int e = (int)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (!e && cached) have[dev][which] = lds_bytes;
  return e;
}

static bool em_rows_ok(int64_t B, int64_t T) {
  return B >= 1 && T >= 1 && B <= EM_MAX_ROWS && T <= EM_MAX_ROWS && B <= EM_MAX_ROWS / T;
}

extern "C" int64_t sbi_amd_embed_param_count(const sbi_amd_fc_embed_config* cfg, int64_t* offsets) {
  EmPlan pl;
  const int rc = em_plan_sizes(cfg, &pl);     // the count does not depend on the LDS budget
  if (rc) return rc;
  if (offsets)
    for (int l = 0; l < pl.L; ++l) {
      offsets[2 * l] = pl.off_w[l];
      offsets[2 * l + 1] = pl.off_b[l];
    }
  return pl.P;
}

extern "C" int64_t sbi_amd_embed_workspace_bytes(const sbi_amd_fc_embed_config* cfg, int64_t rows) {
  EmPlan pl;
  const int rc = em_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!em_rows_ok(rows, 1)) return SBI_AMD_E_BADARG;
  return (int64_t)em_bwd_groups(pl, rows) * pl.P * 4;
}

extern "C" int sbi_amd_embed_plan(const sbi_amd_fc_embed_config* cfg, int64_t B, int64_t T, int32_t* waves,
                                  int32_t* lds_bytes) {
  if (!cfg || B < 1 || T < 1) return SBI_AMD_E_BADARG;
  EmPlan pl;
  const int rc = em_build_plan(cfg, &pl);
  if (rc == SBI_AMD_E_BADARG || rc == SBI_AMD_E_UNSUPPORTED) return rc;
  if (T > 65535 || !em_rows_ok(B, T)) return SBI_AMD_E_UNSUPPORTED;
  if (rc) return rc;
  if (waves) *waves = EM_WAVES;
  if (lds_bytes) *lds_bytes = pl.lds_floats * 4;
  return 0;
}

static int em_launch_forward(const EmPlan& pl, const float* params, const float* x, int64_t N, float* out,
                             hipStream_t stream) {
  EmFwdArgs a = {};
  a.params = params; a.x = x; a.out = out; a.N = N;
  const int lds_bytes = pl.lds_floats * 4;
  const int e = em_set_lds(0, (const void*)em_forward_kernel<false>, lds_bytes);
  if (e) return e;
  const int64_t nchunk = (N + pl.CR - 1) / pl.CR;
  const unsigned grid = (unsigned)(nchunk < EM_FWD_GROUPS ? nchunk : EM_FWD_GROUPS);
  hipLaunchKernelGGL(em_forward_kernel<false>, dim3(grid), dim3(EM_THREADS), lds_bytes, stream, pl, a);
  return (int)hipGetLastError();
}

template <bool POOL>
static int em_launch_backward(const EmPlan& pl, EmBwdArgs a, float* grad_params, hipStream_t stream) {
  const int groups = em_bwd_groups(pl, a.N);
  const int lds_bytes = pl.lds_floats * 4;
  const int e = em_set_lds(POOL ? 3 : 2, (const void*)em_backward_kernel<POOL>, lds_bytes);
  if (e) return e;
  hipLaunchKernelGGL(em_backward_kernel<POOL>, dim3((unsigned)groups), dim3(EM_THREADS), lds_bytes, stream, pl, a);
  hipLaunchKernelGGL(em_reduce_kernel, dim3((unsigned)((pl.P + 255) / 256)), dim3(256), 0, stream,
                     (const float*)a.partial, groups, pl.P, grad_params);
  return (int)hipGetLastError();
}

extern "C" int sbi_amd_fc_embed_forward(const sbi_amd_fc_embed_config* cfg, const float* params, const float* x,
                                        int64_t N, float* out, void* stream) {
  EmPlan pl;
  const int rc = em_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!params || !x || !out || !em_rows_ok(N, 1)) return SBI_AMD_E_BADARG;
  return em_launch_forward(pl, params, x, N, out, (hipStream_t)stream);
}

extern "C" int sbi_amd_fc_embed_backward(const sbi_amd_fc_embed_config* cfg, const float* params, const float* x,
                                         int64_t N, const float* grad_out, float* grad_params, float* grad_x,
                                         void* workspace, void* stream) {
  EmPlan pl;
  const int rc = em_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!params || !x || !grad_out || !grad_params || !workspace || !em_rows_ok(N, 1)) return SBI_AMD_E_BADARG;
  EmBwdArgs a = {};
  a.params = params; a.x = x; a.grad_out = grad_out; a.grad_x = grad_x; a.partial = (float*)workspace; a.N = N;
  a.T = 1;
  return em_launch_backward<false>(pl, a, grad_params, (hipStream_t)stream);
}

static int em_perminv_plans(const sbi_amd_perminv_config* cfg, int64_t B, int64_t T, EmPlan* trial, EmPlan* head) {
  if (!cfg) return SBI_AMD_E_BADARG;
  int rc = em_build_plan(&cfg->trial, trial);
  if (rc) return rc;
  rc = em_build_plan(&cfg->head, head);
  if (rc) return rc;
  if (cfg->head.in_dim != cfg->trial.out_dim + 1 || cfg->aggregation < 0 || cfg->aggregation > 1 || B < 1 || T < 1)
    return SBI_AMD_E_BADARG;
  if (T > 65535 || !em_rows_ok(B, T)) return SBI_AMD_E_UNSUPPORTED;
  return 0;
}

extern "C" int sbi_amd_perminv_forward(const sbi_amd_perminv_config* cfg, const float* trial_params,
                                       const float* head_params, const float* x, int64_t B, int64_t T, float* out,
                                       float* head_in, void* stream) {
  EmPlan tp, hp;
  const int rc = em_perminv_plans(cfg, B, T, &tp, &hp);
  if (rc) return rc;
  if (!trial_params || !head_params || !x || !out || !head_in) return SBI_AMD_E_BADARG;
  EmFwdArgs a = {};
  a.params = trial_params; a.x = x; a.out = head_in; a.N = B * T; a.B = (int)B; a.T = (int)T;
  a.mean = cfg->aggregation;
  // elements per workgroup: at least two chunks of rows, at most EM_FWD_GROUPS workgroups
  int64_t b_per = (2 * tp.CR + T - 1) / T;
  const int64_t spread = (B + EM_FWD_GROUPS - 1) / EM_FWD_GROUPS;
  if (b_per < spread) b_per = spread;
  if (b_per > B) b_per = B;
  a.b_per = (int)b_per;
  const int lds_bytes = tp.lds_floats * 4;
  const int e = em_set_lds(1, (const void*)em_forward_kernel<true>, lds_bytes);
  if (e) return e;
  hipLaunchKernelGGL(em_forward_kernel<true>, dim3((unsigned)((B + b_per - 1) / b_per)), dim3(EM_THREADS), lds_bytes,
                     (hipStream_t)stream, tp, a);
  const int e2 = (int)hipGetLastError();
  if (e2) return e2;
  return em_launch_forward(hp, head_params, head_in, B, out, (hipStream_t)stream);
}

extern "C" int sbi_amd_perminv_backward(const sbi_amd_perminv_config* cfg, const float* trial_params,
                                        const float* head_params, const float* x, int64_t B, int64_t T,
                                        const float* head_in, const float* grad_out, float* grad_trial_params,
                                        float* grad_head_params, float* grad_head_in, void* workspace, void* stream) {
  EmPlan tp, hp;
  const int rc = em_perminv_plans(cfg, B, T, &tp, &hp);
  if (rc) return rc;
  if (!trial_params || !head_params || !x || !head_in || !grad_out || !grad_trial_params || !grad_head_params ||
      !grad_head_in || !workspace)
    return SBI_AMD_E_BADARG;
  EmBwdArgs h = {};
  h.params = head_params; h.x = head_in; h.grad_out = grad_out; h.grad_x = grad_head_in; h.partial = (float*)workspace;
  h.N = B; h.T = 1;
  const int e = em_launch_backward<false>(hp, h, grad_head_params, (hipStream_t)stream);
  if (e) return e;
  EmBwdArgs t = {};
  t.params = trial_params; t.x = x; t.grad_out = grad_head_in; t.head_in = head_in; t.partial = (float*)workspace;
  t.N = B * T; t.T = (int)T; t.mean = cfg->aggregation;
  return em_launch_backward<true>(tp, t, grad_trial_params, (hipStream_t)stream);
}
