// lru_embed.hip -- C ABI of LRUEmbedding's recurrent stack (include/sbi_amd_lru.h); kernels in lru_embed_kernel.h.
#include <mutex>
#include "lru_embed_kernel.h"

// The dynamic-LDS limit sticks to (device, kernel): raise it only when a launch needs more than any launch before it.
#define LR_CACHED_DEVICES 64
static int lr_set_lds(int which, const void* kern, int lds_bytes) {
  static std::mutex lock;
  static int have[LR_CACHED_DEVICES][2];
  int dev = -1;
  const bool cached = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < LR_CACHED_DEVICES;
  std::lock_guard<std::mutex> guard(lock);
  if (cached && have[dev][which] >= lds_bytes) return 0;
  const int e = (int)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (!e && cached) have[dev][which] = lds_bytes;
  return e;
}

// workspace layout in floats: the block inputs h_0 .. h_{NB-1}, the states; backward: the gradient map, the forward
// half's state gradients, the workgroups' partial gradients, their sum before the chain rules
struct LrWorkspace {
  long long maps, xs, gmap, dxs, partial, raw, floats;
};

static LrWorkspace lr_workspace(const LrPlan& pl, int64_t B, int64_t T, bool backward) {
  LrWorkspace w = {};
  const long long rows = (long long)B * T;
  long long o = 0;
  w.maps = o; o += (long long)pl.NB * rows * pl.H;
  w.xs = o; o += rows * pl.W2;
  if (backward) {
    w.gmap = o; o += rows * pl.H;
    w.dxs = o; o += rows * pl.W2;
    w.partial = o; o += (long long)lr_groups(B) * pl.P;
    w.raw = o; o += pl.P;
  }
  w.floats = o;
  return w;
}

extern "C" int64_t sbi_amd_lru_param_count(const sbi_amd_lru_config* cfg, int64_t* offsets) {
  LrPlan pl;
  const int rc = lr_plan_sizes(cfg, &pl);     // the count does not depend on the LDS budget
  if (rc) return rc;
  if (offsets) {
    offsets[0] = 0;
    for (int i = 0; i < pl.NB; ++i) offsets[1 + i] = pl.off_blk0 + (int64_t)i * pl.PB;
  }
  return pl.P;
}

extern "C" int sbi_amd_lru_plan(const sbi_amd_lru_config* cfg, int64_t B, int64_t T, int32_t* lds_bytes,
                                int32_t* fwd_lds_bytes) {
  if (!cfg || B < 1 || T < 1) return SBI_AMD_E_BADARG;
  LrPlan pl;
  int rc = lr_plan_sizes(cfg, &pl);
  if (rc) return rc;
  rc = lr_check_rows(B, T);
  if (rc) return rc;
  if (lds_bytes) *lds_bytes = (int32_t)(pl.bwd_floats * 4);
  if (fwd_lds_bytes) *fwd_lds_bytes = (int32_t)(pl.fwd_floats * 4);
  return pl.bwd_floats * 4 <= LR_LDS_BUDGET ? 0 : SBI_AMD_E_LDS;
}

extern "C" int64_t sbi_amd_lru_workspace_bytes(const sbi_amd_lru_config* cfg, int64_t B, int64_t T, int32_t backward) {
  LrPlan pl;
  int rc = lr_build_plan(cfg, &pl);
  if (rc) return rc;
  rc = lr_check_rows(B, T);
  if (rc) return rc;
  return lr_workspace(pl, B, T, backward != 0).floats * 4;
}

// h_0 and the blocks 0 .. upto - 1 (all: the last one writes the features)
static int lr_run_forward(const LrPlan& pl, const LrWorkspace& w, const float* params, const float* x, int64_t B,
                          int64_t T, float* features, float* ws, int upto, hipStream_t stream) {
  const long long rows = (long long)B * T, map = rows * pl.H;
  const int lds_bytes = (int)pl.fwd_floats * 4;
  const int e = lr_set_lds(0, (const void*)lr_block_kernel<false>, lds_bytes);
  if (e) return e;
  hipLaunchKernelGGL(lr_input_kernel, dim3((unsigned)((map + 255) / 256)), dim3(256), 0, stream, params, x,
                     ws + w.maps, rows, pl.I, pl.H);
  for (int blk = 0; blk < upto; ++blk) {
    LrArgs a = {};
    a.params = params; a.x = x; a.B = (int)B; a.T = (int)T; a.blk = blk;
    a.in = ws + w.maps + blk * map;
    a.out = blk + 1 < pl.NB ? ws + w.maps + (blk + 1) * map : nullptr;
    a.features = features;
    a.xs = ws + w.xs;
    hipLaunchKernelGGL(lr_block_kernel<false>, dim3((unsigned)lr_groups(B)), dim3(LR_THREADS), lds_bytes, stream, pl,
                       a);
  }
  return (int)hipGetLastError();
}

extern "C" int sbi_amd_lru_forward(const sbi_amd_lru_config* cfg, const float* params, const float* x, int64_t B,
                                   int64_t T, float* features, void* workspace, void* stream) {
  LrPlan pl;
  int rc = lr_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!params || !x || !features || !workspace || B < 1 || T < 1) return SBI_AMD_E_BADARG;
  rc = lr_check_rows(B, T);
  if (rc) return rc;
  const LrWorkspace w = lr_workspace(pl, B, T, false);
  return lr_run_forward(pl, w, params, x, B, T, features, (float*)workspace, pl.NB, (hipStream_t)stream);
}

extern "C" int sbi_amd_lru_backward(const sbi_amd_lru_config* cfg, const float* params, const float* x, int64_t B,
                                    int64_t T, const float* grad_features, float* grad_params, void* workspace,
                                    void* stream) {
  LrPlan pl;
  int rc = lr_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!params || !x || !grad_features || !grad_params || !workspace || B < 1 || T < 1) return SBI_AMD_E_BADARG;
  rc = lr_check_rows(B, T);
  if (rc) return rc;
  const LrWorkspace w = lr_workspace(pl, B, T, true);
  float* ws = (float*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const int lds_bytes = (int)pl.bwd_floats * 4;
  int e = lr_set_lds(1, (const void*)lr_block_kernel<true>, lds_bytes);
  if (e) return e;
  e = lr_run_forward(pl, w, params, x, B, T, nullptr, ws, pl.NB - 1, s);      // the inputs of every block
  if (e) return e;
  const long long map = (long long)B * T * pl.H;
  const int groups = lr_groups(B);
  for (int blk = pl.NB - 1; blk >= 0; --blk) {
    LrArgs a = {};
    a.params = params; a.x = x; a.B = (int)B; a.T = (int)T; a.blk = blk;
    a.in = ws + w.maps + blk * map;
    a.xs = ws + w.xs; a.dxs = ws + w.dxs; a.gmap = ws + w.gmap;
    a.gfeat = grad_features;
    a.partial = ws + w.partial;
    hipLaunchKernelGGL(lr_block_kernel<true>, dim3((unsigned)groups), dim3(LR_THREADS), lds_bytes, s, pl, a);
  }
  hipLaunchKernelGGL(lr_reduce_kernel, dim3((unsigned)((pl.P + 255) / 256)), dim3(256), 0, s,
                     (const float*)(ws + w.partial), groups, pl.P, ws + w.raw);
  hipLaunchKernelGGL(lr_chain_kernel, dim3((unsigned)((pl.P + 255) / 256)), dim3(256), 0, s, pl, params,
                     (const float*)(ws + w.raw), grad_params);
  return (int)hipGetLastError();
}
