// fmpe.hip -- C ABI of the FMPE (flow matching) path (include/sbi_amd_fmpe.h); the kernels live in fmpe_kernel.h.
#include "fmpe_kernel.h"

extern "C" {

int64_t sbi_amd_fmpe_param_count(const sbi_amd_fmpe_config* cfg) {
  FmPlan pl;
  int rc = fm_build_plan(cfg, &pl);
  return rc ? rc : pl.P;
}

int64_t sbi_amd_fmpe_param_offset(const sbi_amd_fmpe_config* cfg, int32_t kind, int32_t layer) {
  FmPlan pl;
  int rc = fm_build_plan(cfg, &pl);
  if (rc) return rc;
  if (layer < 0 || layer >= pl.L) return SBI_AMD_E_BADARG;
  switch (kind) {
    case 0: return pl.lin[J_IN].g_w;
    case 1: return pl.lin[J_IN].g_b;
    case 2: return pl.lin[J_CT].g_w;
    case 3: return pl.lin[J_CT].g_b;
    case 4: return pl.lin[J_MA].g_w;
    case 5: return pl.lin[J_MA].g_b;
    case 6: return pl.lin[J_TM].g_w;
    case 7: return pl.lin[J_TM].g_b;
    case 8: return pl.lin[J_L0 + layer].g_w;
    case 9: return pl.lin[J_L0 + layer].g_b;
    case 10: return pl.g_ln + layer * 2 * pl.H;
    case 11: return pl.g_ln + layer * 2 * pl.H + pl.H;
    case 12: return pl.lin[J_L0 + pl.L].g_w;
    case 13: return pl.lin[J_L0 + pl.L].g_b;
    default: return SBI_AMD_E_BADARG;
  }
}

int64_t sbi_amd_fmpe_packed_floats(const sbi_amd_fmpe_config* cfg) {
  FmPlan pl;
  int rc = fm_build_plan(cfg, &pl);
  return rc ? rc : pl.packed_floats;
}

int sbi_amd_fmpe_pack(const sbi_amd_fmpe_config* cfg, const float* params, float* packed, void* stream) {
  FmPlan pl;
  int rc = fm_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!params || !packed) return SBI_AMD_E_BADARG;
  hipLaunchKernelGGL(fm_pack_kernel, dim3(pl.NL, 8), dim3(256), 0, (hipStream_t)stream, pl, params, packed);
  return (int)hipGetLastError();
}

int sbi_amd_fmpe_velocity(const sbi_amd_fmpe_config* cfg, const float* packed, const float* zstats,
                          const float* theta_t, const float* x, int64_t x_rows, const float* times,
                          int64_t t_rows, int64_t n, float* v_out, void* stream) {
  FmPlan pl;
  int rc = fm_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!packed || !zstats || !theta_t || !x || !times || !v_out || n < 0) return SBI_AMD_E_BADARG;
  if ((x_rows != 1 && x_rows != n) || (t_rows != 1 && t_rows != n)) return SBI_AMD_E_BADARG;
  if (n == 0) return 0;
  FmArgs a;
  memset(&a, 0, sizeof(a));
  a.packed = packed; a.zstats = zstats; a.theta = theta_t; a.x = x; a.times = times; a.n = n;
  a.x_rows = (int)(x_rows == 1 ? 1 : 2); a.t_rows = (int)(t_rows == 1 ? 1 : 2);
  if (n == 1) { a.x_rows = 1; a.t_rows = 1; }
  a.v_out = v_out; a.ntiles = (int)((n + FM_ROWS - 1) / FM_ROWS);
  return fm_launch_fwd<0>(pl, a, (hipStream_t)stream);
}

int sbi_amd_fmpe_velocity_div(const sbi_amd_fmpe_config* cfg, const float* packed, const float* zstats,
                              const float* theta_t, const float* x, int64_t x_rows, const float* times,
                              int64_t t_rows, int64_t n, float* v_out, float* div_out, void* stream) {
  FmPlan pl;
  int rc = fm_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!packed || !zstats || !theta_t || !x || !times || !div_out || n < 0) return SBI_AMD_E_BADARG;
  if ((x_rows != 1 && x_rows != n) || (t_rows != 1 && t_rows != n)) return SBI_AMD_E_BADARG;
  if (n == 0) return 0;
  FmArgs a;
  memset(&a, 0, sizeof(a));
  a.packed = packed; a.zstats = zstats; a.theta = theta_t; a.x = x; a.times = times; a.n = n;
  a.x_rows = (int)(x_rows == 1 ? 1 : 2); a.t_rows = (int)(t_rows == 1 ? 1 : 2);
  if (n == 1) { a.x_rows = 1; a.t_rows = 1; }
  a.v_out = v_out; a.div_out = div_out; a.ntiles = (int)((n + FM_WAVES - 1) / FM_WAVES);
  return fm_launch_div(pl, a, (hipStream_t)stream);
}

int sbi_amd_fmpe_loss(const sbi_amd_fmpe_config* cfg, const float* packed, const float* zstats, const float* theta,
                      const float* x, int64_t x_rows, const float* times, const float* noise, int64_t n,
                      float* loss_out, void* stream) {
  FmPlan pl;
  int rc = fm_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!packed || !zstats || !theta || !x || !times || !noise || !loss_out || n < 0) return SBI_AMD_E_BADARG;
  if (x_rows != 1 && x_rows != n) return SBI_AMD_E_BADARG;
  if (n == 0) return 0;
  FmArgs a;
  memset(&a, 0, sizeof(a));
  a.packed = packed; a.zstats = zstats; a.theta = theta; a.x = x; a.times = times; a.noise = noise; a.n = n;
  a.x_rows = (x_rows == 1 || n == 1) ? 1 : 2; a.t_rows = n == 1 ? 1 : 2;
  a.loss_out = loss_out; a.ntiles = (int)((n + FM_ROWS - 1) / FM_ROWS);
  return fm_launch_fwd<1>(pl, a, (hipStream_t)stream);
}

int64_t sbi_amd_fmpe_train_workspace_floats(const sbi_amd_fmpe_config* cfg, int64_t n) {
  FmPlan pl;
  int rc = fm_build_plan(cfg, &pl);
  if (rc) return rc;
  if (n <= 0) return SBI_AMD_E_BADARG;
  return fm_ws_layout(pl, n).total;
}

int sbi_amd_fmpe_loss_fwd_bwd(const sbi_amd_fmpe_config* cfg, const float* params, const float* packed,
                              const float* zstats, const float* theta, const float* x, int64_t x_rows,
                              const float* times, const float* noise, int64_t n, const float* row_weight,
                              float uniform_weight, float* loss_out, float* grad_out, float* workspace,
                              void* stream) {
  FmPlan pl;
  int rc = fm_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!params || !packed || !zstats || !theta || !x || !times || !noise || !loss_out || !grad_out || !workspace ||
      n <= 0)
    return SBI_AMD_E_BADARG;
  if (x_rows != 1 && x_rows != n) return SBI_AMD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const FmWs w = fm_ws_layout(pl, n);
  FmArgs a;
  memset(&a, 0, sizeof(a));
  a.packed = packed; a.zstats = zstats; a.theta = theta; a.x = x; a.times = times; a.noise = noise; a.n = n;
  a.x_rows = (x_rows == 1 || n == 1) ? 1 : 2; a.t_rows = n == 1 ? 1 : 2;
  a.row_weight = row_weight; a.uniform_weight = uniform_weight;
  a.loss_out = loss_out; a.stash = workspace + w.stash; a.ln_part = workspace + w.ln_part; a.ntiles = w.ntiles;
  static long long* tl_dev = nullptr;
  if (sbi_amd_dbg_fm_timeline()) {
    if (!tl_dev) { hipMalloc(&tl_dev, 8 * 32 * 8); }
    hipMemsetAsync(tl_dev, 0, 8 * 32 * 8, st);
    a.timeline = tl_dev;
  }
  rc = fm_launch_fwd<2>(pl, a, st);
  if (rc) return rc;
  if (a.timeline) {
    static int shown = 0;
    if (++shown == 20) {
      long long h[8 * 32];
      hipStreamSynchronize(st);
      hipMemcpy(h, tl_dev, sizeof(h), hipMemcpyDeviceToHost);
      for (int it = 0; it < 3; ++it) {
        fprintf(stderr, "fwd timeline tile-iter %d:", it);
        for (int k = 1; k < 32 && h[it * 32 + k]; ++k) fprintf(stderr, " %lld", h[it * 32 + k] - h[it * 32 + k - 1]);
        fprintf(stderr, "\n");
      }
    }
    a.timeline = nullptr;
  }
  return fm_backward_all(pl, a, w, params, grad_out, workspace, st);
}

}  // extern "C"
