// lc2st.hip -- C ABI of the L-C2ST classifier ensemble (include/sbi_amd_lc2st.h); kernels in lc2st_kernel.h.
#include "lc2st_kernel.h"

static int lc_set_lds(const void* kern, int lds_bytes) {
  return (int)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
}

extern "C" int64_t sbi_amd_lc2st_param_count(const sbi_amd_lc2st_config* cfg) {
  LcPlan pl;
  const int rc = lc_build_plan(cfg, &pl);
  return rc ? rc : pl.P;
}

extern "C" int sbi_amd_lc2st_train_epochs(const sbi_amd_lc2st_config* cfg, const float* data, int64_t R,
                                          const int32_t* rows, const float* labels, int64_t row_stride,
                                          const int32_t* n_train, const int32_t* n_valid, const int32_t* member_id,
                                          int64_t M, uint64_t seed, float* params, float* best_params, float* exp_avg,
                                          float* exp_avg_sq, int32_t* step, float* best, int32_t* misses, int32_t* epoch,
                                          int32_t* best_epoch, int32_t* stopped, float* history,
                                          int32_t epochs_this_launch, void* stream) {
  LcPlan pl;
  const int rc = lc_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!data || !rows || !labels || !n_train || !n_valid || !member_id || !params || !best_params || !exp_avg ||
      !exp_avg_sq || !step || !best || !misses || !epoch || !best_epoch || !stopped || !history)
    return SBI_AMD_E_BADARG;
  if (R < 1 || R > 0x7fffffffll || row_stride < 2 || row_stride > 0x7fffffffll || M < 0 || M > 0x7fffffffll ||
      epochs_this_launch < 1)
    return SBI_AMD_E_BADARG;
  if (M == 0) return 0;
  LcArgs a = {};
  a.data = data; a.R = R; a.rows = rows; a.labels = labels; a.row_stride = row_stride;
  a.n_train = n_train; a.n_valid = n_valid; a.member_id = member_id;
  a.seed_lo = (unsigned)seed; a.seed_hi = (unsigned)(seed >> 32);
  a.params = params; a.best_params = best_params; a.exp_avg = exp_avg; a.exp_avg_sq = exp_avg_sq;
  a.step = step; a.best = best; a.misses = misses; a.epoch = epoch; a.best_epoch = best_epoch; a.stopped = stopped;
  a.history = history; a.epochs = epochs_this_launch;
  const int lds_bytes = pl.lds_floats * 4;
  const int e = lc_set_lds((const void*)lc_train_kernel, lds_bytes);
  if (e) return e;
  hipLaunchKernelGGL(lc_train_kernel, dim3((unsigned)M), dim3(LC_THREADS), lds_bytes, (hipStream_t)stream, pl, a);
  return (int)hipGetLastError();
}

extern "C" int sbi_amd_lc2st_batch_grad(const sbi_amd_lc2st_config* cfg, const float* data, int64_t R,
                                        const int32_t* rows, const float* labels, int64_t row_stride,
                                        const int32_t* n_train, const int32_t* n_valid, const int32_t* member_id,
                                        int64_t M, uint64_t seed, const float* params, int32_t which, int32_t epoch,
                                        int32_t batch, float* loss_out, float* grad_out, void* stream) {
  LcPlan pl;
  const int rc = lc_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!data || !rows || !labels || !n_train || !n_valid || !member_id || !params || !loss_out || !grad_out)
    return SBI_AMD_E_BADARG;
  if (R < 1 || R > 0x7fffffffll || row_stride < 2 || row_stride > 0x7fffffffll || M < 0 || M > 0x7fffffffll ||
      which < 0 || which > 1 || epoch < 0 || batch < 0 || (int64_t)batch * pl.B > 0x7fffffffll)
    return SBI_AMD_E_BADARG;
  if (M == 0) return 0;
  LcArgs a = {};
  a.data = data; a.R = R; a.rows = rows; a.labels = labels; a.row_stride = row_stride;
  a.n_train = n_train; a.n_valid = n_valid; a.member_id = member_id;
  a.seed_lo = (unsigned)seed; a.seed_hi = (unsigned)(seed >> 32);
  a.params_in = params; a.which = which; a.g_epoch = epoch; a.g_batch = batch; a.loss_out = loss_out;
  a.grad_out = grad_out;
  const int lds_bytes = pl.lds_floats * 4;
  const int e = lc_set_lds((const void*)lc_grad_kernel, lds_bytes);
  if (e) return e;
  hipLaunchKernelGGL(lc_grad_kernel, dim3((unsigned)M), dim3(LC_THREADS), lds_bytes, (hipStream_t)stream, pl, a);
  return (int)hipGetLastError();
}

extern "C" int sbi_amd_lc2st_eval(const sbi_amd_lc2st_config* cfg, const float* params, const float* theta,
                                  const float* x_o, int64_t n, int64_t M, int32_t group_size, int32_t theta_groups,
                                  float* proba_out, float* score_out, void* stream) {
  LcPlan pl;
  const int rc = lc_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!params || !theta || !x_o || !proba_out || !score_out) return SBI_AMD_E_BADARG;
  if (n < 1 || n > (1ll << 24) || M < 1 || group_size < 1 || M % group_size != 0) return SBI_AMD_E_BADARG;
  const int64_t groups = M / group_size;
  if (groups > 65535 || (theta_groups != 1 && theta_groups != groups)) return SBI_AMD_E_BADARG;
  const int lds_bytes = pl.lds_floats * 4;
  const int e = lc_set_lds((const void*)lc_eval_kernel, lds_bytes);
  if (e) return e;
  const unsigned blocks = (unsigned)((n + LC_EVAL_ROWS - 1) / LC_EVAL_ROWS);
  hipLaunchKernelGGL(lc_eval_kernel, dim3(blocks, (unsigned)groups), dim3(LC_THREADS), lds_bytes, (hipStream_t)stream,
                     pl, params, theta, x_o, (long long)n, (int)group_size, (int)theta_groups, proba_out);
  hipLaunchKernelGGL(lc_score_kernel, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream,
                     (const float*)proba_out, (long long)n, score_out);
  return (int)hipGetLastError();
}
