// nsf_trials.hip -- log-likelihood of iid trials summed per condition (NLE's potential), C ABI
// sbi_amd_nsf_log_prob_trials.  Replaces the reference's _log_likelihoods_over_trials
// (sbi/inference/potentials/likelihood_based_potential.py:186-236), which expands x_o to (num_trials, num_theta, D),
// evaluates every pair and sums over the trials.  Here nothing is materialised: the density kernels read the trials and
// the conditions in place (row r = theta r / num_trials, trial r % num_trials: nsf_flow_kernel<..., TRI> and
// nsf_coop_fwd_kernel<..., TRI>), store one value per row, and a second launch sums each theta's trials in a fixed order.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include "nsf_flow_kernel.h"
#include "nsf_coop_host.h"

// One wave per condition: lane l accumulates trials l, l + 64, ... in fp64, then a fixed butterfly over the lanes.  The
// order of the additions depends on the trial index alone -- not on where the condition's rows sit in the launch -- so a
// permutation of the conditions permutes the sums bit for bit, and no float atomics are involved.
__global__ void __launch_bounds__(256)
nsf_trials_sum_kernel(const float* __restrict__ rows, long long num_trials, long long num_theta,
                      float* __restrict__ out) {
  const long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= num_theta) return;      // (whole waves: the shuffles below see all 64 lanes of a live wave)
  const float* r = rows + c * num_trials;
  double acc = 0.0;
  for (long long i = lane; i < num_trials; i += 64) acc += (double)r[i];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
  if (lane == 0) out[c] = (float)acc;
}

// the throughput kernel with the paired call's routing (dispatch_flow<false>, no stash): same plan, same layout
// specialisation, so every row runs the arithmetic sbi_amd_nsf_log_prob runs at the same row count
template <int K>
static int launch_trials_flow(const NsfPlan& pl, int nw, const float* packed, const float* zstats, const float* x_trials,
                              const float* theta, int64_t n, int64_t num_trials, float* rows, hipStream_t st) {
  if constexpr (K == 10) {
    if (nw == 8 && flow_plan_is_static(pl, kStaticFlow8))
      return launch_flow<10, 13, false, 8, false, true, 1, true>(pl, nw, packed, zstats, x_trials, theta, n, num_trials,
                                                                 rows, nullptr, nullptr, nullptr, nullptr, st);
  }
  if (pl.KSH == 13)
    return launch_flow<K, 13, false, 0, false, true, 1, true>(pl, nw, packed, zstats, x_trials, theta, n, num_trials, rows,
                                                              nullptr, nullptr, nullptr, nullptr, st);
  return launch_flow<K, 16, false, 0, false, true, 1, true>(pl, nw, packed, zstats, x_trials, theta, n, num_trials, rows,
                                                            nullptr, nullptr, nullptr, nullptr, st);
}

// rows of a call, or SBI_AMD_E_*: the wide (hidden > 64) family has no trials mode
static int64_t trials_rows(const sbi_amd_nsf_config* cfg, int64_t num_trials, int64_t num_theta) {
  if (!cfg || num_trials < 1 || num_theta < 0) return SBI_AMD_E_BADARG;
  NsfPlan pl;
  int rc = nsf_build_plan(cfg, 1, &pl);
  if (rc && rc != SBI_AMD_E_LDS) return rc;
  if (pl.H > 16 * NSF_HT) return SBI_AMD_E_UNSUPPORTED;
  if (num_theta > 4ll * 0x7fffffff || (num_theta > 0 && num_trials > INT64_MAX / 4 / num_theta)) return SBI_AMD_E_BADARG;
  return num_trials * num_theta;
}

extern "C" int64_t sbi_amd_nsf_log_prob_trials_workspace_floats(const sbi_amd_nsf_config* cfg, int64_t num_trials,
                                                                int64_t num_theta) {
  return trials_rows(cfg, num_trials, num_theta);
}

extern "C" int sbi_amd_nsf_log_prob_trials(const sbi_amd_nsf_config* cfg, const float* packed, const float* zstats,
                                           const float* x_trials, int64_t num_trials, const float* theta,
                                           int64_t num_theta, float* loglik_out, float* row_logp_out, float* workspace,
                                           void* stream) {
  const int64_t n = trials_rows(cfg, num_trials, num_theta);
  if (n < 0) return (int)n;
  if (n == 0) return 0;
  if (!packed || !zstats || !x_trials || !theta || !loglik_out || (!row_logp_out && !workspace)) return SBI_AMD_E_BADARG;
  float* rows = row_logp_out ? row_logp_out : workspace;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  NsfPlan pl;
  CoopPlan cp;
  if (n == 1) {         // one pair: exactly the paired call (which may fold the single condition row)
    rc = sbi_amd_nsf_log_prob(cfg, packed, zstats, x_trials, theta, 1, 1, rows, nullptr, stream);
  } else if (coop_applies(cfg, n, false, &pl, &cp)) {      // the routing rule of sbi_amd_nsf_log_prob
    rc = coop_log_prob_trials(cfg, pl, cp, packed + nsf_packed_floats(pl), zstats, x_trials, num_trials, theta, n, rows,
                              stream);
  } else {
    int nw = 0;
    rc = nsf_plan_for_rows(cfg, n, &pl, &nw, false);
    if (!rc)
      rc = nsf_with_bins(cfg->K, [&](auto k) {
        return launch_trials_flow<k>(pl, nw, packed, zstats, x_trials, theta, n, num_trials, rows, st);
      });
  }
  if (rc) return rc;
  hipLaunchKernelGGL(nsf_trials_sum_kernel, dim3((unsigned)((num_theta + 3) / 4)), dim3(256), 0, st, (const float*)rows,
                     (long long)num_trials, (long long)num_theta, loglik_out);
  return (int)hipGetLastError();
}
