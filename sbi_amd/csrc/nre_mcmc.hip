// nre_mcmc.hip -- persistent slice sampler on the NRE ratio classifier, one lane per chain (sbi_amd_nre_mcmc_slice_run).
//
// Batched MCMC runs `chains_per_x` chains for each of `num_x` observations (chain c belongs to observation
// c / chains_per_x).  The classifier kernel evaluates one (theta, x) pair per lane (nre_kernel.h), so a lane can own a
// chain outright: it computes W_x z_x + b of its observation once, and then for `nticks` ticks alternates
//   log r(theta_c, x_b) + log p(theta_c)   (the fma sequence of nre_forward_kernel<HP, false, false>, the box prior's constant)
// with slice_tick_one (mcmc_tick.h) on its own state.  Nothing is exchanged between lanes and nothing returns to the
// host between the ticks of a launch; the weights are wave-uniform scalar loads through the constant address space.
// Lanes of a wave sit in different states of the slice state machine, but all of them evaluate the network: the
// divergence is confined to the few instructions of the tick.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/sbi_amd_nsf.h"
#include "nre_kernel.h"
// mcmc_tick.h switches floating-point contraction off for its own bracket arithmetic and back to the compiler's default
// (fast) at its end: everything below it in this file contracts as the rest of the library does.  The logit is written
// with explicit fmaf and does not depend on the setting.
#include "mcmc_tick.h"

namespace {

constexpr int kMaxChains = 1 << 24;   // int32 state indices (4 c, 8 c) and one lane per chain

template <int HP>
__global__ void __launch_bounds__(256)
nre_mcmc_slice_run_kernel(NreDims d, const float* __restrict__ pk_, const float* __restrict__ zs_,
                          const float* __restrict__ xs, int C, int chains_per_x, int num_samples, int tuning,
                          float max_width, float* x, float* next_param, float* width, int* order, int* istate,
                          float* fstate, float* samples, int* done_count, unsigned long long seed,
                          unsigned long long tick0, int nticks, const float* __restrict__ tp0,
                          const float* __restrict__ tp1, const float* __restrict__ low, const float* __restrict__ high,
                          float prior_lp, float* theta_next, float* lad_next, float* logp_scratch) {
  const nre_cfloat* pk = nre_const(pk_);
  const nre_cfloat* zs = nre_const(zs_);
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  if (istate[4 * c] == ST_DONE) return;
  float hx[HP];
  nre_x_part<HP>(d, pk, zs, xs + (size_t)(c / chains_per_x) * d.C, hx);
  const float* th = theta_next + (size_t)c * d.D;
  for (int t = 0; t < nticks; ++t) {
    if (istate[4 * c] == ST_DONE) break;
    const float lg = nre_logit_from_x_part<HP>(d, pk, zs, th, hx);
    // BoxUniform.log_prob: one constant on [low, high), -inf elsewhere (a theta that rounded onto the upper bound included)
    bool inside = true;
    for (int k = 0; k < d.D; ++k) inside = inside && (th[k] >= low[k]) && (th[k] < high[k]);
    logp_scratch[c] = lg + (inside ? prior_lp : -INFINITY);
    slice_tick_one(c, d.D, num_samples, tuning, max_width, logp_scratch, lad_next, nullptr, x, next_param, width, order,
                   istate, fstate, samples, done_count, seed, tick0 + (unsigned long long)t, 2, tp0, tp1, theta_next,
                   lad_next);
  }
}

template <int HP>
int launch(const NreDims& d, int wg, const float* pk, const float* zs, const float* xs, int C, int chains_per_x,
           int num_samples, int tuning, float max_width, float* x, float* next_param, float* width, int* order,
           int* istate, float* fstate, float* samples, int* done_count, uint64_t seed, uint64_t tick0, int nticks,
           const float* p0, const float* p1, const float* low, const float* high, float prior_lp, float* theta_next,
           float* lad_next, float* logp_scratch, hipStream_t st) {
  hipLaunchKernelGGL(nre_mcmc_slice_run_kernel<HP>, dim3((unsigned)((C + wg - 1) / wg)), dim3(wg), 0, st, d, pk, zs, xs, C,
                     chains_per_x, num_samples, tuning, max_width, x, next_param, width, order, istate, fstate, samples,
                     done_count, (unsigned long long)seed, (unsigned long long)tick0, nticks, p0, p1, low, high, prior_lp,
                     theta_next, lad_next, logp_scratch);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int sbi_amd_nre_mcmc_slice_run(const sbi_amd_nre_config* cfg, const float* packed, const float* zstats,
                                          const float* x_obs, int32_t num_x, int32_t chains_per_x, int32_t num_samples,
                                          int32_t tuning, float max_width, float* x, float* next_param, float* width,
                                          int32_t* order, int32_t* istate, float* fstate, float* samples,
                                          int32_t* done_count, uint64_t seed, uint64_t tick0, int32_t nticks,
                                          int32_t kind, const float* p0, const float* p1, const float* prior_low,
                                          const float* prior_high, float prior_log_prob, float* theta_next,
                                          float* logabsdet_next, float* logp_scratch, int32_t wg_size, void* stream) {
  if (!cfg) return SBI_AMD_E_BADARG;
  if (cfg->D < 1 || cfg->C < 1 || cfg->H < 1 || cfg->NB < 1) return SBI_AMD_E_BADARG;
  if (cfg->D > 64 || cfg->C > 128 || cfg->H > 64 || cfg->NB > 4) return SBI_AMD_E_UNSUPPORTED;
  if (num_x < 1 || chains_per_x < 1 || num_samples < 0 || tuning < 0 || nticks < 1 || kind < 0 || kind > 2)
    return SBI_AMD_E_BADARG;
  if (wg_size != 0 && wg_size != 64 && wg_size != 128 && wg_size != 256) return SBI_AMD_E_BADARG;
  // only a box prior under the logit map: its log-density is one constant inside the support
  if (kind != 2) return SBI_AMD_E_UNSUPPORTED;
  if ((int64_t)num_x * chains_per_x > kMaxChains) return SBI_AMD_E_UNSUPPORTED;
  if (!packed || !zstats || !x_obs || !x || !next_param || !width || !order || !istate || !fstate || !samples ||
      !done_count || !p0 || !p1 || !prior_low || !prior_high || !theta_next || !logabsdet_next || !logp_scratch)
    return SBI_AMD_E_BADARG;
  NreDims d{cfg->D, cfg->C, cfg->H, cfg->NB, 0};
  d.HS = d.H > 48 && d.H <= 56 ? 56 : (d.H + 15) / 16 * 16;
  const int C = num_x * chains_per_x;
  const int wg = wg_size ? wg_size : 64;
  hipStream_t st = (hipStream_t)stream;
#define NRE_MCMC_LAUNCH(HP)                                                                                              \
  return launch<HP>(d, wg, packed, zstats, x_obs, C, chains_per_x, num_samples, tuning, max_width, x, next_param, width, \
                    order, istate, fstate, samples, done_count, seed, tick0, nticks, p0, p1, prior_low, prior_high,      \
                    prior_log_prob, theta_next, logabsdet_next, logp_scratch, st)
  switch (d.HS) {
    case 16: NRE_MCMC_LAUNCH(16);
    case 32: NRE_MCMC_LAUNCH(32);
    case 48: NRE_MCMC_LAUNCH(48);
    case 56: NRE_MCMC_LAUNCH(56);
    default: NRE_MCMC_LAUNCH(64);
  }
#undef NRE_MCMC_LAUNCH
}
