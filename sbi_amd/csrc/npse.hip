// npse.hip -- C ABI of the NPSE (score estimation) path (include/sbi_amd_npse.h).
//
// The score network is the FMPE vector-field MLP, so the kernels are the templates of fmpe_kernel.h: MODE 3 (score /
// ode_fn), 4 / 5 (denoising-score-matching loss without / with the activation stash) and 6 (the Euler-Maruyama
// sampler) of fm_fwd_kernel add the SDE-dependent prologue and epilogue to the shared trunk; the backward, weight-
// gradient and reduce kernels run as they are.
//
// The control variate's second forward (the net at the un-noised mean m theta) is scheduled as a SECOND COLUMN OF THE
// SAME WAVE: with the control variate on, a wave's 16 MFMA columns hold 8 rows twice (columns 0..7 noised, 8..15 at the
// mean).  Both evaluations of a row share its x and t loads, the weight fragments and the LDS staging; term1 reaches its
// row by one cross-lane exchange, and the stash keeps the usual [16 columns] blocks, so the backward and weight-gradient
// kernels see nothing but a batch of 2n columns (mean columns of rows above the threshold carry a zero gradient).  With
// the control variate off (threshold <= 0) a wave holds 16 rows as on the FMPE path.
#include "fmpe_kernel.h"
#include "../../include/sbi_amd_npse.h"
#include "../../include/sbi_amd_npse_iid.h"
#include "npse_iid_kernel.h"

namespace {

int np_build_plan(const sbi_amd_npse_config* cfg, FmPlan* pl) {
  if (!cfg) return SBI_AMD_E_BADARG;
  int rc = fm_build_plan(&cfg->net, pl);
  if (rc) return rc;
  if (cfg->sde < 0 || cfg->sde > 2 || cfg->weight < 0 || cfg->weight > 2) return SBI_AMD_E_UNSUPPORTED;
  if (cfg->sde == 0 && !(cfg->sigma_min > 0.f && cfg->sigma_max > cfg->sigma_min)) return SBI_AMD_E_BADARG;
  pl->sde = cfg->sde; pl->wfn = cfg->weight;
  pl->beta_min = cfg->beta_min; pl->beta_d = cfg->beta_max - cfg->beta_min;
  pl->sig_min = cfg->sigma_min;
  pl->log_sig_ratio = cfg->sde == 0 ? logf(cfg->sigma_max / cfg->sigma_min) : 0.f;
  pl->cv_thr = cfg->cv_threshold;
  return 0;
}

// rows per workgroup: 128, or 64 when every row takes two columns
long long np_columns(const sbi_amd_npse_config* cfg, long long n) { return cfg->cv_threshold > 0.f ? 2 * n : n; }

void np_loss_args(const sbi_amd_npse_config* cfg, FmArgs* a, const float* packed, const float* zstats, const float* theta,
                  const float* x, int64_t x_rows, const float* times, const float* eps, int64_t n, float* loss_out) {
  memset(a, 0, sizeof(*a));
  a->packed = packed; a->zstats = zstats; a->theta = theta; a->x = x; a->times = times; a->noise = eps; a->n = n;
  a->x_rows = (x_rows == 1 || n == 1) ? 1 : 2; a->t_rows = n == 1 ? 1 : 2;
  a->loss_out = loss_out;
  a->pair = cfg->cv_threshold > 0.f ? 1 : 0;
  a->ntiles = (int)((np_columns(cfg, n) + FM_ROWS - 1) / FM_ROWS);
}

}  // namespace

extern "C" {

int sbi_amd_npse_score(const sbi_amd_npse_config* cfg, const float* packed, const float* zstats, const float* theta_t,
                       const float* x, int64_t x_rows, const float* times, int64_t t_rows, int64_t n, int32_t ode,
                       float* out, void* stream) {
  FmPlan pl;
  int rc = np_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!packed || !zstats || !theta_t || !x || !times || !out || n < 0) return SBI_AMD_E_BADARG;
  if ((x_rows != 1 && x_rows != n) || (t_rows != 1 && t_rows != n)) return SBI_AMD_E_BADARG;
  if (n == 0) return 0;
  FmArgs a;
  memset(&a, 0, sizeof(a));
  a.packed = packed; a.zstats = zstats; a.theta = theta_t; a.x = x; a.times = times; a.n = n;
  a.x_rows = (int)(x_rows == 1 ? 1 : 2); a.t_rows = (int)(t_rows == 1 ? 1 : 2);
  if (n == 1) { a.x_rows = 1; a.t_rows = 1; }
  a.ode = ode ? 1 : 0;
  a.v_out = out; a.ntiles = (int)((n + FM_ROWS - 1) / FM_ROWS);
  return fm_launch_fwd<3>(pl, a, (hipStream_t)stream);
}

int sbi_amd_npse_loss(const sbi_amd_npse_config* cfg, const float* packed, const float* zstats, const float* theta,
                      const float* x, int64_t x_rows, const float* times, const float* eps, int64_t n,
                      float* loss_out, void* stream) {
  FmPlan pl;
  int rc = np_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!packed || !zstats || !theta || !x || !times || !eps || !loss_out || n < 0) return SBI_AMD_E_BADARG;
  if (x_rows != 1 && x_rows != n) return SBI_AMD_E_BADARG;
  if (n == 0) return 0;
  FmArgs a;
  np_loss_args(cfg, &a, packed, zstats, theta, x, x_rows, times, eps, n, loss_out);
  return fm_launch_fwd<4>(pl, a, (hipStream_t)stream);
}

int64_t sbi_amd_npse_train_workspace_floats(const sbi_amd_npse_config* cfg, int64_t n) {
  FmPlan pl;
  int rc = np_build_plan(cfg, &pl);
  if (rc) return rc;
  if (n <= 0) return SBI_AMD_E_BADARG;
  return fm_ws_layout(pl, np_columns(cfg, n)).total;
}

int sbi_amd_npse_loss_fwd_bwd(const sbi_amd_npse_config* cfg, const float* params, const float* packed,
                              const float* zstats, const float* theta, const float* x, int64_t x_rows,
                              const float* times, const float* eps, int64_t n, const float* row_weight,
                              float uniform_weight, float* loss_out, float* grad_out, float* workspace, void* stream) {
  FmPlan pl;
  int rc = np_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!params || !packed || !zstats || !theta || !x || !times || !eps || !loss_out || !grad_out || !workspace || n <= 0)
    return SBI_AMD_E_BADARG;
  if (x_rows != 1 && x_rows != n) return SBI_AMD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const FmWs w = fm_ws_layout(pl, np_columns(cfg, n));
  FmArgs a;
  np_loss_args(cfg, &a, packed, zstats, theta, x, x_rows, times, eps, n, loss_out);
  a.row_weight = row_weight; a.uniform_weight = uniform_weight;
  a.stash = workspace + w.stash; a.ln_part = workspace + w.ln_part;
  rc = fm_launch_fwd<5>(pl, a, st);
  if (rc) return rc;
  return fm_backward_all(pl, a, w, params, grad_out, workspace, st);
}

int sbi_amd_npse_sample_sde(const sbi_amd_npse_config* cfg, const float* packed, const float* zstats,
                            const float* base, const float* x, int64_t x_rows, const float* ts, int32_t steps,
                            float eta, const float* noise, uint64_t seed, int64_t row_offset, int64_t n,
                            float* theta_out, void* stream) {
  FmPlan pl;
  int rc = np_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!packed || !zstats || !base || !x || !ts || !theta_out || n < 0 || steps < 0 || row_offset < 0 || !(eta > 0.f))
    return SBI_AMD_E_BADARG;
  if (x_rows != 1 && x_rows != n) return SBI_AMD_E_BADARG;
  if (steps > 65535) return SBI_AMD_E_UNSUPPORTED;
  if (n == 0) return 0;
  FmArgs a;
  memset(&a, 0, sizeof(a));
  a.packed = packed; a.zstats = zstats; a.x = x; a.times = ts; a.n = n;
  a.x_rows = (x_rows == 1 || n == 1) ? 1 : 2; a.t_rows = 1;
  a.steps = steps; a.eta = eta; a.base = base; a.sde_noise = noise; a.seed = seed; a.row_offset = row_offset;
  a.v_out = theta_out; a.ntiles = (int)((n + FM_ROWS - 1) / FM_ROWS);
  return fm_launch_fwd<6>(pl, a, (hipStream_t)stream);
}

// ---- iid observations: the composed score and its sampler (npse_iid_kernel.h)
static int np_iid_envelope(const FmPlan& pl, int64_t N) {
  return (pl.D <= NP_IID_MAX_D && N >= 1 && N <= NP_IID_MAX_N) ? 0 : SBI_AMD_E_UNSUPPORTED;
}

int64_t sbi_amd_npse_iid_workspace_floats(const sbi_amd_npse_config* cfg, int64_t N) {
  FmPlan pl;
  int rc = np_build_plan(cfg, &pl);
  if (rc) return rc;
  if (N < 1) return SBI_AMD_E_BADARG;
  rc = np_iid_envelope(pl, N);
  if (rc) return rc;
  return N * NP_IID_EC;
}

int sbi_amd_npse_score_iid(const sbi_amd_npse_config* cfg, const float* packed, const float* zstats,
                           const float* theta_t, const float* x, int64_t N, const float* time, const float* lam,
                           const float* mats, const float* vec, int64_t n, float* workspace, float* out, void* stream) {
  FmPlan pl;
  int rc = np_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!packed || !zstats || !theta_t || !x || !time || !mats || !vec || !workspace || !out || n < 0 || N < 1)
    return SBI_AMD_E_BADARG;
  rc = np_iid_envelope(pl, N);
  if (rc) return rc;
  if (n == 0) return 0;
  FmArgs a;
  memset(&a, 0, sizeof(a));
  a.packed = packed; a.zstats = zstats; a.theta = theta_t; a.times = time; a.n = n; a.t_rows = 1; a.steps = 1;
  a.v_out = out; a.ntiles = (int)((n + FM_ROWS - 1) / FM_ROWS);
  NpIidArgs q;
  memset(&q, 0, sizeof(q));
  q.xs = x; q.N = (int)N; q.lam = lam; q.mats = mats; q.vecs = vec;
  return np_iid_launch<false>(pl, a, q, workspace, (hipStream_t)stream);
}

int sbi_amd_npse_sample_sde_iid(const sbi_amd_npse_config* cfg, const float* packed, const float* zstats,
                                const float* base, const float* x, int64_t N, const float* ts, int32_t steps, float eta,
                                const float* lam, const float* step_mats, const float* step_vecs, const float* noise,
                                uint64_t seed, int64_t row_offset, int64_t n, float* workspace, float* theta_out,
                                void* stream) {
  FmPlan pl;
  int rc = np_build_plan(cfg, &pl);
  if (rc) return rc;
  if (!packed || !zstats || !base || !x || !ts || !workspace || !theta_out || n < 0 || N < 1 || steps < 0 ||
      row_offset < 0 || !(eta > 0.f) || (steps > 0 && (!step_mats || !step_vecs)))
    return SBI_AMD_E_BADARG;
  if (steps > 65535) return SBI_AMD_E_UNSUPPORTED;
  rc = np_iid_envelope(pl, N);
  if (rc) return rc;
  if (n == 0) return 0;
  FmArgs a;
  memset(&a, 0, sizeof(a));
  a.packed = packed; a.zstats = zstats; a.times = ts; a.n = n; a.t_rows = 1;
  a.steps = steps; a.eta = eta; a.base = base; a.sde_noise = noise; a.seed = seed; a.row_offset = row_offset;
  a.v_out = theta_out; a.ntiles = (int)((n + FM_ROWS - 1) / FM_ROWS);
  NpIidArgs q;
  memset(&q, 0, sizeof(q));
  q.xs = x; q.N = (int)N; q.lam = lam; q.mats = step_mats; q.vecs = step_vecs;
  return np_iid_launch<true>(pl, a, q, workspace, (hipStream_t)stream);
}

int sbi_amd_npse_compose_iid(const float* s, const float* theta, const float* lam, const float* mats, const float* vec,
                             int64_t n, int64_t N, int32_t D, float* out, void* stream) {
  if (!s || !theta || !mats || !vec || !out || n < 0 || N < 1 || N > 0x7fffffff / 128 || D < 1 || D > 128)
    return SBI_AMD_E_BADARG;
  if (n == 0) return 0;
  if (n > 0x7fffffff) return SBI_AMD_E_UNSUPPORTED;
  hipLaunchKernelGGL(np_compose_kernel, dim3((unsigned)n), dim3(128), 0, (hipStream_t)stream, s, theta, lam, mats, vec,
                     (int)N, (int)D, out);
  return (int)hipGetLastError();
}

int sbi_amd_npse_sde_normals(uint64_t seed, int64_t row_offset, int32_t k, int64_t n, int32_t D, float* out,
                              void* stream) {
  if (!out || n < 0 || row_offset < 0 || k < 0 || D < 1 || D > 128) return SBI_AMD_E_BADARG;
  if (n == 0) return 0;
  FmArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n; a.seed = seed; a.row_offset = row_offset;
  const long long threads = n * ((D + 3) / 4);
  hipLaunchKernelGGL(np_normals_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a,
                     (int)D, (int)k, out);
  return (int)hipGetLastError();
}

}  // extern "C"
