// maf_affine.hip -- host side of the affine MAF path (plan, C ABI of include/sbi_amd_maf_affine.h), its pack and
// reduce kernels and the kernel instantiations (hidden K-steps 13 and 16).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include "maf_affine_kernel.h"

static int a_round_up(int v, int m) { return (v + m - 1) / m * m; }
static int a_two_odd(int v) {
  int x = (v + 1) / 2;
  if ((x & 1) == 0) x += 1;
  return 2 * x;
}

// image conventions of maf.hip (m_set_lin): row-major [rows][ldk], ldk = 2 * odd, rows >= out + 1 zero rows;
// `g_out`: rows the layer has in the flat buffer (the final layer: 2 D there, 32 in the image)
static void a_set_lin(LinDesc* L, int* g, int* l, int out, int g_out, int in, int bias_pad, int ksteps_fixed,
                      int min_rows) {
  L->out = out;
  L->in = in;
  L->ksteps = ksteps_fixed > 0 ? ksteps_fixed : a_round_up((in + 3) / 4, 4);
  L->ldk = a_two_odd(ksteps_fixed > 0 ? in : 4 * L->ksteps);
  L->g_w = *g; *g += g_out * in;
  L->g_b = *g; *g += g_out;
  L->l_w = *l;
  int rows = out + 1;
  if (min_rows > rows) rows = min_rows;
  L->rows = rows;
  *l += rows * L->ldk;
  L->l_b = *l;
  *l += bias_pad;
}

static int aff_build_plan(const sbi_amd_maf_affine_config* c, int nw, bool trials, MafAffPlan* ap) {
  if (!c) return SBI_AMD_E_BADARG;
  if (c->D < 1 || c->C < 1 || c->H < 1 || c->T < 1 || c->NB < 0) return SBI_AMD_E_BADARG;
  if (c->D > 16 || c->C > 32 || c->H > 16 * NSF_HT || c->T > NSF_MAX_T || c->NB > MAF_MAX_NB)
    return SBI_AMD_E_UNSUPPORTED;
  if (!(c->epsilon >= 0.f)) return SBI_AMD_E_BADARG;
  memset(ap, 0, sizeof(*ap));
  ap->eps = c->epsilon;
  MafPlan* mp = &ap->m;
  NsfPlan* pl = &mp->n;
  const int D = c->D, C = c->C, H = c->H, NB = c->NB;
  pl->D = D; pl->C = C; pl->H = H; pl->T = c->T; pl->NB = NB;
  pl->P = 2;
  pl->PT = 1;
  pl->KSH = ((H + 3) / 4 == 13) ? 13 : 16;
  pl->log_z = (float)(0.5 * D * log(2.0 * M_PI));
  ShapeDesc* s = &pl->shape[0];
  s->d_id = D; s->d_tr = D; s->in0 = D;
  int g = 0, l = 0;
  const int hb = 16 * NSF_HT, tr_rows = 4 * pl->KSH + 1;
  a_set_lin(&s->lin[0], &g, &l, H, H, D, hb, 0, tr_rows);
  a_set_lin(&s->lin[1], &g, &l, H, H, C, hb, 0, tr_rows);   // (d loss / d x runs the transposed GEMM on it)
  for (int b = 0; b < NB; ++b) a_set_lin(&s->lin[2 + b], &g, &l, H, H, H, hb, pl->KSH, tr_rows);
  s->fin = 2 + NB;
  l = a_round_up(l, 4);
  s->final_off = l;
  a_set_lin(&s->lin[s->fin], &g, &l, 32, 2 * D, H, 32, pl->KSH, 0);
  s->n_params = g;
  mp->n_layer = g;
  l = a_round_up(l + 8, 4);   // slack: the K loop of the last image row runs a few floats past the layer
  mp->l_perm = l; l += 16;
  mp->l_iperm = l; l += 16;
  s->lds_floats = a_round_up(l, 4);
  pl->lds_w_floats = pl->img_floats = s->lds_floats;
  pl->n_params = g * c->T;
  for (int t = 0; t < c->T; ++t) pl->g_layer[t] = t * g;
  // per-wave scratch
  pl->ZW = a_two_odd(D);
  const int ks0 = a_round_up((D + 3) / 4, 4), ksc = a_round_up((C + 3) / 4, 4);
  const int need = 4 * ks0 > D + 4 * ksc ? 4 * ks0 : D + 4 * ksc;
  pl->CINW = a_two_odd(need);
  int o = 0;
  mp->sc_zs = o; o += 16 * pl->ZW + 16;
  mp->sc_us = o; o += 16 * pl->ZW + 16;
  mp->sc_cin = o; o += 16 * pl->CINW + 16;
  if (trials) {
    ap->tz_stride = 16 * pl->ZW + 16;
    ap->sc_tz = o; o += MAF_AFF_TC * ap->tz_stride;
    ap->sc_tld = o; o += MAF_AFF_TC * 64;
  }
  mp->sc_total = a_round_up(o, 4);
  if (4ll * ((int64_t)pl->lds_w_floats + (int64_t)nw * mp->sc_total) > NSF_LDS_LIMIT_BYTES) return SBI_AMD_E_LDS;
  return 0;
}

// 8, 4, 2 or 1 waves, the largest that still yields >= 256 workgroups; if its LDS does not fit, one wave fewer at a
// time until it does (any count works: a wave owns its 16 rows and its scratch)
static int aff_plan_for_rows(const sbi_amd_maf_affine_config* cfg, int64_t n, bool trials, MafAffPlan* ap,
                             int* nw_out) {
  int nw = 8;
  while (nw > 1 && (n + 16 * nw - 1) / (16 * nw) < 256) nw >>= 1;
  for (; nw >= 1; --nw) {
    const int rc = aff_build_plan(cfg, nw, trials, ap);
    if (rc == 0) { *nw_out = nw; return 0; }
    if (rc != SBI_AMD_E_LDS) return rc;
  }
  return SBI_AMD_E_LDS;
}

// ------------------------------------------------------------------ pack
__global__ void __launch_bounds__(256)
maf_aff_pack_kernel(const MafAffPlan ap, const float* __restrict__ params, const int* __restrict__ perms,
                    float* __restrict__ packed) {
  const MafPlan& mp = ap.m;
  const NsfPlan& pl = mp.n;
  const ShapeDesc& S = pl.shape[0];
  const int t = blockIdx.x, D = pl.D;
  float* img = packed + (long long)t * pl.img_floats;
  const float* gl = params + (long long)t * mp.n_layer;
  const int tid = blockIdx.y * blockDim.x + threadIdx.x, nthreads = gridDim.y * blockDim.x;
  const int hb = 16 * NSF_HT;
  maf_pack_linear(img, gl, nullptr, S.lin[0], 0, D, 2, hb, hb, hb, tid, nthreads);
  maf_pack_linear(img, gl, nullptr, S.lin[1], 1, D, 2, hb, hb, hb, tid, nthreads);
  for (int b = 0; b < pl.NB; ++b) maf_pack_linear(img, gl, nullptr, S.lin[2 + b], 2, D, 2, hb, hb, hb, tid, nthreads);
  // final layer: nflows row 2 d + tile -> image row 16 tile + d, output mask (d + 1 > hidden degree) folded in,
  // rows of dims >= D and the padding rows zero
  const LinDesc& L = S.lin[S.fin];
  for (int idx = S.lin[S.fin - 1].l_b + hb + tid; idx < L.l_w; idx += nthreads) img[idx] = 0.f;   // alignment gap
  for (int idx = tid; idx < L.rows * L.ldk; idx += nthreads) {
    const int r = idx / L.ldk, c = idx - r * L.ldk;
    const int tile = r >> 4, d = r & 15;
    float v = 0.f;
    if (r < 32 && d < D && c < L.in && d + 1 > maf_hidden_degree(c, D)) v = gl[L.g_w + (2 * d + tile) * L.in + c];
    img[L.l_w + idx] = v;
  }
  for (int idx = tid; idx < 32; idx += nthreads) {
    const int tile = idx >> 4, d = idx & 15;
    img[L.l_b + idx] = d < D ? gl[L.g_b + 2 * d + tile] : 0.f;
  }
  for (int idx = L.l_b + 32 + tid; idx < pl.img_floats; idx += nthreads)
    if (idx < mp.l_perm || idx >= mp.l_iperm + 16 || ((idx - mp.l_perm) & 15) >= D) img[idx] = 0.f;
  for (int d = tid; d < D; d += nthreads) {
    const int p = perms[t * D + d];
    img[mp.l_perm + d] = __int_as_float(p);
    img[mp.l_iperm + p] = __int_as_float(d);
  }
}

// grad[t][idx] (nflows' order) = fixed-order sum over the chunks (the order of maf_reduce_kernel) of the partials,
// whose final layer is de-interleaved: [Wu (D, H) | Ws (D, H) | bu (D) | bs (D)] at the final layer's offset; the
// final layer's output mask is applied here (the other masks by maf_dw_kernel)
__global__ void __launch_bounds__(256)
maf_aff_reduce_kernel(const float* __restrict__ partial, float* __restrict__ grad, int n_layer, int nchunks, int T,
                      int D, int H, int fin_w, int fin_b) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)T * n_layer) return;
  const int t = (int)(idx / n_layer);
  const int li = (int)(idx - (long long)t * n_layer);
  int src = li;
  bool keep = true;
  if (li >= fin_b) {
    const int o = li - fin_b;
    src = fin_b + (o & 1) * D + (o >> 1);
  } else if (li >= fin_w) {
    const int o = (li - fin_w) / H, c = (li - fin_w) - o * H;
    src = fin_w + ((o & 1) * D + (o >> 1)) * H + c;
    keep = (o >> 1) + 1 > maf_hidden_degree(c, D);
  }
  const float* base = partial + (long long)t * nchunks * n_layer + src;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  int c = 0;
  for (; c + 3 < nchunks; c += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) s[u] += base[(long long)(c + u) * n_layer];
  }
  for (; c < nchunks; ++c) s[0] += base[(long long)c * n_layer];
  grad[idx] = keep ? (s[0] + s[1]) + (s[2] + s[3]) : 0.f;
}

__global__ void maf_aff_neg_copy_kernel(const float* __restrict__ in, float* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = -in[i];
}

// ------------------------------------------------------------------ launchers
template <int KSH, bool INV>
static int aff_launch_flow(const MafAffPlan& ap, int nw, const float* packed, const float* zstats, const float* in,
                           const float* x, int64_t n, int64_t x_rows, float* out_main, float* out_aux, float* z_stash,
                           hipStream_t st) {
  const int lds_bytes = 4 * (ap.m.n.lds_w_floats + nw * ap.m.sc_total);
  auto kern = maf_aff_flow_kernel<KSH, INV>;
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (e != hipSuccess) return (int)e;
  const int64_t grid = (n + 16 * nw - 1) / (16 * nw);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * nw), (size_t)lds_bytes, st, ap, packed, zstats, in, x,
                     (long long)n, (long long)x_rows, out_main, out_aux, z_stash);
  return (int)hipGetLastError();
}
template <bool INV>
static int aff_flow(const MafAffPlan& ap, int nw, const float* packed, const float* zstats, const float* in,
                    const float* x, int64_t n, int64_t x_rows, float* out_main, float* out_aux, float* z_stash,
                    hipStream_t st) {
  if (ap.m.n.KSH == 13)
    return aff_launch_flow<13, INV>(ap, nw, packed, zstats, in, x, n, x_rows, out_main, out_aux, z_stash, st);
  return aff_launch_flow<16, INV>(ap, nw, packed, zstats, in, x, n, x_rows, out_main, out_aux, z_stash, st);
}

template <int KSH>
static int aff_launch_bwd(const MafAffPlan& ap, int nw, const MafBwdArgs& a, float* grad_x, hipStream_t st) {
  const int lds_bytes = 4 * (ap.m.n.lds_w_floats + nw * ap.m.sc_total);
  auto kern = maf_aff_bwd_kernel<KSH>;
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (e != hipSuccess) return (int)e;
  const int64_t grid = (a.n + 16 * nw - 1) / (16 * nw);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * nw), (size_t)lds_bytes, st, ap, a, grad_x);
  return (int)hipGetLastError();
}

template <int KSH>
static int aff_launch_trials(const MafAffPlan& ap, int nw, const float* packed, const float* zstats,
                             const float* x_trials, int64_t num_trials, const float* theta, int64_t num_theta,
                             float* out, hipStream_t st) {
  const int lds_bytes = 4 * (ap.m.n.lds_w_floats + nw * ap.m.sc_total);
  auto kern = maf_aff_trials_kernel<KSH>;
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (e != hipSuccess) return (int)e;
  const int64_t grid = (num_theta + 16 * nw - 1) / (16 * nw);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * nw), (size_t)lds_bytes, st, ap, packed, zstats, x_trials,
                     (long long)num_trials, theta, (long long)num_theta, out);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------ C ABI
static int aff_plan_sizes(const sbi_amd_maf_affine_config* cfg, MafAffPlan* ap) {
  const int rc = aff_build_plan(cfg, 1, false, ap);
  return rc == SBI_AMD_E_LDS ? 0 : rc;
}

extern "C" int64_t sbi_amd_maf_affine_param_count(const sbi_amd_maf_affine_config* cfg) {
  MafAffPlan ap;
  const int rc = aff_plan_sizes(cfg, &ap);
  return rc ? rc : ap.m.n.n_params;
}
extern "C" int64_t sbi_amd_maf_affine_packed_floats(const sbi_amd_maf_affine_config* cfg) {
  MafAffPlan ap;
  const int rc = aff_plan_sizes(cfg, &ap);
  return rc ? rc : (int64_t)ap.m.n.T * ap.m.n.img_floats;
}
extern "C" int64_t sbi_amd_maf_affine_param_offset(const sbi_amd_maf_affine_config* cfg, int32_t t, int32_t which,
                                                   int32_t bias) {
  MafAffPlan ap;
  const int rc = aff_plan_sizes(cfg, &ap);
  if (rc) return rc;
  if (t < 0 || t >= ap.m.n.T || which < 0 || which > ap.m.n.shape[0].fin) return SBI_AMD_E_BADARG;
  const LinDesc& L = ap.m.n.shape[0].lin[which];
  return (int64_t)t * ap.m.n_layer + (bias ? L.g_b : L.g_w);
}

extern "C" int32_t sbi_amd_maf_affine_plan_waves(const sbi_amd_maf_affine_config* cfg, int64_t n, int32_t trials) {
  if (!cfg || n < 1) return SBI_AMD_E_BADARG;
  MafAffPlan ap;
  int nw = 0;
  const int rc = aff_plan_for_rows(cfg, n, trials != 0, &ap, &nw);
  return rc ? rc : nw;
}

extern "C" int sbi_amd_maf_affine_pack(const sbi_amd_maf_affine_config* cfg, const float* params,
                                       const int32_t* perms, float* packed, void* stream) {
  if (!cfg || !params || !perms || !packed) return SBI_AMD_E_BADARG;
  MafAffPlan ap;
  const int rc = aff_plan_sizes(cfg, &ap);
  if (rc) return rc;
  hipLaunchKernelGGL(maf_aff_pack_kernel, dim3(ap.m.n.T, 16), dim3(256), 0, (hipStream_t)stream, ap, params, perms,
                     packed);
  return (int)hipGetLastError();
}

extern "C" int sbi_amd_maf_affine_log_prob(const sbi_amd_maf_affine_config* cfg, const float* packed,
                                           const float* zstats, const float* theta, const float* x, int64_t n,
                                           int64_t x_rows, float* logp_out, float* noise_out, void* stream) {
  if (n == 0) return 0;
  if (!cfg || !packed || !zstats || !theta || !x || !logp_out || n < 0 || x_rows < 1) return SBI_AMD_E_BADARG;
  MafAffPlan ap;
  int nw = 0;
  const int rc = aff_plan_for_rows(cfg, n, false, &ap, &nw);
  if (rc) return rc;
  return aff_flow<false>(ap, nw, packed, zstats, theta, x, n, x_rows, logp_out, noise_out, nullptr,
                         (hipStream_t)stream);
}

extern "C" int sbi_amd_maf_affine_sample(const sbi_amd_maf_affine_config* cfg, const float* packed,
                                         const float* zstats, const float* noise, const float* x, int64_t n,
                                         int64_t x_rows, float* theta_out, float* logabsdet_out, void* stream) {
  if (n == 0) return 0;
  if (!cfg || !packed || !zstats || !noise || !x || !theta_out || n < 0 || x_rows < 1) return SBI_AMD_E_BADARG;
  MafAffPlan ap;
  int nw = 0;
  const int rc = aff_plan_for_rows(cfg, n, false, &ap, &nw);
  if (rc) return rc;
  return aff_flow<true>(ap, nw, packed, zstats, noise, x, n, x_rows, theta_out, logabsdet_out, nullptr,
                        (hipStream_t)stream);
}

extern "C" int sbi_amd_maf_affine_log_prob_trials(const sbi_amd_maf_affine_config* cfg, const float* packed,
                                                  const float* zstats, const float* x_trials, int64_t num_trials,
                                                  const float* theta, int64_t num_theta, float* loglik_out,
                                                  void* stream) {
  if (num_theta == 0) return 0;
  if (!cfg || !packed || !zstats || !x_trials || !theta || !loglik_out || num_trials < 1 || num_theta < 0)
    return SBI_AMD_E_BADARG;
  MafAffPlan ap;
  int nw = 0;
  const int rc = aff_plan_for_rows(cfg, num_theta, true, &ap, &nw);
  if (rc) return rc;
  if (ap.m.n.KSH == 13)
    return aff_launch_trials<13>(ap, nw, packed, zstats, x_trials, num_trials, theta, num_theta, loglik_out,
                                 (hipStream_t)stream);
  return aff_launch_trials<16>(ap, nw, packed, zstats, x_trials, num_trials, theta, num_theta, loglik_out,
                               (hipStream_t)stream);
}

// ---- training workspace layout (floats)
struct AffWs {
  int64_t stash, noise, logp, gza, gzb, gp, act, gbuf, ctx, part, total, npad;
  int nchunks;
};
static AffWs aff_ws_layout(const MafAffPlan& ap, int64_t n) {
  AffWs w;
  const int D = ap.m.n.D, T = ap.m.n.T;
  int64_t o = 0;
  auto take = [&](int64_t sz) { const int64_t at = o; o += (sz + 3) / 4 * 4; return at; };
  w.stash = take((int64_t)T * n * D);
  w.noise = take(n * D);
  w.logp = take(n);
  w.gza = take(n * D);
  w.gzb = take(n * D);
  const int64_t npad = (n + MAF_DW_CHUNK - 1) / MAF_DW_CHUNK * MAF_DW_CHUNK;   // the dW kernel reads whole chunks
  w.npad = npad;
  w.gp = take(npad * 32);
  w.act = take(npad * (MAF_MAX_NB + 1) * MAF_AW);
  w.gbuf = take(npad * (MAF_MAX_NB + 2) * MAF_AW);
  w.ctx = take(npad * MAF_CW);
  w.nchunks = (int)(npad / MAF_DW_CHUNK);
  w.part = take((int64_t)T * w.nchunks * ap.m.n_layer);
  w.total = o;
  return w;
}

extern "C" int64_t sbi_amd_maf_affine_train_workspace_floats(const sbi_amd_maf_affine_config* cfg, int64_t n) {
  MafAffPlan ap;
  const int rc = aff_plan_sizes(cfg, &ap);
  if (rc) return rc;
  return aff_ws_layout(ap, n > 0 ? n : 1).total;
}

extern "C" int sbi_amd_maf_affine_loss_fwd_bwd(const sbi_amd_maf_affine_config* cfg, const float* packed,
                                               const float* zstats, const float* theta, const float* x, int64_t n,
                                               int64_t x_rows, const float* row_weight, float uniform_weight,
                                               float* loss_out, float* grad_out, float* grad_theta_out,
                                               float* grad_x_out, float* workspace, void* stream) {
  if (!cfg || !packed || !zstats || !theta || !x || !grad_out || !workspace || n < 1 || x_rows < 1)
    return SBI_AMD_E_BADARG;
  if (grad_x_out && x_rows != n) return SBI_AMD_E_BADARG;   // one condition row per theta row
  hipStream_t st = (hipStream_t)stream;
  MafAffPlan ap;
  int nw = 0;
  int rc = aff_plan_for_rows(cfg, n, false, &ap, &nw);
  if (rc) return rc;
  const MafPlan& mp = ap.m;
  const AffWs w = aff_ws_layout(ap, n);
  const int D = mp.n.D, T = mp.n.T, NB = mp.n.NB, H = mp.n.H;
  rc = aff_flow<false>(ap, nw, packed, zstats, theta, x, n, x_rows, workspace + w.logp, workspace + w.noise,
                       workspace + w.stash, st);
  if (rc) return rc;
  if (loss_out)
    hipLaunchKernelGGL(maf_aff_neg_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                       workspace + w.logp, loss_out, (long long)n);
  const ShapeDesc& S = mp.n.shape[0];
  const LinDesc& LF = S.lin[S.fin];
  float* gz[2] = {workspace + w.gza, workspace + w.gzb};
  for (int t = T - 1; t >= 0; --t) {
    MafBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.packed = packed; a.zstats = zstats;
    a.z_in = workspace + w.stash + (int64_t)t * n * D;
    a.x = x;
    a.gz_up = (t == T - 1) ? workspace + w.noise : gz[(t + 1) & 1];
    a.row_w = row_weight; a.uni_w = uniform_weight;
    a.n = n; a.x_rows = x_rows;
    a.gz_dn = gz[t & 1];
    a.grad_theta = grad_theta_out;
    a.GP = workspace + w.gp; a.ACT = workspace + w.act; a.G = workspace + w.gbuf; a.CTX = workspace + w.ctx;
    a.npad = w.npad;
    a.t = t; a.is_last = (t == T - 1);
    rc = mp.n.KSH == 13 ? aff_launch_bwd<13>(ap, nw, a, grad_x_out, st) : aff_launch_bwd<16>(ap, nw, a, grad_x_out, st);
    if (rc) return rc;
    MafDwArgs d;
    memset(&d, 0, sizeof(d));
    const int AWS = (MAF_MAX_NB + 1) * MAF_AW;
    const int64_t gts = w.npad * 16;     // floats per m-tile plane
    auto set = [&](int i, const float* G, const float* A, int lda, int out, int in, int g_w, int g_b, int kind,
                   int aperm, int group, int gpad) {
      d.lin[i].G = G; d.lin[i].gts = gts; d.lin[i].A = A; d.lin[i].lda = lda;
      d.lin[i].out = out; d.lin[i].in = in; d.lin[i].in_total = in; d.lin[i].col0 = 0;
      d.lin[i].group = group; d.lin[i].group_pad = gpad;
      d.lin[i].g_w = g_w; d.lin[i].g_b = g_b; d.lin[i].kind = kind;
      d.lin[i].gperm = 1; d.lin[i].aperm = aperm;
    };
    // (G planes and ACT rows are in fragment order, the CTX rows in natural order.)  The final layer goes in as
    // two D-row linears, one per tile, unmasked (kind 1) into the de-interleaved partial layout that
    // maf_aff_reduce_kernel reads back; the hidden layers as in the maf_rqs pass
    int nl = 0;
    for (int b = 0; b < NB; ++b)
      set(nl++, a.G + 4 * (2 + b) * gts, a.ACT + 64 * b, AWS, H, H, S.lin[2 + b].g_w, S.lin[2 + b].g_b, 2, 1, H, 64);
    set(nl++, a.G, a.CTX, MAF_CW, H, D, S.lin[0].g_w, S.lin[0].g_b, 0, 0, H, 64);
    set(nl++, a.G + 4 * gts, a.CTX + D, MAF_CW, H, mp.n.C, S.lin[1].g_w, S.lin[1].g_b, 1, 0, H, 64);
    for (int tile = 0; tile < 2; ++tile)
      set(nl++, a.GP + tile * gts, a.ACT + 64 * NB, AWS, D, H, LF.g_w + tile * D * H, LF.g_w + 2 * D * H + tile * D,
          1, 1, 16, 16);
    d.n = n; d.rows_per_chunk = MAF_DW_CHUNK; d.nchunks = w.nchunks; d.n_layer = mp.n_layer;
    d.D = D; d.P = 2;
    d.partial = workspace + w.part + (int64_t)t * w.nchunks * mp.n_layer;
    rc = maf_launch_dw(d, nl, st);
    if (rc) return rc;
  }
  const int64_t total = (int64_t)T * mp.n_layer;
  hipLaunchKernelGGL(maf_aff_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                     workspace + w.part, grad_out, mp.n_layer, w.nchunks, T, D, H, LF.g_w, LF.g_b);
  return (int)hipGetLastError();
}
