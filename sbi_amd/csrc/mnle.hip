// mnle.hip -- host side of the MNLE path (plan, C ABI of include/sbi_amd_mnle.h), its pack kernels and the dispatch
// over num_bins (the kernels themselves are instantiated in mnle_k*.hip).  The weight gradients reuse the MAF path's
// split-K kernels (maf_launch_dw / maf_launch_reduce).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#define MNLE_MAIN_TU
#include "mnle_kernel.h"

extern template int mnle_dispatch_k<4>(const MnlePlan&, const MnleCall&, hipStream_t);
extern template int mnle_dispatch_k<5>(const MnlePlan&, const MnleCall&, hipStream_t);
extern template int mnle_dispatch_k<8>(const MnlePlan&, const MnleCall&, hipStream_t);
extern template int mnle_dispatch_k<10>(const MnlePlan&, const MnleCall&, hipStream_t);
extern template int mnle_dispatch_k<16>(const MnlePlan&, const MnleCall&, hipStream_t);

static int mnle_dispatch(const MnlePlan& P, const MnleCall& q, hipStream_t st) {
  switch (P.K) {
    case 4: return mnle_dispatch_k<4>(P, q, st);
    case 5: return mnle_dispatch_k<5>(P, q, st);
    case 8: return mnle_dispatch_k<8>(P, q, st);
    case 10: return mnle_dispatch_k<10>(P, q, st);
    case 16: return mnle_dispatch_k<16>(P, q, st);
  }
  return SBI_AMD_E_UNSUPPORTED;
}

// shapes (out, in) of linear `which` in the flat buffer
static void mnle_lin_shape(const MnlePlan& P, int which, int* out, int* in) {
  const int nd = 3 + 3 * P.NB;
  if (which == 0) { *out = P.Hd; *in = P.F; }
  else if (which == 1) { *out = P.Hd; *in = P.C; }
  else if (which < 2 + 3 * P.NB) { *out = P.Hd; *in = (which - 2) % 3 == 2 ? P.C : P.Hd; }
  else if (which == nd - 1) { *out = P.F * P.Kmax; *in = P.Hd; }
  else if (which == nd) { *out = P.E; *in = P.V + P.C; }
  else if (which == nd + 1) { *out = P.E; *in = P.E; }
  else {
    const int per = P.L > 0 ? 3 : 2, r = (which - nd - 2) % per;
    if (r == 0) { *out = P.Hc; *in = P.E; }
    else if (r == 1 && P.L > 0) { *out = P.Hc; *in = P.Hc; }
    else { *out = P.P; *in = P.Hc; }
  }
}

static int mnle_build_plan(const sbi_amd_mnle_config* c, MnlePlan* P, MnleLayout* Ly) {
  if (!c) return SBI_AMD_E_BADARG;
  if (c->V < 1 || c->V > 4 || c->C < 1 || c->C > 64 || c->discrete_hidden < 1 || c->discrete_hidden > 64 ||
      c->discrete_blocks < 0 || c->discrete_blocks > 4 || c->embedding < 1 || c->embedding > 64 || c->hidden < 1 ||
      c->hidden > 64 || c->num_transforms < 1 || c->num_transforms > 16 || c->context_layers < 0 ||
      c->context_layers > 4)
    return SBI_AMD_E_UNSUPPORTED;
  const int K = c->num_bins;
  if (K != 4 && K != 5 && K != 8 && K != 10 && K != 16) return SBI_AMD_E_UNSUPPORTED;
  for (int v = 0; v < c->V; ++v)
    if (c->num_categories[v] < 1 || c->num_categories[v] > 16) return SBI_AMD_E_UNSUPPORTED;
  if (!(c->tail_bound > 0.f)) return SBI_AMD_E_BADARG;
  memset(P, 0, sizeof(*P));
  P->V = c->V; P->F = c->V + 1; P->C = c->C; P->Hd = c->discrete_hidden; P->NB = c->discrete_blocks;
  P->E = c->embedding; P->Hc = c->hidden; P->K = K; P->T = c->num_transforms; P->L = c->context_layers;
  P->P = 3 * K - 1;
  P->PT = (P->P + 15) / 16;
  for (int v = 0; v < 4; ++v) {
    P->nc[v] = v < c->V ? c->num_categories[v] : 1;
    if (v < c->V && P->nc[v] > P->Kmax) P->Kmax = P->nc[v];
  }
  P->VK = P->V * P->Kmax;
  P->PF = (P->F * P->Kmax + 15) / 16;
  P->KSC = (P->C + 3) / 4;
  P->st_final = 1 + P->NB;
  P->st_emb = 2 + P->NB;
  P->st_tr0 = 3 + P->NB;
  P->n_stages = P->st_tr0 + P->T;
  P->img_floats = P->n_stages * MNLE_STAGE;
  P->n_lin = 5 + 3 * P->NB + P->T * (P->L > 0 ? 3 : 2);
  int g = 0;
  for (int i = 0; i < P->n_lin; ++i) {
    int o, in;
    mnle_lin_shape(*P, i, &o, &in);
    if (Ly) { Ly->g_w[i] = g; Ly->g_b[i] = g + o * in; }
    g += o * in + o;
  }
  P->n_params = g;
  P->n_virtual = g + (P->L > 1 ? P->T * (P->L - 1) * (P->Hc * P->Hc + P->Hc) : 0);
  int s = 0;
  P->sc_cs = s; s += 16 * MNLE_CSW;
  P->sc_din = s; s += 16 * MNLE_DW;
  P->sc_sc = s; s += 16 * MNLE_SW;
  P->sc_z = s; s += 16 * MNLE_ZW;
  P->sc_total = (s + 3) / 4 * 4;
  P->log_x = c->log_transform ? 1 : 0;
  P->B = c->tail_bound;
  P->min_w = c->min_bin_width; P->min_h = c->min_bin_height; P->min_d = c->min_derivative;
  P->inv_sqrt_h = (float)(1.0 / sqrt((double)P->Hc));
  P->one_minus_kw = (float)(1.0 - (double)c->min_bin_width * K);
  P->one_minus_kh = (float)(1.0 - (double)c->min_bin_height * K);
  P->d_const = (float)log(exp(1.0 - (double)c->min_derivative) - 1.0);
  P->log_z = (float)(0.5 * log(2.0 * M_PI));
  return 0;
}
static int mnle_lds(const MnlePlan& P, int nw) { return 4 * (MNLE_STAGE + nw * P.sc_total); }
// largest workgroup (4, 2, 1 waves) that still yields >= 256 workgroups: a stage copy is shared by its waves
static int mnle_waves(int64_t n) {
  int nw = 4;
  while (nw > 1 && (n + 16 * nw - 1) / (16 * nw) < 256) nw >>= 1;
  return nw;
}

__device__ __forceinline__ int mnle_hdeg(int i, int V) { return i % V + 1; }

__global__ void __launch_bounds__(256)
mnle_pack_kernel(const MnlePlan P, const MnleLayout Ly, const float* __restrict__ p, float* __restrict__ img) {
  const int total = P.img_floats + P.n_virtual;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    if (idx >= P.img_floats) {        // the flat buffer's mask: dense until mnle_mask_kernel has run
      img[idx] = 1.f;
      continue;
    }
    const int s = idx / MNLE_STAGE, o3 = idx - s * MNLE_STAGE, slot = o3 / MNLE_MAT, o = o3 - slot * MNLE_MAT;
    const bool bias = o >= 64 * MNLE_LD;
    const int r = bias ? o - 64 * MNLE_LD : o / MNLE_LD;
    const int c = bias ? 0 : o - r * MNLE_LD;
    int lin = -1, rows = 0, cols = 0, ld = 0, c0 = 0, r0 = 0, mk = 0;   // mk: 0 dense, 1 initial, 2 hidden, 3 final
    bool has_bias = true;
    if (s == 0) {
      if (slot == 0) { lin = 0; rows = P.Hd; cols = P.F; ld = P.F; mk = 1; }
      else if (slot == 1) { lin = 1; rows = P.Hd; cols = P.C; ld = P.C; }
    } else if (s < P.st_final) {
      lin = 2 + 3 * (s - 1) + slot; rows = P.Hd; cols = slot == 2 ? P.C : P.Hd; ld = cols; mk = slot == 2 ? 0 : 2;
    } else if (s == P.st_final) {
      if (slot == 0) { lin = 2 + 3 * P.NB; rows = P.VK; cols = P.Hd; ld = P.Hd; r0 = P.Kmax; mk = 3; }
    } else if (s == P.st_emb) {
      const int la = 3 + 3 * P.NB;
      if (slot == 0) { lin = la; rows = P.E; cols = P.C; ld = P.V + P.C; c0 = P.V; }
      else if (slot == 1) { lin = la; rows = P.E; cols = P.V; ld = P.V + P.C; has_bias = false; }
      else { lin = la + 1; rows = P.E; cols = P.E; ld = P.E; }
    } else {
      const int per = P.L > 0 ? 3 : 2, base = 5 + 3 * P.NB + (s - P.st_tr0) * per;
      if (slot == 0) { lin = base; rows = P.Hc; cols = P.E; ld = P.E; }
      else if (slot == 1) { if (P.L > 0) { lin = base + 1; rows = P.Hc; cols = P.Hc; ld = P.Hc; } }
      else { lin = base + per - 1; rows = P.P; cols = P.Hc; ld = P.Hc; }
    }
    float v = 0.f;
    if (lin >= 0 && r < rows) {
      if (bias) {
        if (has_bias) v = p[Ly.g_b[lin] + r0 + r];
      } else if (c < cols) {
        bool keep = true;
        if (mk == 1) keep = mnle_hdeg(r, P.V) >= c + 1;
        else if (mk == 2) keep = mnle_hdeg(r, P.V) >= mnle_hdeg(c, P.V);
        else if (mk == 3) keep = (r0 + r) / P.Kmax + 1 > mnle_hdeg(c, P.V);
        if (keep) v = p[Ly.g_w[lin] + (r0 + r) * ld + c0 + c];
      }
    }
    img[idx] = v;
  }
}
// blockIdx.y: 0 initial, 1 final, 2 + 2b + {0, 1}: the blocks' masked linears
__global__ void __launch_bounds__(256)
mnle_mask_kernel(const MnlePlan P, const MnleLayout Ly, float* __restrict__ mask) {
  const int m = blockIdx.y;
  int lin, rows, cols, mk;
  if (m == 0) { lin = 0; rows = P.Hd; cols = P.F; mk = 1; }
  else if (m == 1) { lin = 2 + 3 * P.NB; rows = P.F * P.Kmax; cols = P.Hd; mk = 3; }
  else { lin = 2 + 3 * ((m - 2) >> 1) + ((m - 2) & 1); rows = P.Hd; cols = P.Hd; mk = 2; }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows * cols; i += gridDim.x * blockDim.x) {
    const int r = i / cols, c = i - r * cols;
    bool keep;
    if (mk == 1) keep = mnle_hdeg(r, P.V) >= c + 1;
    else if (mk == 2) keep = mnle_hdeg(r, P.V) >= mnle_hdeg(c, P.V);
    else keep = r / P.Kmax + 1 > mnle_hdeg(c, P.V);
    mask[Ly.g_w[lin] + i] = keep ? 1.f : 0.f;
  }
}

extern "C" int64_t sbi_amd_mnle_param_count(const sbi_amd_mnle_config* cfg) {
  MnlePlan P;
  const int rc = mnle_build_plan(cfg, &P, nullptr);
  return rc ? rc : P.n_params;
}
extern "C" int64_t sbi_amd_mnle_packed_floats(const sbi_amd_mnle_config* cfg) {
  MnlePlan P;
  const int rc = mnle_build_plan(cfg, &P, nullptr);
  return rc ? rc : (int64_t)P.img_floats + P.n_virtual;
}
extern "C" int64_t sbi_amd_mnle_param_offset(const sbi_amd_mnle_config* cfg, int32_t which, int32_t bias) {
  MnlePlan P;
  MnleLayout Ly;
  const int rc = mnle_build_plan(cfg, &P, &Ly);
  if (rc) return rc;
  if (which < 0 || which >= P.n_lin) return SBI_AMD_E_BADARG;
  return bias ? Ly.g_b[which] : Ly.g_w[which];
}

extern "C" int sbi_amd_mnle_pack(const sbi_amd_mnle_config* cfg, const float* params, float* packed, void* stream) {
  MnlePlan P;
  MnleLayout Ly;
  const int rc = mnle_build_plan(cfg, &P, &Ly);
  if (rc) return rc;
  if (!params || !packed) return SBI_AMD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int total = P.img_floats + P.n_virtual;
  hipLaunchKernelGGL(mnle_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, st, P, Ly, params, packed);
  hipLaunchKernelGGL(mnle_mask_kernel, dim3(20, 2 + 2 * P.NB), dim3(256), 0, st, P, Ly, packed + P.img_floats);
  return (int)hipGetLastError();
}

static int mnle_launch_logp(const MnlePlan& P, const float* packed, const float* zstats, const float* x_cont,
                            const int32_t* d_idx, const float* d_val, const float* c, int64_t n, int64_t c_rows,
                            int64_t x_div, int parts, float* out, float* logits, hipStream_t st) {
  MnleCall q;
  memset(&q, 0, sizeof(q));
  q.mode = 0; q.nw = mnle_waves(n); q.lds_bytes = mnle_lds(P, q.nw);
  if (q.lds_bytes > NSF_LDS_LIMIT_BYTES) return SBI_AMD_E_LDS;
  q.packed = packed; q.zstats = zstats; q.x_cont = x_cont; q.d_idx = d_idx; q.d_val = d_val; q.c = c;
  q.n = n; q.c_rows = c_rows; q.x_div = x_div; q.parts = parts; q.out0 = out; q.out1 = logits;
  return mnle_dispatch(P, q, st);
}

extern "C" int sbi_amd_mnle_log_prob(const sbi_amd_mnle_config* cfg, const float* packed, const float* zstats,
                                     const float* x_cont, const int32_t* d_idx, const float* d_val, const float* c,
                                     int64_t n, int64_t c_rows, int32_t parts, float* logp_out, float* logits_out,
                                     void* stream) {
  MnlePlan P;
  const int rc = mnle_build_plan(cfg, &P, nullptr);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!packed || !zstats || !c || !logp_out || n < 0 || c_rows < 1 || (parts & 3) == 0 || (parts & ~3))
    return SBI_AMD_E_BADARG;
  if ((parts & 1) && !d_idx) return SBI_AMD_E_BADARG;
  if ((parts & 2) && (!x_cont || !d_val)) return SBI_AMD_E_BADARG;
  if (logits_out && !(parts & 1)) return SBI_AMD_E_BADARG;
  return mnle_launch_logp(P, packed, zstats, x_cont, d_idx, d_val, c, n, c_rows, 1, parts, logp_out, logits_out,
                          (hipStream_t)stream);
}

extern "C" int sbi_amd_mnle_log_prob_trials(const sbi_amd_mnle_config* cfg, const float* packed, const float* zstats,
                                            const float* x_cont, const int32_t* d_idx, const float* d_val,
                                            const float* c, int64_t num_trials, int64_t num_cond, float* out,
                                            float* workspace, void* stream) {
  MnlePlan P;
  const int rc = mnle_build_plan(cfg, &P, nullptr);
  if (rc) return rc;
  if (num_cond == 0) return 0;
  if (!packed || !zstats || !x_cont || !d_idx || !d_val || !c || !out || !workspace || num_trials < 1 || num_cond < 0)
    return SBI_AMD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  // row r = t * num_cond + j: trial t against condition j, one pair per row of the paired kernel
  const int rc2 = mnle_launch_logp(P, packed, zstats, x_cont, d_idx, d_val, c, num_trials * num_cond, num_cond,
                                   num_cond, 3, workspace, nullptr, st);
  if (rc2) return rc2;
  hipLaunchKernelGGL(mnle_trial_sum_kernel, dim3((unsigned)((num_cond + 255) / 256)), dim3(256), 0, st, workspace,
                     (long long)num_trials, (long long)num_cond, out);
  return (int)hipGetLastError();
}

extern "C" int sbi_amd_mnle_sample(const sbi_amd_mnle_config* cfg, const float* packed, const float* zstats,
                                   const float* u, const float* noise, const float* c, int64_t n, int64_t c_rows,
                                   int32_t* d_idx_out, float* x_cont_out, void* stream) {
  MnlePlan P;
  const int rc = mnle_build_plan(cfg, &P, nullptr);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!packed || !zstats || !u || !noise || !c || !d_idx_out || !x_cont_out || n < 0 || c_rows < 1)
    return SBI_AMD_E_BADARG;
  MnleCall q;
  memset(&q, 0, sizeof(q));
  q.mode = 1; q.nw = mnle_waves(n); q.lds_bytes = mnle_lds(P, q.nw);
  if (q.lds_bytes > NSF_LDS_LIMIT_BYTES) return SBI_AMD_E_LDS;
  q.packed = packed; q.zstats = zstats; q.x_cont = noise; q.d_val = u; q.c = c;
  q.n = n; q.c_rows = c_rows; q.x_div = 1; q.out0 = x_cont_out; q.idx_out = d_idx_out;
  return mnle_dispatch(P, q, (hipStream_t)stream);
}

// ---- training workspace layout (floats)
struct MnleWs {
  int64_t ctx, din, act, g, gf, gp, part, gtmp, total, npad;
  int nchunks, aslots, gslots;
};
static MnleWs mnle_ws_layout(const MnlePlan& P, int64_t n) {
  MnleWs w;
  int64_t o = 0;
  auto take = [&](int64_t sz) { const int64_t at = o; o += (sz + 3) / 4 * 4; return at; };
  w.npad = (n + MAF_DW_CHUNK - 1) / MAF_DW_CHUNK * MAF_DW_CHUNK;   // the dW kernel reads whole chunks
  w.nchunks = (int)(w.npad / MAF_DW_CHUNK);
  w.aslots = 2 * P.NB + 1 + 2 + P.T * (P.L + 1);
  w.gslots = 2 + 3 * P.NB + 2 + P.T * (P.L + 1);
  w.ctx = take(w.npad * 64);
  w.din = take(w.npad * MNLE_DA);
  w.act = take(w.npad * 64 * w.aslots);
  w.g = take(w.npad * 64 * w.gslots);
  w.gf = take(w.npad * 16 * P.PF);
  w.gp = take(w.npad * 16 * P.PT * P.T);
  w.part = take((int64_t)w.nchunks * P.n_virtual);
  w.gtmp = take(P.n_virtual);
  w.total = o;
  return w;
}

extern "C" int64_t sbi_amd_mnle_train_workspace_floats(const sbi_amd_mnle_config* cfg, int64_t n) {
  MnlePlan P;
  const int rc = mnle_build_plan(cfg, &P, nullptr);
  if (rc) return rc;
  return mnle_ws_layout(P, n > 0 ? n : 1).total;
}

extern "C" int sbi_amd_mnle_loss_fwd_bwd(const sbi_amd_mnle_config* cfg, const float* packed, const float* zstats,
                                         const float* x_cont, const int32_t* d_idx, const float* d_val,
                                         const float* c, int64_t n, int64_t c_rows, const float* row_weight,
                                         float uniform_weight, float* loss_out, float* grad_out, float* grad_cond_out,
                                         float* workspace, void* stream) {
  MnlePlan P;
  MnleLayout Ly;
  int rc = mnle_build_plan(cfg, &P, &Ly);
  if (rc) return rc;
  if (!grad_out || n < 0) return SBI_AMD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return (int)hipMemsetAsync(grad_out, 0, sizeof(float) * (size_t)P.n_params, st);
  if (!packed || !zstats || !x_cont || !d_idx || !d_val || !c || !workspace || c_rows < 1) return SBI_AMD_E_BADARG;
  if (grad_cond_out && c_rows != n) return SBI_AMD_E_BADARG;
  const MnleWs w = mnle_ws_layout(P, n);
  MnleBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.packed = packed; a.zstats = zstats; a.x_cont = x_cont; a.d_idx = d_idx; a.d_val = d_val; a.c = c;
  a.row_w = row_weight; a.uni_w = uniform_weight;
  a.n = n; a.c_rows = c_rows; a.npad = w.npad;
  a.loss = loss_out; a.grad_cond = grad_cond_out;
  a.CTX = workspace + w.ctx; a.DIN = workspace + w.din; a.ACT = workspace + w.act; a.G = workspace + w.g;
  a.GF = workspace + w.gf; a.GP = workspace + w.gp;
  MnleCall q;
  memset(&q, 0, sizeof(q));
  q.mode = 2; q.nw = mnle_waves(n); q.lds_bytes = mnle_lds(P, q.nw);
  if (q.lds_bytes > NSF_LDS_LIMIT_BYTES) return SBI_AMD_E_LDS;
  q.n = n; q.bwd = &a;
  rc = mnle_dispatch(P, q, st);
  if (rc) return rc;

  // ---- weight gradients: one MafLin per linear (and per later application of a shared context layer, whose
  // gradient goes to a virtual parameter block behind the real ones and is folded in afterwards)
  const int64_t gts = w.npad * 16, slot = w.npad * 64;
  std::vector<MafLin> lins;
  auto add = [&](const float* G, const float* A, int lda, int out, int in, int in_total, int col0, int gpad, int g_w,
                 int g_b, int gperm, int aperm) {
    MafLin L;
    memset(&L, 0, sizeof(L));
    L.G = G; L.gts = gts; L.A = A; L.lda = lda;
    L.out = out; L.in = in; L.in_total = in_total; L.col0 = col0;
    L.group = out; L.group_pad = gpad;
    L.g_w = g_w; L.g_b = g_b;
    L.kind = 1;
    L.gperm = gperm; L.aperm = aperm;
    lins.push_back(L);
  };
  auto G64 = [&](int s) { return a.G + (int64_t)s * slot; };
  auto ACT = [&](int s) { return a.ACT + (int64_t)s * slot; };
  add(G64(0), a.DIN, MNLE_DA, P.Hd, P.F, P.F, 0, 64, Ly.g_w[0], Ly.g_b[0], 1, 0);
  add(G64(1), a.CTX, 64, P.Hd, P.C, P.C, 0, 64, Ly.g_w[1], Ly.g_b[1], 1, 0);
  for (int b = 0; b < P.NB; ++b) {
    const int l0 = 2 + 3 * b;
    add(G64(l0), ACT(2 * b), 64, P.Hd, P.Hd, P.Hd, 0, 64, Ly.g_w[l0], Ly.g_b[l0], 1, 1);
    add(G64(l0 + 1), ACT(2 * b + 1), 64, P.Hd, P.Hd, P.Hd, 0, 64, Ly.g_w[l0 + 1], Ly.g_b[l0 + 1], 1, 1);
    add(G64(l0 + 2), a.CTX, 64, P.Hd, P.C, P.C, 0, 64, Ly.g_w[l0 + 2], Ly.g_b[l0 + 2], 1, 0);
  }
  const int lf = 2 + 3 * P.NB;
  add(a.GF, ACT(2 * P.NB), 64, P.F * P.Kmax, P.Hd, P.Hd, 0, 16 * P.PF, Ly.g_w[lf], Ly.g_b[lf], 0, 1);
  const int slot0 = 2 * P.NB + 1, gslot0 = 2 + 3 * P.NB;
  add(G64(gslot0), a.DIN + 8, MNLE_DA, P.E, P.V, P.V + P.C, 0, 64, Ly.g_w[lf + 1], Ly.g_b[lf + 1], 1, 0);
  add(G64(gslot0), a.CTX, 64, P.E, P.C, P.V + P.C, P.V, 64, Ly.g_w[lf + 1], Ly.g_b[lf + 1], 1, 0);
  add(G64(gslot0 + 1), ACT(slot0), 64, P.E, P.E, P.E, 0, 64, Ly.g_w[lf + 2], Ly.g_b[lf + 2], 1, 1);
  const int per = P.L > 0 ? 3 : 2, blk = P.Hc * P.Hc + P.Hc;
  for (int t = 0; t < P.T; ++t) {
    const int base = lf + 3 + t * per, as = slot0 + 2 + t * (P.L + 1), gsl = gslot0 + 2 + t * (P.L + 1);
    add(G64(gsl), ACT(slot0 + 1), 64, P.Hc, P.E, P.E, 0, 64, Ly.g_w[base], Ly.g_b[base], 1, 1);
    for (int l = 0; l < P.L; ++l) {
      const int gw = l == 0 ? Ly.g_w[base + 1] : P.n_params + (t * (P.L - 1) + (l - 1)) * blk;
      add(G64(gsl + 1 + l), ACT(as + l), 64, P.Hc, P.Hc, P.Hc, 0, 64, gw, gw + P.Hc * P.Hc, 1, 1);
    }
    add(a.GP + (int64_t)t * P.PT * gts, ACT(as + P.L), 64, P.P, P.Hc, P.Hc, 0, 16 * P.PT, Ly.g_w[base + per - 1],
        Ly.g_b[base + per - 1], 0, 1);
  }
  float* partial = workspace + w.part;
  for (size_t i0 = 0; i0 < lins.size(); i0 += MAF_DW_MAX_LIN) {
    MafDwArgs d;
    memset(&d, 0, sizeof(d));
    const int nl = (int)(lins.size() - i0 < MAF_DW_MAX_LIN ? lins.size() - i0 : MAF_DW_MAX_LIN);
    for (int i = 0; i < nl; ++i) d.lin[i] = lins[i0 + i];
    d.n = n; d.rows_per_chunk = MAF_DW_CHUNK; d.nchunks = w.nchunks; d.n_layer = P.n_virtual;
    d.D = 2; d.P = 1;
    d.partial = partial;
    d.mask = packed + P.img_floats;
    rc = maf_launch_dw(d, nl, st);
    if (rc) return rc;
  }
  if (P.n_virtual == P.n_params) return maf_launch_reduce(partial, grad_out, P.n_params, w.nchunks, 1, st);
  rc = maf_launch_reduce(partial, workspace + w.gtmp, P.n_virtual, w.nchunks, 1, st);
  if (rc) return rc;
  hipLaunchKernelGGL(mnle_fold_kernel, dim3((P.n_params + 255) / 256), dim3(256), 0, st, P, Ly, workspace + w.gtmp,
                     grad_out);
  return (int)hipGetLastError();
}
