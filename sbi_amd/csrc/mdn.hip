// mdn.hip -- host side of the mixture-density-network path (plan, C ABI of include/sbi_amd_mdn.h) and its kernel
// instantiations.  The weight gradients reuse the MAF path's split-K kernels (maf_launch_dw / maf_launch_reduce).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include "mdn_kernel.h"

static int d_round_up(int v, int m) { return (v + m - 1) / m * m; }
static int d_two_odd(int v) {
  int x = (v + 1) / 2;
  if ((x & 1) == 0) x += 1;
  return 2 * x;
}

static int mdn_build_plan(const sbi_amd_mdn_config* c, MdnPlan* P) {
  if (!c) return SBI_AMD_E_BADARG;
  if (!(c->epsilon >= 0.f)) return SBI_AMD_E_BADARG;
  if (c->D < 1 || c->C < 1 || c->H < 1 || c->K < 1 || c->D > 16 || c->C > 64 || c->H > 64 || c->K > 16)
    return SBI_AMD_E_UNSUPPORTED;
  memset(P, 0, sizeof(*P));
  const int D = c->D, C = c->C, H = c->H, K = c->K;
  P->D = D; P->C = C; P->H = H; P->K = K;
  P->U = D * (D - 1) / 2;
  P->R = 1 + 2 * D + P->U;
  P->MT = (P->R + 15) / 16;
  P->RP = 16 * P->MT;
  P->KS1 = (C + 3) / 4;
  P->ld1 = d_two_odd(4 * P->KS1);
  int o = 0;
  P->o_w1 = o; o += 64 * P->ld1;
  P->o_b1 = o; o += 64;
  P->o_w2 = o; o += 64 * MDN_LDH;
  P->o_b2 = o; o += 64;
  P->o_lg = o; o += 16 * MDN_LDH;
  P->o_lgb = o; o += 16;
  P->hid_floats = d_round_up(o, 4);
  P->slice_floats = P->RP * MDN_LDH + P->RP;
  P->img_floats = P->hid_floats + K * P->slice_floats;
  const int outs[6] = {H, H, K, K * D, K * D, K * P->U}, ins[6] = {C, H, H, H, H, H};
  int g = 0;
  for (int i = 0; i < 6; ++i) {
    P->g_w[i] = g; g += outs[i] * ins[i];
    P->g_b[i] = g; g += outs[i];
  }
  P->n_params = g;
  P->SW = P->RP + 4;
  int s = 0;
  P->sc_z = s; s += 16 * MDN_ZW;
  P->sc_y = s; s += 16 * MDN_ZW;
  P->sc_t = s; s += 16 * MDN_ZW;
  s = d_round_up(s, 4);
  P->sc_c = s; s += 16 * P->ld1;
  s = d_round_up(s, 4);
  P->sc_s = s;
  s += 16 * P->SW;
  P->sc_total = d_round_up(s, 4);
  s = 0;
  P->bc_z = s; s += 16 * MDN_ZW;
  P->bc_c = s; s += 16 * P->ld1;
  P->bc_x = s; s += 64 * MDN_ZW;                   // the one-observation sampler: one back-substitution row per lane
  P->bc_total = d_round_up(s, 4);
  P->eps = c->epsilon;
  P->log_z = (float)(0.5 * D * log(2.0 * M_PI));
  return 0;
}
static int mdn_ksh(const MdnPlan& P) { return (P.H + 3) / 4 <= 13 ? 13 : 16; }
static int mdn_paired_lds(const MdnPlan& P, int nw) { return 4 * (P.hid_floats + P.slice_floats + nw * P.sc_total); }
static int mdn_bcast_lds(const MdnPlan& P, int nw) {
  return 4 * (P.hid_floats + P.K * P.RP + P.slice_floats + nw * P.bc_total);
}
// largest workgroup (4, 2, 1 waves) that fits LDS and still yields >= 256 workgroups
static int mdn_waves(const MdnPlan& P, int64_t n) {
  int nw = 4;
  while (nw > 1 && ((n + 16 * nw - 1) / (16 * nw) < 256 || mdn_paired_lds(P, nw) > NSF_LDS_LIMIT_BYTES)) nw >>= 1;
  return nw;
}

__global__ void __launch_bounds__(256)
mdn_pack_kernel(const MdnPlan P, const float* __restrict__ p, float* __restrict__ img) {
  const int D = P.D, H = P.H, K = P.K, U = P.U;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < P.img_floats; idx += gridDim.x * blockDim.x) {
    float v = 0.f;
    if (idx < P.o_b1) {
      const int r = idx / P.ld1, c = idx - r * P.ld1;
      if (r < H && c < P.C) v = p[P.g_w[0] + r * P.C + c];
    } else if (idx < P.o_w2) {
      const int r = idx - P.o_b1;
      if (r < H) v = p[P.g_b[0] + r];
    } else if (idx < P.o_b2) {
      const int o = idx - P.o_w2, r = o / MDN_LDH, c = o - r * MDN_LDH;
      if (r < H && c < H) v = p[P.g_w[1] + r * H + c];
    } else if (idx < P.o_lg) {
      const int r = idx - P.o_b2;
      if (r < H) v = p[P.g_b[1] + r];
    } else if (idx < P.o_lgb) {
      const int o = idx - P.o_lg, r = o / MDN_LDH, c = o - r * MDN_LDH;
      if (r < K && c < H) v = p[P.g_w[2] + r * H + c];
    } else if (idx < P.hid_floats) {
      const int r = idx - P.o_lgb;
      if (r < K) v = p[P.g_b[2] + r];
    } else {
      const int o = idx - P.hid_floats, k = o / P.slice_floats, q = o - k * P.slice_floats;
      const bool bias = q >= P.RP * MDN_LDH;
      const int r = bias ? q - P.RP * MDN_LDH : q / MDN_LDH;
      const int c = bias ? 0 : q - r * MDN_LDH;
      if (r < P.R && c < H) {
        int which, sr;
        if (r == 0) { which = 2; sr = k; }
        else if (r < 1 + D) { which = 3; sr = k * D + r - 1; }
        else if (r < 1 + 2 * D) { which = 4; sr = k * D + r - 1 - D; }
        else { which = 5; sr = k * U + r - 1 - 2 * D; }
        v = bias ? p[P.g_b[which] + sr] : p[P.g_w[which] + sr * H + c];
      }
    }
    img[idx] = v;
  }
}

extern "C" int64_t sbi_amd_mdn_param_count(const sbi_amd_mdn_config* cfg) {
  MdnPlan P;
  const int rc = mdn_build_plan(cfg, &P);
  return rc ? rc : P.n_params;
}
extern "C" int64_t sbi_amd_mdn_packed_floats(const sbi_amd_mdn_config* cfg) {
  MdnPlan P;
  const int rc = mdn_build_plan(cfg, &P);
  return rc ? rc : P.img_floats;
}
extern "C" int64_t sbi_amd_mdn_param_offset(const sbi_amd_mdn_config* cfg, int32_t which, int32_t bias) {
  MdnPlan P;
  const int rc = mdn_build_plan(cfg, &P);
  if (rc) return rc;
  if (which < 0 || which > 5 || (which == 5 && P.U == 0)) return SBI_AMD_E_BADARG;
  return bias ? P.g_b[which] : P.g_w[which];
}

extern "C" int sbi_amd_mdn_pack(const sbi_amd_mdn_config* cfg, const float* params, float* packed, void* stream) {
  MdnPlan P;
  const int rc = mdn_build_plan(cfg, &P);
  if (rc) return rc;
  if (!params || !packed) return SBI_AMD_E_BADARG;
  hipLaunchKernelGGL(mdn_pack_kernel, dim3((P.img_floats + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, params,
                     packed);
  return (int)hipGetLastError();
}

template <int KSH, int MODE>
static int mdn_launch_flow(const MdnPlan& P, const float* packed, const float* zstats, const float* in, const float* x,
                           const float* u, const int* comp, int64_t n, int64_t x_rows, float* o0, float* o1, float* o2,
                           hipStream_t st) {
  const int nw = mdn_waves(P, n);
  const int lds_bytes = mdn_paired_lds(P, nw);
  if (lds_bytes > NSF_LDS_LIMIT_BYTES) return SBI_AMD_E_LDS;
  auto kern = mdn_flow_kernel<KSH, MODE>;
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (e != hipSuccess) return (int)e;
  const int64_t grid = (n + 16 * nw - 1) / (16 * nw);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * nw), (size_t)lds_bytes, st, P, packed, zstats, in, x, u,
                     comp, (long long)n, (long long)x_rows, o0, o1, o2);
  return (int)hipGetLastError();
}
template <int KSH, int MODE>
static int mdn_launch_bcast(const MdnPlan& P, const float* packed, const float* zstats, const float* in,
                            const float* x, const float* u, const int* comp, int64_t n, float* o0, hipStream_t st) {
  const int nw = 4;
  const int lds_bytes = mdn_bcast_lds(P, nw);
  if (lds_bytes > NSF_LDS_LIMIT_BYTES) return SBI_AMD_E_LDS;
  auto kern = mdn_bcast_kernel<KSH, MODE>;
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (e != hipSuccess) return (int)e;
  // every workgroup pays one network evaluation (the head once through LDS): one row group per wave until the chip
  // is covered twice, the workgroups then loop
  const int64_t units = (n + (MODE == 0 ? 16 : 64) - 1) / (MODE == 0 ? 16 : 64);
  int64_t grid = (units + nw - 1) / nw;
  if (grid > 512) grid = 512;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * nw), (size_t)lds_bytes, st, P, packed, zstats, in, x, u,
                     comp, (long long)n, o0);
  return (int)hipGetLastError();
}
#define MDN_KSH_SWITCH(P, CALL13, CALL16) (mdn_ksh(P) == 13 ? (CALL13) : (CALL16))

extern "C" int sbi_amd_mdn_components(const sbi_amd_mdn_config* cfg, const float* packed, const float* zstats,
                                      const float* x, int64_t n, float* logits_out, float* means_out,
                                      float* factors_out, void* stream) {
  MdnPlan P;
  const int rc = mdn_build_plan(cfg, &P);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!packed || !zstats || !x || !logits_out || !means_out || !factors_out || n < 0) return SBI_AMD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  return MDN_KSH_SWITCH(P,
      (mdn_launch_flow<13, 2>(P, packed, zstats, nullptr, x, nullptr, nullptr, n, n, logits_out, means_out, factors_out, st)),
      (mdn_launch_flow<16, 2>(P, packed, zstats, nullptr, x, nullptr, nullptr, n, n, logits_out, means_out, factors_out, st)));
}

extern "C" int sbi_amd_mdn_log_prob(const sbi_amd_mdn_config* cfg, const float* packed, const float* zstats,
                                    const float* theta, const float* x, int64_t n, int64_t x_rows, float* logp_out,
                                    void* stream) {
  MdnPlan P;
  const int rc = mdn_build_plan(cfg, &P);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!packed || !zstats || !theta || !x || !logp_out || n < 0 || x_rows < 1) return SBI_AMD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (x_rows == 1)
    return MDN_KSH_SWITCH(P,
        (mdn_launch_bcast<13, 0>(P, packed, zstats, theta, x, nullptr, nullptr, n, logp_out, st)),
        (mdn_launch_bcast<16, 0>(P, packed, zstats, theta, x, nullptr, nullptr, n, logp_out, st)));
  return MDN_KSH_SWITCH(P,
      (mdn_launch_flow<13, 0>(P, packed, zstats, theta, x, nullptr, nullptr, n, x_rows, logp_out, nullptr, nullptr, st)),
      (mdn_launch_flow<16, 0>(P, packed, zstats, theta, x, nullptr, nullptr, n, x_rows, logp_out, nullptr, nullptr, st)));
}

extern "C" int sbi_amd_mdn_sample(const sbi_amd_mdn_config* cfg, const float* packed, const float* zstats,
                                  const float* u, const int32_t* comp, const float* zeta, const float* x, int64_t n,
                                  int64_t x_rows, float* theta_out, void* stream) {
  MdnPlan P;
  const int rc = mdn_build_plan(cfg, &P);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!packed || !zstats || (!u && !comp) || !zeta || !x || !theta_out || n < 0 || x_rows < 1) return SBI_AMD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (x_rows == 1)
    return MDN_KSH_SWITCH(P,
        (mdn_launch_bcast<13, 1>(P, packed, zstats, zeta, x, u, comp, n, theta_out, st)),
        (mdn_launch_bcast<16, 1>(P, packed, zstats, zeta, x, u, comp, n, theta_out, st)));
  return MDN_KSH_SWITCH(P,
      (mdn_launch_flow<13, 1>(P, packed, zstats, zeta, x, u, comp, n, x_rows, theta_out, nullptr, nullptr, st)),
      (mdn_launch_flow<16, 1>(P, packed, zstats, zeta, x, u, comp, n, x_rows, theta_out, nullptr, nullptr, st)));
}

// ---- training workspace layout (floats)
struct MdnWs {
  int64_t ctx, act1, act2, g1, g2, gh[4], part, total, npad;
  int planes[4], nchunks;
};
static MdnWs mdn_ws_layout(const MdnPlan& P, int64_t n) {
  MdnWs w;
  int64_t o = 0;
  auto take = [&](int64_t sz) { const int64_t at = o; o += (sz + 3) / 4 * 4; return at; };
  w.npad = (n + MAF_DW_CHUNK - 1) / MAF_DW_CHUNK * MAF_DW_CHUNK;   // the dW kernel reads whole chunks
  w.nchunks = (int)(w.npad / MAF_DW_CHUNK);
  w.ctx = take(w.npad * MDN_AW);
  w.act1 = take(w.npad * MDN_AW);
  w.act2 = take(w.npad * MDN_AW);
  w.g1 = take(w.npad * 16 * 4);
  w.g2 = take(w.npad * 16 * 4);
  const int outs[4] = {P.K, P.K * P.D, P.K * P.D, P.K * P.U};
  for (int i = 0; i < 4; ++i) {
    w.planes[i] = (outs[i] + 15) / 16;
    w.gh[i] = take(w.npad * 16 * w.planes[i]);
  }
  w.part = take((int64_t)w.nchunks * P.n_params);
  w.total = o;
  return w;
}

extern "C" int64_t sbi_amd_mdn_train_workspace_floats(const sbi_amd_mdn_config* cfg, int64_t n) {
  MdnPlan P;
  const int rc = mdn_build_plan(cfg, &P);
  if (rc) return rc;
  return mdn_ws_layout(P, n > 0 ? n : 1).total;
}

template <int KSH>
static int mdn_launch_bwd(const MdnPlan& P, const MdnBwdArgs& a, hipStream_t st) {
  const int nw = mdn_waves(P, a.n);
  const int lds_bytes = mdn_paired_lds(P, nw);
  if (lds_bytes > NSF_LDS_LIMIT_BYTES) return SBI_AMD_E_LDS;
  auto kern = mdn_bwd_kernel<KSH>;
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (e != hipSuccess) return (int)e;
  const int64_t grid = (a.n + 16 * nw - 1) / (16 * nw);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * nw), (size_t)lds_bytes, st, P, a);
  return (int)hipGetLastError();
}

extern "C" int sbi_amd_mdn_loss_fwd_bwd(const sbi_amd_mdn_config* cfg, const float* packed, const float* zstats,
                                        const float* theta, const float* x, int64_t n, int64_t x_rows,
                                        const float* row_weight, float uniform_weight, float* loss_out,
                                        float* grad_out, float* grad_theta_out, float* workspace, void* stream) {
  MdnPlan P;
  int rc = mdn_build_plan(cfg, &P);
  if (rc) return rc;
  if (!grad_out || n < 0) return SBI_AMD_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0)       // no rows: the gradient of an empty sum
    return (int)hipMemsetAsync(grad_out, 0, sizeof(float) * (size_t)P.n_params, st);
  if (!packed || !zstats || !theta || !x || !workspace || x_rows < 1) return SBI_AMD_E_BADARG;
  const MdnWs w = mdn_ws_layout(P, n);
  MdnBwdArgs a;
  a.packed = packed; a.zstats = zstats; a.theta = theta; a.x = x;
  a.row_w = row_weight; a.uni_w = uniform_weight;
  a.n = n; a.x_rows = x_rows; a.npad = w.npad;
  a.loss = loss_out; a.grad_theta = grad_theta_out;
  a.CTX = workspace + w.ctx; a.ACT1 = workspace + w.act1; a.ACT2 = workspace + w.act2;
  a.G1 = workspace + w.g1; a.G2 = workspace + w.g2;
  for (int i = 0; i < 4; ++i) a.GH[i] = workspace + w.gh[i];
  rc = MDN_KSH_SWITCH(P, (mdn_launch_bwd<13>(P, a, st)), (mdn_launch_bwd<16>(P, a, st)));
  if (rc) return rc;
  MafDwArgs d;
  memset(&d, 0, sizeof(d));
  const int64_t gts = w.npad * 16;
  int nl = 0;
  auto set = [&](const float* G, const float* A, int out, int in, int gpad, int which, int gperm, int aperm) {
    if (out == 0) return;
    MafLin& L = d.lin[nl++];
    L.G = G; L.gts = gts; L.A = A; L.lda = MDN_AW;
    L.out = out; L.in = in; L.in_total = in; L.col0 = 0;
    L.group = out; L.group_pad = gpad;
    L.g_w = P.g_w[which]; L.g_b = P.g_b[which];
    L.kind = 1;                       // dense: no autoregressive mask
    L.gperm = gperm; L.aperm = aperm;
  };
  // largest first; the heads' gradient planes are in natural column order, the hidden layers' in fragment order
  set(a.GH[3], a.ACT2, P.K * P.U, P.H, 16 * w.planes[3], 5, 0, 1);
  set(a.GH[1], a.ACT2, P.K * P.D, P.H, 16 * w.planes[1], 3, 0, 1);
  set(a.GH[2], a.ACT2, P.K * P.D, P.H, 16 * w.planes[2], 4, 0, 1);
  set(a.GH[0], a.ACT2, P.K, P.H, 16, 2, 0, 1);
  set(a.G2, a.ACT1, P.H, P.H, 64, 1, 1, 1);
  set(a.G1, a.CTX, P.H, P.C, 64, 0, 1, 0);
  d.n = n; d.rows_per_chunk = MAF_DW_CHUNK; d.nchunks = w.nchunks; d.n_layer = P.n_params;
  d.D = 2; d.P = 1;
  d.partial = workspace + w.part;
  rc = maf_launch_dw(d, nl, st);
  if (rc) return rc;
  return maf_launch_reduce(workspace + w.part, grad_out, P.n_params, w.nchunks, 1, st);
}
