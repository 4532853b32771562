// tr_embed.hip -- C ABI of TransformerEmbedding (include/sbi_amd_tr.h); kernels in tr_embed_kernel.h.
#include <mutex>
#include "tr_embed_kernel.h"

// The dynamic-LDS limit sticks to (device, kernel): raise it only when a launch needs more than any launch before it.
#define TR_CACHED_DEVICES 64
static int tr_set_lds(int which, const void* kern, int lds_bytes) {
  static std::mutex lock;
  static int have[TR_CACHED_DEVICES][7];      // one slot per kernel with dynamic LDS
  if (lds_bytes <= 48 * 1024) return 0;
  int dev = -1;
  const bool cached = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < TR_CACHED_DEVICES;
  std::lock_guard<std::mutex> guard(lock);
  if (cached && have[dev][which] >= lds_bytes) return 0;
  const int e = (int)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (!e && cached) have[dev][which] = lds_bytes;
  return e;
}

extern "C" int64_t sbi_amd_tr_param_count(const sbi_amd_tr_config* cfg, int64_t* offsets) {
  TrPlan pl;
  const int rc = tr_plan_sizes(cfg, &pl);
  if (rc) return rc;
  if (offsets) {
    int n = 0;
    offsets[n++] = pl.p_spw;
    offsets[n++] = pl.p_spb;
    for (int l = 0; l < pl.L; ++l) {
      const int64_t base = pl.p_layer0 + l * pl.PL;
      offsets[n++] = base + pl.o_ow;
      offsets[n++] = base + pl.o_qkv;
      offsets[n++] = base + pl.o_gu;
      offsets[n++] = base + pl.o_down;
      offsets[n++] = base + pl.o_ln1;
      offsets[n++] = base + pl.o_ln2;
    }
    offsets[n++] = pl.p_norm;
    offsets[n++] = pl.p_aggw;
    offsets[n++] = pl.p_aggb;
  }
  return pl.P;
}

extern "C" int sbi_amd_tr_plan(const sbi_amd_tr_config* cfg, int64_t B, int64_t T, int32_t* lds_bytes,
                               int32_t* key_tile, int32_t* partials) {
  TrPlan pl;
  TrShape sh;
  const int rc = tr_build_plan(cfg, B, T, &pl, &sh);
  if (rc && rc != SBI_AMD_E_LDS) return rc;
  if (lds_bytes)
    for (int i = 0; i < 6; ++i) lds_bytes[i] = pl.lds[i] * 4;
  if (key_tile) *key_tile = 64;
  if (partials) *partials = (int32_t)sh.G;
  return rc;
}

extern "C" int64_t sbi_amd_tr_workspace_bytes(const sbi_amd_tr_config* cfg, int64_t B, int64_t T, int32_t training) {
  TrPlan pl;
  TrShape sh;
  const int rc = tr_build_plan(cfg, B, T, &pl, &sh);
  if (rc) return rc;
  return tr_workspace_floats(pl, sh, training) * 4;
}

static void tr_block_buffers(const TrPlan& pl, const TrShape& sh, float* ws, int layer, int training, TrArgs* a) {
  float* base = ws + (training ? layer * sh.LS : 0);
  a->h_in = base;
  a->q = base + sh.Q;
  a->k = a->q + sh.Q;
  a->v = a->k + sh.K;
  a->attn = a->v + sh.K;
  a->lse = a->attn + sh.Q;
  a->h1 = a->lse + sh.S;
  a->h_out = training ? base + sh.LS : base;      // the next block's input; in place without a stash
  a->layer = layer;
}

static int tr_fill_args(const TrPlan& pl, const TrShape& sh, TrArgs* a, const float* params, const float* x,
                        int64_t xbs, int64_t xts, float p, uint64_t seed) {
  if (!params || !x || xbs < 0 || xts < 0) return SBI_AMD_E_BADARG;
  if (!(p >= 0.f && p < 1.f)) return SBI_AMD_E_UNSUPPORTED;
  a->params = params; a->x = x; a->xbs = xbs; a->xts = xts;
  a->B = sh.B; a->T = sh.T; a->N = sh.N;
  a->p = p; a->inv_keep = 1.0f / (1.0f - p);
  a->seed_lo = (unsigned)(seed & 0xffffffffu); a->seed_hi = (unsigned)(seed >> 32);
  a->per = sh.per;
  return 0;
}

extern "C" int sbi_amd_tr_forward(const sbi_amd_tr_config* cfg, const float* params, const float* x,
                                  int64_t x_batch_stride, int64_t x_time_stride, int64_t B, int64_t T, float dropout_p,
                                  uint64_t seed, float* out, void* workspace, int32_t training, void* stream) {
  TrPlan pl;
  TrShape sh;
  int rc = tr_build_plan(cfg, B, T, &pl, &sh);
  if (rc) return rc;
  if (!out || !workspace) return SBI_AMD_E_BADARG;
  TrArgs a = {};
  rc = tr_fill_args(pl, sh, &a, params, x, x_batch_stride, x_time_stride, dropout_p, seed);
  if (rc) return rc;
  a.out = out;
  a.training = training ? 1 : 0;
  int e = tr_set_lds(0, (const void*)tr_qkv_kernel, pl.lds[0] * 4);
  if (!e) e = tr_set_lds(1, (const void*)tr_attn_fwd_kernel, pl.lds[1] * 4);
  if (!e) e = tr_set_lds(2, (const void*)tr_tail_kernel, pl.lds[2] * 4);
  if (e) return e;
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const unsigned tiles = (unsigned)sh.tiles;
  const unsigned rows = (unsigned)((sh.S + TR_WAVES - 1) / TR_WAVES);
  tr_block_buffers(pl, sh, ws, 0, a.training, &a);
  hipLaunchKernelGGL(tr_input_kernel, dim3((unsigned)((sh.Q + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0, s,
                     pl, a);
  for (int l = 0; l < pl.L; ++l) {
    tr_block_buffers(pl, sh, ws, l, a.training, &a);
    hipLaunchKernelGGL(tr_qkv_kernel, dim3(tiles), dim3(TR_THREADS), pl.lds[0] * 4, s, pl, a);
    hipLaunchKernelGGL(tr_attn_fwd_kernel, dim3(rows), dim3(TR_THREADS), pl.lds[1] * 4, s, pl, a);
    hipLaunchKernelGGL(tr_tail_kernel, dim3(tiles), dim3(TR_THREADS), pl.lds[2] * 4, s, pl, a);
  }
  a.h_in = a.h_out;
  hipLaunchKernelGGL(tr_final_kernel, dim3((unsigned)B), dim3(128), 0, s, pl, a);
  return (int)hipGetLastError();
}

extern "C" int sbi_amd_tr_backward(const sbi_amd_tr_config* cfg, const float* params, const float* x,
                                   int64_t x_batch_stride, int64_t x_time_stride, int64_t B, int64_t T,
                                   float dropout_p, uint64_t seed, const float* grad_out, float* grad_params,
                                   void* workspace, void* stream) {
  TrPlan pl;
  TrShape sh;
  int rc = tr_build_plan(cfg, B, T, &pl, &sh);
  if (rc) return rc;
  if (!grad_out || !grad_params || !workspace) return SBI_AMD_E_BADARG;
  TrArgs a = {};
  rc = tr_fill_args(pl, sh, &a, params, x, x_batch_stride, x_time_stride, dropout_p, seed);
  if (rc) return rc;
  int e = tr_set_lds(3, (const void*)tr_tail_bwd_kernel, pl.lds[3] * 4);
  if (!e) e = tr_set_lds(4, (const void*)tr_attn_bwd_dq_kernel, pl.lds[4] * 4);
  if (!e) e = tr_set_lds(6, (const void*)tr_attn_bwd_dkv_kernel, pl.lds[4] * 4);
  if (!e) e = tr_set_lds(5, (const void*)tr_qkv_bwd_kernel, pl.lds[5] * 4);
  if (e) return e;
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  float* extra = ws + pl.L * sh.LS + sh.Q;
  a.training = 1;
  a.gout = grad_out;
  a.grad = grad_params;
  a.dh = extra;
  a.dO = a.dh + sh.Q;
  a.dq = a.dO + sh.Q;
  a.dk = a.dq + sh.Q;
  a.dv = a.dk + sh.K;
  a.D = a.dv + sh.K;
  a.ybuf = a.D + sh.S;
  a.cbuf = a.ybuf + B * pl.F;
  a.partial = a.cbuf + B * pl.F;
  e = (int)hipMemsetAsync(a.dh, 0, (size_t)sh.Q * 4, s);
  if (!e) e = (int)hipMemsetAsync(grad_params, 0, (size_t)pl.P * 4, s);
  if (e) return e;
  const unsigned G = (unsigned)sh.G;
  const unsigned rows = (unsigned)((sh.S + TR_WAVES - 1) / TR_WAVES);
  const unsigned krows = (unsigned)((B * pl.KV * T + TR_WAVES - 1) / TR_WAVES);
  a.h_in = ws + pl.L * sh.LS;      // the last block's output
  hipLaunchKernelGGL(tr_final_bwd_kernel, dim3((unsigned)B), dim3(128), 0, s, pl, a);
  hipLaunchKernelGGL(tr_final_wgrad_kernel, dim3((unsigned)((pl.F + pl.E * pl.F + pl.E + TR_THREADS - 1) / TR_THREADS)),
                     dim3(TR_THREADS), 0, s, pl, a);
  for (int l = pl.L - 1; l >= 0; --l) {
    tr_block_buffers(pl, sh, ws, l, 1, &a);
    hipLaunchKernelGGL(tr_tail_bwd_kernel, dim3(G), dim3(TR_THREADS), pl.lds[3] * 4, s, pl, a);
    hipLaunchKernelGGL(tr_attn_bwd_dq_kernel, dim3(rows), dim3(TR_THREADS), pl.lds[4] * 4, s, pl, a);
    hipLaunchKernelGGL(tr_attn_bwd_dkv_kernel, dim3(krows), dim3(TR_THREADS), pl.lds[4] * 4, s, pl, a);
    hipLaunchKernelGGL(tr_qkv_bwd_kernel, dim3(G), dim3(TR_THREADS), pl.lds[5] * 4, s, pl, a);
    hipLaunchKernelGGL(tr_reduce_kernel, dim3((unsigned)((pl.PL + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0,
                       s, (const float*)a.partial, (int)G, pl.PS, 0, (int)pl.PL,
                       grad_params + pl.p_layer0 + l * pl.PL);
    if (l == 0 && pl.scalar)
      hipLaunchKernelGGL(tr_reduce_kernel, dim3((unsigned)((2 * pl.F + TR_THREADS - 1) / TR_THREADS)),
                         dim3(TR_THREADS), 0, s, (const float*)a.partial, (int)G, pl.PS, (int)pl.PL, 2 * pl.F,
                         grad_params + pl.p_spw);
  }
  return (int)hipGetLastError();
}

extern "C" int sbi_amd_tr_dropout_mask(const sbi_amd_tr_config* cfg, int64_t B, int64_t T, float dropout_p,
                                       uint64_t seed, int32_t layer, uint8_t* keep_u8, void* stream) {
  TrPlan pl;
  TrShape sh;
  int rc = tr_build_plan(cfg, B, T, &pl, &sh);
  if (rc) return rc;
  if (!keep_u8 || layer < 0 || layer >= pl.L) return SBI_AMD_E_BADARG;
  if (!(dropout_p >= 0.f && dropout_p < 1.f)) return SBI_AMD_E_UNSUPPORTED;
  const int64_t n = sh.S * T;
  if (n > (((int64_t)1 << 31) - 1)) return SBI_AMD_E_UNSUPPORTED;
  TrArgs a = {};
  a.B = B; a.T = T; a.N = sh.N; a.p = dropout_p; a.layer = layer;
  a.seed_lo = (unsigned)(seed & 0xffffffffu); a.seed_hi = (unsigned)(seed >> 32);
  hipLaunchKernelGGL(tr_mask_kernel, dim3((unsigned)((n + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0,
                     (hipStream_t)stream, pl, a, keep_u8);
  return (int)hipGetLastError();
}
