// resnet_embed.hip -- C ABI of the ResNetEmbedding1D trunk (include/sbi_amd_resnet.h); kernels in resnet_embed_kernel.h.
#include <mutex>
#include "resnet_embed_kernel.h"

// The dynamic-LDS limit sticks to (device, kernel): raise it once per device and kernel.
#define RN_CACHED_DEVICES 64
static int rn_set_lds(int which, const void* kern, int lds_bytes) {
  static std::mutex lock;
  static int have[RN_CACHED_DEVICES][6];
  if (lds_bytes <= 48 * 1024) return 0;
  int dev = -1;
  const bool cached = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < RN_CACHED_DEVICES;
  std::lock_guard<std::mutex> guard(lock);
  if (cached && have[dev][which] >= lds_bytes) return 0;
  const int e = (int)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (!e && cached) have[dev][which] = lds_bytes;
  return e;
}

extern "C" int64_t sbi_amd_resnet_param_count(const sbi_amd_resnet_config* cfg, int64_t* offsets) {
  RnPlan pl;
  const int rc = rn_plan_sizes(cfg, &pl);
  if (rc) return rc;
  if (offsets) {
    int64_t o = 0;
    int e = 0;
    if (pl.has_init) {
      offsets[e++] = o, o += (int64_t)pl.ci * pl.cin;
      offsets[e++] = o, o += pl.ci;
    }
    for (int b = 0; b < pl.nb; ++b) {
      offsets[e++] = o, o += (int64_t)pl.ch * pl.ci;
      offsets[e++] = o, o += pl.ch;
      offsets[e++] = o, o += (int64_t)pl.ch * pl.ch;
      offsets[e++] = o, o += pl.ch;
      offsets[e++] = o, o += (int64_t)pl.ci * pl.ch;
      offsets[e++] = o, o += pl.ci;
    }
  }
  return pl.P;
}

extern "C" int sbi_amd_resnet_plan(const sbi_amd_resnet_config* cfg, int64_t rows, int32_t* row_tile,
                                   int32_t* lds_bytes, int32_t* splits) {
  RnPlan pl;
  RnShape sh;
  int rc = rn_plan_sizes(cfg, &pl);
  if (rc) return rc;
  rc = rn_plan_shape(pl, rows, &sh);
  if (rc) return rc;
  if (row_tile) *row_tile = sh.RT;
  if (lds_bytes) lds_bytes[0] = sh.lds_fwd, lds_bytes[1] = sh.lds_bwd;
  if (splits) *splits = sh.S;
  return 0;
}

extern "C" int64_t sbi_amd_resnet_workspace_bytes(const sbi_amd_resnet_config* cfg, int64_t rows, int32_t training) {
  RnPlan pl;
  RnShape sh;
  int rc = rn_plan_sizes(cfg, &pl);
  if (rc) return rc;
  rc = rn_plan_shape(pl, rows, &sh);
  if (rc) return rc;
  return sh.ws_floats[training ? 1 : 0] * 4;
}

static unsigned rn_grid(int64_t rows, int RT) {
  const int64_t tiles = (rows + RT - 1) / RT;
  return (unsigned)(tiles < RN_GRID ? tiles : RN_GRID);
}

template <int RT, int KP>
static int rn_launch_forward(int which, const RnPlan& pl, const RnShape& sh, const RnFwdArgs& a, hipStream_t s) {
  const int e = rn_set_lds(which, (const void*)rn_forward_kernel<RT, KP>, sh.lds_fwd);
  if (e) return e;
  hipLaunchKernelGGL((rn_forward_kernel<RT, KP>), dim3(rn_grid(a.trows, RT)), dim3(RN_THREADS), sh.lds_fwd, s, pl, a);
  return 0;
}

template <int RT, int KP>
static int rn_launch_delta(int which, const RnPlan& pl, const RnShape& sh, const RnBwdArgs& a, hipStream_t s) {
  const int e = rn_set_lds(which, (const void*)rn_delta_kernel<RT, KP>, sh.lds_bwd);
  if (e) return e;
  hipLaunchKernelGGL((rn_delta_kernel<RT, KP>), dim3(rn_grid(a.rows, RT)), dim3(RN_THREADS), sh.lds_bwd, s, pl, a);
  return 0;
}

extern "C" int sbi_amd_resnet_forward(const sbi_amd_resnet_config* cfg, const float* params, const float* x,
                                      int64_t rows, float* out, void* workspace, int32_t training, void* stream) {
  RnPlan pl;
  RnShape sh;
  int rc = rn_plan_sizes(cfg, &pl);
  if (rc) return rc;
  rc = rn_plan_shape(pl, rows, &sh);
  if (rc) return rc;
  if (!params || !x || !out || !workspace) return SBI_AMD_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  hipLaunchKernelGGL(rn_pack_kernel, dim3((unsigned)((pl.IMG + RN_THREADS - 1) / RN_THREADS)), dim3(RN_THREADS), 0, s,
                     pl, params, ws);
  RnFwdArgs a;
  a.img = ws, a.x = x, a.out = out;
  a.stash = training ? ws + sh.o_stash : nullptr;
  a.rows = rows, a.Rp = sh.Rp, a.trows = training ? sh.Rp : rows;
  if (sh.RT == 16) rc = rn_launch_forward<16, 64>(0, pl, sh, a, s);
  else if (sh.RT == 32) rc = rn_launch_forward<32, 64>(1, pl, sh, a, s);
  else rc = rn_launch_forward<64, 32>(2, pl, sh, a, s);
  if (rc) return rc;
  return (int)hipGetLastError();
}

extern "C" int sbi_amd_resnet_backward(const sbi_amd_resnet_config* cfg, const float* params, const float* x,
                                       int64_t rows, const float* grad_out, float* grad_params, void* workspace,
                                       void* stream) {
  RnPlan pl;
  RnShape sh;
  int rc = rn_plan_sizes(cfg, &pl);
  if (rc) return rc;
  rc = rn_plan_shape(pl, rows, &sh);
  if (rc) return rc;
  if (!params || !x || !grad_out || !grad_params || !workspace) return SBI_AMD_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int64_t slab = sh.Rp * pl.CI;
  float* stash = ws + sh.o_stash;
  float* delta = ws + sh.o_delta;
  const bool split = sh.S > 1;
  const int ci = pl.ci, ch = pl.ch;
  const int strips = (pl.CI > pl.CH ? pl.CI : pl.CH) / 16;

  for (int b = pl.nb - 1; b >= 0; --b) {
    RnBwdArgs a;
    a.img = ws;
    a.xin = stash + b * slab, a.xout = stash + (b + 1) * slab;
    const bool last = b == pl.nb - 1;
    a.dsrc = last ? grad_out : delta;
    a.dstride = last ? ci : pl.CI, a.drows = last ? rows : sh.Rp, a.dcols = last ? ci : pl.CI;
    a.dout = delta;
    a.dz = ws + sh.o_dz, a.ha = ws + sh.o_a, a.hc = ws + sh.o_c, a.da = ws + sh.o_da, a.dc = ws + sh.o_dc;
    a.rows = sh.Rp, a.block = b;
    if (sh.RT == 16) rc = rn_launch_delta<16, 64>(3, pl, sh, a, s);
    else if (sh.RT == 32) rc = rn_launch_delta<32, 64>(4, pl, sh, a, s);
    else rc = rn_launch_delta<64, 32>(5, pl, sh, a, s);
    if (rc) return rc;

    RnWgArgs w;
    const int64_t o_w0 = 0, o_b0 = (int64_t)ch * ci, o_w2 = o_b0 + ch, o_b2 = o_w2 + (int64_t)ch * ch, o_w4 = o_b2 + ch,
                  o_b4 = o_w4 + (int64_t)ci * ch;
    w.m[0] = RnWgMat{a.da, a.xin, pl.CI, sh.Rp, ch, pl.CH, ci, o_w0, o_b0};
    w.m[1] = RnWgMat{a.dc, a.ha, pl.CH, sh.Rp, ch, pl.CH, ch, o_w2, o_b2};
    w.m[2] = RnWgMat{a.dz, a.hc, pl.CH, sh.Rp, ci, pl.CI, ch, o_w4, o_b4};
    float* gblock = grad_params + pl.PI + b * pl.PB;
    w.out = split ? ws + sh.o_part : gblock;
    w.out_stride = split ? sh.PS : 0;
    w.Rp = sh.Rp, w.chunk = sh.chunk;
    hipLaunchKernelGGL(rn_wgrad_kernel, dim3(strips, sh.S, 3), dim3(RN_THREADS), 0, s, w);
    if (split)
      hipLaunchKernelGGL(rn_reduce_kernel, dim3((unsigned)((pl.PB + RN_THREADS - 1) / RN_THREADS)), dim3(RN_THREADS), 0,
                         s, (const float*)(ws + sh.o_part), sh.S, sh.PS, pl.PB, gblock);
  }
  if (pl.has_init) {
    RnWgArgs w;
    w.m[0] = RnWgMat{delta, x, pl.cin, rows, ci, pl.CI, pl.cin, 0, (int64_t)ci * pl.cin};
    w.m[1] = w.m[2] = w.m[0];
    w.out = split ? ws + sh.o_part : grad_params;
    w.out_stride = split ? sh.PS : 0;
    w.Rp = sh.Rp, w.chunk = sh.chunk;
    hipLaunchKernelGGL(rn_wgrad_kernel, dim3(pl.CI / 16, sh.S, 1), dim3(RN_THREADS), 0, s, w);
    if (split)
      hipLaunchKernelGGL(rn_reduce_kernel, dim3((unsigned)((pl.PI + RN_THREADS - 1) / RN_THREADS)), dim3(RN_THREADS), 0,
                         s, (const float*)(ws + sh.o_part), sh.S, sh.PS, pl.PI, grad_params);
  }
  return (int)hipGetLastError();
}
