// nsf_train.hip -- training pass C ABI, gradient reduction, num_bins = 10 instantiations of the
// backward kernel (other bin counts: nsf_train_k5.hip / nsf_train_k8.hip, separate TUs for a parallel build).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include "nsf_train_kernel.h"
#include "debug_env.h"
#include "nsf_coop_host.h"

// grad[p] = sum over workgroups of the partial slabs (fixed association => deterministic);
// finishes LULinear's diagonal: d/d(unconstrained_upper_diag_i) =
//   (dL/dU_ii + (sum_n dL/dlogabsdet_n) / U_ii) * sigmoid(unconstrained_i)
// block = 64 params x 8 slab groups: enough loads in flight to stream the ~100 MB of partials.
#ifndef RED_GROUPS
#define RED_GROUPS 8
#endif
// grid (ceil(PLP / 256), T): one thread sums FOUR consecutive slab words (16-byte loads, 4 x 8-way in flight) over the
// workgroups' slabs; a slab is indexed relative to its transform's parameter block, so the words are 16-byte aligned
__global__ void __launch_bounds__(64 * RED_GROUPS)
nsf_grad_reduce_kernel(const NsfPlan pl, const TrainPlan tp, const float* __restrict__ params,
                       const float* __restrict__ partial, float* __restrict__ grad,
                       const float* __restrict__ logp, float* __restrict__ loss_out, long long n_rows,
                       float* __restrict__ sq_out) {
  // rider (saves a launch per step): the per-row loss of the one-call form, loss = -log p
  if (loss_out)
    for (long long i = ((long long)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x; i < n_rows;
         i += (long long)gridDim.x * gridDim.y * blockDim.x)
      loss_out[i] = -logp[i];
  typedef float f4r __attribute__((ext_vector_type(4)));
  __shared__ f4r red[RED_GROUPS][64];
  __shared__ float red_sgl[RED_GROUPS];
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int t = blockIdx.y;
  const ShapeDesc& S = pl.shape[pl.ctx_mlp ? 0 : (t & 1)];
  const int li = 4 * (blockIdx.x * 64 + lane);
  const bool live = li < S.n_params;
  const float* base = partial + (long long)t * tp.grid * tp.PLP;
  const int ntri = pl.D * (pl.D - 1) / 2;
  const int d0 = S.g_lu + 2 * ntri;
  f4r a = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    f4r acc4[4] = {a, a, a, a};
    int w = grp;
    for (; w + 3 * RED_GROUPS < tp.grid; w += 4 * RED_GROUPS) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc4[u] += *reinterpret_cast<const f4r*>(base + (long long)(w + u * RED_GROUPS) * tp.PLP + li);
    }
    for (; w < tp.grid; w += RED_GROUPS) acc4[0] += *reinterpret_cast<const f4r*>(base + (long long)w * tp.PLP + li);
    a = (acc4[0] + acc4[1]) + (acc4[2] + acc4[3]);
  }
  red[grp][lane] = a;
  {   // sum_n d loss / d logabsdet_n: one word per slab (slot n_params)
    float sgl = 0.f;
    if (!pl.ctx_mlp)
      for (int w2 = grp * 64 + lane; w2 < tp.grid; w2 += 64 * RED_GROUPS) sgl += base[(long long)w2 * tp.PLP + S.n_params];
    for (int off = 32; off > 0; off >>= 1) sgl += __shfl_xor(sgl, off);
    if (lane == 0) red_sgl[grp] = sgl;
  }
  __syncthreads();
  if (grp == 0) {
    float sq = 0.f;     // second rider: this workgroup's share of |grad|^2 (the clip's norm: no separate pass over grad)
    if (live) {
      f4r tot = {0.f, 0.f, 0.f, 0.f};
      float tsg = 0.f;
#pragma unroll
      for (int g = 0; g < RED_GROUPS; ++g) { tot += red[g][lane]; tsg += red_sgl[g]; }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (li + r >= S.n_params) continue;
        const int idx = pl.g_layer[t] + li + r;
        float v = tot[r];
        if (!pl.ctx_mlp && li + r >= d0 && li + r < d0 + pl.D) {
          const float ud = params[idx];
          const float uii = softplus_f(ud) + pl.lu_eps;
          v = (v + tsg / uii) * (1.f / (1.f + expf(-ud)));
        }
        grad[idx] = v;
        sq += v * v;
      }
    }
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off);     // fixed butterfly: deterministic
    if (lane == 0 && sq_out) sq_out[blockIdx.y * gridDim.x + blockIdx.x] = sq;
  }
}

__global__ void neg_copy_kernel(const float* __restrict__ in, float* __restrict__ out, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = -in[i];
}

// ------------------------------------------------------------------ host side
// generic training pass (nsf_gtrain.hip) for the shapes the wave-specialised backward kernel refuses
int64_t nsf_g_workspace_floats(const sbi_amd_nsf_config* cfg, int64_t n);
int nsf_g_train_forward(const sbi_amd_nsf_config* cfg, const float* packed, const float* zstats, const float* theta,
                        const float* x, int64_t n, int64_t x_rows, float* logp_out, float* workspace, void* stream);
int nsf_g_train_backward(const sbi_amd_nsf_config* cfg, const float* params, const float* packed, const float* zstats,
                         const float* x, int64_t n, int64_t x_rows, const float* row_weight, float uniform_weight,
                         float* grad_out, float* grad_theta_out, float* workspace, void* stream);
const float* nsf_g_logp(const sbi_amd_nsf_config* cfg, int64_t n, const float* workspace);
// SBI_AMD_ABLATE bit 2048 (diagnostic): route every shape through the generic pass
static bool fast_path_refuses(int rc) {
  return rc == SBI_AMD_E_UNSUPPORTED || rc == SBI_AMD_E_LDS || (rc == 0 && (sbi_amd_dbg_ablate() & 2048));
}

// The kernel family of an n-row training pass, with the plans it runs on.  Every entry point of the pass (workspace
// size, forward, backward, norm parts) takes its decision here, so the two halves always agree on the workspace layout.
enum { WS_FAM_THROUGHPUT = 0, WS_FAM_COOP = 1, WS_FAM_GENERIC = 2 };
struct TrainRoute {
  int fam;
  NsfPlan pl;         // COOP: the 1-wave plan; THROUGHPUT / GENERIC: the 4-wave plan
  CoopPlan cp;        // COOP
  TrainPlan tp;       // THROUGHPUT
  int refusal;        // GENERIC: why the wave-specialised kernel refused (reported when the generic pass refuses too)
};
static int train_route(const sbi_amd_nsf_config* cfg, int64_t n, TrainRoute* r) {
  if (coop_applies(cfg, n, true, &r->pl, &r->cp)) {
    r->fam = WS_FAM_COOP;
    return 0;
  }
  // (an E_LDS here speaks about the FORWARD kernel's 4-wave layout; the backward kernel has its own budget, checked
  // by build_train_plan, and the training forward picks its workgroup size in nsf_plan_for_rows)
  const int rc = nsf_build_plan(cfg, TR_NW, &r->pl);
  if (rc && rc != SBI_AMD_E_LDS) return rc;
  r->refusal = build_train_plan(r->pl, n, &r->tp);
  if (fast_path_refuses(r->refusal)) {
    r->fam = WS_FAM_GENERIC;
    return 0;
  }
  if (r->refusal) return r->refusal;
  r->fam = WS_FAM_THROUGHPUT;
  return 0;
}

// workgroups of nsf_grad_reduce_kernel = partial sums of squares it leaves behind the activation stash
static inline int64_t thr_sq_parts(const NsfPlan& pl, const TrainPlan& tp) { return (int64_t)((tp.PLP / 4 + 63) / 64) * pl.T; }
// training workspace of the throughput path (float offsets): per-transform input state, z_T, log p, the two dz
// buffers, partial slabs, activation and spline-parameter stashes, the reduction's partial sums of squares of the
// gradient (the clip's norm), the debug timeline
struct ThrWs {
  int64_t stash, noise, logp, gza, gzb, part, ast, pst, sq, dbg, total;
};
static ThrWs thr_ws_layout(const NsfPlan& pl, const TrainPlan& tp, int64_t n) {
  ThrWs w;
  int64_t o = 0;
  w.stash = o; o += (int64_t)pl.T * n * pl.D;
  w.noise = o; o += n * pl.D;
  w.logp = o; o += (n + 3) / 4 * 4;
  w.gza = o; o += n * pl.D;
  w.gzb = o; o += n * pl.D;
  o = (o + 3) / 4 * 4;
  w.part = o; o += (int64_t)pl.T * tp.grid * tp.PLP;
  o = (o + 3) / 4 * 4;
  w.ast = o;   // activation stash: T x ceil(n/16) wave-tiles x slots x 1024 floats
  o += (int64_t)pl.T * ((n + 15) / 16) * nsf_ast_slots(pl) * 1024;
  w.pst = o;   // spline-parameter stash: T x ceil(n/16) wave-tiles x d_tr x PT x 256 floats
  if (TR_PSTASH) o += (int64_t)pl.T * ((n + 15) / 16) * nsf_pst_tile_floats(pl);
  w.sq = o; o += (thr_sq_parts(pl, tp) + 3) / 4 * 4;
  w.dbg = o; o += 2048;   // debug timeline (SBI_AMD_TIMELINE): 1024 int64
  w.total = o;
  return w;
}

extern "C" int64_t sbi_amd_nsf_train_workspace_floats(const sbi_amd_nsf_config* cfg, int64_t n) {
  TrainRoute r;
  const int rc = train_route(cfg, n > 0 ? n : 1, &r);
  if (rc) return rc;
  switch (r.fam) {
    case WS_FAM_COOP: return coop_workspace_floats(r.pl, r.cp, n > 0 ? n : 1);
    case WS_FAM_GENERIC: {
      const int64_t g = nsf_g_workspace_floats(cfg, n);
      return (g >= 0 || g == SBI_AMD_E_LDS) ? g : r.refusal;
    }
  }
  return thr_ws_layout(r.pl, r.tp, n > 0 ? n : 1).total;
}

#define BWD_EXTERN(KK) extern template int launch_bwd_k<KK>(const NsfPlan&, const TrainPlan&, const BwdIo&, hipStream_t);
NSF_FOR_EACH_BINS(BWD_EXTERN)   // (every K lives in nsf_train_k<K>.hip but 10, instantiated here)
template int launch_bwd_k<10>(const NsfPlan&, const TrainPlan&, const BwdIo&, hipStream_t);

// Which kernel family laid out a workspace: the two halves of a training pass take the decision independently from
// (cfg, n) and a process-wide threshold (sbi_amd_nsf_set_coop_max_rows); a backward pass that would read a stash the
// OTHER family wrote (the threshold moved in between) is refused instead of walking a foreign layout.
#include <mutex>
#include <unordered_map>
static std::mutex g_ws_mu;
static std::unordered_map<const void*, std::pair<int, int64_t>> g_ws_family;
static void ws_family_record(const void* ws, int fam, int64_t n) {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  if (g_ws_family.size() > 256) g_ws_family.clear();     // (workspaces are few and long-lived; bound it anyway)
  g_ws_family[ws] = {fam, n};
}
// true: this workspace was last written by a forward pass of a different family / row count
static bool ws_family_mismatch(const void* ws, int fam, int64_t n) {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  auto it = g_ws_family.find(ws);
  return it != g_ws_family.end() && (it->second.first != fam || it->second.second != n);
}

// forward half of the training pass: log p of every row + the per-transform state / activation stash
static int train_forward_impl(const TrainRoute& r, const sbi_amd_nsf_config* cfg, const float* packed,
                              const float* zstats, const float* theta, const float* x, int64_t n, int64_t x_rows,
                              float* logp_out, float* workspace, void* stream, bool fp32_bin) {
  ws_family_record(workspace, r.fam, n);
  if (r.fam == WS_FAM_COOP)
    return coop_train_forward(cfg, r.pl, r.cp, packed + nsf_packed_floats(r.pl), zstats, theta, x, n, x_rows, logp_out,
                              workspace, stream);
  if (r.fam == WS_FAM_GENERIC) {
    const int rg = nsf_g_train_forward(cfg, packed, zstats, theta, x, n, x_rows, logp_out, workspace, stream);
    return fast_path_refuses(rg) ? r.refusal : rg;
  }
  const ThrWs w = thr_ws_layout(r.pl, r.tp, n);
  int rc = dispatch_flow<false>(cfg, packed, zstats, theta, x, n, x_rows, workspace + w.logp, workspace + w.noise,
                                workspace + w.stash, workspace + w.ast, TR_PSTASH ? workspace + w.pst : nullptr, stream,
                                fp32_bin);
  if (rc) return rc;
  if (logp_out) {
    hipError_t e = hipMemcpyAsync(logp_out, workspace + w.logp, sizeof(float) * n, hipMemcpyDeviceToDevice,
                                  (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

extern "C" int sbi_amd_nsf_train_forward(const sbi_amd_nsf_config* cfg, const float* packed, const float* zstats,
                                         const float* theta, const float* x, int64_t n, int64_t x_rows,
                                         float* logp_out, float* workspace, void* stream) {
  if (!cfg || !packed || !zstats || !theta || !x || !workspace || n < 1 || x_rows < 1) return SBI_AMD_E_BADARG;
  TrainRoute r;
  const int rc = train_route(cfg, n, &r);
  return rc ? rc : train_forward_impl(r, cfg, packed, zstats, theta, x, n, x_rows, logp_out, workspace, stream, false);
}

// backward half; loss_out (optional) = -log p of the stash's forward pass, written by the reduction kernel
static int train_backward_impl(const TrainRoute& r, const sbi_amd_nsf_config* cfg, const float* params,
                               const float* packed, const float* zstats, const float* x, int64_t n, int64_t x_rows,
                               const float* row_weight, float uniform_weight, float* grad_out, float* grad_theta_out,
                               float* grad_x_out, float* workspace, float* loss_out, void* stream) {
  if (ws_family_mismatch(workspace, r.fam, n)) return SBI_AMD_E_BADARG;
  if (r.fam == WS_FAM_COOP)   // ONE cooperative backward launch over all transforms, then the fixed-order reduction
    return coop_train_backward(cfg, r.pl, r.cp, params, packed + nsf_packed_floats(r.pl), zstats, x, n, x_rows,
                               row_weight, uniform_weight, grad_out, grad_theta_out, grad_x_out, loss_out, workspace,
                               stream);
  if (r.fam == WS_FAM_GENERIC) {
    if (grad_x_out) return r.refusal;   // d loss / d embedded x comes from the wave-specialised kernel only
    if (loss_out) {
      const float* logp = nsf_g_logp(cfg, n, workspace);
      if (!logp) return r.refusal;
      hipLaunchKernelGGL(neg_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logp,
                         loss_out, (long long)n);
    }
    const int rg = nsf_g_train_backward(cfg, params, packed, zstats, x, n, x_rows, row_weight, uniform_weight,
                                        grad_out, grad_theta_out, workspace, stream);
    return fast_path_refuses(rg) ? r.refusal : rg;
  }
  const NsfPlan& pl = r.pl;
  TrainPlan tp = r.tp;
  tp.grad_x = grad_x_out;
  hipStream_t st = (hipStream_t)stream;
  const ThrWs w = thr_ws_layout(pl, tp, n);
  BwdIo io{};
  io.t_hi = pl.T - 1;
  io.t_lo = 0;
  io.packed = packed;
  io.zstats = zstats;
  io.stash = workspace + w.stash;
  io.x = x;
  io.noise = workspace + w.noise;
  io.gz[0] = workspace + w.gza;
  io.gz[1] = workspace + w.gzb;
  io.row_w = row_weight;
  io.uni_w = uniform_weight;
  io.n = n;
  io.x_rows = x_rows;
  io.partial = workspace + w.part;
  io.grad_theta = grad_theta_out;
  io.astash = workspace + w.ast;
  io.pstash = TR_PSTASH ? workspace + w.pst : nullptr;
  io.dbg = sbi_amd_dbg_timeline() ? (long long*)(workspace + w.dbg) : nullptr;
  const int rc = nsf_with_bins(cfg->K, [&](auto k) { return launch_bwd_k<k>(pl, tp, io, st); });
  if (rc) return rc;
  hipLaunchKernelGGL(nsf_grad_reduce_kernel, dim3((tp.PLP / 4 + 63) / 64, pl.T), dim3(64 * RED_GROUPS), 0, st, pl, tp,
                     params, (const float*)(workspace + w.part), grad_out, (const float*)(workspace + w.logp), loss_out,
                     (long long)n, workspace + w.sq);
  return (int)hipGetLastError();
}

// backward half: consumes the stash the preceding sbi_amd_nsf_train_forward left in `workspace`
// (same cfg, n, x, x_rows, packed image and stream order); grad_out = d( sum_n w_n * (-log p_n) ) / d params
extern "C" int sbi_amd_nsf_train_backward(const sbi_amd_nsf_config* cfg, const float* params, const float* packed,
                                          const float* zstats, const float* x, int64_t n, int64_t x_rows,
                                          const float* row_weight, float uniform_weight, float* grad_out,
                                          float* grad_theta_out, float* grad_x_out, float* workspace, void* stream) {
  if (!cfg || !params || !packed || !zstats || !x || !grad_out || !workspace || n < 1 || x_rows < 1)
    return SBI_AMD_E_BADARG;
  if (grad_x_out && x_rows != n) return SBI_AMD_E_BADARG;   // one context row per theta row (no reduction here)
  TrainRoute r;
  const int rc = train_route(cfg, n, &r);
  return rc ? rc : train_backward_impl(r, cfg, params, packed, zstats, x, n, x_rows, row_weight, uniform_weight,
                                       grad_out, grad_theta_out, grad_x_out, workspace, nullptr, stream);
}

// one-call form: forward + backward with weights known up front (plain NPE loss)
extern "C" int sbi_amd_nsf_loss_fwd_bwd(const sbi_amd_nsf_config* cfg, const float* params, const float* packed,
                                        const float* zstats, const float* theta, const float* x, int64_t n,
                                        int64_t x_rows, const float* row_weight, float uniform_weight,
                                        float* loss_out, float* grad_out, float* grad_theta_out, float* grad_x_out,
                                        float* workspace, void* stream) {
  if (!cfg || !params || !packed || !zstats || !theta || !x || !grad_out || !workspace || n < 1 || x_rows < 1)
    return SBI_AMD_E_BADARG;
  TrainRoute r;
  int rc = train_route(cfg, n, &r);
  if (rc) return rc;
  // (the fused step's forward: its log p is the reported training loss only -- plain fp32 bin, nsf_device.h)
  rc = train_forward_impl(r, cfg, packed, zstats, theta, x, n, x_rows, nullptr, workspace, stream, true);
  if (rc) return rc;
  if (grad_x_out && x_rows != n) return SBI_AMD_E_BADARG;
  return train_backward_impl(r, cfg, params, packed, zstats, x, n, x_rows, row_weight, uniform_weight, grad_out,
                             grad_theta_out, grad_x_out, workspace, loss_out, stream);
}

// Where the gradient reduction of the last training pass of an n-row batch left the partial sums of squares of grad_out
// (their sum = |grad_out|^2, what clip_grad_norm_ needs: sbi_amd_adam_clip_step_parts), and how many there are.
// NULL / 0: that pass does not leave any (the generic training pass), the caller runs sbi_amd_adam_clip_step.
extern "C" const float* sbi_amd_nsf_train_sqnorm_parts(const sbi_amd_nsf_config* cfg, int64_t n, const float* workspace,
                                                       int64_t* n_parts) {
  if (n_parts) *n_parts = 0;
  if (!cfg || !workspace || n < 1) return nullptr;
  TrainRoute r;
  if (train_route(cfg, n, &r)) return nullptr;
  if (r.fam == WS_FAM_COOP) return coop_sqnorm_parts(r.pl, r.cp, n, workspace, n_parts);
  if (r.fam == WS_FAM_GENERIC) return nullptr;
  if (n_parts) *n_parts = thr_sq_parts(r.pl, r.tp);
  return workspace + thr_ws_layout(r.pl, r.tp, n).sq;
}
