// npse_iid_kernel.h -- compositional score of N iid observations around the vector-field trunk of fmpe_kernel.h
// (included by npse.hip after it): the one-step composed score and the Euler-Maruyama sampler on it, one launch each.
//
// Reference behaviour: IIDScoreFunction.__call__ of sbi/inference/potentials/vector_field_adaptor.py:725-1031 (fnpe,
// gauss, auto_gauss) under a Gaussian prior, where everything but the per-observation scores s_i = score(theta, t | x_i)
// is theta-independent.  The host turns that part into per-step tables in fp64 and the kernel evaluates
//     score_k(theta) = Linv_k (C_k sum_i s_i + sum_i Lam_i s_i) + A_k theta + b_k.
//
// Execution model (D <= 16: theta, u = sum s_i, v = sum Lam_i s_i and every table matrix are ONE 16x16 MFMA tile)
//   * a wave owns 16 rows (draws) for all steps, as in MODE 6 of fm_fwd_kernel; a lane keeps theta, u and v of its row
//     in the B / D fragment layout (lane (c, g): features 4g..4g+3 of row c), so the four table mat-vecs are
//     4 MFMAs each with the matrix as the A operand (lane (c, g): M[c][4g..4g+3], read from L2 once per step).
//   * per step the input layer, its half of the merge (hA = W_ma gelu(ie) + b_ma) and the time embedding run once;
//     the observation loop i = 0..N-1 repeats only  gelu(hA + e_i) -> L residual blocks -> output layer.
//     e_i = W_mb gelu(W_ct xhat_i + b_ct) depends on neither step nor row: fm_iid_cond_kernel writes it once per call
//     into the workspace ([N][128] floats) and the lanes read their features back (L2 hits, the same address for the
//     16 lanes of a g).
//   * the time embedding is the same for all rows: each wave keeps its copy in LDS (128 floats behind the z-score
//     tail) instead of in registers.
//   * the sums over observations run in the fixed order i = 0..N-1 in registers: no atomics, and a row's result
//     depends on neither n nor its tile.
//   * weight staging: the same two LDS buffers and group images as FmPipe, but the order of the groups is no longer a
//     plain cycle: NpIidPipe follows the VISIT list  IN MA TM (L0 .. L(L-1) OUT) x N  and, on entering a group, stages
//     the next group of that list which differs from the resident one -- inside the observation loop that is the
//     first residual group again, so the input-side groups are not replayed.
#ifndef SBI_AMD_NPSE_IID_KERNEL_H
#define SBI_AMD_NPSE_IID_KERNEL_H

namespace {

#define NP_IID_MAX_D 16
#define NP_IID_MAX_N 1024
#define NP_IID_EC 128          // floats per observation in the condition workspace (16 * HB <= 128)
#define NP_IID_PRO 3           // visits before the observation loop: IN MA TM

struct NpIidArgs {
  const float* xs;             // [N][C] observations
  int N;
  const float* lam;            // [N][D][D] or nullptr (all zero)
  const float* mats;           // [steps][3][D][D]: Linv, C, A of step k at index k - 1
  const float* vecs;           // [steps][D]: b
  const float* econd;          // [N][NP_IID_EC]: e_i
  int nvis;                    // visits per step and observation list: NP_IID_PRO + L + 1
  int vis_grp[FM_MAX_LIN];     // staging group of visit v (IN MA TM L0 .. OUT)
};

// e_i = W_mb gelu(W_ct xhat_i + b_ct): one block per observation, one thread per hidden feature, weights from the
// packed forward images (zero padded, so features >= H come out as 0)
__global__ void __launch_bounds__(128) fm_iid_cond_kernel(const FmPlan pl, const float* __restrict__ packed,
                                                          const float* __restrict__ zstats,
                                                          const float* __restrict__ xs, float* __restrict__ econd) {
  __shared__ float xh[128], hh[128];
  const int i = blockIdx.x, o = threadIdx.x, D = pl.D, C = pl.C;
  xh[o] = o < C ? (xs[(long long)i * C + o] - zstats[2 * D + o]) * (1.0f / zstats[2 * D + C + o]) : 0.f;
  __syncthreads();
  {
    const FmLin& q = pl.lin[J_CT];
    const int rows = 16 * q.OB;
    float ce = 0.f;
    if (o < rows) {
      ce = packed[q.w_off + rows * q.ldk + o];
      for (int j = 0; j < C; ++j) ce = fmaf(packed[q.w_off + o * q.ldk + j], xh[j], ce);
    }
    hh[o] = o < rows ? gelu_f(ce) : 0.f;
  }
  __syncthreads();
  {
    const FmLin& q = pl.lin[J_MB];
    const int rows = 16 * q.OB, cols = 16 * q.KB;
    float e = 0.f;
    if (o < rows)
      for (int j = 0; j < cols; ++j) e = fmaf(packed[q.w_off + o * q.ldk + j], hh[j], e);
    econd[(long long)i * NP_IID_EC + o] = e;
  }
}

struct NpIidPipe {
  float* lds;
  const float* packed;
  const int* goff;
  const int* gfloats;
  const int* vgrp;
  int buf_floats, nvis, N, cur, par, wave, lane;
  // the group of the first visit after (v, i) that is not g, or -1 (one group holds everything)
  __device__ __forceinline__ int next_group(int v, int i, int g) const {
    for (int w = v + 1; w < nvis; ++w)
      if (vgrp[w] != g) return vgrp[w];
    if (i + 1 < N)                         // further observations repeat the same list: one pass decides
      for (int w = NP_IID_PRO; w < nvis; ++w)
        if (vgrp[w] != g) return vgrp[w];
    for (int w = 0; w < nvis; ++w)         // the next step (or tile) starts over
      if (vgrp[w] != g) return vgrp[w];
    return -1;
  }
  __device__ __forceinline__ void stage_next(int v, int i) {
    const int nx = next_group(v, i, cur);
    if (nx >= 0) fm_stage_async(lds + (par ^ 1) * buf_floats, packed + goff[nx], gfloats[nx], wave, lane);
  }
  __device__ __forceinline__ void init(float* lds_, const float* packed_, const int* goff_, const int* gfloats_,
                                       const int* vgrp_, int nvis_, int N_, int buf_floats_, int wave_, int lane_) {
    lds = lds_; packed = packed_; goff = goff_; gfloats = gfloats_; vgrp = vgrp_; nvis = nvis_; N = N_;
    buf_floats = buf_floats_; wave = wave_; lane = lane_; par = 0; cur = vgrp[0];
    fm_stage_async(lds, packed + goff[cur], gfloats[cur], wave, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    stage_next(0, 0);
  }
  // before the linear of visit v of observation i: if its group is not the resident one it is the one in flight
  __device__ __forceinline__ const float* visit(int v, int i) {
    const int g = vgrp[v];
    if (g != cur) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // it has landed ...
      __syncthreads();                                   // ... for every wave, and all are done with the other buffer
      par ^= 1;
      cur = g;
      stage_next(v, i);
    }
    return lds + par * buf_floats;
  }
  __device__ __forceinline__ void drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
};

__device__ __forceinline__ float np_uniform(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
__device__ __forceinline__ f4 np_mv16(f4 m, f4 x, f4 acc) {   // acc += M x for one row per column (M as A operand)
#pragma unroll
  for (int r = 0; r < 4; ++r) acc = MFMA16(m[r], x[r], acc);
  return acc;
}

// SAMPLE false: out[n][D] = composed score at a.theta, a.times[0], tables of one step
// SAMPLE true:  the Euler-Maruyama sampler of MODE 6 with score replaced by the composed score of step k
template <int HB, bool SAMPLE>
__global__ void __launch_bounds__(FM_THREADS, 1) fm_iid_kernel(const FmPlan pl, const FmArgs a, const NpIidArgs q) {
  extern __shared__ __align__(16) float lds[];
  float* zs = lds + 2 * pl.lds_fwd_floats;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int D = pl.D, H = pl.H, L = pl.L, N = q.N;
  float* z_mean = zs; float* z_std = zs + 128;
  float* tm = zs + FM_ZS_FLOATS + wave * 128;   // this wave's time embedding (the same for all of its rows)
  for (int i = tid; i < 128; i += FM_THREADS) {
    z_mean[i] = i < D ? a.zstats[i] : 0.f;
    z_std[i] = i < D ? a.zstats[D + i] : 1.f;
  }
  const float invH = 1.0f / (float)H;
  const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
  NpIidPipe pipe;
  pipe.init(lds, a.packed, pl.fgrp_off, pl.fgrp_floats, q.vis_grp, q.nvis, N, pl.lds_fwd_floats, wave, lane);
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const long long row_raw = ((long long)tile * FM_WAVES + wave) * 16 + c;
    const bool valid = row_raw < a.n;
    const long long row = valid ? row_raw : a.n - 1;
    f4 th = zero4;                       // theta of this lane's features 4g..4g+3
    if constexpr (SAMPLE) {              // theta ~ N(mean_base, std_base): draw 0
      const f4 z = fm_sde_draw4(a, D, row, 0, 0, g);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int f = 4 * g + j;
        if (f < D) th[j] = a.base[f] + a.base[D + f] * z[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int f = 4 * g + j;
        if (f < D) th[j] = a.theta[row * D + f];
      }
    }
    const int nsteps = SAMPLE ? a.steps : 1;
    for (int k = 1; k <= nsteps; ++k) {
      const float t = a.times[SAMPLE ? k - 1 : 0];
      FmSde sq = fm_sde_at(pl, t);         // wave-uniform: kept in scalar registers across the observation loop
      sq.m = np_uniform(sq.m); sq.s = np_uniform(sq.s); sq.beta = np_uniform(sq.beta); sq.g2 = np_uniform(sq.g2);
      f4 acc[HB], h[HB], hA[HB];
      // ---- input layer: theta_t -> time-dependent z-score -> Linear(D, H)
      const float* wb = pipe.visit(0, 0);
      {
        f4 zin;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int f = 4 * g + j;
          const float sd = sq.m * z_std[f < D ? f : 0];
          zin[j] = f < D ? (th[j] - sq.m * z_mean[f]) / sqrtf(sd * sd + sq.s * sq.s) : 0.f;
        }
        const FmLin& ql = pl.lin[J_IN];
#pragma unroll
        for (int ob = 0; ob < HB; ++ob) acc[ob] = *reinterpret_cast<const f4*>(wb + ql.lb + 16 * ob + 4 * g);
        gemm_blk<HB>(wb + ql.lw + c * ql.ldk + 4 * g, ql.ldk, 0, zin, acc);
#pragma unroll
        for (int ob = 0; ob < HB; ++ob) h[ob] = gelu4(acc[ob]);
      }
      // ---- theta half of the merge (with the merge bias)
      wb = pipe.visit(1, 0);
      {
        const FmLin& ql = pl.lin[J_MA];
#pragma unroll
        for (int ob = 0; ob < HB; ++ob) hA[ob] = *reinterpret_cast<const f4*>(wb + ql.lb + 16 * ob + 4 * g);
        gemm_rr<HB, HB>(wb + ql.lw + c * ql.ldk + 4 * g, ql.ldk, h, hA);
      }
      // ---- time embedding
      wb = pipe.visit(2, 0);
      {
        const FmLin& ql = pl.lin[J_TM];
#pragma unroll
        for (int ob = 0; ob < HB; ++ob) acc[ob] = *reinterpret_cast<const f4*>(wb + ql.lb + 16 * ob + 4 * g);
        const float* wl = wb + ql.lw + c * ql.ldk + 4 * g;
        for (int kb = 0; kb < pl.EB; ++kb) {
          f4 v;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int e = 16 * kb + 4 * g + j;
            float val = 0.f;
            if (e < pl.E) {
              const float w = expf(-(float)(e & ~1) * pl.log_max_freq_over_E);
              const float ang = sq.s * w;
              val = (e & 1) ? cosf(ang) : sinf(ang);
            }
            v[j] = val;
          }
          gemm_blk<HB>(wl, ql.ldk, kb, v, acc);
        }
        if (c == 0) {
#pragma unroll
          for (int ob = 0; ob < HB; ++ob) *reinterpret_cast<f4*>(tm + 16 * ob + 4 * g) = acc[ob];
        }
      }
      // ---- observations, in order: u = sum s_i, v = sum Lam_i s_i
      const float ms = np_uniform(sq.m / sq.s);
      f4 u = zero4, v = zero4;
      for (int i = 0; i < N; ++i) {
        const float* ec = q.econd + (long long)i * NP_IID_EC + 4 * g;
#pragma unroll
        for (int ob = 0; ob < HB; ++ob) acc[ob] = *reinterpret_cast<const f4*>(ec + 16 * ob);
#pragma unroll
        for (int ob = 0; ob < HB; ++ob) h[ob] = gelu4(acc[ob] + hA[ob]);
        // residual blocks: h <- LayerNorm(GELU(W h + b) + temb + h)
        for (int l = 0; l < L; ++l) {
          wb = pipe.visit(NP_IID_PRO + l, i);
          const FmLin& ql = pl.lin[J_L0 + l];
#pragma unroll
          for (int ob = 0; ob < HB; ++ob) acc[ob] = *reinterpret_cast<const f4*>(wb + ql.lb + 16 * ob + 4 * g);
          gemm_rr<HB, HB>(wb + ql.lw + c * ql.ldk + 4 * g, ql.ldk, h, acc);
          float s1 = 0.f;
#pragma unroll
          for (int ob = 0; ob < HB; ++ob) {
            acc[ob] = gelu4(acc[ob]) + *reinterpret_cast<const f4*>(tm + 16 * ob + 4 * g) + h[ob];
            s1 += (acc[ob][0] + acc[ob][1]) + (acc[ob][2] + acc[ob][3]);
          }
          const float mean = sum_over_g(s1) * invH;
          float s2 = 0.f;
#pragma unroll
          for (int ob = 0; ob < HB; ++ob) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float d = (16 * ob + 4 * g + j) < H ? acc[ob][j] - mean : 0.f;
              acc[ob][j] = d;
              s2 += d * d;
            }
          }
          const float rstd = 1.0f / sqrtf(sum_over_g(s2) * invH + pl.ln_eps);
#pragma unroll
          for (int ob = 0; ob < HB; ++ob) {
            const f4 gam = *reinterpret_cast<const f4*>(wb + ql.lb + 16 * HB + 16 * ob + 4 * g);
            const f4 bet = *reinterpret_cast<const f4*>(wb + ql.lb + 32 * HB + 16 * ob + 4 * g);
            h[ob] = acc[ob] * rstd * gam + bet;
          }
        }
        // output layer (one 16-feature block) -> s_i
        f4 lamc = zero4;                 // Lam_i: row c, columns 4g..4g+3 (lands under the output GEMM)
        if (q.lam && c < D) {
          const float* lp = q.lam + ((long long)i * D + c) * D;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (4 * g + j < D) lamc[j] = lp[4 * g + j];
        }
        wb = pipe.visit(NP_IID_PRO + L, i);
        {
          const FmLin& ql = pl.lin[J_L0 + L];
          const float* wl = wb + ql.lw + c * ql.ldk + 4 * g;
          f4 o0 = *reinterpret_cast<const f4*>(wb + ql.lb + 4 * g), o1 = zero4;
#pragma unroll
          for (int kb = 0; kb < HB; ++kb) {
            const f4 av = *reinterpret_cast<const f4*>(wl + 16 * kb);
            if (kb & 1) {
#pragma unroll
              for (int r = 0; r < 4; ++r) o1 = MFMA16(av[r], h[kb][r], o1);
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r) o0 = MFMA16(av[r], h[kb][r], o0);
            }
          }
          o0 += o1;
          f4 si;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int f = 4 * g + j;
            const float sd = sq.m * z_std[f < D ? f : 0];
            si[j] = f < D ? -ms * o0[j] - (th[j] - sq.m * z_mean[f]) / (sd * sd + sq.s * sq.s) : 0.f;
          }
          u += si;
          if (q.lam) v = np_mv16(lamc, si, v);
        }
      }
      // ---- composition: Linv (C u + v) + A theta + b
      // tables of this step: A-operand fragments (row c, columns 4g..4g+3) and b of this lane's features
      const float* mk = q.mats + (long long)(k - 1) * 3 * D * D;
      const float* vk = q.vecs + (long long)(k - 1) * D;
      f4 mL = zero4, mC = zero4, mA = zero4, bv = zero4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int f = 4 * g + j;
        if (f < D) {
          bv[j] = vk[f];
          if (c < D) {
            mL[j] = mk[c * D + f];
            mC[j] = mk[D * D + c * D + f];
            mA[j] = mk[2 * D * D + c * D + f];
          }
        }
      }
      const f4 w = np_mv16(mC, u, v);
      f4 sc = np_mv16(mA, th, bv);
      sc = np_mv16(mL, w, sc);
      if constexpr (SAMPLE) {   // theta <- theta - (f - (1 + eta^2)/2 g^2 score) dt + eta g sqrt(dt) z_k
        const float dt = t - a.times[k];
        const float c1 = 0.5f * (1.0f + a.eta * a.eta) * sq.g2, gn = a.eta * sqrtf(sq.g2 * dt);
        const f4 z = fm_sde_draw4(a, D, row, k, 0, g);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (4 * g + j < D) th[j] = th[j] - (-0.5f * sq.beta * th[j] - c1 * sc[j]) * dt + gn * z[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (4 * g + j < D && valid) a.v_out[row * D + 4 * g + j] = sc[j];
      }
    }
    if constexpr (SAMPLE) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * g + j < D && valid) a.v_out[row * D + 4 * g + j] = th[j];
    }
  }
  pipe.drain();
}

// out[n][D] = the standard-normal draws z_k of the samplers (fm_sde_draw4: Philox keyed by seed, row + row_offset, k,
// 4-dim block), for the host-loop leg: one thread per row and block of four dims
__global__ void __launch_bounds__(256) np_normals_kernel(const FmArgs a, int D, int k, float* __restrict__ out) {
  const int nb = (D + 3) / 4;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.n * nb) return;
  const long long row = idx / nb;
  const int b = (int)(idx - row * nb);
  const f4 z = fm_sde_draw4(a, D, row, k, b >> 2, b & 3);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (4 * b + j < D) out[row * D + 4 * b + j] = z[j];
}

// The composition for the host-loop leg, any D <= 128 and any N: out[row] = Linv (C sum_i s_i + sum_i Lam_i s_i) + A theta + b
// from s [n][N][D].  One block per row, thread d owns output feature d; every sum runs sequentially in index order (i, then
// e), so a row's bits depend on nothing but that row -- unlike a BLAS product, whose kernel is chosen by the batch shape.
__global__ void __launch_bounds__(128) np_compose_kernel(const float* __restrict__ s, const float* __restrict__ theta,
                                                         const float* __restrict__ lam, const float* __restrict__ mats,
                                                         const float* __restrict__ vec, int N, int D,
                                                         float* __restrict__ out) {
  __shared__ float u[128], w[128], th[128];
  const long long row = blockIdx.x;
  const int d = threadIdx.x;
  const float* sr = s + row * N * D;
  float acc = 0.f;
  if (d < D) {
    for (int i = 0; i < N; ++i) acc += sr[i * D + d];
    th[d] = theta[row * D + d];
  }
  u[d] = acc;
  __syncthreads();
  acc = 0.f;
  if (d < D) {
    const float* C = mats + D * D + d * D;
    for (int e = 0; e < D; ++e) acc = fmaf(C[e], u[e], acc);
    if (lam)
      for (int i = 0; i < N; ++i) {
        const float* L = lam + ((long long)i * D + d) * D;
        for (int e = 0; e < D; ++e) acc = fmaf(L[e], sr[i * D + e], acc);
      }
  }
  w[d] = acc;
  __syncthreads();
  if (d < D) {
    const float* Li = mats + d * D;
    const float* A = mats + 2 * D * D + d * D;
    acc = vec[d];
    for (int e = 0; e < D; ++e) acc = fmaf(A[e], th[e], acc);
    for (int e = 0; e < D; ++e) acc = fmaf(Li[e], w[e], acc);
    out[row * D + d] = acc;
  }
}

template <bool SAMPLE>
static int np_iid_launch(const FmPlan& pl, const FmArgs& a, NpIidArgs q, float* econd, hipStream_t st) {
  // staging group of every linear, in the forward image order IN MA CT MB TM L0 .. OUT
  int grp[FM_MAX_LIN], order[FM_MAX_LIN], gi = -1;
  for (int j = 0; j < pl.NL; ++j) order[j] = j;
  order[0] = J_IN; order[1] = J_MA; order[2] = J_CT; order[3] = J_MB; order[4] = J_TM;
  for (int k = 0; k < pl.NL; ++k) {
    if (pl.lin[order[k]].fg_first) ++gi;
    grp[order[k]] = gi;
  }
  q.nvis = NP_IID_PRO + pl.L + 1;
  q.vis_grp[0] = grp[J_IN]; q.vis_grp[1] = grp[J_MA]; q.vis_grp[2] = grp[J_TM];
  for (int l = 0; l <= pl.L; ++l) q.vis_grp[NP_IID_PRO + l] = grp[J_L0 + l];
  q.econd = econd;
  hipLaunchKernelGGL(fm_iid_cond_kernel, dim3(q.N), dim3(128), 0, st, pl, a.packed, a.zstats, q.xs, econd);
  const size_t lds = 4ull * (2 * pl.lds_fwd_floats + FM_ZS_FLOATS + FM_WAVES * 128);
  const int grid = fm_grid(a.ntiles);
#define NP_IID_CASE(HBV)                                                                                        \
  case HBV: {                                                                                                   \
    hipError_t e = hipFuncSetAttribute((const void*)fm_iid_kernel<HBV, SAMPLE>,                                 \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                   \
    if (e != hipSuccess) return (int)e;                                                                         \
    hipLaunchKernelGGL((fm_iid_kernel<HBV, SAMPLE>), dim3(grid), dim3(FM_THREADS), lds, st, pl, a, q);          \
    break;                                                                                                      \
  }
  switch (pl.HB) {
    NP_IID_CASE(4)
    NP_IID_CASE(7)
    NP_IID_CASE(8)
    default: return SBI_AMD_E_UNSUPPORTED;
  }
#undef NP_IID_CASE
  return (int)hipGetLastError();
}

}  // namespace
#endif
