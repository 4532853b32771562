// philox.h -- the counter-based generator of the device-side samplers (slice sampler: mcmc_tick.h; SDE sampler:
// fmpe_kernel.h).
#pragma once
#include <hip/hip_runtime.h>

// Philox4x32-10 (Salmon et al., SC'11): counter = (tick, tick >> 32, chain, block), key = the run's seed.  The
// reference's slice sampler draws from NumPy's global generator (slice_numpy.py:353-587) -- there is no stream to
// reproduce, only a distribution; the seed comes from torch's generator, so `torch.manual_seed` fixes a run.
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ float u01(unsigned r) { return (float)(r >> 8) * (1.0f / 16777216.0f); }   // [0, 1), as torch.rand
