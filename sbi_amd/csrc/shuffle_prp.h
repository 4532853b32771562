// shuffle_prp.h -- the keyed pseudo-random permutation of [0, n) behind the device-side minibatch orders: shuffle.hip's
// gather (the NPE inner loop) and lc2st_kernel.h's per-member epoch orders evaluate the same function, so one Python
// restatement (tests/shuffle_restatement.py) pins both.  A 6-round balanced Feistel network on the smallest even-width
// binary domain >= n with cycle walking (Black & Rogaway 2002); see shuffle.hip for the why.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__host__ __device__ __forceinline__ uint32_t shf_mix(uint32_t v) {     // murmur3's 32-bit finaliser
  v ^= v >> 16; v *= 0x85ebca6bu; v ^= v >> 13; v *= 0xc2b2ae35u; v ^= v >> 16;
  return v;
}
// position i of the order -> element pi(i) of [0, n); hb = bits per Feistel half (2 hb >= ceil(log2 n))
__host__ __device__ __forceinline__ uint32_t shf_prp(uint32_t i, uint32_t n, int hb, uint64_t key) {
  const uint32_t mask = (1u << hb) - 1u;
  const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  uint32_t v = i;
  do {
    uint32_t l = v >> hb, r = v & mask;
#pragma unroll
    for (int round = 0; round < 6; ++round) {
      const uint32_t f = shf_mix(r + 0x9e3779b9u * (uint32_t)(round + 1) + ((round & 1) ? k1 : k0)) & mask;
      const uint32_t t = l ^ f;
      l = r;
      r = t;
    }
    v = (l << hb) | r;
  } while (v >= n);
  return v;
}

// bits per Feistel half for a permutation of [0, n)
__host__ __device__ __forceinline__ int shf_half_bits(long long n) {
  int bits = 2;
  while (bits < 32 && (1ll << bits) < n) ++bits;
  return (bits + 1) / 2;
}
