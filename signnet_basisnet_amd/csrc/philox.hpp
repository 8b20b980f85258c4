// philox.hpp — Philox4x32-10 (Salmon et al., SC'11; the Random123 constants) and the attention-dropout mask built on it: what
// dropout.hip and the four attention kernels (attention16.hip, ops.hip, backward.hip) share.
#pragma once
#include "common.hpp"

namespace sn {

struct philox_out { uint32_t w[4]; };

__device__ __forceinline__ philox_out philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  philox_out o;
  o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
  return o;
}

// The counter source of the attention-dropout mask (signnet_hip.h, sn_set_attention_drop_f32): passed by value to all four attention
// kernels; the explicit-mask / no-mask instantiations never read it.
struct AttnDrop {
  uint32_t threshold;      // floor(p * 2^32)
  float scale;             // float32(1 / (1 - p))
  const int64_t* state;    // {seed, step}: device words, read when the kernel runs
  uint32_t site;
};

// f[r] = the factor (0 or scale) of P[row = n*H + h][query][key 4*kgroup + r]: one generator call per aligned group of four keys
__device__ __forceinline__ void attn_drop_factors(const AttnDrop& d, uint32_t row, int query, int kgroup, float (&f)[4]) {
  const uint64_t seed = (uint64_t)d.state[0];
  const uint32_t step = (uint32_t)(uint64_t)d.state[1];
  const philox_out o = philox4x32_10(row, ((uint32_t)query << 16) | (uint32_t)kgroup, d.site, step, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
  for (int r = 0; r < 4; ++r) f[r] = o.w[r] >= d.threshold ? d.scale : 0.f;
}

}  // namespace sn
