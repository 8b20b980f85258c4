// dropout.hip — train-mode dropout with a counter-based mask (Philox4x32-10, Salmon et al., SC'11; the Random123 constants).
// Nothing of the mask's size is stored: the forward and the backward evaluate the same generator at the same logical index, and the
// (seed, step) pair is read from device memory at run time, so a replay of a captured graph draws the current step's mask.
//
//   i    = base + r*C + c                              (logical index: independent of the row strides and of the pointers)
//   w    = philox4x32_10(counter = (lo32(i>>2), hi32(i>>2), site, lo32(step)), key = (lo32(seed), hi32(seed)))
//   keep = w[i & 3] >= threshold                       (threshold = floor(p * 2^32) on the host)
//   y    = (keep ? x * scale : 0) + residual
//
// One Philox call yields the four words of one aligned group of four logical elements; a lane owns one group.  Memory-bound, and at
// this project's shapes ([3001, 128], [E, 77]: ~100-400 K elements) latency-bound: one group per lane keeps every load of a lane in
// flight at once, the grid is capped at 2048 blocks (8 per CU) and strides beyond that.
#include "philox.hpp"

namespace sn {

constexpr int DROPOUT_MAX_BLOCKS = 2048;

// Vector path: C % 4 == 0, base % 4 == 0, every ld % 4 == 0, every pointer 16-byte aligned — a group is four consecutive columns
// of one row: one 128-bit load (two with a residual) and one 128-bit store per Philox call.
__global__ __launch_bounds__(256) void k_dropout_vec(const float* __restrict__ x, int ldx, int64_t n_groups, int C, uint32_t threshold,
                                                     float scale, const int64_t* __restrict__ state, uint32_t site, int64_t base,
                                                     const float* __restrict__ res, int ldr, float* __restrict__ y, int ldy) {
  const uint64_t seed = (uint64_t)state[0];
  const uint32_t step = (uint32_t)(uint64_t)state[1];
  const int64_t g0 = base >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_groups; t += stride) {
    const int64_t j = t << 2;
    const int64_t r = j / C;
    const int c = (int)(j - r * C);
    const uint64_t g = (uint64_t)(g0 + t);
    const philox_out o = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), site, step, (uint32_t)seed, (uint32_t)(seed >> 32));
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + r * ldx + c);
    f32x4 v;
    v.x = o.w[0] >= threshold ? xv.x * scale : 0.f;
    v.y = o.w[1] >= threshold ? xv.y * scale : 0.f;
    v.z = o.w[2] >= threshold ? xv.z * scale : 0.f;
    v.w = o.w[3] >= threshold ? xv.w * scale : 0.f;
    if (res) v += *reinterpret_cast<const f32x4*>(res + r * ldr + c);
    *reinterpret_cast<f32x4*>(y + r * ldy + c) = v;
  }
}

// Scalar path: any C, any ld >= C, 4-byte-aligned pointers, any base.  A lane still owns one aligned group of four logical indices
// [4g, 4g + 4); the group may start before `base`, end after the last element, and straddle a row boundary.
__global__ __launch_bounds__(256) void k_dropout_scalar(const float* __restrict__ x, int ldx, int64_t total, int64_t n_groups, int C,
                                                        uint32_t threshold, float scale, const int64_t* __restrict__ state, uint32_t site,
                                                        int64_t base, const float* __restrict__ res, int ldr, float* __restrict__ y,
                                                        int ldy) {
  const uint64_t seed = (uint64_t)state[0];
  const uint32_t step = (uint32_t)(uint64_t)state[1];
  const int64_t g0 = base >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_groups; t += stride) {
    const uint64_t g = (uint64_t)(g0 + t);
    const philox_out o = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), site, step, (uint32_t)seed, (uint32_t)(seed >> 32));
    const int64_t j0 = (int64_t)(g << 2) - base;      // position of the group's first index in [0, total): may be negative
    int64_t r = j0 >= 0 ? j0 / C : 0;
    int64_t c = j0 - r * C;                            // (negative for the indices before `base`)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t j = j0 + k;
      if (j >= 0 && j < total) {
        float v = o.w[k] >= threshold ? x[r * ldx + c] * scale : 0.f;
        if (res) v += res[r * ldr + c];
        y[r * ldy + c] = v;
      }
      if (++c == C) { c = 0; ++r; }
    }
  }
}

}  // namespace sn

extern "C" int sn_dropout_f32(const float* x, int ldx, int64_t R, int C, uint32_t threshold, float scale, const int64_t* state,
                              uint32_t site, int64_t base, const float* residual, int ldr, float* y, int ldy, void* stream) {
  using namespace sn;
  SN_REQUIRE(x && y && state && C > 0 && R >= 0 && ldx >= C && ldy >= C && base >= 0, "sn_dropout_f32: bad arguments");
  SN_REQUIRE(!residual || ldr >= C, "sn_dropout_f32: residual rows too narrow");
  SN_REQUIRE(R <= (INT64_MAX >> 3) / C && base <= (INT64_MAX >> 3) - R * C, "sn_dropout_f32: logical index out of range");
  SN_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(residual) |
               reinterpret_cast<uintptr_t>(state)) & 3) == 0 && (reinterpret_cast<uintptr_t>(state) & 7) == 0,
             "sn_dropout_f32: misaligned pointer");
  if (R == 0) return SN_OK;
  const int64_t total = R * C;
  const uintptr_t align = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(residual);
  const bool vec = (C & 3) == 0 && (base & 3) == 0 && (ldx & 3) == 0 && (ldy & 3) == 0 && (!residual || (ldr & 3) == 0) && (align & 15) == 0;
  if (vec) {
    const int64_t n_groups = total >> 2;
    const int64_t blocks = cdiv(n_groups, 256);
    hipLaunchKernelGGL(k_dropout_vec, dim3((unsigned)(blocks < DROPOUT_MAX_BLOCKS ? blocks : DROPOUT_MAX_BLOCKS)), dim3(256), 0,
                       (hipStream_t)stream, x, ldx, n_groups, C, threshold, scale, state, site, base, residual, ldr, y, ldy);
  } else {
    const int64_t n_groups = ((base + total - 1) >> 2) - (base >> 2) + 1;
    const int64_t blocks = cdiv(n_groups, 256);
    hipLaunchKernelGGL(k_dropout_scalar, dim3((unsigned)(blocks < DROPOUT_MAX_BLOCKS ? blocks : DROPOUT_MAX_BLOCKS)), dim3(256), 0,
                       (hipStream_t)stream, x, ldx, total, n_groups, C, threshold, scale, state, site, base, residual, ldr, y, ldy);
  }
  SN_CHECK_LAUNCH("sn_dropout_f32");
  return SN_OK;
}
