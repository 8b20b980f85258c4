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

// ---------------------------------------------------------------------------------------------------------------------------------
// BatchNorm apply + dropout in one launch (sn_affine_dropout_f32): y = rowvalid(r) && keep(r,c) ? fma(x, scale[c], shift[c]) * pscale : 0.
// The mask is k_dropout_*'s, the affine is k_affine's (ops.hip) — there `v * scale[c] + shift[c]` is contracted to one v_fma_f32 by
// the compiler's default, here it is written as fmaf — and the product with pscale is rounded on its own, so the result equals the two
// launches composed bit for bit.  Three kernels, one Philox call per aligned group of four logical indices in each.

// rows < 2^31 where nvalid is given (the host checks): the row mask of k_affine
__device__ __forceinline__ bool row_ok(const int32_t* __restrict__ nvalid, int K, int64_t r) {
  if (!nvalid) return true;
  const unsigned node = (unsigned)r / (unsigned)K;
  return (int)((unsigned)r - node * (unsigned)K) < nvalid[node];
}

__device__ __forceinline__ float affdrop1(bool keep, float x, float sc, float sh, bool affine, float pscale) {
  return keep ? (affine ? fmaf(x, sc, sh) : x) * pscale : 0.f;
}

// Row-vector path: C % 4 == 0, every ld % 4 == 0, base % 4 == 0, x / y / scale / shift 16-byte aligned: a group is four columns of
// one row; x, y, scale and shift move in 128-bit accesses.
__global__ __launch_bounds__(256) void k_affdrop_row(const float* __restrict__ x, int ldx, int64_t n_groups, int C,
                                                     const int32_t* __restrict__ nvalid, int K, const float* __restrict__ scale,
                                                     const float* __restrict__ shift, uint32_t threshold, float pscale,
                                                     const int64_t* __restrict__ state, uint32_t site, int64_t base,
                                                     float* __restrict__ y, int ldy) {
  const uint64_t seed = (uint64_t)state[0];
  const uint32_t step = (uint32_t)(uint64_t)state[1];
  const int64_t g0 = base >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const bool affine = scale != nullptr;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_groups; t += stride) {
    const int64_t j = t << 2;
    const int64_t r = j / C;
    const int c = (int)(j - r * C);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row_ok(nvalid, K, r)) {
      const uint64_t g = (uint64_t)(g0 + t);
      const philox_out o = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), site, step, (uint32_t)seed, (uint32_t)(seed >> 32));
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + r * ldx + c);
      f32x4 sc = {0.f, 0.f, 0.f, 0.f}, sh = {0.f, 0.f, 0.f, 0.f};
      if (affine) {
        sc = *reinterpret_cast<const f32x4*>(scale + c);
        sh = *reinterpret_cast<const f32x4*>(shift + c);
      }
      v.x = affdrop1(o.w[0] >= threshold, xv.x, sc.x, sh.x, affine, pscale);
      v.y = affdrop1(o.w[1] >= threshold, xv.y, sc.y, sh.y, affine, pscale);
      v.z = affdrop1(o.w[2] >= threshold, xv.z, sc.z, sh.z, affine, pscale);
      v.w = affdrop1(o.w[3] >= threshold, xv.w, sc.w, sh.w, affine, pscale);
    }
    *reinterpret_cast<f32x4*>(y + r * ldy + c) = v;
  }
}

// Flat-vector path: ldx == ldy == C (any C), base % 4 == 0, x / y 16-byte aligned: the tensor is one contiguous run of `total` floats,
// group t is the floats [4t, 4t + 4) — one 128-bit load and store — and may straddle a row boundary (several when C < 4): the row's
// validity and the column of scale / shift are taken per element.  The last group of a run whose length is no multiple of four is
// done element by element, so nothing past `total` is read or written.
__global__ __launch_bounds__(256) void k_affdrop_flat(const float* __restrict__ x, int64_t total, int64_t n_groups, int C,
                                                      const int32_t* __restrict__ nvalid, int K, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, uint32_t threshold, float pscale,
                                                      const int64_t* __restrict__ state, uint32_t site, int64_t base,
                                                      float* __restrict__ y) {
  const uint64_t seed = (uint64_t)state[0];
  const uint32_t step = (uint32_t)(uint64_t)state[1];
  const int64_t g0 = base >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const bool affine = scale != nullptr;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_groups; t += stride) {
    const int64_t j = t << 2;
    int64_t r = j / C;
    int c = (int)(j - r * C);
    const uint64_t g = (uint64_t)(g0 + t);
    const philox_out o = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), site, step, (uint32_t)seed, (uint32_t)(seed >> 32));
    const bool full = j + 4 <= total;
    float xv[4] = {0.f, 0.f, 0.f, 0.f}, v[4];
    if (full) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(x + j);
      xv[0] = q.x; xv[1] = q.y; xv[2] = q.z; xv[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j + k < total) xv[k] = x[j + k];
    }
    bool ok = row_ok(nvalid, K, r);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = 0.f;
      if (j + k < total) {
        const float sc = affine ? scale[c] : 0.f, sh = affine ? shift[c] : 0.f;
        v[k] = affdrop1(ok && o.w[k] >= threshold, xv[k], sc, sh, affine, pscale);
      }
      if (++c == C) {
        c = 0;
        ++r;
        if (j + k + 1 < total) ok = row_ok(nvalid, K, r);
      }
    }
    if (full) {
      f32x4 q;
      q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
      *reinterpret_cast<f32x4*>(y + j) = q;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j + k < total) y[j + k] = v[k];
    }
  }
}

// Scalar path: any C, any ld >= C, 4-byte-aligned pointers, any base: the group handling of k_dropout_scalar.
__global__ __launch_bounds__(256) void k_affdrop_scalar(const float* __restrict__ x, int ldx, int64_t total, int64_t n_groups, int C,
                                                        const int32_t* __restrict__ nvalid, int K, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, uint32_t threshold, float pscale,
                                                        const int64_t* __restrict__ state, uint32_t site, int64_t base,
                                                        float* __restrict__ y, int ldy) {
  const uint64_t seed = (uint64_t)state[0];
  const uint32_t step = (uint32_t)(uint64_t)state[1];
  const int64_t g0 = base >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const bool affine = scale != nullptr;
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
        float v = 0.f;
        if (row_ok(nvalid, K, r)) {
          const float sc = affine ? scale[c] : 0.f, sh = affine ? shift[c] : 0.f;
          v = affdrop1(o.w[k] >= threshold, x[r * ldx + c], sc, sh, affine, pscale);
        }
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

extern "C" int sn_affine_dropout_f32(const float* x, int ldx, int64_t R, int C, const int32_t* nvalid, int K, const float* scale,
                                     const float* shift, uint32_t threshold, float pscale, const int64_t* state, uint32_t site,
                                     int64_t base, float* y, int ldy, void* stream) {
  using namespace sn;
  SN_REQUIRE(x && y && state && C > 0 && R >= 0 && ldx >= C && ldy >= C && base >= 0, "sn_affine_dropout_f32: bad arguments");
  SN_REQUIRE((scale != nullptr) == (shift != nullptr), "sn_affine_dropout_f32: scale and shift go together");
  SN_REQUIRE(!nvalid || (K > 0 && R <= (int64_t)INT32_MAX), "sn_affine_dropout_f32: nvalid needs K > 0 and fewer than 2^31 rows");
  SN_REQUIRE(R <= (INT64_MAX >> 3) / C && base <= (INT64_MAX >> 3) - R * C, "sn_affine_dropout_f32: logical index out of range");
  SN_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(scale) |
               reinterpret_cast<uintptr_t>(shift) | reinterpret_cast<uintptr_t>(nvalid) | reinterpret_cast<uintptr_t>(state)) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(state) & 7) == 0,
             "sn_affine_dropout_f32: misaligned pointer");
  if (R == 0) return SN_OK;
  const int64_t total = R * C;
  const bool aligned = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0 && (base & 3) == 0;
  const bool params16 = ((reinterpret_cast<uintptr_t>(scale) | reinterpret_cast<uintptr_t>(shift)) & 15) == 0;
  const hipStream_t st = (hipStream_t)stream;
  if (aligned && (C & 3) == 0 && (ldx & 3) == 0 && (ldy & 3) == 0 && params16) {
    const int64_t n_groups = total >> 2;
    const int64_t blocks = cdiv(n_groups, 256);
    hipLaunchKernelGGL(k_affdrop_row, dim3((unsigned)(blocks < DROPOUT_MAX_BLOCKS ? blocks : DROPOUT_MAX_BLOCKS)), dim3(256), 0, st, x, ldx,
                       n_groups, C, nvalid, K, scale, shift, threshold, pscale, state, site, base, y, ldy);
  } else if (aligned && ldx == C && ldy == C) {
    const int64_t n_groups = (total + 3) >> 2;
    const int64_t blocks = cdiv(n_groups, 256);
    hipLaunchKernelGGL(k_affdrop_flat, dim3((unsigned)(blocks < DROPOUT_MAX_BLOCKS ? blocks : DROPOUT_MAX_BLOCKS)), dim3(256), 0, st, x, total,
                       n_groups, C, nvalid, K, scale, shift, threshold, pscale, state, site, base, y);
  } else {
    const int64_t n_groups = ((base + total - 1) >> 2) - (base >> 2) + 1;
    const int64_t blocks = cdiv(n_groups, 256);
    hipLaunchKernelGGL(k_affdrop_scalar, dim3((unsigned)(blocks < DROPOUT_MAX_BLOCKS ? blocks : DROPOUT_MAX_BLOCKS)), dim3(256), 0, st, x, ldx,
                       total, n_groups, C, nvalid, K, scale, shift, threshold, pscale, state, site, base, y, ldy);
  }
  SN_CHECK_LAUNCH("sn_affine_dropout_f32");
  return SN_OK;
}
