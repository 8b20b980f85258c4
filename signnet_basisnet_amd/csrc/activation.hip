// activation.hip — tanh / ELU(alpha = 1) of the DGL tree's sign-invariant encoders (`--sign_inv_activation`), forward and adjoint.
//
//   sn_act_affine_f32      y[r,c]  = rowvalid(r) ? fma(act(x[r,c]), scale[c], shift[c]) : 0        (scale = shift = NULL: y = act(x))
//   sn_act_affine_bwd_f32  dx[r,c] = rowvalid(r) ? dy[r,c] * act'(a[r,c]) : 0,  a = act(x): the forward's output WITHOUT an affine
//       tanh: act' = 1 - a*a, evaluated as fma(-a, a, 1);   elu: act' = a > 0 ? 1 : a + 1
//
// tanh is tanhf and elu's negative branch expm1f — the device library's accurate versions, no fast-math intrinsic — so a NaN stays a
// NaN and +-inf saturates (tanh: +-1; elu: +inf, -1).  Streaming kernels: one read and one write per element, no LDS, no atomics.  At
// the shapes of this project (~1.6 .. 7.5 M elements) they are bound by memory and launch latency; a lane owns four elements per
// iteration, the grid is capped at 2048 blocks (8 per CU) and strides beyond that, as dropout.hip.  Three access paths, chosen on the
// host, with the same per-element expression in each — the same bits:
//   row-vector   C % 4 == 0, every ld % 4 == 0, every pointer (scale / shift included) 16-byte aligned: a group is four columns of a row;
//   flat-vector  every ld == C (any C), the matrix pointers 16-byte aligned: one contiguous run, a group may straddle rows;
//   scalar       anything else: any ld >= C, 4-byte-aligned pointers, one element per lane and iteration.
#include "common.hpp"

namespace sn {

constexpr int ACT_MAX_BLOCKS = 2048;

// rows < 2^31 where nvalid is given (the host checks): the row mask of k_affine (ops.hip)
__device__ __forceinline__ bool act_row_ok(const int32_t* __restrict__ nvalid, int K, int64_t r) {
  if (!nvalid) return true;
  const unsigned node = (unsigned)r / (unsigned)K;
  return (int)((unsigned)r - node * (unsigned)K) < nvalid[node];
}

// The one per-element expression of every path.  Forward: p = x, q unused.  Adjoint: p = dy, q = a.
template <int ACT, bool BWD>
__device__ __forceinline__ float act1(float p, float q, float sc, float sh, bool affine) {
  if (BWD) {
    const float d = ACT == SN_ACT_TANH ? fmaf(-q, q, 1.f) : (q > 0.f ? 1.f : q + 1.f);
    return p * d;
  }
  const float a = ACT == SN_ACT_TANH ? tanhf(p) : (p > 0.f ? p : expm1f(p));
  return affine ? fmaf(a, sc, sh) : a;
}

template <int ACT, bool BWD>
__global__ __launch_bounds__(256) void k_act_row(const float* __restrict__ p, int ldp, const float* __restrict__ q, int ldq,
                                                 int64_t n_groups, int C, const int32_t* __restrict__ nvalid, int K,
                                                 const float* __restrict__ scale, const float* __restrict__ shift,
                                                 float* __restrict__ y, int ldy) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  const bool affine = !BWD && scale != nullptr;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_groups; t += stride) {
    const int64_t j = t << 2;
    const int64_t r = j / C;
    const int c = (int)(j - r * C);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (act_row_ok(nvalid, K, r)) {
      const f32x4 pv = *reinterpret_cast<const f32x4*>(p + r * ldp + c);
      f32x4 qv = {0.f, 0.f, 0.f, 0.f}, sc = {0.f, 0.f, 0.f, 0.f}, sh = {0.f, 0.f, 0.f, 0.f};
      if (BWD) qv = *reinterpret_cast<const f32x4*>(q + r * ldq + c);
      if (affine) {
        sc = *reinterpret_cast<const f32x4*>(scale + c);
        sh = *reinterpret_cast<const f32x4*>(shift + c);
      }
      v.x = act1<ACT, BWD>(pv.x, qv.x, sc.x, sh.x, affine);
      v.y = act1<ACT, BWD>(pv.y, qv.y, sc.y, sh.y, affine);
      v.z = act1<ACT, BWD>(pv.z, qv.z, sc.z, sh.z, affine);
      v.w = act1<ACT, BWD>(pv.w, qv.w, sc.w, sh.w, affine);
    }
    *reinterpret_cast<f32x4*>(y + r * ldy + c) = v;
  }
}

// Group t is the floats [4t, 4t + 4) of the contiguous run; the last group of a run whose length is no multiple of four is done
// element by element, so nothing past `total` is read or written.
template <int ACT, bool BWD>
__global__ __launch_bounds__(256) void k_act_flat(const float* __restrict__ p, const float* __restrict__ q, int64_t total,
                                                  int64_t n_groups, int C, const int32_t* __restrict__ nvalid, int K,
                                                  const float* __restrict__ scale, const float* __restrict__ shift,
                                                  float* __restrict__ y) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  const bool affine = !BWD && scale != nullptr;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_groups; t += stride) {
    const int64_t j = t << 2;
    int64_t r = j / C;
    int c = (int)(j - r * C);
    const bool full = j + 4 <= total;
    float pv[4] = {0.f, 0.f, 0.f, 0.f}, qv[4] = {0.f, 0.f, 0.f, 0.f}, v[4];
    if (full) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(p + j);
      pv[0] = a.x; pv[1] = a.y; pv[2] = a.z; pv[3] = a.w;
      if (BWD) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(q + j);
        qv[0] = b.x; qv[1] = b.y; qv[2] = b.z; qv[3] = b.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j + k < total) {
          pv[k] = p[j + k];
          if (BWD) qv[k] = q[j + k];
        }
    }
    bool ok = act_row_ok(nvalid, K, r);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = 0.f;
      if (j + k < total && ok) {
        const float sc = affine ? scale[c] : 0.f, sh = affine ? shift[c] : 0.f;
        v[k] = act1<ACT, BWD>(pv[k], qv[k], sc, sh, affine);
      }
      if (++c == C) {
        c = 0;
        ++r;
        if (j + k + 1 < total) ok = act_row_ok(nvalid, K, r);
      }
    }
    if (full) {
      f32x4 o;
      o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
      *reinterpret_cast<f32x4*>(y + j) = o;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j + k < total) y[j + k] = v[k];
    }
  }
}

template <int ACT, bool BWD>
__global__ __launch_bounds__(256) void k_act_scalar(const float* __restrict__ p, int ldp, const float* __restrict__ q, int ldq,
                                                    int64_t total, int C, const int32_t* __restrict__ nvalid, int K,
                                                    const float* __restrict__ scale, const float* __restrict__ shift,
                                                    float* __restrict__ y, int ldy) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  const bool affine = !BWD && scale != nullptr;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < total; j += stride) {
    const int64_t r = j / C;
    const int c = (int)(j - r * C);
    float v = 0.f;
    if (act_row_ok(nvalid, K, r)) {
      const float sc = affine ? scale[c] : 0.f, sh = affine ? shift[c] : 0.f;
      v = act1<ACT, BWD>(p[r * ldp + c], BWD ? q[r * ldq + c] : 0.f, sc, sh, affine);
    }
    y[r * ldy + c] = v;
  }
}

template <int ACT, bool BWD>
static void act_launch(const float* p, int ldp, const float* q, int ldq, int64_t R, int C, const int32_t* nvalid, int K,
                       const float* scale, const float* shift, float* y, int ldy, hipStream_t st) {
  const int64_t total = R * C;
  const uintptr_t mats = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(y);
  const uintptr_t vecs = reinterpret_cast<uintptr_t>(scale) | reinterpret_cast<uintptr_t>(shift);
  const bool ld4 = ((ldp | ldy | (BWD ? ldq : 0)) & 3) == 0;
  const bool flat = ldp == C && ldy == C && (!BWD || ldq == C);
  if ((mats & 15) == 0 && (vecs & 15) == 0 && (C & 3) == 0 && ld4) {
    const int64_t n_groups = total >> 2;
    const int64_t blocks = cdiv(n_groups, 256);
    hipLaunchKernelGGL((k_act_row<ACT, BWD>), dim3((unsigned)(blocks < ACT_MAX_BLOCKS ? blocks : ACT_MAX_BLOCKS)), dim3(256), 0, st, p, ldp,
                       q, ldq, n_groups, C, nvalid, K, scale, shift, y, ldy);
  } else if ((mats & 15) == 0 && flat) {
    const int64_t n_groups = (total + 3) >> 2;
    const int64_t blocks = cdiv(n_groups, 256);
    hipLaunchKernelGGL((k_act_flat<ACT, BWD>), dim3((unsigned)(blocks < ACT_MAX_BLOCKS ? blocks : ACT_MAX_BLOCKS)), dim3(256), 0, st, p, q,
                       total, n_groups, C, nvalid, K, scale, shift, y);
  } else {
    const int64_t blocks = cdiv(total, 256);
    hipLaunchKernelGGL((k_act_scalar<ACT, BWD>), dim3((unsigned)(blocks < ACT_MAX_BLOCKS ? blocks : ACT_MAX_BLOCKS)), dim3(256), 0, st, p,
                       ldp, q, ldq, total, C, nvalid, K, scale, shift, y, ldy);
  }
}

}  // namespace sn

extern "C" int sn_act_affine_f32(const float* x, int ldx, int64_t R, int C, const int32_t* nvalid, int K, int act, const float* scale,
                                 const float* shift, float* y, int ldy, void* stream) {
  using namespace sn;
  SN_REQUIRE(x && y && C > 0 && R >= 0 && ldx >= C && ldy >= C, "sn_act_affine_f32: bad arguments");
  SN_REQUIRE(act == SN_ACT_TANH || act == SN_ACT_ELU, "sn_act_affine_f32: unknown activation %d (SN_ACT_TANH, SN_ACT_ELU)", act);
  SN_REQUIRE((scale != nullptr) == (shift != nullptr), "sn_act_affine_f32: scale and shift go together");
  SN_REQUIRE(!nvalid || (K > 0 && R <= (int64_t)INT32_MAX), "sn_act_affine_f32: nvalid needs K > 0 and fewer than 2^31 rows");
  SN_REQUIRE(R <= (INT64_MAX >> 3) / C, "sn_act_affine_f32: element index out of range");
  SN_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(scale) |
               reinterpret_cast<uintptr_t>(shift) | reinterpret_cast<uintptr_t>(nvalid)) & 3) == 0,
             "sn_act_affine_f32: misaligned pointer");
  if (R == 0) return SN_OK;
  if (act == SN_ACT_TANH)
    act_launch<SN_ACT_TANH, false>(x, ldx, nullptr, 0, R, C, nvalid, K, scale, shift, y, ldy, (hipStream_t)stream);
  else
    act_launch<SN_ACT_ELU, false>(x, ldx, nullptr, 0, R, C, nvalid, K, scale, shift, y, ldy, (hipStream_t)stream);
  SN_CHECK_LAUNCH("sn_act_affine_f32");
  return SN_OK;
}

extern "C" int sn_act_affine_bwd_f32(const float* dy, int lddy, const float* a, int lda, int64_t R, int C, const int32_t* nvalid, int K,
                                     int act, float* dx, int lddx, void* stream) {
  using namespace sn;
  SN_REQUIRE(dy && a && dx && C > 0 && R >= 0 && lddy >= C && lda >= C && lddx >= C, "sn_act_affine_bwd_f32: bad arguments");
  SN_REQUIRE(act == SN_ACT_TANH || act == SN_ACT_ELU, "sn_act_affine_bwd_f32: unknown activation %d (SN_ACT_TANH, SN_ACT_ELU)", act);
  SN_REQUIRE(!nvalid || (K > 0 && R <= (int64_t)INT32_MAX), "sn_act_affine_bwd_f32: nvalid needs K > 0 and fewer than 2^31 rows");
  SN_REQUIRE(R <= (INT64_MAX >> 3) / C, "sn_act_affine_bwd_f32: element index out of range");
  SN_REQUIRE(((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(dx) |
               reinterpret_cast<uintptr_t>(nvalid)) & 3) == 0,
             "sn_act_affine_bwd_f32: misaligned pointer");
  if (R == 0) return SN_OK;
  if (act == SN_ACT_TANH)
    act_launch<SN_ACT_TANH, true>(dy, lddy, a, lda, R, C, nvalid, K, nullptr, nullptr, dx, lddx, (hipStream_t)stream);
  else
    act_launch<SN_ACT_ELU, true>(dy, lddy, a, lda, R, C, nvalid, K, nullptr, nullptr, dx, lddx, (hipStream_t)stream);
  SN_CHECK_LAUNCH("sn_act_affine_bwd_f32");
  return SN_OK;
}
