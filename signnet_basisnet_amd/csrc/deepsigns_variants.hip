// deepsigns_variants.hip — the two operations the 'gcn' and 'transformer' sign-invariant encoders of the DGL tree add
// (GraphPrediction/layers/deepsigns.py:13-31,89-119): dgl.nn.pytorch.GraphConv's symmetric-normalised propagation and the per-graph
// multi-head self-attention of dgl.nn.pytorch.glob.SetTransformerEncoder, both restated from DGL's published definitions.
#include "common.hpp"

namespace {
using namespace sn;

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ============================================================================ GraphConv(norm='both') propagation
// out[i, c] = cin[i] * sum_{e in in(i), edge-id order} cout[col[e]] * x[col[e], c]  (+ bias[c % width])
//   cin[i] = clamp(rowptr[i+1] - rowptr[i], 1)^-1/2, cout[j] = clamp(rowptr_t[j+1] - rowptr_t[j], 1)^-1/2.
// One thread owns one output element (VEC: four consecutive channels); the products are rounded before they are added, as
// the reference's `feat * norm` followed by copy_u / sum rounds them.  No atomics, fixed order: bit-reproducible.
template <bool VEC>
__global__ __launch_bounds__(256) void k_gcn_propagate(const float* __restrict__ x, int64_t ldx, int64_t N, int CV,
                                                       const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                       const int32_t* __restrict__ rowptr_t, const float* __restrict__ bias, int width,
                                                       float* __restrict__ out, int64_t ldo) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t i = idx / CV;
  if (i >= N) return;
  const int c = (int)(idx - i * CV) * (VEC ? 4 : 1);
  const int lo = rowptr[i], hi = rowptr[i + 1];
  const int din = hi - lo;
  const float cin = 1.f / sqrtf((float)(din > 1 ? din : 1));
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int e = lo; e < hi; ++e) {
    const int64_t j = col[e];
    if (j < 0 || j >= N) continue;                         // (a malformed plan is reported by its own status word)
    const int dout = rowptr_t[j + 1] - rowptr_t[j];
    const float cj = 1.f / sqrtf((float)(dout > 1 ? dout : 1));
    if (VEC) {
      const float4 v = *reinterpret_cast<const float4*>(x + j * ldx + c);
      a0 = __fadd_rn(a0, __fmul_rn(v.x, cj));
      a1 = __fadd_rn(a1, __fmul_rn(v.y, cj));
      a2 = __fadd_rn(a2, __fmul_rn(v.z, cj));
      a3 = __fadd_rn(a3, __fmul_rn(v.w, cj));
    } else {
      a0 = __fadd_rn(a0, __fmul_rn(x[j * ldx + c], cj));
    }
  }
  if (VEC) {
    float4 r = make_float4(__fmul_rn(a0, cin), __fmul_rn(a1, cin), __fmul_rn(a2, cin), __fmul_rn(a3, cin));
    if (bias) {
      const float4 b = *reinterpret_cast<const float4*>(bias + c % width);
      r.x += b.x; r.y += b.y; r.z += b.z; r.w += b.w;
    }
    *reinterpret_cast<float4*>(out + i * ldo + c) = r;
  } else {
    float r = __fmul_rn(a0, cin);
    if (bias) r += bias[c % width];
    out[i * ldo + c] = r;
  }
}

// ============================================================================ per-graph multi-head self-attention
// A set is (graph b, slot s): the rows node * S + s of the nodes of graph b.  One wave per (set, head); a thread owns a query (forward,
// dq) or a key (dk, dv), the other side streams through LDS in tiles of ATT_T rows and is read as a broadcast.  A set of at most
// ATT_T nodes is staged once; a larger one is walked tile by tile with an online softmax.  DHP = dh rounded up to the template's
// width, zero padded in registers and LDS, so every inner loop has a constant trip count.
constexpr int ATT_T = 64;

template <int DHP>
__device__ __forceinline__ void att_stage(float* __restrict__ dst, const float* __restrict__ src, int64_t ld, int64_t row0, int S, int tn,
                                          int dh) {
  for (int idx = threadIdx.x; idx < ATT_T * DHP; idx += 64) {
    const int r = idx / DHP, d = idx - r * DHP;
    dst[idx] = (r < tn && d < dh) ? src[(row0 + (int64_t)r * S) * ld + d] : 0.f;
  }
}

template <int DHP>
__device__ __forceinline__ float att_dot(const float* __restrict__ a, const float* __restrict__ lds_row) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < DHP; d += 4) {
    const float4 t = *reinterpret_cast<const float4*>(lds_row + d);
    s = fmaf(a[d], t.x, s); s = fmaf(a[d + 1], t.y, s); s = fmaf(a[d + 2], t.z, s); s = fmaf(a[d + 3], t.w, s);
  }
  return s;
}

template <int DHP>
__device__ __forceinline__ void att_axpy(float* __restrict__ acc, float w, const float* __restrict__ lds_row) {
#pragma unroll
  for (int d = 0; d < DHP; d += 4) {
    const float4 t = *reinterpret_cast<const float4*>(lds_row + d);
    acc[d] = fmaf(w, t.x, acc[d]); acc[d + 1] = fmaf(w, t.y, acc[d + 1]);
    acc[d + 2] = fmaf(w, t.z, acc[d + 2]); acc[d + 3] = fmaf(w, t.w, acc[d + 3]);
  }
}

struct AttSet { int64_t n0; int n, s, h; };

__device__ __forceinline__ AttSet att_set(const int32_t* __restrict__ graph_ptr, int64_t N, int S, int heads) {
  const int64_t blk = blockIdx.x;
  const int h = (int)(blk % heads);
  const int64_t bs = blk / heads;
  const int s = (int)(bs % S);
  const int64_t b = bs / S;
  int64_t n0 = graph_ptr[b], n1 = graph_ptr[b + 1];
  if (n0 < 0) n0 = 0;
  if (n1 > N) n1 = N;
  return AttSet{n0, n1 > n0 ? (int)(n1 - n0) : 0, s, h};
}

template <int DHP>
__global__ __launch_bounds__(64) void k_graph_attention(const float* __restrict__ q, const float* __restrict__ k,
                                                        const float* __restrict__ v, int64_t ld, const int32_t* __restrict__ graph_ptr,
                                                        int64_t N, int S, int heads, int dh, float scale, float* __restrict__ out,
                                                        int64_t ldo, float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) float Ks[ATT_T * DHP];
  __shared__ __attribute__((aligned(16))) float Vs[ATT_T * DHP];
  const AttSet st = att_set(graph_ptr, N, S, heads);
  if (st.n == 0) return;
  const int hoff = st.h * dh;
  for (int q0 = 0; q0 < st.n; q0 += 64) {
    const int qi = q0 + (int)threadIdx.x;
    const bool live = qi < st.n;
    const int64_t qrow = (st.n0 + (live ? qi : 0)) * S + st.s;
    float qr[DHP], acc[DHP];
#pragma unroll
    for (int d = 0; d < DHP; ++d) {
      qr[d] = (live && d < dh) ? q[qrow * ld + hoff + d] : 0.f;
      acc[d] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    for (int j0 = 0; j0 < st.n; j0 += ATT_T) {
      const int tn = st.n - j0 < ATT_T ? st.n - j0 : ATT_T;
      __syncthreads();
      att_stage<DHP>(Ks, k + hoff, ld, (st.n0 + j0) * S + st.s, S, tn, dh);
      att_stage<DHP>(Vs, v + hoff, ld, (st.n0 + j0) * S + st.s, S, tn, dh);
      __syncthreads();
      for (int j = 0; j < tn; ++j) {
        const float sc = att_dot<DHP>(qr, Ks + j * DHP) * scale;
        if (sc > m) {
          const float c = expf(m - sc);                       // (first key: exp(-inf) = 0)
          l *= c;
#pragma unroll
          for (int d = 0; d < DHP; ++d) acc[d] *= c;
          m = sc;
        }
        const float p = expf(sc - m);
        l += p;
        att_axpy<DHP>(acc, p, Vs + j * DHP);
      }
    }
    if (live) {
#pragma unroll
      for (int d = 0; d < DHP; ++d)
        if (d < dh) out[qrow * ldo + hoff + d] = acc[d] / l;
      lse[qrow * heads + st.h] = m + logf(l);
    }
  }
}

// Backward: delta = dout . out per query, then dq per query over key tiles, then dk / dv per key over query tiles; every sum has one
// owner and runs in node order.  P = exp(q.k * scale - lse), dS = P * (dout.v - delta), dq = scale * dS k, dk = scale * dS^T q, dv = P^T dout.
template <int DHP>
__global__ __launch_bounds__(64) void k_graph_attention_bwd(const float* __restrict__ q, const float* __restrict__ k,
                                                            const float* __restrict__ v, int64_t ld, const float* __restrict__ out,
                                                            int64_t ldo, const float* __restrict__ lse, const float* __restrict__ dout,
                                                            int64_t lddo, const int32_t* __restrict__ graph_ptr, int64_t N, int S,
                                                            int heads, int dh, float scale, float* __restrict__ dq,
                                                            float* __restrict__ dk, float* __restrict__ dv, int64_t ldg,
                                                            float* delta) {
  __shared__ __attribute__((aligned(16))) float As[ATT_T * DHP];
  __shared__ __attribute__((aligned(16))) float Bs[ATT_T * DHP];
  __shared__ float Ls[ATT_T], Ds[ATT_T];
  const AttSet st = att_set(graph_ptr, N, S, heads);
  if (st.n == 0) return;
  const int hoff = st.h * dh;
  // ---- delta, dq: a thread per query, K and V in LDS
  for (int q0 = 0; q0 < st.n; q0 += 64) {
    const int qi = q0 + (int)threadIdx.x;
    const bool live = qi < st.n;
    const int64_t qrow = (st.n0 + (live ? qi : 0)) * S + st.s;
    float qr[DHP], go[DHP], acc[DHP];
    float dl = 0.f;
#pragma unroll
    for (int d = 0; d < DHP; ++d) {
      const bool on = live && d < dh;
      qr[d] = on ? q[qrow * ld + hoff + d] : 0.f;
      go[d] = on ? dout[qrow * lddo + hoff + d] : 0.f;
      dl = fmaf(go[d], on ? out[qrow * ldo + hoff + d] : 0.f, dl);
      acc[d] = 0.f;
    }
    const float li = live ? lse[qrow * heads + st.h] : 0.f;
    if (live) delta[qrow * heads + st.h] = dl;
    for (int j0 = 0; j0 < st.n; j0 += ATT_T) {
      const int tn = st.n - j0 < ATT_T ? st.n - j0 : ATT_T;
      __syncthreads();
      att_stage<DHP>(As, k + hoff, ld, (st.n0 + j0) * S + st.s, S, tn, dh);
      att_stage<DHP>(Bs, v + hoff, ld, (st.n0 + j0) * S + st.s, S, tn, dh);
      __syncthreads();
      for (int j = 0; j < tn; ++j) {
        const float p = expf(att_dot<DHP>(qr, As + j * DHP) * scale - li);
        const float ds = p * (att_dot<DHP>(go, Bs + j * DHP) - dl);
        att_axpy<DHP>(acc, ds, As + j * DHP);
      }
    }
    if (live) {
#pragma unroll
      for (int d = 0; d < DHP; ++d)
        if (d < dh) dq[qrow * ldg + hoff + d] = acc[d] * scale;
    }
  }
  // ---- dk, dv: a thread per key, Q and dout (with lse and delta) in LDS.  delta was written by this workgroup: made visible by the barrier.
  __threadfence_block();
  for (int k0 = 0; k0 < st.n; k0 += 64) {
    const int ki = k0 + (int)threadIdx.x;
    const bool live = ki < st.n;
    const int64_t krow = (st.n0 + (live ? ki : 0)) * S + st.s;
    float kr[DHP], vr[DHP], gk[DHP], gv[DHP];
#pragma unroll
    for (int d = 0; d < DHP; ++d) {
      const bool on = live && d < dh;
      kr[d] = on ? k[krow * ld + hoff + d] : 0.f;
      vr[d] = on ? v[krow * ld + hoff + d] : 0.f;
      gk[d] = 0.f;
      gv[d] = 0.f;
    }
    for (int i0 = 0; i0 < st.n; i0 += ATT_T) {
      const int tn = st.n - i0 < ATT_T ? st.n - i0 : ATT_T;
      __syncthreads();
      att_stage<DHP>(As, q + hoff, ld, (st.n0 + i0) * S + st.s, S, tn, dh);
      att_stage<DHP>(Bs, dout + hoff, lddo, (st.n0 + i0) * S + st.s, S, tn, dh);
      if ((int)threadIdx.x < tn) {
        const int64_t r = (st.n0 + i0 + threadIdx.x) * S + st.s;
        Ls[threadIdx.x] = lse[r * heads + st.h];
        Ds[threadIdx.x] = delta[r * heads + st.h];
      }
      __syncthreads();
      for (int i = 0; i < tn; ++i) {
        const float p = expf(att_dot<DHP>(kr, As + i * DHP) * scale - Ls[i]);
        const float ds = p * (att_dot<DHP>(vr, Bs + i * DHP) - Ds[i]);
        att_axpy<DHP>(gv, p, Bs + i * DHP);
        att_axpy<DHP>(gk, ds, As + i * DHP);
      }
    }
    if (live) {
#pragma unroll
      for (int d = 0; d < DHP; ++d)
        if (d < dh) {
          dk[krow * ldg + hoff + d] = gk[d] * scale;
          dv[krow * ldg + hoff + d] = gv[d];
        }
    }
  }
}

int att_args(const char* fn, int64_t N, int64_t B, int S, int heads, int dh, int64_t ld) {
  SN_REQUIRE(N >= 0 && B >= 0 && S >= 1 && heads >= 1 && dh >= 1, "%s: bad sizes", fn);
  SN_REQUIRE(ld >= (int64_t)heads * dh, "%s: row stride smaller than heads * dh", fn);
  SN_REQUIRE(B * S * heads < ((int64_t)1 << 31), "%s: too many sets for one launch", fn);
  if (dh > 64) return sn::fail(SN_ERR_UNSUPPORTED, "%s: head width %d > 64 is not built", fn, dh);
  return SN_OK;
}

}  // namespace

extern "C" int sn_gcn_propagate_f32(const float* x, int64_t ldx, int64_t N, int C, const int32_t* rowptr, const int32_t* col,
                                    const int32_t* rowptr_t, const float* bias, int width, float* out, int64_t ldo, void* stream) {
  SN_REQUIRE(x && out && rowptr && col && rowptr_t && N >= 0 && C > 0, "sn_gcn_propagate_f32: bad arguments");
  SN_REQUIRE(ldx >= C && ldo >= C, "sn_gcn_propagate_f32: row stride smaller than C");
  SN_REQUIRE(x != out, "sn_gcn_propagate_f32: in-place propagation is not supported");
  SN_REQUIRE(!bias || (width > 0 && C % width == 0), "sn_gcn_propagate_f32: bias needs a width that divides C");
  if (N == 0) return SN_OK;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = C % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && al16(x) && al16(out) && (!bias || (width % 4 == 0 && al16(bias)));
  const int CV = vec ? C / 4 : C;
  const int64_t nblk = cdiv(N * CV, 256);
  SN_REQUIRE(nblk < ((int64_t)1 << 31), "sn_gcn_propagate_f32: too many elements for one launch");
  if (vec)
    hipLaunchKernelGGL((k_gcn_propagate<true>), dim3((unsigned)nblk), dim3(256), 0, st, x, ldx, N, CV, rowptr, col, rowptr_t, bias, width, out, ldo);
  else
    hipLaunchKernelGGL((k_gcn_propagate<false>), dim3((unsigned)nblk), dim3(256), 0, st, x, ldx, N, CV, rowptr, col, rowptr_t, bias, width, out, ldo);
  SN_CHECK_LAUNCH("sn_gcn_propagate_f32");
  return SN_OK;
}

extern "C" int sn_graph_attention_f32(const float* q, const float* k, const float* v, int64_t ld, const int32_t* graph_ptr, int64_t N,
                                      int64_t B, int S, int heads, int dh, float* out, int64_t ldo, float* lse, void* stream) {
  SN_REQUIRE(q && k && v && graph_ptr && out && lse, "sn_graph_attention_f32: bad arguments");
  const int rc = att_args("sn_graph_attention_f32", N, B, S, heads, dh, ld);
  if (rc != SN_OK) return rc;
  SN_REQUIRE(ldo >= (int64_t)heads * dh, "sn_graph_attention_f32: output row stride smaller than heads * dh");
  if (N == 0 || B == 0) return SN_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(B * S * heads)), block(64);
  const float scale = 1.f / sqrtf((float)dh);
#define SN_ATT_FWD(D) hipLaunchKernelGGL((k_graph_attention<D>), grid, block, 0, st, q, k, v, ld, graph_ptr, N, S, heads, dh, scale, out, ldo, lse)
  if (dh <= 8) SN_ATT_FWD(8);
  else if (dh <= 16) SN_ATT_FWD(16);
  else if (dh <= 32) SN_ATT_FWD(32);
  else if (dh <= 48) SN_ATT_FWD(48);
  else SN_ATT_FWD(64);
#undef SN_ATT_FWD
  SN_CHECK_LAUNCH("sn_graph_attention_f32");
  return SN_OK;
}

extern "C" int sn_graph_attention_bwd_f32(const float* q, const float* k, const float* v, int64_t ld, const float* out, int64_t ldo,
                                          const float* lse, const float* dout, int64_t lddo, const int32_t* graph_ptr, int64_t N, int64_t B,
                                          int S, int heads, int dh, float* dq, float* dk, float* dv, int64_t ldg, float* delta,
                                          void* stream) {
  SN_REQUIRE(q && k && v && out && lse && dout && graph_ptr && dq && dk && dv && delta, "sn_graph_attention_bwd_f32: bad arguments");
  const int rc = att_args("sn_graph_attention_bwd_f32", N, B, S, heads, dh, ld);
  if (rc != SN_OK) return rc;
  SN_REQUIRE(ldo >= (int64_t)heads * dh && lddo >= (int64_t)heads * dh && ldg >= (int64_t)heads * dh,
             "sn_graph_attention_bwd_f32: a row stride is smaller than heads * dh");
  if (N == 0 || B == 0) return SN_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(B * S * heads)), block(64);
  const float scale = 1.f / sqrtf((float)dh);
#define SN_ATT_BWD(D)                                                                                                                  \
  hipLaunchKernelGGL((k_graph_attention_bwd<D>), grid, block, 0, st, q, k, v, ld, out, ldo, lse, dout, lddo, graph_ptr, N, S, heads, dh, \
                     scale, dq, dk, dv, ldg, delta)
  if (dh <= 8) SN_ATT_BWD(8);
  else if (dh <= 16) SN_ATT_BWD(16);
  else if (dh <= 32) SN_ATT_BWD(32);
  else if (dh <= 48) SN_ATT_BWD(48);
  else SN_ATT_BWD(64);
#undef SN_ATT_BWD
  SN_CHECK_LAUNCH("sn_graph_attention_bwd_f32");
  return SN_OK;
}
