// set2set.hip — the Set2Set readout (Vinyals et al., "Order Matters"; PyG's Set2Set(d, processing_steps=T), one LSTM layer) of the
// Alchemy baseline (baseline_gin.py:43,58): one launch per direction, one 256-thread workgroup per graph, all T steps inside it.
//
//   q* = 0 [2d], h = c = 0;  for t = 1..T:
//     gates = W_ih q* + b_ih + W_hh h + b_hh   (rows i | f | g | o);  c = s(f) c + s(i) tanh(g);  h = s(o) tanh(c);  q = h
//     e_n = <x_n, q>;  a = softmax over the graph's nodes (max subtracted, denominator + 1e-16);  r = sum_n a_n x_n;  q* = [q, r]
//
// No workgroup talks to another; nothing is accumulated with atomics: every sum has one owner and a fixed order, so forward and
// adjoint are bit-reproducible.  The graph's rows are streamed node by node (wave w owns nodes n0 + w, n0 + w + 4, ...: any graph size)
// and re-read from L2 every step; lanes own channels c = lane, lane + 64.  Only 4-byte alignment is assumed of any pointer.
#include <math.h>

#include "common.hpp"

namespace sn {
namespace {

constexpr int S2S_THREADS = 256;
constexpr int S2S_WAVES = S2S_THREADS / WAVE;
constexpr int S2S_MAX_D = 128;

__device__ __forceinline__ float sigmoid_acc(float v) { return 1.0f / (1.0f + expf(-v)); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}

// wt [3d][4d]: wt[k][j] = k < 2d ? W_ih[j][k] : W_hh[j][k - 2d]  (consecutive lanes read consecutive gate rows);  bias [4d] = b_ih + b_hh
__global__ void k_s2s_pack(const float* __restrict__ w_ih, const float* __restrict__ w_hh, const float* __restrict__ b_ih,
                           const float* __restrict__ b_hh, int d, float* __restrict__ wt, float* __restrict__ bias) {
  const int G = 4 * d, total = 3 * d * G;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total + G; i += gridDim.x * blockDim.x) {
    if (i < total) {
      const int k = i / G, j = i - k * G;
      wt[i] = k < 2 * d ? w_ih[(int64_t)j * 2 * d + k] : w_hh[(int64_t)j * d + (k - 2 * d)];
    } else {
      bias[i - total] = b_ih[i - total] + b_hh[i - total];
    }
  }
}

__device__ __forceinline__ void graph_range(const int32_t* graph_ptr, int64_t b, int64_t N, int64_t& n0, int64_t& n1) {
  n0 = graph_ptr[b];
  n1 = graph_ptr[b + 1];
  n0 = n0 < 0 ? 0 : (n0 > N ? N : n0);              // a malformed pointer array never indexes outside x
  n1 = n1 < n0 ? n0 : (n1 > N ? N : n1);
}

// Tape (TRAIN): in [T][B][3d] the LSTM input of step t (q, r, h of step t-1; zeros at t = 0), act [T][B][4d] the activated gates,
// cell [T][B][d], e [T][N] the attention logits, md [T][B][2] their per-graph maximum and the softmax denominator.
template <bool TRAIN>
__global__ __launch_bounds__(S2S_THREADS) void k_set2set(const float* __restrict__ x, int64_t N, int d, const int32_t* __restrict__ graph_ptr,
                                                         int64_t B, const float* __restrict__ wt, const float* __restrict__ bias, int T,
                                                         float* __restrict__ out, float* __restrict__ tape_in, float* __restrict__ tape_act,
                                                         float* __restrict__ tape_cell, float* __restrict__ tape_e,
                                                         float* __restrict__ tape_md) {
  __shared__ float s_in[3 * S2S_MAX_D];             // q | r | h
  __shared__ float s_gate[4 * S2S_MAX_D];
  __shared__ float s_c[S2S_MAX_D];
  __shared__ float s_part[S2S_WAVES][S2S_MAX_D];
  __shared__ float s_m[S2S_WAVES], s_s[S2S_WAVES];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = 4 * d;
  int64_t n0, n1;
  graph_range(graph_ptr, b, N, n0, n1);
  for (int i = tid; i < 3 * d; i += S2S_THREADS) s_in[i] = 0.0f;
  if (tid < d) s_c[tid] = 0.0f;
  __syncthreads();
  const int c0 = lane, c1 = lane + 64;
  for (int t = 0; t < T; ++t) {
    const int64_t tb = (int64_t)t * B + b;
    if (TRAIN)
      for (int i = tid; i < 3 * d; i += S2S_THREADS) tape_in[tb * 3 * d + i] = s_in[i];
    // ---- LSTM cell: 4d gate rows over the 3d inputs
    for (int j = tid; j < G; j += S2S_THREADS) {
      float acc = bias[j];
      for (int k = 0; k < 3 * d; ++k) acc = fmaf(wt[(int64_t)k * G + j], s_in[k], acc);
      s_gate[j] = acc;
    }
    __syncthreads();
    if (tid < d) {
      const float gi = sigmoid_acc(s_gate[tid]), gf = sigmoid_acc(s_gate[d + tid]);
      const float gg = tanhf(s_gate[2 * d + tid]), go = sigmoid_acc(s_gate[3 * d + tid]);
      const float c = gf * s_c[tid] + gi * gg;
      const float h = go * tanhf(c);
      s_c[tid] = c;
      s_in[tid] = h;                                 // q
      s_in[2 * d + tid] = h;                         // h
      if (TRAIN) {
        float* a = tape_act + tb * G;
        a[tid] = gi;
        a[d + tid] = gf;
        a[2 * d + tid] = gg;
        a[3 * d + tid] = go;
        tape_cell[tb * d + tid] = c;
      }
    }
    __syncthreads();
    // ---- attention readout: one pass with a running maximum per wave
    const float q0 = c0 < d ? s_in[c0] : 0.0f, q1 = c1 < d ? s_in[c1] : 0.0f;
    float m = -INFINITY, s = 0.0f, r0 = 0.0f, r1 = 0.0f;
    for (int64_t n = n0 + wave; n < n1; n += S2S_WAVES) {
      const float* xr = x + n * d;
      const float x0 = c0 < d ? xr[c0] : 0.0f, x1 = c1 < d ? xr[c1] : 0.0f;
      const float e = wave_sum(fmaf(x0, q0, x1 * q1));
      if (TRAIN && lane == 0) tape_e[(int64_t)t * N + n] = e;
      if (e > m) {
        const float sc = expf(m - e);                // (first node: exp(-inf) = 0)
        s *= sc;
        r0 *= sc;
        r1 *= sc;
        m = e;
      }
      const float p = expf(e - m);
      s += p;
      r0 = fmaf(p, x0, r0);
      r1 = fmaf(p, x1, r1);
    }
    if (lane == 0) {
      s_m[wave] = m;
      s_s[wave] = s;
    }
    if (c0 < d) s_part[wave][c0] = r0;
    if (c1 < d) s_part[wave][c1] = r1;
    __syncthreads();
    if (tid < d) {
      float M = s_m[0];
#pragma unroll
      for (int w = 1; w < S2S_WAVES; ++w) M = fmaxf(M, s_m[w]);
      float den = 0.0f, r = 0.0f;
#pragma unroll
      for (int w = 0; w < S2S_WAVES; ++w) {
        if (s_m[w] == -INFINITY) continue;           // a wave without nodes (and every wave of an empty graph)
        const float sc = expf(s_m[w] - M);
        den = fmaf(s_s[w], sc, den);
        r = fmaf(s_part[w][tid], sc, r);
      }
      den += 1e-16f;
      r = r / den;                                   // empty graph: 0 / 1e-16 = 0
      s_in[d + tid] = r;
      if (TRAIN && tid == 0) {
        tape_md[tb * 2] = M;
        tape_md[tb * 2 + 1] = den;
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < 2 * d; i += S2S_THREADS) out[b * 2 * d + i] = s_in[i];
}

// Adjoint.  Per graph, t = T-1 .. 0:  with a_n = exp(e_n - M) / den and g = d r_t:
//   d e_n = a_n (<g, x_n> - <g, r_t>)   (sum_m a_m <g, x_m> = <g, r_t>);  dx_n += a_n g + d e_n q_t;  d q_t += sum_n d e_n x_n
//   d h_t = d q_t (attention) + the carries of step t+1's input [q_t | r_t | h_t];  LSTM cell adjoint -> dgate [T][B][4d] (pre-activation);
//   carries for step t-1: d in_k = sum_j W[j][k] dgate_j   (W_ih / W_hh row-major: k is contiguous across lanes).
// dx_n is owned by one wave for all steps (the forward's node assignment): written at t = T-1, read-modify-written after.
__global__ __launch_bounds__(S2S_THREADS) void k_set2set_bwd(const float* __restrict__ x, int64_t N, int d,
                                                             const int32_t* __restrict__ graph_ptr, int64_t B,
                                                             const float* __restrict__ w_ih, const float* __restrict__ w_hh, int T,
                                                             const float* __restrict__ out, const float* __restrict__ dout,
                                                             const float* __restrict__ tape_in, const float* __restrict__ tape_act,
                                                             const float* __restrict__ tape_cell, const float* __restrict__ tape_e,
                                                             const float* __restrict__ tape_md, float* __restrict__ dx,
                                                             float* __restrict__ dgate) {
  __shared__ float s_car[3 * S2S_MAX_D];            // carries: d q | d r | d h of the current step's outputs
  __shared__ float s_dc[S2S_MAX_D];
  __shared__ float s_dg[4 * S2S_MAX_D];
  __shared__ float s_q[S2S_MAX_D], s_r[S2S_MAX_D];
  __shared__ float s_part[S2S_WAVES][S2S_MAX_D];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = 4 * d;
  int64_t n0, n1;
  graph_range(graph_ptr, b, N, n0, n1);
  for (int i = tid; i < 3 * d; i += S2S_THREADS) s_car[i] = i < 2 * d ? dout[b * 2 * d + i] : 0.0f;
  if (tid < d) s_dc[tid] = 0.0f;
  const int c0 = lane, c1 = lane + 64;
  for (int t = T - 1; t >= 0; --t) {
    const int64_t tb = (int64_t)t * B + b;
    // q_t, r_t: the next step's input, or the output after the last step
    const float* qr = t == T - 1 ? out + b * 2 * d : tape_in + (tb + B) * 3 * d;
    if (tid < d) {
      s_q[tid] = qr[tid];
      s_r[tid] = qr[d + tid];
    }
    __syncthreads();
    // ---- attention adjoint
    const float g0 = c0 < d ? s_car[d + c0] : 0.0f, g1 = c1 < d ? s_car[d + c1] : 0.0f;
    const float q0 = c0 < d ? s_q[c0] : 0.0f, q1 = c1 < d ? s_q[c1] : 0.0f;
    const float gr = wave_sum(fmaf(g0, c0 < d ? s_r[c0] : 0.0f, g1 * (c1 < d ? s_r[c1] : 0.0f)));
    const float M = tape_md[tb * 2], den = tape_md[tb * 2 + 1];
    float dq0 = 0.0f, dq1 = 0.0f;
    for (int64_t n = n0 + wave; n < n1; n += S2S_WAVES) {
      const float* xr = x + n * d;
      const float x0 = c0 < d ? xr[c0] : 0.0f, x1 = c1 < d ? xr[c1] : 0.0f;
      const float a = expf(tape_e[(int64_t)t * N + n] - M) / den;
      const float gx = wave_sum(fmaf(g0, x0, g1 * x1));
      const float de = a * (gx - gr);
      dq0 = fmaf(de, x0, dq0);
      dq1 = fmaf(de, x1, dq1);
      float* dxr = dx + n * d;
      if (c0 < d) dxr[c0] = fmaf(de, q0, a * g0) + (t == T - 1 ? 0.0f : dxr[c0]);
      if (c1 < d) dxr[c1] = fmaf(de, q1, a * g1) + (t == T - 1 ? 0.0f : dxr[c1]);
    }
    if (c0 < d) s_part[wave][c0] = dq0;
    if (c1 < d) s_part[wave][c1] = dq1;
    __syncthreads();
    // ---- LSTM cell adjoint
    if (tid < d) {
      float dh = s_car[tid] + s_car[2 * d + tid];
#pragma unroll
      for (int w = 0; w < S2S_WAVES; ++w) dh += s_part[w][tid];
      const float* a = tape_act + tb * G;
      const float gi = a[tid], gf = a[d + tid], gg = a[2 * d + tid], go = a[3 * d + tid];
      const float tc = tanhf(tape_cell[tb * d + tid]);
      const float cprev = t > 0 ? tape_cell[(tb - B) * d + tid] : 0.0f;
      const float dc = fmaf(dh * go, 1.0f - tc * tc, s_dc[tid]);
      const float di = dc * gg * gi * (1.0f - gi);
      const float df = dc * cprev * gf * (1.0f - gf);
      const float dg = dc * gi * (1.0f - gg * gg);
      const float dO = dh * tc * go * (1.0f - go);
      s_dc[tid] = dc * gf;
      s_dg[tid] = di;
      s_dg[d + tid] = df;
      s_dg[2 * d + tid] = dg;
      s_dg[3 * d + tid] = dO;
      float* o = dgate + tb * G;
      o[tid] = di;
      o[d + tid] = df;
      o[2 * d + tid] = dg;
      o[3 * d + tid] = dO;
    }
    __syncthreads();
    // ---- carries into step t-1's outputs (step 0 reads the constant zero state)
    if (t > 0) {
      for (int k = tid; k < 3 * d; k += S2S_THREADS) {
        const float* w = k < 2 * d ? w_ih + k : w_hh + (k - 2 * d);
        const int ld = k < 2 * d ? 2 * d : d;
        float acc = 0.0f;
        for (int j = 0; j < G; ++j) acc = fmaf(w[(int64_t)j * ld], s_dg[j], acc);
        s_car[k] = acc;
      }
    }
    __syncthreads();
  }
}

}  // namespace
}  // namespace sn

using namespace sn;

extern "C" int sn_set2set_f32(const float* x, int64_t N, int d, const int32_t* graph_ptr, int64_t B, const float* w_ih, const float* w_hh,
                              const float* b_ih, const float* b_hh, int T, float* out, float* work /* [12 d^2 + 4 d] */,
                              float* tape_in, float* tape_act, float* tape_cell, float* tape_e, float* tape_md, void* stream) {
  SN_REQUIRE(x && graph_ptr && w_ih && w_hh && b_ih && b_hh && out && work, "sn_set2set_f32: bad arguments");
  SN_REQUIRE(d >= 1 && d <= S2S_MAX_D, "sn_set2set_f32: d must be in [1, %d]", S2S_MAX_D);
  SN_REQUIRE(N >= 0 && B >= 0 && T >= 1 && B < (1ll << 31), "sn_set2set_f32: bad sizes");
  const int ntape = (tape_in != nullptr) + (tape_act != nullptr) + (tape_cell != nullptr) + (tape_e != nullptr) + (tape_md != nullptr);
  SN_REQUIRE(ntape == 0 || ntape == 5, "sn_set2set_f32: the tape is all five buffers or none");
  if (B == 0) return SN_OK;
  hipStream_t st = (hipStream_t)stream;
  float* wt = work;
  float* bias = work + (int64_t)12 * d * d;
  hipLaunchKernelGGL(k_s2s_pack, dim3((unsigned)cdiv((int64_t)12 * d * d + 4 * d, 256)), dim3(256), 0, st, w_ih, w_hh, b_ih, b_hh, d, wt, bias);
  SN_CHECK_LAUNCH("k_s2s_pack");
  if (ntape)
    hipLaunchKernelGGL(k_set2set<true>, dim3((unsigned)B), dim3(S2S_THREADS), 0, st, x, N, d, graph_ptr, B, (const float*)wt,
                       (const float*)bias, T, out, tape_in, tape_act, tape_cell, tape_e, tape_md);
  else
    hipLaunchKernelGGL(k_set2set<false>, dim3((unsigned)B), dim3(S2S_THREADS), 0, st, x, N, d, graph_ptr, B, (const float*)wt,
                       (const float*)bias, T, out, tape_in, tape_act, tape_cell, tape_e, tape_md);
  SN_CHECK_LAUNCH("sn_set2set_f32");
  return SN_OK;
}

extern "C" int sn_set2set_bwd_f32(const float* x, int64_t N, int d, const int32_t* graph_ptr, int64_t B, const float* w_ih,
                                  const float* w_hh, int T, const float* out, const float* dout, const float* tape_in,
                                  const float* tape_act, const float* tape_cell, const float* tape_e, const float* tape_md, float* dx,
                                  float* dgate, void* stream) {
  SN_REQUIRE(x && graph_ptr && w_ih && w_hh && out && dout && tape_in && tape_act && tape_cell && tape_e && tape_md && dx && dgate,
             "sn_set2set_bwd_f32: bad arguments");
  SN_REQUIRE(d >= 1 && d <= S2S_MAX_D, "sn_set2set_bwd_f32: d must be in [1, %d]", S2S_MAX_D);
  SN_REQUIRE(N >= 0 && B >= 0 && T >= 1 && B < (1ll << 31), "sn_set2set_bwd_f32: bad sizes");
  if (B == 0) return SN_OK;
  hipLaunchKernelGGL(k_set2set_bwd, dim3((unsigned)B), dim3(S2S_THREADS), 0, (hipStream_t)stream, x, N, d, graph_ptr, B, w_ih, w_hh, T, out,
                     dout, tape_in, tape_act, tape_cell, tape_e, tape_md, dx, dgate);
  SN_CHECK_LAUNCH("sn_set2set_bwd_f32");
  return SN_OK;
}
