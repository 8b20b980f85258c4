// full_attention.hip — the graph Transformer's full-graph attention (GraphPrediction/layers/transformer.py:155-228 with full_graph
// True) and the device form of data/molecules.py:211-235 `make_full_graph`.
//
// Every node attends to every other node of its molecule.  A pair that is a bond ("real", r = 1) is scored through Q / K / E, every
// other pair ("fake", r = 0) through Q_2 / K_2 / E_2, and the two kinds are mixed by L = clamp(gamma, 0, 1):
//   t   = sum_c ((A[j,h,c] * B[i,h,c]) / sqrt(dk)) * T[cls,h,c]        r = 1: A, B, T = K, Q, T_real;  r = 0: K_2, Q_2, T_fake
//   s   = exp(clamp(t, -5, 5)) / (L + 1)  (real),   (L * exp(clamp(t, -5, 5))) / (L + 1)  (fake)
//   out[i,h,:] = sum_e s * V[j,h,:] / (sum_e s + 1e-6)
// E and E_2 have no bias, so E(embedding_e(e))[edge] = (E(embedding_e.weight))[e[edge]]: the kernels read one int32 code
// (2 * class + real) per edge and a [C, heads*dk] class table per kind — no [E_full, heads*dk] matrix exists, forward or backward.
// The iteration space is the destination-sorted CSR of sn_batch_plan (in-edges in edge-id order, the order DGL's reduce sees them):
// no atomics in any sum, one owner per output element, repeated calls are bit-identical.  One thread per (node, head), the head
// width padded to a compile-time bound (4 / 8 / 16 / 32) so that the per-thread rows stay in registers.
#include "common.hpp"

namespace sn {

constexpr int FA_MAX_CLASSES = 16;
constexpr int FA_TAB_THREADS = 256;     // the table-gradient kernel's workgroup: (sub-chunk, column) pairs
constexpr int FA_TAB_BLOCKS = 1024;     // at most this many partial tables

// the weight of an edge's exp: the reference's operations in its order (exp_real / exp_fake, transformer.py:35-46)
__device__ __forceinline__ float fa_weight(float ex, bool real, float L) { return real ? ex / (L + 1.0f) : (L * ex) / (L + 1.0f); }

template <int DKP>
__global__ __launch_bounds__(256) void k_full_attention(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                        const float* __restrict__ Q2, const float* __restrict__ K2, int64_t ld,
                                                        const float* __restrict__ Tr, const float* __restrict__ Tf, int C,
                                                        const int32_t* __restrict__ codes, const float* __restrict__ gamma, int64_t N, int H,
                                                        int dk, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                        const int32_t* __restrict__ eperm, float* __restrict__ out, float* __restrict__ den,
                                                        int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N * H) return;
  const int64_t n = i / H;
  const int h = (int)(i - n * H);
  const int d = H * dk;
  const float root = sqrtf((float)dk);
  const float L = fminf(fmaxf(gamma[0], 0.f), 1.f);
  float q[DKP], q2[DKP], acc[DKP];
#pragma unroll
  for (int c = 0; c < DKP; ++c) {
    q[c] = c < dk ? Q[n * ld + h * dk + c] : 0.f;
    q2[c] = c < dk ? Q2[n * ld + h * dk + c] : 0.f;
    acc[c] = 0.f;
  }
  float z = 0.f;
  bool bad = false;
  for (int e = rowptr[n]; e < rowptr[n + 1]; ++e) {
    const int64_t j = col[e];
    const int code = codes[eperm[e]];
    const int cls = code >> 1;
    const bool real = code & 1;
    if (cls < 0 || cls >= C) { bad = true; continue; }             // never dereferenced: the edge contributes nothing
    const float* kr = (real ? K : K2) + j * ld + h * dk;
    const float* tr = (real ? Tr : Tf) + (int64_t)cls * d + h * dk;
    const float* vr = V + j * ld + h * dk;
    float sc = 0.f;
#pragma unroll
    for (int c = 0; c < DKP; ++c)
      if (c < dk) sc += ((kr[c] * (real ? q[c] : q2[c])) / root) * tr[c];     // src_dot_dst, scaling, imp_exp_attn — in the reference's order
    const float s = fa_weight(expf(fminf(fmaxf(sc, -5.f), 5.f)), real, L);
    z += s;
#pragma unroll
    for (int c = 0; c < DKP; ++c)
      if (c < dk) acc[c] += vr[c] * s;
  }
  den[i] = z;
#pragma unroll
  for (int c = 0; c < DKP; ++c)
    if (c < dk) out[n * d + h * dk + c] = acc[c] / (z + 1e-6f);
  if (bad && status != nullptr) atomicOr(status, 1);
}

// Adjoint, destination side: dQ, dQ_2 [N, H*dk], the per-(edge, head) scalars the other passes need — wv = s / Z and dsc = dt — and
// this workgroup's share of dL = sum_e ds * exp(clamp t) * (-/+ 1 / (L + 1)^2), summed in thread order in float64.
template <int DKP>
__global__ __launch_bounds__(256) void k_full_attention_bwd_dst(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                                const float* __restrict__ Q2, const float* __restrict__ K2, int64_t ld,
                                                                const float* __restrict__ Tr, const float* __restrict__ Tf, int C,
                                                                const int32_t* __restrict__ codes, const float* __restrict__ gamma,
                                                                const float* __restrict__ out, const float* __restrict__ den,
                                                                const float* __restrict__ dout, int64_t N, int H, int dk,
                                                                const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                const int32_t* __restrict__ eperm, float* __restrict__ dQ,
                                                                float* __restrict__ dQ2, float* __restrict__ wv, float* __restrict__ dsc,
                                                                double* __restrict__ gpart) {
  __shared__ double red[256];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float dl = 0.f;
  if (i < N * H) {
    const int64_t n = i / H;
    const int h = (int)(i - n * H);
    const int d = H * dk;
    const float root = sqrtf((float)dk);
    const float L = fminf(fmaxf(gamma[0], 0.f), 1.f);
    const float dw = 1.0f / ((L + 1.0f) * (L + 1.0f));
    float q[DKP], q2[DKP], go[DKP], aq[DKP], aq2[DKP];
    float gdo = 0.f;
#pragma unroll
    for (int c = 0; c < DKP; ++c) {
      const bool ok = c < dk;
      q[c] = ok ? Q[n * ld + h * dk + c] : 0.f;
      q2[c] = ok ? Q2[n * ld + h * dk + c] : 0.f;
      go[c] = ok ? dout[n * d + h * dk + c] : 0.f;
      gdo += ok ? go[c] * out[n * d + h * dk + c] : 0.f;
      aq[c] = 0.f;
      aq2[c] = 0.f;
    }
    const float r = 1.0f / (den[i] + 1e-6f);
    for (int e = rowptr[n]; e < rowptr[n + 1]; ++e) {
      const int64_t j = col[e], eid = eperm[e];
      const int code = codes[eid];
      const int cls = code >> 1;
      const bool real = code & 1;
      if (cls < 0 || cls >= C) {
        wv[eid * H + h] = 0.f;
        dsc[eid * H + h] = 0.f;
        continue;
      }
      const float* kr = (real ? K : K2) + j * ld + h * dk;
      const float* tr = (real ? Tr : Tf) + (int64_t)cls * d + h * dk;
      const float* vr = V + j * ld + h * dk;
      float sc = 0.f, gv = 0.f;
#pragma unroll
      for (int c = 0; c < DKP; ++c)
        if (c < dk) { sc += ((kr[c] * (real ? q[c] : q2[c])) / root) * tr[c]; gv += go[c] * vr[c]; }
      const bool inside = sc > -5.f && sc < 5.f;
      const float ex = expf(fminf(fmaxf(sc, -5.f), 5.f));
      const float s = fa_weight(ex, real, L);
      const float ds = r * (gv - gdo);                              // d s_e
      const float dscore = inside ? ds * s : 0.f;
      dl += ds * ex * (real ? -dw : dw);
      wv[eid * H + h] = s * r;
      dsc[eid * H + h] = dscore;
#pragma unroll
      for (int c = 0; c < DKP; ++c)
        if (c < dk) {
          const float v = dscore * (kr[c] / root) * tr[c];
          if (real) aq[c] += v; else aq2[c] += v;
        }
    }
#pragma unroll
    for (int c = 0; c < DKP; ++c)
      if (c < dk) { dQ[n * d + h * dk + c] = aq[c]; dQ2[n * d + h * dk + c] = aq2[c]; }
  }
  red[threadIdx.x] = (double)dl;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {           // a fixed tree: the same order on every call
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) gpart[blockIdx.x] = red[0];
}

// Source side over the reverse CSR (rcol = destination node, rperm = edge id): dK[j] / dK_2[j] = sum_out dsc * (B[dst] / sqrt(dk)) * T[cls],
// dV[j] = sum_out wv * dout[dst]
template <int DKP>
__global__ __launch_bounds__(256) void k_full_attention_bwd_src(const float* __restrict__ Q, const float* __restrict__ Q2, int64_t ld,
                                                                const float* __restrict__ Tr, const float* __restrict__ Tf, int C,
                                                                const int32_t* __restrict__ codes, const float* __restrict__ dout,
                                                                const float* __restrict__ wv, const float* __restrict__ dsc, int64_t N, int H,
                                                                int dk, const int32_t* __restrict__ rrow, const int32_t* __restrict__ rcol,
                                                                const int32_t* __restrict__ rperm, float* __restrict__ dK,
                                                                float* __restrict__ dK2, float* __restrict__ dV) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N * H) return;
  const int64_t n = i / H;
  const int h = (int)(i - n * H);
  const int d = H * dk;
  const float root = sqrtf((float)dk);
  float ak[DKP], ak2[DKP], av[DKP];
#pragma unroll
  for (int c = 0; c < DKP; ++c) { ak[c] = 0.f; ak2[c] = 0.f; av[c] = 0.f; }
  for (int e = rrow[n]; e < rrow[n + 1]; ++e) {
    const int64_t t = rcol[e], eid = rperm[e];
    const int code = codes[eid];
    const int cls = code >> 1;
    const bool real = code & 1;
    if (cls < 0 || cls >= C) continue;
    const float w = wv[eid * H + h], ds = dsc[eid * H + h];
    const float* qr = (real ? Q : Q2) + t * ld + h * dk;
    const float* tr = (real ? Tr : Tf) + (int64_t)cls * d + h * dk;
    const float* gr = dout + t * d + h * dk;
#pragma unroll
    for (int c = 0; c < DKP; ++c)
      if (c < dk) {
        const float v = ds * (qr[c] / root) * tr[c];
        if (real) ak[c] += v; else ak2[c] += v;
        av[c] += w * gr[c];
      }
  }
#pragma unroll
  for (int c = 0; c < DKP; ++c)
    if (c < dk) { dK[n * d + h * dk + c] = ak[c]; dK2[n * d + h * dk + c] = ak2[c]; dV[n * d + h * dk + c] = av[c]; }
}

// Table gradients, partial sums: dT[code][h,c] = sum over the edges with that code of dsc[e,h] * (A[j,h,c] * B[i,h,c]) / sqrt(dk).
// A workgroup owns a run of `per` destination nodes and a tile of W = min(H*dk, 256) columns at a time; thread (sub, col) walks the
// nodes sub, sub + nsub, ... of the run and adds into ITS OWN LDS cell [sub][code][col] — no two threads share a cell, so there is
// no atomic and the order of every sum is fixed; the nsub cells of a (code, col) are then added in sub order into part[block].
__global__ __launch_bounds__(FA_TAB_THREADS) void k_full_attention_bwd_tab(const float* __restrict__ Q, const float* __restrict__ K,
                                                                           const float* __restrict__ Q2, const float* __restrict__ K2,
                                                                           int64_t ld, int C, const int32_t* __restrict__ codes,
                                                                           const float* __restrict__ dsc, int64_t N, int64_t per, int H, int dk,
                                                                           const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                           const int32_t* __restrict__ eperm, float* __restrict__ part) {
  __shared__ float cell[2 * FA_MAX_CLASSES * FA_TAB_THREADS];
  const int d = H * dk;
  const int W = d < FA_TAB_THREADS ? d : FA_TAB_THREADS;
  const int nsub = FA_TAB_THREADS / W;
  const int sub = (int)threadIdx.x / W, cw = (int)threadIdx.x - sub * W;
  const bool live = sub < nsub;
  const int ncode = 2 * C;
  const float root = sqrtf((float)dk);
  const int64_t n0 = (int64_t)blockIdx.x * per;
  const int64_t n1 = n0 + per < N ? n0 + per : N;
  float* mine = cell + ((int64_t)sub * ncode) * W + cw;              // [sub][code][cw]
  float* dst = part + (int64_t)blockIdx.x * ncode * d;
  for (int c0 = 0; c0 < d; c0 += W) {
    const int cc = c0 + cw;
    const bool on = live && cc < d;
    if (live)
      for (int k = 0; k < ncode; ++k) mine[k * W] = 0.f;
    if (on) {
      const int h = cc / dk;
      for (int64_t n = n0 + sub; n < n1; n += nsub) {
        const float qv = Q[n * ld + cc], qv2 = Q2[n * ld + cc];
        for (int e = rowptr[n]; e < rowptr[n + 1]; ++e) {
          const int64_t j = col[e], eid = eperm[e];
          const int code = codes[eid];
          if (code < 0 || code >= ncode) continue;
          const bool real = code & 1;
          const float a = (real ? K : K2)[j * ld + cc];
          mine[code * W] += dsc[eid * H + h] * ((a * (real ? qv : qv2)) / root);
        }
      }
    }
    __syncthreads();
    for (int o = (int)threadIdx.x; o < ncode * W; o += FA_TAB_THREADS) {
      const int k = o / W, w = o - k * W;
      if (c0 + w < d) {
        float s = 0.f;
        for (int u = 0; u < nsub; ++u) s += cell[((int64_t)u * ncode + k) * W + w];
        dst[(int64_t)k * d + c0 + w] = s;
      }
    }
    __syncthreads();
  }
}

// The deterministic finish: dT_real / dT_fake [C, H*dk] = the partial tables added in workgroup order; dgamma = the destination
// pass's float64 partials added in workgroup order, passed where torch.clamp passes its gradient (0 <= gamma <= 1).
__global__ __launch_bounds__(256) void k_full_attention_bwd_finish(const float* __restrict__ part, int nblk, int C, int d,
                                                                   const double* __restrict__ gpart, int ngp, const float* __restrict__ gamma,
                                                                   float* __restrict__ dTr, float* __restrict__ dTf, float* __restrict__ dgamma) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t tot = (int64_t)2 * C * d;
  if (o < tot) {
    float s = 0.f;
    for (int b = 0; b < nblk; ++b) s += part[(int64_t)b * tot + o];
    const int64_t code = o / d, c = o - code * d;
    ((code & 1) ? dTr : dTf)[(code >> 1) * d + c] = s;
  }
  if (o == 0) {
    double s = 0.0;
    for (int b = 0; b < ngp; ++b) s += gpart[b];
    const float g = gamma[0];
    dgamma[0] = (g >= 0.f && g <= 1.f) ? (float)s : 0.f;
  }
}

// data/molecules.py:211-235 for a whole batch: one workgroup per graph.  The graph's pairs are numbered u-major, v ascending, v != u
// (networkx.complete_graph(n).to_directed().edges()); the pair (u -> v) is real when the sparse graph has that edge — looked up in
// v's in-edge range of the plan — and then keeps its class; any other pair gets real = 0, class 0.  A self loop or a repeated (u, v)
// has no defined meaning in the reference's assignment: status bit 0 / bit 1.
__global__ __launch_bounds__(256) void k_make_full_graph(const int32_t* __restrict__ graph_ptr, int64_t B, int64_t N,
                                                         const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                         const int32_t* __restrict__ eperm, const int64_t* __restrict__ e, int64_t E_full,
                                                         int64_t* __restrict__ src, int64_t* __restrict__ dst, int64_t* __restrict__ real,
                                                         int64_t* __restrict__ efull, int32_t* __restrict__ status) {
  __shared__ long long red[256];
  const int64_t b = blockIdx.x;
  long long mine = 0;
  for (int64_t g = threadIdx.x; g < b; g += 256) {
    const long long n = graph_ptr[g + 1] - graph_ptr[g];
    mine += n > 0 ? n * (n - 1) : 0;
  }
  red[threadIdx.x] = mine;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  const int64_t off = red[0];
  const int64_t base = graph_ptr[b];
  const int64_t n = (int64_t)graph_ptr[b + 1] - base;
  if (n <= 0 || base < 0 || base + n > N) return;
  int flag = 0;
  for (int64_t t = threadIdx.x; t < n * n; t += 256) {
    const int64_t u = t / n, v = t - u * n;
    const int32_t gu = (int32_t)(base + u);
    int hits = 0;
    int64_t cls = 0;
    for (int p = rowptr[base + v]; p < rowptr[base + v + 1]; ++p)
      if (col[p] == gu) {
        if (hits == 0) cls = e[eperm[p]];
        ++hits;
      }
    if (u == v) {
      if (hits) flag |= 1;
      continue;
    }
    if (hits > 1) flag |= 2;
    const int64_t o = off + u * (n - 1) + (v > u ? v - 1 : v);
    if (o >= E_full) { flag |= 4; continue; }          // the caller's size does not fit the node counts: nothing is written past it
    src[o] = base + u;
    dst[o] = base + v;
    real[o] = hits ? 1 : 0;
    efull[o] = hits ? cls : 0;
  }
  if (flag) atomicOr(status, flag);
}

template <int DKP>
static void fa_launch_fwd(hipStream_t st, dim3 grid, const float* Q, const float* K, const float* V, const float* Q2, const float* K2, int64_t ld,
                          const float* Tr, const float* Tf, int C, const int32_t* codes, const float* gamma, int64_t N, int H, int dk,
                          const int32_t* rowptr, const int32_t* col, const int32_t* eperm, float* out, float* den, int32_t* status) {
  hipLaunchKernelGGL(k_full_attention<DKP>, grid, dim3(256), 0, st, Q, K, V, Q2, K2, ld, Tr, Tf, C, codes, gamma, N, H, dk, rowptr, col, eperm,
                     out, den, status);
}

template <int DKP>
static void fa_launch_bwd(hipStream_t st, dim3 grid, const float* Q, const float* K, const float* V, const float* Q2, const float* K2, int64_t ld,
                          const float* Tr, const float* Tf, int C, const int32_t* codes, const float* gamma, const float* out, const float* den,
                          const float* dout, int64_t N, int H, int dk, const int32_t* rowptr, const int32_t* col, const int32_t* eperm,
                          const int32_t* rrow, const int32_t* rcol, const int32_t* rperm, float* dQ, float* dK, float* dV, float* dQ2,
                          float* dK2, float* wv, float* dsc, double* gpart) {
  hipLaunchKernelGGL(k_full_attention_bwd_dst<DKP>, grid, dim3(256), 0, st, Q, K, V, Q2, K2, ld, Tr, Tf, C, codes, gamma, out, den, dout, N, H, dk,
                     rowptr, col, eperm, dQ, dQ2, wv, dsc, gpart);
  hipLaunchKernelGGL(k_full_attention_bwd_src<DKP>, grid, dim3(256), 0, st, Q, Q2, ld, Tr, Tf, C, codes, dout, (const float*)wv, (const float*)dsc,
                     N, H, dk, rrow, rcol, rperm, dK, dK2, dV);
}

static int64_t fa_tab_blocks(int64_t N) {
  const int64_t b = cdiv(N, 16);
  return b < 1 ? 1 : (b > FA_TAB_BLOCKS ? FA_TAB_BLOCKS : b);
}

}  // namespace sn

using namespace sn;

#define FA_DISPATCH(dk, call)            \
  do {                                   \
    if ((dk) <= 4) { call(4); }          \
    else if ((dk) <= 8) { call(8); }     \
    else if ((dk) <= 16) { call(16); }   \
    else { call(32); }                   \
  } while (0)

extern "C" int sn_full_attention_f32(const float* Q, const float* K, const float* V, const float* Q2, const float* K2, int64_t ld,
                                     const float* T_real, const float* T_fake, int C, const int32_t* codes, const float* gamma, int64_t N,
                                     int heads, int dk, const int32_t* rowptr, const int32_t* col, const int32_t* eperm, float* out, float* den,
                                     int32_t* status, void* stream) {
  SN_REQUIRE(Q && K && V && Q2 && K2 && T_real && T_fake && codes && gamma && rowptr && col && eperm && out && den && N >= 0 && heads > 0,
             "sn_full_attention_f32: bad arguments");
  SN_REQUIRE(dk >= 1 && dk <= 32, "sn_full_attention_f32: head width %d not in [1, 32]", dk);
  SN_REQUIRE(C >= 1 && C <= FA_MAX_CLASSES, "sn_full_attention_f32: %d edge classes not in [1, %d]", C, FA_MAX_CLASSES);
  SN_REQUIRE(ld >= (int64_t)heads * dk, "sn_full_attention_f32: row stride shorter than heads * dk");
  if (N == 0) return SN_OK;
  const dim3 grid((unsigned)cdiv(N * heads, 256));
  hipStream_t st = (hipStream_t)stream;
#define FA_FWD(P) fa_launch_fwd<P>(st, grid, Q, K, V, Q2, K2, ld, T_real, T_fake, C, codes, gamma, N, heads, dk, rowptr, col, eperm, out, den, status)
  FA_DISPATCH(dk, FA_FWD);
#undef FA_FWD
  SN_CHECK_LAUNCH("sn_full_attention_f32");
  return SN_OK;
}

extern "C" int64_t sn_full_attention_bwd_scratch_floats(int64_t N, int64_t E, int heads, int dk, int C) {
  if (N < 0 || E < 0 || heads <= 0 || dk <= 0 || C <= 0) return 0;
  const int64_t gp = 2 * cdiv(N * heads, 256) + 2;                       // float64 partials of dgamma, counted in floats
  return 2 * E * heads + fa_tab_blocks(N) * 2 * C * heads * dk + gp;
}

extern "C" int sn_full_attention_bwd_f32(const float* Q, const float* K, const float* V, const float* Q2, const float* K2, int64_t ld,
                                         const float* T_real, const float* T_fake, int C, const int32_t* codes, const float* gamma,
                                         const float* out, const float* den, const float* dout, int64_t N, int64_t E, int heads, int dk,
                                         const int32_t* rowptr, const int32_t* col, const int32_t* eperm, const int32_t* rev_rowptr,
                                         const int32_t* rev_col, const int32_t* rev_eperm, float* dQ, float* dK, float* dV, float* dQ2,
                                         float* dK2, float* dT_real, float* dT_fake, float* dgamma, float* scratch, void* stream) {
  SN_REQUIRE(Q && K && V && Q2 && K2 && T_real && T_fake && gamma && out && den && dout && rowptr && rev_rowptr && dQ && dK && dV && dQ2 &&
                 dK2 && dT_real && dT_fake && dgamma && scratch && N >= 0 && E >= 0 && heads > 0,
             "sn_full_attention_bwd_f32: bad arguments");
  SN_REQUIRE(dk >= 1 && dk <= 32, "sn_full_attention_bwd_f32: head width %d not in [1, 32]", dk);
  SN_REQUIRE(C >= 1 && C <= FA_MAX_CLASSES, "sn_full_attention_bwd_f32: %d edge classes not in [1, %d]", C, FA_MAX_CLASSES);
  SN_REQUIRE(ld >= (int64_t)heads * dk, "sn_full_attention_bwd_f32: row stride shorter than heads * dk");
  SN_REQUIRE(E == 0 || (codes && col && eperm && rev_col && rev_eperm), "sn_full_attention_bwd_f32: null edge arrays");
  SN_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, "sn_full_attention_bwd_f32: scratch must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int d = heads * dk;
  const int64_t nb = cdiv(N * heads, 256);
  const int64_t tb = N > 0 ? fa_tab_blocks(N) : 0;
  // scratch: [float64 dgamma partials (nb, padded to an even float count + 2) | wv [E, heads] | dsc [E, heads] | partial tables]
  double* gpart = reinterpret_cast<double*>(scratch);
  float* wv = scratch + 2 * nb + 2;
  float* dsc = wv + E * heads;
  float* part = dsc + E * heads;
  if (N > 0) {
    const dim3 grid((unsigned)nb);
#define FA_BWD(P)                                                                                                                              \
  fa_launch_bwd<P>(st, grid, Q, K, V, Q2, K2, ld, T_real, T_fake, C, codes, gamma, out, den, dout, N, heads, dk, rowptr, col, eperm, rev_rowptr, \
                   rev_col, rev_eperm, dQ, dK, dV, dQ2, dK2, wv, dsc, gpart)
    FA_DISPATCH(dk, FA_BWD);
#undef FA_BWD
    hipLaunchKernelGGL(k_full_attention_bwd_tab, dim3((unsigned)tb), dim3(FA_TAB_THREADS), 0, st, Q, K, Q2, K2, ld, C, codes, (const float*)dsc, N,
                       cdiv(N, tb), heads, dk, rowptr, col, eperm, part);
  }
  hipLaunchKernelGGL(k_full_attention_bwd_finish, dim3((unsigned)cdiv((int64_t)2 * C * d, 256)), dim3(256), 0, st, (const float*)part, (int)tb, C, d,
                     (const double*)gpart, (int)nb, gamma, dT_real, dT_fake, dgamma);
  SN_CHECK_LAUNCH("sn_full_attention_bwd_f32");
  return SN_OK;
}

extern "C" int sn_make_full_graph(const int32_t* graph_ptr, int64_t B, int64_t N, const int32_t* rowptr, const int32_t* col,
                                  const int32_t* eperm, const int64_t* e, int64_t E, int64_t E_full, int64_t* src, int64_t* dst,
                                  int64_t* real, int64_t* e_full, int32_t* status, void* stream) {
  SN_REQUIRE(graph_ptr && rowptr && status && B >= 0 && N >= 0 && E >= 0 && E_full >= 0, "sn_make_full_graph: bad arguments");
  SN_REQUIRE(E == 0 || (col && eperm && e), "sn_make_full_graph: null edge arrays");
  SN_REQUIRE(E_full == 0 || (src && dst && real && e_full), "sn_make_full_graph: null output arrays");
  if (B == 0) return SN_OK;
  hipLaunchKernelGGL(k_make_full_graph, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, graph_ptr, B, N, rowptr, col, eperm, e, E_full, src,
                     dst, real, e_full, status);
  SN_CHECK_LAUNCH("sn_make_full_graph");
  return SN_OK;
}
