// simplified_pna.hip — the message side of SimplifiedPNAConv (GINESignNetPyG/core/model_utils/pyg_gnn_wrapper.py:53-106,
// aggregators=['mean']): pre_nn = Linear(3d -> 3d) -> BatchNorm1d over the E edge rows -> ReLU -> Linear(3d -> d) on
// cat[x_i, x_j, e], mean over each node's in-edges.  Two exact rearrangements:
//   z_e = A[dst(e)] + B[src(e)] + Q[e]     the first Linear split over the concatenation: A, B are [N, C] node GEMMs, Q one [E, d] x [d, C]
//   the second Linear commutes with the mean, so what is reduced here is r[i] = mean_e relu(bn(z_e)), an [N, C] matrix, C = 3d.
// Neither cat[x_i, x_j, e] nor z is ever stored: every kernel forms z_e = (A[dst] + B[src]) + Q[e] on the fly, with the same three
// float additions in the same order, so the ReLU mask of the adjoint is the mask of the forward bit for bit.
//
// Iteration space: the destination-sorted CSR of sn_batch_plan (in-edges in edge-id order).  Lane map: a thread owns (node, V consecutive
// channels), V = 4 (one 16-byte access per row) when C, the row strides and the pointers allow, V = 1 otherwise; consecutive lanes take
// consecutive channel groups of the SAME node, so the A / B / Q rows of an edge are read as contiguous 16-byte pieces by neighbouring lanes
// (C = 384: 96 lanes = 1.5 waves per row).  One owner per output element, no atomics, every sum in a fixed order.
#include "common.hpp"

namespace sn {

namespace {

template <int V> struct Vec;
template <> struct Vec<1> {
  float v[1];
  __device__ __forceinline__ static Vec ld(const float* p) { Vec r; r.v[0] = *p; return r; }
  __device__ __forceinline__ void st(float* p) const { *p = v[0]; }
};
template <> struct Vec<4> {
  float v[4];
  __device__ __forceinline__ static Vec ld(const float* p) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    Vec r; r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w; return r;
  }
  __device__ __forceinline__ void st(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

struct Msg {                 // the operands of z_e
  const float* A; int64_t lda;
  const float* B; int64_t ldb;
  const float* Q; int64_t ldq;
  int C; int64_t N; int64_t E;
  const int32_t* rowptr; const int32_t* col; const int32_t* eperm;
  const int32_t* valid;      // masked forms: 0/1 per node, a node with 0 is left out with all its in-edges; NULL: every node counts
};

// A malformed batch is reported by the plan's own status word, and its arrays may then hold anything: the row range is clamped to the
// E slots there are, and a slot whose source node or edge id is out of range is skipped.
__device__ __forceinline__ void row_range(const int32_t* __restrict__ rowptr, int64_t n, int64_t E, int& lo, int& hi) {
  int64_t a = rowptr[n], b = rowptr[n + 1];
  a = a < 0 ? 0 : (a > E ? E : a);
  b = b < a ? a : (b > E ? E : b);
  lo = (int)a;
  hi = (int)b;
}
__device__ __forceinline__ bool slot_ok(const Msg& m, int e, int64_t& j, int64_t& eid) {
  j = m.col[e];
  eid = m.eperm[e];
  return j >= 0 && j < m.N && eid >= 0 && eid < m.E;
}

// The column-reduction launches (statistics, adjoint sums) cut the nodes into `nblk` consecutive chunks of `npb` nodes, one workgroup
// each (x) times `ny` column chunks of `gw` channel groups (y); a workgroup's 256 threads are (slot = t / gw, group = t % gw): the
// slots stride over the chunk's nodes.
struct Cut { int nblk, npb, ny, gw, slots; };

inline Cut make_cut(int64_t N, int G) {
  Cut c;
  c.ny = (int)cdiv(G, 256);
  c.gw = (int)cdiv(G, c.ny);
  c.slots = 256 / c.gw;
  int64_t want = cdiv(N > 0 ? N : 1, (int64_t)c.slots * 4);       // >= 4 nodes per slot
  if (want > 256) want = 256;                                        // one per compute unit
  c.npb = (int)cdiv(N > 0 ? N : 1, want);
  c.nblk = (int)cdiv(N > 0 ? N : 1, c.npb);
  return c;
}

// Chan's merge of (n, mean, M2) partials, in double
__device__ __forceinline__ void chan(double& n, double& mu, double& m2, double nb, double mub, double m2b) {
  if (nb <= 0.0) return;
  const double nt = n + nb, d = mub - mu;
  mu += d * (nb / nt);
  m2 += m2b + d * d * (n * nb / nt);
  n = nt;
}

// ---- statistics: per-workgroup (count, mean, M2) of z over the chunk's in-edges, per column.  part[blk][3][C].
template <int V>
__global__ __launch_bounds__(256) void k_spna_stats(Msg m, Cut cut, float* __restrict__ part) {
  __shared__ float sh[3][256 * V];
  const int t = threadIdx.x, slot = t / cut.gw, gl = t - slot * cut.gw;
  const int g = blockIdx.y * cut.gw + gl, G = m.C / V;
  const bool on = slot < cut.slots && g < G && gl < cut.gw;
  const int c = g * V;
  float cnt = 0.f, s1[V], s2[V], piv[V];
#pragma unroll
  for (int k = 0; k < V; ++k) { s1[k] = 0.f; s2[k] = 0.f; piv[k] = 0.f; }
  if (on) {
    const int64_t n0 = (int64_t)blockIdx.x * cut.npb;
    const int64_t n1 = n0 + cut.npb < m.N ? n0 + cut.npb : m.N;
    for (int64_t n = n0 + slot; n < n1; n += cut.slots) {
      int lo, hi;
      row_range(m.rowptr, n, m.E, lo, hi);
      if (lo == hi || (m.valid && !m.valid[n])) continue;
      const Vec<V> a = Vec<V>::ld(m.A + n * m.lda + c);
      for (int e = lo; e < hi; ++e) {
        int64_t j, eid;
        if (!slot_ok(m, e, j, eid)) continue;
        const Vec<V> b = Vec<V>::ld(m.B + j * m.ldb + c);
        const Vec<V> q = Vec<V>::ld(m.Q + eid * m.ldq + c);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const float z = (a.v[k] + b.v[k]) + q.v[k];
          if (cnt == 0.f) piv[k] = z;               // shifted sums around the first value seen: no cancellation in s2 - s1^2/n
          const float dz = z - piv[k];
          s1[k] += dz;
          s2[k] += dz * dz;
        }
        cnt += 1.f;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const float mu = cnt > 0.f ? s1[k] / cnt : 0.f;
    sh[0][t * V + k] = cnt;
    sh[1][t * V + k] = piv[k] + mu;
    sh[2][t * V + k] = cnt > 0.f ? fmaxf(s2[k] - s1[k] * mu, 0.f) : 0.f;
  }
  __syncthreads();
  if (on && slot == 0) {                              // slot order: fixed
#pragma unroll
    for (int k = 0; k < V; ++k) {
      double n = 0.0, mu = 0.0, m2 = 0.0;
      for (int s = 0; s < cut.slots; ++s) {
        const int u = (s * cut.gw + gl) * V + k;
        chan(n, mu, m2, sh[0][u], sh[1][u], sh[2][u]);
      }
      float* p = part + (int64_t)blockIdx.x * 3 * m.C;
      p[c + k] = (float)n;
      p[m.C + c + k] = (float)mu;
      p[2 * m.C + c + k] = (float)m2;
    }
  }
}

// merge in block order; state[0..4][C] = mean, biased variance, rstd, scale, shift; count[0] = E; running statistics (unbiased variance).
// counts != NULL (masked form): the row count of both variances and of count[0] is the device count block's counts[1].
__global__ __launch_bounds__(256) void k_spna_stats_finish(const float* __restrict__ part, int nblk, int C, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float eps, float momentum,
                                                           float* __restrict__ running_mean, float* __restrict__ running_var,
                                                           float* __restrict__ state, float* __restrict__ count,
                                                           const int32_t* __restrict__ counts) {
  // a workgroup owns 16 columns; its 16 lanes per column merge 16 consecutive ranges of the partials, then lane 0 merges the 16 range
  // results in order: the serial chain is nblk / 16 + 16 merges instead of nblk (measured at 369 partials: the chain was the launch)
  __shared__ double sh[3][16][17];
  const int cl = threadIdx.x & 15, lane = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  double n = 0.0, mu = 0.0, m2 = 0.0;
  if (c < C) {
    const int per = (nblk + 15) / 16, b0 = lane * per, b1 = b0 + per < nblk ? b0 + per : nblk;
    for (int b = b0; b < b1; ++b) {
      const float* p = part + (int64_t)b * 3 * C;
      chan(n, mu, m2, p[c], p[C + c], p[2 * C + c]);
    }
  }
  sh[0][lane][cl] = n; sh[1][lane][cl] = mu; sh[2][lane][cl] = m2;
  __syncthreads();
  if (c >= C || lane != 0) return;
  for (int l = 1; l < 16; ++l) chan(n, mu, m2, sh[0][l][cl], sh[1][l][cl], sh[2][l][cl]);
  if (counts != nullptr) n = (double)counts[1];
  const double var = n > 0.0 ? m2 / n : 0.0;
  const float rstd = 1.0f / sqrtf((float)var + eps);
  const float sc = (gamma ? gamma[c] : 1.f) * rstd;
  state[c] = (float)mu;
  state[C + c] = (float)var;
  state[2 * C + c] = rstd;
  state[3 * C + c] = sc;
  state[4 * C + c] = (beta ? beta[c] : 0.f) - (float)mu * sc;
  if (c == 0) count[0] = (float)n;
  if (running_mean != nullptr && n > 1.0) {
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mu;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)(m2 / (n - 1.0));
  }
}

// ---- mean: r[i, c] = (1 / max(deg_i, 1)) sum_{e in in(i)} relu(z_e[c] * scale[c] + shift[c])
template <int V>
__global__ __launch_bounds__(256) void k_spna_mean(Msg m, const float* __restrict__ scale, const float* __restrict__ shift,
                                                   float* __restrict__ r, int64_t ldr) {
  const int G = m.C / V;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m.N * G) return;
  const int64_t n = i / G;
  const int c = (int)(i - n * G) * V;
  int lo, hi;
  row_range(m.rowptr, n, m.E, lo, hi);
  Vec<V> acc;
#pragma unroll
  for (int k = 0; k < V; ++k) acc.v[k] = 0.f;
  if (hi > lo) {
    const Vec<V> a = Vec<V>::ld(m.A + n * m.lda + c), sc = Vec<V>::ld(scale + c), sf = Vec<V>::ld(shift + c);
    for (int e0 = lo; e0 < hi; e0 += 2) {               // two in-edges in flight
      int64_t j0, i0, j1 = 0, i1 = 0;
      const bool ok0 = slot_ok(m, e0, j0, i0);
      const bool ok1 = e0 + 1 < hi && slot_ok(m, e0 + 1, j1, i1);
      const Vec<V> b0 = Vec<V>::ld(m.B + (ok0 ? j0 : 0) * m.ldb + c);
      const Vec<V> q0 = Vec<V>::ld(m.Q + (ok0 ? i0 : 0) * m.ldq + c);
      const Vec<V> b1 = Vec<V>::ld(m.B + (ok1 ? j1 : 0) * m.ldb + c);
      const Vec<V> q1 = Vec<V>::ld(m.Q + (ok1 ? i1 : 0) * m.ldq + c);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        if (ok0) acc.v[k] += fmaxf(fmaf((a.v[k] + b0.v[k]) + q0.v[k], sc.v[k], sf.v[k]), 0.f);
        if (ok1) acc.v[k] += fmaxf(fmaf((a.v[k] + b1.v[k]) + q1.v[k], sc.v[k], sf.v[k]), 0.f);
      }
    }
    const float inv = 1.0f / (float)(hi - lo);
#pragma unroll
    for (int k = 0; k < V; ++k) acc.v[k] *= inv;
  }
  acc.st(r + n * ldr + c);
}

// ---- adjoint, pass 1 (train mode): per-workgroup column sums of g_e = dr[dst] / deg * [bn(z_e) > 0] and of g_e * xhat_e,
// xhat = (z - mean) * rstd.  sums[blk][2][C]
template <int V>
__global__ __launch_bounds__(256) void k_spna_bwd_sums(Msg m, const float* __restrict__ dr, int64_t lddr, const float* __restrict__ state,
                                                       Cut cut, float* __restrict__ sums) {
  __shared__ float sh[2][256 * V];
  const int t = threadIdx.x, slot = t / cut.gw, gl = t - slot * cut.gw;
  const int g = blockIdx.y * cut.gw + gl, G = m.C / V, C = m.C;
  const bool on = slot < cut.slots && g < G && gl < cut.gw;
  const int c = g * V;
  float s1[V], s2[V];
#pragma unroll
  for (int k = 0; k < V; ++k) { s1[k] = 0.f; s2[k] = 0.f; }
  if (on) {
    const Vec<V> mu = Vec<V>::ld(state + c), rs = Vec<V>::ld(state + 2 * C + c), sc = Vec<V>::ld(state + 3 * C + c),
                 sf = Vec<V>::ld(state + 4 * C + c);
    const int64_t n0 = (int64_t)blockIdx.x * cut.npb;
    const int64_t n1 = n0 + cut.npb < m.N ? n0 + cut.npb : m.N;
    for (int64_t n = n0 + slot; n < n1; n += cut.slots) {
      int lo, hi;
      row_range(m.rowptr, n, m.E, lo, hi);
      if (lo == hi || (m.valid && !m.valid[n])) continue;
      const Vec<V> a = Vec<V>::ld(m.A + n * m.lda + c), d = Vec<V>::ld(dr + n * lddr + c);
      const float inv = 1.0f / (float)(hi - lo);
      for (int e = lo; e < hi; ++e) {
        int64_t j, eid;
        if (!slot_ok(m, e, j, eid)) continue;
        const Vec<V> b = Vec<V>::ld(m.B + j * m.ldb + c);
        const Vec<V> q = Vec<V>::ld(m.Q + eid * m.ldq + c);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const float z = (a.v[k] + b.v[k]) + q.v[k];
          const float ge = fmaf(z, sc.v[k], sf.v[k]) > 0.f ? d.v[k] * inv : 0.f;
          s1[k] += ge;
          s2[k] += ge * ((z - mu.v[k]) * rs.v[k]);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) { sh[0][t * V + k] = s1[k]; sh[1][t * V + k] = s2[k]; }
  __syncthreads();
  if (on && slot == 0) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      double a1 = 0.0, a2 = 0.0;
      for (int s = 0; s < cut.slots; ++s) {
        const int u = (s * cut.gw + gl) * V + k;
        a1 += sh[0][u];
        a2 += sh[1][u];
      }
      float* p = sums + (int64_t)blockIdx.x * 2 * C;
      p[c + k] = (float)a1;
      p[C + c + k] = (float)a2;
    }
  }
}

// d beta = sum g, d gamma = sum g xhat (block order); coef[0..2][C] = gamma * rstd, d beta / E, d gamma / E
__global__ __launch_bounds__(256) void k_spna_bwd_finish(const float* __restrict__ sums, int nblk, int C, const float* __restrict__ state,
                                                         const float* __restrict__ gamma, int64_t E, float* __restrict__ coef,
                                                         float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                         const int32_t* __restrict__ counts) {
  __shared__ double sh[2][16][17];                       // 16 columns x 16 consecutive ranges of the partials, as k_spna_stats_finish
  const int cl = threadIdx.x & 15, lane = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  double a1 = 0.0, a2 = 0.0;
  if (c < C) {
    const int per = (nblk + 15) / 16, b0 = lane * per, b1 = b0 + per < nblk ? b0 + per : nblk;
    for (int b = b0; b < b1; ++b) {
      a1 += sums[(int64_t)b * 2 * C + c];
      a2 += sums[(int64_t)b * 2 * C + C + c];
    }
  }
  sh[0][lane][cl] = a1; sh[1][lane][cl] = a2;
  __syncthreads();
  if (c >= C || lane != 0) return;
  for (int l = 1; l < 16; ++l) { a1 += sh[0][l][cl]; a2 += sh[1][l][cl]; }
  if (counts != nullptr) E = counts[1] > 0 ? counts[1] : 1;      // (masked form: the valid edge rows, a device value)
  coef[c] = (gamma ? gamma[c] : 1.f) * state[2 * C + c];
  coef[C + c] = (float)(a1 / (double)E);
  coef[2 * C + c] = (float)(a2 / (double)E);
  if (dgamma) dgamma[c] = (float)a2;
  if (dbeta) dbeta[c] = (float)a1;
}

// ---- adjoint, pass 2: dz_e = coef_a (g_e - coef_b - xhat_e coef_c) (train) or g_e * scale (eval: state == NULL);
// dQ[e] = dz_e (edge-id rows), dA[i] = sum_{in(i)} dz_e
template <int V>
__global__ __launch_bounds__(256) void k_spna_bwd_apply(Msg m, const float* __restrict__ dr, int64_t lddr, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, const float* __restrict__ state,
                                                        const float* __restrict__ coef, float* __restrict__ dA, int64_t ldda,
                                                        float* __restrict__ dQ, int64_t lddq) {
  const int G = m.C / V, C = m.C;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m.N * G) return;
  const int64_t n = i / G;
  const int c = (int)(i - n * G) * V;
  int lo, hi;
  row_range(m.rowptr, n, m.E, lo, hi);
  Vec<V> acc;
#pragma unroll
  for (int k = 0; k < V; ++k) acc.v[k] = 0.f;
  if (m.valid && !m.valid[n]) {                         // masked form, padding node: zero dQ rows for its in-edges, a zero dA row
    for (int e = lo; e < hi; ++e) {
      int64_t j, eid;
      if (slot_ok(m, e, j, eid)) acc.st(dQ + eid * lddq + c);
    }
  } else if (hi > lo) {
    const bool train = state != nullptr;
    const Vec<V> a = Vec<V>::ld(m.A + n * m.lda + c), d = Vec<V>::ld(dr + n * lddr + c);
    const Vec<V> sc = Vec<V>::ld(scale + c), sf = Vec<V>::ld(shift + c);
    Vec<V> mu = sc, rs = sc, ca = sc, cb = sc, cc = sc;
    if (train) {
      mu = Vec<V>::ld(state + c); rs = Vec<V>::ld(state + 2 * C + c);
      ca = Vec<V>::ld(coef + c); cb = Vec<V>::ld(coef + C + c); cc = Vec<V>::ld(coef + 2 * C + c);
    }
    const float inv = 1.0f / (float)(hi - lo);
    for (int e = lo; e < hi; ++e) {
      int64_t j, eid;
      if (!slot_ok(m, e, j, eid)) continue;
      const Vec<V> b = Vec<V>::ld(m.B + j * m.ldb + c);
      const Vec<V> q = Vec<V>::ld(m.Q + eid * m.ldq + c);
      Vec<V> dz;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float z = (a.v[k] + b.v[k]) + q.v[k];
        const float ge = fmaf(z, sc.v[k], sf.v[k]) > 0.f ? d.v[k] * inv : 0.f;
        dz.v[k] = train ? ca.v[k] * ((ge - cb.v[k]) - ((z - mu.v[k]) * rs.v[k]) * cc.v[k]) : ge * sc.v[k];
        acc.v[k] += dz.v[k];
      }
      dz.st(dQ + eid * lddq + c);
    }
  }
  acc.st(dA + n * ldda + c);
}

// dB[j] = sum over j's out-edges (CSR of the flipped edge list, edge-id order) of dQ[e]
template <int V>
__global__ __launch_bounds__(256) void k_spna_rows_sum(const float* __restrict__ dQ, int64_t lddq, int C, int64_t N, int64_t E,
                                                       const int32_t* __restrict__ rowptr, const int32_t* __restrict__ eperm,
                                                       float* __restrict__ dB, int64_t lddb) {
  const int G = C / V;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N * G) return;
  const int64_t n = i / G;
  const int c = (int)(i - n * G) * V;
  Vec<V> acc;
#pragma unroll
  for (int k = 0; k < V; ++k) acc.v[k] = 0.f;
  int lo, hi;
  row_range(rowptr, n, E, lo, hi);
  for (int e = lo; e < hi; ++e) {
    const int64_t eid = eperm[e];
    if (eid < 0 || eid >= E) continue;
    const Vec<V> v = Vec<V>::ld(dQ + eid * lddq + c);
#pragma unroll
    for (int k = 0; k < V; ++k) acc.v[k] += v.v[k];
  }
  acc.st(dB + n * lddb + c);
}

inline bool a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int check_msg(const char* fn, const float* A, int64_t lda, const float* B, int64_t ldb, const float* Q, int64_t ldq, int C, int64_t N,
              int64_t E, const int32_t* rowptr, const int32_t* col, const int32_t* eperm) {
  if (!(A && B && Q && rowptr && col && eperm)) return fail(SN_ERR_ARG, "%s: null argument", fn);
  if (!(C >= 3 && C <= SN_SPNA_MAX_CHANNELS)) return fail(SN_ERR_ARG, "%s: C = %d not in [3, %d]", fn, C, SN_SPNA_MAX_CHANNELS);
  if (!(N >= 0 && E >= 0 && lda >= C && ldb >= C && ldq >= C)) return fail(SN_ERR_ARG, "%s: bad sizes or row strides", fn);
  if (!(N * (int64_t)C < ((int64_t)1 << 38))) return fail(SN_ERR_ARG, "%s: too many elements for one launch", fn);
  return SN_OK;
}

}  // namespace

}  // namespace sn

using namespace sn;

extern "C" int sn_spna_blocks(int64_t N, int C) {
  if (C < 1) C = 1;
  // (the partial buffers are sized for the scalar cut, which is never smaller than the vector one)
  const Cut a = make_cut(N, C), b = make_cut(N, (C + 3) / 4);
  return a.nblk > b.nblk ? a.nblk : b.nblk;
}

extern "C" int sn_spna_vector_path(int C, int64_t lda, int64_t ldb, int64_t ldq, int64_t ldo, const void* a, const void* b, const void* q,
                                   const void* o) {
  return (C % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && ldq % 4 == 0 && ldo % 4 == 0 && a16(a) && a16(b) && a16(q) && a16(o)) ? 1 : 0;
}

static int spna_stats(const char* fn, const float* A, int64_t lda, const float* B, int64_t ldb, const float* Q, int64_t ldq, int C, int64_t N,
                      int64_t E, const int32_t* rowptr, const int32_t* col, const int32_t* eperm, const int32_t* valid,
                      const int32_t* counts, const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                      float* running_var, float* state, float* count, float* work, void* stream) {
  int rc = check_msg(fn, A, lda, B, ldb, Q, ldq, C, N, E, rowptr, col, eperm);
  if (rc != SN_OK) return rc;
  SN_REQUIRE(state && count && work, "%s: null output", fn);
  SN_REQUIRE(E >= 2, "%s: train-mode BatchNorm needs more than one edge row (E = %lld)", fn, (long long)E);
  SN_REQUIRE(N >= 1, "%s: edges without nodes", fn);
  SN_REQUIRE((running_mean != nullptr) == (running_var != nullptr), "%s: running_mean / running_var go together", fn);
  const Msg m{A, lda, B, ldb, Q, ldq, C, N, E, rowptr, col, eperm, valid};
  hipStream_t st = (hipStream_t)stream;
  const bool vec = sn_spna_vector_path(C, lda, ldb, ldq, 4, A, B, Q, nullptr) != 0;
  const Cut cut = make_cut(N, vec ? C / 4 : C);
  if (vec) hipLaunchKernelGGL(k_spna_stats<4>, dim3((unsigned)cut.nblk, (unsigned)cut.ny), dim3(256), 0, st, m, cut, work);
  else hipLaunchKernelGGL(k_spna_stats<1>, dim3((unsigned)cut.nblk, (unsigned)cut.ny), dim3(256), 0, st, m, cut, work);
  SN_CHECK_LAUNCH(fn);
  hipLaunchKernelGGL(k_spna_stats_finish, dim3((unsigned)cdiv(C, 16)), dim3(256), 0, st, work, cut.nblk, C, gamma, beta, eps, momentum,
                     running_mean, running_var, state, count, counts);
  SN_CHECK_LAUNCH(fn);
  return SN_OK;
}

extern "C" int sn_spna_stats_f32(const float* A, int64_t lda, const float* B, int64_t ldb, const float* Q, int64_t ldq, int C, int64_t N,
                                 int64_t E, const int32_t* rowptr, const int32_t* col, const int32_t* eperm, const float* gamma,
                                 const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* state,
                                 float* count, float* work, void* stream) {
  return spna_stats("sn_spna_stats_f32", A, lda, B, ldb, Q, ldq, C, N, E, rowptr, col, eperm, nullptr, nullptr, gamma, beta, eps, momentum,
                    running_mean, running_var, state, count, work, stream);
}

extern "C" int sn_spna_stats_masked_f32(const float* A, int64_t lda, const float* B, int64_t ldb, const float* Q, int64_t ldq, int C,
                                        int64_t N, int64_t E, const int32_t* rowptr, const int32_t* col, const int32_t* eperm,
                                        const int32_t* node_valid, const int32_t* counts, const float* gamma, const float* beta, float eps,
                                        float momentum, float* running_mean, float* running_var, float* state, float* count, float* work,
                                        void* stream) {
  SN_REQUIRE(node_valid && counts, "sn_spna_stats_masked_f32: null validity vector or count block");
  return spna_stats("sn_spna_stats_masked_f32", A, lda, B, ldb, Q, ldq, C, N, E, rowptr, col, eperm, node_valid, counts, gamma, beta, eps,
                    momentum, running_mean, running_var, state, count, work, stream);
}

extern "C" int sn_spna_mean_f32(const float* A, int64_t lda, const float* B, int64_t ldb, const float* Q, int64_t ldq, int C, int64_t N,
                                int64_t E, const int32_t* rowptr, const int32_t* col, const int32_t* eperm, const float* scale,
                                const float* shift, float* r, int64_t ldr, void* stream) {
  int rc = check_msg("sn_spna_mean_f32", A, lda, B, ldb, Q, ldq, C, N, E, rowptr, col, eperm);
  if (rc != SN_OK) return rc;
  SN_REQUIRE(scale && shift && r && ldr >= C, "sn_spna_mean_f32: bad arguments");
  if (N == 0) return SN_OK;
  const Msg m{A, lda, B, ldb, Q, ldq, C, N, E, rowptr, col, eperm, nullptr};
  hipStream_t st = (hipStream_t)stream;
  const bool vec = sn_spna_vector_path(C, lda, ldb, ldq, ldr, A, B, Q, r) != 0 && a16(scale) && a16(shift);
  if (vec) hipLaunchKernelGGL(k_spna_mean<4>, dim3((unsigned)cdiv(N * (C / 4), 256)), dim3(256), 0, st, m, scale, shift, r, ldr);
  else hipLaunchKernelGGL(k_spna_mean<1>, dim3((unsigned)cdiv(N * C, 256)), dim3(256), 0, st, m, scale, shift, r, ldr);
  SN_CHECK_LAUNCH("sn_spna_mean_f32");
  return SN_OK;
}

static int spna_bwd(const char* fn, const float* A, int64_t lda, const float* B, int64_t ldb, const float* Q, int64_t ldq, int C, int64_t N,
                    int64_t E, const int32_t* rowptr, const int32_t* col, const int32_t* eperm, const int32_t* rowptr_t,
                    const int32_t* eperm_t, const int32_t* valid, const int32_t* counts, const float* dr, int64_t lddr, const float* scale,
                    const float* shift, const float* state, const float* gamma, float* dA, int64_t ldda, float* dB, int64_t lddb, float* dQ,
                    int64_t lddq, float* dgamma, float* dbeta, float* work, void* stream) {
  int rc = check_msg(fn, A, lda, B, ldb, Q, ldq, C, N, E, rowptr, col, eperm);
  if (rc != SN_OK) return rc;
  SN_REQUIRE(rowptr_t && eperm_t && dr && dA && dB && dQ && lddr >= C && ldda >= C && lddb >= C && lddq >= C, "%s: bad arguments", fn);
  SN_REQUIRE(state || (scale && shift), "%s: eval mode needs scale / shift", fn);
  SN_REQUIRE(!state || (work && E >= 2), "%s: train mode needs the work buffer and more than one edge row", fn);
  if (N == 0) return SN_OK;
  const Msg m{A, lda, B, ldb, Q, ldq, C, N, E, rowptr, col, eperm, valid};
  hipStream_t st = (hipStream_t)stream;
  if (state) { scale = state + 3 * (int64_t)C; shift = state + 4 * (int64_t)C; }
  const bool vec = sn_spna_vector_path(C, lda, ldb, ldq, lddr, A, B, Q, dr) != 0 && sn_spna_vector_path(C, ldda, lddb, lddq, 4, dA, dB, dQ, nullptr) != 0 &&
                   a16(scale) && a16(shift) && (!state || (a16(state) && a16(work)));
  float* coef = nullptr;
  if (state) {
    const Cut cut = make_cut(N, vec ? C / 4 : C);
    coef = work + (int64_t)sn_spna_blocks(N, C) * 2 * C;          // (a multiple of 4 floats when C is)
    if (vec) hipLaunchKernelGGL(k_spna_bwd_sums<4>, dim3((unsigned)cut.nblk, (unsigned)cut.ny), dim3(256), 0, st, m, dr, lddr, state, cut, work);
    else hipLaunchKernelGGL(k_spna_bwd_sums<1>, dim3((unsigned)cut.nblk, (unsigned)cut.ny), dim3(256), 0, st, m, dr, lddr, state, cut, work);
    SN_CHECK_LAUNCH(fn);
    hipLaunchKernelGGL(k_spna_bwd_finish, dim3((unsigned)cdiv(C, 16)), dim3(256), 0, st, work, cut.nblk, C, state, gamma, E, coef, dgamma, dbeta,
                       counts);
    SN_CHECK_LAUNCH(fn);
  }
  if (vec) {
    hipLaunchKernelGGL(k_spna_bwd_apply<4>, dim3((unsigned)cdiv(N * (C / 4), 256)), dim3(256), 0, st, m, dr, lddr, scale, shift, state, coef, dA,
                       ldda, dQ, lddq);
    hipLaunchKernelGGL(k_spna_rows_sum<4>, dim3((unsigned)cdiv(N * (C / 4), 256)), dim3(256), 0, st, dQ, lddq, C, N, E, rowptr_t, eperm_t, dB, lddb);
  } else {
    hipLaunchKernelGGL(k_spna_bwd_apply<1>, dim3((unsigned)cdiv(N * C, 256)), dim3(256), 0, st, m, dr, lddr, scale, shift, state, coef, dA, ldda,
                       dQ, lddq);
    hipLaunchKernelGGL(k_spna_rows_sum<1>, dim3((unsigned)cdiv(N * C, 256)), dim3(256), 0, st, dQ, lddq, C, N, E, rowptr_t, eperm_t, dB, lddb);
  }
  SN_CHECK_LAUNCH(fn);
  return SN_OK;
}

extern "C" int sn_spna_bwd_f32(const float* A, int64_t lda, const float* B, int64_t ldb, const float* Q, int64_t ldq, int C, int64_t N,
                               int64_t E, const int32_t* rowptr, const int32_t* col, const int32_t* eperm, const int32_t* rowptr_t,
                               const int32_t* eperm_t, const float* dr, int64_t lddr, const float* scale, const float* shift,
                               const float* state, const float* gamma, float* dA, int64_t ldda, float* dB, int64_t lddb, float* dQ,
                               int64_t lddq, float* dgamma, float* dbeta, float* work, void* stream) {
  return spna_bwd("sn_spna_bwd_f32", A, lda, B, ldb, Q, ldq, C, N, E, rowptr, col, eperm, rowptr_t, eperm_t, nullptr, nullptr, dr, lddr, scale,
                  shift, state, gamma, dA, ldda, dB, lddb, dQ, lddq, dgamma, dbeta, work, stream);
}

extern "C" int sn_spna_bwd_masked_f32(const float* A, int64_t lda, const float* B, int64_t ldb, const float* Q, int64_t ldq, int C, int64_t N,
                                      int64_t E, const int32_t* rowptr, const int32_t* col, const int32_t* eperm, const int32_t* rowptr_t,
                                      const int32_t* eperm_t, const int32_t* node_valid, const int32_t* counts, const float* dr,
                                      int64_t lddr, const float* state, const float* gamma, float* dA, int64_t ldda, float* dB,
                                      int64_t lddb, float* dQ, int64_t lddq, float* dgamma, float* dbeta, float* work, void* stream) {
  SN_REQUIRE(node_valid && counts && state, "sn_spna_bwd_masked_f32: null validity vector, count block or state (train mode only)");
  return spna_bwd("sn_spna_bwd_masked_f32", A, lda, B, ldb, Q, ldq, C, N, E, rowptr, col, eperm, rowptr_t, eperm_t, node_valid, counts, dr,
                  lddr, nullptr, nullptr, state, gamma, dA, ldda, dB, lddb, dQ, lddq, dgamma, dbeta, work, stream);
}
