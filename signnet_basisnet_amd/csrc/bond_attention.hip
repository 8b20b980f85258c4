// bond_attention.hip — full-graph attention of the graph Transformer computed directly from the molecular (bond) graph: what
// sn_full_attention_f32 computes on the output of sn_make_full_graph (full_attention.hip), without the edge list of sum n (n - 1) pairs.
//
// The complete graph of a molecule is its node range graph_ptr[g] .. graph_ptr[g + 1]; the pair (j -> i) is real exactly when j -> i is a
// bond (an in-edge of i in the plan's destination-sorted CSR) and then has the bond's class e[edge]; every other pair is class 0 of the
// fake table.  Per pair, in the reference's order of operations:
//   t = sum_c ((A[j,h,c] * B[i,h,c]) / sqrt(dk)) * T[h,c]          real: A, B, T = K, Q, T_real[class];  fake: K_2, Q_2, T_fake[0]
//   s = exp(clamp(t, -5, 5)) / (L + 1)  (real),  (L * exp(clamp(t, -5, 5))) / (L + 1)  (fake),  L = clamp(gamma, 0, 1)
//   out[i,h,:] = sum_{j != i} s * V[j,h,:] / (sum s + 1e-6)
//
// One workgroup per (graph, head).  The head's K | K_2 | V columns of the graph's rows (the adjoint: also Q | Q_2 | dout and two
// per-node scalars) and an n x n byte table of pair codes (0 fake, 1 + class real, 0x7f a class outside the table) are staged in LDS
// once; whether a graph fits is decided in the kernel from graph_ptr (ba_lds_bytes), and a graph that does not fit takes the
// global-memory instantiation of the SAME body: rows read in place, the pair code found by scanning i's in-edges.  Floating-point
// contraction is off in this file, so both instantiations round every operation alike and a graph's result does not depend on the
// path, on the other graphs of the batch or on padding.
//
// The adjoint re-scores: a destination pass (wave 0, thread = destination i: dQ, dQ_2, dgamma's share, and i's share of the
// class-table gradients into its OWN scratch rows) beside a source pass (wave 1, thread = source j: dK, dK_2, dV), then a per-graph sum
// of the scratch rows in node order.  A finish launch adds the per-graph tables and the float64 per-(graph, head) dgamma partials.  No
// atomics in any sum, one owner per output element; nothing of size sum n^2 is allocated.
#include "common.hpp"

#pragma clang fp contract(off)

namespace sn {

constexpr int BA_MAX_CLASSES = 16;
constexpr int BA_THREADS = 128;          // two waves (the adjoint gives each of its two passes one)
static_assert(BA_THREADS == 2 * WAVE, "the adjoint runs its destination pass on wave 0 and its source pass on wave 1");
constexpr int BA_FWD_LDS = 32768;        // bytes of staging per workgroup, forward
constexpr int BA_BWD_LDS = 36864;        // adjoint (with the tables and the reduction cells: four workgroups per CU, as the forward)
constexpr int BA_BAD = 0x7f;             // pair code: the bond's class lies outside the table (the pair contributes nothing)
constexpr int BA_SELF_LOOP = 1, BA_REPEATED = 2, BA_CROSSING = 4;      // status[1]: the first two as sn_make_full_graph

__host__ __device__ inline int64_t ba_lds_bytes(int64_t n, int dk, bool bwd) {
  const int64_t per = bwd ? 6 * (int64_t)dk + 2 : 3 * (int64_t)dk;
  return 4 * n * per + ((n * n + 3) & ~(int64_t)3);
}

__device__ __forceinline__ float ba_weight(float ex, bool real, float L) { return real ? ex / (L + 1.0f) : (L * ex) / (L + 1.0f); }

struct BaGraph {                       // one graph's slice of the plan and the validity vectors
  const int32_t* rowptr;
  const int32_t* col;
  const int32_t* eperm;
  const int64_t* e;
  const int32_t* evalid;
  int64_t base, n;
  int C;
};

__device__ __forceinline__ bool ba_edge_on(const BaGraph& G, int p) { return G.evalid == nullptr || G.evalid[G.eperm[p]] != 0; }

// the pair code of (j -> i) without the table: i's first valid in-edge from j
__device__ __forceinline__ int ba_scan(const BaGraph& G, int64_t i, int64_t j) {
  const int32_t want = (int32_t)(G.base + j);
  for (int p = G.rowptr[G.base + i]; p < G.rowptr[G.base + i + 1]; ++p)
    if (G.col[p] == want && ba_edge_on(G, p)) {
      const int64_t cls = G.e[G.eperm[p]];
      return (cls < 0 || cls >= G.C) ? BA_BAD : 1 + (int)cls;
    }
  return 0;
}

// in-edge p of node i is the bond of its pair: valid, inside the graph, no self loop, the first of its (u, v)
__device__ __forceinline__ bool ba_first(const BaGraph& G, int64_t i, int p) {
  const int32_t c = G.col[p];
  for (int q = G.rowptr[G.base + i]; q < p; ++q)
    if (G.col[q] == c && ba_edge_on(G, q)) return false;
  return true;
}

// Fill column i of the pair table from i's in-edges (one thread per column: no two threads share a byte); returns the graph flags.
__device__ __forceinline__ int ba_fill(const BaGraph& G, unsigned char* tab, int64_t i, bool& bad) {
  int flag = 0;
  for (int p = G.rowptr[G.base + i]; p < G.rowptr[G.base + i + 1]; ++p) {
    if (!ba_edge_on(G, p)) continue;
    const int64_t jl = (int64_t)G.col[p] - G.base;
    if (jl < 0 || jl >= G.n) { flag |= BA_CROSSING; continue; }
    if (jl == i) { flag |= BA_SELF_LOOP; continue; }
    unsigned char& b = tab[jl * G.n + i];
    if (b) { flag |= BA_REPEATED; continue; }
    const int64_t cls = G.e[G.eperm[p]];
    if (cls < 0 || cls >= G.C) { bad = true; b = BA_BAD; } else b = (unsigned char)(1 + cls);
  }
  return flag;
}

// the same flags without a table
__device__ __forceinline__ int ba_flags(const BaGraph& G, int64_t i, bool& bad) {
  int flag = 0;
  for (int p = G.rowptr[G.base + i]; p < G.rowptr[G.base + i + 1]; ++p) {
    if (!ba_edge_on(G, p)) continue;
    const int64_t jl = (int64_t)G.col[p] - G.base;
    if (jl < 0 || jl >= G.n) { flag |= BA_CROSSING; continue; }
    if (jl == i) { flag |= BA_SELF_LOOP; continue; }
    if (!ba_first(G, i, p)) { flag |= BA_REPEATED; continue; }
    const int64_t cls = G.e[G.eperm[p]];
    if (cls < 0 || cls >= G.C) bad = true;
  }
  return flag;
}

// the head's slices of the class tables: rows 0 .. C-1 = T_real, row C = T_fake[0]
template <int DKP>
__device__ __forceinline__ void ba_stage_tables(float* tT, const float* __restrict__ Tr, const float* __restrict__ Tf, int C, int d, int h, int dk) {
  for (int o = (int)threadIdx.x; o < (C + 1) * dk; o += BA_THREADS) {
    const int r = o / dk, c = o - r * dk;
    tT[r * DKP + c] = r < C ? Tr[(int64_t)r * d + h * dk + c] : Tf[h * dk + c];
  }
}

template <int DKP, bool STAGED>
__device__ __forceinline__ void ba_forward(const BaGraph& G, const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                           const float* __restrict__ Q2, const float* __restrict__ K2, int64_t ld, const float* lds,
                                           const unsigned char* tab, const float* tT, float L, int H, int h, int dk, float* __restrict__ out,
                                           float* __restrict__ den) {
  const int d = H * dk;
  const float root = sqrtf((float)dk);
  const int64_t n = G.n, base = G.base;
  const int rs = 3 * dk;
  for (int64_t i = threadIdx.x; i < n; i += BA_THREADS) {
    float q[DKP], q2[DKP], acc[DKP];
#pragma unroll
    for (int c = 0; c < DKP; ++c) {
      q[c] = c < dk ? Q[(base + i) * ld + h * dk + c] : 0.f;
      q2[c] = c < dk ? Q2[(base + i) * ld + h * dk + c] : 0.f;
      acc[c] = 0.f;
    }
    float z = 0.f;
    for (int64_t j = 0; j < n; ++j) {
      if (j == i) continue;
      const int code = STAGED ? (int)tab[j * n + i] : ba_scan(G, i, j);
      if (code == BA_BAD) continue;
      const bool real = code != 0;
      const float *kr, *vr;
      if (STAGED) {
        kr = lds + j * rs + (real ? 0 : dk);
        vr = lds + j * rs + 2 * dk;
      } else {
        kr = (real ? K : K2) + (base + j) * ld + h * dk;
        vr = V + (base + j) * ld + h * dk;
      }
      const float* tr = tT + (real ? code - 1 : G.C) * DKP;
      float sc = 0.f;
#pragma unroll
      for (int c = 0; c < DKP; ++c)
        if (c < dk) sc += ((kr[c] * (real ? q[c] : q2[c])) / root) * tr[c];
      const float s = ba_weight(expf(fminf(fmaxf(sc, -5.f), 5.f)), real, L);
      z += s;
#pragma unroll
      for (int c = 0; c < DKP; ++c)
        if (c < dk) acc[c] += vr[c] * s;
    }
    den[(base + i) * H + h] = z;
#pragma unroll
    for (int c = 0; c < DKP; ++c)
      if (c < dk) out[(base + i) * d + h * dk + c] = acc[c] / (z + 1e-6f);
  }
}

template <int DKP>
__global__ __launch_bounds__(BA_THREADS) void k_bond_attention(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                               const float* __restrict__ Q2, const float* __restrict__ K2, int64_t ld,
                                                               const float* __restrict__ Tr, const float* __restrict__ Tf, int C,
                                                               const int64_t* __restrict__ e, const float* __restrict__ gamma, int64_t N, int H,
                                                               int dk, const int32_t* __restrict__ graph_ptr, const int32_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ col, const int32_t* __restrict__ eperm,
                                                               const int32_t* __restrict__ gvalid, const int32_t* __restrict__ evalid,
                                                               float* __restrict__ out, float* __restrict__ den, int32_t* __restrict__ status) {
  __shared__ float lds[BA_FWD_LDS / 4];
  __shared__ float tT[(BA_MAX_CLASSES + 1) * DKP];
  const int64_t g = blockIdx.x;
  const int h = (int)blockIdx.y;
  const int d = H * dk;
  BaGraph G{rowptr, col, eperm, e, evalid, graph_ptr[g], 0, C};
  G.n = (int64_t)graph_ptr[g + 1] - G.base;
  if (G.n <= 0 || G.base < 0 || G.base + G.n > N) return;
  if (gvalid != nullptr && gvalid[g] == 0) {                // a padding graph: exact zeros, no flag, whatever it holds
    for (int64_t i = threadIdx.x; i < G.n; i += BA_THREADS) {
      den[(G.base + i) * H + h] = 0.f;
      for (int c = 0; c < dk; ++c) out[(G.base + i) * d + h * dk + c] = 0.f;
    }
    return;
  }
  const float L = fminf(fmaxf(gamma[0], 0.f), 1.f);
  ba_stage_tables<DKP>(tT, Tr, Tf, C, d, h, dk);
  bool bad = false;
  int flag = 0;
  if (ba_lds_bytes(G.n, dk, false) <= BA_FWD_LDS) {
    const int rs = 3 * dk;
    unsigned char* tab = reinterpret_cast<unsigned char*>(lds + G.n * rs);
    for (int64_t o = threadIdx.x; o < G.n * rs; o += BA_THREADS) {
      const int64_t i = o / rs;
      const int r = (int)(o - i * rs), blk = r / dk, c = r - blk * dk;
      lds[o] = (blk == 0 ? K : blk == 1 ? K2 : V)[(G.base + i) * ld + h * dk + c];
    }
    for (int64_t o = threadIdx.x; o < G.n * G.n; o += BA_THREADS) tab[o] = 0;
    __syncthreads();
    for (int64_t i = threadIdx.x; i < G.n; i += BA_THREADS) flag |= ba_fill(G, tab, i, bad);
    __syncthreads();
    ba_forward<DKP, true>(G, Q, K, V, Q2, K2, ld, lds, tab, tT, L, H, h, dk, out, den);
  } else {
    for (int64_t i = threadIdx.x; i < G.n; i += BA_THREADS) flag |= ba_flags(G, i, bad);
    __syncthreads();
    ba_forward<DKP, false>(G, Q, K, V, Q2, K2, ld, nullptr, nullptr, tT, L, H, h, dk, out, den);
  }
  if (status != nullptr && h == 0) {
    if (bad) atomicOr(status, 1);
    if (flag) atomicOr(status + 1, flag);
  }
}

// ---------------------------------------------------------------------------------------------------------------- the adjoint
// what a pass needs of the OTHER end's node: its row pointers and the two scalars gdo = dout . out, r = 1 / (den + 1e-6)
__device__ __forceinline__ float ba_gdo(const float* go, const float* o, int dk) {
  float s = 0.f;
  for (int c = 0; c < dk; ++c) s += go[c] * o[c];
  return s;
}

template <int DKP, bool STAGED>
__device__ __forceinline__ double ba_backward_dst(const BaGraph& G, const float* __restrict__ Q, const float* __restrict__ K,
                                                  const float* __restrict__ V, const float* __restrict__ Q2, const float* __restrict__ K2,
                                                  int64_t ld, const float* lds, const unsigned char* tab, const float* tT, float L,
                                                  const float* __restrict__ out, const float* __restrict__ den, const float* __restrict__ dout,
                                                  int H, int h, int dk, float* __restrict__ dQ, float* __restrict__ dQ2, float* __restrict__ ur,
                                                  int t0, int nt) {
  const int d = H * dk, C = G.C;
  const float root = sqrtf((float)dk);
  const float dw = 1.0f / ((L + 1.0f) * (L + 1.0f));
  const int64_t n = G.n, base = G.base;
  const int rs = 6 * dk;
  double dl = 0.0;
  for (int64_t i = t0; i < n; i += nt) {
    float q[DKP], q2[DKP], go[DKP], aq[DKP], aq2[DKP], uf[DKP];
#pragma unroll
    for (int c = 0; c < DKP; ++c) {
      const bool ok = c < dk;
      q[c] = ok ? Q[(base + i) * ld + h * dk + c] : 0.f;
      q2[c] = ok ? Q2[(base + i) * ld + h * dk + c] : 0.f;
      go[c] = ok ? dout[(base + i) * d + h * dk + c] : 0.f;
      aq[c] = 0.f;
      aq2[c] = 0.f;
      uf[c] = 0.f;
    }
    const float gdo = ba_gdo(dout + (base + i) * d + h * dk, out + (base + i) * d + h * dk, dk);
    const float r = 1.0f / (den[(base + i) * H + h] + 1e-6f);
    float* mine = ur + (base + i) * (C + 1) * d + h * dk;             // [C + 1][d]: this node's share of the table gradients
    for (int k = 0; k < C; ++k)
      for (int c = 0; c < dk; ++c) mine[(int64_t)k * d + c] = 0.f;
    // the bonds, in the order of i's in-edges
    for (int p = G.rowptr[base + i]; p < G.rowptr[base + i + 1]; ++p) {
      if (!ba_edge_on(G, p)) continue;
      const int64_t j = (int64_t)G.col[p] - base;
      if (j < 0 || j >= n || j == i) continue;
      if (!ba_first(G, i, p)) continue;              // a repeated (u, v) is taken once
      int cls;
      if (STAGED) {
        const int b = tab[j * n + i];
        if (b == BA_BAD) continue;
        cls = b - 1;
      } else {
        const int64_t c64 = G.e[G.eperm[p]];
        if (c64 < 0 || c64 >= C) continue;
        cls = (int)c64;
      }
      const float* kr = STAGED ? lds + j * rs : K + (base + j) * ld + h * dk;
      const float* vr = STAGED ? lds + j * rs + 2 * dk : V + (base + j) * ld + h * dk;
      const float* tr = tT + cls * DKP;
      float sc = 0.f, gv = 0.f;
#pragma unroll
      for (int c = 0; c < DKP; ++c)
        if (c < dk) { sc += ((kr[c] * q[c]) / root) * tr[c]; gv += go[c] * vr[c]; }
      const bool inside = sc > -5.f && sc < 5.f;
      const float ex = expf(fminf(fmaxf(sc, -5.f), 5.f));
      const float s = ba_weight(ex, true, L);
      const float ds = r * (gv - gdo);
      const float dscore = inside ? ds * s : 0.f;
      dl += (double)(ds * ex * (-dw));
#pragma unroll
      for (int c = 0; c < DKP; ++c)
        if (c < dk) {
          aq[c] += dscore * (kr[c] * tr[c]);                     // (the common 1 / sqrt(dk) of a sum is applied once, to the sum)
          mine[(int64_t)cls * d + c] += dscore * (kr[c] * q[c]);
        }
    }
    // every other pair, j ascending
    for (int64_t j = 0; j < n; ++j) {
      if (j == i) continue;
      const int code = STAGED ? (int)tab[j * n + i] : ba_scan(G, i, j);
      if (code != 0) continue;
      const float* kr = STAGED ? lds + j * rs + dk : K2 + (base + j) * ld + h * dk;
      const float* vr = STAGED ? lds + j * rs + 2 * dk : V + (base + j) * ld + h * dk;
      const float* tr = tT + C * DKP;
      float sc = 0.f, gv = 0.f;
#pragma unroll
      for (int c = 0; c < DKP; ++c)
        if (c < dk) { sc += ((kr[c] * q2[c]) / root) * tr[c]; gv += go[c] * vr[c]; }
      const bool inside = sc > -5.f && sc < 5.f;
      const float ex = expf(fminf(fmaxf(sc, -5.f), 5.f));
      const float s = ba_weight(ex, false, L);
      const float ds = r * (gv - gdo);
      const float dscore = inside ? ds * s : 0.f;
      dl += (double)(ds * ex * dw);
#pragma unroll
      for (int c = 0; c < DKP; ++c)
        if (c < dk) {
          aq2[c] += dscore * (kr[c] * tr[c]);
          uf[c] += dscore * (kr[c] * q2[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < DKP; ++c)
      if (c < dk) {
        dQ[(base + i) * d + h * dk + c] = aq[c] / root;
        dQ2[(base + i) * d + h * dk + c] = aq2[c] / root;
        mine[(int64_t)C * d + c] = uf[c];
      }
  }
  return dl;
}

template <int DKP, bool STAGED>
__device__ __forceinline__ void ba_backward_src(const BaGraph& G, const float* __restrict__ Q, const float* __restrict__ K,
                                                const float* __restrict__ V, const float* __restrict__ Q2, const float* __restrict__ K2,
                                                int64_t ld, const float* lds, const unsigned char* tab, const float* tT, float L,
                                                const float* __restrict__ out, const float* __restrict__ den, const float* __restrict__ dout,
                                                int H, int h, int dk, float* __restrict__ dK, float* __restrict__ dK2, float* __restrict__ dV,
                                                int t0, int nt) {
  const int d = H * dk, C = G.C;
  const float root = sqrtf((float)dk);
  const int64_t n = G.n, base = G.base;
  const int rs = 6 * dk;
  const float* gdo_l = lds + n * rs;           // (STAGED) [n] dout . out, then [n] 1 / (den + 1e-6)
  const float* r_l = gdo_l + n;
  for (int64_t j = t0; j < n; j += nt) {
    float kk[DKP], kk2[DKP], vv[DKP], ak[DKP], ak2[DKP], av[DKP];
#pragma unroll
    for (int c = 0; c < DKP; ++c) {
      const bool ok = c < dk;
      kk[c] = ok ? K[(base + j) * ld + h * dk + c] : 0.f;
      kk2[c] = ok ? K2[(base + j) * ld + h * dk + c] : 0.f;
      vv[c] = ok ? V[(base + j) * ld + h * dk + c] : 0.f;
      ak[c] = 0.f;
      ak2[c] = 0.f;
      av[c] = 0.f;
    }
    for (int64_t i = 0; i < n; ++i) {
      if (i == j) continue;
      const int code = STAGED ? (int)tab[j * n + i] : ba_scan(G, i, j);
      if (code == BA_BAD) continue;
      const bool real = code != 0;
      const float *qr, *gr;
      float gdo, r;
      if (STAGED) {
        qr = lds + i * rs + (real ? 3 * dk : 4 * dk);
        gr = lds + i * rs + 5 * dk;
        gdo = gdo_l[i];
        r = r_l[i];
      } else {
        qr = (real ? Q : Q2) + (base + i) * ld + h * dk;
        gr = dout + (base + i) * d + h * dk;
        gdo = ba_gdo(gr, out + (base + i) * d + h * dk, dk);
        r = 1.0f / (den[(base + i) * H + h] + 1e-6f);
      }
      const float* tr = tT + (real ? code - 1 : C) * DKP;
      float sc = 0.f, gv = 0.f;
#pragma unroll
      for (int c = 0; c < DKP; ++c)
        if (c < dk) { sc += (((real ? kk[c] : kk2[c]) * qr[c]) / root) * tr[c]; gv += gr[c] * vv[c]; }
      const bool inside = sc > -5.f && sc < 5.f;
      const float ex = expf(fminf(fmaxf(sc, -5.f), 5.f));
      const float s = ba_weight(ex, real, L);
      const float ds = r * (gv - gdo);
      const float dscore = inside ? ds * s : 0.f;
      const float w = s * r;
#pragma unroll
      for (int c = 0; c < DKP; ++c)
        if (c < dk) {
          const float v = dscore * (qr[c] * tr[c]);
          if (real) ak[c] += v; else ak2[c] += v;
          av[c] += w * gr[c];
        }
    }
#pragma unroll
    for (int c = 0; c < DKP; ++c)
      if (c < dk) {
        dK[(base + j) * d + h * dk + c] = ak[c] / root;
        dK2[(base + j) * d + h * dk + c] = ak2[c] / root;
        dV[(base + j) * d + h * dk + c] = av[c];
      }
  }
}

template <int DKP>
__global__ __launch_bounds__(BA_THREADS) void k_bond_attention_bwd(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                                   const float* __restrict__ Q2, const float* __restrict__ K2, int64_t ld,
                                                                   const float* __restrict__ Tr, const float* __restrict__ Tf, int C,
                                                                   const int64_t* __restrict__ e, const float* __restrict__ gamma,
                                                                   const float* __restrict__ out, const float* __restrict__ den,
                                                                   const float* __restrict__ dout, int64_t N, int H, int dk,
                                                                   const int32_t* __restrict__ graph_ptr, const int32_t* __restrict__ rowptr,
                                                                   const int32_t* __restrict__ col, const int32_t* __restrict__ eperm,
                                                                   const int32_t* __restrict__ gvalid, const int32_t* __restrict__ evalid,
                                                                   float* __restrict__ dQ, float* __restrict__ dK, float* __restrict__ dV,
                                                                   float* __restrict__ dQ2, float* __restrict__ dK2, float* __restrict__ ur,
                                                                   float* __restrict__ part, double* __restrict__ gpart) {
  __shared__ float lds[BA_BWD_LDS / 4];
  __shared__ float tT[(BA_MAX_CLASSES + 1) * DKP];
  __shared__ double red[BA_THREADS];
  const int64_t g = blockIdx.x;
  const int h = (int)blockIdx.y;
  const int d = H * dk;
  BaGraph G{rowptr, col, eperm, e, evalid, graph_ptr[g], 0, C};
  G.n = (int64_t)graph_ptr[g + 1] - G.base;
  float* mypart = part + g * (C + 1) * d + h * dk;              // [C + 1][d]: this graph's partial tables, this head's columns
  const bool sound = G.n > 0 && G.base >= 0 && G.base + G.n <= N;
  if (!sound || (gvalid != nullptr && gvalid[g] == 0)) {       // an empty or a padding graph: zeros everywhere it owns
    for (int o = (int)threadIdx.x; o < (C + 1) * dk; o += BA_THREADS) mypart[(int64_t)(o / dk) * d + o % dk] = 0.f;
    if (threadIdx.x == 0) gpart[g * H + h] = 0.0;
    if (sound)
      for (int64_t i = threadIdx.x; i < G.n; i += BA_THREADS)
        for (int c = 0; c < dk; ++c) {
          const int64_t o = (G.base + i) * d + h * dk + c;
          dQ[o] = 0.f; dK[o] = 0.f; dV[o] = 0.f; dQ2[o] = 0.f; dK2[o] = 0.f;
        }
    return;
  }
  const float L = fminf(fmaxf(gamma[0], 0.f), 1.f);
  ba_stage_tables<DKP>(tT, Tr, Tf, C, d, h, dk);
  double dl = 0.0;
  const bool dst_wave = threadIdx.x < WAVE;             // wave 0: the destination pass, wave 1: the source pass
  const int tw = (int)threadIdx.x % WAVE;
  if (ba_lds_bytes(G.n, dk, true) <= BA_BWD_LDS) {
    const int rs = 6 * dk;
    float* gdo_l = lds + G.n * rs;
    float* r_l = gdo_l + G.n;
    unsigned char* tab = reinterpret_cast<unsigned char*>(r_l + G.n);
    for (int64_t o = threadIdx.x; o < G.n * rs; o += BA_THREADS) {
      const int64_t i = o / rs;
      const int r = (int)(o - i * rs), blk = r / dk, c = r - blk * dk;
      lds[o] = blk < 5 ? (blk == 0 ? K : blk == 1 ? K2 : blk == 2 ? V : blk == 3 ? Q : Q2)[(G.base + i) * ld + h * dk + c]
                       : dout[(G.base + i) * d + h * dk + c];
    }
    for (int64_t i = threadIdx.x; i < G.n; i += BA_THREADS) {
      gdo_l[i] = ba_gdo(dout + (G.base + i) * d + h * dk, out + (G.base + i) * d + h * dk, dk);
      r_l[i] = 1.0f / (den[(G.base + i) * H + h] + 1e-6f);
    }
    for (int64_t o = threadIdx.x; o < G.n * G.n; o += BA_THREADS) tab[o] = 0;
    __syncthreads();
    bool bad = false;
    for (int64_t i = threadIdx.x; i < G.n; i += BA_THREADS) ba_fill(G, tab, i, bad);
    __syncthreads();
    // the two passes run side by side, a wave each: they share inputs only
    if (dst_wave) dl = ba_backward_dst<DKP, true>(G, Q, K, V, Q2, K2, ld, lds, tab, tT, L, out, den, dout, H, h, dk, dQ, dQ2, ur, tw, WAVE);
    else ba_backward_src<DKP, true>(G, Q, K, V, Q2, K2, ld, lds, tab, tT, L, out, den, dout, H, h, dk, dK, dK2, dV, tw, WAVE);
  } else {
    __syncthreads();
    if (dst_wave) dl = ba_backward_dst<DKP, false>(G, Q, K, V, Q2, K2, ld, nullptr, nullptr, tT, L, out, den, dout, H, h, dk, dQ, dQ2, ur, tw, WAVE);
    else ba_backward_src<DKP, false>(G, Q, K, V, Q2, K2, ld, nullptr, nullptr, tT, L, out, den, dout, H, h, dk, dK, dK2, dV, tw, WAVE);
  }
  red[threadIdx.x] = dl;
  __syncthreads();                            // (also: every node's scratch rows are written)
  for (int w = BA_THREADS / 2; w > 0; w >>= 1) {           // a fixed tree: the same order on every call
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) gpart[g * H + h] = red[0];
  // this graph's partial tables: its nodes' shares added in node order
  for (int o = (int)threadIdx.x; o < (C + 1) * dk; o += BA_THREADS) {
    const int r = o / dk, c = o - r * dk;
    const float* src = ur + (G.base * (C + 1) + r) * d + h * dk + c;
    float s = 0.f;
    for (int64_t i = 0; i < G.n; ++i) s += src[i * (C + 1) * d];
    mypart[(int64_t)r * d + c] = s / sqrtf((float)dk);
  }
}

// The deterministic finish: dT_real [C, d] = the per-graph tables added in graph order, dT_fake row 0 likewise and rows >= 1 zero.  An
// output element belongs to 16 lanes: lane l adds the graphs l, l + 16, ... in ascending order, the 16 partial sums are then added in lane
// order.  dgamma = the float64 per-(graph, head) partials — entry t on thread t % 256, then a fixed tree — passed where torch.clamp
// passes its gradient (0 <= gamma <= 1).  Either grouping depends on an entry's index only, so the zero entries of trailing padding
// graphs change nothing.
constexpr int BA_FIN_LANES = 16;

__global__ __launch_bounds__(256) void k_bond_attention_bwd_finish(const float* __restrict__ part, int64_t B, int C, int d,
                                                                   const double* __restrict__ gpart, int64_t ngp, const float* __restrict__ gamma,
                                                                   float* __restrict__ dTr, float* __restrict__ dTf, float* __restrict__ dgamma) {
  __shared__ float cell[256];
  __shared__ double red[256];
  const int l = (int)threadIdx.x % BA_FIN_LANES;
  const int64_t o = (int64_t)blockIdx.x * (256 / BA_FIN_LANES) + threadIdx.x / BA_FIN_LANES;
  const int64_t tot = (int64_t)2 * C * d;
  const int64_t row = o / d, c = o - row * d;
  float s = 0.f;
  if (o < tot && row <= C)
    for (int64_t b = l; b < B; b += BA_FIN_LANES) s += part[(b * (C + 1) + row) * d + c];
  cell[threadIdx.x] = s;
  __syncthreads();
  if (o < tot && l == 0) {
    float t = 0.f;
    for (int k = 0; k < BA_FIN_LANES; ++k) t += cell[threadIdx.x + k];
    if (row < C) dTr[row * d + c] = t;
    else dTf[(row - C) * d + c] = row == C ? t : 0.f;
  }
  if (blockIdx.x == 0) {
    double g = 0.0;
    for (int64_t t = threadIdx.x; t < ngp; t += 256) g += gpart[t];
    red[threadIdx.x] = g;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const float gm = gamma[0];
      dgamma[0] = (gm >= 0.f && gm <= 1.f) ? (float)red[0] : 0.f;
    }
  }
}

}  // namespace sn

using namespace sn;

#define BA_DISPATCH(dk, call)            \
  do {                                   \
    if ((dk) <= 4) { call(4); }          \
    else if ((dk) <= 8) { call(8); }     \
    else if ((dk) <= 16) { call(16); }   \
    else { call(32); }                   \
  } while (0)

extern "C" int64_t sn_bond_full_attention_staged_nodes(int dk, int bwd) {
  if (dk < 1 || dk > 32) return 0;
  int64_t n = 0;
  while (ba_lds_bytes(n + 1, dk, bwd != 0) <= (bwd ? BA_BWD_LDS : BA_FWD_LDS)) ++n;
  return n;
}

extern "C" int sn_bond_full_attention_f32(const float* Q, const float* K, const float* V, const float* Q2, const float* K2, int64_t ld,
                                          const float* T_real, const float* T_fake, int C, const int64_t* e, const float* gamma, int64_t N,
                                          int64_t B, int64_t E, int heads, int dk, const int32_t* graph_ptr, const int32_t* rowptr,
                                          const int32_t* col, const int32_t* eperm, const int32_t* graph_valid, const int32_t* edge_valid,
                                          float* out, float* den, int32_t* status, void* stream) {
  SN_REQUIRE(Q && K && V && Q2 && K2 && T_real && T_fake && gamma && graph_ptr && rowptr && out && den && N >= 0 && B >= 0 && E >= 0 && heads > 0,
             "sn_bond_full_attention_f32: bad arguments");
  SN_REQUIRE(dk >= 1 && dk <= 32, "sn_bond_full_attention_f32: head width %d not in [1, 32]", dk);
  SN_REQUIRE(C >= 1 && C <= BA_MAX_CLASSES, "sn_bond_full_attention_f32: %d edge classes not in [1, %d]", C, BA_MAX_CLASSES);
  SN_REQUIRE(ld >= (int64_t)heads * dk, "sn_bond_full_attention_f32: row stride shorter than heads * dk");
  SN_REQUIRE(E == 0 || (col && eperm && e), "sn_bond_full_attention_f32: null edge arrays");
  SN_REQUIRE(B <= 0x7fffffff && heads <= 65535, "sn_bond_full_attention_f32: %lld graphs x %d heads exceed the launch grid", (long long)B, heads);
  if (N == 0 || B == 0) return SN_OK;
  const dim3 grid((unsigned)B, (unsigned)heads);
  hipStream_t st = (hipStream_t)stream;
#define BA_FWD(P)                                                                                                                                 \
  hipLaunchKernelGGL(k_bond_attention<P>, grid, dim3(BA_THREADS), 0, st, Q, K, V, Q2, K2, ld, T_real, T_fake, C, e, gamma, N, heads, dk, graph_ptr, \
                     rowptr, col, eperm, graph_valid, edge_valid, out, den, status)
  BA_DISPATCH(dk, BA_FWD);
#undef BA_FWD
  SN_CHECK_LAUNCH("sn_bond_full_attention_f32");
  return SN_OK;
}

extern "C" int64_t sn_bond_full_attention_bwd_scratch_floats(int64_t N, int64_t B, int heads, int dk, int C) {
  if (N < 0 || B < 0 || heads <= 0 || dk <= 0 || C <= 0) return 0;
  const int64_t d = (int64_t)heads * dk;
  return 2 * B * heads + 2 + B * (C + 1) * d + N * (C + 1) * d;
}

extern "C" int sn_bond_full_attention_bwd_f32(const float* Q, const float* K, const float* V, const float* Q2, const float* K2, int64_t ld,
                                              const float* T_real, const float* T_fake, int C, const int64_t* e, const float* gamma,
                                              const float* out, const float* den, const float* dout, int64_t N, int64_t B, int64_t E, int heads,
                                              int dk, const int32_t* graph_ptr, const int32_t* rowptr, const int32_t* col, const int32_t* eperm,
                                              const int32_t* graph_valid, const int32_t* edge_valid, float* dQ, float* dK, float* dV, float* dQ2,
                                              float* dK2, float* dT_real, float* dT_fake, float* dgamma, float* scratch, void* stream) {
  SN_REQUIRE(Q && K && V && Q2 && K2 && T_real && T_fake && gamma && out && den && dout && graph_ptr && rowptr && dQ && dK && dV && dQ2 && dK2 &&
                 dT_real && dT_fake && dgamma && scratch && N >= 0 && B >= 0 && E >= 0 && heads > 0,
             "sn_bond_full_attention_bwd_f32: bad arguments");
  SN_REQUIRE(dk >= 1 && dk <= 32, "sn_bond_full_attention_bwd_f32: head width %d not in [1, 32]", dk);
  SN_REQUIRE(C >= 1 && C <= BA_MAX_CLASSES, "sn_bond_full_attention_bwd_f32: %d edge classes not in [1, %d]", C, BA_MAX_CLASSES);
  SN_REQUIRE(ld >= (int64_t)heads * dk, "sn_bond_full_attention_bwd_f32: row stride shorter than heads * dk");
  SN_REQUIRE(E == 0 || (col && eperm && e), "sn_bond_full_attention_bwd_f32: null edge arrays");
  SN_REQUIRE(B <= 0x7fffffff && heads <= 65535, "sn_bond_full_attention_bwd_f32: %lld graphs x %d heads exceed the launch grid", (long long)B, heads);
  SN_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, "sn_bond_full_attention_bwd_f32: scratch must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int d = heads * dk;
  const int64_t nb = N > 0 ? B : 0;
  // scratch: [float64 dgamma partials [B, heads] (+ 2 floats) | per-graph partial tables [B, C + 1, d] | per-node shares [N, C + 1, d]]
  double* gpart = reinterpret_cast<double*>(scratch);
  float* part = scratch + 2 * B * heads + 2;
  float* ur = part + B * (C + 1) * d;
  if (nb > 0) {
    const dim3 grid((unsigned)B, (unsigned)heads);
#define BA_BWD(P)                                                                                                                                    \
  hipLaunchKernelGGL(k_bond_attention_bwd<P>, grid, dim3(BA_THREADS), 0, st, Q, K, V, Q2, K2, ld, T_real, T_fake, C, e, gamma, out, den, dout, N, heads, \
                     dk, graph_ptr, rowptr, col, eperm, graph_valid, edge_valid, dQ, dK, dV, dQ2, dK2, ur, part, gpart)
    BA_DISPATCH(dk, BA_BWD);
#undef BA_BWD
  }
  hipLaunchKernelGGL(k_bond_attention_bwd_finish, dim3((unsigned)cdiv((int64_t)2 * C * d, 256 / BA_FIN_LANES)), dim3(256), 0, st, (const float*)part, nb, C, d,
                     (const double*)gpart, nb * heads, gamma, dT_real, dT_fake, dgamma);
  SN_CHECK_LAUNCH("sn_bond_full_attention_bwd_f32");
  return SN_OK;
}
