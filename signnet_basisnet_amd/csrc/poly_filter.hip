// poly_filter.hip — polynomial filters of ONE sparse operator on ONE fixed graph: the propagation of the LearningFilters baselines
// (BernNet, GPRNet, ChebNet, GcnNet; LearningFilters/models.py:138-377), all K steps of a layer in one launch.
//
//   S = diag_add * I + scale * W,   (W x)_i = sum_{e in row i} w_e x_{col_e}      (CSR by destination, self loops ordinary entries)
//
//   sn_poly_basis_f32     B_0 = x;  monomial: B_k = S B_{k-1};  Chebyshev: B_1 = S B_0, B_k = 2 S B_{k-1} - B_{k-2}
//                         (+ per-slice partial dots <B_k, g_k> for coefficient gradients)
//   sn_poly_combine_f32   y = sum_k c_k P_k(S) a_k:  Horner   h_K = c_K a_K, h_k = S h_{k+1} + c_k a_k, y = h_0          (monomial)
//                                                    Clenshaw b_k = c_k a_k + 2 S b_{k+1} - b_{k+2}, y = c_0 a_0 + S b_1 - b_2
//   The two are adjoint: d a_k = c_k P_k(S^T) g is basis over the transposed CSR, d x of basis is combine over it.
//
// Propagation never mixes feature channels, so a workgroup owns a slice of cs channels (cs = 4, 2 or 1 by N: slice_width) of all N nodes,
// keeps the current and the previous iterate of its slice in LDS ([N][cs] each, 2 * N * cs * 8 bytes <= 128 KiB) and runs every step
// without talking to another workgroup.  The iterates are DOUBLES: inputs, the stored stack and y are fp32, but nothing is rounded to fp32
// between the K steps of a launch — Bernstein's (2I - L)^k x grows like 2^k before L^i and the 2^-K factor bring it back, and an fp32
// rounding per step there costs more than the 1e-5 the networks are held to.  The new iterate overwrites the one two steps back in
// place (element idx of it is read only by the thread that writes element idx), so both three-term recurrences need two buffers.
// Every sum has one owner and a fixed order (a row's entries in CSR order; the dot of a slice by thread, wave, then wave order): no
// atomics, bit-reproducible.
// Entries whose column is outside [0, N) are skipped and rowptr is clamped to [0, nnz]: a malformed CSR never indexes outside LDS.
#include "common.hpp"

namespace sn {
namespace {

constexpr int PF_MAX_THREADS = 1024;
constexpr int PF_MAX_NODES = 8192;                         // cs = 1: 2 * 8192 * 8 B = 128 KiB of the 160 KiB a workgroup can have
constexpr int PF_LDS_ELEMS = 2 * PF_MAX_NODES;
constexpr int PF_RED = PF_MAX_THREADS / WAVE;

__host__ __device__ inline int slice_width_log2(int64_t N) { return N <= PF_MAX_NODES / 4 ? 2 : (N <= PF_MAX_NODES / 2 ? 1 : 0); }

struct Csr {
  const int32_t* rowptr;
  const int32_t* col;
  const float* w;
  int nnz;
  float diag_add, scale;
};

// (S v)[idx] for the slice image v [N][cs]; idx = node * cs + channel
__device__ __forceinline__ double apply_s(const Csr& G, const double* v, int N, int csl, int idx) {
  const int i = idx >> csl, ch = idx & ((1 << csl) - 1);
  int e0 = G.rowptr[i], e1 = G.rowptr[i + 1];
  e0 = e0 < 0 ? 0 : (e0 > G.nnz ? G.nnz : e0);
  e1 = e1 < e0 ? e0 : (e1 > G.nnz ? G.nnz : e1);
  double acc = 0.0;
  for (int e = e0; e < e1; ++e) {
    const int j = G.col[e];
    if ((unsigned)j < (unsigned)N) acc = fma((double)G.w[e], v[(j << csl) + ch], acc);
  }
  return fma((double)G.scale, acc, (double)G.diag_add * v[idx]);
}

// sum of v over the workgroup in a fixed order: lanes by xor-shuffle, then the waves in order (thread 0 returns the total)
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) t += red[wv];
  return t;
}

// element (k, node, channel) of a stack sits at base + k * sk + node * ld + channel (in elements); sk = 0: one [N, d] block shared by
// every k.  f64: the elements are doubles — the stack one launch hands the next (BernConv's (2I - L)^k x, 2^k large, goes through L^i
// and the 2^-K weights in the second launch: an fp32 rounding between the two is amplified like one between two steps).
struct Stack {
  const void* p;
  int64_t sk, ld;
  int reverse, f64;
  __device__ __forceinline__ double at(int64_t off) const {
    return f64 ? static_cast<const double*>(p)[off] : (double)static_cast<const float*>(p)[off];
  }
};

__global__ __launch_bounds__(PF_MAX_THREADS) void k_poly_basis(const float* __restrict__ x, int N, int d, int K, int cheb, Csr G, void* B,
                                                               int64_t b_sk, int64_t b_ld, int b_f64, Stack g, float* __restrict__ dot_part) {
  extern __shared__ __align__(16) double lds[];
  const int csl = slice_width_log2(N), cs = 1 << csl, total = N << csl;
  double* buf0 = lds;
  double* buf1 = lds + total;
  double* red = lds + 2 * total;
  const int c0 = blockIdx.x << csl, tid = threadIdx.x, nt = blockDim.x;
  const int cw = d - c0 < cs ? d - c0 : cs;                 // the last slice may be ragged
  for (int k = 0; k <= K; ++k) {
    double* cur = (k & 1) ? buf1 : buf0;                    // receives B_k; holds B_{k-2}
    const double* prev = (k & 1) ? buf0 : buf1;             // B_{k-1}
    const int64_t gk = (int64_t)(g.reverse ? K - k : k) * g.sk;
    double dot = 0.0;
    for (int idx = tid; idx < total; idx += nt) {
      const int i = idx >> csl, ch = idx & (cs - 1);
      double v;
      if (k == 0) {
        v = ch < cw ? (double)x[(int64_t)i * d + c0 + ch] : 0.0;
      } else {
        v = apply_s(G, prev, N, csl, idx);
        if (cheb && k >= 2) v = fma(2.0, v, -cur[idx]);
      }
      cur[idx] = v;
      if (ch < cw) {
        const int64_t bo = (int64_t)k * b_sk + (int64_t)i * b_ld + c0 + ch;
        if (B && b_f64) static_cast<double*>(B)[bo] = v;
        else if (B) static_cast<float*>(B)[bo] = (float)v;
        if (g.p) dot = fma(v, g.at(gk + (int64_t)i * g.ld + c0 + ch), dot);
      }
    }
    if (dot_part) {
      const double t = block_sum(dot, red);
      if (tid == 0) dot_part[(int64_t)blockIdx.x * (K + 1) + k] = (float)t;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(PF_MAX_THREADS) void k_poly_combine(Stack a, int N, int d, int K, int cheb, Csr G, const float* __restrict__ c,
                                                                 float* __restrict__ y) {
  extern __shared__ __align__(16) double lds[];
  const int csl = slice_width_log2(N), cs = 1 << csl, total = N << csl;
  double* buf0 = lds;
  double* buf1 = lds + total;
  const int c0 = blockIdx.x << csl, tid = threadIdx.x, nt = blockDim.x;
  const int cw = d - c0 < cs ? d - c0 : cs;
  if (cheb)                                                  // b_{K+1} = b_{K+2} = 0 (Horner reads neither before writing it)
    for (int idx = tid; idx < 2 * total; idx += nt) lds[idx] = 0.0;
  __syncthreads();
  for (int k = K; k >= 0; --k) {
    double* cur = ((K - k) & 1) ? buf1 : buf0;              // receives h_k / b_k; holds b_{k+2}
    const double* prev = ((K - k) & 1) ? buf0 : buf1;       // h_{k+1} / b_{k+1}
    const int64_t ak = (int64_t)(a.reverse ? K - k : k) * a.sk;
    const double ck = c ? (double)c[k] : 1.0;
    for (int idx = tid; idx < total; idx += nt) {
      const int i = idx >> csl, ch = idx & (cs - 1);
      double v = ch < cw ? ck * a.at(ak + (int64_t)i * a.ld + c0 + ch) : 0.0;
      if (k < K) {
        const double s = apply_s(G, prev, N, csl, idx);
        if (!cheb) v += s;
        else v += (k > 0 ? fma(2.0, s, -cur[idx]) : s - cur[idx]);
      }
      if (k > 0) cur[idx] = v;
      else if (ch < cw) y[(int64_t)i * d + c0 + ch] = (float)v;
    }
    __syncthreads();
  }
}

int check_common(const char* fn, int64_t N, int d, int K, int mode, const int32_t* rowptr, const int32_t* col, const float* w, int64_t nnz) {
  SN_REQUIRE(N >= 1 && d >= 1 && K >= 0 && K <= 4096, "%s: bad sizes (N %lld, d %d, K %d)", fn, (long long)N, d, K);
  SN_REQUIRE(mode == SN_POLY_MONOMIAL || mode == SN_POLY_CHEBYSHEV, "%s: mode must be SN_POLY_MONOMIAL or SN_POLY_CHEBYSHEV", fn);
  SN_REQUIRE(N <= PF_MAX_NODES, "%s: N = %lld exceeds the LDS-bound node capacity %d (sn_poly_filter_max_nodes)", fn, (long long)N, PF_MAX_NODES);
  SN_REQUIRE(rowptr && nnz >= 0 && nnz < (1ll << 31) && (nnz == 0 || (col && w)), "%s: bad CSR", fn);
  return SN_OK;
}

struct Launch {
  dim3 grid, block;
  size_t lds;
};
Launch launch_shape(int64_t N, int d) {
  const int csl = slice_width_log2(N);
  const int64_t total = N << csl;
  int nt = (int)(cdiv(total, WAVE) * WAVE);
  nt = nt > PF_MAX_THREADS ? PF_MAX_THREADS : nt;
  return {dim3((unsigned)cdiv(d, 1 << csl)), dim3((unsigned)nt), (size_t)(2 * total + PF_RED) * sizeof(double)};
}

template <typename Kern>
int raise_lds(Kern kern, const char* fn) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)((PF_LDS_ELEMS + PF_RED) * sizeof(double))) != hipSuccess)
    return fail(SN_ERR_LAUNCH, "%s: cannot raise the dynamic LDS limit", fn);
  return SN_OK;
}

}  // namespace
}  // namespace sn

using namespace sn;

extern "C" int sn_poly_filter_max_nodes(int K, int mode) {
  if (K < 0 || (mode != SN_POLY_MONOMIAL && mode != SN_POLY_CHEBYSHEV)) return 0;
  return PF_MAX_NODES;                                       // two iterates per slice whatever K and the recurrence
}

extern "C" int sn_poly_filter_launch_shape(int64_t N, int d, int* threads, int64_t* lds_bytes) {
  if (N < 1 || N > PF_MAX_NODES || d < 1) return 0;
  const Launch L = launch_shape(N, d);
  if (threads) *threads = (int)L.block.x;
  if (lds_bytes) *lds_bytes = (int64_t)L.lds;
  return (int)L.grid.x;
}

extern "C" int sn_poly_basis_f32(const float* x, int64_t N, int d, int K, int mode, const int32_t* rowptr, const int32_t* col, const float* w,
                                 int64_t nnz, float diag_add, float scale, void* B, int64_t b_sk, int64_t b_ld, int b_f64, const void* g,
                                 int64_t g_sk, int64_t g_ld, int g_reverse, int g_f64, float* dot_part, void* stream) {
  if (int rc = check_common("sn_poly_basis_f32", N, d, K, mode, rowptr, col, w, nnz)) return rc;
  SN_REQUIRE(x && (B || dot_part), "sn_poly_basis_f32: bad arguments");
  SN_REQUIRE(!B || (b_ld >= d && b_sk >= 0), "sn_poly_basis_f32: bad strides of B");
  SN_REQUIRE((g != nullptr) == (dot_part != nullptr) && (!g || (g_ld >= d && g_sk >= 0)), "sn_poly_basis_f32: g and dot_part go together");
  static bool init = false;
  if (!init) {
    if (int rc = raise_lds(k_poly_basis, "sn_poly_basis_f32")) return rc;
    init = true;
  }
  const Launch L = launch_shape(N, d);
  const Csr G{rowptr, col, w, (int)nnz, diag_add, scale};
  const Stack gs{g, g_sk, g_ld, g_reverse, g_f64 != 0};
  hipLaunchKernelGGL(k_poly_basis, L.grid, L.block, L.lds, (hipStream_t)stream, x, (int)N, d, K, (int)(mode == SN_POLY_CHEBYSHEV), G, B, b_sk,
                     b_ld, (int)(b_f64 != 0), gs, dot_part);
  SN_CHECK_LAUNCH("sn_poly_basis_f32");
  return SN_OK;
}

extern "C" int sn_poly_combine_f32(const void* a, int64_t a_sk, int64_t a_ld, int a_reverse, int a_f64, int64_t N, int d, int K, int mode,
                                   const int32_t* rowptr, const int32_t* col, const float* w, int64_t nnz, float diag_add, float scale,
                                   const float* c, float* y, void* stream) {
  if (int rc = check_common("sn_poly_combine_f32", N, d, K, mode, rowptr, col, w, nnz)) return rc;
  SN_REQUIRE(a && y && a_ld >= d && a_sk >= 0, "sn_poly_combine_f32: bad arguments");
  static bool init = false;
  if (!init) {
    if (int rc = raise_lds(k_poly_combine, "sn_poly_combine_f32")) return rc;
    init = true;
  }
  const Launch L = launch_shape(N, d);
  const Csr G{rowptr, col, w, (int)nnz, diag_add, scale};
  const Stack as{a, a_sk, a_ld, a_reverse, a_f64 != 0};
  hipLaunchKernelGGL(k_poly_combine, L.grid, L.block, L.lds, (hipStream_t)stream, as, (int)N, d, K, (int)(mode == SN_POLY_CHEBYSHEV), G, c, y);
  SN_CHECK_LAUNCH("sn_poly_combine_f32");
  return SN_OK;
}
