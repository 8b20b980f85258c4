// filter_attention.hip — torch_geometric's GATConv on ONE fixed graph, forward and adjoint (the GatNet baseline of the LearningFilters
// table, LearningFilters/models.py:256-272: GATConv(..., concat=True, dropout=0) followed by F.elu).
//
//   attention set of node i, head h:  the CSR in-edges of i in stored order, then i itself (PyG drops the input self loops and gives
//   every node exactly one; here the loop is implicit — the CSR holds none)
//   e_ij = leaky_relu(feat_j . att_l[h] + feat_i . att_r[h]),  a = softmax over the set,  out[i,h,:] = act(sum_j a_ij feat[j,h,:] + bias[h,:])
//
// An ITEM is one (node, head).  A group of Gw = min(64, pow2 >= C) adjacent lanes owns an item, lane l the channels l and l + 64 (the
// second only for C > 64): with C = 8 a 256-thread workgroup carries 32 items, not 4.  Adjacent groups are adjacent heads of one node, so
// a workgroup's loads of a feat row are contiguous.  Rows are short (the grid: at most 4 neighbours and the loop), so a group walks its
// row serially with an online softmax; there is no in-degree threshold.  The only dispatch thresholds are the widths at which Gw doubles
// and C = 64 -> 65 (one -> two channels per lane): sn_gat_conv_group_width.
//
// Logits, the running maximum and every dot product are doubles (a logit of magnitude 80 carries 4e-6 of fp32 rounding, all of which
// would land in the probabilities); probabilities and the accumulated rows are fp32.
//
// Adjoint, two launches and the block-order reduction of the parameter partials:
//   k_gat_bwd_dst  by destination (the forward CSR): per item al = feat_i . att_l, ar = feat_i . att_r, the row's log-sum-exp again
//                  in double, delta = sum_j a_ij <dz_i, feat_j>, d ar = sum_j a_ij (<dz_i, feat_j> - delta) leaky'  -> work [5][N*heads]
//   k_gat_bwd_src  by source (the CSR of the flipped edge list): d al_j = sum_i ds_ij, dfeat[j] = sum_i a_ij dz_i + d al_j att_l + d ar_j att_r,
//                  and per workgroup the partial sums of d att_l = sum_j d al_j feat_j, d att_r = sum_j d ar_j feat_j, d bias = sum_j dz_j
//   dz = dout * act'(out) is formed on load (ELU: 1 where out > 0, else out + 1).  The probabilities are recomputed from the
//   log-sum-exp; nothing of size E is kept.  One owner per element, fixed orders, no atomics: bit-reproducible.
// Entries whose column is outside [0, N) are skipped and rowptr is clamped to [0, nnz]: a malformed CSR never indexes outside the arrays.
#include <math.h>

#include "common.hpp"

namespace sn {
namespace {

constexpr int GA_THREADS = 256;
constexpr int GA_MAX_HEADS = 16;                            // 3 * heads * C doubles of parameter partials live in LDS: 48 KiB at 16 x 128
constexpr int GA_MAX_C = 128;                               // two channels per lane of a 64-lane group
constexpr int GA_MAX_BLOCKS = 1 << 16;                      // forward / by-destination grid (grid-stride beyond)
constexpr int GA_BWD_MAX_BLOCKS = 512;                      // rows of the partials block

__host__ __device__ inline int group_log2(int C) {
  int g = 0;
  while ((1 << g) < C && g < 6) ++g;
  return g;
}

struct Gcsr {
  const int32_t* rowptr;
  const int32_t* col;
  int nnz;
};

__device__ __forceinline__ void row_range(const Gcsr& G, int64_t i, int& e0, int& e1) {
  e0 = G.rowptr[i];
  e1 = G.rowptr[i + 1];
  e0 = e0 < 0 ? 0 : (e0 > G.nnz ? G.nnz : e0);
  e1 = e1 < e0 ? e0 : (e1 > G.nnz ? G.nnz : e1);
}

// sum over the Gw lanes of a group (xor butterfly: every lane gets the same total, in one fixed order)
__device__ __forceinline__ double group_sum(double v, int Gw) {
  for (int o = Gw >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, Gw);
  return v;
}

__device__ __forceinline__ float act_slope(float out, int act) { return act ? (out > 0.f ? 1.f : out + 1.f) : 1.f; }

template <int CPL>
__global__ __launch_bounds__(GA_THREADS) void k_gat_fwd(const float* __restrict__ feat, const float* __restrict__ att_l,
                                                        const float* __restrict__ att_r, const float* __restrict__ bias, int64_t N, int H,
                                                        int C, float slope, int act, Gcsr G, float* __restrict__ out,
                                                        float* __restrict__ lse) {
  const int gl = group_log2(C), Gw = 1 << gl, ipb = GA_THREADS >> gl;
  const int l = threadIdx.x & (Gw - 1), slot = threadIdx.x >> gl;
  const int64_t items = N * H, chunks = (items + ipb - 1) / ipb, D = (int64_t)H * C;
  for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    const int64_t item = chunk * ipb + slot;
    if (item >= items) continue;                            // a whole group leaves together
    const int64_t i = item / H;
    const int h = (int)(item - i * H);
    float wl[CPL], fi[CPL], acc[CPL];
    bool ok[CPL];
    double dr = 0.0, dl = 0.0;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int c = l + k * 64;
      ok[k] = c < C;
      wl[k] = ok[k] ? att_l[h * C + c] : 0.f;
      fi[k] = ok[k] ? feat[i * D + h * C + c] : 0.f;
      dl += (double)fi[k] * wl[k];
      dr += ok[k] ? (double)fi[k] * att_r[h * C + c] : 0.0;
      acc[k] = 0.f;
    }
    const double ar = group_sum(dr, Gw);
    double m = -INFINITY;
    float s = 0.f;
    int e0, e1;
    row_range(G, i, e0, e1);
    for (int e = e0; e <= e1; ++e) {                        // e == e1: the node itself
      float fj[CPL];
      double d;
      if (e < e1) {
        const int j = G.col[e];
        if ((uint64_t)(int64_t)j >= (uint64_t)N) continue;
        d = 0.0;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          fj[k] = ok[k] ? feat[(int64_t)j * D + h * C + l + k * 64] : 0.f;
          d += (double)fj[k] * wl[k];
        }
      } else {
        d = dl;
#pragma unroll
        for (int k = 0; k < CPL; ++k) fj[k] = fi[k];
      }
      const double sij = group_sum(d, Gw) + ar;
      const double eij = sij > 0.0 ? sij : (double)slope * sij;
      const double mn = eij > m ? eij : m;
      const float rescale = expf((float)(m - mn)), p = expf((float)(eij - mn));
      s = s * rescale + p;
#pragma unroll
      for (int k = 0; k < CPL; ++k) acc[k] = acc[k] * rescale + p * fj[k];
      m = mn;
    }
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      if (!ok[k]) continue;
      const int c = l + k * 64;
      float z = acc[k] / s;
      if (bias) z += bias[h * C + c];
      out[i * D + h * C + c] = (act && z <= 0.f) ? expm1f(z) : z;
    }
    if (l == 0) lse[item] = (float)(m + log((double)s));
  }
}

// work: [5][N*H] doubles — al, ar, the log-sum-exp, delta, d ar
template <int CPL>
__global__ __launch_bounds__(GA_THREADS) void k_gat_bwd_dst(const float* __restrict__ feat, const float* __restrict__ att_l,
                                                            const float* __restrict__ att_r, const float* __restrict__ out,
                                                            const float* __restrict__ lse, const float* __restrict__ dout, int64_t N, int H,
                                                            int C, float slope, int act, Gcsr G, double* __restrict__ work) {
  const int gl = group_log2(C), Gw = 1 << gl, ipb = GA_THREADS >> gl;
  const int l = threadIdx.x & (Gw - 1), slot = threadIdx.x >> gl;
  const int64_t items = N * H, chunks = (items + ipb - 1) / ipb, D = (int64_t)H * C;
  for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    const int64_t item = chunk * ipb + slot;
    if (item >= items) continue;
    const int64_t i = item / H;
    const int h = (int)(item - i * H);
    float wl[CPL], fi[CPL], dz[CPL];
    bool ok[CPL];
    double dr = 0.0, dl = 0.0;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int c = l + k * 64;
      ok[k] = c < C;
      const int64_t at = i * D + h * C + c;
      wl[k] = ok[k] ? att_l[h * C + c] : 0.f;
      fi[k] = ok[k] ? feat[at] : 0.f;
      dz[k] = ok[k] ? dout[at] * act_slope(out[at], act) : 0.f;
      dl += (double)fi[k] * wl[k];
      dr += ok[k] ? (double)fi[k] * att_r[h * C + c] : 0.0;
    }
    const double ar = group_sum(dr, Gw), al_i = group_sum(dl, Gw), L = (double)lse[item];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;          // sum a, sum a da, sum a da leaky', sum a leaky'
    int e0, e1;
    row_range(G, i, e0, e1);
    for (int e = e0; e <= e1; ++e) {
      double d, da = 0.0;
      if (e < e1) {
        const int j = G.col[e];
        if ((uint64_t)(int64_t)j >= (uint64_t)N) continue;
        d = 0.0;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          const float fj = ok[k] ? feat[(int64_t)j * D + h * C + l + k * 64] : 0.f;
          d += (double)fj * wl[k];
          da += (double)fj * dz[k];
        }
        d = group_sum(d, Gw);
      } else {
        d = al_i;
#pragma unroll
        for (int k = 0; k < CPL; ++k) da += (double)fi[k] * dz[k];
      }
      da = group_sum(da, Gw);
      const double sij = d + ar;
      const double a = (double)expf((float)((sij > 0.0 ? sij : (double)slope * sij) - L));
      const double lk = sij > 0.0 ? 1.0 : (double)slope;
      s0 += a;
      s1 += a * da;
      s2 += a * da * lk;
      s3 += a * lk;
    }
    if (l == 0) {
      // the fp32 log-sum-exp is off by up to half an ulp of its magnitude, the same factor in every probability of the row: s0 is that
      // factor, and dividing by it normalises the row again
      const double delta = s1 / s0;
      work[item] = al_i;
      work[items + item] = ar;
      work[2 * items + item] = L + log(s0);
      work[3 * items + item] = delta;
      work[4 * items + item] = (s2 - delta * s3) / s0;
    }
  }
}

template <int CPL>
__global__ __launch_bounds__(GA_THREADS) void k_gat_bwd_src(const float* __restrict__ feat, const float* __restrict__ att_l,
                                                            const float* __restrict__ att_r, const float* __restrict__ out,
                                                            const float* __restrict__ dout, int64_t N, int H, int C, float slope, int act,
                                                            Gcsr T, const double* __restrict__ work, float* __restrict__ dfeat,
                                                            float* __restrict__ part) {
  extern __shared__ __align__(16) double lds[];
  const int gl = group_log2(C), Gw = 1 << gl, ipb = GA_THREADS >> gl;
  const int l = threadIdx.x & (Gw - 1), slot = threadIdx.x >> gl;
  const int64_t items = N * H, chunks = (items + ipb - 1) / ipb, D = (int64_t)H * C;
  const int HC = H * C;
  double* accd = lds;                                       // [3][H*C]: d att_l | d att_r | d bias of this workgroup
  double* stage = lds + 3 * HC;                             // [ipb][3][C]: the items of the current chunk
  for (int idx = threadIdx.x; idx < 3 * HC; idx += GA_THREADS) accd[idx] = 0.0;
  for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {      // trip count uniform over the workgroup
    const int64_t item0 = chunk * ipb, item = item0 + slot;
    if (item < items) {
      const int64_t j = item / H;
      const int h = (int)(item - j * H);
      float wl[CPL], fj[CPL], g[CPL], dzj[CPL];
      bool ok[CPL];
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int c = l + k * 64;
        ok[k] = c < C;
        wl[k] = ok[k] ? att_l[h * C + c] : 0.f;
        fj[k] = ok[k] ? feat[j * D + h * C + c] : 0.f;
        g[k] = dzj[k] = 0.f;
      }
      const double al = work[item];
      double dal = 0.0;
      int e0, e1;
      row_range(T, j, e0, e1);
      for (int e = e0; e <= e1; ++e) {                      // the targets of j's out-edges, then j's own loop
        int64_t i = j;
        if (e < e1) {
          i = T.col[e];
          if ((uint64_t)i >= (uint64_t)N) continue;
        }
        const int64_t it = i * H + h;
        float dz[CPL];
        double da = 0.0;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          const int64_t at = i * D + h * C + l + k * 64;
          dz[k] = ok[k] ? dout[at] * act_slope(out[at], act) : 0.f;
          da += (double)fj[k] * dz[k];
        }
        da = group_sum(da, Gw);
        const double sij = al + work[items + it];
        const double a = (double)expf((float)((sij > 0.0 ? sij : (double)slope * sij) - work[2 * items + it]));
        dal += a * (da - work[3 * items + it]) * (sij > 0.0 ? 1.0 : (double)slope);
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          g[k] += (float)a * dz[k];
          if (e == e1) dzj[k] = dz[k];
        }
      }
      const double dar = work[4 * items + item];
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        if (!ok[k]) continue;
        const int c = l + k * 64;
        dfeat[j * D + h * C + c] = (float)((double)g[k] + dal * wl[k] + dar * att_r[h * C + c]);
        double* st = stage + (int64_t)slot * 3 * C + c;
        st[0] = dal * fj[k];
        st[C] = dar * fj[k];
        st[2 * C] = (double)dzj[k];
      }
    }
    __syncthreads();
    // every (gradient, head, channel) adds the chunk's items of its head in item order
    const int live = items - item0 < ipb ? (int)(items - item0) : ipb;
    const int h0 = (int)(item0 % H);
    for (int idx = threadIdx.x; idx < 3 * HC; idx += GA_THREADS) {
      const int q = idx / HC, r = idx - q * HC, h = r / C, c = r - h * C;
      double t = accd[idx];
      for (int sl = (h - h0 + H) % H; sl < live; sl += H) t += stage[(sl * 3 + q) * C + c];
      accd[idx] = t;
    }
    __syncthreads();
  }
  for (int idx = threadIdx.x; idx < 3 * HC; idx += GA_THREADS) part[(int64_t)blockIdx.x * 3 * HC + idx] = (float)accd[idx];
}

int check_sizes(const char* fn, int64_t N, int heads, int C, int act, int64_t nnz) {
  SN_REQUIRE(N >= 1, "%s: N must be >= 1 (got %lld)", fn, (long long)N);
  SN_REQUIRE(heads >= 1, "%s: heads must be >= 1 (got %d)", fn, heads);
  SN_REQUIRE(C >= 1, "%s: C must be >= 1 (got %d)", fn, C);
  SN_REQUIRE(act == SN_GAT_ACT_NONE || act == SN_GAT_ACT_ELU, "%s: act must be SN_GAT_ACT_NONE (0) or SN_GAT_ACT_ELU (1), got %d", fn, act);
  SN_REQUIRE(nnz >= 0 && nnz < (1ll << 31), "%s: nnz must be in [0, 2^31) (got %lld)", fn, (long long)nnz);
  if (heads > GA_MAX_HEADS) return fail(SN_ERR_UNSUPPORTED, "%s: heads = %d exceeds the limit %d", fn, heads, GA_MAX_HEADS);
  if (C > GA_MAX_C) return fail(SN_ERR_UNSUPPORTED, "%s: C = %d exceeds the limit %d", fn, C, GA_MAX_C);
  return SN_OK;
}

int64_t chunk_count(int64_t N, int heads, int C) { return cdiv(N * heads, GA_THREADS >> group_log2(C)); }

}  // namespace
}  // namespace sn

using namespace sn;

extern "C" int sn_gat_conv_max_heads(void) { return GA_MAX_HEADS; }
extern "C" int sn_gat_conv_max_channels(void) { return GA_MAX_C; }

extern "C" int sn_gat_conv_group_width(int C) { return C < 1 || C > GA_MAX_C ? 0 : 1 << group_log2(C); }

extern "C" int sn_gat_conv_bwd_blocks(int64_t N, int heads, int C) {
  if (N < 1 || heads < 1 || heads > GA_MAX_HEADS || C < 1 || C > GA_MAX_C) return 0;
  const int64_t chunks = chunk_count(N, heads, C);
  return (int)(chunks < GA_BWD_MAX_BLOCKS ? chunks : GA_BWD_MAX_BLOCKS);
}

extern "C" int sn_gat_conv_f32(const float* feat, const float* att_l, const float* att_r, const float* bias, int64_t N, int heads, int C,
                               float negative_slope, int act, const int32_t* rowptr, const int32_t* col, int64_t nnz, float* out,
                               float* lse, void* stream) {
  if (int rc = check_sizes("sn_gat_conv_f32", N, heads, C, act, nnz)) return rc;
  SN_REQUIRE(feat && att_l && att_r && out && lse, "sn_gat_conv_f32: feat, att_l, att_r, out and lse must not be NULL");
  SN_REQUIRE(rowptr && (nnz == 0 || col), "sn_gat_conv_f32: rowptr (and col, for nnz > 0) must not be NULL");
  const int64_t chunks = chunk_count(N, heads, C);
  const dim3 grid((unsigned)(chunks < GA_MAX_BLOCKS ? chunks : GA_MAX_BLOCKS)), block(GA_THREADS);
  const Gcsr G{rowptr, col, (int)nnz};
  if (C <= 64)
    hipLaunchKernelGGL(k_gat_fwd<1>, grid, block, 0, (hipStream_t)stream, feat, att_l, att_r, bias, N, heads, C, negative_slope, act, G, out, lse);
  else
    hipLaunchKernelGGL(k_gat_fwd<2>, grid, block, 0, (hipStream_t)stream, feat, att_l, att_r, bias, N, heads, C, negative_slope, act, G, out, lse);
  SN_CHECK_LAUNCH("sn_gat_conv_f32");
  return SN_OK;
}

extern "C" int sn_gat_conv_bwd_f32(const float* feat, const float* att_l, const float* att_r, const float* out, const float* lse,
                                   const float* dout, int64_t N, int heads, int C, float negative_slope, int act, const int32_t* rowptr,
                                   const int32_t* col, const int32_t* rowptr_t, const int32_t* col_t, int64_t nnz, float* dfeat,
                                   float* part, double* work, void* stream) {
  if (int rc = check_sizes("sn_gat_conv_bwd_f32", N, heads, C, act, nnz)) return rc;
  SN_REQUIRE(feat && att_l && att_r && out && lse && dout, "sn_gat_conv_bwd_f32: feat, att_l, att_r, out, lse and dout must not be NULL");
  SN_REQUIRE(dfeat && part && work, "sn_gat_conv_bwd_f32: dfeat, part and work must not be NULL");
  SN_REQUIRE(rowptr && rowptr_t && (nnz == 0 || (col && col_t)), "sn_gat_conv_bwd_f32: both CSRs must be given");
  const int64_t chunks = chunk_count(N, heads, C);
  const dim3 grid((unsigned)(chunks < GA_MAX_BLOCKS ? chunks : GA_MAX_BLOCKS)), block(GA_THREADS);
  const dim3 grid_src((unsigned)sn_gat_conv_bwd_blocks(N, heads, C));
  const Gcsr G{rowptr, col, (int)nnz}, T{rowptr_t, col_t, (int)nnz};
  // 3 * heads * C accumulators and one chunk of staged items (256 >> log2 Gw items of 3 * C values): at most 48 + 12 KiB
  const size_t lds = (size_t)(3 * heads * C + (GA_THREADS >> group_log2(C)) * 3 * C) * sizeof(double);
  if (C <= 64) {
    hipLaunchKernelGGL(k_gat_bwd_dst<1>, grid, block, 0, (hipStream_t)stream, feat, att_l, att_r, out, lse, dout, N, heads, C, negative_slope, act, G, work);
    hipLaunchKernelGGL(k_gat_bwd_src<1>, grid_src, block, lds, (hipStream_t)stream, feat, att_l, att_r, out, dout, N, heads, C, negative_slope, act, T, work, dfeat, part);
  } else {
    hipLaunchKernelGGL(k_gat_bwd_dst<2>, grid, block, 0, (hipStream_t)stream, feat, att_l, att_r, out, lse, dout, N, heads, C, negative_slope, act, G, work);
    hipLaunchKernelGGL(k_gat_bwd_src<2>, grid_src, block, lds, (hipStream_t)stream, feat, att_l, att_r, out, dout, N, heads, C, negative_slope, act, T, work, dfeat, part);
  }
  SN_CHECK_LAUNCH("sn_gat_conv_bwd_f32");
  return SN_OK;
}
