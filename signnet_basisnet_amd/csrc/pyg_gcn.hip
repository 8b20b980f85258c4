// pyg_gcn.hip — the propagation of torch_geometric's GCNConv (gcn_norm with add_self_loops=True, unit edge weights), which the plain GNN
// of GINESignNetPyG builds for model.gnn_type GCNConv (core/model_utils/pyg_gnn_wrapper.py:39-48), restated from the library's
// documented definition: the input's self loops are replaced by exactly one unit loop per node, multi-edges are kept, and BOTH factors
// deg^-1/2 come from the in-degree (the sum over the target index) of A + I:
//   dis[i] = (1 + #{e in in(i): src(e) != i})^-1/2
//   out[i] = dis[i] * (sum_{e in in(i), src(e) != i} dis[src(e)] x[src(e)] + dis[i] x[i])
// over the destination-sorted CSR of sn_batch_plan (in-edges in edge-id order; the plan keeps the input's self loops: they are skipped
// here).  sn_gcn_propagate_f32 (deepsigns_variants.hip) is DGL's normalisation — the second factor from the OUT-degree, no self loop —
// and agrees with this one only on symmetric edge lists.  One owner per output element, no atomics, fixed order: bit-reproducible.
#include "common.hpp"

namespace {
using namespace sn;

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ __forceinline__ void row_range(const int32_t* __restrict__ rowptr, int64_t n, int64_t E, int& lo, int& hi) {
  int64_t a = rowptr[n], b = rowptr[n + 1];           // (a malformed plan is reported by its own status word: clamp)
  a = a < 0 ? 0 : (a > E ? E : a);
  b = b < a ? a : (b > E ? E : b);
  lo = (int)a;
  hi = (int)b;
}

__global__ __launch_bounds__(256) void k_gcn_pyg_coef(int64_t N, int64_t E, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                      float* __restrict__ dis) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  int lo, hi;
  row_range(rowptr, i, E, lo, hi);
  int d = 1;
  for (int e = lo; e < hi; ++e) d += col[e] != i ? 1 : 0;
  dis[i] = 1.f / sqrtf((float)d);
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_gcn_pyg_propagate(const float* __restrict__ x, int64_t ldx, int64_t N, int CV, int64_t E,
                                                           const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                           const float* __restrict__ dis, float* __restrict__ out, int64_t ldo) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t i = idx / CV;
  if (i >= N) return;
  const int c = (int)(idx - i * CV) * (VEC ? 4 : 1);
  int lo, hi;
  row_range(rowptr, i, E, lo, hi);
  const float di = dis[i];
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int e = lo; e <= hi; ++e) {                       // the last turn is the node's own unit loop
    const int64_t j = e < hi ? (int64_t)col[e] : i;
    if (j < 0 || j >= N || (e < hi && j == i)) continue;
    const float cj = dis[j];
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
  if (VEC) *reinterpret_cast<float4*>(out + i * ldo + c) = make_float4(__fmul_rn(a0, di), __fmul_rn(a1, di), __fmul_rn(a2, di), __fmul_rn(a3, di));
  else out[i * ldo + c] = __fmul_rn(a0, di);
}

}  // namespace

extern "C" int sn_gcn_pyg_coef_f32(int64_t N, int64_t E, const int32_t* rowptr, const int32_t* col, float* dis, void* stream) {
  SN_REQUIRE(rowptr && col && dis && N >= 0 && E >= 0, "sn_gcn_pyg_coef_f32: bad arguments");
  if (N == 0) return SN_OK;
  hipLaunchKernelGGL(k_gcn_pyg_coef, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, N, E, rowptr, col, dis);
  SN_CHECK_LAUNCH("sn_gcn_pyg_coef_f32");
  return SN_OK;
}

extern "C" int sn_gcn_pyg_propagate_f32(const float* x, int64_t ldx, int64_t N, int C, int64_t E, const int32_t* rowptr, const int32_t* col,
                                        const float* dis, float* out, int64_t ldo, void* stream) {
  SN_REQUIRE(x && out && rowptr && col && dis && N >= 0 && E >= 0 && C > 0, "sn_gcn_pyg_propagate_f32: bad arguments");
  SN_REQUIRE(ldx >= C && ldo >= C, "sn_gcn_pyg_propagate_f32: row stride smaller than C");
  SN_REQUIRE(x != out, "sn_gcn_pyg_propagate_f32: in-place propagation is not supported");
  if (N == 0) return SN_OK;
  const bool vec = C % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && al16(x) && al16(out);
  const int CV = vec ? C / 4 : C;
  const int64_t nblk = cdiv(N * CV, 256);
  SN_REQUIRE(nblk < ((int64_t)1 << 31), "sn_gcn_pyg_propagate_f32: too many elements for one launch");
  if (vec) hipLaunchKernelGGL(k_gcn_pyg_propagate<true>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, x, ldx, N, CV, E, rowptr, col, dis, out, ldo);
  else hipLaunchKernelGGL(k_gcn_pyg_propagate<false>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, x, ldx, N, CV, E, rowptr, col, dis, out, ldo);
  SN_CHECK_LAUNCH("sn_gcn_pyg_propagate_f32");
  return SN_OK;
}
