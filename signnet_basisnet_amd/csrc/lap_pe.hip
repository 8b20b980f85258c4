// lap_pe.hip — the network-free branches of the DGL tree's handle_lap (train/train_ZINC_graph_regression.py:13-51) on the device.
//
//   sn_lap_pe_transform_f32 : p [N, K] -> out [N, K] in ONE launch with no host read, so that a captured training step can record it.
//                             Modes: copy, one random sign per column, |p|, and the per-graph canonical sign.
//
// The op moves ~100 KB per batch and is bound by its launch; nothing here is tuned.
//   k_lap_pointwise : grid-stride over the N*K entries (copy / sign flip / abs).
//   k_lap_canonical : one wave per graph (grid-stride over graphs), lanes over columns (looping for K > 64).  A lane walks its column
//                     over the graph's rows in node order twice: the first pass counts and sums, the second writes.  SUMMATION ORDER:
//                     s_pos and s_neg of (graph, column) are fp32 sums accumulated by that one lane from the graph's first row to its
//                     last.  They depend on the graph's own rows only — not on the batch, the grid or N — so a graph gets the same
//                     signs alone, in a batch and in a padded capacity buffer, bit for bit.  A lane is the only reader and the only
//                     writer of its (graph, column): with out == p the column is read completely before any of it is written.
//                     Rows at or beyond graph_ptr[B] are copied by the whole grid afterwards (with out == p: rewritten unchanged).
// Row offsets read from graph_ptr are clamped to [0, N] and to a non-negative length: no access leaves p / out whatever it holds.
// No atomics, no LDS, plain vector loads and stores.
#include "common.hpp"

namespace sn {

constexpr int LAP_T = 256;
constexpr int LAP_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(LAP_T) void k_lap_pointwise(const float* p, int ldp, float* out, int ldo, int64_t total, int K,
                                                         int mode, const float* __restrict__ u) {
  for (int64_t i = (int64_t)blockIdx.x * LAP_T + threadIdx.x; i < total; i += (int64_t)gridDim.x * LAP_T) {
    const int64_t r = i / K;
    const int c = (int)(i - r * K);
    const float v = p[r * ldp + c];
    float y = v;
    if (mode == SN_LAP_SIGN_FLIP) y = v * (u[c] >= 0.5f ? 1.0f : -1.0f);
    else if (mode == SN_LAP_ABS_VAL) y = fabsf(v);
    out[r * ldo + c] = y;
  }
}

__device__ __forceinline__ int64_t lap_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(WAVE) void k_lap_canonical(const float* p, int ldp, float* out, int ldo, int N, int K,
                                                        const int32_t* __restrict__ graph_ptr, int B) {
  const int lane = threadIdx.x;
  for (int g = blockIdx.x; g < B; g += gridDim.x) {
    const int64_t r0 = lap_clamp(graph_ptr[g], 0, N);
    const int64_t r1 = lap_clamp(graph_ptr[g + 1], r0, N);
    for (int c = lane; c < K; c += WAVE) {
      int n_pos = 0, n_neg = 0;
      float s_pos = 0.0f, s_neg = 0.0f;
      for (int64_t r = r0; r < r1; ++r) {
        const float v = p[r * ldp + c];
        if (v >= 0.0f) {
          ++n_pos;
          s_pos += v;
        } else if (v < 0.0f) {
          ++n_neg;
          s_neg += -v;
        }
      }
      const float sign = (n_pos < n_neg || s_pos < s_neg) ? -1.0f : 1.0f;
      for (int64_t r = r0; r < r1; ++r) out[r * ldo + c] = sign * p[r * ldp + c];
    }
  }
  // rows no graph owns (a capacity buffer longer than the plan): copied
  const int64_t tail0 = lap_clamp(graph_ptr[B], 0, N);
  const int64_t total = ((int64_t)N - tail0) * K;
  for (int64_t i = (int64_t)blockIdx.x * WAVE + lane; i < total; i += (int64_t)gridDim.x * WAVE) {
    const int64_t r = tail0 + i / K;
    const int c = (int)(i % K);
    out[r * ldo + c] = p[r * ldp + c];
  }
}

}  // namespace sn

extern "C" int sn_lap_pe_transform_f32(const float* p, int ldp, float* out, int ldo, int N, int K, int mode, const float* u,
                                       const int32_t* graph_ptr, int B, void* stream) {
  using namespace sn;
  SN_REQUIRE(N >= 0 && K >= 0, "sn_lap_pe_transform_f32: negative size");
  SN_REQUIRE(mode == SN_LAP_NONE || mode == SN_LAP_SIGN_FLIP || mode == SN_LAP_ABS_VAL || mode == SN_LAP_CANONICAL,
             "sn_lap_pe_transform_f32: unknown mode %d", mode);
  if (N == 0 || K == 0) return SN_OK;
  SN_REQUIRE(p && out, "sn_lap_pe_transform_f32: null p / out");
  SN_REQUIRE(ldp >= K && ldo >= K, "sn_lap_pe_transform_f32: row stride smaller than K");
  SN_REQUIRE(mode != SN_LAP_SIGN_FLIP || u, "sn_lap_pe_transform_f32: SN_LAP_SIGN_FLIP needs the uniforms u [K]");
  SN_REQUIRE(mode != SN_LAP_CANONICAL || (graph_ptr && B >= 0), "sn_lap_pe_transform_f32: SN_LAP_CANONICAL needs graph_ptr [B + 1], B >= 0");
  if (mode == SN_LAP_CANONICAL) {
    const int64_t tail_blocks = cdiv((int64_t)N * K, WAVE);
    int64_t blocks = B > tail_blocks ? B : tail_blocks;      // (B graphs, or enough waves to copy a buffer no graph owns)
    blocks = blocks < 1 ? 1 : (blocks > LAP_MAX_BLOCKS ? LAP_MAX_BLOCKS : blocks);
    hipLaunchKernelGGL(k_lap_canonical, dim3((unsigned)blocks), dim3(WAVE), 0, (hipStream_t)stream, p, ldp, out, ldo, N, K, graph_ptr, B);
  } else {
    const int64_t total = (int64_t)N * K;
    int64_t blocks = cdiv(total, LAP_T);
    blocks = blocks > LAP_MAX_BLOCKS ? LAP_MAX_BLOCKS : blocks;
    hipLaunchKernelGGL(k_lap_pointwise, dim3((unsigned)blocks), dim3(LAP_T), 0, (hipStream_t)stream, p, ldp, out, ldo, total, K, mode, u);
  }
  SN_CHECK_LAUNCH("sn_lap_pe_transform_f32");
  return SN_OK;
}
