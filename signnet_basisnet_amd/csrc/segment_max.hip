// segment_max.hip — readout 'max' of the DGL tree's nets (dgl.max_nodes): the per-graph channel maximum with the row that attains
// it, and its adjoint (the gradient goes to that one row).  Rules:
//   ties    of equal values the LOWEST row wins — in a lane (rows arrive ascending, the test is strict) and in the fold (a total order
//           on (value, row)), so the result does not depend on how the rows are dealt to the row lanes;
//   NaN     a NaN among a graph's rows makes the graph's value NaN (torch.amax); arg is the first NaN row;
//   empty   a graph without rows gives value 0 and arg -1 (the unused graph slots of a padded bucket; sum / mean give 0 there too).
// No atomics: bitwise reproducible.
#include "common.hpp"

namespace sn {

constexpr int SEG_NONE = 0x7fffffff;      // the row of a lane that has seen no row yet

// the next row of a lane (rows ascend within a lane): a strictly larger value, or the lane's first NaN
__device__ __forceinline__ void seg_take(float& bv, int& br, float v, int r) {
  if (br == SEG_NONE || v > bv || (v != v && bv == bv)) { bv = v; br = r; }
}

// whether pair b precedes pair a in the order (NaN first, then the larger value, then the lower row); a pair without a row is last
__device__ __forceinline__ bool seg_before(float bv, int br, float av, int ar) {
  if (br == SEG_NONE) return false;
  if (ar == SEG_NONE) return true;
  const bool an = av != av, bn = bv != bv;
  if (bn) return !an || br < ar;
  return !an && (bv > av || (bv == av && br < ar));
}

// One workgroup per segment, as k_segment_pool: 256 threads = up to 256 / CW row lanes x CW column lanes, folded in LDS.  V = 4: a column lane
// owns four consecutive channels and reads them with one 128-bit load (C % 4 == 0, x 16-byte aligned); V = 1: the scalar path.
// Column chunks of 256 channels are spread over blockIdx.y.
template <int V>
__global__ __launch_bounds__(256) void k_segment_max(const float* __restrict__ x, int C, const int32_t* __restrict__ graph_ptr,
                                                     float* __restrict__ out, int32_t* __restrict__ arg) {
  __shared__ float rv[V * 256];
  __shared__ int rr[V * 256];
  const int g = blockIdx.x;
  const int lo = graph_ptr[g], hi = graph_ptr[g + 1];
  const int Q = C / V;                                      // column lanes' units: channels (V = 1) or channel quads
  int CW = 1;
  while (CW < Q && CW < 256 / V) CW <<= 1;
  const int cl = threadIdx.x & (CW - 1), rl = threadIdx.x / CW;
  // row lanes in use: halved while a lane would still see at most eight rows (the unroll depth) — a ZINC-sized graph then folds in two
  // LDS steps instead of up to eight; the (value, row) order is total, so the result does not depend on this count
  int RL = 256 / CW;
  while (RL > 4 && (RL >> 1) * 8 >= hi - lo) RL >>= 1;
  for (int q0 = blockIdx.y * CW; q0 < Q; q0 += gridDim.y * CW) {
    const int q = q0 + cl;
    float bv[V];
    int br[V];
#pragma unroll
    for (int t = 0; t < V; ++t) { bv[t] = -INFINITY; br[t] = SEG_NONE; }
    if (q < Q && rl < RL) {
      int i = lo + rl;
      // eight independent loads in flight per thread, taken in row order; a row past the segment's end is not read (its slot loads
      // the lane's first row again, which is inside the segment) and not taken
      for (; i < hi; i += 8 * RL) {
        float v[8][V];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int row = i + u * RL < hi ? i + u * RL : i;
          const float* p = x + (int64_t)row * C + (int64_t)q * V;
          if constexpr (V == 4) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(p);
            v[u][0] = w[0]; v[u][1] = w[1]; v[u][2] = w[2]; v[u][3] = w[3];
          } else {
            v[u][0] = p[0];
          }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (i + u * RL < hi) {
#pragma unroll
            for (int t = 0; t < V; ++t) seg_take(bv[t], br[t], v[u][t], i + u * RL);
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < V; ++t) { rv[t * 256 + threadIdx.x] = bv[t]; rr[t * 256 + threadIdx.x] = br[t]; }
    __syncthreads();
    for (int o = (RL * CW) >> 1; o >= CW; o >>= 1) {
      if ((int)threadIdx.x < o) {
#pragma unroll
        for (int t = 0; t < V; ++t) {
          const int a = t * 256 + threadIdx.x;
          const float ov = rv[a + o];
          const int orow = rr[a + o];
          if (seg_before(ov, orow, rv[a], rr[a])) { rv[a] = ov; rr[a] = orow; }
        }
      }
      __syncthreads();
    }
    if (rl == 0 && q < Q) {
#pragma unroll
      for (int t = 0; t < V; ++t) {
        const int64_t o = (int64_t)g * C + (int64_t)q * V + t;
        const int r = rr[t * 256 + cl];
        out[o] = r == SEG_NONE ? 0.f : rv[t * 256 + cl];
        if (arg != nullptr) arg[o] = r == SEG_NONE ? -1 : r;
      }
    }
    __syncthreads();
  }
}

// dx[row, c] = dy[b, c] where arg[b, c] == row, else 0 — every element of the graph's rows is written (no memset in front).
__global__ __launch_bounds__(256) void k_segment_max_bwd(const float* __restrict__ dy, const int32_t* __restrict__ arg, int C,
                                                         const int32_t* __restrict__ graph_ptr, float* __restrict__ dx) {
  const int b = blockIdx.x;
  const int lo = graph_ptr[b], hi = graph_ptr[b + 1];
  for (int64_t i = threadIdx.x; i < (int64_t)(hi - lo) * C; i += 256) {
    const int r = (int)(i / C);
    const int c = (int)(i - (int64_t)r * C);
    dx[(int64_t)lo * C + i] = arg[(int64_t)b * C + c] == lo + r ? dy[(int64_t)b * C + c] : 0.f;
  }
}

}  // namespace sn
using namespace sn;

extern "C" int sn_segment_max_f32(const float* x, int64_t B, int C, const int32_t* graph_ptr, float* out, int32_t* arg, void* stream) {
  SN_REQUIRE(x && out && graph_ptr && B >= 0 && C > 0, "sn_segment_max_f32: bad arguments");
  if (B == 0) return SN_OK;
  const dim3 grid((unsigned)B, (unsigned)cdiv(C, 256));
  if (C % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0)
    hipLaunchKernelGGL(k_segment_max<4>, grid, dim3(256), 0, (hipStream_t)stream, x, C, graph_ptr, out, arg);
  else
    hipLaunchKernelGGL(k_segment_max<1>, grid, dim3(256), 0, (hipStream_t)stream, x, C, graph_ptr, out, arg);
  SN_CHECK_LAUNCH("sn_segment_max_f32");
  return SN_OK;
}

extern "C" int sn_segment_max_bwd_f32(const float* dy, const int32_t* arg, int64_t B, int C, const int32_t* graph_ptr, float* dx,
                                      void* stream) {
  SN_REQUIRE(dy && arg && dx && graph_ptr && B >= 0 && C > 0, "sn_segment_max_bwd_f32: bad arguments");
  if (B == 0) return SN_OK;
  hipLaunchKernelGGL(k_segment_max_bwd, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, dy, arg, C, graph_ptr, dx);
  SN_CHECK_LAUNCH("sn_segment_max_bwd_f32");
  return SN_OK;
}
