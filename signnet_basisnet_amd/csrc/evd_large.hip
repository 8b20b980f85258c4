// evd_large.hip — Laplacian eigendecomposition of the graphs of 65 .. 128 nodes of a collated batch (the graphs
// sn_laplacian_evd_f32 of evd.hip only flags: its kernel holds a graph's columns in the 64 lanes of a wave).
//
// Same method and numerics as k_evd_jacobi: parallel one-sided (Hestenes) Jacobi on G = L V, rotation in the
// Rutishauser form with the three-transcendental parameters, rotate while |g_i.g_j| > 5e-7 |g_i||g_j|, columns below 1e-6 of the
// largest norm left alone, eigenvalues as Rayleigh quotients, ranked and stored ascending in the reference's wire format.
//
// Layout (new): ONE workgroup of EVDL_WV waves per graph; lane k of every wave holds TWO columns — the pair that rotates this step
// (Brent-Luk systolic order) — so the three dot products of a pair are formed inside a lane, with no cross-lane traffic on the decision
// path.  Rows are dealt round-robin to the waves (row r belongs to wave r % WV, RW live rows per wave: a compile-time bound, as in
// evd_jacobi_rows); the waves' partial sums meet in LDS once per step (two alternating slots, one barrier), every wave adds them in
// wave order, so the rotate / skip / converged decisions are workgroup-uniform and the barrier count cannot diverge.
// After the step the columns move one place round the tournament ring: the "top" columns one lane up, the "bottom" columns one lane
// down (whole-wave DPP shifts: no LDS), turning round in the last lane of the graph; the top column of lane 0 stays.
// After m - 1 steps (m = n rounded up to even) every pair has met once and every column is back where it started.
#include "common.hpp"

namespace sn {
namespace {

constexpr int EVDL_MIN_N = 65;
constexpr int EVDL_MAX_N = 128;
constexpr int EVDL_WV = 8;              // waves per workgroup: 16 rows of G and V per column and lane at n = 128
constexpr int EVDL_MAX_SWEEPS = 24;     // (the largest count observed on the GPU is recorded in DESIGN.md §4.4)
constexpr float EVDL_TOL = 5e-7f;
constexpr float EVDL_NOCONV_TOL = 1e-5f;
constexpr float EVDL_ZERO = 1e-6f;

constexpr int EVDL_ST_CROSS = 1;        // an edge of a mid-size graph leaves its graph / bad node id / bad graph_ptr
constexpr int EVDL_ST_OVERSIZE = 2;     // a graph has more than 128 nodes (its outputs are not written)
constexpr int EVDL_ST_NOCONV = 4;
constexpr int EVDL_ST_SPACE = 8;        // a mid-size graph's block does not fit `total`

// ---- list of the mid-size graphs (one workgroup): work[0 .. count) = graph ids, work[B] = count
__global__ __launch_bounds__(256) void k_evdl_prep(const int32_t* __restrict__ graph_ptr, int B, int64_t N, int64_t total,
                                                     const int64_t* __restrict__ evoff, int32_t* __restrict__ list,
                                                     int32_t* __restrict__ status) {
  __shared__ int cnt;
  const int tid = threadIdx.x;
  if (tid == 0) cnt = 0;
  if (tid < 4) status[tid] = 0;          // (this kernel is the call's first: the later ones only OR / max into the words)
  __syncthreads();
  int flags = 0;
  for (int g = tid; g < B; g += 256) {
    const int n0 = graph_ptr[g], n1 = graph_ptr[g + 1], n = n1 - n0;
    if (n > EVDL_MAX_N) flags |= EVDL_ST_OVERSIZE;
    if (n < EVDL_MIN_N || n > EVDL_MAX_N) continue;
    if (n0 < 0 || n1 > N) { flags |= EVDL_ST_CROSS; continue; }
    const int64_t off = evoff[g];
    if (off < 0 || off + (int64_t)n * n > total) { flags |= EVDL_ST_SPACE; continue; }
    list[atomicAdd(&cnt, 1)] = g;
  }
  if (tid == 0 && evoff[B] > total) flags |= EVDL_ST_SPACE;
  if (flags) atomicOr(&status[0], flags);
  __syncthreads();
  if (tid == 0) list[B] = cnt;
  // (the list's order depends on the atomics' order: it decides only which workgroup serves which graph)
}

// ---- the listed graphs' eigenvector blocks to zero (they double as the dense-adjacency scratch)
__global__ __launch_bounds__(256) void k_evdl_clear(const int32_t* __restrict__ graph_ptr, int B,
                                                      const int64_t* __restrict__ evoff, const int32_t* __restrict__ list,
                                                      float* __restrict__ vec) {
  if ((int)blockIdx.x >= list[B]) return;
  const int g = list[blockIdx.x];
  const int n = graph_ptr[g + 1] - graph_ptr[g];
  float* blk = vec + evoff[g];
  for (int i = threadIdx.x; i < n * n; i += 256) blk[i] = 0.f;
}

// ---- dense adjacency of the mid-size graphs (undirected closure, self loops dropped, duplicates coalesced)
// graph of node x (last g with graph_ptr[g] <= x), or -1 for an id outside [0, min(N, graph_ptr[B]))
__device__ __forceinline__ int evdl_graph_of(int64_t x, int64_t N, const int32_t* __restrict__ graph_ptr, int B) {
  if (x < 0 || x >= N || x >= graph_ptr[B] || x < graph_ptr[0]) return -1;
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (graph_ptr[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_evdl_scatter(const int64_t* __restrict__ edge_index, int64_t E, int64_t N,
                                                        const int32_t* __restrict__ graph_ptr, int B,
                                                        const int64_t* __restrict__ evoff, int64_t total,
                                                        float* __restrict__ vec, int32_t* __restrict__ status) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const int64_t s = edge_index[e], d = edge_index[E + e];
  if (s == d) return;
  const int gs = evdl_graph_of(s, N, graph_ptr, B), gd = evdl_graph_of(d, N, graph_ptr, B);
  auto mid_size = [&](int g) {
    if (g < 0) return false;
    const int n = graph_ptr[g + 1] - graph_ptr[g];
    return n >= EVDL_MIN_N && n <= EVDL_MAX_N;
  };
  if (gs != gd) {            // the edge leaves its graph: this entry point's concern when an end lies in a mid-size graph
    if (mid_size(gs) || mid_size(gd)) atomicOr(&status[0], EVDL_ST_CROSS);
    return;
  }
  if (!mid_size(gs)) return;
  const int n0 = graph_ptr[gs], n1 = graph_ptr[gs + 1], n = n1 - n0;
  const int64_t off = evoff[gs];
  if (n1 > N || off < 0 || off + (int64_t)n * n > total) return;        // (k_evdl_prep has flagged it)
  const int a = (int)(s - n0), b = (int)(d - n0);
  vec[off + (int64_t)a * n + b] = 1.0f;
  vec[off + (int64_t)b * n + a] = 1.0f;
}

struct EvdLargeArgs {
  const int32_t* graph_ptr;
  const int64_t* evoff;
  const int32_t* list;         // [B] ids of the mid-size graphs, [B] = their count
  float* val;                  // [N]
  float* vec;                  // adjacency in, eigenvectors out
  float* pos_enc;              // [N, k] or null
  int32_t* status;
  int norm, k, skip;
  float tol2;                  // EVDL_TOL^2
};

// whole-wave shifts by one lane (DPP wave_shr:1 / wave_shl:1 — VALU, no LDS): lane l takes `v` of lane l - 1 (l + 1); the lane
// without a source (0 / 63) keeps `old`
__device__ __forceinline__ float from_lane_below(float old, float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float from_lane_above(float old, float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), 0x130, 0xf, 0xf, false));
}

// LDS: part[2][WV][64] float4 (the waves' partial sums), aux[128] (a value per column: D^-1/2, then the Rayleigh quotients)
constexpr int EVDL_LDS_FLOATS = 2 * EVDL_WV * 64 * 4 + EVDL_MAX_N;

template <int WV, int RW>
__device__ __noinline__ void evdl_jacobi_rows(const EvdLargeArgs& a, int n, int n0, int64_t off, float* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = (n + 1) & ~1, h = m >> 1;          // m columns (one of padding when n is odd), h lanes
  const int ct = lane, cb = lane + h;              // my columns at the start of every sweep: "top" and "bottom"
  const bool tcol = lane < h, bcol = lane < h && cb < n;
  float4* part = reinterpret_cast<float4*>(lds);
  float* aux = lds + 2 * WV * 64 * 4;
  float* blk = a.vec + off;
#define EVDL_ROWS(...)                                 \
  _Pragma("unroll") for (int i = 0; i < RW; ++i) {     \
    const int r = wave + WV * i;                       \
    (void)r;                                           \
    __VA_ARGS__                                        \
  }
  // the waves' partials of a lane's pair meet: every wave adds them in wave order (the same bits in all)
  auto meet = [&](int sl, float x, float y, float z, float& sx, float& sy, float& sz) {
    part[(sl * WV + wave) * 64 + lane] = make_float4(x, y, z, 0.f);
    __syncthreads();
    sx = 0.f; sy = 0.f; sz = 0.f;
#pragma unroll
    for (int w = 0; w < WV; ++w) {
      const float4 t = part[(sl * WV + w) * 64 + lane];
      sx += t.x; sy += t.y; sz += t.z;
    }
  };
  // rows r >= n of every column are padding: zero in G and V, and they stay zero
  float Gt[RW], Gb[RW], Vt[RW], Vb[RW];
  float dt = 0.f, db = 0.f, unused;
  EVDL_ROWS(
    Gt[i] = (tcol && r < n) ? blk[(int64_t)r * n + ct] : 0.f;
    Gb[i] = (bcol && r < n) ? blk[(int64_t)r * n + cb] : 0.f;
    Vt[i] = (tcol && r == ct) ? 1.f : 0.f;
    Vb[i] = (bcol && r == cb) ? 1.f : 0.f;
    dt += Gt[i]; db += Gb[i];)
  meet(0, dt, db, 0.f, dt, db, unused);            // degrees (small integers: exact in any order)
  if (a.norm == 1) {       // get_laplacian(normalization='sym'): I - D^-1/2 A D^-1/2, 1/sqrt(0) -> 0, unit diagonal everywhere
    const float dist = dt > 0.f ? 1.0f / sqrtf(dt) : 0.f, disb = db > 0.f ? 1.0f / sqrtf(db) : 0.f;
    if (wave == 0) {
      if (tcol) aux[ct] = dist;
      if (bcol) aux[cb] = disb;
    }
    __syncthreads();
    EVDL_ROWS(
      const float dr = r < n ? aux[r] : 0.f;
      Gt[i] = -(Gt[i] * dr) * dist;
      Gb[i] = -(Gb[i] * dr) * disb;
      if (tcol && r == ct) Gt[i] = 1.f;
      if (bcol && r == cb) Gb[i] = 1.f;)
  } else {                 // normalization=None: D - A
    EVDL_ROWS(
      Gt[i] = -Gt[i];
      Gb[i] = -Gb[i];
      if (tcol && r == ct) Gt[i] = dt;
      if (bcol && r == cb) Gb[i] = db;)
  }
  float alpha = 0.f, beta = 0.f, gamma;
  EVDL_ROWS(alpha = fmaf(Gt[i], Gt[i], alpha); beta = fmaf(Gb[i], Gb[i], beta);)
  meet(1, alpha, beta, 0.f, alpha, beta, unused);
  float amax = fmaxf(alpha, beta);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
  const float athr = EVDL_ZERO * EVDL_ZERO * amax;

  bool pending = false;
  int sweep = 0, sl = 0;
  for (; sweep < EVDL_MAX_SWEEPS; ++sweep) {
    bool rotated = false;
    pending = false;
    for (int step = 0; step < m - 1; ++step) {
      float al0 = 0.f, al1 = 0.f, be0 = 0.f, be1 = 0.f, ga0 = 0.f, ga1 = 0.f;
      EVDL_ROWS(
        if (i & 1) { al1 = fmaf(Gt[i], Gt[i], al1); be1 = fmaf(Gb[i], Gb[i], be1); ga1 = fmaf(Gt[i], Gb[i], ga1); }
        else { al0 = fmaf(Gt[i], Gt[i], al0); be0 = fmaf(Gb[i], Gb[i], be0); ga0 = fmaf(Gt[i], Gb[i], ga0); })
      meet(sl, al0 + al1, be0 + be1, ga0 + ga1, alpha, beta, gamma);
      sl ^= 1;
      const float lo = alpha, hi = beta;             // the top column plays the lower one's part
      const bool rot = tcol && gamma * gamma > a.tol2 * (lo * hi) && fminf(lo, hi) > athr;
      if (__ballot(rot) != 0ull) {                   // (every wave holds the same pairs and the same sums: workgroup-uniform)
        rotated |= rot;
        pending |= rot && gamma * gamma > (EVDL_NOCONV_TOL * EVDL_NOCONV_TOL) * (lo * hi);
        float s = 0.f, tau = 0.f;
        if (rot) {
          // zeta = d / gamma, d = (hi - lo) / 2;  with R = sqrt(d^2 + gamma^2) and w = 1 / sqrt(2 R (R + |d|)):
          // c = (R + |d|) w,  s = sgn(d) gamma w,  tau = s / (1 + c)     
          const float d = 0.5f * (hi - lo);
          const float R = __builtin_amdgcn_sqrtf(fmaf(d, d, gamma * gamma));
          const float u = R + fabsf(d);
          const float w = __builtin_amdgcn_rsqf(2.0f * R * u);
          const float c = u * w;
          s = (d < 0.f ? -gamma : gamma) * w;
          tau = s * __builtin_amdgcn_rcpf(1.0f + c);
        }
        // top: x - s (y + tau x);  bottom: y + s (x - tau y)
        EVDL_ROWS(
          const float x = Gt[i]; const float y = Gb[i];
          Gt[i] = fmaf(-s, fmaf(tau, x, y), x);
          Gb[i] = fmaf(s, fmaf(-tau, y, x), y);)
        EVDL_ROWS(
          const float x = Vt[i]; const float y = Vb[i];
          Vt[i] = fmaf(-s, fmaf(tau, x, y), x);
          Vb[i] = fmaf(s, fmaf(-tau, y, x), y);)
      }
      // the ring moves one place: top k <- top k-1 (top 1 <- bottom 0, top 0 stays), bottom k <- bottom k+1 (bottom h-1 <- top h-1)
      const bool first = lane == 0, last = lane == h - 1;
#define EVDL_SHIFT(T, Bm)                                                        \
      EVDL_ROWS(                                                                 \
        const float t = T[i]; const float b = Bm[i];                             \
        const float nt = from_lane_below(t, first ? b : t);                      \
        const float nb = from_lane_above(t, b);                                  \
        T[i] = nt; Bm[i] = last ? t : nb;)
      EVDL_SHIFT(Gt, Gb)
      EVDL_SHIFT(Vt, Vb)
#undef EVDL_SHIFT
    }
    if (__ballot(rotated) == 0ull) break;
  }
  if (wave == 0) {
    if (__ballot(pending) != 0ull && lane == 0) atomicOr(&a.status[0], EVDL_ST_NOCONV);
    if (lane == 0) atomicMax(&a.status[1], min(sweep + 1, EVDL_MAX_SWEEPS));     // most sweeps any graph needed (diagnostic)
  }

  // Rayleigh quotients (the columns are back at ct / cb: only whole sweeps run), ascending rank (ties by column index), stores
  float lt = 0.f, lb = 0.f;
  EVDL_ROWS(lt = fmaf(Vt[i], Gt[i], lt); lb = fmaf(Vb[i], Gb[i], lb);)
  meet(sl, lt, lb, 0.f, lt, lb, unused);
  __syncthreads();                                   // (aux may still be read as D^-1/2 by a slower wave)
  if (wave == 0) {
    if (tcol) aux[ct] = lt;
    if (bcol) aux[cb] = lb;
  }
  __syncthreads();
  int rt = 0, rb = 0;
  for (int i = 0; i < n; ++i) {
    const float li = aux[i];
    rt += (li < lt || (li == lt && i < ct)) ? 1 : 0;
    rb += (li < lb || (li == lb && i < cb)) ? 1 : 0;
  }
  if (wave == 0) {
    if (tcol) a.val[n0 + rt] = lt;
    if (bcol) a.val[n0 + rb] = lb;
  }
  EVDL_ROWS(
    if (r < n) {
      if (tcol) blk[(int64_t)r * n + rt] = Vt[i];
      if (bcol) blk[(int64_t)r * n + rb] = Vb[i];
    })
  if (a.pos_enc != nullptr) {
    const int c0 = rt - a.skip, c1 = rb - a.skip;
    EVDL_ROWS(
      if (r < n) {
        if (tcol && c0 >= 0 && c0 < a.k) a.pos_enc[(int64_t)(n0 + r) * a.k + c0] = Vt[i];
        if (bcol && c1 >= 0 && c1 < a.k) a.pos_enc[(int64_t)(n0 + r) * a.k + c1] = Vb[i];
      })
    // zero padding when n - skip < k (this entry point does not rely on an earlier memset)
    const int pad0 = max(0, n - a.skip);
    if (pad0 < a.k) {
      const int pw = a.k - pad0;
      for (int i = threadIdx.x; i < n * pw; i += 64 * WV) a.pos_enc[(int64_t)(n0 + i / pw) * a.k + pad0 + i % pw] = 0.f;
    }
  }
#undef EVDL_ROWS
}

__global__ __launch_bounds__(64 * EVDL_WV) void k_evdl_jacobi(EvdLargeArgs a, int B) {
  __shared__ __align__(16) float lds[EVDL_LDS_FLOATS];
  if ((int)blockIdx.x >= a.list[B]) return;          // (workgroup-uniform)
  const int g = a.list[blockIdx.x];
  const int n0 = a.graph_ptr[g];
  const int n = __builtin_amdgcn_readfirstlane(a.graph_ptr[g + 1] - n0);
  const int64_t off = a.evoff[g];
  const int rows = (((n + 1) & ~1) + EVDL_WV - 1) / EVDL_WV;       // live rows per wave: 9 .. 16
  if (rows > 14) return evdl_jacobi_rows<EVDL_WV, 16>(a, n, n0, off, lds);
  if (rows > 12) return evdl_jacobi_rows<EVDL_WV, 14>(a, n, n0, off, lds);
  if (rows > 10) return evdl_jacobi_rows<EVDL_WV, 12>(a, n, n0, off, lds);
  return evdl_jacobi_rows<EVDL_WV, 10>(a, n, n0, off, lds);
}

}  // namespace
}  // namespace sn

extern "C" int sn_evd_large_max_nodes(void) { return sn::EVDL_MAX_N; }
extern "C" int64_t sn_evd_large_work_ints(int64_t B) { return B + 8; }

extern "C" int sn_laplacian_evd_large_f32(const int64_t* edge_index, int64_t E, const int32_t* graph_ptr, int64_t B, int64_t N,
                                          int norm, const int64_t* evoff, float* eigen_values, float* eigen_vectors,
                                          int64_t total, float* pos_enc, int k, int skip, int32_t* work, int32_t* status,
                                          void* stream) {
  using namespace sn;
  SN_REQUIRE(graph_ptr && evoff && eigen_values && eigen_vectors && work && status, "sn_laplacian_evd_large_f32: null pointer");
  SN_REQUIRE(E == 0 || edge_index, "sn_laplacian_evd_large_f32: null edge_index with E = %lld", (long long)E);
  SN_REQUIRE(B >= 0 && N >= 0 && E >= 0 && total >= 0 && B < (1ll << 31) && N < (1ll << 31), "sn_laplacian_evd_large_f32: bad sizes");
  SN_REQUIRE(norm == 0 || norm == 1, "sn_laplacian_evd_large_f32: norm must be 0 (None: D - A) or 1 ('sym'), got %d", norm);
  SN_REQUIRE(pos_enc == nullptr || (k > 0 && skip >= 0), "sn_laplacian_evd_large_f32: pos_enc needs k > 0, skip >= 0");
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) {
    hipError_t e = hipMemsetAsync(status, 0, 4 * sizeof(int32_t), st);
    if (e != hipSuccess) return fail(SN_ERR_LAUNCH, "sn_laplacian_evd_large_f32: memset: %s", hipGetErrorString(e));
    return SN_OK;
  }
  // the number of mid-size graphs is known on the device only: B workgroups are launched, those beyond the count return at once
  hipLaunchKernelGGL(k_evdl_prep, dim3(1), dim3(256), 0, st, graph_ptr, (int)B, N, total, evoff, work, status);
  SN_CHECK_LAUNCH("k_evdl_prep");
  hipLaunchKernelGGL(k_evdl_clear, dim3((unsigned)B), dim3(256), 0, st, graph_ptr, (int)B, evoff, work, eigen_vectors);
  SN_CHECK_LAUNCH("k_evdl_clear");
  if (E) {
    hipLaunchKernelGGL(k_evdl_scatter, dim3((unsigned)cdiv(E, 256)), dim3(256), 0, st, edge_index, E, N, graph_ptr, (int)B,
                       evoff, total, eigen_vectors, status);
    SN_CHECK_LAUNCH("k_evdl_scatter");
  }
  EvdLargeArgs a{graph_ptr, evoff, work, eigen_values, eigen_vectors, pos_enc, status, norm, k, skip, EVDL_TOL * EVDL_TOL};
  hipLaunchKernelGGL(k_evdl_jacobi, dim3((unsigned)B), dim3(64 * EVDL_WV), 0, st, a, (int)B);
  SN_CHECK_LAUNCH("k_evdl_jacobi");
  return SN_OK;
}
