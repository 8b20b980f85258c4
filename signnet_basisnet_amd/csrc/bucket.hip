// bucket.hip — variable-shape training batches in fixed-capacity buffers (train_graph.BucketedStep).
//
//   sn_bucket_pack        : ONE launch copies a batch of any shape into the capacity buffers of its bucket and writes the padding, the
//                           0/1 validity vectors (node, edge, graph) and the device count block [N, E, B, S].
//   sn_bucket_pack_dgl    : the same for a DGL batch (train_graph.DGLBucketedStep): edge list, atom / bond ids, pos_enc, snorm_n,
//                           targets, the padded per-graph node counts, the validity vectors, the node-slot vector and [N, E, B].
//   sn_batch_plan_padded: sn_batch_plan_ex, then the padding graphs (id >= counts[2]) get nvalid = 0 and empty eigenvector blocks.
//   sn_masked_l1_f32 / _bwd_f32 : mean |y - t| over the valid rows, divided by the device row count; its adjoint.
//
// Padding convention: valid rows first; padding nodes belong to the spare graph B_cap-1; graphs [B, B_cap-1) are empty; padding edges
// are self-loops spread over the padding nodes (edge E + i on node N + i % (N_cap - N)); padding features, eigenvalues, eigenvector entries and targets are zeros (id 0
// is a valid embedding row).  The capacities are host values of the capture; nothing inside a captured step reads N, E, B or S on
// the host — the kernels read the count block or the validity vectors.
#include "common.hpp"

namespace sn {

// The copy is bandwidth bound (~0.3 MB per 128-graph batch): one flat grid-stride space of 16-byte chunks over all segments, a 16-byte
// load + store where source and destination are aligned and the chunk is inside the copied part, word by word at the seams.
constexpr int PACK_SEGS = 12;
constexpr int PACK_T = 256;

struct PackSeg {
  const uint32_t* src;     // NULL: the copied part is the constant `val`
  uint32_t* dst;
  int64_t ncopy, ntot;     // 4-byte words: [0, ncopy) from src (or val), [ncopy, ntot) padding
  int64_t chunk0;          // first chunk of this segment in the flat space
  uint32_t val, fill_lo, fill_hi;   // padding word = fill_lo at even, fill_hi at odd word offsets (int64 fills: low / high half)
  int vec, dvec;           // src / dst 16-byte aligned
  int64_t spread;          // > 0 (edge endpoints, int64): padding element i gets fill_lo + (i - ncopy / 2) % spread instead
};

// The per-graph node counts of a DGL batch, padded to B_cap (sn_bucket_pack_dgl): the B real counts, 0 for the empty graphs,
// N_cap - N for the spare graph.  The node -> graph vector is rebuilt from them on the device (repeat_interleave with
// output_size = N_cap), which is only in bounds if they total N_cap: counts that are negative, above N or do not sum to N (a
// batch_num_nodes() inconsistent with the feature rows) are replaced by ONE graph holding all N_cap nodes and flagged in `error`
// (train_graph.DGLBucketedStep.check() raises the eager step's ValueError).
struct NodeCountJob {
  const int64_t* src;      // [B]
  int64_t* dst;            // [B_cap]; NULL: no job (sn_bucket_pack)
  int32_t* error;          // [1]
  int64_t B, Bc, N, Nc;
};

struct PackTab {
  PackSeg s[PACK_SEGS];
  int n;
  int ncnt;                // words of the count block: 4 ([N, E, B, S]) or 3 ([N, E, B])
  int64_t chunks;
  int32_t* counts;
  int32_t cnt[4];
  NodeCountJob nc;
};

// one workgroup: sum and range check of the B counts (fixed order), then the padded counts
__device__ void pack_node_counts(const NodeCountJob& j) {
  __shared__ int64_t s_sum[PACK_T];
  __shared__ int s_bad[PACK_T];
  const int t = threadIdx.x;
  int64_t sum = 0;
  int bad = 0;
  for (int64_t i = t; i < j.B; i += PACK_T) {
    const int64_t v = j.src[i];
    bad |= (v < 0) | (v > j.N);          // (each count <= N: the sum of B < 2^31 of them cannot overflow)
    sum += v;
  }
  s_sum[t] = sum;
  s_bad[t] = bad;
  __syncthreads();
  for (int w = PACK_T / 2; w > 0; w >>= 1) {
    if (t < w) {
      s_sum[t] += s_sum[t + w];
      s_bad[t] |= s_bad[t + w];
    }
    __syncthreads();
  }
  const bool ok = !s_bad[0] && s_sum[0] == j.N;
  for (int64_t i = t; i < j.Bc; i += PACK_T)
    j.dst[i] = i == j.Bc - 1 ? (ok ? j.Nc - j.N : j.Nc) : (ok && i < j.B ? j.src[i] : 0);
  if (t == 0) j.error[0] = ok ? 0 : 1;
}

__global__ __launch_bounds__(PACK_T) void k_bucket_pack(const PackTab tab) {
  if (blockIdx.x == 0 && (int)threadIdx.x < tab.ncnt) tab.counts[threadIdx.x] = tab.cnt[threadIdx.x];
  if (blockIdx.x == 0 && tab.nc.dst) pack_node_counts(tab.nc);
  for (int64_t c = (int64_t)blockIdx.x * PACK_T + threadIdx.x; c < tab.chunks; c += (int64_t)gridDim.x * PACK_T) {
    int k = 0;
#pragma unroll
    for (int j = 1; j < PACK_SEGS; ++j)
      if (j < tab.n && c >= tab.s[j].chunk0) k = j;
    const PackSeg& sg = tab.s[k];
    const int64_t w0 = (c - sg.chunk0) * 4;
    uint4 v;
    if (sg.vec && w0 + 4 <= sg.ncopy) {
      v = *reinterpret_cast<const uint4*>(sg.src + w0);
    } else {
      uint32_t t[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t w = w0 + u;
        t[u] = w < sg.ncopy ? (sg.src ? sg.src[w] : sg.val)
             : (w & 1) ? sg.fill_hi
             : sg.spread > 0 ? sg.fill_lo + (uint32_t)(((w - sg.ncopy) >> 1) % sg.spread) : sg.fill_lo;
      }
      v = make_uint4(t[0], t[1], t[2], t[3]);
    }
    if (sg.dvec && w0 + 4 <= sg.ntot) {
      *reinterpret_cast<uint4*>(sg.dst + w0) = v;
    } else {
      const uint32_t t[4] = {v.x, v.y, v.z, v.w};
      for (int u = 0; u < 4 && w0 + u < sg.ntot; ++u) sg.dst[w0 + u] = t[u];
    }
  }
}

// The padding graphs of a plan built over capacity buffers: nodes of graphs >= B get no eigenvector slot, graphs > B an empty
// eigenvector block (evoff[g] = evoff[B]: the spare graph's n^2 block would reach past the packed entries).
__global__ __launch_bounds__(256) void k_plan_pad(const int32_t* __restrict__ counts, const int32_t* __restrict__ node_graph, int64_t N,
                                                  int64_t Bc, int32_t* __restrict__ nvalid, int64_t* __restrict__ evoff) {
  const int B = counts[2];
  const int64_t n = N > Bc + 1 ? N : Bc + 1;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < N && node_graph[i] >= B) nvalid[i] = 0;
    if (i > B && i <= Bc) evoff[i] = evoff[B];
  }
}

// loss = sum_{valid rows r, c < C} |y - t| / (count * C), one workgroup, fixed summation order (reproducible)
__global__ __launch_bounds__(256) void k_masked_l1(const float* __restrict__ y, const float* __restrict__ t, int64_t R, int C,
                                                   const int32_t* __restrict__ valid, const int32_t* __restrict__ count,
                                                   float* __restrict__ loss) {
  __shared__ float red[256];
  float s = 0.f;
  const int64_t n = R * C;
  for (int64_t i = threadIdx.x; i < n; i += 256)
    if (valid[i / C]) s += fabsf(y[i] - t[i]);
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = red[0] / (float)((int64_t)count[0] * C);
}

__global__ __launch_bounds__(256) void k_masked_l1_bwd(const float* __restrict__ y, const float* __restrict__ t, int64_t R, int C,
                                                       const int32_t* __restrict__ valid, const int32_t* __restrict__ count,
                                                       const float* __restrict__ dloss, float* __restrict__ dy) {
  const int64_t n = R * C;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float g = dloss[0] / (float)((int64_t)count[0] * C);      // (mean's adjoint, then abs's: the order autograd takes)
  const float d = y[i] - t[i];
  dy[i] = valid[i / C] ? g * (float)((d > 0.f) - (d < 0.f)) : 0.f;
}

}  // namespace sn

using namespace sn;

static int add_seg(PackTab& tb, const char* who, const void* src, void* dst, int64_t ncopy_bytes, int64_t ntot_bytes, uint32_t val,
                   uint32_t lo, uint32_t hi, int64_t spread = 0) {
  SN_REQUIRE(tb.n < PACK_SEGS, "%s: too many segments", who);
  SN_REQUIRE(ncopy_bytes % 4 == 0 && ntot_bytes % 4 == 0 && ncopy_bytes >= 0 && ncopy_bytes <= ntot_bytes,
             "%s: segment of %lld bytes into %lld (rows must be whole 4-byte words and fit the capacity)", who,
             (long long)ncopy_bytes, (long long)ntot_bytes);
  SN_REQUIRE(ntot_bytes == 0 || dst, "%s: null capacity buffer", who);
  SN_REQUIRE((reinterpret_cast<uintptr_t>(dst) & 3) == 0 && (ncopy_bytes == 0 || (reinterpret_cast<uintptr_t>(src) & 3) == 0),
             "%s: arrays must be 4-byte aligned", who);
  if (ntot_bytes == 0) return SN_OK;
  PackSeg& s = tb.s[tb.n++];
  s.src = static_cast<const uint32_t*>(src);
  s.dst = static_cast<uint32_t*>(dst);
  s.ncopy = ncopy_bytes / 4;
  s.ntot = ntot_bytes / 4;
  s.chunk0 = tb.chunks;
  s.val = val;
  s.fill_lo = lo;
  s.fill_hi = hi;
  s.vec = src && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
  s.dvec = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  s.spread = spread;
  tb.chunks += cdiv(s.ntot, 4);
  return SN_OK;
}

#define SN_TRY(x)                  \
  do {                             \
    const int rc__ = (x);          \
    if (rc__ != SN_OK) return rc__; \
  } while (0)

static int launch_pack(const PackTab& tb, void* stream, const char* who) {
  int64_t blocks = cdiv(tb.chunks > 0 ? tb.chunks : 1, PACK_T);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(k_bucket_pack, dim3((unsigned)blocks), dim3(PACK_T), 0, (hipStream_t)stream, tb);
  SN_CHECK_LAUNCH(who);
  return SN_OK;
}

// `plain`: a batch without eigen data (sn_bucket_pack_plain): eigen_values / eigen_vectors may be NULL, S must then be 0 and the two
// capacity buffers are zero-filled (a NULL source is the constant 0 of add_seg).
static int bucket_pack(const sn_bucket_pack_args* a, void* stream, bool plain) {
  SN_REQUIRE(a, "sn_bucket_pack: null args");
  SN_REQUIRE(!plain || a->eigen_vectors || a->S == 0, "sn_bucket_pack_plain: S = %lld eigenvector entries without a source array",
             (long long)a->S);
  const int64_t N = a->N, E = a->E, B = a->B, S = a->S, Nc = a->N_cap, Ec = a->E_cap, Bc = a->B_cap, Sc = a->S_cap;
  SN_REQUIRE(N >= 0 && E >= 0 && B >= 0 && S >= 0, "sn_bucket_pack: negative size");
  SN_REQUIRE(N < Nc && E <= Ec && B < Bc && S <= Sc, "sn_bucket_pack: batch (N %lld, E %lld, B %lld, S %lld) does not fit the bucket "
             "(N_cap %lld > N, E_cap %lld, B_cap %lld > B, S_cap %lld)", (long long)N, (long long)E, (long long)B, (long long)S,
             (long long)Nc, (long long)Ec, (long long)Bc, (long long)Sc);
  SN_REQUIRE(Nc < (1ll << 31) && Ec < (1ll << 31) && Bc < (1ll << 31) && Sc < (1ll << 31), "sn_bucket_pack: capacities exceed int32");
  SN_REQUIRE(a->x_row_bytes >= 0 && a->edge_row_bytes >= 0 && a->target_row_bytes >= 0, "sn_bucket_pack: negative row size");
  SN_REQUIRE((N == 0 || (a->batch && (a->eigen_values || plain))) && (E == 0 || a->edge_index) && (S == 0 || a->eigen_vectors) &&
             (N == 0 || a->x_row_bytes == 0 || a->x) && (E == 0 || a->edge_row_bytes == 0 || a->edge_attr) &&
             (B == 0 || a->target_row_bytes == 0 || a->target),
             "sn_bucket_pack: null source array");
  SN_REQUIRE(a->batch_out && a->eigen_values_out && a->node_valid && a->graph_valid && a->counts && (Ec == 0 || (a->edge_index_out && a->edge_valid)),
             "sn_bucket_pack: null capacity buffer");
  PackTab tb{};
  const char* who = plain ? "sn_bucket_pack_plain" : "sn_bucket_pack";
  // padding edge i (0-based) is a self-loop on padding node N + i % (N_cap - N): spread over the padding nodes, never hundreds of
  // in-edges on one node (the aggregations walk a node's in-edges serially: one node with 250 self-loops was a 0.3 ms tail per step)
  const uint32_t pad_node = (uint32_t)N, pad_graph = (uint32_t)(Bc - 1);
  SN_TRY(add_seg(tb, who, a->x, a->x_out, N * a->x_row_bytes, Nc * a->x_row_bytes, 0, 0, 0));
  SN_TRY(add_seg(tb, who, a->edge_index, a->edge_index_out, 8 * E, 8 * Ec, 0, pad_node, 0, Nc - N));
  SN_TRY(add_seg(tb, who, a->edge_index ? a->edge_index + E : nullptr, a->edge_index_out ? a->edge_index_out + Ec : nullptr, 8 * E, 8 * Ec,
                 0, pad_node, 0, Nc - N));
  SN_TRY(add_seg(tb, who, a->edge_attr, a->edge_attr_out, E * a->edge_row_bytes, Ec * a->edge_row_bytes, 0, 0, 0));
  SN_TRY(add_seg(tb, who, a->batch, a->batch_out, 8 * N, 8 * Nc, 0, pad_graph, 0));
  SN_TRY(add_seg(tb, who, a->eigen_values, a->eigen_values_out, 4 * N, 4 * Nc, 0, 0, 0));
  SN_TRY(add_seg(tb, who, a->eigen_vectors, a->eigen_vectors_out, 4 * S, 4 * Sc, 0, 0, 0));
  SN_TRY(add_seg(tb, who, a->target, a->target_out, B * a->target_row_bytes, Bc * a->target_row_bytes, 0, 0, 0));
  SN_TRY(add_seg(tb, who, nullptr, a->node_valid, 4 * N, 4 * Nc, 1u, 0, 0));
  SN_TRY(add_seg(tb, who, nullptr, a->edge_valid, 4 * E, 4 * Ec, 1u, 0, 0));
  SN_TRY(add_seg(tb, who, nullptr, a->graph_valid, 4 * B, 4 * Bc, 1u, 0, 0));
  tb.counts = a->counts;
  tb.ncnt = 4;
  tb.cnt[0] = (int32_t)N;
  tb.cnt[1] = (int32_t)E;
  tb.cnt[2] = (int32_t)B;
  tb.cnt[3] = (int32_t)S;
  return launch_pack(tb, stream, who);
}

extern "C" int sn_bucket_pack(const sn_bucket_pack_args* a, void* stream) { return bucket_pack(a, stream, false); }

extern "C" int sn_bucket_pack_plain(const sn_bucket_pack_args* a, void* stream) { return bucket_pack(a, stream, true); }

extern "C" int sn_bucket_pack_dgl(const sn_bucket_pack_dgl_args* a, void* stream) {
  SN_REQUIRE(a, "sn_bucket_pack_dgl: null args");
  const int64_t N = a->N, E = a->E, B = a->B, K = a->K, Nc = a->N_cap, Ec = a->E_cap, Bc = a->B_cap;
  SN_REQUIRE(N >= 0 && E >= 0 && B >= 0 && K >= 0, "sn_bucket_pack_dgl: negative size");
  SN_REQUIRE(N < Nc && E <= Ec && B < Bc, "sn_bucket_pack_dgl: batch (N %lld, E %lld, B %lld) does not fit the bucket "
             "(N_cap %lld > N, E_cap %lld, B_cap %lld > B)", (long long)N, (long long)E, (long long)B, (long long)Nc, (long long)Ec,
             (long long)Bc);
  SN_REQUIRE(Nc < (1ll << 31) && Ec < (1ll << 31) && Bc < (1ll << 31) && K < (1ll << 31) && Nc * K < (1ll << 40),
             "sn_bucket_pack_dgl: capacities exceed int32");
  SN_REQUIRE((E == 0 || (a->src && a->dst)) && (N == 0 || (a->h && (K == 0 || a->p))) && (B == 0 || (a->target && a->batch_num_nodes)) &&
             (E == 0 || !a->e_out || a->e) && (N == 0 || !a->snorm_n_out || a->snorm_n),
             "sn_bucket_pack_dgl: null source array");
  SN_REQUIRE(a->h_out && (K == 0 || a->p_out) && a->target_out && a->batch_num_nodes_out && a->node_valid && a->graph_valid && a->node_slots &&
             a->counts && a->count_error && (Ec == 0 || (a->src_out && a->dst_out && a->edge_valid)),
             "sn_bucket_pack_dgl: null capacity buffer");
  PackTab tb{};
  const char* who = "sn_bucket_pack_dgl";
  const uint32_t pad_node = (uint32_t)N;
  // the padding convention of sn_bucket_pack: padding edge E + i is a self-loop on padding node N + i % (N_cap - N)
  SN_TRY(add_seg(tb, who, a->src, a->src_out, 8 * E, 8 * Ec, 0, pad_node, 0, Nc - N));
  SN_TRY(add_seg(tb, who, a->dst, a->dst_out, 8 * E, 8 * Ec, 0, pad_node, 0, Nc - N));
  SN_TRY(add_seg(tb, who, a->h, a->h_out, 8 * N, 8 * Nc, 0, 0, 0));
  if (a->e_out) SN_TRY(add_seg(tb, who, a->e, a->e_out, 8 * E, 8 * Ec, 0, 0, 0));
  SN_TRY(add_seg(tb, who, a->p, a->p_out, 4 * N * K, 4 * Nc * K, 0, 0, 0));
  if (a->snorm_n_out) SN_TRY(add_seg(tb, who, a->snorm_n, a->snorm_n_out, 4 * N, 4 * Nc, 0, 0, 0));
  SN_TRY(add_seg(tb, who, a->target, a->target_out, 4 * B, 4 * Bc, 0, 0, 0));
  SN_TRY(add_seg(tb, who, nullptr, a->node_valid, 4 * N, 4 * Nc, 1u, 0, 0));
  SN_TRY(add_seg(tb, who, nullptr, a->edge_valid, 4 * E, 4 * Ec, 1u, 0, 0));
  SN_TRY(add_seg(tb, who, nullptr, a->graph_valid, 4 * B, 4 * Bc, 1u, 0, 0));
  SN_TRY(add_seg(tb, who, nullptr, a->node_slots, 4 * N, 4 * Nc, (uint32_t)K, 0, 0));
  // per-graph node counts: the B real ones, 0 for the empty graphs [B, B_cap-1), N_cap - N for the spare graph (workgroup 0)
  tb.nc = NodeCountJob{a->batch_num_nodes, a->batch_num_nodes_out, a->count_error, B, Bc, N, Nc};
  tb.counts = a->counts;
  tb.ncnt = 3;
  tb.cnt[0] = (int32_t)N;
  tb.cnt[1] = (int32_t)E;
  tb.cnt[2] = (int32_t)B;
  return launch_pack(tb, stream, who);
}

extern "C" int sn_batch_plan_padded(const int64_t* batch, int64_t N, int64_t B, const int64_t* edge_index, int64_t E, int kmax,
                                    int32_t* graph_ptr, int32_t* node_graph, int32_t* nvalid, int64_t* evoff, int32_t* rowptr,
                                    int32_t* col, int32_t* eperm, int32_t* status, const sn_plan_bins* bins, int32_t* scratch,
                                    const sn_plan_early* early, const int32_t* counts, void* stream) {
  SN_REQUIRE(counts, "sn_batch_plan_padded: null count block");
  SN_REQUIRE(B >= 1, "sn_batch_plan_padded: a padded batch has at least the spare graph");
  SN_TRY(sn_batch_plan_ex(batch, N, B, edge_index, E, kmax, graph_ptr, node_graph, nvalid, evoff, rowptr, col, eperm, status, bins, scratch,
                          early, stream));
  const int64_t n = N > B + 1 ? N : B + 1;
  hipLaunchKernelGGL(k_plan_pad, dim3((unsigned)(cdiv(n, 256) < 1024 ? cdiv(n, 256) : 1024)), dim3(256), 0, (hipStream_t)stream, counts,
                     node_graph, N, B, nvalid, evoff);
  SN_CHECK_LAUNCH("sn_batch_plan_padded");
  return SN_OK;
}

extern "C" int sn_masked_l1_f32(const float* y, const float* target, int64_t R, int C, const int32_t* valid, const int32_t* count,
                                float* loss, void* stream) {
  SN_REQUIRE(R >= 0 && C > 0, "sn_masked_l1_f32: bad shape");
  SN_REQUIRE((R == 0 || (y && target && valid)) && count && loss, "sn_masked_l1_f32: null argument");
  hipLaunchKernelGGL(k_masked_l1, dim3(1), dim3(256), 0, (hipStream_t)stream, y, target, R, C, valid, count, loss);
  SN_CHECK_LAUNCH("sn_masked_l1_f32");
  return SN_OK;
}

extern "C" int sn_masked_l1_bwd_f32(const float* y, const float* target, int64_t R, int C, const int32_t* valid, const int32_t* count,
                                    const float* dloss, float* dy, void* stream) {
  SN_REQUIRE(R >= 0 && C > 0, "sn_masked_l1_bwd_f32: bad shape");
  SN_REQUIRE((R == 0 || (y && target && valid && dy)) && count && dloss, "sn_masked_l1_bwd_f32: null argument");
  if (R == 0) return SN_OK;
  hipLaunchKernelGGL(k_masked_l1_bwd, dim3((unsigned)cdiv(R * C, 256)), dim3(256), 0, (hipStream_t)stream, y, target, R, C, valid, count,
                     dloss, dy);
  SN_CHECK_LAUNCH("sn_masked_l1_bwd_f32");
  return SN_OK;
}
