// padded_operator.hip — GATConv's operator pair built on the device from a batch's plans, with shapes that depend on capacities only
// (train_graph.BucketedStep: the captured step of pyg_gnn_types.GNN with gnn_type GATConv).
//
// The eager step builds the CSR without the input self loops with boolean indexing, argsort and bincount (pyg_gnn_types._gat_operator):
// data-dependent shapes and host waits, neither of which a captured step may have.  sn_csr_drop_loops takes the two plans the step
// builds anyway — sn_batch_plan's destination-sorted CSR of the edge list and of the flipped edge list, rows in edge-id order — and
// writes, into buffers of the plans' own sizes (rowptr [N + 1], col [E]):
//   the CSR by destination without the entries col == row, every row ordered by (source, input position) — the order of
//   filter_baselines._csr, so a node's softmax is summed in the eager step's order — and the same for the flipped list (the adjoint's).
// The live entry count exists on the device only (rowptr_out[N]); col_out beyond it is zero-filled, so the bytes are a function of the
// input alone.  The padding edges of sn_bucket_pack are self loops and vanish with the input's own.
//
// Three launches for both operators (blockIdx.y picks one): kept entries per row; an in-place scan by one workgroup; one thread per CSR
// slot finds its row (binary search in rowptr), ranks itself among the row's kept entries and stores its source at that rank.  A row
// is ranked by its own entries only, so any in-degree works (a padding node with E_cap - E self loops, an empty row); one owner per
// output element, no atomics: identical bytes on every call.
#include "common.hpp"

namespace sn {
namespace {

constexpr int OP_T = 256;
constexpr int OP_SCAN_T = 1024;

struct OpJob {
  const int32_t* rowptr;     // [N + 1] input CSR (clamped to [0, E] and to a non-decreasing range on every read)
  const int32_t* col;        // [E]
  int32_t* rowptr_out;       // [N + 1]
  int32_t* col_out;          // [E]
};
struct OpPair { OpJob j[2]; };

__device__ __forceinline__ void op_range(const int32_t* __restrict__ rowptr, int64_t n, int64_t E, int& lo, int& hi) {
  int64_t a = rowptr[n], b = rowptr[n + 1];
  a = a < 0 ? 0 : (a > E ? E : a);
  b = b < a ? a : (b > E ? E : b);
  lo = (int)a;
  hi = (int)b;
}
__device__ __forceinline__ bool op_kept(int c, int64_t row, int64_t N) { return c >= 0 && c < N && c != row; }

__global__ __launch_bounds__(OP_T) void k_op_count(OpPair P, int64_t N, int64_t E) {
  const OpJob J = P.j[blockIdx.y];
  const int64_t n = (int64_t)blockIdx.x * OP_T + threadIdx.x;
  if (n >= N) return;
  int lo, hi;
  op_range(J.rowptr, n, E, lo, hi);
  int cnt = 0;
  for (int e = lo; e < hi; ++e) cnt += op_kept(J.col[e], n, N) ? 1 : 0;
  J.rowptr_out[n + 1] = cnt;
}

// rowptr_out[1..N] holds the counts: inclusive scan in place, chunks of OP_SCAN_T with a running carry; rowptr_out[0] = 0
__global__ __launch_bounds__(OP_SCAN_T) void k_op_scan(OpPair P, int64_t N) {
  __shared__ int sh[OP_SCAN_T];
  const OpJob J = P.j[blockIdx.y];
  const int t = threadIdx.x;
  int carry = 0;
  if (t == 0) J.rowptr_out[0] = 0;
  for (int64_t base = 0; base < N; base += OP_SCAN_T) {
    const int64_t i = base + t;
    int v = i < N ? J.rowptr_out[i + 1] : 0;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < OP_SCAN_T; o <<= 1) {
      const int add = t >= o ? sh[t - o] : 0;
      __syncthreads();
      v += add;
      sh[t] = v;
      __syncthreads();
    }
    if (i < N) J.rowptr_out[i + 1] = carry + v;
    carry += sh[OP_SCAN_T - 1];
    __syncthreads();
  }
}

__global__ __launch_bounds__(OP_T) void k_op_place(OpPair P, int64_t N, int64_t E) {
  const OpJob J = P.j[blockIdx.y];
  const int64_t p = (int64_t)blockIdx.x * OP_T + threadIdx.x;
  if (p >= E) return;
  const int64_t total = J.rowptr_out[N];
  if (p >= total) J.col_out[p] = 0;                   // (kept entries land below `total`: the two stores never meet)
  // the row of slot p: the last row whose first slot is <= p (rows in front of it may be empty)
  int64_t a = 0, b = N;                               // first k in [0, N] with rowptr[k] > p
  while (a < b) {
    const int64_t mid = (a + b) >> 1;
    if ((int64_t)J.rowptr[mid] > p) b = mid; else a = mid + 1;
  }
  const int64_t row = a - 1;
  if (row < 0 || row >= N) return;
  int lo, hi;
  op_range(J.rowptr, row, E, lo, hi);
  if (p < lo || p >= hi) return;
  const int c = J.col[p];
  if (!op_kept(c, row, N)) return;
  int rank = 0;
  for (int q = lo; q < hi; ++q) {
    const int cq = J.col[q];
    rank += (op_kept(cq, row, N) && (cq < c || (cq == c && q < p))) ? 1 : 0;
  }
  const int64_t at = (int64_t)J.rowptr_out[row] + rank;
  if (at >= 0 && at < total && at < E) J.col_out[at] = c;
}

}  // namespace
}  // namespace sn

using namespace sn;

extern "C" int sn_csr_drop_loops(int64_t N, int64_t E, const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_t,
                                 const int32_t* col_t, int32_t* rowptr_out, int32_t* col_out, int32_t* rowptr_t_out, int32_t* col_t_out,
                                 void* stream) {
  SN_REQUIRE(N >= 1 && E >= 0 && N < (1ll << 31) - 1 && E < (1ll << 31), "sn_csr_drop_loops: N = %lld, E = %lld out of range", (long long)N,
             (long long)E);
  SN_REQUIRE(rowptr && rowptr_t && rowptr_out && rowptr_t_out, "sn_csr_drop_loops: null row pointer array");
  SN_REQUIRE(E == 0 || (col && col_t && col_out && col_t_out), "sn_csr_drop_loops: null column array");
  SN_REQUIRE(rowptr_out != rowptr_t_out && (E == 0 || col_out != col_t_out), "sn_csr_drop_loops: the two outputs must be distinct buffers");
  const OpPair P{{{rowptr, col, rowptr_out, col_out}, {rowptr_t, col_t, rowptr_t_out, col_t_out}}};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_op_count, dim3((unsigned)cdiv(N, OP_T), 2), dim3(OP_T), 0, st, P, N, E);
  SN_CHECK_LAUNCH("sn_csr_drop_loops");
  hipLaunchKernelGGL(k_op_scan, dim3(1, 2), dim3(OP_SCAN_T), 0, st, P, N);
  SN_CHECK_LAUNCH("sn_csr_drop_loops");
  if (E > 0) {
    hipLaunchKernelGGL(k_op_place, dim3((unsigned)cdiv(E, OP_T), 2), dim3(OP_T), 0, st, P, N, E);
    SN_CHECK_LAUNCH("sn_csr_drop_loops");
  }
  return SN_OK;
}
