// collate.hip — a training batch gathered out of a device-resident graph store (data.GraphStore / data.DGLGraphStore).
//
//   sn_store_gather : ONE launch takes B graph indices (device memory) and writes the batch of those graphs, in index order, into the
//                     capacity buffers of a bucket: what a host collate (torch.cat, edge ids re-based) followed by sn_bucket_pack /
//                     sn_bucket_pack_dgl writes, byte for byte — valid rows first, edge endpoints re-based to batch node positions,
//                     the batch vector / the padded per-graph node counts, the validity vectors, the count block and the padding of
//                     bucket.hip's header.  `exact`: capacities = the exact totals, no padding, no spare graph (evaluation batches).
//
// A store is a set of concatenated arrays (segments) of four kinds — node, edge, eig (n^2 entries per graph) and graph rows — and the
// int64 offset tables node_ptr / edge_ptr / eig_ptr [G + 1].  Edge endpoints are stored with graph-local node ids.
//
// The one launch has two parts, both in every workgroup (no second launch, no grid-wide wait, no atomics):
//   1. the exclusive prefix sums of the B selected graphs' node, edge and n^2 counts (256 threads x 4 graphs, a block scan in LDS;
//      B <= 1024).  Every workgroup computes the same sums: ~7 table reads per graph out of L2, cheaper than a launch.
//   2. a grid-stride loop over the DESTINATION in 16-byte chunks, as in k_bucket_pack.  A chunk finds the graph of its first row by a
//      binary search of the prefix.  A graph's source offset and its destination offset differ modulo 16 in general (n^2 and E are odd
//      for many graphs): where the chunk lies inside one graph and the source address is 16-byte aligned it is one 16-byte load, else
//      its four words are fetched one by one (each word finds its own graph and source row: the seams between graphs need no special
//      case).  The store to the destination is 16 bytes wide either way, except at an unaligned or short tail.
// Every write goes through a destination offset < the segment's capacity, whatever the indices hold.  An index outside [0, G) is an
// empty graph (status flag 1).  Device totals that differ from the host's N, E, S or exceed a capacity (status flag 2) make the whole
// batch padding: nothing a later kernel indexes with can then lie outside the capacity buffers.
// The batch is ~1 MB: the kernel is bound by its launch and the prefix, not by HBM.
#include "common.hpp"

namespace sn {

constexpr int GATHER_T = 256;
constexpr int GATHER_PER = 4;                                   // graphs per thread in the scan
constexpr int GATHER_MAX_GRAPHS = GATHER_T * GATHER_PER;        // 1024
constexpr int GATHER_SEGS = SN_STORE_MAX_SEGS;
constexpr int KIND_NODE = SN_STORE_NODE, KIND_EDGE = SN_STORE_EDGE, KIND_EIG = SN_STORE_EIG, KIND_GRAPH = SN_STORE_GRAPH;
constexpr uint32_t NO_VEC = 255;

struct GatherSeg {
  const uint32_t* src;     // concatenated rows of all G graphs (NULL for generated segments)
  uint32_t* dst;
  uint32_t ntot;           // destination words (capacity rows x row words)
  uint32_t rw;             // words per row
  uint32_t chunk0;         // first chunk of this segment in the flat space
  int32_t val;             // SN_GATHER_CONST: the word written on valid rows
  uint8_t kind, op;
  uint8_t svec;            // (source address / 4) & 3, NO_VEC: no 16-byte loads (generated segment)
  uint8_t dvec;            // destination 16-byte aligned
};

struct GatherTab {
  GatherSeg s[GATHER_SEGS];
  int n, exact;
  uint32_t chunks;
  int B, ncnt;
  const int64_t* ptr[3];   // node_ptr, edge_ptr, eig_ptr (NULL: no eig segment)
  const int64_t* index;
  int64_t G;
  int64_t host[3];         // N, E, S as the host computed them
  int64_t cap[3];          // N_cap, E_cap, S_cap
  int64_t Bcap;
  int32_t* counts;
  int32_t* count_error;
  int32_t* status;
};

__global__ __launch_bounds__(GATHER_T) void k_store_gather(const GatherTab tab) {
  // s_pre[k][j]: batch row at which graph j's rows of kind k start (kind graph: j itself); s_base[k][j]: its first source row
  // (kind graph: the graph index, -1 if out of range)
  __shared__ int32_t s_pre[4][GATHER_MAX_GRAPHS + 1];
  __shared__ int64_t s_base[4][GATHER_MAX_GRAPHS];
  __shared__ int64_t s_part[3][GATHER_T];
  const int t = threadIdx.x, B = tab.B;

  // ---- part 1: prefix sums over the selected graphs (sums in int64: a total past int32 is a mismatch, its prefix is never used)
  int64_t cnt[3][GATHER_PER], sum[3] = {0, 0, 0};
  int bad = 0;
#pragma unroll
  for (int u = 0; u < GATHER_PER; ++u) {
    const int j = t * GATHER_PER + u;
    int64_t g = -1;
    if (j < B) {
      g = tab.index[j];
      if (g < 0 || g >= tab.G) {
        g = -1;
        bad = 1;
      }
      s_base[KIND_GRAPH][j] = g;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      int64_t a = 0, c = 0;
      if (g >= 0 && tab.ptr[k]) {
        a = tab.ptr[k][g];
        c = tab.ptr[k][g + 1] - a;
        if (c < 0) c = 0;
      }
      if (j < B) s_base[k][j] = a;
      cnt[k][u] = c;
      sum[k] += c;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) s_part[k][t] = sum[k];
  __syncthreads();
  for (int off = 1; off < GATHER_T; off <<= 1) {
    int64_t v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = t >= off ? s_part[k][t - off] : 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) s_part[k][t] += v[k];
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int64_t run = s_part[k][t] - sum[k];
#pragma unroll
    for (int u = 0; u < GATHER_PER; ++u) {
      const int j = t * GATHER_PER + u;
      if (j < B) s_pre[k][j] = (int32_t)run;
      run += cnt[k][u];
    }
    if (t == GATHER_T - 1) s_pre[k][B] = (int32_t)run;       // (the last thread's running sum: the total)
  }
  for (int j = t; j <= B; j += GATHER_T) s_pre[KIND_GRAPH][j] = j;
  bad = __syncthreads_or(bad);

  const int64_t devN = s_part[0][GATHER_T - 1], devE = s_part[1][GATHER_T - 1], devS = s_part[2][GATHER_T - 1];
  const int64_t limN = tab.exact ? tab.cap[0] : tab.cap[0] - 1;
  const bool mis = devN != tab.host[0] || devE != tab.host[1] || devS != tab.host[2] || devN > limN || devE > tab.cap[1] ||
                   devS > tab.cap[2];
  // valid rows per kind; a mismatch leaves none (all padding)
  const uint32_t vN = mis ? 0u : (uint32_t)devN, vE = mis ? 0u : (uint32_t)devE, vS = mis ? 0u : (uint32_t)devS,
                 vB = mis ? 0u : (uint32_t)B;
  const uint32_t Ncap = (uint32_t)tab.cap[0], Bcap = (uint32_t)tab.Bcap;
  const uint32_t spread = Ncap - vN;                            // padding nodes (0 only in the exact mode)

  if (blockIdx.x == 0 && t == 0) {
    const int64_t big = 0x7fffffff;
    tab.status[0] = (bad ? 1 : 0) | (mis ? 2 : 0);
    tab.status[1] = (int32_t)(devN < big ? devN : big);
    tab.status[2] = (int32_t)(devE < big ? devE : big);
    tab.status[3] = (int32_t)(devS < big ? devS : big);
    if (tab.counts) {
      tab.counts[0] = (int32_t)vN;
      tab.counts[1] = (int32_t)vE;
      tab.counts[2] = (int32_t)vB;
      if (tab.ncnt > 3) tab.counts[3] = (int32_t)vS;
    }
    if (tab.count_error) tab.count_error[0] = 0;
  }

  // ---- part 2: the copy, one 16-byte destination chunk per iteration
  for (uint32_t c = blockIdx.x * GATHER_T + t; c < tab.chunks; c += gridDim.x * GATHER_T) {
    int k = 0;
#pragma unroll
    for (int j = 1; j < GATHER_SEGS; ++j)
      if (j < tab.n && c >= tab.s[j].chunk0) k = j;
    const GatherSeg& sg = tab.s[k];
    const uint32_t w0 = (c - sg.chunk0) * 4, rw = sg.rw, ntot = sg.ntot;
    const int kind = sg.kind, op = sg.op;
    const uint32_t vrows = kind == KIND_NODE ? vN : kind == KIND_EDGE ? vE : kind == KIND_EIG ? vS : vB;
    const uint32_t nvw = vrows * rw;                            // valid words (<= ntot < 2^31)
    uint32_t r = w0 / rw, col = w0 - r * rw;
    const int32_t* pre = s_pre[kind];
    const int64_t* base = s_base[kind];

    int j = -1;
    if (w0 < nvw) {                                             // the graph of the chunk's first row: largest j with pre[j] <= r
      int lo = 0, hi = B;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)pre[mid] <= r) lo = mid; else hi = mid;
      }
      j = lo;
    }

    uint4 v;
    bool done = false;
    if (op == SN_GATHER_COPY && sg.svec != NO_VEC && w0 + 4 <= nvw) {
      const uint32_t rlast = (w0 + 3) / rw;
      if (rlast < (uint32_t)pre[j + 1] && base[j] >= 0) {
        const int64_t sw = (base[j] + (int64_t)(r - (uint32_t)pre[j])) * rw + col;
        if (((sw + sg.svec) & 3) == 0) {
          v = *reinterpret_cast<const uint4*>(sg.src + sw);
          done = true;
        }
      }
    }
    if (!done) {
      uint32_t wd[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t w = w0 + u;
        uint32_t word = 0;
        if (w < nvw) {
          while (r >= (uint32_t)pre[j + 1]) ++j;                // (r < the valid rows = pre[B]: ends at j < B; skips empty graphs)
          const int64_t srow = base[j] + (int64_t)(r - (uint32_t)pre[j]);
          if (op == SN_GATHER_COPY) {
            word = base[j] >= 0 ? sg.src[srow * rw + col] : 0u;
          } else if (op == SN_GATHER_ENDPOINT) {
            const int64_t id = reinterpret_cast<const int64_t*>(sg.src)[srow] + s_pre[KIND_NODE][j];
            word = col ? (uint32_t)((uint64_t)id >> 32) : (uint32_t)id;
          } else if (op == SN_GATHER_GRAPH_ID) {
            word = col ? 0u : (uint32_t)j;
          } else if (op == SN_GATHER_CONST) {
            word = (uint32_t)sg.val;
          } else {                                              // SN_GATHER_NODE_COUNT
            word = col ? 0u : (uint32_t)(s_pre[KIND_NODE][j + 1] - s_pre[KIND_NODE][j]);
          }
        } else if (col == 0) {                                  // padding (the high words of the int64 paddings are 0)
          if (op == SN_GATHER_ENDPOINT) {
            const uint32_t i = (w - nvw) >> 1;
            word = spread ? vN + i % spread : (Ncap ? Ncap - 1 : 0u);
          } else if (op == SN_GATHER_GRAPH_ID) {
            word = Bcap - 1;
          } else if (op == SN_GATHER_NODE_COUNT) {
            word = (!tab.exact && r == Bcap - 1) ? spread : 0u;
          }
        }
        wd[u] = word;
        if (++col == rw) {
          col = 0;
          ++r;
        }
      }
      v = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    }
    if (sg.dvec && w0 + 4 <= ntot) {
      *reinterpret_cast<uint4*>(sg.dst + w0) = v;
    } else {
      const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (w0 + u < ntot) sg.dst[w0 + u] = wd[u];
    }
  }
}

}  // namespace sn

using namespace sn;

extern "C" int sn_store_gather_max_graphs(void) { return GATHER_MAX_GRAPHS; }

extern "C" int sn_store_gather(const sn_store_gather_args* a, void* stream) {
  const char* who = "sn_store_gather";
  SN_REQUIRE(a, "%s: null args", who);
  const int64_t N = a->N, E = a->E, B = a->B, S = a->S, Nc = a->N_cap, Ec = a->E_cap, Bc = a->B_cap, Sc = a->S_cap;
  SN_REQUIRE(N >= 0 && E >= 0 && B >= 0 && S >= 0 && a->G >= 0, "%s: negative size", who);
  if (B > GATHER_MAX_GRAPHS)
    return sn::fail(SN_ERR_UNSUPPORTED, "%s: %lld graphs per call, built for at most %d", who, (long long)B, GATHER_MAX_GRAPHS);
  SN_REQUIRE(a->nseg >= 0 && a->nseg <= GATHER_SEGS, "%s: %d segments (at most %d)", who, a->nseg, GATHER_SEGS);
  if (a->exact)
    SN_REQUIRE(N == Nc && E == Ec && B == Bc && S == Sc, "%s: exact mode needs capacities equal to the totals (N %lld / %lld, E %lld / "
               "%lld, B %lld / %lld, S %lld / %lld)", who, (long long)N, (long long)Nc, (long long)E, (long long)Ec, (long long)B,
               (long long)Bc, (long long)S, (long long)Sc);
  else
    SN_REQUIRE(N < Nc && E <= Ec && B < Bc && S <= Sc, "%s: batch (N %lld, E %lld, B %lld, S %lld) does not fit the bucket "
               "(N_cap %lld > N, E_cap %lld, B_cap %lld > B, S_cap %lld)", who, (long long)N, (long long)E, (long long)B, (long long)S,
               (long long)Nc, (long long)Ec, (long long)Bc, (long long)Sc);
  SN_REQUIRE(Nc < (1ll << 31) && Ec < (1ll << 31) && Bc < (1ll << 31) && Sc < (1ll << 31), "%s: capacities exceed int32", who);
  SN_REQUIRE(a->node_ptr && a->edge_ptr && a->status && (B == 0 || a->index), "%s: null offset table, index or status block", who);
  SN_REQUIRE(((reinterpret_cast<uintptr_t>(a->node_ptr) | reinterpret_cast<uintptr_t>(a->edge_ptr) |
               reinterpret_cast<uintptr_t>(a->eig_ptr) | reinterpret_cast<uintptr_t>(a->index)) & 7) == 0 &&
             ((reinterpret_cast<uintptr_t>(a->status) | reinterpret_cast<uintptr_t>(a->counts) |
               reinterpret_cast<uintptr_t>(a->count_error)) & 3) == 0, "%s: offset tables / index must be 8-byte, status words 4-byte aligned", who);
  SN_REQUIRE(a->S == 0 || a->eig_ptr, "%s: S > 0 without eig_ptr", who);
  SN_REQUIRE(!a->counts || a->ncounts == 3 || a->ncounts == 4, "%s: the count block has 3 or 4 words", who);

  GatherTab tb{};
  int64_t chunks = 0;
  for (int i = 0; i < a->nseg; ++i) {
    const sn_store_seg& s = a->seg[i];
    SN_REQUIRE(s.kind >= 0 && s.kind <= 3 && s.op >= SN_GATHER_COPY && s.op <= SN_GATHER_NODE_COUNT, "%s: segment %d: kind %d / op %d",
               who, i, s.kind, s.op);
    SN_REQUIRE(s.row_bytes > 0 && s.row_bytes % 4 == 0, "%s: segment %d: rows of %lld bytes (rows must be whole 4-byte words)", who, i,
               (long long)s.row_bytes);
    const int64_t rows = s.kind == KIND_NODE ? Nc : s.kind == KIND_EDGE ? Ec : s.kind == KIND_EIG ? Sc : Bc;
    const int64_t used = s.kind == KIND_NODE ? N : s.kind == KIND_EDGE ? E : s.kind == KIND_EIG ? S : B;
    const int64_t ntot = rows * (s.row_bytes / 4);
    SN_REQUIRE(ntot < (1ll << 31), "%s: segment %d: capacity of %lld words exceeds int32", who, i, (long long)ntot);
    if (ntot == 0) continue;
    const bool reads = s.op == SN_GATHER_COPY || s.op == SN_GATHER_ENDPOINT;
    const int wide = s.op == SN_GATHER_ENDPOINT || s.op == SN_GATHER_GRAPH_ID || s.op == SN_GATHER_NODE_COUNT;   // int64 rows
    SN_REQUIRE(s.dst, "%s: segment %d: null capacity buffer", who, i);
    SN_REQUIRE(!reads || used == 0 || s.src, "%s: segment %d: null source array", who, i);
    SN_REQUIRE((reinterpret_cast<uintptr_t>(s.dst) & (wide ? 7 : 3)) == 0 && (reinterpret_cast<uintptr_t>(s.src) & (wide ? 7 : 3)) == 0,
               "%s: segment %d: arrays must be %d-byte aligned", who, i, wide ? 8 : 4);
    SN_REQUIRE(!wide || s.row_bytes == 8, "%s: segment %d: op %d writes int64 rows (row_bytes %lld)", who, i, s.op, (long long)s.row_bytes);
    SN_REQUIRE(s.op != SN_GATHER_CONST || s.row_bytes == 4, "%s: segment %d: a constant segment has int32 rows", who, i);
    SN_REQUIRE((s.op != SN_GATHER_ENDPOINT || s.kind == KIND_EDGE) && (s.op != SN_GATHER_GRAPH_ID || s.kind == KIND_NODE) &&
               (s.op != SN_GATHER_NODE_COUNT || s.kind == KIND_GRAPH), "%s: segment %d: op %d on kind %d", who, i, s.op, s.kind);
    SN_REQUIRE(s.kind != KIND_EIG || a->eig_ptr, "%s: segment %d: an eig segment without eig_ptr", who, i);
    GatherSeg& g = tb.s[tb.n++];
    g.src = reads ? static_cast<const uint32_t*>(s.src) : nullptr;
    g.dst = static_cast<uint32_t*>(s.dst);
    g.ntot = (uint32_t)ntot;
    g.rw = (uint32_t)(s.row_bytes / 4);
    g.chunk0 = (uint32_t)chunks;
    g.val = s.val;
    g.kind = (uint8_t)s.kind;
    g.op = (uint8_t)s.op;
    g.svec = s.op == SN_GATHER_COPY && s.src ? (uint8_t)((reinterpret_cast<uintptr_t>(s.src) >> 2) & 3) : (uint8_t)NO_VEC;
    g.dvec = (reinterpret_cast<uintptr_t>(s.dst) & 15) == 0;
    chunks += cdiv(ntot, 4);
  }
  SN_REQUIRE(chunks < (1ll << 31), "%s: %lld chunks exceed int32", who, (long long)chunks);
  tb.exact = a->exact ? 1 : 0;
  tb.chunks = (uint32_t)chunks;
  tb.B = (int)B;
  tb.ncnt = (int)a->ncounts;
  tb.ptr[0] = a->node_ptr;
  tb.ptr[1] = a->edge_ptr;
  tb.ptr[2] = a->eig_ptr;
  tb.index = a->index;
  tb.G = a->G;
  tb.host[0] = N; tb.host[1] = E; tb.host[2] = S;
  tb.cap[0] = Nc; tb.cap[1] = Ec; tb.cap[2] = Sc;
  tb.Bcap = Bc;
  tb.counts = a->counts;
  tb.count_error = a->count_error;
  tb.status = a->status;
  // >= 4 chunks per thread: every workgroup repeats the prefix, so few, busy workgroups; at most one per CU
  int64_t blocks = cdiv(chunks > 0 ? chunks : 1, GATHER_T * 4);
  if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL(k_store_gather, dim3((unsigned)blocks), dim3(GATHER_T), 0, (hipStream_t)stream, tb);
  SN_CHECK_LAUNCH(who);
  return SN_OK;
}
