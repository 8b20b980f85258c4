// gnn_front.hpp — what the GINE stage kernel (fused_gnn.hip) and the front workgroups of the plan launch (plan.hip) share: the
// stage's LDS geometry, the split image, a split-packed weight tile in registers, and the front record with the code that writes it.
#pragma once
#include "fused_common.hpp"

namespace sn {

constexpr int GNN_ROWS = SN_GNN_MAX_NODES;   // 64
constexpr int GNN_WAVES = 8;
constexpr int GNN_EMAX = 192;                // in-edges of one graph staged in LDS
constexpr int GNN_CLS = 16;                  // edge-feature classes per graph whose embeddings stay in LDS for all layers
constexpr int GNN_EEMAX = 96;                // rows of the edge-embedding area (class x layer table, or per-edge staging)
constexpr int GNN_EEPF = (GNN_EEMAX * 32 + GNN_WAVES * 64 - 1) / (GNN_WAVES * 64);   // float4 per thread (d_pad = 128)

// split image: three bf16 planes [64 rows][256 bytes]; inside a row the k-slots of K block kb and lane group g are one 16-byte chunk
// (8 bf16 = channels 32kb + 16(s>>2) + 4g + (s&3)) -> one ds_read_b128 per plane.  Chunk c = 4 kb + g of row r lives at chunk
// c ^ (r & 15) of the row (round 5): a ds_read_b128 is served in groups of 16 lanes — rows {0-3, 12-15} of lane group g with rows
// 4-11 of lane group g + 1 — and with the rows merely staggered (272-byte stride until round 4) every group had two lanes on one
// bank quad: 2 LDS cycles per group instead of 1, 43 % of the kernel's LDS cycles (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE,
// profiles/r04_pmc_sq_detail.txt); the XOR puts the 16 lanes of every group on 16 different quads (stores: unchanged, 2-way).
constexpr int SP_STRIDE = 256;
constexpr int SP_PLANE = GNN_ROWS * SP_STRIDE;
constexpr int SP_IMAGE = 52224;                      // 3 planes (49152 bytes) + room for the Transformer mode's fp32 Q | K | V rows
static_assert(SP_IMAGE >= 3 * SP_PLANE && SP_IMAGE % 16 == 0, "three planes fit an image");
__device__ __forceinline__ int sp_chunk(int row, int c) { return ((c ^ row) & 15) << 4; }   // byte offset of logical chunk c in its row

// the four channels 16*ot + 4g + t of `row` -> the three planes of a split image (exact 3-way split, fused_common.hpp)
__device__ __forceinline__ void sp_store4(unsigned char* img, int row, int ot, int g, f32x4 v) {
  float h[4], m[4], l[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    h[i] = __uint_as_float(__float_as_uint(v[i]) & 0xffff0000u);
    const float r = v[i] - h[i];
    m[i] = __uint_as_float(__float_as_uint(r) & 0xffff0000u);
    l[i] = r - m[i];
  }
  unsigned char* p = img + row * SP_STRIDE + sp_chunk(row, (ot >> 1) * 4 + g) + (ot & 1) * 8;
  *reinterpret_cast<uint2*>(p) = make_uint2(pack_hi16(h[0], h[1]), pack_hi16(h[2], h[3]));
  *reinterpret_cast<uint2*>(p + SP_PLANE) = make_uint2(pack_hi16(m[0], m[1]), pack_hi16(m[2], m[3]));
  *reinterpret_cast<uint2*>(p + 2 * SP_PLANE) = make_uint2(pack_hi16(l[0], l[1]), pack_hi16(l[2], l[3]));
}

// One output tile of a split-packed Linear in registers: NKB x 3 weight fragments + the 3 epilogue vectors.
template <int NKB>
struct WSplit { u32x4 f[NKB * 3]; f32x4 e[SPLIT_EPI]; };

template <int NKB>
__device__ __forceinline__ void wload(WSplit<NKB>& p, const void* wsp, int ot, int lane) {
  constexpr int NFE = 3 * NKB + SPLIT_EPI;
  const __amdgpu_buffer_rsrc_t rs = weight_rsrc(reinterpret_cast<const float*>(wsp), 0x7fffffff);
  const int voff = lane * 16;
  const int base = __builtin_amdgcn_readfirstlane(ot * NFE * 1024);
#pragma unroll
  for (int i = 0; i < 3 * NKB; ++i) p.f[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, base + i * 1024, 0);
#pragma unroll
  for (int j = 0; j < SPLIT_EPI; ++j) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, base + (3 * NKB + j) * 1024, 0);
    p.e[j] = f32x4{__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3])};
  }
}

// the six partial products of one K block, smallest first, on two accumulator chains
__device__ __forceinline__ void mfma_split_kb(u32x4 wh, u32x4 wm, u32x4 wl, const Split8& x, f32x4& a0, f32x4& a1) {
  a1 = mfma_bf(wl, x.h, a1);
  a0 = mfma_bf(wm, x.h, a0);
  a1 = mfma_bf(wh, x.l, a1);
  a0 = mfma_bf(wh, x.m, a0);
  a1 = mfma_bf(wm, x.m, a1);
  a0 = mfma_bf(wh, x.h, a0);
}

template <int NKB>
__device__ __forceinline__ f32x4 mfma_split_tile(const WSplit<NKB>& w, const Split8 (&x)[NKB]) {
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) mfma_split_kb(w.f[3 * kb], w.f[3 * kb + 1], w.f[3 * kb + 2], x[kb], a0, a1);
  return a0 + a1;
}

// rows of the stage kernel's LDS edge-embedding area at width 16 * NT (launch_gnn): what is left of the CU's LDS beside the two split
// images, the fp32 rows and the edge lists, less the zero row behind them
__host__ __device__ inline int gnn_ee_rows(int NT, int edge_words) {
  const size_t LD = 16 * NT + 4;
  const size_t base = (size_t)2 * SP_IMAGE + (size_t)((GNN_ROWS + 1) * LD) * sizeof(float) +
                      (size_t)(GNN_ROWS + 4 + GNN_EMAX * (3 + edge_words) + GNN_CLS) * sizeof(int);
  const size_t lds_cap = 160 * 1024 - 512;
  const size_t room = base < lds_cap ? lds_cap - base : 0;
  int ee_rows = (int)(room / (LD * sizeof(float))) - 1;
  if (ee_rows > GNN_EEMAX) ee_rows = GNN_EEMAX;
  return ee_rows < 0 ? 0 : ee_rows;
}

// ============================================================================ the front record (d = 128, one discrete node and edge column)
// What the GINE stage's prologue derives from the batch and the weights alone, written per graph by the front workgroups of the plan
// launch (plan.hip: front_block) and read by gnn_graph<8, 0, TC, FRONT = true> in one burst of 16-byte loads:
//   [0]      int4   valid | n | ne | ncls
//   [16]     int4 x 64   per node row: in-degree (-1: no such row) | first four source rows, a byte each (a_sr) | their edge classes
//                        (a_er; 255: no such edge) | first in-edge (erow)
//   [1040]   int x 192   esrc: local source row of every in-edge, in-edges by (destination, edge id)
//   [1808]   int x 192   ecls: edge class (rank of the feature value among the values present in the graph)
//   [2576]   float [64][128]   lin_a . encoder(x): the fp32 sums epi_a parks in X1 (rows >= n of the last row tile: +0)
//   [35344]  float [n_layers * ncls][128]   edge-embedding rows, (layer, class) major
constexpr int FR_D = 128;
constexpr int FR_INFO = 16, FR_ESRC = FR_INFO + 16 * GNN_ROWS, FR_ECLS = FR_ESRC + 4 * GNN_EMAX, FR_X1 = FR_ECLS + 4 * GNN_EMAX;
constexpr int FR_EE = FR_X1 + GNN_ROWS * FR_D * 4;
static_assert(FR_X1 % 16 == 0 && FR_EE % 16 == 0, "16-byte loads");
__host__ __device__ inline long long front_stride(int ee_cap) { return (long long)FR_EE + (long long)ee_cap * FR_D * 4; }
// rows of the record's edge-embedding table for a parameter block: every (layer, class) row a graph can need, and no more than the
// stage kernel's LDS table holds (a graph with more runs the stage's own prologue)
inline int front_ee_cap(const sn_gnn_params& P) {
  const int cls = P.edge_vocab < GNN_CLS ? P.edge_vocab : GNN_CLS;
  const int rows = P.n_layers * cls, room = gnn_ee_rows(8, 1);
  return rows < room ? rows : room;
}

struct FrontDev {
  const int64_t* x;          // [N, ldx] atom ids (column 0)
  int ldx;
  const int64_t* edge_attr;  // [E, lde] bond ids (column 0)
  int lde;
  const float* ntab;         // [node_vocab, 128]
  int node_vocab, edge_vocab, n_layers;
  const void* lin_a;
  const float* etab[SN_GNN_MAX_LAYERS];   // [edge_vocab, 128] of every layer
  int ee_rows;               // rows of the stage kernel's LDS table (gnn_ee_rows)
  int ee_cap;                // rows of the record's
  unsigned char* rec;        // [B] records, `stride` bytes each; NULL: no front workgroups
  long long stride;
};

// the class of feature value v among the values `present` in the graph, and the packed first-four in-edges of a node row — the
// words the layer loop keeps in registers (gnn_graph: a_sr, a_er)
__device__ __forceinline__ int front_class(unsigned present, int v) { return __popc(present & ((1u << v) - 1u)); }

// One graph's record: a workgroup of 1024 threads of the plan launch.  Depends on nothing the plan's own workgroups write: the node
// range comes from the batch vector (sorted: checked here too), the in-edges from edge_index[1].  Every index is checked before it
// is used; a graph the record cannot describe gets valid = 0 and nothing else (the stage kernel then runs its own prologue, which
// raises the flags).
__device__ __forceinline__ void front_block(const int64_t* __restrict__ batch, int N, int B, const int64_t* __restrict__ ei, int E,
                                            const FrontDev& F, int gi, int* sm) {
  constexpr int FT = 1024, NPT = 4, EPT = 12;      // PS_NMAX / FT nodes and PS_EMAX / FT edges per thread
  const int t = threadIdx.x;
  unsigned char* rec = F.rec + (size_t)gi * (size_t)F.stride;
  // [0] first node  [1] end node  [2] batch not sorted  [3] in-edges  [4] feature values present  [5] bad node id  [6] bad edge
  __shared__ int s_f[8];
  int* deg = sm;                // [64]
  int* erow = deg + GNN_ROWS;   // [65]
  int* lfill = erow + GNN_ROWS + 4;      // [192] in-edges in arrival order: edge id << 11 | feature value << 6 | source row
  int* lperm = lfill + GNN_EMAX;         // [192] ... by (destination, edge id)
  int* lst = lperm + GNN_EMAX;           // [192] the graph's in-edges as found: destination row << 14 | edge id
  unsigned char* SB = reinterpret_cast<unsigned char*>(lst + GNN_EMAX);    // split image of the encoder rows
  static_assert(((2 * GNN_ROWS + 4 + 3 * GNN_EMAX) * 4) % 16 == 0, "the image is 16-byte aligned");
  if (t < 8) s_f[t] = t == 0 ? N : 0;
  if (t < GNN_ROWS) deg[t] = 0;
  // every global read that needs no other: the batch vector and edge_index[1] (coalesced)
  long long bcur[NPT], bprev[NPT];
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int i = t + k * FT;
    bcur[k] = i < N ? batch[i] : 0;
    bprev[k] = (i < N && i > 0) ? batch[i - 1] : -1;
  }
  long long dv[EPT];
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = t + k * FT;
    dv[k] = e < E ? ei[(long long)E + e] : -1;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int i = t + k * FT;
    if (i < N) {
      if (bprev[k] > bcur[k]) atomicOr(&s_f[2], 1);                         // not sorted: the ranges below mean nothing
      if (bcur[k] == gi && bprev[k] != gi) atomicMin(&s_f[0], i);
      if (bcur[k] != gi && bprev[k] == gi) atomicMax(&s_f[1], i);
      if (bcur[k] == gi && i == N - 1) atomicMax(&s_f[1], N);
    }
  }
  __syncthreads();
  const int gs = s_f[0], n = s_f[1] - gs;
  if (s_f[2] != 0 || n <= 0 || n > GNN_ROWS) {
    if (t == 0) *reinterpret_cast<int4*>(rec) = make_int4(0, 0, 0, 0);
    return;
  }
  const int T = (n + 15) >> 4;
  // the atom ids of my two (row, channel quad) items of the encoder image
  long long xid[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = (t >> 5) + 32 * j;
    xid[j] = row < n ? F.x[(long long)(gs + row) * F.ldx] : 0;
  }
  // ---- the graph's in-edges (sorted batch vector: an edge belongs to the graph of its destination's range), as a list in LDS
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int e = t + k * FT;
    if (e < E && dv[k] >= gs && dv[k] < gs + n) {
      const int slot = atomicAdd(&s_f[3], 1);
      if (slot < GNN_EMAX) lst[slot] = (((int)dv[k] - gs) << 14) | e;        // (e < 2^14: E <= 12288 in a one-launch plan)
    }
  }
  // the encoder rows (DiscreteEncoder, one column): requested under the edge work
  f32x4 nrow[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = (t >> 5) + 32 * j;
    nrow[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (row < n) {
      long long xv = xid[j];
      if ((unsigned long long)xv >= (unsigned long long)F.node_vocab) { xv = 0; atomicOr(&s_f[5], 1); }
      nrow[j] = ld4(F.ntab + xv * FR_D + 4 * (t & 31));
    }
  }
  __syncthreads();
  const int ne = s_f[3];
  if (s_f[5] != 0 || ne > GNN_EMAX) {
    if (t == 0) *reinterpret_cast<int4*>(rec) = make_int4(0, 0, 0, 0);
    return;
  }
  // ---- one in-edge per thread from here on: source, bond id, arrival position in its destination's segment
  int key = 0, dl = 0, pos = 0;
  if (t < ne) {
    const int e = lst[t] & 16383;
    dl = lst[t] >> 14;
    const long long sv = ei[e];
    const long long v = F.edge_attr[(long long)e * F.lde];
    pos = atomicAdd(&deg[dl], 1);
    int src = 0, ev = 0;
    if (sv < gs || sv >= gs + n) atomicOr(&s_f[6], 1);                       // an edge across graphs / out of range
    else src = (int)sv - gs;
    // a bond id outside the table (nn.Embedding raises IndexError) or past the class mask: the stage kernel's own prologue decides
    if ((unsigned long long)v >= (unsigned long long)F.edge_vocab || v >= 32) atomicOr(&s_f[6], 1);
    else { ev = (int)v; atomicOr(reinterpret_cast<unsigned*>(&s_f[4]), 1u << ev); }
    key = (e << 11) | (ev << 6) | src;
  }
  // the encoder image: rows < n split in place, the rest of the last row tile zero
  for (int i = t; i < (16 * T - n) * 48; i += FT) {
    const int row = n + i / 48, c = i % 48;
    *reinterpret_cast<uint4*>(SB + (c >> 4) * SP_PLANE + row * SP_STRIDE + (c & 15) * 16) = make_uint4(0u, 0u, 0u, 0u);
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = (t >> 5) + 32 * j, c4 = t & 31;
    if (row < n) sp_store4(SB, row, c4 >> 2, c4 & 3, nrow[j]);
  }
  __syncthreads();
  if (t < 64) {                 // erow = exclusive scan of the in-degrees (rows >= n: 0 in-edges, erow = ne)
    const int dg = t < n ? deg[t] : 0;
    int inc = dg;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(inc, off, 64);
      if (t >= off) inc += o;
    }
    erow[t] = inc - dg;
    if (t == 63) erow[64] = inc;
  }
  __syncthreads();
  if (t < ne) lfill[erow[dl] + pos] = key;
  __syncthreads();
  // ---- by edge id inside every segment: an in-edge's place is the number of smaller keys (the keys are distinct)
  if (t < ne) {
    const int lo = erow[dl], hi = erow[dl + 1];
    int rank = 0;
    for (int q = lo; q < hi; ++q) rank += lfill[q] < key ? 1 : 0;
    lperm[lo + rank] = key;
  }
  __syncthreads();
  const unsigned present = (unsigned)s_f[4];
  const int ncls = __popc(present);
  if (s_f[6] != 0 || ncls > GNN_CLS || F.n_layers * ncls > F.ee_rows || F.n_layers * ncls > F.ee_cap) {
    if (t == 0) *reinterpret_cast<int4*>(rec) = make_int4(0, 0, 0, 0);
    return;
  }
  // ---- the record
  if (t < GNN_ROWS) {
    int4 info = make_int4(-1, 0, 0, ne);
    if (t < n) {
      const int e_lo = erow[t], dg = erow[t + 1] - e_lo;
      unsigned sr = 0u, er = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int key = lperm[k < dg ? e_lo + k : 0];
        sr |= (unsigned)(k < dg ? (key & 63) : GNN_ROWS) << (8 * k);
        er |= (unsigned)(k < dg ? front_class(present, (key >> 6) & 31) : 255) << (8 * k);
      }
      info = make_int4(dg, (int)sr, (int)er, e_lo);
    }
    reinterpret_cast<int4*>(rec + FR_INFO)[t] = info;
  }
  if (t >= 64 && t < 64 + GNN_EMAX) {
    const int k = t - 64;
    const int key = k < ne ? lperm[k] : 0;
    reinterpret_cast<int*>(rec + FR_ESRC)[k] = key & 63;
    reinterpret_cast<int*>(rec + FR_ECLS)[k] = k < ne ? front_class(present, (key >> 6) & 31) : 0;
  }
  for (int i = t; i < F.n_layers * ncls * (FR_D / 4); i += FT) {
    const int rowi = i / (FR_D / 4), ch = 4 * (i % (FR_D / 4));
    const int l = rowi / ncls, c = rowi - l * ncls;
    unsigned m = present;
    for (int q = 0; q < c; ++q) m &= m - 1u;           // the c-th value present
    const f32x4 v = ld4(F.etab[l] + (long long)__builtin_ctz(m) * FR_D + ch);
    *reinterpret_cast<float4*>(rec + FR_EE + (size_t)i * 16) = make_float4(v[0], v[1], v[2], v[3]);
  }
  // ---- lin_a . encoder rows: wave w takes output tile w & 7 and the row tiles w >> 3, (w >> 3) + 2 — the products and their order
  //      are mfma_split_tile's, K block by K block (this launch has half the stage kernel's registers per lane)
  {
    const int lane = t & 63, w = t >> 6, ot = w & 7, g = lane >> 4, li = lane & 15;
    const __amdgpu_buffer_rsrc_t rs = weight_rsrc(reinterpret_cast<const float*>(F.lin_a), 0x7fffffff);
    const int base = __builtin_amdgcn_readfirstlane(ot * (3 * 4 + SPLIT_EPI) * 1024);
    for (int rt = w >> 3; rt < T; rt += 2) {
      const unsigned char* p = SB + (rt * 16 + li) * SP_STRIDE;
      const int cx = li ^ g;
      f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        const unsigned char* pc = p + (((4 * kb) ^ cx) << 4);
        Split8 x;
        x.h = *reinterpret_cast<const u32x4*>(pc);
        x.m = *reinterpret_cast<const u32x4*>(pc + SP_PLANE);
        x.l = *reinterpret_cast<const u32x4*>(pc + 2 * SP_PLANE);
        const u32x4 wh = __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, base + (3 * kb) * 1024, 0);
        const u32x4 wm = __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, base + (3 * kb + 1) * 1024, 0);
        const u32x4 wl = __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, base + (3 * kb + 2) * 1024, 0);
        mfma_split_kb(wh, wm, wl, x, a0, a1);
      }
      const f32x4 acc = a0 + a1;
      *reinterpret_cast<float4*>(rec + FR_X1 + (size_t)((rt * 16 + li) * FR_D + 16 * ot + 4 * g) * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
  }
  if (t == 0) *reinterpret_cast<int4*>(rec) = make_int4(1, n, ne, ncls);
}

}  // namespace sn
