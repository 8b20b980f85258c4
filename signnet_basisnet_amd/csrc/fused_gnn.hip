// fused_gnn.hip — the GINE network that consumes the positional encoding, whole stack in ONE launch.
// Replaces (eval mode) the tail of SetTransformer.forward — `self.out` Linear+BatchNorm on the slot sum
// (sign_net.py:71) — and GNN.forward (Alchemy/sign_net/model.py:36-64, GINESignNetPyG/core/model.py:44-79):
// input encoder, Linear(cat[x, pos]), nl_gnn x [edge encoder, GINEConv (pyg_gnn_wrapper.py:19-28),
// BatchNorm, ReLU, residual], add-pooling over each graph and the 2-layer output encoder.
//
// This stage has few rows (one per node, no eigenvector-slot factor) and a long dependent chain
// (3 + 2*nl_gnn + 2 Linear layers), so it is latency-bound, not throughput-bound.  Mapping: ONE workgroup of
// 8 waves per graph (n <= 64 nodes) keeps the graph's node rows in LDS for the whole stack:
//   * X1 [64][d_pad+4] fp32 — the layer input h: read by the GINE neighbour sum relu(h_j + e_ji), by the residual and
//     by the pooling;
//   * SA, SB — every Linear's INPUT rows, stored already split into three bf16 planes (the fp32 products are six
//     bf16 partial products, fused_common.hpp §"fp32 GEMMs on the bf16 matrix pipe"): the producer of a value splits
//     it once (5.5 VALU ops) and every consumer wave reads ready-made MFMA operands (ds_read_b128 per plane, K block);
//   * the (output tile, row tile) pairs of a Linear are dealt OUTPUT-TILE MAJOR to the 8 waves, so each weight tile
//     (split-packed, with its epilogue vectors, sn_pack_split_f32) is fetched by exactly one wave — the weight traffic
//     of a Linear is the matrix once per CU; one barrier per Linear;
//   * edges of a graph repeat a handful of feature tuples (ZINC: 3 bond types): their embeddings for every layer are
//     built once into an LDS table indexed by edge class.
//
// Round 4: the same mapping serves two base nets of the DGL tree (GraphPrediction/nets/ZINC_graph_regression), each as ONE launch —
// gnn_graph<NT, MODE>: MODE 1 = gin_net.py (sn_gin_net_fused_f32: no edge term, plain messages, nothing behind the MLP's second Linear,
// a three-Linear readout), MODE 2 = transformer_net.py (sn_transformer_net_fused_f32: hidden 64, every stage a [64, 64] Linear, the edge
// attention one lane per (node, head), the two split images swapping roles per layer).  The mode is a template parameter: the GINE
// instantiations carry none of it.
//
// Front records (gnn_front.hpp): with sn_gnn_fused_front_f32 the part of a graph's prologue that depends on the batch
// and the weights alone — CSR slice, edge classes, table rows, the lin_a stage — arrives ready-made from the plan launch
// (k_gnn_coop<8, 0, true>, gnn_graph_front<TC> of fused_gnn_graph.hpp); the shared pieces (split image, register weight tile) live in
// gnn_front.hpp.
#include "gnn_front.hpp"

namespace sn {

#ifdef SN_PROFILE
static __device__ int g_prof_block = 0;
#undef SN_STAMP
#undef SN_ACCUM
#define SN_STAMP(i) do { if ((int)blockIdx.x == g_prof_block && threadIdx.x == 0) g_prof[i] = clock64(); } while (0)
#define SN_ACCUM(i, t0) do { if ((int)blockIdx.x == g_prof_block && threadIdx.x == 0) g_prof[i] += clock64() - (t0); } while (0)
#endif


struct GnnStruct {
  const void* x;          // int64 [N, ldx] (discrete) or float [N, F]
  int ldx;
  const void* edge_attr;  // int64 [E, lde] (discrete) or float [E, F_e]
  int lde;
  const float* rho_sum;   // [N, d]
  const int32_t* graph_ptr;
  const int32_t* rowptr;
  const int32_t* col;
  const int32_t* eperm;
  int32_t* status;        // status[3] |= 1 if a graph has more than 64 nodes (host falls back)
  float* y;               // [B, n_out]
  int ee_rows;            // rows of the edge-embedding area
  const int32_t* flags_src;   // the batch's flag block [status(8) | bins meta(8)]: read for upstream failures, optionally reported
  int n_flags;
  int32_t* flags_host;
  int rho_ld, rho_w;      // row stride / width of rho_sum (the GINE net: both d; the DGL GIN net: the positional encoding [N, k])
  const void* head_mid;   // DGL GIN net: the middle Linear of MLPReadout (split-packed, (e0, e1) = (1, bias))
  int pool_mean;          // DGL nets: the readout, SN_READOUT_SUM / _MEAN / _MAX
  const unsigned char* front;   // front records of the batch (gnn_front.hpp), written by the plan launch; NULL: none
  long long front_stride;
};



// The (output tile, row tile) pairs a wave owns in one Linear: a contiguous range [t_lo, t_hi) of the flattened index
// t = ot*T + rt (T = row tiles of the graph, <= 4) — OUTPUT-TILE MAJOR, so that a wave works on one output tile (two
// at most) for all the graph's row tiles and every weight fragment is fetched by exactly one wave of the workgroup.
struct TileRange {
  int t_lo, t_hi, T;
  __device__ __forceinline__ bool empty() const { return t_lo >= t_hi; }
  __device__ __forceinline__ void decode(int t, int& ot, int& rt) const { ot = t / T; rt = t - ot * T; }
  __device__ __forceinline__ int first_ot() const { return t_lo / T; }
};


// One Linear over the workgroup's rows.  The wave's TileRange is <= 4 (ot, rt) pairs touching <= 2 output tiles.
// Weight tiles ping-pong between `pre` and `alt`: `pre` holds the first output tile on entry (fetched during the
// previous stage); a second output tile — or, at the end, the NEXT Linear's first tile — is fetched while the current
// one computes.  img: split input image; epi(rt, ot, acc, e0, e1, e2) with e* the tile's epilogue vectors.
template <int NKB, typename Epi>
__device__ __forceinline__ void coop_gemm(WSplit<NKB>& pre, WSplit<NKB>& alt, const void* wsp, const unsigned char* img,
                                          TileRange tr, int lane, Epi epi, const void* next_wsp, TileRange next_tr) {
  if (tr.empty()) {
    if (next_wsp && !next_tr.empty()) wload<NKB>(pre, next_wsp, next_tr.first_ot(), lane);   // idle here: keep the chain going
    return;
  }
  // (the range is laundered per call: its decoded (output tile, row tile) pairs and every LDS address derived from them are wave
  //  constants the compiler would otherwise compute once and keep in registers across all the Linears of the kernel — at NT = 7 they
  //  did not fit and 28 of them lived in a private segment)
  asm volatile("" : "+v"(tr.t_lo), "+v"(tr.t_hi), "+v"(tr.T));
  int ot0, rt0;
  tr.decode(tr.t_lo, ot0, rt0);
  int otl, rtl;
  tr.decode(tr.t_hi - 1, otl, rtl);
  const bool two_ots = otl != ot0;
  const unsigned char* rowbase = img + (lane & 15) * SP_STRIDE;
  auto load_rows = [&](int rt, Split8 (&x)[NKB]) {
    const unsigned char* p = rowbase + rt * 16 * SP_STRIDE;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      const unsigned char* pc = p + sp_chunk(lane & 15, kb * 4 + (lane >> 4));
      x[kb].h = *reinterpret_cast<const u32x4*>(pc);
      x[kb].m = *reinterpret_cast<const u32x4*>(pc + SP_PLANE);
      x[kb].l = *reinterpret_cast<const u32x4*>(pc + 2 * SP_PLANE);
    }
  };
#ifdef SN_PROFILE
  long long ct = clock64();
#endif
  Split8 in[NKB];
  load_rows(rt0, in);
#ifdef SN_PROFILE
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  SN_ACCUM(42, ct);
  ct = clock64();
#endif
  // prefetch: second output tile of this Linear, else the next Linear's first tile
  bool next_in_alt = false;
  if (two_ots) wload<NKB>(alt, wsp, otl, lane);
  else if (next_wsp && !next_tr.empty()) { wload<NKB>(alt, next_wsp, next_tr.first_ot(), lane); next_in_alt = true; }
  bool cur_is_pre = true;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = tr.t_lo + i;
    if (t < tr.t_hi) {
      int ot, rt;
      tr.decode(t, ot, rt);
      if (ot != ot0 && cur_is_pre) {
        cur_is_pre = false;                                   // switch to the second tile (in alt); pre is free again:
        if (next_wsp && !next_tr.empty()) wload<NKB>(pre, next_wsp, next_tr.first_ot(), lane);   // next Linear's first tile
      }
#ifdef SN_PROFILE
      ct = clock64();
#endif
      if (i > 0) load_rows(rt, in);
#ifdef SN_PROFILE
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      SN_ACCUM(42, ct);
      ct = clock64();
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // weights of this tile
      SN_ACCUM(41, ct);
      ct = clock64();
      f32x4 accp = cur_is_pre ? mfma_split_tile<NKB>(pre, in) : mfma_split_tile<NKB>(alt, in);
      asm volatile("" :: "v"(accp));
      SN_ACCUM(43, ct);
      ct = clock64();
      if (cur_is_pre) epi(rt, ot, accp, pre.e[0], pre.e[1], pre.e[2]);
      else epi(rt, ot, accp, alt.e[0], alt.e[1], alt.e[2]);
      SN_ACCUM(44, ct);
#else
      if (cur_is_pre) epi(rt, ot, mfma_split_tile<NKB>(pre, in), pre.e[0], pre.e[1], pre.e[2]);
      else epi(rt, ot, mfma_split_tile<NKB>(alt, in), alt.e[0], alt.e[1], alt.e[2]);
#endif
    }
  }
  if (next_in_alt) {   // single-tile range: the next Linear's first tile sits in alt — hand it over in pre
#pragma unroll
    for (int i = 0; i < 3 * NKB; ++i) pre.f[i] = alt.f[i];
#pragma unroll
    for (int j = 0; j < SPLIT_EPI; ++j) pre.e[j] = alt.e[j];
  }
}

// NT >= 7 (d = 112, 128): every wave owns exactly ONE output tile of every Linear, so the two register tiles simply alternate
// from stage to stage and each is refilled — with the tile of the stage AFTER the next — as soon as its last product and epilogue are
// done.  A tile is then on its way for a whole stage (the barrier, the other register tile's Linear, possibly an aggregation) before
// it is needed; with the ping-pong of coop_gemm it is needed one short stage (~1 us of work per wave) after its issue, and every one of
// the 22 stages waited out most of a memory round trip (fetch-size sweep: DESIGN.md §8).
// kb0: first K block of the operand rows (the Transformer mode's FFN 2 reads the two halves of its 128 hidden channels as K blocks 0-1
// and 2-3 of one image).
template <int NKB, typename Epi>
__device__ __forceinline__ void coop_gemm_roll(WSplit<NKB>& cur, const unsigned char* img, TileRange tr, int lane, Epi epi,
                                               const void* nn_wsp, TileRange nn_tr, int kb0 = 0) {
  if (!tr.empty()) {
    asm volatile("" : "+v"(tr.t_lo), "+v"(tr.t_hi), "+v"(tr.T));     // (see coop_gemm)
    const unsigned char* rowbase = img + (lane & 15) * SP_STRIDE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = tr.t_lo + i;
      if (t < tr.t_hi) {
        int ot, rt;
        tr.decode(t, ot, rt);
        Split8 in[NKB];
        const unsigned char* p = rowbase + rt * 16 * SP_STRIDE;
        int cx = (lane & 15) ^ (lane >> 4) ^ (kb0 << 2);             // my chunk of K block kb: (4 kb) ^ cx
        asm volatile("" : "+v"(cx));                                   // (per pair: else the chunk addresses of all four pairs are kept live)
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
          const unsigned char* pc = p + (((4 * kb) ^ cx) << 4);
          in[kb].h = *reinterpret_cast<const u32x4*>(pc);
          in[kb].m = *reinterpret_cast<const u32x4*>(pc + SP_PLANE);
          in[kb].l = *reinterpret_cast<const u32x4*>(pc + 2 * SP_PLANE);
        }
        epi(rt, ot, mfma_split_tile<NKB>(cur, in), cur.e[0], cur.e[1], cur.e[2]);
      }
    }
  }
  if (nn_wsp != nullptr && !nn_tr.empty()) wload<NKB>(cur, nn_wsp, nn_tr.first_ot(), lane);
}

// coop_gemm_roll for a graph whose row-tile count is a COMPILE-TIME constant (PAIRS; NT = 8: wave w owns output tile w and the row
// tiles 0 .. PAIRS-1): the refill of `cur` is issued INSIDE the last tile product — K block kb's three weight fragments are dead as
// soon as its six MFMAs are issued, so the next tile's fragments of that K block are requested right there, and the epilogue vectors
// behind the epilogue.  With coop_gemm_roll all 15 loads of every wave sit between the last epilogue and the stage's barrier: 8
// waves x 15 KB through the CU's 64 B/clk vector-memory path, ~1.9 k cycles per stage that nothing overlaps
// (profiles/r04_gnn_stage_stamps.txt: 3.6 k cycles of every stage do not depend on the graph's size).  The refill is unconditional
// (`nn_wsp` / `nn_ot` always name a valid tile: a wave without work in the stage after the next fetches one it will not use), so the
// register tile has ONE definition per call — as a branch the woven form made the compiler copy tiles at every join (900 bytes of
// private segment per lane).
template <int NKB, int PAIRS, typename Epi>
__device__ __forceinline__ void coop_gemm_weave(WSplit<NKB>& cur, const unsigned char* img, int ot, int lane, Epi epi,
                                                const void* nn_wsp, int nn_ot) {
  constexpr int NFE = 3 * NKB + SPLIT_EPI;
  const __amdgpu_buffer_rsrc_t rs = weight_rsrc(reinterpret_cast<const float*>(nn_wsp), 0x7fffffff);
  const int voff = lane * 16;
  const int base = __builtin_amdgcn_readfirstlane(nn_ot * NFE * 1024);
  const unsigned char* rowbase = img + (lane & 15) * SP_STRIDE;
#pragma unroll
  for (int rt = 0; rt < PAIRS; ++rt) {
    Split8 in[NKB];
    const unsigned char* p = rowbase + rt * 16 * SP_STRIDE;
    int cx = (lane & 15) ^ (lane >> 4);
    asm volatile("" : "+v"(cx));                                   // (per pair: see coop_gemm_roll)
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      const unsigned char* pc = p + (((4 * kb) ^ cx) << 4);
      in[kb].h = *reinterpret_cast<const u32x4*>(pc);
      in[kb].m = *reinterpret_cast<const u32x4*>(pc + SP_PLANE);
      in[kb].l = *reinterpret_cast<const u32x4*>(pc + 2 * SP_PLANE);
    }
    if (rt + 1 < PAIRS) {
      epi(rt, ot, mfma_split_tile<NKB>(cur, in), cur.e[0], cur.e[1], cur.e[2]);
      __builtin_amdgcn_sched_barrier(0);                           // pairs stay sequential (registers)
    } else {
      f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        const u32x4 wh = cur.f[3 * kb], wm = cur.f[3 * kb + 1], wl = cur.f[3 * kb + 2];
        a1 = mfma_bf(wl, in[kb].h, a1);
        a0 = mfma_bf(wm, in[kb].h, a0);
        a1 = mfma_bf(wh, in[kb].l, a1);
        a0 = mfma_bf(wh, in[kb].m, a0);
        a1 = mfma_bf(wm, in[kb].m, a1);
        a0 = mfma_bf(wh, in[kb].h, a0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 3; ++j) cur.f[3 * kb + j] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, base + (3 * kb + j) * 1024, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      epi(rt, ot, a0 + a1, cur.e[0], cur.e[1], cur.e[2]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < SPLIT_EPI; ++j) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, base + (3 * NKB + j) * 1024, 0);
        cur.e[j] = f32x4{__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3])};
      }
    }
  }
}

// DGL = true: the GraphPrediction tree's GIN net on the same mapping (nets/ZINC_graph_regression/gin_net.py:83-126 in eval mode):
//   h = embedding_h[atom] + embedding_p(p)          -> the input stage with lin_a = I, lin_b = embedding_p (bias in e0), "slot sum" = p
//   L x  h = MLP((1 + eps) h_i + sum_{j -> i} h_j)  -> no edge term and no ReLU in the message; Linear . ReLU . [BN folded] . Linear,
//                                                      nothing behind the second Linear (no BatchNorm, ReLU or residual)
//   readout sum / mean, MLPReadout (three Linears)  -> one more head stage (S.head_mid)
// MODE 2: the DGL tree's sparse graph Transformer on the same mapping (transformer_net.py:88-140 with layers/transformer.py:150-312,
// eval mode, d = 64, 8 heads; all stages are [64, 64] Linears — NT = 4):
//   per layer  Q, K, V (fp32 rows parked in the OTHER split image's space) -> one lane per (node, head): the edge attention of
//   sn_edge_attention_f32 over the node's in-edges, E_ij read from the [E, L*d] projection in global memory -> O_h + x, BatchNorm ->
//   FFN 1 (two 64-column halves of the 128 hidden channels) -> FFN 2 (two 64-deep halves, the first one's sums parked in fp32) + x1,
//   BatchNorm.  The two split images swap roles every layer (operand in one, Q | K | V / the next operand in the other).
// The eight stage matrices of layer l are layers[l].etab[0..7] = Q, K, V, O_h, FFN1[:64], FFN1[64:], FFN2[:, :64], FFN2[:, 64:]
// (w1s / w2s repeat etab[0] / etab[1]: what the input stage prefetches).
// TC > 0 (the GINE net at NT = 8 only): the graph's row-tile count as a compile-time constant — the node-row Linears run on
// coop_gemm_weave (the kernel dispatches on ceil(n / 16)).
#define GNN_FRONT 0
#include "fused_gnn_graph.hpp"
#undef GNN_FRONT
#define GNN_FRONT 1
#include "fused_gnn_graph.hpp"
#undef GNN_FRONT

// FRONT: the launch has front records (sn_gnn_fused_front_f32); a graph whose record is not valid runs the in-kernel prologue.
template <int NT, int MODE = 0, bool FRONT = false>
__global__ __launch_bounds__(GNN_WAVES * 64, 2) void k_gnn_coop(GnnStruct S, sn_gnn_params P) {
  static_assert(!FRONT || (NT == 8 && MODE == 0), "front records: the NT = 8 GINE kernel");
  if constexpr (FRONT) {
    const int n = S.graph_ptr[blockIdx.x + 1] - S.graph_ptr[blockIdx.x];
    const int4 hdr = *reinterpret_cast<const int4*>(S.front + (size_t)blockIdx.x * (size_t)S.front_stride);
    const bool have = hdr.x == 1 && hdr.y == n && hdr.z >= 0 && hdr.z <= GNN_EMAX && hdr.w >= 0 && hdr.w <= GNN_CLS &&
                      P.n_layers * hdr.w <= S.ee_rows;
    // (a graph without a valid record: the general row-tile form — the four compile-time forms beside the four below did not fit
    //  the register file; same products in the same order)
    const int T = __builtin_amdgcn_readfirstlane(have ? (n + 15) >> 4 : (n > 0 && n <= GNN_ROWS ? 0 : -1));
    switch (T) {
      case 1: gnn_graph_front<1>(S, P, hdr.z, hdr.w); break;
      case 2: gnn_graph_front<2>(S, P, hdr.z, hdr.w); break;
      case 3: gnn_graph_front<3>(S, P, hdr.z, hdr.w); break;
      case 4: gnn_graph_front<4>(S, P, hdr.z, hdr.w); break;
      case 0: gnn_graph<NT, MODE, 0>(S, P); break;
      default:                                          // an empty / oversize graph: a NaN output row and its flag
        if (threadIdx.x == 0) atomicOr(&S.status[3], n > GNN_ROWS ? 1 : 8);
        if ((int)threadIdx.x < P.n_out) S.y[(int64_t)blockIdx.x * P.n_out + threadIdx.x] = __uint_as_float(0x7fc00000u);
        break;
    }
  } else if constexpr (NT == 8 && MODE == 0) {
    // one instantiation per row-tile count from two on (a graph's nodes: 17-32, 33-48, 49-64; see coop_gemm_weave) — with a fourth
    // one for 1-16 nodes in the same kernel the compiler's allocation ended in 2.3 KB of private segment per lane; such a graph runs
    // the general form (its chain is the shortest of the batch anyway)
    const int n = S.graph_ptr[blockIdx.x + 1] - S.graph_ptr[blockIdx.x];
    switch ((n + 15) >> 4) {
      case 1: gnn_graph<NT, MODE, 1>(S, P); break;
      case 2: gnn_graph<NT, MODE, 2>(S, P); break;
      case 3: gnn_graph<NT, MODE, 3>(S, P); break;
      case 4: gnn_graph<NT, MODE, 4>(S, P); break;
      default:                                          // an empty / oversize graph: a NaN output row and its flag
        if (threadIdx.x == 0) atomicOr(&S.status[3], n > GNN_ROWS ? 1 : 8);
        if ((int)threadIdx.x < P.n_out) S.y[(int64_t)blockIdx.x * P.n_out + threadIdx.x] = __uint_as_float(0x7fc00000u);
        break;
    }
  } else {
    gnn_graph<NT, MODE>(S, P);
  }
  // Flag report by the last workgroup to finish.  The FRONT form carries none: a plan with front records is a one-launch plan, whose
  // own workgroups report the same verdicts in the first microseconds of the forward (sn_plan_early) — a launch with front records
  // and flags_host is served by the form below (gnn_fused_impl).
  if constexpr (!FRONT) {
    if (S.flags_host != nullptr) {
      __syncthreads();
      if (threadIdx.x < 64) {                                         // wave 0
        int last = 0;
        if (threadIdx.x == 0) {
          __threadfence();                                            // my flag updates are visible device-wide
          last = atomicAdd(&S.status[4], 1) == (int)gridDim.x - 1;    // every other workgroup has passed its fence
        }
        if (__shfl(last, 0, 64)) {
          __threadfence();
          // one word per lane (n_flags <= 64): one load and one store in flight per lane instead of n_flags dependent round trips
          // over the host link; the fence below waits for all of the wave's stores before lane 0 publishes the ready word
          if ((int)threadIdx.x < S.n_flags)
            S.flags_host[threadIdx.x] = __hip_atomic_load(&S.flags_src[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __threadfence_system();
          if (threadIdx.x == 0)                                       // "ready": a host polling this word sees the flags
            __hip_atomic_store(&S.flags_host[S.n_flags], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
      }
    }
  }
}

template <int NT, int MODE = 0, bool FRONT = false>
static int launch_gnn(const GnnStruct& S, const sn_gnn_params& P, int64_t B, hipStream_t st) {
  constexpr bool DGL = MODE != 0;
  constexpr int LD = 16 * NT + 4;
  const size_t base = (size_t)2 * SP_IMAGE + (size_t)((GNN_ROWS + 1) * LD) * sizeof(float) +
                      (size_t)(GNN_ROWS + 4 + GNN_EMAX * (3 + (P.n_layers > 0 ? P.edge_nf : 0)) + GNN_CLS) * sizeof(int);
  const size_t lds_cap = 160 * 1024 - 512;     // the kernel also has a few bytes of static LDS (__syncthreads_count)
  const int ee_rows = gnn_ee_rows(NT, P.n_layers > 0 ? P.edge_nf : 0);     // (one more row behind them: the zero row a missing in-edge reads)
  GnnStruct S2 = S;
  S2.ee_rows = MODE == 2 ? GNN_ROWS : ((!DGL && P.n_layers > 0) ? ee_rows : 0);        // (Transformer mode: the fp32 partial-sum image)
  const size_t lds = base + (size_t)(S2.ee_rows + 1) * LD * sizeof(float);
  static bool init = false;
  if (!init) {
    const size_t lds_max = lds_cap;
    if (lds_max > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(k_gnn_coop<NT, MODE, FRONT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds_max) != hipSuccess)
      return fail(SN_ERR_LAUNCH, "sn_gnn_fused_f32: cannot raise the dynamic LDS limit to %zu", lds_max);
    init = true;
  }
  hipLaunchKernelGGL((k_gnn_coop<NT, MODE, FRONT>), dim3((unsigned)B), dim3(GNN_WAVES * 64), lds, st, S2, P);
  return SN_OK;
}

}  // namespace sn

using namespace sn;

#ifdef SN_PROFILE
extern "C" int sn_prof_read_gnn(long long* host) { return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_prof), sizeof(long long) * 64); }
extern "C" int sn_prof_set_block(int b) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_prof_block), &b, sizeof(int)); }
#endif

static int gnn_fused_impl(const sn_gnn_params* params, const void* x, int ldx, const void* edge_attr, int lde,
                          const float* rho_sum, const int32_t* graph_ptr, int64_t B, const int32_t* rowptr,
                          const int32_t* col, const int32_t* eperm, int32_t* status, float* y,
                          const int32_t* flags_src, int n_flags, int32_t* flags_host, const void* front, void* stream) {
  SN_REQUIRE(params && x && rho_sum && graph_ptr && rowptr && status && y && B >= 0, "sn_gnn_fused_f32: null pointer");
  const sn_gnn_params& P = *params;
  SN_REQUIRE(P.d > 0 && P.d <= 128, "sn_gnn_fused_f32: hidden width %d not in (0, 128]", P.d);
  SN_REQUIRE(P.n_layers >= 0 && P.n_layers <= SN_GNN_MAX_LAYERS, "sn_gnn_fused_f32: %d layers unsupported", P.n_layers);
  SN_REQUIRE(P.n_out >= 1 && P.n_out <= 16, "sn_gnn_fused_f32: n_out=%d not in [1,16]", P.n_out);
  SN_REQUIRE(P.node_nf >= 1 && P.node_nf <= (P.node_discrete ? 10 : 16) && ldx >= P.node_nf,
             "sn_gnn_fused_f32: node feature count %d unsupported", P.node_nf);
  SN_REQUIRE(P.n_layers == 0 || (edge_attr && P.edge_nf >= 1 && P.edge_nf <= (P.edge_discrete ? 10 : 16) && lde >= P.edge_nf),
             "sn_gnn_fused_f32: edge feature count %d unsupported", P.edge_nf);
  SN_REQUIRE(P.lin_a && P.lin_b && P.head_w1 && P.head_w2, "sn_gnn_fused_f32: parameters missing");
  SN_REQUIRE(P.rho_out_w == nullptr, "sn_gnn_fused_f32: rho_out_w must be NULL — fold rho.out into lin_b (see signnet_hip.h)");
  if (P.node_discrete) { for (int f = 0; f < P.node_nf; ++f) SN_REQUIRE(P.ntab[f], "sn_gnn_fused_f32: node table %d missing", f); }
  else SN_REQUIRE(P.nw && P.n_scale && P.n_shift, "sn_gnn_fused_f32: node MLP parameters missing");
  for (int l = 0; l < P.n_layers; ++l) {
    const sn_gnn_layer& L = P.layers[l];
    SN_REQUIRE(L.w1s && L.w2s && L.eps, "sn_gnn_fused_f32: layer %d parameters missing", l);
    if (P.edge_discrete) { for (int f = 0; f < P.edge_nf; ++f) SN_REQUIRE(L.etab[f], "sn_gnn_fused_f32: layer %d edge table %d missing", l, f); }
    else SN_REQUIRE(L.ew && L.e_scale && L.e_shift, "sn_gnn_fused_f32: layer %d edge MLP parameters missing", l);
  }
  if (B == 0) return SN_OK;
  SN_REQUIRE(!flags_host || (flags_src && n_flags > 0 && n_flags <= 64), "sn_gnn_fused_f32: flag report needs flags_src and 0 < n_flags <= 64");
  SN_REQUIRE(!flags_src || n_flags >= 1, "sn_gnn_fused_f32: flags_src needs n_flags >= 1");
  SN_REQUIRE((!P.node_discrete || P.node_vocab > 0) && (P.n_layers == 0 || !P.edge_discrete || P.edge_vocab > 0),
             "sn_gnn_fused_f32: node_vocab / edge_vocab (rows of the embedding tables) missing");
  GnnStruct S{x, ldx, edge_attr, lde, rho_sum, graph_ptr, rowptr, col, eperm, status, y, 0, flags_src, n_flags, flags_host,
              P.d, P.d, nullptr, 0, nullptr, 0};
  hipStream_t st = (hipStream_t)stream;
  int rc = SN_OK;
  if (front != nullptr) {
    SN_REQUIRE(P.d == FR_D && P.node_discrete == 1 && P.node_nf == 1 && P.edge_discrete == 1 && P.edge_nf == 1 && P.n_layers >= 1,
               "sn_gnn_fused_front_f32: the front record serves d = 128 with one discrete node and one discrete edge feature column");
    SN_REQUIRE((reinterpret_cast<uintptr_t>(front) & 15) == 0, "sn_gnn_fused_front_f32: the record buffer must be 16-byte aligned");
  }
  // (front records + flags_host: the form without records below — it carries the in-kernel report, and its outputs are the same bits)
  if (front != nullptr && flags_host == nullptr) {
    S.front = reinterpret_cast<const unsigned char*>(front);
    S.front_stride = front_stride(front_ee_cap(P));
    rc = launch_gnn<8, 0, true>(S, P, B, st);
    if (rc != SN_OK) return rc;
    SN_CHECK_LAUNCH("sn_gnn_fused_front_f32");
    return SN_OK;
  }
  switch ((P.d + 15) / 16) {
    case 1: rc = launch_gnn<1>(S, P, B, st); break;
    case 2: rc = launch_gnn<2>(S, P, B, st); break;
    case 3: rc = launch_gnn<3>(S, P, B, st); break;
    case 4: rc = launch_gnn<4>(S, P, B, st); break;
    case 5: rc = launch_gnn<5>(S, P, B, st); break;
    case 6: rc = launch_gnn<6>(S, P, B, st); break;
    case 7: rc = launch_gnn<7>(S, P, B, st); break;
    default: rc = launch_gnn<8>(S, P, B, st); break;
  }
  if (rc != SN_OK) return rc;
  SN_CHECK_LAUNCH("sn_gnn_fused_f32");
  return SN_OK;
}

extern "C" int sn_gnn_fused_f32(const sn_gnn_params* params, const void* x, int ldx, const void* edge_attr, int lde,
                                const float* rho_sum, const int32_t* graph_ptr, int64_t B, const int32_t* rowptr,
                                const int32_t* col, const int32_t* eperm, int32_t* status, float* y,
                                const int32_t* flags_src, int n_flags, int32_t* flags_host, void* stream) {
  return gnn_fused_impl(params, x, ldx, edge_attr, lde, rho_sum, graph_ptr, B, rowptr, col, eperm, status, y, flags_src, n_flags,
                        flags_host, nullptr, stream);
}

// The same with the batch's front records (sn_batch_plan_front): a graph with a valid record starts at the slot sum and lin_b.
extern "C" int sn_gnn_fused_front_f32(const sn_gnn_params* params, const void* x, int ldx, const void* edge_attr, int lde,
                                      const float* rho_sum, const int32_t* graph_ptr, int64_t B, const int32_t* rowptr,
                                      const int32_t* col, const int32_t* eperm, int32_t* status, float* y,
                                      const int32_t* flags_src, int n_flags, int32_t* flags_host, const void* front, void* stream) {
  SN_REQUIRE(front, "sn_gnn_fused_front_f32: null record buffer");
  return gnn_fused_impl(params, x, ldx, edge_attr, lde, rho_sum, graph_ptr, B, rowptr, col, eperm, status, y, flags_src, n_flags,
                        flags_host, front, stream);
}

// The DGL tree's GIN net (gin_net.py:83-126, eval mode) on the same per-graph stage kernel: see gnn_graph<NT, DGL = true>.
extern "C" int sn_gin_net_fused_f32(const sn_gnn_params* params, const void* head_mid, int pool_mean, const int64_t* atom, const float* p,
                                    int ldp, int kp, const int32_t* graph_ptr, int64_t B, const int32_t* rowptr, const int32_t* col,
                                    const int32_t* eperm, int32_t* status, float* y, const int32_t* flags_src, int n_flags, void* stream) {
  SN_REQUIRE(params && head_mid && atom && p && graph_ptr && rowptr && col && eperm && status && y && B >= 0, "sn_gin_net_fused_f32: null pointer");
  const sn_gnn_params& P = *params;
  SN_REQUIRE(P.d > 0 && P.d <= 128 && (P.d & 3) == 0, "sn_gin_net_fused_f32: padded hidden width %d must be a multiple of 4 in (0, 128]", P.d);
  SN_REQUIRE(P.n_layers >= 1 && P.n_layers <= SN_GNN_MAX_LAYERS, "sn_gin_net_fused_f32: %d layers unsupported", P.n_layers);
  SN_REQUIRE(P.n_out >= 1 && P.n_out <= 16, "sn_gin_net_fused_f32: n_out=%d not in [1,16]", P.n_out);
  SN_REQUIRE(P.node_discrete == 1 && P.node_nf == 1 && P.ntab[0] && P.node_vocab > 0, "sn_gin_net_fused_f32: one atom-type table expected");
  SN_REQUIRE(P.edge_nf == 0, "sn_gin_net_fused_f32: the GIN net has no edge term (edge_nf must be 0)");
  SN_REQUIRE(P.lin_a && P.lin_b && P.head_w1 && P.head_w2 && P.rho_out_w == nullptr, "sn_gin_net_fused_f32: parameters missing");
  SN_REQUIRE(kp >= 1 && kp <= P.d && ldp >= kp, "sn_gin_net_fused_f32: positional encoding width %d unsupported", kp);
  for (int l = 0; l < P.n_layers; ++l) {
    const sn_gnn_layer& L = P.layers[l];
    SN_REQUIRE(L.w1s && L.w2s && L.eps, "sn_gin_net_fused_f32: layer %d parameters missing", l);
  }
  SN_REQUIRE(!flags_src || n_flags >= 1, "sn_gin_net_fused_f32: flags_src needs n_flags >= 1");
  if (B == 0) return SN_OK;
  GnnStruct S{atom, 1, nullptr, 0, p, graph_ptr, rowptr, col, eperm, status, y, 0, flags_src, n_flags, nullptr, ldp, kp, head_mid, pool_mean, nullptr, 0};
  hipStream_t st = (hipStream_t)stream;
  int rc = SN_OK;
  switch ((P.d + 15) / 16) {          // (the widths the shipped nets pad to; others round up to the next one at pack time)
    case 1: case 2: case 3: case 4: rc = launch_gnn<4, 1>(S, P, B, st); break;
    case 5: case 6: rc = launch_gnn<6, 1>(S, P, B, st); break;
    default: rc = launch_gnn<8, 1>(S, P, B, st); break;
  }
  if (rc != SN_OK) return rc;
  SN_CHECK_LAUNCH("sn_gin_net_fused_f32");
  return SN_OK;
}

// The DGL tree's sparse graph Transformer (transformer_net.py:88-140, eval mode, hidden 64, 8 heads) on the per-graph stage kernel:
// see gnn_graph<4, MODE = 2>.
extern "C" int sn_transformer_net_fused_f32(const sn_gnn_params* params, const void* head_mid, int pool_mean, const int64_t* atom,
                                            const float* p, int ldp, int kp, const float* e_proj, int lde, const int32_t* graph_ptr, int64_t B,
                                            const int32_t* rowptr, const int32_t* col, const int32_t* eperm, int32_t* status, float* y,
                                            const int32_t* flags_src, int n_flags, void* stream) {
  SN_REQUIRE(params && head_mid && atom && p && e_proj && graph_ptr && rowptr && col && eperm && status && y && B >= 0,
             "sn_transformer_net_fused_f32: null pointer");
  const sn_gnn_params& P = *params;
  SN_REQUIRE(P.d == 64, "sn_transformer_net_fused_f32: hidden width %d (the stage kernel is written for 64 = 8 heads of 8)", P.d);
  SN_REQUIRE(P.n_layers >= 1 && P.n_layers <= SN_GNN_MAX_LAYERS, "sn_transformer_net_fused_f32: %d layers unsupported", P.n_layers);
  SN_REQUIRE(P.n_out >= 1 && P.n_out <= 16, "sn_transformer_net_fused_f32: n_out=%d not in [1,16]", P.n_out);
  SN_REQUIRE(P.node_discrete == 1 && P.node_nf == 1 && P.ntab[0] && P.node_vocab > 0, "sn_transformer_net_fused_f32: one atom-type table expected");
  SN_REQUIRE(P.edge_nf == 0, "sn_transformer_net_fused_f32: edge_nf must be 0 (the edge term is e_proj)");
  SN_REQUIRE(P.lin_a && P.lin_b && P.head_w1 && P.head_w2 && P.rho_out_w == nullptr, "sn_transformer_net_fused_f32: parameters missing");
  SN_REQUIRE(kp >= 1 && kp <= P.d && ldp >= kp && lde >= P.n_layers * P.d && (lde & 3) == 0 && (reinterpret_cast<uintptr_t>(e_proj) & 15) == 0,
             "sn_transformer_net_fused_f32: positional encoding / edge projection shapes");
  for (int l = 0; l < P.n_layers; ++l) {
    const sn_gnn_layer& L = P.layers[l];
    for (int j = 0; j < 8; ++j) SN_REQUIRE(L.etab[j], "sn_transformer_net_fused_f32: layer %d stage matrix %d missing", l, j);
    SN_REQUIRE(L.w1s == (const void*)L.etab[0] && L.w2s == (const void*)L.etab[1], "sn_transformer_net_fused_f32: w1s / w2s must repeat etab[0] / etab[1]");
  }
  SN_REQUIRE(!flags_src || n_flags >= 1, "sn_transformer_net_fused_f32: flags_src needs n_flags >= 1");
  if (B == 0) return SN_OK;
  GnnStruct S{atom, 1, e_proj, lde, p, graph_ptr, rowptr, col, eperm, status, y, 0, flags_src, n_flags, nullptr, ldp, kp, head_mid, pool_mean, nullptr, 0};
  const int rc = launch_gnn<4, 2>(S, P, B, (hipStream_t)stream);
  if (rc != SN_OK) return rc;
  SN_CHECK_LAUNCH("sn_transformer_net_fused_f32");
  return SN_OK;
}
