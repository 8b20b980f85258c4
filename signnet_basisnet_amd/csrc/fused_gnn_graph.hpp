// fused_gnn_graph.hpp — gnn_graph<NT, MODE, TC>, one graph of the stage kernel of fused_gnn.hip, which includes this text TWICE:
// with GNN_FRONT 0 (the function as ever) and with GNN_FRONT 1 — gnn_graph_front<TC>, the NT = 8 GINE form for a graph with a valid
// front record (gnn_front.hpp; fr_ne in-edges, fr_ncls edge classes): everything the prologue derives from the batch and the weights
// alone, the parked sums of the lin_a stage included, is loaded from the record in one burst, and the chain starts at the slot sum
// and lin_b.  Everything from lin_b on is the same text.  (A template parameter and `if constexpr` would do — but the block scope
// that puts around the in-kernel prologue changes the lifetimes the register allocator sees, and the 254-VGPR headline instantiation
// then ends with 2.2 KB of private segment per lane.)  No include guard on purpose.
#if GNN_FRONT
template <int TC>
__device__ __forceinline__ void gnn_graph_front(const GnnStruct& S, const sn_gnn_params& P, int fr_ne, int fr_ncls) {
  constexpr int NT = 8, MODE = 0;
  constexpr bool FRONT = true;
#else
template <int NT, int MODE = 0, int TC = 0>
__device__ __forceinline__ void gnn_graph(const GnnStruct& S, const sn_gnn_params& P) {
  constexpr bool FRONT = false;
  constexpr int fr_ne = 0;
#endif
  constexpr bool DGL = MODE != 0, TF = MODE == 2;
  static_assert(TC == 0 || (NT == 8 && MODE == 0), "compile-time row tiles: the GINE net at NT = 8");
  static_assert(!FRONT || TC > 0, "the front record serves the NT = 8 GINE instantiations");
  static_assert(!TF || NT == 4, "the Transformer mode is written for d = 64");
  constexpr int D = 16 * NT;
  constexpr int LD = D + 4;
  constexpr int NKB = (NT + 1) / 2;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  unsigned char* SA = lds_raw;                                   // split image: slot sum, then u, then the pooled row
  unsigned char* SB = lds_raw + SP_IMAGE;                        // split image: encoder output, pos, hidden rows
  float* X1 = reinterpret_cast<float*>(lds_raw + 2 * SP_IMAGE);  // [64 + 1][LD] fp32: h; row 64 stays zero (what a missing in-edge reads)
  int* erow = reinterpret_cast<int*>(X1 + (GNN_ROWS + 1) * LD);  // [65]  CSR row pointers local to the graph
  int* esrc = erow + GNN_ROWS + 4;                               // [GNN_EMAX] local source row of every in-edge
  int* efeat = esrc + GNN_EMAX;                                  // [GNN_EMAX][edge_nf] feature words (int idx / float)
  int* ecls = efeat + GNN_EMAX * (P.n_layers > 0 ? P.edge_nf : 0);   // [GNN_EMAX] feature class of every in-edge
  int* elead = ecls + GNN_EMAX;                                     // [GNN_EMAX] first edge with the same features (scratch)
  int* cedge = elead + GNN_EMAX;                                    // [GNN_CLS]  representative edge of every class
  float* EE = reinterpret_cast<float*>(cedge + GNN_CLS);           // [ee_rows][LD] edge embeddings (per class x layer, or per edge)
  float* PART = EE;                                                  // Transformer mode (no edge tables): [64][LD] fp32 sums of FFN 2's first half
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, li = lane & 15;
  const int gi = blockIdx.x;
  SN_STAMP(0);
#ifdef SN_PROFILE
  if ((int)blockIdx.x == g_prof_block && threadIdx.x == 0) for (int i = 8; i < 20; ++i) g_prof[i] = 0;
  long long pt = 0;
#endif
  WSplit<NKB> pre, alt;
  const int gs = S.graph_ptr[gi], n = S.graph_ptr[gi + 1] - gs;
  // a graph that cannot be evaluated gets a NaN output row (never uninitialised memory): see sn_gnn_fused_f32
  auto give_up = [&](int bit) {
    if (threadIdx.x == 0 && bit) atomicOr(&S.status[3], bit);
    if ((int)threadIdx.x < P.n_out) S.y[(int64_t)gi * P.n_out + threadIdx.x] = __uint_as_float(0x7fc00000u);
  };
  // earlier stages of this batch failed (malformed batch: status[0]; phi / rho bins not laid out: meta[1], meta[5])
  if (S.flags_src != nullptr && (S.flags_src[0] != 0 || (S.n_flags >= 16 && (S.flags_src[9] != 0 || S.flags_src[13] != 0)))) { give_up(0); return; }
  if (n <= 0) { give_up(8); return; }          // (a graph without nodes: flagged — the layer path evaluates it as the reference does)
  if (n > GNN_ROWS) { give_up(1); return; }
  const int e_base = FRONT ? 0 : S.rowptr[gs];
  const int ne = FRONT ? fr_ne : S.rowptr[gs + n] - e_base;   // (checked below, behind the loads that need `gs` only)
  const int d = P.d;
  // block-wide facts of the prologue: [0] a discrete feature id of this graph lies outside its embedding table, [1] an edge feature
  // value the small class table cannot index, [2] bit v: edge feature value v occurs (one discrete edge feature column)
  __shared__ unsigned s_pro[3];
  if (threadIdx.x == 0) { s_pro[0] = 0u; s_pro[1] = 0u; s_pro[2] = 0u; }
  const int T = TC > 0 ? TC : (n + 15) >> 4;                // row tiles (1..4)
  const int ntile = T * NT;
  TileRange tr;                                               // my share of every node-row Linear (output-tile major)
  tr.T = T;
  if constexpr (GNN_WAVES % NT == 0) {
    // NT divides the wave count: GNN_WAVES / NT waves share an output tile and split its row tiles — every wave stays on ONE output
    // tile for any T (what coop_gemm_roll needs), with at most ceil(T / (GNN_WAVES / NT)) pairs
    constexpr int WPO = GNN_WAVES / NT;
    const int ot = wave / WPO, h = wave % WPO, per = (T + WPO - 1) / WPO;
    tr.t_lo = ot * T + (h * per < T ? h * per : T);
    tr.t_hi = ot * T + ((h + 1) * per < T ? (h + 1) * per : T);
  } else {
    const int q = (ntile + GNN_WAVES - 1) / GNN_WAVES;        // pairs per wave (<= T since NT <= 8: at most 2 output tiles)
    tr.t_lo = wave * q < ntile ? wave * q : ntile;
    tr.t_hi = tr.t_lo + q < ntile ? tr.t_lo + q : ntile;
  }
  TileRange hr;                                               // my share of the output encoder (one pooled row tile)
  hr.T = 1;
  hr.t_lo = wave < NT ? wave : NT;
  hr.t_hi = wave < NT ? wave + 1 : NT;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  // Edges of a graph repeat a handful of feature tuples (ZINC: 3 bond types), and an edge's embedding depends on
  // nothing else.  The staging code below groups the graph's edges into classes of identical features; with at
  // most GNN_CLS classes the embeddings of every (layer, class) are built ONCE into LDS (use_tab) and the aggregation
  // reads edge e's embedding as row ecls[e] — no per-edge, per-layer gather.  Otherwise the current layer's
  // per-edge embeddings are staged (use_ee), or gathered directly.
  bool use_tab = false;   // decided after the classes are known
  int ncls = 0;
  bool use_ee = !DGL && P.n_layers > 0 && ne <= S.ee_rows;
  // embedding of edge k, channels [c, c+4) for layer Lq: DiscreteEncoder sum (elements.py:31-37) or MLP(F_e, d, 1)
  auto edge_embed = [&](const sn_gnn_layer& Lq, int k, int c) -> f32x4 {
    const int EF = P.edge_nf;
    f32x4 ef = zero4;
    if (P.edge_discrete) {
      for (int f = 0; f < EF; ++f) {
        const float* trow = Lq.etab[f] + (int64_t)efeat[k * EF + f] * d;
        if ((d & 3) == 0) { if (c < d) ef += ld4(trow + c); }
        else {
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) if (c + qq < d) ef[qq] += trow[c + qq];
        }
      }
    } else {
      f32x4 acc = zero4;
      for (int f = 0; f < EF; ++f) {
        const float a = __int_as_float(efeat[k * EF + f]);
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) acc[qq] += a * Lq.ew[(c + qq) * EF + f];
      }
      ef = relu4(acc * ld4(Lq.e_scale + c) + ld4(Lq.e_shift + c));
    }
    return ef;
  };
  // one layer's embeddings of all the graph's edges: fetched into registers early, parked in LDS between barriers
  f32x4 eepf[GNN_EEPF];
  auto ee_fetch = [&](int l) {
    if (!use_ee || l >= P.n_layers) return;
    const sn_gnn_layer& Lq = P.layers[l];
    int t0 = threadIdx.x;
    asm volatile("" : "+v"(t0));      // (per call: the (edge, channel) pair of every slot is a lane constant the compiler would otherwise
                                      //  keep in registers across the layers — with D/4 not a power of two it is not rematerialised)
#pragma unroll
    for (int i = 0; i < GNN_EEPF; ++i) {
      const int idx = t0 + i * GNN_WAVES * 64;
      eepf[i] = zero4;
      if (idx < ne * (D / 4)) eepf[i] = edge_embed(Lq, idx / (D / 4), 4 * (idx % (D / 4)));
    }
  };
  bool tab_pending = false;    // the class table's rows are in registers (eepf), stored by ee_store() behind the input Linears
  auto ee_store = [&]() {
    if (tab_pending) {
      tab_pending = false;
      int t1 = threadIdx.x;
      asm volatile("" : "+v"(t1));
#pragma unroll
      for (int i = 0; i < GNN_EEPF; ++i) {
        const int idx = t1 + i * GNN_WAVES * 64;
        if (idx < P.n_layers * ncls * (D / 4)) lds_st4(EE + (idx / (D / 4)) * LD + 4 * (idx % (D / 4)), eepf[i]);
      }
      return;
    }
    if (!use_ee) return;
    int t0 = threadIdx.x;
    asm volatile("" : "+v"(t0));
#pragma unroll
    for (int i = 0; i < GNN_EEPF; ++i) {
      const int idx = t0 + i * GNN_WAVES * 64;
      if (idx < ne * (D / 4)) lds_st4(EE + (idx / (D / 4)) * LD + 4 * (idx % (D / 4)), eepf[i]);
    }
  };

  // one output tile per wave and Linear -> coop_gemm_roll: NT in {1, 2, 4, 8} by the range split above; NT = 7: the wave's share
  // q = ceil(7 T / 8) of the (tile, row tile) pairs equals T for every T <= 4
  constexpr bool ROLL = NT >= 7 || GNN_WAVES % NT == 0;
  static_assert(GNN_WAVES == 8, "the ROLL condition assumes 8 waves");
  TileRange h2;                               // my share of the last Linear (one tile: wave 0)
  h2.T = 1;
  h2.t_lo = 0;
  h2.t_hi = wave == 0 ? 1 : 0;
  // The graph's own inputs are requested FIRST: the memory counter is in-order, so every later wait for one of them would also wait
  // for whatever was issued before it — the two 15 KB weight tiles below.  One CSR row pointer, one in-edge (source, edge id) and up
  // to four float4 of the slot sum per thread cover the whole graph (n <= 64, ne <= 192 < blockDim).
  static_assert(GNN_EMAX <= GNN_WAVES * 64 && GNN_ROWS < GNN_WAVES * 64 && GNN_ROWS * (D / 4) <= 4 * GNN_WAVES * 64, "one pass of the block covers the graph");
  const int tid = threadIdx.x;
#if !GNN_FRONT
  // Round 5: what needs only the graph's first node — CSR row pointers, the slot sum, the node feature ids of my rows — is requested
  // before the in-edge count is even known; the edge lists follow, then the edge features and the node-table rows (as soon as their
  // ids are there), and only then the two 15 KB weight tiles: every wait below names loads issued before them.  The prologue used to be
  // six dependent round trips (graph_ptr, rowptr, edge lists, edge features, class table | node ids, node table): the node side now
  // runs beside the edge side and the class table's rows land under the two input Linears.
  const int rp_v = tid <= n ? S.rowptr[gs + tid] : 0;
  const int rho_ld = S.rho_ld, rho_w = S.rho_w;
  const bool rs_vec = ((rho_ld | rho_w) & 3) == 0;
  f32x4 rs_v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    rs_v[j] = zero4;
    const int i = tid + j * GNN_WAVES * 64;
    if (rs_vec && i < n * (D / 4)) {
      const int rr = i / (D / 4), c4 = i % (D / 4);
      if (4 * c4 < rho_w) rs_v[j] = ld4(S.rho_sum + (int64_t)(gs + rr) * rho_ld + 4 * c4);
    }
  }
  const bool xid_pref = P.node_discrete && P.node_nf == 1 && (d & 3) == 0;     // one id column: the ids of my (<= 4) rows, up front
  long long xid[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    xid[i] = -1;
    const int t = tr.t_lo + i;
    if (xid_pref && t < tr.t_hi) {
      int ot, rt;
      tr.decode(t, ot, rt);
      if (rt * 16 + li < n) xid[i] = reinterpret_cast<const int64_t*>(S.x)[(int64_t)(gs + rt * 16 + li) * S.ldx];
    }
  }
  if (ne > GNN_EMAX) { give_up(2); return; }
  const int src_v = tid < ne ? S.col[e_base + tid] : 0;
  const int eid_v = tid < ne ? S.eperm[e_base + tid] : 0;
  SN_STAMP(30);
  // ---------------------------------------------------------------- clear the split images (K padding must read as 0)
  for (int i = threadIdx.x; i < 2 * SP_IMAGE / 16; i += GNN_WAVES * 64)
    reinterpret_cast<uint4*>(lds_raw)[i] = make_uint4(0u, 0u, 0u, 0u);
  if ((int)threadIdx.x < LD) { X1[GNN_ROWS * LD + threadIdx.x] = 0.f; EE[S.ee_rows * LD + threadIdx.x] = 0.f; }   // the two zero rows
  lds_barrier();               // (the prologue's flags are initialised)
  SN_STAMP(31);
  // ---------------------------------------------------------------- per-graph CSR + edge data -> LDS (once)
  const bool efast = !DGL && P.n_layers > 0 && P.edge_discrete && P.edge_nf == 1 && (d & 3) == 0;   // classes = the feature values
  int my_ev = 0;
  {
    const int EF = P.edge_nf;
    if (tid <= n) erow[tid] = rp_v - e_base;
    if (tid < ne) {
      const int k = tid;
      esrc[k] = src_v - gs;
      const int eid = eid_v;
      if (TF) ecls[k] = eid;                              // the attention reads E[eid] from global memory
      if (!DGL && P.n_layers > 0) {
        if (P.edge_discrete) {
          const int64_t* ei = reinterpret_cast<const int64_t*>(S.edge_attr) + (int64_t)eid * S.lde;
          for (int f = 0; f < EF; ++f) {
            const int64_t v = ei[f];
            const bool ok = (uint64_t)v < (uint64_t)P.edge_vocab;      // nn.Embedding would raise IndexError: never dereferenced
            efeat[k * EF + f] = ok ? (int)v : 0;
            if (!ok) { atomicOr(&S.status[3], 4); atomicOr(&s_pro[0], 1u); }
            if (efast) {
              my_ev = ok ? (int)v : 0;
              if (my_ev < 32) atomicOr(&s_pro[2], 1u << my_ev); else atomicOr(&s_pro[1], 1u);
            }
          }
        } else {
          const float* ea = reinterpret_cast<const float*>(S.edge_attr) + (int64_t)eid * S.lde;
          for (int f = 0; f < EF; ++f) efeat[k * EF + f] = __float_as_int(ea[f]);
        }
      }
    }
  }
  // the node-table rows of my pairs (their ids were the first loads): in flight during the class work below
  f32x4 nrow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    nrow[i] = zero4;
    const int t = tr.t_lo + i;
    if (xid_pref && t < tr.t_hi && xid[i] != -1) {
      int ot, rt;
      tr.decode(t, ot, rt);
      long long xv = xid[i];
      if ((uint64_t)xv >= (uint64_t)P.node_vocab) { xv = 0; atomicOr(&S.status[3], 4); atomicOr(&s_pro[0], 1u); }
      const int c = 16 * ot + 4 * g;
      if (c < d) nrow[i] = ld4(P.ntab[0] + xv * d + c);
    }
  }
  // (both weight tiles behind every load of the graph's own data; measured and dropped: the first tile right behind the edge lists
  //  — prologue 20.3 k -> 22.5 k cycles — and in front of everything — 23.6 k)
  if (!tr.empty()) {
    wload<NKB>(pre, P.lin_a, tr.first_ot(), lane);                      // in flight while the inputs are staged
    if constexpr (ROLL) wload<NKB>(alt, P.lin_b, tr.first_ot(), lane);
  }
  lds_barrier();               // images cleared, CSR / edge features staged (an LDS-only barrier: the loads above stay in flight)
  SN_STAMP(32);
  // ---------------------------------------------------------------- edge-feature classes (see use_tab above)
  if (efast && s_pro[1] == 0u) {
    // one discrete feature column with small values (ZINC: bond types 1..3): the class of an edge IS its value's rank among the
    // values present — no search over the edges, no further barrier; row (l, c) of the table = layer l's embedding of value c
    const unsigned present = s_pro[2];
    ncls = __popc(present);
    if (tid < ne) ecls[tid] = __popc(present & ((1u << my_ev) - 1u));
    use_tab = ncls <= GNN_CLS && P.n_layers * ncls <= S.ee_rows;
    if (use_tab) {
      use_ee = false;
      tab_pending = true;
      int t0 = threadIdx.x;
      asm volatile("" : "+v"(t0));
#pragma unroll
      for (int i = 0; i < GNN_EEPF; ++i) {
        const int idx = t0 + i * GNN_WAVES * 64;
        eepf[i] = zero4;
        if (idx < P.n_layers * ncls * (D / 4)) {
          const int rowi = idx / (D / 4), ch = 4 * (idx % (D / 4));
          const int l = rowi / ncls, c = rowi - l * ncls;
          unsigned m = present;
          for (int q = 0; q < c; ++q) m &= m - 1u;           // the c-th value present
          if (ch < d) eepf[i] = ld4(P.layers[l].etab[0] + (int64_t)__builtin_ctz(m) * d + ch);
        }
      }
    }
  }
  if (!DGL && P.n_layers > 0 && !tab_pending && !(efast && s_pro[1] == 0u)) {
    const int EF = P.edge_nf;
    // lead = first edge with my feature tuple.  Every thread walks ALL the edges with block-uniform (broadcast) LDS reads and no
    // early exit: the reads pipeline, where a scan that stops at the first match serialises one LDS round trip per candidate and
    // the whole wave waits for the rarest class's first edge.  Leaders of the three edge waves are published as ballots; the dense
    // class id of a leader is the number of leaders before it.
    __shared__ unsigned long long lmask[(GNN_EMAX + 63) / 64];
    int lead = -1;
    if (tid < GNN_EMAX) {                              // whole waves: the ballot below needs every lane of an edge wave
      if (tid < ne) {
        lead = tid;
        if (EF == 1) {
          const int mine = efeat[tid];
#pragma unroll 8
          for (int j = 0; j < ne; ++j) lead = (efeat[j] == mine && j < lead) ? j : lead;
        } else {
          for (int j = 0; j < ne; ++j) {
            bool same = true;
            for (int f = 0; f < EF; ++f) same = same && (efeat[j * EF + f] == efeat[tid * EF + f]);
            lead = (same && j < lead) ? j : lead;
          }
        }
        elead[tid] = lead;
      }
      const unsigned long long m = __ballot(tid < ne && lead == tid);
      if (lane == 0) lmask[tid >> 6] = m;
    }
    __syncthreads();
    ncls = 0;
#pragma unroll
    for (int w = 0; w < (GNN_EMAX + 63) / 64; ++w) ncls += __popcll(lmask[w]);
    if (tid < ne) {
      int c = 0;
#pragma unroll
      for (int w = 0; w < (GNN_EMAX + 63) / 64; ++w) {
        const int below = lead - 64 * w;               // leaders of word w that precede my leader
        const unsigned long long keep = below >= 64 ? ~0ull : (below > 0 ? (1ull << below) - 1 : 0ull);
        c += __popcll(lmask[w] & keep);
      }
      ecls[tid] = c;                                   // dense class id = number of leaders before my leader
      if (lead == tid && c < GNN_CLS) cedge[c] = lead;
    }
    use_tab = ncls <= GNN_CLS && P.n_layers * ncls <= S.ee_rows;
    if (use_tab) use_ee = false;
    __syncthreads();
    if (use_tab) {   // EE[l * ncls + c][:] = embedding of class c's representative edge in layer l (padded channels: 0)
      for (int i = threadIdx.x; i < P.n_layers * ncls * (D / 4); i += GNN_WAVES * 64) {
        const int rowi = i / (D / 4), ch = 4 * (i % (D / 4));
        const int l = rowi / ncls, c = rowi - l * ncls;
        lds_st4(EE + rowi * LD + ch, edge_embed(P.layers[l], cedge[c], ch));
      }
    }
  }
  SN_STAMP(33);
  // ---------------------------------------------------------------- stage the slot sum (rho output), split, in SA
  if (rs_vec) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = tid + j * GNN_WAVES * 64;
      if (i < n * (D / 4)) {
        const int rr = i / (D / 4), c4 = i % (D / 4);
        sp_store4(SA, rr, c4 >> 2, c4 & 3, rs_v[j]);
      }
    }
  } else {
    for (int i = threadIdx.x; i < n * (D / 4); i += GNN_WAVES * 64) {
      const int rr = i / (D / 4), c4 = i % (D / 4);
      f32x4 v = zero4;
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) if (4 * c4 + qq < rho_w) v[qq] = S.rho_sum[(int64_t)(gs + rr) * rho_ld + 4 * c4 + qq];
      sp_store4(SA, rr, c4 >> 2, c4 & 3, v);
    }
  }
  SN_STAMP(34);
  // ---------------------------------------------------------------- input encoder -> SB (model.py:37)
  if (xid_pref) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = tr.t_lo + i;
      if (t < tr.t_hi && xid[i] != -1) {
        int ot, rt;
        tr.decode(t, ot, rt);
        sp_store4(SB, rt * 16 + li, ot, g, nrow[i]);
      }
    }
  } else if (P.node_discrete) {
    for (int t = tr.t_lo; t < tr.t_hi; ++t) {
      int ot, rt;
      tr.decode(t, ot, rt);
      const int row = rt * 16 + li, c = 16 * ot + 4 * g;
      if (row < n) {
        const int64_t* xi = reinterpret_cast<const int64_t*>(S.x) + (int64_t)(gs + row) * S.ldx;
        f32x4 s = zero4;
        for (int f = 0; f < P.node_nf; ++f) {
          int64_t xv = xi[f];
          if ((uint64_t)xv >= (uint64_t)P.node_vocab) { xv = 0; atomicOr(&S.status[3], 4); atomicOr(&s_pro[0], 1u); }    // see the edge features above
          const float* trow = P.ntab[f] + xv * d;
          if ((d & 3) == 0) { if (c < d) s += ld4(trow + c); }
          else {
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) if (c + qq < d) s[qq] += trow[c + qq];
          }
        }
        sp_store4(SB, row, ot, g, s);
      }
    }
  } else {
    // MLP(nfeat, d, 1): Linear(no bias) . BN . ReLU on <= 16 continuous features — VALU, one output tile at a time
    for (int t = tr.t_lo; t < tr.t_hi; ++t) {
      int ot, rt;
      tr.decode(t, ot, rt);
      const int row = rt * 16 + li, c = 16 * ot + 4 * g;
      if (row < n) {
        const float* xr = reinterpret_cast<const float*>(S.x) + (int64_t)(gs + row) * S.ldx;
        f32x4 acc = zero4;
        for (int f = 0; f < P.node_nf; ++f) {
          const float a = xr[f];
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) acc[qq] += a * P.nw[(c + qq) * P.node_nf + f];   // nw: [d_pad, F] row-major
        }
        sp_store4(SB, row, ot, g, relu4(acc * ld4(P.n_scale + c) + ld4(P.n_shift + c)));
      }
    }
  }
  SN_STAMP(35);
  lds_barrier();                           // inputs staged; LDS-only like every later barrier:
  const int graph_bad = (int)s_pro[0];     // (did anyone see a bad feature id)
  SN_STAMP(1);                             // a __syncthreads() would also drain the weight prefetch in flight (vmcnt(0))
#else
  const int graph_bad = 0;                 // (a graph with a valid record has no bad feature id)
#endif
  // (round 5: read here, under the wait for the first weight tile, not in front of layer 0)
  int a_dg[4];
  unsigned a_sr[4], a_er[4];       // four source rows (< 64) / four edge classes or edge ids (< 256), a byte each
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a_dg[i] = -1;
    a_sr[i] = 0u;
    a_er[i] = 0u;
    const int t = tr.t_lo + i;
    if (!FRONT && !TF && t < tr.t_hi && (DGL || use_tab || use_ee)) {
      int ot, rt;
      tr.decode(t, ot, rt);
      const int row = rt * 16 + li;
      if (row < n) {
        const int e_lo = erow[row], dg = erow[row + 1] - e_lo;
        a_dg[i] = dg;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int ei = k < dg ? e_lo + k : 0;
          a_sr[i] |= (unsigned)(k < dg ? esrc[ei] : GNN_ROWS) << (8 * k);              // (a missing in-edge: the zero row of X1 ...
          if (!DGL) a_er[i] |= (unsigned)(k < dg ? (use_tab ? ecls[ei] : ei) : 255) << (8 * k);   //  ... and, marked 255, the zero row of EE)
        }
      }
    }
  }
#if GNN_FRONT
  {
    // ---------------------------------------------------------------- the front record: one burst of 16-byte loads, then rho's rows
    const unsigned char* rec = S.front + (size_t)gi * (size_t)S.front_stride;
    int4 ri[TC];                                               // my rows' packed in-edges
#pragma unroll
    for (int i = 0; i < TC; ++i) ri[i] = reinterpret_cast<const int4*>(rec + FR_INFO)[i * 16 + li];
    int4 rrow = make_int4(0, 0, 0, 0);                         // wave 0: erow; waves 1, 2: esrc, ecls
    uint4 elist = make_uint4(0u, 0u, 0u, 0u);
    if (tid < GNN_ROWS) rrow = reinterpret_cast<const int4*>(rec + FR_INFO)[tid];
    else if (tid < 64 + GNN_EMAX / 4) elist = reinterpret_cast<const uint4*>(rec + FR_ESRC)[tid - 64];
    else if (tid >= 128 && tid < 128 + GNN_EMAX / 4) elist = reinterpret_cast<const uint4*>(rec + FR_ECLS)[tid - 128];
    f32x4 x1v[TC];                                             // the parked lin_a sums: 16 TC rows of 32 quads = TC per thread
#pragma unroll
    for (int j = 0; j < TC; ++j) x1v[j] = ld4(reinterpret_cast<const float*>(rec + FR_X1) + (size_t)(tid + j * GNN_WAVES * 64) * 4);
    ncls = fr_ncls;
    use_tab = true;
    use_ee = false;
    tab_pending = true;                                        // the (layer, class) rows: parked behind lin_b like the in-kernel table
    {
      int t0 = threadIdx.x;
      asm volatile("" : "+v"(t0));
#pragma unroll
      for (int i = 0; i < GNN_EEPF; ++i) {
        const int idx = t0 + i * GNN_WAVES * 64;
        eepf[i] = zero4;
        if (idx < P.n_layers * ncls * (D / 4)) eepf[i] = ld4(reinterpret_cast<const float*>(rec + FR_EE) + (size_t)idx * 4);
      }
    }
    f32x4 rs_v[TC];
#pragma unroll
    for (int j = 0; j < TC; ++j) {
      rs_v[j] = zero4;
      const int i = tid + j * GNN_WAVES * 64;
      if (i < n * (D / 4)) rs_v[j] = ld4(S.rho_sum + (int64_t)(gs + (i / (D / 4))) * S.rho_ld + 4 * (i % (D / 4)));
    }
    wload<NKB>(alt, P.lin_b, wave, lane);
    wload<NKB>(pre, P.n_layers > 0 ? P.layers[0].w1s : P.head_w1, P.n_layers > 0 ? wave : (wave < NT ? wave : NT), lane);
    SN_STAMP(30);
    // LDS: the two zero rows, the rows of the last row tile behind the graph (operand rows of every Linear: defined, zero), the lists
    if ((int)threadIdx.x < LD) { X1[GNN_ROWS * LD + threadIdx.x] = 0.f; EE[S.ee_rows * LD + threadIdx.x] = 0.f; }
    for (int i = tid; i < (16 * TC - n) * 48; i += GNN_WAVES * 64) {
      const int row = n + i / 48, c = i % 48;
      *reinterpret_cast<uint4*>(SA + (c >> 4) * SP_PLANE + row * SP_STRIDE + (c & 15) * 16) = make_uint4(0u, 0u, 0u, 0u);
    }
    if (tid < n) erow[tid] = rrow.w;
    if (tid == 0) erow[n] = ne;
    if (tid >= 64 && tid < 64 + GNN_EMAX / 4) reinterpret_cast<uint4*>(esrc)[tid - 64] = elist;
    if (tid >= 128 && tid < 128 + GNN_EMAX / 4) reinterpret_cast<uint4*>(ecls)[tid - 128] = elist;
#pragma unroll
    for (int j = 0; j < TC; ++j) {
      const int i = tid + j * GNN_WAVES * 64;
      lds_st4(X1 + (i / (D / 4)) * LD + 4 * (i % (D / 4)), x1v[j]);
    }
    SN_STAMP(33);
#pragma unroll
    for (int j = 0; j < TC; ++j) {
      const int i = tid + j * GNN_WAVES * 64;
      if (i < n * (D / 4)) {
        const int rr = i / (D / 4), c4 = i % (D / 4);
        sp_store4(SA, rr, c4 >> 2, c4 & 3, rs_v[j]);
      }
    }
    SN_STAMP(34);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < TC) { a_dg[i] = ri[i].x; a_sr[i] = (unsigned)ri[i].y; a_er[i] = (unsigned)ri[i].z; }
    }
    lds_barrier();
    SN_STAMP(1);
  }
#endif
  ee_fetch(0);     // needs efeat (staged above); the loads fly during the three Linears below
  // ---------------------------------------------------------------- h = Linear(cat[x, pos]) (model.py:39-40), pos = BN(W_out . slot_sum)
  //   (sign_net.py:71).  Order: x part (SB -> X1), pos (SA -> SB, SB being free after a barrier), pos part (SB -> X1 +=).
  const void* first_w = P.n_layers > 0 ? P.layers[0].w1s : P.head_w1;
  const TileRange first_tr = P.n_layers > 0 ? tr : hr;
  {
    // rho.out folded into the pos half of `linear` by the caller (lin_b = W_pos . diag(bn scale) . W_out, bias' = W_pos . bn shift + b):
    // h = lin_a . x + lin_b . slot_sum + bias' — two GEMMs over two images that are both complete; each lane parks its own
    // tiles of the first product in X1 and reads them back itself: no barrier between the two
    auto epi_a = [&](int rt, int ot, f32x4 acc, f32x4, f32x4, f32x4) { lds_st4(X1 + (rt * 16 + li) * LD + 16 * ot + 4 * g, acc); };
    auto epi_b = [&](int rt, int ot, f32x4 acc, f32x4 bias, f32x4, f32x4) {
      float* o = X1 + (rt * 16 + li) * LD + 16 * ot + 4 * g;
      lds_st4(o, (lds_ld4(o) + acc) + bias);
    };
    const bool hasl = P.n_layers > 0;
    if constexpr (FRONT) { }                                  // (the record's rows are in X1, `pre` holds the first layer's tile)
    else if constexpr (TC > 0) coop_gemm_weave<NKB, TC>(pre, SB, wave, lane, epi_a, first_w, first_tr.first_ot());
    else if constexpr (ROLL) coop_gemm_roll<NKB>(pre, SB, tr, lane, epi_a, first_w, first_tr);
    else coop_gemm<NKB>(pre, alt, P.lin_a, SB, tr, lane, epi_a, P.lin_b, tr);
    SN_STAMP(20);
    if constexpr (TC > 0) coop_gemm_weave<NKB, TC>(alt, SA, wave, lane, epi_b, hasl ? P.layers[0].w2s : P.head_w2, hasl ? wave : 0);
    else if constexpr (ROLL) coop_gemm_roll<NKB>(alt, SA, tr, lane, epi_b, hasl ? P.layers[0].w2s : P.head_w2, hasl ? tr : h2);
    else coop_gemm<NKB>(pre, alt, P.lin_b, SA, tr, lane, epi_b, first_w, first_tr);
  }
  ee_store();
  lds_barrier();
  SN_STAMP(2);
  if constexpr (TF) {
    // ---------------------------------------------------------------- graph Transformer layers: h in X1 (fp32) and split in image A
    static_assert(ROLL, "one output tile per wave and Linear");
    for (int t = tr.t_lo; t < tr.t_hi; ++t) {
      int ot, rt;
      tr.decode(t, ot, rt);
      const int row = rt * 16 + li, c = 16 * ot + 4 * g;
      sp_store4(SA, row, ot, g, lds_ld4(X1 + row * LD + c));
    }
    lds_barrier();
    unsigned char* A = SA;
    unsigned char* B = SB;
    const float* Eg = reinterpret_cast<const float*>(S.edge_attr);
    const int an = (int)threadIdx.x >> 3, ah = (int)threadIdx.x & 7;          // the attention's (node, head) of this lane
    const float root = sqrtf(8.f);
    // my node's in-edges do not change from layer to layer: degree and the first four (source row, edge id) pairs are read ONCE, and a
    // layer's E rows of those edges are requested at the layer's entry — three Linear stages before the attention needs them
    int at_lo = 0, at_dg = 0, at_sr[4] = {0, 0, 0, 0};
    const float* at_er[4] = {Eg, Eg, Eg, Eg};
    if (an < n) {
      at_lo = erow[an];
      at_dg = erow[an + 1] - at_lo;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < at_dg) {
          at_sr[k] = esrc[at_lo + k];
          at_er[k] = Eg + (int64_t)ecls[at_lo + k] * S.lde + 8 * ah;
        }
      }
    }
    for (int l = 0; l < P.n_layers; ++l) {
      f32x4 pe0[4], pe1[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        pe0[k] = zero4; pe1[k] = zero4;
        if (k < at_dg) { pe0[k] = ld4(at_er[k] + l * D); pe1[k] = ld4(at_er[k] + l * D + 4); }
      }
      const sn_gnn_layer& Lp = P.layers[l];
      const bool lastl = l + 1 == P.n_layers;
      // the stage matrices in launch order, running on into the next layer / the readout (what every stage prefetches two ahead)
      auto seq = [&](int j) -> const void* {
        if (j < 8) return Lp.etab[j];
        if (!lastl) return P.layers[l + 1].etab[j - 8];
        return j == 8 ? P.head_w1 : S.head_mid;
      };
      auto seq_tr = [&](int j) { return (j < 8 || !lastl) ? tr : hr; };
      float* Qi = reinterpret_cast<float*>(B);            // Q | K | V rows, fp32, in the other image's space (3 * 64 * LD floats = one image)
      float* Ki = Qi + GNN_ROWS * LD;
      float* Vi = Ki + GNN_ROWS * LD;
      static_assert((size_t)3 * GNN_ROWS * LD * sizeof(float) <= (size_t)SP_IMAGE, "Q | K | V fit one split image");
      auto epi_q = [&](int rt, int ot, f32x4 acc, f32x4, f32x4, f32x4) { lds_st4(Qi + (rt * 16 + li) * LD + 16 * ot + 4 * g, acc); };
      auto epi_k = [&](int rt, int ot, f32x4 acc, f32x4, f32x4, f32x4) { lds_st4(Ki + (rt * 16 + li) * LD + 16 * ot + 4 * g, acc); };
      auto epi_v = [&](int rt, int ot, f32x4 acc, f32x4, f32x4, f32x4) { lds_st4(Vi + (rt * 16 + li) * LD + 16 * ot + 4 * g, acc); };
      coop_gemm_roll<NKB>(pre, A, tr, lane, epi_q, seq(2), seq_tr(2));
      coop_gemm_roll<NKB>(alt, A, tr, lane, epi_k, seq(3), seq_tr(3));
      coop_gemm_roll<NKB>(pre, A, tr, lane, epi_v, seq(4), seq_tr(4));
      lds_barrier();
      // the edge attention (layers/transformer.py:150-228; arithmetic of k_edge_attention, csrc/dgl_layers.hip): one lane per (node, head)
      if (an < n) {
        const f32x4 q0 = lds_ld4(Qi + an * LD + 8 * ah), q1 = lds_ld4(Qi + an * LD + 8 * ah + 4);
        f32x4 a0 = zero4, a1 = zero4;
        float z = 0.f;
        auto edge = [&](int sr, f32x4 e0, f32x4 e1) {
          const f32x4 k0 = lds_ld4(Ki + sr * LD + 8 * ah), k1 = lds_ld4(Ki + sr * LD + 8 * ah + 4);
          const f32x4 v0 = lds_ld4(Vi + sr * LD + 8 * ah), v1 = lds_ld4(Vi + sr * LD + 8 * ah + 4);
          float sc = 0.f;
#pragma unroll
          for (int c = 0; c < 4; ++c) sc += ((k0[c] * q0[c]) / root) * e0[c];
#pragma unroll
          for (int c = 0; c < 4; ++c) sc += ((k1[c] * q1[c]) / root) * e1[c];
          const float sw = expf(fminf(fmaxf(sc, -5.f), 5.f));
          z += sw;
#pragma unroll
          for (int c = 0; c < 4; ++c) { a0[c] += v0[c] * sw; a1[c] += v1[c] * sw; }
        };
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < at_dg) edge(at_sr[k], pe0[k], pe1[k]);              // edge-id order: the first four from the prefetched rows
        for (int e = at_lo + 4; e < at_lo + at_dg; ++e) {              // a node with more in-edges: the rest straight from memory
          const float* er = Eg + (int64_t)ecls[e] * S.lde + l * D + 8 * ah;
          edge(esrc[e], ld4(er), ld4(er + 4));
        }
        const float rz = 1.0f / (z + 1e-6f);
        sp_store4(A, an, ah >> 1, 2 * (ah & 1), a0 * rz);
        sp_store4(A, an, ah >> 1, 2 * (ah & 1) + 1, a1 * rz);
      }
      lds_barrier();
      // x1 = BatchNorm(x + O_h(a)) -> X1 and, split, the other image (Q | K | V are dead)
      auto epi_o = [&](int rt, int ot, f32x4 acc, f32x4 bias, f32x4 sc, f32x4 sh) {
        float* o = X1 + (rt * 16 + li) * LD + 16 * ot + 4 * g;
        f32x4 v = acc + bias;
        v = v + lds_ld4(o);
        v = v * sc + sh;
        lds_st4(o, v);
        sp_store4(B, rt * 16 + li, ot, g, v);
      };
      coop_gemm_roll<NKB>(alt, A, tr, lane, epi_o, seq(5), seq_tr(5));
      lds_barrier();
      // FFN layer 1 in two halves of 64 hidden channels: relu(W x1 + b) -> image A, channels [0, 64) and [64, 128)
      auto epi_f1a = [&](int rt, int ot, f32x4 acc, f32x4 bias, f32x4, f32x4) { sp_store4(A, rt * 16 + li, ot, g, relu4(acc + bias)); };
      auto epi_f1b = [&](int rt, int ot, f32x4 acc, f32x4 bias, f32x4, f32x4) { sp_store4(A, rt * 16 + li, ot + NT, g, relu4(acc + bias)); };
      coop_gemm_roll<NKB>(pre, B, tr, lane, epi_f1a, seq(6), seq_tr(6));
      coop_gemm_roll<NKB>(alt, B, tr, lane, epi_f1b, seq(7), seq_tr(7));
      lds_barrier();
      // FFN layer 2 in two halves of its 128-deep sum: the first half's sums parked in fp32, then x = BatchNorm(x1 + W f + b)
      auto epi_f2a = [&](int rt, int ot, f32x4 acc, f32x4, f32x4, f32x4) { lds_st4(PART + (rt * 16 + li) * LD + 16 * ot + 4 * g, acc); };
      auto epi_f2b = [&](int rt, int ot, f32x4 acc, f32x4 bias, f32x4 sc, f32x4 sh) {
        const int off = (rt * 16 + li) * LD + 16 * ot + 4 * g;
        f32x4 v = (lds_ld4(PART + off) + acc) + bias;
        v = v + lds_ld4(X1 + off);
        v = v * sc + sh;
        lds_st4(X1 + off, v);
        sp_store4(B, rt * 16 + li, ot, g, v);
      };
      coop_gemm_roll<NKB>(pre, A, tr, lane, epi_f2a, seq(8), seq_tr(8));
      coop_gemm_roll<NKB>(alt, A, tr, lane, epi_f2b, seq(9), seq_tr(9), 2);      // K blocks 2, 3 of the hidden rows
      lds_barrier();
      unsigned char* tsw = A; A = B; B = tsw;
    }
  } else {
  // ---------------------------------------------------------------- GINE layers: h lives in X1           (model.py:47-55)
  // The in-edges of my pairs' rows do not change from layer to layer: degree, the first four source rows and their edge classes
  // (or edge ids) are read ONCE — the aggregation of every layer then starts with its row reads instead of two dependent index
  // round trips per pair.
  for (int l = 0; l < P.n_layers; ++l) {
    const sn_gnn_layer& Lp = P.layers[l];
    // u = sum_{j->i} relu(h_j + e_ji) + (1+eps) h_i  for my (channel tile, row tile) pairs: X1 -> SA (split)
#ifdef SN_PROFILE
    pt = clock64();
#endif
    ee_fetch(l + 1);   // next layer's edge embeddings: in flight during this aggregation
    {
      const float sc = 1.f + *Lp.eps;
      if (DGL || use_tab || use_ee) {
        // my (up to four) pairs, one after the other; the in-edge indices of their rows were read once before the layer loop (a_*)
        const int eoff = use_tab ? l * ncls : 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (a_dg[i] >= 0) {
            const int t = tr.t_lo + i;
            int ot, rt;
            tr.decode(t, ot, rt);
            const int row = rt * 16 + li, c = 16 * ot + 4 * g, dg = a_dg[i];
            // the first four in-edges (molecular graphs: all) with unrolled reads: the eight row reads, then the adds in edge order; a
            // missing in-edge reads the two zero rows, relu(0 + 0) = +0 is added: no select on the values (round 5: 16 of a pair's ~95
            // vector instructions were those selects)
            f32x4 hv[4], ev[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int sr = (int)((a_sr[i] >> (8 * k)) & 255u), er = (int)((a_er[i] >> (8 * k)) & 255u);
              hv[k] = lds_ld4(X1 + sr * LD + c);
              if (!DGL) ev[k] = lds_ld4(EE + (er == 255 ? S.ee_rows : er + eoff) * LD + c);
            }
            f32x4 u = zero4;
#pragma unroll
            for (int k = 0; k < 4; ++k) u += DGL ? hv[k] : relu4(hv[k] + ev[k]);
            if (dg > 4) {
              const int e_lo = erow[row], e_hi = e_lo + dg;
              for (int e = e_lo + 4; e < e_hi; ++e) {
                if (DGL) { u += lds_ld4(X1 + esrc[e] * LD + c); continue; }
                const f32x4 ef = use_tab ? lds_ld4(EE + (l * ncls + ecls[e]) * LD + c) : lds_ld4(EE + e * LD + c);
                u += relu4(lds_ld4(X1 + esrc[e] * LD + c) + ef);
              }
            }
            {
#pragma clang fp contract(off)
              const f32x4 self = lds_ld4(X1 + row * LD + c) * sc;
              u = u + self;
            }
            sp_store4(SA, row, ot, g, u);
          }
          __builtin_amdgcn_sched_barrier(0);      // pairs stay sequential: four pairs' row reads at once would not fit the registers
        }
      } else {
#pragma unroll 1
        for (int t = tr.t_lo; t < tr.t_hi; ++t) {
          int ot, rt;
          tr.decode(t, ot, rt);
          const int row = rt * 16 + li, c = 16 * ot + 4 * g;
          if (row >= n) continue;
          f32x4 u = zero4;
          const int e_lo = erow[row], e_hi = erow[row + 1];
          for (int e = e_lo; e < e_hi; ++e) u += relu4(lds_ld4(X1 + esrc[e] * LD + c) + edge_embed(Lp, e, c));
          {
#pragma clang fp contract(off)
            const f32x4 self = lds_ld4(X1 + row * LD + c) * sc;
            u = u + self;
          }
          sp_store4(SA, row, ot, g, u);
        }
      }
    }
    lds_barrier();
    SN_ACCUM(9, pt);
#ifdef SN_PROFILE
    pt = clock64();
#endif
    ee_store();        // every wave is done reading this layer's embeddings
    // nn: Linear . BN . ReLU : SA -> SB
    const bool lastl = l + 1 == P.n_layers;
    auto epi_1 = [&](int rt, int ot, f32x4 acc, f32x4 sc, f32x4 sh, f32x4) { sp_store4(SB, rt * 16 + li, ot, g, relu4(acc * sc + sh)); };
    if constexpr (TC > 0) coop_gemm_weave<NKB, TC>(pre, SA, wave, lane, epi_1, lastl ? P.head_w1 : P.layers[lastl ? l : l + 1].w1s, wave);
    else if constexpr (ROLL) coop_gemm_roll<NKB>(pre, SA, tr, lane, epi_1, lastl ? P.head_w1 : P.layers[lastl ? l : l + 1].w1s, lastl ? hr : tr);
    else coop_gemm<NKB>(pre, alt, Lp.w1s, SA, tr, lane, epi_1, Lp.w2s, tr);
    lds_barrier();
    SN_ACCUM(11, pt);
#ifdef SN_PROFILE
    pt = clock64();
#endif
    // Linear ; BN . ReLU ; + previous_x : SB -> X1 (my tiles only: nobody else reads them at this point)
    auto epi_2 = [&](int rt, int ot, f32x4 acc, f32x4 sc, f32x4 sh, f32x4) {
      float* o = X1 + (rt * 16 + li) * LD + 16 * ot + 4 * g;
      if (DGL) lds_st4(o, acc * sc + sh);           // the MLP's last Linear: nothing behind it
      else lds_st4(o, relu4(acc * sc + sh) + lds_ld4(o));
    };
    if constexpr (TC > 0) coop_gemm_weave<NKB, TC>(alt, SB, wave, lane, epi_2, lastl ? P.head_w2 : P.layers[lastl ? l : l + 1].w2s, lastl ? 0 : wave);
    else if constexpr (ROLL) coop_gemm_roll<NKB>(alt, SB, tr, lane, epi_2, lastl ? (DGL ? S.head_mid : P.head_w2) : P.layers[lastl ? l : l + 1].w2s,
                                            lastl ? (DGL ? hr : h2) : tr);
    else coop_gemm<NKB>(pre, alt, Lp.w2s, SB, tr, lane, epi_2, lastl ? P.head_w1 : P.layers[lastl ? l : l + 1].w1s, lastl ? hr : tr);
    // TC > 0 (NT = 8): wave w owns channel tile w of EVERY row, in this Linear and in the next layer's aggregation alike — the rows the
    // aggregation gathers were written by this very wave (LDS operations of a wave execute in order): no workgroup barrier between
    // the two, only in front of the pooling, which reads all channels
    if (TC > 0 && !lastl) asm volatile("" ::: "memory");
    else lds_barrier();
    SN_ACCUM(12, pt);
    SN_STAMP(24 + l);
  }
  }
  SN_STAMP(3);
  // ---------------------------------------------------------------- add pooling -> row 0 of SA (rows 1..15: zero)   (model.py:57-61)
  // (sixteen interleaved partial sums per channel quad, then their sum in order: 4 + 16 dependent adds instead of n)
  static_assert(16 * (D / 4) <= GNN_WAVES * 64 && (size_t)16 * D * sizeof(float) <= (size_t)(SP_PLANE - 16 * SP_STRIDE), "one pass; the partial sums fit");
  // [16][D], parked in rows 16.. of image A's first plane: the head reads row tile 0 only, and unlike image B's — whose K padding of
  // rows 0-15 the head's second Linear reads and must find zero — nothing there is looked at again
  float* PS = reinterpret_cast<float*>(SA + 16 * SP_STRIDE);
  {
    const int pj = threadIdx.x / (D / 4), pc4 = threadIdx.x % (D / 4);
    // the DGL nets' readout 'max' (S.pool_mean == SN_READOUT_MAX): the same sixteen partials with max and -inf — a NaN among the rows
    // is kept, a graph without nodes reads 0
    bool pmax = false;
    if constexpr (DGL) pmax = S.pool_mean == SN_READOUT_MAX;
    if (pj < 16) {
      f32x4 s = zero4;
      if (pmax) {
        s = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        for (int r = pj; r < n; r += 16) s = nan_max4(s, lds_ld4(X1 + r * LD + 4 * pc4));
      } else {
        for (int r = pj; r < n; r += 16) s += lds_ld4(X1 + r * LD + 4 * pc4);
      }
      lds_st4(PS + pj * D + 4 * pc4, s);
    }
    lds_barrier();
    if (pj < 16) {
      f32x4 s = zero4;
      if (pj == 0) {
        if (pmax) {
          s = lds_ld4(PS + 4 * pc4);
#pragma unroll
          for (int j = 1; j < 16; ++j) s = nan_max4(s, lds_ld4(PS + j * D + 4 * pc4));
          if (n <= 0) s = zero4;
        } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) s += lds_ld4(PS + j * D + 4 * pc4);
        if (DGL && S.pool_mean) s = s / (float)n;
        }
      }
      sp_store4(SA, pj, pc4 >> 2, pc4 & 3, s);
    }
  }
  lds_barrier();
  SN_STAMP(4);
  // ---------------------------------------------------------------- output encoder on the pooled row     (model.py:63)
  auto epi_h1 = [&](int rt, int ot, f32x4 acc, f32x4 sc, f32x4 sh, f32x4) { sp_store4(SB, li, ot, g, relu4(acc * sc + sh)); };
  auto epi_h2 = [&](int rt, int ot, f32x4 acc, f32x4 bias, f32x4, f32x4) {
    if (li == 0) {
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const int c = 4 * g + qq;
        if (c < P.n_out) S.y[(int64_t)gi * P.n_out + c] = graph_bad ? __uint_as_float(0x7fc00000u) : acc[qq] + bias[qq];
      }
    }
  };
  if constexpr (DGL) {
    // MLPReadout (layers/mlp_readout_layer.py): Linear . ReLU . Linear . ReLU . Linear — SA -> SB -> SA -> y
    auto epi_hm = [&](int rt, int ot, f32x4 acc, f32x4 sc, f32x4 sh, f32x4) { sp_store4(SA, li, ot, g, relu4(acc * sc + sh)); };
    if constexpr (ROLL) coop_gemm_roll<NKB>(pre, SA, hr, lane, epi_h1, wave == 0 ? P.head_w2 : nullptr, h2);
    else coop_gemm<NKB>(pre, alt, P.head_w1, SA, hr, lane, epi_h1, S.head_mid, hr);
    lds_barrier();
    if constexpr (ROLL) coop_gemm_roll<NKB>(alt, SB, hr, lane, epi_hm, nullptr, h2);
    else coop_gemm<NKB>(pre, alt, S.head_mid, SB, hr, lane, epi_hm, wave == 0 ? P.head_w2 : nullptr, h2);
    lds_barrier();
    if constexpr (ROLL) coop_gemm_roll<NKB>(pre, SA, h2, lane, epi_h2, nullptr, h2);
    else coop_gemm<NKB>(pre, alt, P.head_w2, SA, h2, lane, epi_h2, nullptr, h2);
  } else {
  if constexpr (ROLL) coop_gemm_roll<NKB>(pre, SA, hr, lane, epi_h1, nullptr, h2);
  else coop_gemm<NKB>(pre, alt, P.head_w1, SA, hr, lane, epi_h1, wave == 0 ? P.head_w2 : nullptr, h2);
  lds_barrier();
  if constexpr (ROLL) coop_gemm_roll<NKB>(alt, SB, h2, lane, epi_h2, nullptr, h2);
  else coop_gemm<NKB>(pre, alt, P.head_w2, SB, h2, lane, epi_h2, nullptr, h2);
  }
  SN_STAMP(5);
#ifdef SN_PROFILE
  if ((int)blockIdx.x == g_prof_block && threadIdx.x == 0) { g_prof[6] = n; g_prof[7] = ne; }
#endif
}

// One workgroup per graph; the last workgroup to finish reports the batch's flags to the host (no separate copy).
