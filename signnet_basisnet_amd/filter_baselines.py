"""The spectral graph-convolution baselines of the LearningFilters filter table on the HIP stack: BernNet, GPRNet, ChebNet, GcnNet
(LearningFilters/models.py:138-377; training.py:152-165 builds them by name, BernNet is the script's default --net).

All four are polynomial filters of one sparse operator on the one fixed grid graph, so each conv layer's propagation is one or two
launches of csrc/poly_filter.hip whatever K (autograd.py: bern_prop, poly_combine_shared, cheb_conv); the weight GEMMs, bias, ReLU and
the head are the layer-path ops of every other model here (AG.linear).  Per conv layer, beyond the GEMMs and the finishing reductions:

  BernNet   forward 2 (basis over 2I - L, combine over L)     backward 2 (basis over L^T with the coe dots, combine over (2I - L)^T)
  GPRNet    forward 1 (combine, c = temp)                     backward 2 (combine over S^T, basis dots for d temp)
  ChebNet   forward 2 (Clenshaw combine, bias / ReLU)         backward 2 (ReLU adjoint, basis over S^T)
  GcnNet    forward 1 (combine, c = [0, 1])                   backward 1 (combine over S^T)

Constructors and state_dict keys / shapes are the reference's: BernNet `convs.i.weight [in, out]`, `convs.i.bias`, `coe`, `fc2.*`;
GPRNet `lins.i.*`, `prop1.temp [K+1]`, `fc2.*`; ChebNet `convs.i.lins.k.weight`, `convs.i.bias` and GcnNet `convs.i.lin.weight`,
`convs.i.bias` as torch_geometric 2.0.1 lays ChebConv / GCNConv out (restated from its documented definition, like the GIN layers).
`prop1.temp` is float64 in the reference (torch.tensor of a numpy array); here it is float32 and load_state_dict converts.

GatNet and ARMANet (models.py:256-272, 221-236) are not polynomial filters of the operator (attention with ELU and self loops;
ARMAConv's skip) and stay out of NETS: gen_model(..., baselines=True) and gen_baseline(name, ...) raise NotImplementedError for them as
before.  They are EXTRA_NETS, built by gen_baseline(name, ..., extra=True) / gen_model(..., baselines="all"):

  GatNet    per conv: forward 2 (the GEMM; sn_gat_conv_f32: attention over the in-edges and the implicit self loop, bias, ELU)
                      backward 3 for the attention (sn_gat_conv_bwd_f32's two launches, the reduction of the d att_l | d att_r | d bias partials)
  ARMANet   per conv: forward 1 (combine, c = [0, 1], over FilterGraph.arma) and ONE GEMM over [S x | x]   backward 1 (combine over S^T)

GATConv and ARMAConv are restated from torch_geometric 2.0.1's documented definitions (PyG is not a dependency), their parameter names
and key order from memory of that release: `att_l`, `att_r` [1, heads, out], `bias`, `lin_l.weight` and the alias `lin_r.weight`;
`init_weight` [K, in, out], `weight` [max(1, T-1), K, out, out] (unused and without gradient at T = 1), `root_weight` [T, K, in, out],
`bias` [T, K, 1, out].  Only what the reference sets is built; everything else raises.

The operator follows PyG's source_to_target flow: messages go from edge_index[0] to edge_index[1]; multi-edges add.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn

from . import autograd as AG
from . import ops

NOT_BUILT = ("GatNet", "ARMANet")


def _csr(src, dst, w, N):
    """Rows by destination: (W x)_i = sum over the edges e with dst_e = i of w_e x[src_e]; a row's entries in (source, input) order."""
    order = torch.argsort(dst * N + src, stable=True)
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device=src.device)
    rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=N), 0)
    return rowptr.to(torch.int32), src[order].to(torch.int32).contiguous(), w[order].to(torch.float32).contiguous()


def _operator_pair(src, dst, w, N):
    fwd = ops.SparseOperator(*_csr(src, dst, w, N), N)
    bwd = ops.SparseOperator(*_csr(dst, src, w, N), N, fwd)
    fwd.t = bwd
    return fwd


class FilterGraph:
    """The per-graph constants of the four baselines, built once (torch ops, on edge_index's device) and kept on the device:

      lap  A = D^-1/2 A D^-1/2 as get_laplacian(edge_index, normalization='sym') weighs it: input self loops removed, degree over the
           SOURCE index, inf -> 0.  L = I - A is (diag_add, scale) = (1, -1), 2I - L = (1, +1), ChebConv's L^ = L - I (lambda_max 2) = (0, -1).
      gcn  gcn_norm's weights: input self loops replaced by one unit loop per node, degree over the TARGET index; used at (0, 1).

    Both are ops.SparseOperator in CSR by destination with `.t` the transposed operator (the adjoints)."""

    def __init__(self, edge_index, num_nodes):
        N = int(num_nodes)
        ei = torch.as_tensor(edge_index)
        if ei.dim() != 2 or ei.shape[0] != 2 or ei.dtype.is_floating_point:
            raise ValueError("FilterGraph: edge_index must be an integer [2, E] tensor")
        if N < 1:
            raise ValueError("FilterGraph: num_nodes must be >= 1")
        ei = ei.long()
        if ei.numel() and (int(ei.min()) < 0 or int(ei.max()) >= N):
            raise ValueError(f"FilterGraph: edge_index has entries outside [0, {N})")
        self.N, self.device = N, ei.device
        keep = ei[0] != ei[1]
        s, t = ei[0][keep], ei[1][keep]
        one = torch.ones(s.numel(), dtype=torch.float32, device=ei.device)
        deg = torch.zeros(N, dtype=torch.float32, device=ei.device).index_add_(0, s, one)
        dis = deg.pow(-0.5)
        dis.masked_fill_(dis == float("inf"), 0)
        self.lap = _operator_pair(s, t, dis[s] * one * dis[t], N)
        loop = torch.arange(N, device=ei.device)
        s2, t2 = torch.cat([s, loop]), torch.cat([t, loop])
        one2 = torch.ones(s2.numel(), dtype=torch.float32, device=ei.device)
        deg2 = torch.zeros(N, dtype=torch.float32, device=ei.device).index_add_(0, t2, one2)
        dis2 = deg2.pow(-0.5)
        dis2.masked_fill_(dis2 == float("inf"), 0)
        self.gcn = _operator_pair(s2, t2, dis2[s2] * one2 * dis2[t2], N)
        self._edges, self._arma = ei, None

    @property
    def arma(self):
        """ARMAConv's operator, gcn_norm(..., add_self_loops=False): every input edge kept (a self loop is an ordinary entry), unit
        weights, degree over the TARGET index, inf -> 0.  Built on first use (only ARMANet asks for it)."""
        if self._arma is None:
            s, t = self._edges[0], self._edges[1]
            one = torch.ones(s.numel(), dtype=torch.float32, device=self.device)
            deg = torch.zeros(self.N, dtype=torch.float32, device=self.device).index_add_(0, t, one)
            dis = deg.pow(-0.5)
            dis.masked_fill_(dis == float("inf"), 0)
            self._arma = _operator_pair(s, t, dis[s] * one * dis[t], self.N)
        return self._arma


_GRAPHS = {}


def as_filter_graph(edge_index, num_nodes):
    """A FilterGraph as is; an edge tensor through a cache keyed by its storage pointer, shape and version counter (the workload has one
    graph: data.edge_index of every call is the same tensor)."""
    if isinstance(edge_index, FilterGraph):
        if edge_index.N != num_nodes:
            raise ValueError(f"the FilterGraph has {edge_index.N} nodes, x has {num_nodes}")
        return edge_index
    if not torch.is_tensor(edge_index):
        raise TypeError("the model's second argument must be a FilterGraph or an edge_index tensor")
    key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, edge_index.device, int(num_nodes))
    g = _GRAPHS.get(key)
    if g is None:
        if len(_GRAPHS) >= 8:
            _GRAPHS.clear()
        g = _GRAPHS[key] = FilterGraph(edge_index, num_nodes)
    return g


def _graph_for(x, edge_index):
    ops.require_cuda(x)
    if x.dim() != 2:
        raise ValueError("the filter baselines take x [N, F] of one graph")
    g = as_filter_graph(edge_index, x.shape[0])
    if g.device != x.device:
        raise ValueError(f"the graph is on {g.device}, x on {x.device}")
    return g


# ----------------------------------------------------------------------------- BernNet (models.py:291-377)
class BernConv(nn.Module):
    """The parameters of models.py:291-314 (weight [in, out], bias); the propagation is BernNet.forward's."""

    def __init__(self, in_channels, out_channels, K, bias=True):
        super().__init__()
        assert K > 0
        self.in_channels, self.out_channels, self.K = in_channels, out_channels, K
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        """Glorot-uniform weight over (in + out), zero bias — the state the reference's constructor leaves."""
        with torch.no_grad():
            nn.init.xavier_uniform_(self.weight)           # bound sqrt(6 / (fan_in + fan_out)): the same for [in, out] as for [out, in]
            if self.bias is not None:
                self.bias.zero_()


class BernNet(nn.Module):
    def __init__(self, in_channels, hidden_channels=32, num_layers=2, K=10):
        super().__init__()
        self.convs = nn.ModuleList([BernConv(in_channels, hidden_channels, K)])
        for _ in range(num_layers - 1):
            self.convs.append(BernConv(hidden_channels, hidden_channels, K))
        self.fc2 = nn.Linear(hidden_channels, 1)
        self.coe = nn.Parameter(torch.empty(K + 1))
        self.K = K
        # comb(K, i) / 2^K: exact in float64, rounded once (models.py:332,340 multiply a Python float into the float32 tensor)
        self.register_buffer("_binom", torch.tensor([math.comb(K, i) / 2.0 ** K for i in range(K + 1)], dtype=torch.float32),
                             persistent=False)
        self.reset_parameters()

    def reset_parameters(self):
        self.coe.data.fill_(1)

    def forward(self, x, edge_index):
        g = _graph_for(x, edge_index)
        c = torch.relu(self.coe) * self._binom         # shared by the layers: once per forward, torch's own autograd back to coe
        crev = c.detach().flip(0)
        h = x.float()
        for conv in self.convs:
            p = AG.bern_prop(h, c, crev, g.lap, self.K)
            h = AG.linear_io(p, conv.weight, conv.bias, relu=True)
        return AG.linear(h, self.fc2.weight, self.fc2.bias)


# ----------------------------------------------------------------------------- GPRNet (models.py:138-218)
def _ppr_coefficients(K, alpha):
    """Truncated personalised-PageRank weights: alpha (1 - alpha)^k for k < K, and the remaining mass (1 - alpha)^K on the last."""
    k = torch.arange(K + 1, dtype=torch.float64)
    t = alpha * (1.0 - alpha) ** k
    t[K] = (1.0 - alpha) ** K
    return t


class GPR_prop(nn.Module):
    """The generalised-PageRank propagation of GPRNet (models.py:138-198): hidden = sum_k temp[k] A^k x over gcn_norm's operator, one
    combine launch.  `temp` [K + 1] is float32 here (float64 in the reference; load_state_dict converts).

    Init 'Random' (the default, the only one GPRNet uses) keeps the reference's quirk: K + 1 uniforms in +-sqrt(3 / (K + 1)) drawn from
    `np.random` at construction, scaled to unit l1 norm.  'PPR' is what `reset_parameters` writes.  The reference's other starting points
    ('SGC', 'NPPR', 'WS' with a given Gamma) are not built."""

    def __init__(self, K, alpha=0.1, Init="Random", Gamma=None, bias=True, **kwargs):
        super().__init__()
        self.K, self.Init, self.alpha = int(K), Init, float(alpha)
        if Init == "Random":
            half_width = math.sqrt(3.0 / (self.K + 1))
            draw = np.random.uniform(-half_width, half_width, self.K + 1)
            start = torch.from_numpy(draw / np.abs(draw).sum())
        elif Init == "PPR":
            start = _ppr_coefficients(self.K, self.alpha)
        else:
            raise NotImplementedError(f"GPR_prop: Init={Init!r} is not built (the reference's GPRNet uses the default 'Random'; 'PPR' is "
                                      "also available)")
        self.temp = nn.Parameter(start.float())

    def reset_parameters(self):
        with torch.no_grad():
            self.temp.copy_(_ppr_coefficients(self.K, self.alpha))

    def forward(self, x, edge_index):
        g = _graph_for(x, edge_index)
        return AG.poly_combine_shared(x, self.temp, g.gcn, self.K, "monomial", 0.0, 1.0)


class GPRNet(nn.Module):
    def __init__(self, in_channels, hidden_channels=32, num_layers=2, K=10):
        super().__init__()
        self.lins = nn.ModuleList([nn.Linear(in_channels, hidden_channels)])
        for _ in range(num_layers - 1):
            self.lins.append(nn.Linear(hidden_channels, hidden_channels))
        self.prop1 = GPR_prop(K)
        self.fc2 = nn.Linear(hidden_channels, 1)

    def reset_parameters(self):
        self.prop1.reset_parameters()

    def forward(self, x, edge_index):
        g = _graph_for(x, edge_index)
        h = x.float()
        for lin in self.lins:
            h = AG.linear(h, lin.weight, lin.bias, relu=True)
        h = self.prop1(h, g)
        return AG.linear(h, self.fc2.weight, self.fc2.bias)


# ----------------------------------------------------------------------------- ChebNet (models.py:274-289; PyG 2.0.1 ChebConv, restated)
class ChebConv(nn.Module):
    """torch_geometric 2.0.1's ChebConv(in, out, K, normalization='sym') from its documented definition: K bias-free Linears `lins` and a
    `bias`; out = sum_{k<K} T_k(L^) x lins[k].weight^T + bias with L^ = 2 L / lambda_max - I, lambda_max = 2 (the 'sym' default)."""

    def __init__(self, in_channels, out_channels, K, normalization="sym", bias=True):
        super().__init__()
        assert K > 0
        if normalization != "sym":
            raise NotImplementedError("ChebConv: normalization 'sym' only (the reference's)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lins = nn.ModuleList([nn.Linear(in_channels, out_channels, bias=False) for _ in range(K)])
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        for lin in self.lins:
            nn.init.xavier_uniform_(lin.weight)       # PyG's 'glorot'
        nn.init.zeros_(self.bias)


class ChebNet(nn.Module):
    def __init__(self, in_channels, hidden_channels=32, num_layers=2, K=3):
        super().__init__()
        self.convs = nn.ModuleList([ChebConv(in_channels, hidden_channels, K)])
        for _ in range(num_layers - 1):
            self.convs.append(ChebConv(hidden_channels, hidden_channels, K))
        self.fc2 = nn.Linear(hidden_channels, 1)

    def forward(self, x, edge_index):
        g = _graph_for(x, edge_index)
        h = x.float()
        for conv in self.convs:
            h = AG.cheb_conv(h, [lin.weight for lin in conv.lins], conv.bias, g.lap, 0.0, -1.0, relu=True)
        return AG.linear(h, self.fc2.weight, self.fc2.bias)


# ----------------------------------------------------------------------------- GcnNet (models.py:238-254; PyG 2.0.1 GCNConv, restated)
class GCNConv(nn.Module):
    """torch_geometric 2.0.1's GCNConv(in, out) from its documented definition: a bias-free Linear `lin`, gcn_norm with self loops, a
    `bias` added after the propagation."""

    def __init__(self, in_channels, out_channels, cached=False, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.lin.weight)
        nn.init.zeros_(self.bias)


class GcnNet(nn.Module):
    def __init__(self, in_channels, hidden_channels=32, num_layers=2):
        super().__init__()
        self.convs = nn.ModuleList([GCNConv(in_channels, hidden_channels, cached=False)])
        for _ in range(num_layers - 1):
            self.convs.append(GCNConv(hidden_channels, hidden_channels, cached=False))
        self.fc2 = nn.Linear(hidden_channels, 1)
        self.register_buffer("_c01", torch.tensor([0.0, 1.0]), persistent=False)

    def forward(self, x, edge_index):
        g = _graph_for(x, edge_index)
        h = x.float()
        for conv in self.convs:
            # A (x W^T) + b = (A x) W^T + b: the propagation commutes with the GEMM, so bias and ReLU ride in the GEMM's epilogue
            p = AG.poly_combine_shared(h, self._c01, g.gcn, 1, "monomial", 0.0, 1.0)
            h = AG.linear(p, conv.lin.weight, conv.bias, relu=True)
        return AG.linear(h, self.fc2.weight, self.fc2.bias)


# ----------------------------------------------------------------------------- GatNet (models.py:256-272; PyG 2.0.1 GATConv, restated)
def _glorot(t):
    """PyG's 'glorot': uniform in +-sqrt(6 / (size(-2) + size(-1))), whatever the leading dimensions."""
    bound = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        t.uniform_(-bound, bound)


class GATConv(nn.Module):
    """torch_geometric 2.0.1's GATConv from its documented definition (PyG is not installed here; the parameter layout and key order are
    restated from memory of 2.0.1): a bias-free Linear `lin_l` [heads * out, in] that `lin_r` aliases (both keys are in the state_dict),
    `att_l`, `att_r` [1, heads, out] (glorot) and `bias` [heads * out] (zeros).  The input self loops are removed and every node gets
    exactly one; e_ij = leaky_relu(att_l . x'_j + att_r . x'_i), softmax over j, out_i = sum_j a_ij x'_j + bias, heads concatenated.
    Only what the reference's GatNet sets is built: concat=True, dropout=0, add_self_loops=True."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True, bias=True):
        super().__init__()
        if dropout != 0:
            raise NotImplementedError("GATConv: dropout != 0 is not built (the reference's GatNet sets 0)")
        if not concat:
            raise NotImplementedError("GATConv: concat=False is not built (the reference's GatNet concatenates the heads)")
        if not add_self_loops:
            raise NotImplementedError("GATConv: add_self_loops=False is not built (the kernel's self loop is implicit)")
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope, self.dropout, self.add_self_loops = concat, negative_slope, dropout, add_self_loops
        self.lin_l = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.lin_r = self.lin_l
        self.att_l = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_r = nn.Parameter(torch.empty(1, heads, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(heads * out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        _glorot(self.lin_l.weight)
        _glorot(self.att_l)
        _glorot(self.att_r)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x, edge_index, act=None):
        """Two launches: the GEMM and the attention (bias and `act` — None or 'elu' — in the attention launch)."""
        g = _graph_for(x, edge_index)
        f = AG.linear(x.float(), self.lin_l.weight)
        return AG.gat_conv(f, self.att_l, self.att_r, self.bias, g, self.heads, act, self.negative_slope)


class GatNet(nn.Module):
    def __init__(self, in_channels, hidden_channels=32, num_heads=4, num_layers=2):
        super().__init__()
        if num_layers > 1 and hidden_channels % num_heads:
            raise ValueError(f"GatNet: hidden_channels = {hidden_channels} is not a multiple of num_heads = {num_heads}: the second layer "
                             "would not take the first one's output (the reference fails in forward there)")
        self.convs = nn.ModuleList([GATConv(in_channels, hidden_channels // num_heads, heads=num_heads, concat=True, dropout=0.0)])
        for _ in range(num_layers - 1):
            self.convs.append(GATConv(hidden_channels, hidden_channels // num_heads, heads=num_heads, concat=True, dropout=0.0))
        self.fc2 = nn.Linear(hidden_channels, 1)

    def forward(self, x, edge_index):
        g = _graph_for(x, edge_index)
        h = x.float()
        for conv in self.convs:
            h = conv(h, g, act="elu")                  # F.elu(conv(x, edge_index)): the ELU rides in the attention launch
        return AG.linear(h, self.fc2.weight, self.fc2.bias)


# ----------------------------------------------------------------------------- ARMANet (models.py:221-236; PyG 2.0.1 ARMAConv, restated)
class ARMAConv(nn.Module):
    """torch_geometric 2.0.1's ARMAConv from its documented definition (restated; key order from memory of 2.0.1): `init_weight`
    [K, in, out], `weight` [max(1, T-1), K, out, out], `root_weight` [T, K, in, out] (glorot) and `bias` [T, K, 1, out] (zeros) for
    K = num_stacks, T = num_layers.  One stack of one layer — all the reference's ARMANet builds — is
    act(S (x init_weight) + x root_weight + bias) with S = gcn_norm without added self loops; `weight` is unused at T = 1 and gets
    no gradient, as in PyG.  act: ReLU only."""

    def __init__(self, in_channels, out_channels, num_stacks=1, num_layers=1, shared_weights=False, act="relu", dropout=0.0, bias=True):
        super().__init__()
        if num_stacks != 1 or num_layers != 1:
            raise NotImplementedError("ARMAConv: one stack of one layer only (the reference's ARMANet builds ARMAConv(in, out, 1, 1, False))")
        if shared_weights:
            raise NotImplementedError("ARMAConv: shared_weights=True is not built (the reference passes False)")
        if dropout != 0:
            raise NotImplementedError("ARMAConv: dropout != 0 is not built (the reference sets 0)")
        if not (act == "relu" or act is torch.relu or act is torch.nn.functional.relu or isinstance(act, nn.ReLU)):
            raise NotImplementedError("ARMAConv: ReLU only (PyG's default)")
        K, T = num_stacks, num_layers
        self.in_channels, self.out_channels, self.num_stacks, self.num_layers = in_channels, out_channels, K, T
        self.shared_weights, self.dropout = shared_weights, dropout
        self.init_weight = nn.Parameter(torch.empty(K, in_channels, out_channels))
        self.weight = nn.Parameter(torch.empty(max(1, T - 1), K, out_channels, out_channels))
        self.root_weight = nn.Parameter(torch.empty(T, K, in_channels, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(T, K, 1, out_channels))
        else:
            self.register_parameter("bias", None)
        self.register_buffer("_c01", torch.tensor([0.0, 1.0]), persistent=False)
        self.reset_parameters()

    def reset_parameters(self):
        _glorot(self.init_weight)
        _glorot(self.weight)
        _glorot(self.root_weight)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x, edge_index):
        g = _graph_for(x, edge_index)
        x = x.float()
        # S (x W_init) = (S x) W_init: one propagation, then ONE GEMM over [S x | x] with [W_init; W_root], bias and ReLU in its epilogue
        p = AG.poly_combine_shared(x, self._c01, g.arma, 1, "monomial", 0.0, 1.0)
        W = torch.cat([self.init_weight[0], self.root_weight[0, 0]], dim=0)
        return AG.linear_io(torch.cat([p, x], dim=1), W, None if self.bias is None else self.bias.reshape(-1), relu=True)


class ARMANet(nn.Module):
    def __init__(self, in_channels, hidden_channels=32, num_layers=2):
        super().__init__()
        self.convs = nn.ModuleList([ARMAConv(in_channels, hidden_channels, 1, 1, False, dropout=0)])
        for _ in range(num_layers - 1):
            self.convs.append(ARMAConv(hidden_channels, hidden_channels, 1, 1, False, dropout=0))
        self.fc2 = nn.Linear(hidden_channels, 1)

    def forward(self, x, edge_index):
        g = _graph_for(x, edge_index)
        h = x.float()
        for conv in self.convs:
            h = conv(h, g)                             # F.relu(conv(...)): the conv ends in a ReLU already, the second one is idempotent
        return AG.linear(h, self.fc2.weight, self.fc2.bias)


NETS = {"BernNet": BernNet, "GPRNet": GPRNet, "ChebNet": ChebNet, "GcnNet": GcnNet}
EXTRA_NETS = {"GatNet": GatNet, "ARMANet": ARMANet}        # opt-in: gen_baseline(..., extra=True), gen_model(..., baselines="all")


def gen_baseline(name, in_channels, hidden_channels=32, num_layers=2, extra=False):
    """training.py:154-165 for the four names built here; extra=True: GatNet and ARMANet too."""
    if extra and name in EXTRA_NETS:
        return EXTRA_NETS[name](in_channels, hidden_channels=hidden_channels, num_layers=num_layers)
    if name in NOT_BUILT:
        raise NotImplementedError(f"{name} is not a polynomial filter of the graph operator (PyG's GATConv / ARMAConv) and is not built on "
                                  "the HIP stack; BernNet, GPRNet, ChebNet and GcnNet are")
    if name not in NETS:
        raise ValueError("Invalid model")
    return NETS[name](in_channels, hidden_channels=hidden_channels, num_layers=num_layers)
