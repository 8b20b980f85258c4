"""DGL-tree sign-invariant networks (drop-in `nn.Module` surface, HIP forward).

Mirrors GraphPrediction/layers/deepsigns.py:13-119 (GCNDeepSigns, GINDeepSigns, MaskedGINDeepSigns, TransformerDeepSigns),
layers/gnns.py:15-45 (GCN) and :81-114 (GIN), layers/mlp.py:5-56 (MLP) and the factory
nets/ZINC_graph_regression/sign_inv_net.py:3-17 — same constructor arguments, same `forward(g, x[N,K,1]) -> [N,K,1]`, same
state_dict keys (GIN: `enc.layers.{l}.apply_func.lins.{i}.*`, `enc.layers.{l}.eps`, `enc.bns.{l}.*`; GCN: `enc.layers.{l}.weight`,
`enc.layers.{l}.bias`, `enc.bns.{l}.*`; Transformer: `embed.*`, `enc.layers.{l}.mha.proj_{q,k,v,o}.weight`,
`enc.layers.{l}.mha.ffn.{0,3}.*`, `enc.layers.{l}.mha.norm_{in,inter}.*`; all: `rho.lins.{i}.*`, `rho.bns.{i}.*`).  DGL's own layers
(GINConv, GraphConv, SetTransformerEncoder) are restated from their published definitions: the reference does not pin a DGL version.

`g` is duck-typed: anything with `.edges() -> (src, dst)` int64 tensors and `.batch_num_nodes()` (a DGL batched
graph, or `signnet_basisnet_amd.dgl_deepsigns.Graph`).  Eval mode (BatchNorm with running statistics) runs
entirely in the HIP kernels of libsignnet_hip.so; there is no CPU path.  Train mode without autograd gives the forward VALUE with
batch-statistic BatchNorm (and updates the running statistics); under autograd `_forward_grad` records the same launches as
torch.autograd.Function nodes whose backward are the hand-written adjoints.

All four encoders derive from `_SignInvEncoder`, which holds what does not look into `enc`: the one `forward` (contract checks, the
dispatch to `_forward_grad`, the cache of prepared parameters and its invalidation, the dropout snapshot, the hook `_forward_stages`,
then `_forward_value`), rho on the value path and under autograd (`_mlp_grad`, the one MLP runner of the autograd paths), the -x
constants and the per-call plans of the autograd paths.  Every plan is built from `_plan_inputs` (graph object -> batch vector,
edge index, graph count, with the node-total check) and, for the flipped graph, `_flipped`: `cached_plan` / `_cached_rplan` keep
theirs on the graph object, `_grad_plans` builds per call.  `sign_inv_net_from` is the factory body over a table of the four classes.

The GIN encoders (`_DeepSignsBase`) have one-launch stage kernels (`fused_stages`, `matmul_precision`, `overlap`), tried through the
hook; the GCN and Transformer encoders run layer by layer — one sn_gcn_propagate_f32 / sn_graph_attention_f32 launch per layer for both
signs and every slot, everything else on the layer-path ops — and offer neither switch (`matmul_precision` accepts "highest" only).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops


class Graph:
    """Minimal batched graph: edge list + per-graph node counts (what the reference reads from a DGLGraph)."""

    def __init__(self, src, dst, batch_num_nodes, batch_num_edges=None):
        self.src, self.dst = src, dst
        self._bnn = torch.as_tensor(batch_num_nodes)
        self._bne = None if batch_num_edges is None else torch.as_tensor(batch_num_edges)    # per-graph edge counts, as DGL keeps them
        self._edata, self._ndata = {}, {}

    @property
    def edata(self):
        """Per-edge tensors by name, as DGL's g.edata (a full graph's 'real' flags: ops.make_full_graph)."""
        return self._edata

    @property
    def ndata(self):
        return self._ndata

    def edges(self):
        return self.src, self.dst

    def batch_num_nodes(self):
        return self._bnn

    def batch_num_edges(self):
        return self._bne

    def to(self, device):
        g = Graph(self.src.to(device), self.dst.to(device), self._bnn.to(device), None if self._bne is None else self._bne.to(device))
        g._edata.update({k: v.to(device) for k, v in self._edata.items()})
        g._ndata.update({k: v.to(device) for k, v in self._ndata.items()})
        return g


class MLP(nn.Module):
    """Linear -> activation -> BatchNorm per hidden layer, final Linear (mlp.py:5-56); all Linears have bias."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, use_bn=False, use_ln=False, dropout=0.5,
                 activation="relu", residual=False, _activations=("relu",)):
        super().__init__()
        if use_ln or residual or (activation != "relu" and tuple(_activations) == ("relu",)):
            raise ValueError("HIP path: only relu / no LayerNorm / no residual (what every shipped config uses)")
        if activation not in ("relu", "elu", "tanh"):
            raise ValueError("Invalid activation")                    # mlp.py:23-30
        self.activation = activation
        self.lins = nn.ModuleList()
        if use_bn:
            self.bns = nn.ModuleList()
        if num_layers == 1:
            self.lins.append(nn.Linear(in_channels, out_channels))
        else:
            self.lins.append(nn.Linear(in_channels, hidden_channels))
            if use_bn:
                self.bns.append(nn.BatchNorm1d(hidden_channels))
            for _ in range(num_layers - 2):
                self.lins.append(nn.Linear(hidden_channels, hidden_channels))
                if use_bn:
                    self.bns.append(nn.BatchNorm1d(hidden_channels))
            self.lins.append(nn.Linear(hidden_channels, out_channels))
        self.use_bn, self.dropout = use_bn, dropout


class _GINConv(nn.Module):
    """dgl.nn.pytorch.GINConv(apply_func, 'sum'): eps is a non-learned buffer initialised to 0."""

    def __init__(self, apply_func):
        super().__init__()
        self.apply_func = apply_func
        self.register_buffer("eps", torch.zeros(1))


_GNN_ACTIVATIONS = {"relu": "relu", "tanh": "tanh"}        # gnns.py:13: what GCN / GIN look the name up in (anything else: KeyError)


class GIN(nn.Module):
    def __init__(self, in_channels, hidden_channels, out_channels, n_layers, use_bn=True, dropout=0.5, activation="relu",
                 _activations=("relu",)):
        super().__init__()
        if tuple(_activations) != ("relu",):
            _GNN_ACTIVATIONS[activation]                               # gnns.py:87, in front of the first MLP
        self.layers = nn.ModuleList()
        if use_bn:
            self.bns = nn.ModuleList()
        self.use_bn = use_bn
        self.layers.append(_GINConv(MLP(in_channels, hidden_channels, hidden_channels, 2, use_bn=use_bn, dropout=dropout,
                                        activation=activation, _activations=_activations)))
        for _ in range(n_layers - 2):
            self.layers.append(_GINConv(MLP(hidden_channels, hidden_channels, hidden_channels, 2, use_bn=use_bn,
                                            dropout=dropout, activation=activation, _activations=_activations)))
            if use_bn:
                self.bns.append(nn.BatchNorm1d(hidden_channels))
        self.layers.append(_GINConv(MLP(hidden_channels, hidden_channels, out_channels, 2, use_bn=use_bn, dropout=dropout,
                                        activation=activation, _activations=_activations)))
        if use_bn:
            self.bns.append(nn.BatchNorm1d(hidden_channels))


def _pack(lin):
    w = lin.weight.detach()
    return ops.PackedLinear(ops.pack_weight(w), w.shape[0], w.shape[1], None if lin.bias is None else lin.bias.detach().contiguous())


class _BNSite:
    """A BatchNorm1d of the layer path: eval -> running statistics folded to (scale, shift) once; train -> the module,
    whose batch statistics are taken per forward (and whose running statistics are updated)."""
    __slots__ = ("mod", "scale", "shift")

    def __init__(self, bn, train):
        self.mod = bn
        self.scale, self.shift = (None, None) if train else ops.bn_fold(bn)

    def affine(self, y, train):
        """(scale, shift) to apply to the rows `y` [R, C] (train: from y's own column statistics)."""
        if not train:
            return self.scale, self.shift
        m = self.mod
        mean, var, count = ops.masked_colstats(y)
        ops.bn_running_update(m, mean, var, count)
        return ops.bn_fold_stats(None if m.weight is None else m.weight.detach(), None if m.bias is None else m.bias.detach(),
                                 mean, var, m.eps)


def _prep_mlp(mlp: MLP, train=False):
    """[(packed linear, BN site or None)] per layer."""
    out = []
    for i, lin in enumerate(mlp.lins):
        bn = _BNSite(mlp.bns[i], train) if (mlp.use_bn and i < len(mlp.lins) - 1) else None
        out.append((_pack(lin), bn))
    return out


def _run_mlp(prep, x, nvalid=None, K=0, tail_bn=None, train=False, drop=None, tail_drop=None, fuse_drop=False, act=None):
    """mlp.py:37-56: hidden layers = bias -> relu -> BN [-> dropout]; the final Linear optionally followed by the
    BatchNorm that GIN.forward applies before the NEXT GINConv (gnns.py:105-112; in eval folded into the GEMM epilogue).
    train: BatchNorm over ALL rows of the layer (the reference normalises [N, C, K] tensors, padded slots included).
    drop = (p, snap, first site): the train-mode dropout behind hidden layer i (mlp.py:51) is site `first + i` on the [R, C] rows —
    rows node * K + slot with the channels contiguous, the reference's row-major [N, k, C], for the sign-invariant encoders.
    fuse_drop (the encoders of dropout_signinv.py): where a BatchNorm precedes the site, its apply pass and the mask are ONE launch
    (ops.affine_dropout) instead of masked_affine + dropout — the same bits.  tail_drop: the site of GIN.forward's inter-layer dropout
    (gnns.py:105), applied to the final Linear's output in front of `tail_bn`.
    act = 'tanh' | 'elu' (activation_signinv.py; None: ReLU, the GEMM's own epilogue): a hidden layer is the Linear with its bias, then
    ONE ops.act_affine launch — in eval with the folded BatchNorm, in train mode bare, the batch statistics taken on its output."""
    for i, (pl, bn) in enumerate(prep):
        last = i == len(prep) - 1
        site = tail_bn if last else bn
        relu = not last and act is None
        if not train:
            sc, sh = (None, None) if site is None else (site.scale, site.shift)
            if last or act is None:
                x = ops.masked_linear(x, pl, nvalid, K, relu_pre=relu, scale=sc, shift=sh)
            else:
                x = ops.act_affine(ops.masked_linear(x, pl, nvalid, K), act, nvalid, K, scale=sc, shift=sh)
        else:
            x = ops.masked_linear(x, pl, nvalid, K, relu=relu)
            if not last and act is not None:
                x = ops.act_affine(x, act, nvalid, K)
            dropped = drop is not None and not last and drop[0]
            if last and tail_drop is not None and drop is not None and drop[0]:
                x = ops.dropout(x, drop[0], drop[1], tail_drop)
            if site is not None:
                sc, sh = site.affine(x, True)
                if dropped and fuse_drop:
                    x = ops.affine_dropout(x, sc, sh, drop[0], drop[1], drop[2] + i)
                    continue
                x = ops.masked_affine(x, scale=sc, shift=sh)
            if dropped:
                x = ops.dropout(x, drop[0], drop[1], drop[2] + i)
    return x


def _no_dropout(dropout, who):
    """The reference applies F.dropout(p=dropout) in MLP.forward / GIN.forward while training (mlp.py:52, gnns.py:104); the shipped
    sign_inv configs all set dropout 0.0.  A non-zero value is refused instead of being silently ignored."""
    if float(dropout) != 0.0:
        raise NotImplementedError(f"{who}: dropout={dropout} is not implemented by the HIP modules (the shipped configs use 0.0); "
                                  "pass dropout=0.0")


class _EncoderDropout(ops.DropoutHolder):
    """Train-mode dropout of a sign-invariant encoder.  Opt-in by class: with `_signinv_dropout` False — the classes
    of this module — `dropout > 0` is refused as before; the subclasses of dropout_signinv.py set it True and are their own
    DropoutHolder.  site = ops.SIGNINV_DROP_SITE + the ordinal of the F.dropout / nn.Dropout call within one forward of the
    reference module — enc(g, x), then enc(g, -x), then rho — so the two encoder calls draw different masks and a train-mode
    forward with p > 0 is not sign-invariant, there as here; eval draws nothing and stays invariant bit for bit."""

    _signinv_dropout = False
    _signinv_activations = ("relu",)     # what `activation=` may name; the subclasses of activation_signinv.py widen it

    @property
    def _act(self):
        """None for ReLU (the epilogue of the layer-path GEMM), else 'tanh' | 'elu': an ops.act_affine launch per activation site."""
        a = getattr(self.rho, "activation", "relu")
        return None if a == "relu" else a

    def _init_dropout(self, dropout, who):
        if not self._signinv_dropout:
            _no_dropout(dropout, who)
        self.p_drop = ops.check_dropout_p(dropout, f"{who}: dropout")

    def _drop_begin(self, train, device):
        """(p, {seed, step} snapshot) of this train-mode forward — the step advances once, here — or None when no site is active."""
        p = getattr(self, "p_drop", 0.0)
        return (p, self._dropout_begin(device)) if train and p > 0.0 else None

    def _rho_site0(self):
        """Ordinal of rho's first site: behind the sites of the two encoder calls."""
        return ops.SIGNINV_DROP_SITE + 2 * self._enc_sites()


def _pad_mat(W, dp):
    out = torch.zeros(dp, dp, dtype=torch.float32, device=W.device)
    out[:W.shape[0], :W.shape[1]].copy_(W.detach())
    return out


def _fold_bn_before(lin, site):
    """Linear(BatchNorm(h)) with an eval BatchNorm (scale, shift) -> one Linear: W' = W diag(scale), b' = b + W shift.  On the device
    ops (a column scaling and one [1, d] GEMM), run once per parameter version."""
    W, b = lin.weight.detach().contiguous(), lin.bias.detach().contiguous()
    if site is None:
        return W, b
    Wf = ops.masked_affine(W, scale=site.scale, shift=torch.zeros_like(site.shift))
    bf = ops.masked_linear(site.shift.view(1, -1).contiguous(), ops.PackedLinear(ops.pack_weight(W), W.shape[0], W.shape[1], b)).view(-1)
    return Wf, bf


class _FusedDeepSigns:
    """Packed eval-mode parameters of a (Masked)GINDeepSigns for the two stage kernels: sn_deepsigns_phi_f32 (enc(g,x) + enc(g,-x),
    all GIN layers, one launch) and sn_mlp_chain_f32 (rho, with the masked slot sum in front for the masked variant).  With
    sn_batch_plan that is three launches per forward (deepsigns.py:45-51 / :72-86).  `ok` is False for shapes the stage kernels do
    not take (hidden > 112, k > 64, k * phi_out > 128, MLPs that are not the reference's 2-layer GIN MLP): the layer path serves those."""

    def __init__(self, mod):
        from .fused import _PhiParams
        import ctypes as C
        enc, rho, K = mod.enc, mod.rho, mod.k
        self.ok = False
        if mod._act is not None:          # the stage kernels' arithmetic is ReLU: a tanh / elu encoder runs the layer path
            return
        L = len(enc.layers)
        mlps = [c.apply_func for c in enc.layers]
        if any(len(m.lins) != 2 for m in mlps) or mlps[0].lins[0].weight.shape[1] != 1:
            return
        hidden = mlps[0].lins[0].weight.shape[0]
        out = mlps[-1].lins[1].weight.shape[0]
        dp = 16 * ((max(hidden, out) + 15) // 16)
        dp = max(dp, 48)
        d_in = out if mod.masked else K * out
        rdims = [d_in] + [l.weight.shape[0] for l in rho.lins]
        rp = max(48, 16 * ((max(rdims) + 15) // 16))
        if not (dp <= 112 and rp <= 128 and 1 <= L <= 16 and K <= 64 and len(rho.lins) <= 16):
            return
        keep = self._keep = []

        def hold(t):
            keep.append(t)
            return t.data_ptr()

        dev = mlps[0].lins[0].weight.device
        ones = ops.pad_vec(torch.ones(hidden, device=dev), dp)
        P = _PhiParams()
        P.d, P.n_layers, P.hid0, P.reserved = dp, L, dp, out
        for l, m in enumerate(mlps):
            site_mid = _BNSite(m.bns[0], False) if m.use_bn else None                       # after the ReLU, before lins[1]
            site_out = _BNSite(enc.bns[l], False) if (enc.use_bn and l < L - 1) else None   # in front of layer l + 1 (gnns.py:105-110)
            W1, b1 = _fold_bn_before(m.lins[1], site_mid)
            no = W1.shape[0]
            e1 = ops.pad_vec(site_out.scale if site_out is not None else torch.ones(no, device=dev), dp)
            e2 = ops.pad_vec(site_out.shift if site_out is not None else torch.zeros(no, device=dev), dp)
            w2 = ops.pack_split(_pad_mat(W1, dp), ops.pad_vec(b1, dp), e1, e2)
            b0 = ops.pad_vec(m.lins[0].bias, dp)
            if l == 0:
                P.l0_w1 = hold(ops.pad_vec(m.lins[0].weight[:, 0], dp))
                P.l0_bn0_scale, P.l0_bn0_shift = hold(ones), hold(b0)
                P.l0_w2 = hold(w2)
                P.l0_eps = hold(enc.layers[0].eps.detach().float().contiguous())
            else:
                Lp = P.layers[l - 1]
                Lp.w1s = hold(ops.pack_split(_pad_mat(m.lins[0].weight, dp), ones, b0, None))
                Lp.w2s = hold(w2)
                Lp.eps = hold(enc.layers[l].eps.detach().float().contiguous())
        self.phi = P
        # rho: relu(W0 x + b0), then every later Linear with the BatchNorm in front of it folded in
        ws = []
        for i, lin in enumerate(rho.lins):
            site = _BNSite(rho.bns[i - 1], False) if (rho.use_bn and i > 0) else None
            W, b = _fold_bn_before(lin, site)
            ws.append(hold(ops.pack_split(_pad_mat(W, rp), ops.pad_vec(b, rp), None, None)))
        self.rho_w = (C.c_void_p * len(ws))(*ws)
        self.n_rho, self.rp, self.d_in, self.out, self.K, self.masked = len(ws), rp, d_in, out, K, mod.masked
        self.ok = True

    def run(self, plan, x, N, precision=0):
        """precision: SN_PREC_* of the Linears of both stage kernels (fused.PRECISIONS)."""
        import ctypes as C
        from ._lib import check, lib, ptr, stream
        K, out = self.K, self.out
        # the reduced modes are entry points of their own, with the mode in front of the stream (both record under the default's name)
        phi, chain, tail = ("sn_deepsigns_phi_prec_f32", "sn_mlp_chain_prec_f32", (int(precision), stream())) if precision else \
                           ("sn_deepsigns_phi_f32", "sn_mlp_chain_f32", (stream(),))
        z = torch.empty(N * K, out, dtype=torch.float32, device=x.device)
        with ops._span("sn_deepsigns_phi_f32"):
            check(getattr(lib(), phi)(C.byref(self.phi), ptr(x), K, ptr(plan.graph_ptr), ptr(plan.rowptr), ptr(plan.col),
                                      C.byref(plan.bins.cstruct), K, ptr(z), *tail), phi)
        y = torch.empty(N, K, dtype=torch.float32, device=x.device)
        # masked: the slot sum over the valid slots in front of rho [N, out]; else rho reads the K * out columns of a node as they lie
        width, nvalid, kv = (out, ptr(plan.nvalid), K) if self.masked else (K * out, None, 0)
        with ops._span("sn_mlp_chain_f32"):
            check(getattr(lib(), chain)(ptr(z), width, N, width, nvalid, kv, self.rho_w, self.n_rho, self.rp, ptr(y), K, K, *tail), chain)
        return y, z


def _node_counts(g):
    """(largest graph, total nodes) of the batch, read ONCE per graph object — free when batch_num_nodes() is a host tensor, one
    two-scalar read otherwise — and cached on it."""
    mc = getattr(g, "_sn_node_counts", None)
    if mc is None:
        bnn = g.batch_num_nodes()
        mc = tuple(int(v) for v in torch.stack([bnn.max(), bnn.sum()]).tolist()) if bnn.numel() else (0, 0)
        try:
            g._sn_node_counts = mc
        except Exception:
            pass
    return mc


def _max_nodes(g):
    """Largest graph of the batch (the stage kernels keep a whole graph in one 64-row bin column)."""
    return _node_counts(g)[0]


def _max_in_edges(g):
    """Most edges of one graph of the batch (the one-launch GatedGCN kernel stages a graph's in-edges in LDS), or None when the graph
    object does not say: DGL's batch_num_edges() — per-graph counts DGL keeps with the batch, like batch_num_nodes() — read ONCE per
    graph object and cached on it.  Never derived from the edge list: that is a device reduction and a host wait per new graph object,
    which the one-launch path exists to avoid (the device-side guard covers graphs whose counts are not known)."""
    me = getattr(g, "_sn_max_edges", None)
    if me is None:
        bne = getattr(g, "batch_num_edges", None)
        t = bne() if callable(bne) else None
        if t is None:
            return None
        me = int(t.max()) if t.numel() else 0
        try:
            g._sn_max_edges = me
        except Exception:
            pass
    return me


_bucket_rows = ops.bucket_validity          # (vN, vE, vB, k1) of a module under train_graph.DGLBucketedStep


def _await_side(g, plan=None):
    """The sign-invariant net may have built this graph's plan — and its own output — on its side stream (`overlap = True`): whoever picks
    the plan up on another stream first waits for that stream's event there and tells the allocator (once per graph object)."""
    pend = getattr(g, "_sn_side", None)
    if pend is None:
        return
    ev, side, tensors = pend
    cur = torch.cuda.current_stream()
    if cur.cuda_stream == side.cuda_stream:
        return
    cur.wait_event(ev)
    plans = [plan] if plan is not None else list(getattr(g, "_sn_plans", {}).values())
    for t in tuple(tensors) + tuple(a for pl in plans for a in (pl.graph_ptr, pl.evoff)):
        t.record_stream(cur)
    g._sn_side = None


def _plan_inputs(g, N, error=ops.NODE_COUNT_ERROR):
    """(batch [N], edge index [2, E], B) of a batched graph: what ops.build_plan reads.  Index plumbing only.  The node total comes from
    the graph object's cached host counts — repeat_interleave without output_size would read the sum back from the device, a host
    wait per batch and not recordable in a HIP graph — and output_size=N trusts N: a mismatch would be an uninitialised tail or a
    write past it, so it raises `error` (may name {total} and {N})."""
    src, dst = g.edges()
    bnn = g.batch_num_nodes().to(src.device)
    B = int(bnn.numel())
    total = _node_counts(g)[1]
    if total != N:
        raise ValueError(error.format(total=total, N=N))
    batch = torch.repeat_interleave(torch.arange(B, device=src.device), bnn, output_size=N)
    return batch.long(), torch.stack([src.long(), dst.long()]), B


_CACHED_PLAN_ERROR = "batch_num_nodes() sums to {total} but the feature matrix has {N} rows"       # cached_plan's own wording


def _flipped(ei):
    """The edge index of the FLIPPED graph (rows = source nodes: the out-degrees of GraphConv's norm, the CSR of an aggregation's
    adjoint); its batch vector and graph count are the graph's own."""
    return ei.flip(0).contiguous()


def cached_plan(g, N, k=None):
    """The CSR / graph_ptr plan of a batched graph (sn_batch_plan), built once per graph OBJECT and kept on it — as DGL keeps a
    graph's sparse formats on the graph.  k: also lay out the stage kernels' work bins over all k eigenvector slots (kmax = -k);
    a request without k is served by any plan already on the graph (the CSR arrays do not depend on k), so the sign-invariant net
    and the base network that consumes its output share ONE launch per batch."""
    cache = getattr(g, "_sn_plans", None)
    if cache is None:
        cache = {}
        try:
            g._sn_plans = cache
        except Exception:
            pass
    key = ("bins", int(k)) if k else ("csr",)
    if key in cache or (k is None and cache):
        plan = cache[key] if key in cache else next(iter(cache.values()))
        _await_side(g, plan)
        return plan
    batch, ei, B = _plan_inputs(g, N, _CACHED_PLAN_ERROR)
    plan = ops.build_plan(batch, ei, B, -int(k), bins=True) if k else ops.build_plan(batch, ei, B, 0)
    cache[key] = plan
    return plan


def _cached_rplan(g, N):
    """The plan of the FLIPPED edge list, kept on the graph object next to its plans and dropped with them (serving.GraphedDGLForward
    resets `_sn_plans` inside the recorded step: the flipped plan is then rebuilt there too).  Call after cached_plan(g, N)."""
    cache = getattr(g, "_sn_plans", None)
    held = getattr(g, "_sn_rplan", None)
    if held is not None and held[0] is cache:
        return held[1]
    batch, ei, B = _plan_inputs(g, N, _CACHED_PLAN_ERROR)
    rplan = ops.build_plan(batch, _flipped(ei), B, 0)
    try:
        g._sn_rplan = (cache, rplan)
    except Exception:
        pass
    return rplan


def _mlp_grad(mlp, h, act, drop, nv=None, kv=0, site0=0, tail_bn=None, tail_site=None):
    """An MLP under autograd (mlp.py:37-56: bias -> act -> BN [-> dropout] per hidden layer): rows outside (nv, kv) — the padding of a
    bucketed batch — enter no statistic and no gradient, the statistics run over ALL other rows, as in the reference.  drop = (p, snap):
    hidden layer i is followed by site `site0 + i`, one launch with the BatchNorm apply where there is one.  tail_bn / tail_site: the
    BatchNorm GIN.forward applies in front of the NEXT GINConv and the dropout site in front of it (gnns.py:105-110)."""
    from . import autograd as AG
    n = len(mlp.lins)
    for i, lin in enumerate(mlp.lins):
        last = i == n - 1
        h = AG.linear(h, lin.weight, lin.bias, nv, kv, relu=not last and act is None)
        if not last and act is not None:
            h = AG.activation(h, act, nv, kv)
        bn = tail_bn if last else (mlp.bns[i] if mlp.use_bn else None)
        if drop is not None and last and tail_site is not None:
            h = AG.dropout(h, drop[0], drop[1], tail_site)
        if drop is not None and not last:
            h = AG.bn_drop(h, bn, drop[0], drop[1], site0 + i, nv, kv) if bn is not None else AG.dropout(h, drop[0], drop[1], site0 + i)
        elif bn is not None:
            h = AG.bn_act(h, bn, nv, kv, relu=False)
    return h


class _SignInvEncoder(_EncoderDropout, nn.Module):
    """What the four sign-invariant nets share (nothing here looks into `enc`): the forward contract and its dispatch to the three
    forward paths — eval and the train-mode value (`_forward_value`), train under autograd (`_forward_grad`) — the cache of prepared
    parameters and its invalidation, rho on either path, and the per-call plans of the autograd path.  A subclass provides
    `_prepare(train) -> P` (with P["rho"]), `_enc_sites()`, `_forward_value(P, g, x, train, drop)` and `_forward_grad(g, x, drop)`."""
    masked = False

    def __init__(self):
        super().__init__()
        # fires also when a PARENT module's load_state_dict recurses into this one (its own override below does not)
        self.register_load_state_dict_post_hook(lambda m, keys=None: m._invalidate())
        self._prep = None

    @property
    def matmul_precision(self):
        """"highest" only: an encoder without stage kernels runs every Linear as the fp32 layer-path GEMM.  Assigning "high" or "medium"
        raises ValueError — a mode is never replaced by another."""
        return "highest"

    @matmul_precision.setter
    def matmul_precision(self, name):
        if name != "highest":
            raise ValueError(f"{type(self).__name__}: matmul_precision {name!r} is not built for this encoder (it has no stage kernels); "
                             "only 'highest'")

    def _invalidate(self):
        self._prep = None

    def train(self, mode=True):
        self._invalidate()
        return super().train(mode)

    def _apply(self, fn, *a, **k):
        self._invalidate()
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._invalidate()
        return super().load_state_dict(*a, **k)

    def _neg(self, x2):
        """-x of a row matrix (one launch; the constants are kept with the prepared parameters' device)."""
        c = getattr(self, "_neg1", None)
        if c is None or c[0].device != x2.device:
            c = self._neg1 = (torch.full((1,), -1.0, device=x2.device), torch.zeros(1, device=x2.device))
        return ops.masked_affine(x2, scale=c[0], shift=c[1])

    def _grad_plans(self, g, N, kmax=0, counts=None):
        """(plan, plan of the flipped edge list), built per call: under train_graph.DGLBucketedStep the graph object is a static buffer
        whose contents change between replays, so nothing is cached on it.  counts: the device count block of such a padded batch —
        its padding graphs get no slot."""
        batch, ei, B = _plan_inputs(g, N)
        return ops.build_plan(batch, ei, B, kmax, counts=counts), ops.build_plan(batch, _flipped(ei), B, kmax)

    def _rho_grad(self, z, drop=None):
        """rho under autograd: padded rows of a bucketed batch enter no statistic and no gradient; its sites start at `_rho_site0()`."""
        vN, _, _, k1 = _bucket_rows(self)
        return _mlp_grad(self.rho, z, self._act, drop, vN, k1, self._rho_site0())

    def _rho_value(self, P, z, train, drop):
        rd = None if drop is None else (drop[0], drop[1], self._rho_site0())
        return _run_mlp(P["rho"], z, train=train, drop=rd, fuse_drop=True, act=self._act)

    def _forward_stages(self, g, x, copied):
        """Hook of an encoder with stage kernels: the eval output where they serve this call, else None (the layer path follows).
        copied: x is a converted copy (dtype / layout) queued on the caller's stream a moment ago."""
        return None

    def forward(self, g, x):
        train = self.training     # train: batch statistics + running-statistics update, dropout where `p_drop` > 0
        ops.require_cuda(x)
        if x.dim() != 3 or x.shape[1] != self.k or x.shape[2] != 1:
            raise ValueError(f"expected x of shape [N, {self.k}, 1]")
        xin = x.contiguous().float()
        drop = self._drop_begin(train, x.device)      # the dropout step advances here: once per train-mode forward, never in eval
        if train and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return self._forward_grad(g, xin, drop)
        if train:
            P = self._prepare(True)          # parameters may change between training-mode calls: nothing is cached
        else:
            if self._prep is None:
                self._prep = self._prepare(False)
            P = self._prep
            y = self._forward_stages(g, xin, xin.data_ptr() != x.data_ptr())
            if y is not None:
                return y
        return self._forward_value(P, g, xin, train, drop)


class _DeepSignsBase(_SignInvEncoder):
    """The GIN pair: the layer path of the base class and, in eval, the two stage kernels in front of it."""

    def _enc_sites(self):
        """Dropout sites of ONE enc call: a hidden site per GIN MLP (mlp.py:51) and one in front of every layer but the first
        (gnns.py:105), in the order m0, d1, m1, d2, m2, ..."""
        return 2 * len(self.enc.layers) - 1

    fused_stages = True      # eval: the two stage kernels (3 launches); False forces the layer-at-a-time path
    _fused = None            # _FusedDeepSigns of the current parameters, packed by the first eval forward that may use it

    @property
    def matmul_precision(self):
        """"highest" (default) | "high" | "medium": how many of the six bf16 partial products every fp32 Linear of the fused eval
        forward pays for (enc(g, x) + enc(g, -x) and the rho MLP chain: fused.PRECISIONS) — six, three ("bf16x3") or one.
        The 8-layer encoder has no residual or LayerNorm to damp the error: "high" is 3e-5 .. 2.5e-4 of the output's scale on the
        shipped shapes, "medium" 7e-3 .. 5e-2.  Not applied in train mode and on the layer path (`fused_stages = False`, shapes the
        stage kernels do not take).  The reduced modes are built for padded hidden widths 64, 80 and 96 (hidden 49..96: every shipped
        configuration); elsewhere assigning one raises ValueError — a mode is never replaced by another."""
        return getattr(self, "_matmul_precision", "highest")

    @matmul_precision.setter
    def matmul_precision(self, name):
        from . import fused
        if self._act is not None and name != "highest":
            raise ValueError(f"{type(self).__name__}: matmul_precision {name!r} is not built for a {self._act} encoder (it runs the "
                             "layer path, not the stage kernels); only 'highest'")
        hidden = self.enc.layers[0].apply_func.lins[0].weight.shape[0]
        out = self.enc.layers[-1].apply_func.lins[-1].weight.shape[0]
        dp = max(48, 16 * ((max(hidden, out) + 15) // 16))          # the stage kernel's padded width (_FusedDeepSigns)
        fused.precision_code(name, dp // 16, fused.REDUCED_TILES_DGL, what=f"this net (hidden width {hidden})")
        self._matmul_precision = name                                # (nothing is repacked)

    @property
    def _prec(self):
        from . import fused
        return fused.PRECISIONS[self.matmul_precision]

    def _invalidate(self):
        super()._invalidate()
        self._fused = None

    def _prepare(self, train=False):
        enc = self.enc
        P = dict(gin=[], rho=_prep_mlp(self.rho, train))
        L = len(enc.layers)
        for l, conv in enumerate(enc.layers):
            nxt = _BNSite(enc.bns[l], train) if (enc.use_bn and l < L - 1) else None   # BN applied before layer l+1
            P["gin"].append(dict(eps=conv.eps, mlp=_prep_mlp(conv.apply_func, train), next_bn=nxt))
        return P

    def _plan(self, g, N, counts=None):
        """The k-slot plan of the layer path (kmax = k: `nvalid` is min(n, k) per node).  counts: the device count block of a padded
        batch (train_graph.DGLBucketedStep): its padding graphs get no slot."""
        batch, ei, B = _plan_inputs(g, N)
        return ops.build_plan(batch, ei, B, self.k, counts=counts)

    def _phi(self, P, plan, x, N, K, train=False, drop=None):
        """enc(g, x) + enc(g, -x): GIN.forward, gnns.py:102-114, twice.  drop = (p, snap): the sites of _enc_sites per call."""
        outs = []
        L = len(P["gin"])
        for sign in (0, 1):
            h = x
            s0 = ops.SIGNINV_DROP_SITE + sign * self._enc_sites()
            for l, Lp in enumerate(P["gin"]):
                a = ops.gin_aggregate(h.reshape(N, -1), plan, Lp["eps"], negate=(sign == 1 and l == 0))
                d = None if drop is None else (drop[0], drop[1], s0 + 2 * l)
                h = _run_mlp(Lp["mlp"], a.view(N * K, -1), tail_bn=Lp["next_bn"], train=train, drop=d,
                             tail_drop=s0 + 2 * l + 1 if l < L - 1 else None, fuse_drop=True, act=self._act)
            outs.append(h)
        return outs

    def _forward_grad(self, g, x, drop):
        """Differentiable train-mode forward: the same launches as the value path, recorded as
        torch.autograd.Function nodes whose backward are the hand-written adjoints of csrc/backward.hip, so that the
        gradient a DGL base network sends back into `p = sign_inv_net(g, pos_enc)` (train_ZINC_graph_regression.py:20-25)
        reaches these parameters.  With `p_drop` > 0 (dropout_signinv.py) every site of the reference draws its mask: a post-BatchNorm
        site is ONE launch with the BatchNorm apply (AG.bn_drop), an inter-layer site AG.dropout in front of the BatchNorm.

        Under the switch `_bucket` (train_graph.DGLBucketedStep) `g` is a PADDED batch: the plan gives the padding graphs no slot
        (sn_batch_plan_padded), the ops over the N*K slot rows take the node-slot vector (K on valid nodes, 0 on padding nodes: every
        slot of a valid node counts, as in the reference's BatchNorm over all rows), those over the N rows of rho the node validity."""
        from . import autograd as AG
        N, K = x.shape[0], self.k
        pad = getattr(self, "_bucket", None)
        # (the flipped plan: the out-edge CSR of the aggregation's adjoint)
        plan, rplan = self._grad_plans(g, N, K, None if pad is None else pad.counts)
        enc = self.enc
        sv, sk = (None, 0) if pad is None else (pad.node_slots, K)               # the N*K slot rows
        act = self._act
        outs = []
        L = len(enc.layers)
        for sign in (0, 1):
            h = x
            s0 = ops.SIGNINV_DROP_SITE + sign * self._enc_sites()
            for l, conv in enumerate(enc.layers):
                a = AG.gin_aggregate(h.reshape(N, -1), conv.eps, plan, rplan, negate=(sign == 1 and l == 0))
                h = _mlp_grad(conv.apply_func, a.view(N * K, -1), act, drop, sv, sk, s0 + 2 * l,
                              enc.bns[l] if (enc.use_bn and l < L - 1) else None, s0 + 2 * l + 1 if l < L - 1 else None)
            outs.append(h)
        if self.masked:
            z = AG.slot_sum(AG.masked_add(outs[0], outs[1], plan.nvalid, K), N, K, plan.nvalid)
        else:
            z = AG.masked_add(outs[0], outs[1], sv, sk).view(N, -1)
        return self._rho_grad(z, drop).view(N, K, 1)

    def _phi_eval_merged(self, P, plan, x, N, K):
        """Eval: enc(g, x) and enc(g, -x) in ONE pass — the two signs ride in the feature axis ([N, 2, K, C]), so a layer is one
        aggregation launch and two Linears instead of two and four (folded BatchNorm is row-wise, the signs never mix until the
        final sum).  Returns phi(x) + phi(-x) as [N*K, c]."""
        xm = self._neg(x.view(N * K, 1)).view(N, K, 1)
        h = torch.stack([x, xm], dim=1).contiguous()                                                        # [N, 2, K, 1]
        for Lp in P["gin"]:
            a = ops.gin_aggregate(h.reshape(N, -1), plan, Lp["eps"])
            h = _run_mlp(Lp["mlp"], a.view(N * 2 * K, -1), tail_bn=Lp["next_bn"], act=self._act)
        return ops.slot_sum(h.view(N * 2, -1), N, 2).view(N * K, -1)                                         # sum over the sign axis

    def _forward_side(self, g, xin, N, K, copied):
        """`overlap = True` (opt-in, eval, stage kernels): the batch plan and the two stage launches are queued on a side stream of this
        module and the result is handed over with an event kept on the graph object; the base network that consumes it (any net of
        dgl_nets: its first `cached_plan(g, ...)` waits for the event on ITS stream) then runs behind it, and the NEXT batch's
        sign-invariant net — queued while that network is still running — shares the GPU with it.  The returned tensor is complete only
        for consumers that go through the graph's plan (the reference's loop does: train_ZINC_graph_regression.py:20-25 hands it
        straight to the model); anything else must `torch.cuda.current_stream().wait_event(g._sn_side[0])` first.  Precondition as for
        pyg.SignNetGNN.overlap_front: the graph's tensors and x are complete on the device when forward is called."""
        from . import _lib as _lib_mod
        if getattr(self, "_side_stream", None) is None:
            self._side_stream = torch.cuda.Stream(device=xin.device)
        side = self._side_stream
        if copied:
            # x was converted (dtype / layout) by a kernel queued on the caller's stream a moment ago: the side stream must see it
            side.wait_stream(torch.cuda.current_stream(xin.device))
        with torch.cuda.stream(side), _lib_mod.stream_scope():
            y, z = self._fused.run(cached_plan(g, N, K), xin, N, self._prec)
            ev = torch.cuda.Event()
            ev.record(side)
        src, dst = g.edges()
        for t in (xin, src, dst):
            t.record_stream(side)
        y = y.view(N, K, 1)
        g._sn_side = (ev, side, (y,))
        return y

    def _forward_stages(self, g, x, copied):
        """Eval: sn_batch_plan and the two stage kernels, where the shapes are theirs (the layer path's `_prep` is packed either way)."""
        N, K = x.shape[0], self.k
        if not self.fused_stages:
            return None
        if self._fused is None:
            self._fused = _FusedDeepSigns(self)
        if not (self._fused.ok and N > 0 and _max_nodes(g) <= ops.PHI_BIN_ROWS and int(g.batch_num_nodes().numel()) <= 6144):
            return None
        if getattr(self, "overlap", False):
            return self._forward_side(g, x.view(N, K), N, K, copied)
        y, _ = self._fused.run(cached_plan(g, N, K), x.view(N, K), N, self._prec)
        return y.view(N, K, 1)

    def _forward_value(self, P, g, x, train, drop=None):
        N, K = x.shape[0], self.k
        plan = self._plan(g, N)
        if not train:
            z = self._phi_eval_merged(P, plan, x, N, K)
            if self.masked:
                z = ops.masked_affine(z, plan.nvalid, K)                     # x[~mask] = 0       (deepsigns.py:76-80)
        else:
            zp, zm = self._phi(P, plan, x, N, K, train, drop)
            z = ops.masked_affine(zp, plan.nvalid, K, residual=zm) if self.masked else ops.masked_affine(zp, residual=zm)
        # masked: sum over K ; rho(c -> hidden -> K) (deepsigns.py:81-84); else rho over the K * c columns of a node (deepsigns.py:47-49)
        z = ops.slot_sum(z, N, K) if self.masked else z.view(N, -1)
        return self._rho_value(P, z, train, drop).view(N, K, 1)


class GINDeepSigns(_DeepSignsBase):
    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, k, use_bn=False, use_ln=False, dropout=0.5,
                 activation="relu"):
        super().__init__()
        self._init_dropout(dropout, "GINDeepSigns")
        self.enc = GIN(in_channels, hidden_channels, out_channels, num_layers, use_bn=use_bn, dropout=dropout, activation=activation,
                       _activations=self._signinv_activations)
        self.rho = MLP(out_channels * k, hidden_channels, k, num_layers, use_bn=use_bn, dropout=dropout, activation=activation,
                       _activations=self._signinv_activations)
        self.k = k


class MaskedGINDeepSigns(_DeepSignsBase):
    masked = True

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, k, device=None, use_bn=False, use_ln=False,
                 dropout=0.5, activation="relu"):
        super().__init__()
        self._init_dropout(dropout, "MaskedGINDeepSigns")
        self.device = device
        self.enc = GIN(in_channels, hidden_channels, out_channels, num_layers, use_bn=use_bn, dropout=dropout, activation=activation,
                       _activations=self._signinv_activations)
        self.rho = MLP(out_channels, hidden_channels, k, num_layers, use_bn=use_bn, dropout=dropout, activation=activation,
                       _activations=self._signinv_activations)
        self.k = k


# ----------------------------------------------------------------------------- the 'gcn' and 'transformer' encoders
class _GraphConv(nn.Module):
    """dgl.nn.pytorch.GraphConv(in_feats, out_feats, norm='both', weight=True, bias=True, activation=...), restated from DGL's published
    definition (DGL is not pinned by the reference): parameters `weight` [in, out] (Glorot uniform) and `bias` [out] (zeros);
    rst = D_in^-1/2 A D_out^-1/2 h W + bias with degrees clamped to 1, the weight applied BEFORE the aggregation when in > out; a node
    without in-edges raises (allow_zero_in_degree=False)."""

    def __init__(self, in_feats, out_feats, activation=None):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(in_feats, out_feats))
        self.bias = nn.Parameter(torch.zeros(out_feats))
        nn.init.xavier_uniform_(self.weight)
        self.relu = activation == "relu"
        self.act = None if activation in (None, "relu") else activation      # 'tanh': an ops.act_affine launch behind the bias


class GCN(nn.Module):
    """layers/gnns.py:15-45: GraphConv(in, hidden, act), n_layers - 2 x GraphConv(hidden, hidden, act), GraphConv(hidden, out); before every
    layer i >= 1 the BatchNorm1d bns[i-1] over all N*K rows.  Parameters only: GCNDeepSigns runs it."""

    def __init__(self, in_channels, hidden_channels, out_channels, n_layers, use_bn=True, dropout=0.5, activation="relu",
                 _activations=("relu",)):
        super().__init__()
        if tuple(_activations) == ("relu",):
            if activation != "relu":
                raise ValueError("HIP path: only relu (what every shipped config uses)")
        else:
            _GNN_ACTIVATIONS[activation]                               # gnns.py:21
        self.layers = nn.ModuleList()
        if use_bn:
            self.bns = nn.ModuleList()
        self.use_bn = use_bn
        self.layers.append(_GraphConv(in_channels, hidden_channels, activation))
        for _ in range(n_layers - 2):
            self.layers.append(_GraphConv(hidden_channels, hidden_channels, activation))
            if use_bn:
                self.bns.append(nn.BatchNorm1d(hidden_channels))
        self.layers.append(_GraphConv(hidden_channels, out_channels))
        if use_bn:
            self.bns.append(nn.BatchNorm1d(hidden_channels))


class _MultiHeadAttention(nn.Module):
    """dgl.nn.pytorch.glob.MultiHeadAttention (the `mha` of a SetAttentionBlock), restated from DGL's published definition: bias-free
    q / k / v / o projections, a two-layer ReLU feed-forward net (indices 0 and 3 of the Sequential; 1 and 2 are ReLU and Dropout) and two
    LayerNorms (eps 1e-5); every parameter with more than one dimension Glorot uniform."""

    def __init__(self, d_model, num_heads, d_head, d_ff):
        super().__init__()
        self.d_model, self.num_heads, self.d_head, self.d_ff = d_model, num_heads, d_head, d_ff
        self.proj_q = nn.Linear(d_model, num_heads * d_head, bias=False)
        self.proj_k = nn.Linear(d_model, num_heads * d_head, bias=False)
        self.proj_v = nn.Linear(d_model, num_heads * d_head, bias=False)
        self.proj_o = nn.Linear(num_heads * d_head, d_model, bias=False)
        self.ffn = nn.Sequential(nn.Linear(d_model, d_ff), nn.ReLU(), nn.Dropout(0.0), nn.Linear(d_ff, d_model))
        self.norm_in = nn.LayerNorm(d_model)
        self.norm_inter = nn.LayerNorm(d_model)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)


class _SetAttentionBlock(nn.Module):
    def __init__(self, d_model, num_heads, d_head, d_ff):
        super().__init__()
        self.mha = _MultiHeadAttention(d_model, num_heads, d_head, d_ff)


class SetTransformerEncoder(nn.Module):
    """dgl.nn.pytorch.glob.SetTransformerEncoder(d_model, n_heads, d_head, d_ff, n_layers, block_type='sab', dropouth=0, dropouta=0):
    n_layers SetAttentionBlocks — x = norm_in(x + proj_o(attention over the nodes of the row's graph)), x = norm_inter(x + ffn(x)).
    Parameters only: TransformerDeepSigns runs it."""

    def __init__(self, d_model, n_heads, d_head, d_ff, n_layers=1):
        super().__init__()
        self.layers = nn.ModuleList([_SetAttentionBlock(d_model, n_heads, d_head, d_ff) for _ in range(n_layers)])


_ZERO_IN_DEGREE = ("There are 0-in-degree nodes in the graph: GraphConv's normalised sum is undefined for them (DGL raises DGLError here "
                   "unless allow_zero_in_degree is set, which layers/gnns.py:23-29 leaves at False)")


class GCNDeepSigns(_SignInvEncoder):
    """layers/deepsigns.py:13-31: rho(enc(g, x) + enc(g, -x)) with enc = GCN (layers/gnns.py:15-45) over [N, k, c] features and
    rho = MLP(out * k, hidden, k, num_layers).  state_dict keys `enc.layers.{l}.weight` / `.bias`, `enc.bns.{l}.*`, `rho.lins.{i}.*`,
    `rho.bns.{i}.*`.  The propagation D_in^-1/2 A D_out^-1/2 h is ONE launch per layer (sn_gcn_propagate_f32; eval: both signs in the
    slot axis); weight, bias, ReLU and the eval BatchNorm in front of the next layer are the layer-path GEMM and its epilogue (the weight
    runs first where in > out, as in GraphConv; its bias then rides in the propagation).  A node without in-edges raises ValueError."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, k, use_bn=False, use_ln=False, dropout=0.5,
                 activation="relu"):
        super().__init__()
        self._init_dropout(dropout, "GCNDeepSigns")
        if use_ln:
            raise ValueError("HIP path: only relu / no LayerNorm / no residual (what every shipped config uses)")
        self.enc = GCN(in_channels, hidden_channels, out_channels, num_layers, use_bn=use_bn, dropout=dropout, activation=activation,
                       _activations=self._signinv_activations)
        self.rho = MLP(out_channels * k, hidden_channels, k, num_layers, use_bn=use_bn, dropout=dropout, activation=activation,
                       _activations=self._signinv_activations)
        self.k = k

    def _enc_sites(self):
        """Dropout sites of ONE enc call: in front of every layer but the first (gnns.py:36)."""
        return len(self.enc.layers) - 1

    def _prepare(self, train=False):
        enc, L = self.enc, len(self.enc.layers)
        layers = []
        for l, conv in enumerate(enc.layers):
            W = conv.weight.detach()
            d_in, d_out = W.shape
            first = d_in > d_out                          # GraphConv: the weight in front of the aggregation
            b = conv.bias.detach().contiguous()
            pl = ops.PackedLinear(ops.pack_weight_t(W), d_out, d_in, None if first else b)         # weight [in, out] = Linear weight^T
            nxt = _BNSite(enc.bns[l], train) if (enc.use_bn and l < L - 1) else None               # applied before layer l + 1 (gnns.py:37-43)
            layers.append(dict(pl=pl, first=first, bias=b, width=d_out, relu=conv.relu, act=conv.act, next_bn=nxt))
        return dict(layers=layers, rho=_prep_mlp(self.rho, train))

    def _zero_in_degree(self, plan, valid=None):
        """As dgl_nets.GATNet: checked at once eagerly, handed to the collector of ops.defer_status() in a recorded step; in a padded
        batch only valid nodes count (the padding self-loops may not reach every padding node)."""
        z = plan.rowptr[1:] == plan.rowptr[:-1]
        zero = (z if valid is None else z & (valid != 0)).any()
        if ops.deferring():
            ops.defer("plan", plan)
            ops.defer("flag", zero, _ZERO_IN_DEGREE)
        elif bool(zero):
            raise ValueError(_ZERO_IN_DEGREE)

    def _enc_value(self, P, plan, rplan, h, N, S, train, drop=None):
        """GCN.forward on [N, S, c] features held as rows node * S + slot (eval: folded BatchNorm in the GEMM epilogue).
        drop = (p, snap, first site) in train mode: layer l's output is dropped (site first + l, gnns.py:36) in front of the BatchNorm."""
        n_layers = len(P["layers"])
        for l, Lp in enumerate(P["layers"]):
            site = Lp["next_bn"]
            dsite = drop[2] + l if (drop is not None and l < n_layers - 1) else None
            relu, act = Lp["relu"], Lp["act"]
            # eval: the folded BatchNorm rides with the activation; train: its batch statistics are taken behind it (the tail below)
            sc, sh = (None, None) if (train or site is None) else (site.scale, site.shift)
            if Lp["first"]:       # the weight in front: nothing follows the propagation but its bias, so the activation is a launch of its own
                z = ops.masked_linear(h, Lp["pl"])
                h = ops.gcn_propagate(z.view(N, -1), plan, rplan, Lp["bias"], Lp["width"]).view(N * S, -1)
                if act:
                    h = ops.act_affine(h, act, scale=sc, shift=sh)
                elif train:
                    if relu:
                        h = ops.masked_affine(h, relu=True)
                elif relu or site is not None:
                    h = ops.masked_affine(h, relu_pre=relu, scale=sc, shift=sh)
            else:                 # the weight behind: ReLU (and in eval the folded BatchNorm) in the GEMM's epilogue
                a = ops.gcn_propagate(h.view(N, -1), plan, rplan).view(N * S, -1)
                if act:
                    h = ops.act_affine(ops.masked_linear(a, Lp["pl"]), act, scale=sc, shift=sh)
                elif train:
                    h = ops.masked_linear(a, Lp["pl"], relu=relu)
                else:
                    h = ops.masked_linear(a, Lp["pl"], relu_pre=relu, scale=sc, shift=sh)
            if train:
                if dsite is not None:
                    h = ops.dropout(h, drop[0], drop[1], dsite)
                if site is not None:
                    sc, sh = site.affine(h, True)
                    h = ops.masked_affine(h, scale=sc, shift=sh)
        return h

    def _forward_value(self, P, g, x, train, drop=None):
        N, K = x.shape[0], self.k
        plan = cached_plan(g, N)
        rplan = _cached_rplan(g, N)
        self._zero_in_degree(plan)
        x2 = x.view(N * K, 1)
        if not train:
            # both signs in the slot axis ([N, 2, K, c]): one propagation launch per layer (folded BatchNorm is row-wise)
            h = torch.stack([x, self._neg(x2).view(N, K, 1)], dim=1).reshape(N * 2 * K, 1)
            h = self._enc_value(P, plan, rplan, h, N, 2 * K, False)
            z = ops.slot_sum(h.view(N * 2, -1), N, 2)                                  # sum over the sign axis -> [N, K * out]
        else:
            # enc(g, x) then enc(g, -x): each call normalises with its own batch statistics and moves the running statistics
            S0, ns = ops.SIGNINV_DROP_SITE, self._enc_sites()
            zp = self._enc_value(P, plan, rplan, x2, N, K, True, None if drop is None else (drop[0], drop[1], S0))
            zm = self._enc_value(P, plan, rplan, self._neg(x2), N, K, True, None if drop is None else (drop[0], drop[1], S0 + ns))
            z = ops.masked_affine(zp, residual=zm).view(N, -1)
        return self._rho_value(P, z, train, drop).view(N, K, 1)                        # deepsigns.py:27-30

    def _forward_grad(self, g, x, drop):
        """Differentiable train-mode forward: the launches of the value path as autograd nodes (the propagation's adjoint is the same
        kernel on the flipped plan).  Under the switch `_bucket` (train_graph.DGLBucketedStep) `g` is a PADDED batch: the ops over the
        N*K slot rows take the node-slot vector, those over the N rows of rho the node validity, as _DeepSignsBase._forward_grad."""
        from . import autograd as AG
        N, K = x.shape[0], self.k
        pad = getattr(self, "_bucket", None)
        plan, rplan = self._grad_plans(g, N)
        self._zero_in_degree(plan, None if pad is None else pad.node_valid)
        enc, L = self.enc, len(self.enc.layers)
        sv, sk = (None, 0) if pad is None else (pad.node_slots, K)
        x2 = x.view(N * K, 1)
        outs = []
        for sign in (0, 1):
            h = x2 if sign == 0 else self._neg(x2)
            s0 = ops.SIGNINV_DROP_SITE + sign * self._enc_sites()
            for l, conv in enumerate(enc.layers):
                d_in, d_out = conv.weight.shape
                bn = enc.bns[l] if (enc.use_bn and l < L - 1) else None
                # GraphConv's weight is [in, out]: the Linear weight is its transpose (in = 1: the same floats, viewed as a column)
                Wt = conv.weight.view(d_out, 1) if d_in == 1 else conv.weight.t()
                if d_in > d_out:
                    z = AG.linear(h, Wt, None, sv, sk)
                    h = AG.gcn_propagate(z.view(N, -1), plan, rplan, conv.bias, d_out).view(N * K, -1)
                    if conv.relu:
                        h = AG.act_residual(h, act="relu")
                    elif conv.act:
                        h = AG.activation(h, conv.act, sv, sk)
                else:
                    a = AG.gcn_propagate(h.view(N, -1), plan, rplan).view(N * K, -1)
                    h = AG.linear(a, Wt, conv.bias, sv, sk, relu=conv.relu)
                    if conv.act:
                        h = AG.activation(h, conv.act, sv, sk)
                if drop is not None and l < L - 1:
                    h = AG.dropout(h, drop[0], drop[1], s0 + l)                    # gnns.py:36, in front of the BatchNorm
                if bn is not None:
                    h = AG.bn_act(h, bn, sv, sk, relu=False)
            outs.append(h)
        z = AG.masked_add(outs[0], outs[1], sv, sk)
        return self._rho_grad(z.view(N, -1), drop).view(N, K, 1)


class TransformerDeepSigns(_SignInvEncoder):
    """layers/deepsigns.py:89-119: embed = Linear(1, hidden); enc = SetTransformerEncoder(hidden, 2 heads of hidden // 2, d_ff =
    2 * (hidden // 2), num_layers blocks); rho = MLP(hidden * k, hidden, k, 4); forward = rho(cat_i [enc(g, embed(x)[:, i]) +
    enc(g, embed(-x)[:, i])]).  `out_channels` is unused, as in the reference.  state_dict keys `embed.*`,
    `enc.layers.{l}.mha.proj_{q,k,v,o}.weight`, `enc.layers.{l}.mha.ffn.{0,3}.*`, `enc.layers.{l}.mha.norm_{in,inter}.*`, `rho.*`.
    The reference calls the encoder 2 k times per forward, each a padded dense attention per graph; here the 2 k (sign, slot) pairs ride
    in the row axis and one sn_graph_attention_f32 launch per block serves every graph, slot, sign and head."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, k, use_bn=False, use_ln=False, dropout=0.5,
                 activation="relu"):
        super().__init__()
        self._init_dropout(dropout, "TransformerDeepSigns")
        if use_ln:
            raise ValueError("HIP path: only relu / no LayerNorm / no residual (what every shipped config uses)")
        heads = 2
        d_head = hidden_channels // heads
        if d_head < 1 or d_head > ops.GRAPH_ATTENTION_MAX_HEAD:
            raise ValueError(f"TransformerDeepSigns: head width {d_head} outside 1..{ops.GRAPH_ATTENTION_MAX_HEAD} (sn_graph_attention_f32)")
        self.enc = SetTransformerEncoder(d_model=hidden_channels, n_heads=heads, d_head=d_head, d_ff=heads * d_head, n_layers=num_layers)
        self.embed = nn.Linear(1, hidden_channels)
        self.rho = MLP(hidden_channels * k, hidden_channels, k, 4, use_bn=use_bn, dropout=dropout, activation=activation,
                       _activations=self._signinv_activations)
        self.k = k

    def _enc_sites(self):
        """None: the reference builds SetTransformerEncoder with dropouth = dropouta = 0, and a call with p = 0 takes no ordinal."""
        return 0

    def _prepare(self, train=False):
        layers = []
        for blk in self.enc.layers:
            m = blk.mha
            Wqkv = torch.cat([m.proj_q.weight.detach(), m.proj_k.weight.detach(), m.proj_v.weight.detach()], dim=0)       # (a copy, no arithmetic)
            layers.append(dict(qkv=ops.PackedLinear(ops.pack_weight(Wqkv), Wqkv.shape[0], Wqkv.shape[1], None), o=_pack(m.proj_o),
                               f0=_pack(m.ffn[0]), f3=_pack(m.ffn[3]), heads=m.num_heads,
                               ln1=(m.norm_in.weight.detach(), m.norm_in.bias.detach(), m.norm_in.eps),
                               ln2=(m.norm_inter.weight.detach(), m.norm_inter.bias.detach(), m.norm_inter.eps)))
        return dict(embed=_pack(self.embed), layers=layers, rho=_prep_mlp(self.rho, train))

    def _forward_value(self, P, g, x, train, drop=None):
        """Eval and the train-mode value: the encoder has no BatchNorm, so both signs ride in the slot axis in either mode (rho's
        BatchNorms see the batch once per forward, as in the reference)."""
        N, K = x.shape[0], self.k
        S = 2 * K
        plan = cached_plan(g, N)
        h = torch.stack([x, self._neg(x.view(N * K, 1)).view(N, K, 1)], dim=1).reshape(N * S, 1)         # rows node * 2K + sign * K + slot
        h = ops.masked_linear(h, P["embed"])
        for Lp in P["layers"]:
            qkv = ops.masked_linear(h, Lp["qkv"])
            D = qkv.shape[1] // 3
            att, _ = ops.graph_attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], plan.graph_ptr, N, S, Lp["heads"])
            h = ops.masked_layernorm(ops.masked_linear(att, Lp["o"]), h, *Lp["ln1"])
            f = ops.masked_linear(ops.masked_linear(h, Lp["f0"], relu=True), Lp["f3"])
            h = ops.masked_layernorm(f, h, *Lp["ln2"])
        z = ops.slot_sum(h.view(N * 2, -1), N, 2)                                      # sum over the sign axis -> [N, K * hidden]
        return self._rho_value(P, z, train, drop).view(N, K, 1)                        # deepsigns.py:116-118

    def _forward_grad(self, g, x, drop):
        """Differentiable train-mode forward: one attention launch per block forward, one backward.  Under `_bucket` the padding nodes
        form the batch's spare graph: attention never mixes them with valid nodes, and their rows are masked out of every Linear."""
        from . import autograd as AG
        N, K = x.shape[0], self.k
        S = 2 * K
        pad = getattr(self, "_bucket", None)
        plan, _ = self._grad_plans(g, N)
        if ops.deferring():
            ops.defer("plan", plan)
        sv = None if pad is None else pad.node_slots * 2                               # 2K slot rows on valid nodes, 0 on padding (index plumbing)
        sk = 0 if pad is None else S
        h = torch.stack([x, self._neg(x.view(N * K, 1)).view(N, K, 1)], dim=1).reshape(N * S, 1)
        h = AG.linear(h, self.embed.weight, self.embed.bias, sv, sk)
        for blk in self.enc.layers:
            m = blk.mha
            Wqkv = torch.cat([m.proj_q.weight, m.proj_k.weight, m.proj_v.weight], dim=0)
            att = AG.graph_attention(AG.linear(h, Wqkv, None, sv, sk), plan.graph_ptr, N, S, m.num_heads)
            h = AG.masked_layernorm(AG.linear(att, m.proj_o.weight, None, sv, sk), h, m.norm_in.weight, m.norm_in.bias, m.norm_in.eps, sv, sk)
            f = AG.linear(AG.linear(h, m.ffn[0].weight, m.ffn[0].bias, sv, sk, relu=True), m.ffn[3].weight, m.ffn[3].bias, sv, sk)
            h = AG.masked_layernorm(f, h, m.norm_inter.weight, m.norm_inter.bias, m.norm_inter.eps, sv, sk)
        z = AG.slot_sum(h.view(N * 2, -1), N, 2)
        return self._rho_grad(z, drop).view(N, K, 1)


ENCODERS = {"gcn": GCNDeepSigns, "gin": GINDeepSigns, "masked_gin": MaskedGINDeepSigns, "transformer": TransformerDeepSigns}


def sign_inv_net_from(net_params, encoders):
    """nets/ZINC_graph_regression/sign_inv_net.py:3-17 over a table of the four classes (this module's, or the opt-in subclasses of
    dropout_signinv.py / activation_signinv.py): 'gcn', 'gin', 'masked_gin' and 'transformer' with the reference's argument lists
    (a shipped config selects 'gin' or 'masked_gin'; the main script's --sign_inv_net takes all four); anything
    else raises ValueError('Invalid sign inv net')."""
    assert net_params["sign_inv_net"] is not None, "did not specify sign inv net"
    kind = net_params["sign_inv_net"]
    if kind not in encoders:
        raise ValueError("Invalid sign inv net")
    args = (1, net_params["hidden_dim"], net_params["phi_out_dim"], net_params["sign_inv_layers"], net_params["pos_enc_dim"])
    if kind == "masked_gin":
        args += (net_params["device"],)
    return encoders[kind](*args, use_bn=True, dropout=net_params["dropout"], activation=net_params["sign_inv_activation"])


def get_sign_inv_net(net_params):
    """The reference's factory over the classes of this module (dropout 0 and ReLU only: see ENCODERS of the opt-in modules)."""
    return sign_inv_net_from(net_params, ENCODERS)
