"""The DGL tree's five base networks on the HIP layer kernels (the consumers of the sign-invariant positional
encoding in the tree that owns main_ZINC_graph_regression.py): `GINNet`, `GatedGCNNet`, `PNANet`, `TransformerNet`, `GATNet`.

Each mirrors its nets/ZINC_graph_regression/*_net.py for the configurations the shipped JSONs select — pe_init = 'lap_pe',
lap_lspe = False — with the same constructor (`net_params`), forward contract `model(g, h, p, e, snorm_n) -> (scores, g)` and
state_dict keys, and `model.sign_inv_net` attached as in the reference.  Eval, train-mode value and — with gradients enabled — the
differentiable path (autograd.py).  The LSPE / random-walk variants (p_out, Whp, lapeig loss) are not built and raise.

The baseline rows of the same table run on the same nets: pe_init = 'no_pe' (the *_NoPE configs: no embedding_p, `p` is not read and may
be None) and pe_init = 'lap_pe' behind `handle_lap` with lap_method 'sign_flip' / 'abs_val' / 'canonical' / 'none' (the *_LapPE
configs); a sign_inv_net is built for lap_method 'sign_inv' only, pe_proj for pe_aggregate 'concat' (GatedGCN, Transformer), as in
the reference.

What the five share lives in `_DGLNet`: the constructor's head and tail, the forward prologue, the input encoder and the read-out
(value and differentiable form each), `loss`, the one-launch eval kernels' eligibility (`_stage`) and their deferred error report
(`check_last`).  A net adds its layer parameters, its layer loop and, where it has them, its padded / fused eval layouts.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from types import SimpleNamespace

from . import autograd as AG
from . import ops
from ._lib import check, lib, ptr, stream
from .dgl_deepsigns import MLP, cached_plan, _await_side, _bucket_rows, _max_nodes, _max_in_edges, _node_counts, _BNSite, _GINConv, _fold_bn_before, _pack, _pad_mat, _prep_mlp, _run_mlp, get_sign_inv_net


def handle_lap(model, batch_pos_enc, batch_graphs, device=None, *, u=None):
    """train/train_ZINC_graph_regression.py:13-51: the raw Laplacian positional encoding [N, k] as `model.lap_method` hands it to the
    net — 'sign_inv' through model.sign_inv_net, 'none' unchanged, 'sign_flip' / 'abs_val' / 'canonical' through ONE launch of
    sn_lap_pe_transform_f32 (no host read: recordable).  'sign_flip' draws torch.rand(k) from the CPU default generator, as the
    reference does (the same torch.manual_seed gives the same flips), and uploads it through pinned memory without a blocking copy;
    `u`: the k uniforms instead (host or device; the static buffer of a captured step).  'canonical' reads graph_ptr from
    cached_plan(batch_graphs, N): the plan the net's value paths use.  `device`: accepted for the reference's signature; the
    encoding's own device is used.  Any other method: the reference's ValueError."""
    method = model.lap_method
    if method == "sign_inv":
        return model.sign_inv_net(batch_graphs, batch_pos_enc.unsqueeze(-1)).squeeze(-1)          # n x k -> n x k x 1 -> n x k (:20-25)
    if method == "none":
        return batch_pos_enc                                                                      # raw eigenvectors (:45-47)
    if method not in ("sign_flip", "abs_val", "canonical"):
        raise ValueError("invalid laplacian method")
    ops.require_cuda(batch_pos_enc)
    p = batch_pos_enc.detach().contiguous().float()
    if method == "abs_val":
        return ops.lap_pe_transform(p, "abs_val")
    if method == "sign_flip":
        if u is None:
            u = torch.rand(p.size(1))                                                             # (:15: the CPU default generator)
        u = u.detach().reshape(-1).float()
        if not u.is_cuda:
            u = u.pin_memory().to(p.device, non_blocking=True)
        return ops.lap_pe_transform(p, "sign_flip", u=u.contiguous())
    return ops.lap_pe_transform(p, "canonical", graph_ptr=cached_plan(batch_graphs, p.shape[0]).graph_ptr)


_READOUT_MODE = {"sum": 0, "mean": 1, "max": 2}       # SN_READOUT_* of signnet_hip.h; any other name pools as mean, as before


def _check_pe_init(name, pe_init, lap_lspe, use_lapeig_loss):
    """What every net here covers of the PE switches: pe_init 'lap_pe' (the LapPE rows: sign_inv, sign_flip, abs_val, canonical, none)
    or 'no_pe' (the NoPE rows), without LSPE and without the eigenvector loss."""
    if pe_init not in ("lap_pe", "no_pe") or lap_lspe or use_lapeig_loss:
        raise NotImplementedError(f"HIP {name} covers pe_init='lap_pe' / 'no_pe' with lap_lspe=False, use_lapeig_loss=False "
                                  "(the sign-invariant, LapPE and NoPE configs)")


def _zero_pe(net, N, dev):
    """[>= N, 1] zeros, kept with the eval cache: the positional encoding a NoPE net hands to a one-launch kernel whose input stage
    adds a projection of it (the projection is zero too: the stage computes embedding_h alone)."""
    make = lambda: torch.zeros(max(int(N), 256), 1, dtype=torch.float32, device=dev)
    z = net._cached("zero_pe", make)
    if z.shape[0] < N or z.device != dev:          # grown on demand
        del net._cache["zero_pe"]
        z = net._cached("zero_pe", make)
    return z


class MLPReadout(nn.Module):
    """layers/mlp_readout_layer.py:9-24: L halving Linear+ReLU layers, then Linear to the output."""

    def __init__(self, input_dim, output_dim, L=2):
        super().__init__()
        dims = [input_dim // 2 ** l for l in range(L + 1)]
        self.FC_layers = nn.ModuleList([nn.Linear(dims[l], dims[l + 1], bias=True) for l in range(L)] +
                                       [nn.Linear(dims[L], output_dim, bias=True)])
        self.L = L


class _PackCache:
    """Eval-mode cache of packed Linears / folded BatchNorms (rebuilt after train(), .to(), load_state_dict(); call
    `invalidate()` after changing parameters in place while in eval mode).  Train mode packs per call: parameters move."""

    def invalidate(self):
        self._cache = {}

    def train(self, mode=True):
        self._cache = {}
        return super().train(mode)

    def _apply(self, fn, *a, **k):
        self._cache = {}
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._cache = {}
        return super().load_state_dict(*a, **k)

    def _load_from_state_dict(self, *a, **k):
        # reached also when a PARENT module's load_state_dict recurses into this one (the override above is not)
        self._cache = {}
        return super()._load_from_state_dict(*a, **k)

    def _cached(self, key, build):
        """The cache's entry `key`, made by `build()` on its first use since the cache was emptied."""
        c = self.__dict__.setdefault("_cache", {})
        if key not in c:
            c[key] = build()
        return c[key]

    def _pk(self, lin):
        return _pack(lin) if self.training else self._cached(id(lin), lambda: _pack(lin))

    def _bn(self, bn, train):
        return _BNSite(bn, True) if train else self._cached(id(bn), lambda: _BNSite(bn, False))

    def _abde(self, L):
        """The four node Linears of a GatedGCN layer packed as one [4d, d] Linear (eval cache)."""
        def build():
            W = torch.cat([getattr(L, n).weight.detach() for n in "ABDE"], 0).contiguous()
            b = torch.cat([getattr(L, n).bias.detach() for n in "ABDE"], 0).contiguous()
            return ops.PackedLinear(ops.pack_weight(W), W.shape[0], W.shape[1], b)
        return self._cached(("abde", id(L)), build)

    def _mlp(self, mlp, train):
        return _prep_mlp(mlp, True) if train else self._cached(id(mlp), lambda: _prep_mlp(mlp, False))


class _DGLNet(ops.DropoutHolder, _PackCache, nn.Module):
    """What GINNet, GatedGCNNet, PNANet, TransformerNet and GATNet share.  A net's __init__ is `_init_common`, its own layers,
    `_init_tail`; its forward is `_prologue`, then `_encode` / its layer loop / `_readout` (or their `_grad` forms)."""

    _max_readout = False     # readout 'max' is refused, as before; readout_models.py's subclasses set True
    _feature_dropout = False # dropout / in_feat_dropout > 0 are refused, as before; dropout_models.py's subclasses set True
    _sign_inv_factory = staticmethod(get_sign_inv_net)     # builds `sign_inv_net`; dropout_signinv.py's subclasses hand in their own
    _stage_cls = None        # the packer of the net's one-launch eval kernel (_FusedGin, _FusedGated, _FusedTransformer), if it has one
    _stage_edges = 192       # the most in-edges of a graph that kernel holds; None: the packer's own `max_edges`
    _malformed_note = ""     # check_last()'s wording of a malformed batch and of the size limit
    _limit_text = "192 in-edges"

    def _init_common(self, net_params, name, refusals, *, edge_dim=None, in_feat_dropout=None):
        """The constructor's head: the attributes every net reads from `net_params`, the refusals — the PE switches, then `refusals`
        ((condition, what the net covers instead) pairs, in order) —, the two dropout probabilities and the input embeddings.  `edge_dim`: the width of
        embedding_e where it is not hidden_dim; `in_feat_dropout`: where the reference registers its nn.Dropout ('before_h': in front
        of embedding_h, 'after_e': behind embedding_e; None: the net has none)."""
        p = net_params
        hidden = p["hidden_dim"]
        self._who = name
        self.n_layers, self.readout, self.batch_norm = p["L"], p["readout"], p["batch_norm"]
        self.residual, self.edge_feat, self.device = p["residual"], p["edge_feat"], p["device"]
        self.pe_init, self.lap_method, self.lap_lspe = p["pe_init"], p["lap_method"], p["lap_lspe"]
        self.use_lapeig_loss, self.lambda_loss, self.alpha_loss = p["use_lapeig_loss"], p["lambda_loss"], p["alpha_loss"]
        self.pos_enc_dim = p["pos_enc_dim"]
        _check_pe_init(name, self.pe_init, self.lap_lspe, self.use_lapeig_loss)
        for refused, covered in refusals:
            if refused:
                raise NotImplementedError(f"HIP {name}: {covered}")
        # train-mode dropout (ops.dropout: counter-based masks, site = the ordinal of the reference forward's dropout call; site 0 is
        # in_feat_dropout).  Eval never reads either value.
        self.p_in_feat = ops.check_dropout_p(p.get("in_feat_dropout", 0.0), f"HIP {name}: in_feat_dropout")
        self.p_drop = ops.check_dropout_p(p.get("dropout", 0.0), f"HIP {name}: dropout")
        if (self.p_in_feat or self.p_drop) and not self._feature_dropout:      # opt-in: the classes of dropout_models.py take it
            raise NotImplementedError(f"HIP {name}: dropout 0.0 (as in the shipped configs)")
        if self.pe_init == "lap_pe":
            self.embedding_p = nn.Linear(self.pos_enc_dim, hidden)
        if in_feat_dropout == "before_h":
            self.in_feat_dropout = nn.Dropout(self.p_in_feat)
        self.embedding_h = nn.Embedding(p["num_atom_type"], hidden)
        self.embedding_e = nn.Embedding(p["num_bond_type"], edge_dim or hidden) if self.edge_feat else nn.Linear(1, hidden)
        if in_feat_dropout == "after_e":
            self.in_feat_dropout = nn.Dropout(self.p_in_feat)

    def _init_tail(self, net_params):
        """The constructor's tail, behind the net's own layers: the read-out MLP, `g`, sign_inv_net and pe_proj, in the reference's order."""
        self.MLP_layer = MLPReadout(net_params["out_dim"], 1)
        self.g = None
        if self.lap_method == "sign_inv":
            self.sign_inv_net = self._sign_inv_factory(net_params)
        if getattr(self, "pe_aggregate", "add") == "concat":
            self.pe_proj = nn.Linear(2 * net_params["hidden_dim"], net_params["hidden_dim"])

    # ------------------------------------------------------------------ forward: prologue, input encoder, read-out
    def _prologue(self, g, h, p):
        """-> (pe, N, hidx, p, train, grad): whether p is read, the node count, the atom types as int64 [N], p as contiguous float (None
        for NoPE: p is not read, as in the reference), the mode, and whether this call takes the differentiable path."""
        _await_side(g)          # a sign_inv_net in overlap mode hands p over with an event kept on the graph
        ops.require_cuda(h)
        pe = self.pe_init == "lap_pe"
        if pe and p is None:
            raise NotImplementedError(f"HIP {self._who} with pe_init='lap_pe' needs the positional encoding p")
        N = h.shape[0]
        train = self.training
        grad = train and torch.is_grad_enabled() and any(q.requires_grad for q in self.parameters())
        return pe, N, h.long().reshape(N), p.contiguous().float() if pe else None, train, grad

    def _drop_snap(self, train, device):
        """The {seed, step} snapshot of this train-mode forward (the step advances once, here), or None when no site is active."""
        return self._dropout_begin(device) if train and self._dropout_active() else None

    def _plan(self, g, N):
        src, dst = g.edges()
        bnn = g.batch_num_nodes().to(src.device)
        B = int(bnn.numel())
        # (the node total comes from the graph object's cached host counts: repeat_interleave without output_size would read the sum
        #  back from the device — a host wait per batch, and not recordable in a HIP graph)
        if _node_counts(g)[1] != N:
            raise ValueError("batch_num_nodes does not sum to the number of feature rows")
        batch = torch.repeat_interleave(torch.arange(B, device=src.device), bnn, output_size=N)      # index plumbing only
        return batch.long(), torch.stack([src.long(), dst.long()]), B

    def _encode(self, x, p, snap=None):
        """The input encoder of the value paths behind x = embedding_h(h): h + embedding_p(p), or pe_proj(cat[h, embedding_p(p)]) for
        pe_aggregate 'concat' (gatedgcn_net.py:93-103, transformer_net.py:96-102); NoPE leaves h alone.  snap: a train-mode forward's
        dropout snapshot — in_feat_dropout (site 0) acts on embedding_h(h) first."""
        if snap is not None and self.p_in_feat:
            x = ops.dropout(x, self.p_in_feat, snap, 0)
        if self.pe_init != "lap_pe":
            return x
        if getattr(self, "pe_aggregate", "add") == "concat":
            pp = ops.masked_linear(p, self._pk(self.embedding_p))
            return ops.masked_linear(torch.cat([x, pp], dim=1), self._pk(self.pe_proj))
        return ops.masked_linear(p, self._pk(self.embedding_p), residual=x)

    def _encode_grad(self, hidx, p, vN, k1, snap=None):
        """embedding_h and the input encoder as autograd nodes (vN, k1: the valid rows of a padded batch, see _bucket_rows)."""
        x = AG.embedding_sum(hidx, [self.embedding_h.weight])
        if snap is not None and self.p_in_feat:
            x = AG.dropout(x, self.p_in_feat, snap, 0)
        if self.pe_init != "lap_pe":
            return AG.mask_rows(x, vN, k1)
        pp = AG.linear(p, self.embedding_p.weight, self.embedding_p.bias, vN, k1)
        if getattr(self, "pe_aggregate", "add") == "concat":
            return AG.linear(torch.cat([x, pp], dim=1), self.pe_proj.weight, self.pe_proj.bias, vN, k1)
        return AG.masked_add(pp, x, vN, k1)

    def _readout(self, x, plan, first=None):
        """mean / sum / max pooling over each graph's nodes, then MLPReadout.  `first`: the first Linear packed for padded channels of x."""
        if self.readout == "max":
            hg = ops.segment_max(x, plan)
        else:
            hg = ops.segment_pool(x, plan, "mean" if self.readout != "sum" else "add")
        fcs = self.MLP_layer.FC_layers
        for i, fc in enumerate(fcs):
            hg = ops.masked_linear(hg, first if i == 0 and first is not None else self._pk(fc), relu=i < len(fcs) - 1)
        return hg

    def _readout_grad(self, x, plan, vB, k1):
        if self.readout == "max":
            hg = AG.segment_max(x, plan)
        else:
            hg = AG.segment_pool(x, plan, "mean" if self.readout != "sum" else "add")
        fcs = self.MLP_layer.FC_layers
        for i, fc in enumerate(fcs):
            hg = AG.linear(hg, fc.weight, fc.bias, vB, k1, relu=i < len(fcs) - 1)
        return hg

    def loss(self, scores, targets):
        """*_net.py `loss` with use_lapeig_loss = False: the L1 task loss (a torch reduction over B scalars)."""
        return (scores - targets).abs().mean()

    # ------------------------------------------------------------------ the one-launch eval kernels: eligibility, deferred errors
    def _stage(self, g):
        """The packed stage-kernel parameters if this batch can take the net's one-launch eval path, else None.  A graph with more than
        64 nodes, or more in-edges than the kernel's LDS image holds (192; GatedGCN: sn_gatedgcn_max_edges(d), 176 at hidden 68), takes
        the layer path, as the reference evaluates any graph: both counts come with a DGL batch (batch_num_nodes(), batch_num_edges())
        and are read once per graph object.  A duck-typed graph without edge counts reaches the kernel, which flags such a graph on
        the device — NaN score, check_last()."""
        if self._stage_cls is None or self.training or not self.fused_stages:
            return None
        fz = self._cached("stage", lambda: self._stage_cls(self))
        if not fz.ok:
            return None
        me = _max_in_edges(g)
        return fz if 0 < _max_nodes(g) <= 64 and (me is None or me <= (self._stage_edges or fz.max_edges)) else None

    def check_last(self):
        """Raise what the last one-launch eval forward flagged on the device (its scores are NaN in that case): a node / edge type
        outside the embedding tables (IndexError, as nn.Embedding), a malformed batch, or a graph the stage kernel could not hold.  One
        host sync; also run by train().  The layer path (fused_stages = False, train mode; PNA and GAT always) raises immediately
        instead and leaves nothing to check."""
        plan, self._last_plan = getattr(self, "_last_plan", None), None
        if plan is None:
            return
        st = plan.status.tolist()
        if st[3] or st[5]:
            plan.status[3:6].zero_()         # (the plan is cached on the graph object: a later forward of the same graph starts clean)
        if st[0]:
            raise ValueError(f"{self._who}: the last batch is malformed ({self._malformed_note}sn_batch_plan status {st[0]})")
        if (st[3] & 4) or st[5]:
            raise IndexError(ops.EMBEDDING_INDEX_ERROR)
        if st[3] & 8:
            raise RuntimeError(f"{self._who}: a graph of the last batch has no nodes; its score is NaN — set fused_stages = False "
                               "for such batches")
        if st[3] & 3:
            raise RuntimeError(f"{self._who}: a graph of the last batch has more than 64 nodes or {self._limit_text}; its score is "
                               "NaN — set fused_stages = False for such batches")

    def train(self, mode=True):
        self.check_last()
        return super().train(mode)


class _FusedGin:
    """Packed eval-mode parameters of a GINNet for sn_gin_net_fused_f32: embedding_h + embedding_p, every GIN layer, the readout and
    MLPReadout in ONE launch — one workgroup per graph on the stage kernel of the PyG tree's GINE net (csrc/fused_gnn.hip, DGL mode).
    `ok` False: shapes the kernel does not take (width > 128, more than 16 layers, MLPs that are not the reference's
    Linear-ReLU-BN-Linear, a readout other than the 3-Linear MLPReadout to one score) — the layer path serves those."""

    def __init__(self, net):
        from .fused import _GnnParams, GNN_MAX_LAYERS
        self.ok = False
        convs, fcs = list(net.layers), list(net.MLP_layer.FC_layers)
        nope = net.pe_init != "lap_pe"       # NoPE: a zero projection of a one-column zero encoding (h = embedding_h(h) + 0)
        hid, kp = net.embedding_h.weight.shape[1], 1 if nope else net.embedding_p.weight.shape[1]
        widths = [hid] + [w for c in convs for w in (c.apply_func.lins[0].weight.shape[0], c.apply_func.lins[-1].weight.shape[0])] + \
                 [fc.weight.shape[0] for fc in fcs[:-1]]
        dmax = max(widths + [kp])
        if dmax > 128 or len(convs) > GNN_MAX_LAYERS or len(convs) < 1 or len(fcs) != 3 or fcs[2].weight.shape[0] != 1:
            return
        if any(len(c.apply_func.lins) != 2 for c in convs):
            return
        dp = 64 if dmax <= 64 else (96 if dmax <= 96 else 128)
        dev = net.embedding_h.weight.device
        keep = self._keep = []

        def hold(t):
            keep.append(t)
            return t.data_ptr()

        ones = torch.ones(dp, dtype=torch.float32, device=dev)
        P = _GnnParams()
        P.d, P.n_layers, P.n_out = dp, len(convs), 1
        P.node_discrete, P.node_nf, P.edge_discrete, P.edge_nf = 1, 1, 0, 0
        P.node_vocab, P.edge_vocab = net.embedding_h.weight.shape[0], 0
        E = torch.zeros(net.embedding_h.weight.shape[0], dp, dtype=torch.float32, device=dev)
        E[:, :hid].copy_(net.embedding_h.weight.detach())
        P.ntab[0] = hold(E)
        P.rho_out_w = None
        P.lin_a = hold(ops.pack_split(torch.eye(dp, dtype=torch.float32, device=dev)))
        if nope:
            P.lin_b = hold(ops.pack_split(torch.zeros(dp, dp, dtype=torch.float32, device=dev), torch.zeros(dp, dtype=torch.float32, device=dev)))
        else:
            P.lin_b = hold(ops.pack_split(_pad_mat(net.embedding_p.weight, dp), ops.pad_vec(net.embedding_p.bias, dp)))
        for l, conv in enumerate(convs):
            m = conv.apply_func
            site = net._bn(m.bns[0], False) if m.use_bn else None        # the BatchNorm between the ReLU and the second Linear: folded
            W2, b2 = _fold_bn_before(m.lins[1], site)
            Lp = P.layers[l]
            Lp.w1s = hold(ops.pack_split(_pad_mat(m.lins[0].weight, dp), ones, ops.pad_vec(m.lins[0].bias, dp)))
            Lp.w2s = hold(ops.pack_split(_pad_mat(W2, dp), ones, ops.pad_vec(b2, dp)))
            Lp.eps = hold(conv.eps.detach().float().reshape(1).contiguous())
        P.head_w1 = hold(ops.pack_split(_pad_mat(fcs[0].weight, dp), ones, ops.pad_vec(fcs[0].bias, dp)))
        self.head_mid = hold(ops.pack_split(_pad_mat(fcs[1].weight, dp), ones, ops.pad_vec(fcs[1].bias, dp)))
        P.head_w2 = hold(ops.pack_split(_pad_mat(fcs[2].weight, dp), ops.pad_vec(fcs[2].bias, dp)))
        self.params, self.kp, self.pool_mean = P, kp, _READOUT_MODE.get(net.readout, 1)
        self.ok = True

    def run(self, plan, hidx, p):
        """atom types [N] int64, positional encoding [N, k] -> scores [B, 1]"""
        y = torch.empty(plan.B, 1, dtype=torch.float32, device=p.device)
        with ops._span("sn_gin_net_fused_f32"):
            check(lib().sn_gin_net_fused_f32(C.byref(self.params), self.head_mid, self.pool_mean, ptr(hidx), ptr(p), p.shape[1], self.kp,
                                             ptr(plan.graph_ptr), plan.B, ptr(plan.rowptr), ptr(plan.col), ptr(plan.eperm),
                                             ptr(plan.status), ptr(y), ptr(plan.status), 8, stream()), "sn_gin_net_fused_f32")
        return y


class GINNet(_DGLNet):
    """nets/ZINC_graph_regression/gin_net.py:19-139 for the configuration GIN_ZINC_LapPE_signinv_GIN.json selects:
    `h = embedding_h(h) + embedding_p(p)` (:80-92), L x dgl GINConv(MLP(hidden, hidden, out, 2, use_bn), 'sum') (:58-66, 99-100),
    mean / sum readout (:126-133), MLPReadout."""

    fused_stages = True      # eval: embeddings, every layer and the readout in ONE launch (sn_gin_net_fused_f32); False: the layer path
    _stage_cls = _FusedGin

    def __init__(self, net_params):
        super().__init__()
        p = net_params
        hidden, out_dim = p["hidden_dim"], p["out_dim"]
        self._init_common(p, "GINNet", [(p["readout"] == "max" and not self._max_readout, "readout 'sum' or 'mean'")], in_feat_dropout="after_e")      # (embedding_e: unused by GIN)
        self.layers = nn.ModuleList(
            [_GINConv(MLP(hidden, hidden, hidden, 2, use_bn=self.batch_norm, dropout=self.p_drop, activation="relu")) for _ in range(self.n_layers - 1)] +
            [_GINConv(MLP(hidden, hidden, out_dim, 2, use_bn=self.batch_norm, dropout=self.p_drop, activation="relu"))])
        self._init_tail(p)

    def _gin_padded(self):
        """Eval cache: the net's parameters with every channel axis zero-padded to a multiple of 4 (pad rows / columns of the weights,
        pad entries of biases and folded BatchNorms are zero, so pad channels stay exactly 0 through ReLU and the aggregations)."""
        return self._cached("gin_padded", self._pad_gin)

    def _pad_gin(self):
        dev = self.embedding_h.weight.device
        up = lambda k: (k + 3) // 4 * 4

        def padw(lin, rows, cols):           # (a rectangular pad: _pad_mat makes squares)
            Wp = torch.zeros(rows, cols, dtype=torch.float32, device=dev)
            Wp[:lin.weight.shape[0], :lin.weight.shape[1]] = lin.weight.detach().float()
            return ops.PackedLinear(ops.pack_weight(Wp), rows, cols, ops.pad_vec(lin.bias, rows))

        hid = self.embedding_h.weight.shape[1]
        E = torch.zeros(self.embedding_h.weight.shape[0], up(hid), dtype=torch.float32, device=dev)
        E[:, :hid] = self.embedding_h.weight.detach().float()
        P = {"emb_h": E}
        if self.pe_init == "lap_pe":
            P["emb_p"] = padw(self.embedding_p, up(hid), self.embedding_p.weight.shape[1])
        layers, keep = [], []
        for conv in self.layers:
            m = conv.apply_func
            chain = []
            for i, lin in enumerate(m.lins):
                rows, site = up(lin.weight.shape[0]), None
                if m.use_bn and i < len(m.lins) - 1:
                    s0 = self._bn(m.bns[i], False)          # a folded BatchNorm on the padded channels (what _run_mlp reads)
                    site = SimpleNamespace(scale=ops.pad_vec(s0.scale, rows), shift=ops.pad_vec(s0.shift, rows))
                chain.append((padw(lin, rows, up(lin.weight.shape[1])), site))
            # the whole MLP as one sn_mlp_chain_f32 launch: Linear -> ReLU -> [BatchNorm folded into the next Linear] ... -> Linear
            fused = None
            widths = [up(m.lins[0].weight.shape[1])] + [up(l.weight.shape[0]) for l in m.lins]
            rp = max(48, 16 * ((max(widths) + 15) // 16))
            if rp <= 128 and len(m.lins) <= 16:
                ws = []
                for i, lin in enumerate(m.lins):
                    site = self._bn(m.bns[i - 1], False) if (m.use_bn and i > 0) else None
                    Wf, bf = _fold_bn_before(lin, site)
                    ws.append(ops.pack_split(_pad_mat(Wf, rp), ops.pad_vec(bf, rp), None, None))
                keep.extend(ws)
                fused = ((C.c_void_p * len(ws))(*[w.data_ptr() for w in ws]), len(ws), rp, up(m.lins[-1].weight.shape[0]))
            layers.append((conv.eps, chain, fused))
        P["layers"] = layers
        P["keep"] = keep
        fc0 = self.MLP_layer.FC_layers[0]
        P["fc0"] = padw(fc0, fc0.weight.shape[0], up(fc0.weight.shape[1]))
        return P

    def forward(self, g, h, p, e, snorm_n=None):
        pe, N, hidx, p, train, grad = self._prologue(g, h, p)
        if grad:
            batch, ei, B = self._plan(g, N)
            plan = ops.build_plan(batch, ei, B, 0)
            y = self._forward_grad(plan, batch, ei, B, hidx, p)
        else:
            plan = cached_plan(g, N)       # the sign-invariant net's plan of this graph object, if there is one: ONE sn_batch_plan per batch
            with torch.no_grad():
                fz = self._stage(g)
                if fz is not None:
                    # no host sync on this path: a bad atom type / an oversize graph is flagged in the plan's status block, the score is
                    # NaN, check_last() raises
                    self._last_plan = plan
                    y = fz.run(plan, hidx.contiguous(), p if pe else _zero_pe(self, N, h.device)[:N])
                elif not train and self.embedding_h.weight.shape[1] % 4:
                    # eval, hidden width not a multiple of 4 (GIN_ZINC_LapPE_signinv_GIN.json: 95): every row would be misaligned and every
                    # Linear on the scalar kernel; run on zero-padded channels instead (`_gin_padded`: 95 -> 96, all rows 16-byte aligned)
                    P = self._gin_padded()
                    x = ops.embedding_sum(hidx, [P["emb_h"]])
                    if pe:
                        x = ops.masked_linear(p, P["emb_p"], residual=x)
                    for eps, chain, fused in P["layers"]:
                        a = ops.gin_aggregate(x, plan, eps)
                        if fused is None:
                            x = _run_mlp(chain, a)
                            continue
                        ws, n_l, rp, d_out = fused                     # the layer's MLP in one launch (sn_mlp_chain_f32)
                        x = torch.empty(a.shape[0], d_out, dtype=torch.float32, device=a.device)
                        with ops._span("sn_mlp_chain_f32"):
                            check(lib().sn_mlp_chain_f32(ptr(a), a.shape[1], a.shape[0], a.shape[1], None, 0, ws, n_l, rp, ptr(x), d_out, d_out,
                                                         stream()), "sn_mlp_chain_f32")
                    y = self._readout(x, plan, first=P["fc0"])
                else:
                    snap = self._drop_snap(train, h.device)
                    x = self._encode(ops.embedding_sum(hidx, [self.embedding_h.weight]), p, snap)          # h + embedding_p(p)   (:87-92)
                    site = 1                # mlp.py:51: one dropout behind every hidden layer of every GINConv's MLP, in forward order
                    for conv in self.layers:
                        a = ops.gin_aggregate(x, plan, conv.eps)
                        mlp = conv.apply_func
                        x = _run_mlp(self._mlp(mlp, train), a, train=train, drop=(mlp.dropout, snap, site) if snap is not None else None)
                        site += len(mlp.lins) - 1
                    y = self._readout(x, plan)
        self.g = g
        return y, g

    def _forward_grad(self, plan, batch, ei, B, hidx, p):
        vN, _, vB, k1 = _bucket_rows(self)          # (train_graph.DGLBucketedStep: padding rows enter no statistic and no gradient)
        rplan = ops.build_plan(batch, ei.flip(0).contiguous(), B, 0)
        snap = self._drop_snap(True, hidx.device)
        x = self._encode_grad(hidx, p, vN, k1, snap)
        site = 1
        for conv in self.layers:
            mlp = conv.apply_func
            a = AG.gin_aggregate(x, conv.eps, plan, rplan)
            n = len(mlp.lins)
            for i, lin in enumerate(mlp.lins):
                a = AG.linear(a, lin.weight, lin.bias, vN, k1, relu=i < n - 1)
                if mlp.use_bn and i < n - 1:
                    a = AG.bn_act(a, mlp.bns[i], vN, k1, relu=False)
                if i < n - 1:
                    if mlp.dropout:
                        a = AG.dropout(a, mlp.dropout, snap, site)
                    site += 1
            x = a
        return self._readout_grad(x, plan, vB, k1)


# ---------------------------------------------------------------------------------------------------------------
class GatedGCNLayer(nn.Module):
    """layers/gatedgcn_layer.py:12-81 (parameters only; the arithmetic is in GatedGCNNet.forward)."""

    def __init__(self, input_dim, output_dim, dropout, batch_norm, residual=False, graph_norm=True, feature_dropout=False):
        super().__init__()
        if (dropout and not feature_dropout) or graph_norm:
            raise NotImplementedError("HIP GatedGCNLayer: dropout 0.0 and graph_norm=False (what gatedgcn_net.py builds for lap_pe)")
        self.dropout = ops.check_dropout_p(dropout, "HIP GatedGCNLayer")
        self.in_channels, self.out_channels = input_dim, output_dim
        self.batch_norm, self.residual = batch_norm, residual and input_dim == output_dim
        for n in "ABCDE":
            setattr(self, n, nn.Linear(input_dim, output_dim, bias=True))
        self.bn_node_h = nn.BatchNorm1d(output_dim)
        self.bn_node_e = nn.BatchNorm1d(output_dim)


GATED_MAX_LAYERS = 32


class _GatedLayerC(C.Structure):
    _fields_ = [("wabde", C.c_void_p), ("wc", C.c_void_p), ("h_scale", C.c_void_p), ("h_shift", C.c_void_p), ("residual", C.c_int),
                ("reserved", C.c_int)]


class _GatedParamsC(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("d", "d_out", "n_layers", "readout_mean", "ro_d1", "ro_d2")] + \
               [(n, C.c_void_p) for n in ("ro_w0", "ro_b0", "ro_w1", "ro_b1", "ro_w2", "ro_b2")] + \
               [("layers", _GatedLayerC * GATED_MAX_LAYERS)]


class _FusedGated:
    """Packed eval-mode parameters of a GatedGCNNet's layer stack + readout for sn_gatedgcn_fused_f32 (one launch).  `ok` False:
    shapes the stage kernel does not take (hidden not a multiple of 4 in [4, 96], a readout other than the 3-Linear MLPReadout,
    differing layer widths) — the layer path serves those."""

    def __init__(self, net):
        self.ok = False
        Ls = list(net.layers)
        d = Ls[0].in_channels
        fcs = list(net.MLP_layer.FC_layers)
        if not (4 <= d <= 96 and d % 4 == 0 and len(Ls) <= GATED_MAX_LAYERS and len(fcs) == 3 and fcs[2].weight.shape[0] == 1):
            return
        dp = max(48, 16 * ((d + 15) // 16))
        if any(L.in_channels != d for L in Ls) or any(L.out_channels != d for L in Ls[:-1]) or Ls[-1].out_channels > dp:
            return
        if fcs[0].weight.shape[0] > 128 or fcs[1].weight.shape[0] > 128 or fcs[0].weight.shape[1] != Ls[-1].out_channels:
            return
        keep = self._keep = []

        def hold(t):
            keep.append(t)
            return t.data_ptr()

        dev = Ls[0].A.weight.device
        P = _GatedParamsC()
        P.d, P.d_out, P.n_layers, P.readout_mean = d, Ls[-1].out_channels, len(Ls), _READOUT_MODE.get(net.readout, 1)
        P.ro_d1, P.ro_d2 = fcs[0].weight.shape[0], fcs[1].weight.shape[0]
        for i, fc in enumerate(fcs):
            setattr(P, f"ro_w{i}", hold(fc.weight.detach().float().contiguous()))
            setattr(P, f"ro_b{i}", hold(fc.bias.detach().float().contiguous()))
        rows_a, rows_c = 4 * dp, dp
        for l, L in enumerate(Ls):
            W = torch.zeros(rows_a, dp, dtype=torch.float32, device=dev)
            b = torch.zeros(rows_a, dtype=torch.float32, device=dev)
            for k, nme in enumerate("ABDE"):
                lin = getattr(L, nme)
                W[k * dp:k * dp + lin.weight.shape[0], :lin.weight.shape[1]].copy_(lin.weight.detach())
                b[k * dp:k * dp + lin.bias.shape[0]].copy_(lin.bias.detach())
            Wc = torch.zeros(rows_c, dp, dtype=torch.float32, device=dev)
            Wc[:L.C.weight.shape[0], :L.C.weight.shape[1]].copy_(L.C.weight.detach())
            hs, ht = ops.bn_fold(L.bn_node_h, dp)
            es, et = ops.bn_fold(L.bn_node_e, rows_c)
            Lp = P.layers[l]
            Lp.wabde = hold(ops.pack_split(W, b, None, None))
            Lp.wc = hold(ops.pack_split(Wc, ops.pad_vec(L.C.bias, rows_c), es, et))
            Lp.h_scale, Lp.h_shift = hold(hs), hold(ht)
            Lp.residual = 1 if L.residual else 0
        self.params, self.d = P, d
        self.max_edges = int(lib().sn_gatedgcn_max_edges(d))
        self.ok = True

    def run(self, plan, h0, e0):
        """h0 [N, d], e0 [E, d] (e0 is consumed: updated in place) -> scores [B, 1]"""
        y = torch.empty(plan.B, dtype=torch.float32, device=h0.device)
        with ops._span("sn_gatedgcn_fused_f32"):
            check(lib().sn_gatedgcn_fused_f32(C.byref(self.params), ptr(h0), ptr(e0), ptr(plan.graph_ptr), plan.B, ptr(plan.rowptr),
                                              ptr(plan.col), ptr(plan.eperm), ptr(plan.status), ptr(y), stream()), "sn_gatedgcn_fused_f32")
        return y.view(-1, 1)


class GatedGCNNet(_DGLNet):
    """nets/ZINC_graph_regression/gatedgcn_net.py:18-148 for pe_init = 'lap_pe', lap_lspe = False (the sign-invariant PE configs
    GatedGCN_ZINC_LapPE_signinv_GIN[_mask].json): embedding_h / embedding_p with `add` or `concat` + pe_proj (:93-103), edge
    embedding, L GatedGCN layers on sn_gated_aggregate_f32, mean / sum readout, MLPReadout.  Same constructor, forward contract
    `model(g, h, p, e, snorm_n) -> (scores, g)`, state_dict keys and attached `sign_inv_net` as the reference."""

    fused_stages = True      # eval: layers + readout in ONE launch (sn_gatedgcn_fused_f32); False forces the layer path
    _stage_cls, _stage_edges = _FusedGated, None
    _malformed_note = "batch_num_nodes / edges do not describe a batched graph; "
    _limit_text = "more in-edges than the one-launch kernel holds"

    def __init__(self, net_params):
        super().__init__()
        p = net_params
        hidden, out_dim = p["hidden_dim"], p["out_dim"]
        self.pe_aggregate = p["pe_aggregate"]
        self._init_common(p, "GatedGCNNet", [((p["readout"] == "max" and not self._max_readout) or not p["edge_feat"] or not p["batch_norm"],
                                              "readout sum/mean, edge_feat=True, batch_norm=True")], in_feat_dropout="after_e")
        self.layers = nn.ModuleList([GatedGCNLayer(hidden, hidden, self.p_drop, True, residual=self.residual, graph_norm=False,
                                                   feature_dropout=self._feature_dropout)
                                     for _ in range(self.n_layers - 1)] +
                                    [GatedGCNLayer(hidden, out_dim, self.p_drop, True, residual=self.residual, graph_norm=False,
                                                  feature_dropout=self._feature_dropout)])
        self._init_tail(p)

    _fused_gated = _DGLNet._stage        # (the name the topology tests ask by)

    def _forward_behind_side(self, g, h, p, e, fused):
        """The sign-invariant net ran in overlap mode (its event is on the graph): the input encoders (embeddings, PE projection) are
        queued on ITS side stream, right behind it, and only the one-launch GatedGCN stack waits for that stream on the caller's —
        two balanced stages (plan + phi + rho + encoders | 16 layers + read-out) whose consecutive batches overlap."""
        from . import _lib as _lib_mod
        ev, side, tensors = g._sn_side
        N = h.shape[0]
        with torch.no_grad(), torch.cuda.stream(side), _lib_mod.stream_scope():
            plan = cached_plan(g, N)
            hidx, eidx = h.long().reshape(N), e.long().reshape(-1)
            st5 = plan.status[5:6]
            x = self._encode(ops.embedding_sum(hidx, [self.embedding_h.weight], status=st5), p.contiguous().float())
            ee = ops.embedding_sum(eidx, [self.embedding_e.weight], status=st5)
            ev2 = torch.cuda.Event()
            ev2.record(side)
        for t in (h, e):
            t.record_stream(side)
        g._sn_side = (ev2, side, tuple(tensors) + (x, ee))
        _await_side(g, plan)
        self._last_plan = plan
        with torch.no_grad(), _lib_mod.stream_scope():
            return fused.run(plan, x, ee)

    def forward(self, g, h, p, e, snorm_n=None):
        if getattr(g, "_sn_side", None) is not None and p is not None and not self.training and self.pe_init == "lap_pe":
            fz = self._stage(g)
            if fz is not None:
                ops.require_cuda(h)
                y = self._forward_behind_side(g, h, p, e, fz)
                self.g = g
                return y, g
        pe, N, hidx, p, train, grad = self._prologue(g, h, p)
        eidx = e.long().reshape(-1)
        if grad:
            batch, ei, B = self._plan(g, N)
            y = self._forward_grad(ops.build_plan(batch, ei, B, 0), batch, ei, B, hidx, p, eidx)
        else:
            with torch.no_grad():
                plan = cached_plan(g, N)
                y = self._forward_value(plan, hidx, p, eidx, train, self._stage(g))
        self.g = g
        return y, g

    def _forward_value(self, plan, hidx, p, eidx, train, fused=None):
        if fused is not None:
            # no host sync on this path: out-of-range ids are flagged in the plan's status block, the stage kernel then returns NaN
            # scores, check_last() raises
            st5 = plan.status[5:6]
            x = self._encode(ops.embedding_sum(hidx, [self.embedding_h.weight], status=st5), p)
            e = ops.embedding_sum(eidx, [self.embedding_e.weight], status=st5)
            self._last_plan = plan
            return fused.run(plan, x, e)
        snap = self._drop_snap(train, hidx.device)
        x = self._encode(ops.embedding_sum(hidx, [self.embedding_h.weight]), p, snap)
        e = ops.embedding_sum(eidx, [self.embedding_e.weight])
        for li, L in enumerate(self.layers):
            if not train:
                # eval: A, B, D, E as ONE GEMM ([4d, d] weight, column blocks of the result go to the gather kernel by stride),
                # BatchNorm (folded) + ReLU + residual of both h and e fused into the gather pass: 3 launches per layer
                d = L.out_channels
                Y = ops.masked_linear(x, self._abde(L))
                Ce = ops.masked_linear(e, self._pk(L.C))
                sh, se = self._bn(L.bn_node_h, False), self._bn(L.bn_node_e, False)
                x, e = ops.gated_aggregate(Y[:, 0:d], Y[:, d:2 * d], Y[:, 2 * d:3 * d], Y[:, 3 * d:4 * d], Ce, plan,
                                           epilogue=(sh.scale, sh.shift, se.scale, se.shift, x if L.residual else None,
                                                     e if L.residual else None))
                continue
            Ah, Bh, Dh, Eh = (ops.masked_linear(x, self._pk(getattr(L, n))) for n in "ABDE")
            Ce = ops.masked_linear(e, self._pk(L.C))
            h2, e2 = ops.gated_aggregate(Ah, Bh, Dh, Eh, Ce, plan)
            sh, se = self._bn(L.bn_node_h, train), self._bn(L.bn_node_e, train)
            sc, sf = sh.affine(h2, train)
            x = ops.masked_affine(h2, scale=sc, shift=sf, relu=True, residual=x if L.residual else None)
            sc, sf = se.affine(e2, train)
            e = ops.masked_affine(e2, scale=sc, shift=sf, relu=True, residual=e if L.residual else None)
            if L.dropout:           # gatedgcn_layer.py:74-75: h and e behind the residual, sites 1 + 2l and 2 + 2l
                x = ops.dropout(x, L.dropout, snap, 1 + 2 * li)
                e = ops.dropout(e, L.dropout, snap, 2 + 2 * li)
        return self._readout(x, plan)

    def _forward_grad(self, plan, batch, ei, B, hidx, p, eidx):
        vN, vE, vB, k1 = _bucket_rows(self)         # (train_graph.DGLBucketedStep: padding rows enter no statistic and no gradient)
        rplan = ops.build_plan(batch, ei.flip(0).contiguous(), B, 0)
        snap = self._drop_snap(True, hidx.device)
        x = self._encode_grad(hidx, p, vN, k1, snap)
        e = AG.embedding_sum(eidx, [self.embedding_e.weight])
        for li, L in enumerate(self.layers):
            Ah, Bh, Dh, Eh = (AG.linear(x, getattr(L, n).weight, getattr(L, n).bias, vN, k1) for n in "ABDE")
            Ce = AG.linear(e, L.C.weight, L.C.bias, vE, k1)
            h2, e2 = AG.gated_aggregate(Ah, Bh, Dh, Eh, Ce, plan, rplan)
            x = AG.bn_act(h2, L.bn_node_h, vN, k1, relu=True, residual=x if L.residual else None)
            e = AG.bn_act(e2, L.bn_node_e, vE, k1, relu=True, residual=e if L.residual else None)
            if L.dropout:
                x = AG.dropout(x, L.dropout, snap, 1 + 2 * li)
                e = AG.dropout(e, L.dropout, snap, 2 + 2 * li)
        return self._readout_grad(x, plan, vB, k1)


# ---------------------------------------------------------------------------------------------------------------
# PNA: layers/pna_layer.py:16-160, layers/pna_utils.py, nets/ZINC_graph_regression/pna_net.py:19-170
class FCLayer(nn.Module):
    """layers/pna_utils.py:170-243 (parameters only): `linear` (+ the activation name; no dropout, no b_norm in the shipped nets)."""

    def __init__(self, in_size, out_size, activation="relu"):
        super().__init__()
        self.in_size, self.out_size, self.activation = in_size, out_size, activation
        self.linear = nn.Linear(in_size, out_size, bias=True)
        nn.init.xavier_uniform_(self.linear.weight, 1 / in_size)       # FCLayer.reset_parameters (:223-228)
        self.linear.bias.data.zero_()


class _PnaMLP(nn.Module):
    """layers/pna_utils.py:246-279 with layers = 1 (pretrans_layers = posttrans_layers = 1 in every shipped PNA config)."""

    def __init__(self, in_size, hidden_size, out_size, layers, mid_activation="relu", last_activation="none"):
        super().__init__()
        if layers != 1:
            raise NotImplementedError("HIP PNA: pretrans_layers = posttrans_layers = 1 (the shipped configs)")
        self.fully_connected = nn.ModuleList([FCLayer(in_size, out_size, activation=last_activation)])


class PNATower(nn.Module):
    def __init__(self, in_dim, out_dim, edge_dim, dropout=0.0):
        super().__init__()
        self.dropout = ops.check_dropout_p(dropout, "HIP PNATower")          # pna_layer.py:79, behind the BatchNorm
        self.batchnorm_h = nn.BatchNorm1d(out_dim)
        self.pretrans_h = _PnaMLP(2 * in_dim + edge_dim, in_dim, in_dim, 1)
        self.posttrans_h = _PnaMLP(13 * in_dim, out_dim, out_dim, 1)          # (4 aggregators x 3 scalers + 1) * in_dim


class PNALayer(nn.Module):
    def __init__(self, in_dim, out_dim, towers, edge_dim, residual, dropout=0.0):
        super().__init__()
        if in_dim % towers or out_dim % towers:
            raise ValueError("the number of towers has to divide in_dim and out_dim")
        self.in_dim, self.out_dim, self.n_towers = in_dim, out_dim, towers
        self.residual = residual and in_dim == out_dim
        self.towers = nn.ModuleList([PNATower(in_dim // towers, out_dim // towers, edge_dim, dropout) for _ in range(towers)])
        self.mixing_network_h = FCLayer(out_dim, out_dim, activation="LeakyReLU")


class PNANet(_DGLNet):
    """nets/ZINC_graph_regression/pna_net.py:19-170 for the configuration PNA_ZINC_LapPE_signinv_GIN[_mask].json selects: pe_init
    'lap_pe', lap_lspe False, aggregators 'mean max min std', scalers 'identity amplification attenuation', towers with divided
    input, edge features, graph_norm + batch_norm, residual, no GRU, sum / mean readout.  Same constructor (`net_params`), forward
    contract `model(g, h, p, e, snorm_n) -> (scores, g)`, state_dict keys and attached `sign_inv_net`.  Per layer and tower:
    gather cat[h_src, h_dst, e] -> pretrans Linear -> sn_pna_aggregate_f32 -> posttrans Linear -> sn_pointwise_f32 (snorm_n and
    BatchNorm); then the mixing Linear + LeakyReLU + residual.  In eval mode the towers of a layer run side by side and the pretrans
    gather is folded into the aggregation, on activations padded to 16-byte rows (sn_pna_aggregate_gather_f32,
    `_forward_eval_padded`).  Eval, train-mode value (batch-statistic BatchNorm, running statistics updated) and — with gradients
    enabled — the differentiable path (`_forward_grad`)."""

    fused_layers = True      # eval, padded layout: one edge-term Linear for all layers, LeakyReLU + residual as the mixing Linear's epilogue

    def __init__(self, net_params):
        super().__init__()
        p = net_params
        hidden, out_dim, edge_dim = p["hidden_dim"], p["out_dim"], p["edge_dim"]
        self.graph_norm = p["graph_norm"]
        self.aggregators, self.scalers, self.avg_d, self.towers = p["aggregators"], p["scalers"], p["avg_d"], p["towers"]
        self._init_common(p, "PNANet", [
            (self.aggregators.split() != ["mean", "max", "min", "std"] or self.scalers.split() != ["identity", "amplification", "attenuation"],
             "aggregators 'mean max min std', scalers 'identity amplification attenuation'"),
            (not (self.graph_norm and p["batch_norm"] and p["edge_feat"]) or p["gru"] or (p["readout"] == "max" and not self._max_readout),
             "graph_norm, batch_norm, edge_feat True; gru False; readout sum / mean"),
            (not (p["divide_input_first"] and p["divide_input_last"]), "divide_input_first / _last True (the shipped configs)")],
            edge_dim=edge_dim, in_feat_dropout="before_h")
        self.layers = nn.ModuleList([PNALayer(hidden, hidden, self.towers, edge_dim, self.residual, self.p_drop) for _ in range(self.n_layers - 1)] +
                                    [PNALayer(hidden, out_dim, self.towers, edge_dim, self.residual, self.p_drop)])
        if p["pretrans_layers"] != 1 or p["posttrans_layers"] != 1:
            raise NotImplementedError("HIP PNANet: pretrans_layers = posttrans_layers = 1")
        self._init_tail(p)

    def forward(self, g, h, p, e, snorm_n):
        if snorm_n is None or (p is None and self.pe_init == "lap_pe"):
            raise NotImplementedError("HIP PNANet needs snorm_n (graph_norm) and, with pe_init='lap_pe', the positional encoding p")
        pe, N, hidx, p, train, grad = self._prologue(g, h, p)
        avg_log = float(self.avg_d["log"])
        sn = snorm_n.reshape(N).contiguous().float()
        eidx = e.long().reshape(-1)
        if grad:
            batch, ei, B = self._plan(g, N)
            hg = self._forward_grad(ops.build_plan(batch, ei, B, 0), batch, ei, B, hidx, p, eidx, sn, avg_log)
            self.g = g
            return hg, g
        plan = cached_plan(g, N)           # shared with the sign-invariant net: ONE sn_batch_plan per batch
        with torch.no_grad():
            if not train and self._pna_padded()["ok"]:
                hg = self._forward_eval_padded(plan, hidx, p, eidx, sn, avg_log)
                self.g = g
                return hg, g
            src, dst = (t.long() for t in g.edges())
            snap = self._drop_snap(train, h.device)
            x = self._encode(ops.embedding_sum(hidx, [self.embedding_h.weight]), p, snap)                        # h + embedding_p(p)  (:124-126)
            ef = ops.embedding_sum(eidx, [self.embedding_e.weight])
            for li, L in enumerate(self.layers):
                it = L.in_dim // L.n_towers
                outs = []
                for t, T in enumerate(L.towers):
                    ht = x[:, t * it:(t + 1) * it].contiguous()                                                       # copies / concats: plumbing
                    z = torch.cat([ht.index_select(0, src), ht.index_select(0, dst), ef], dim=1)                      # pretrans_edges (:38-44)
                    m = ops.masked_linear(z, self._pk(T.pretrans_h.fully_connected[0].linear))
                    a = ops.pna_aggregate(m, ht, plan, avg_log)                                                       # (:50-56, :69)
                    y = ops.masked_linear(a, self._pk(T.posttrans_h.fully_connected[0].linear))
                    site = self._bn(T.batchnorm_h, train)
                    if not train:
                        y = ops.pointwise(y, rowscale=sn, scale=site.scale, shift=site.shift)                          # * snorm_n, BatchNorm (:75-79)
                    else:
                        y = ops.pointwise(y, rowscale=sn)
                        sc, sh = site.affine(y, True)
                        y = ops.pointwise(y, scale=sc, shift=sh)
                        if T.dropout:          # site 1 + (layer, tower) in forward order
                            y = ops.dropout(y, T.dropout, snap, 1 + li * L.n_towers + t)
                    outs.append(y)
                hc = torch.cat(outs, dim=1)
                mix = ops.masked_linear(hc, self._pk(L.mixing_network_h.linear))
                x = ops.pointwise(mix, act="leaky", slope=0.01, residual=x if L.residual else None)                  # FCLayer LeakyReLU + residual
            hg = self._readout(x, plan)
        self.g = g
        self._h_last = x
        return hg, g

    @staticmethod
    def _pad_map(Cc, nt, dev):
        """Tower t's channels [t*it, (t+1)*it) -> [t*it_p, t*it_p + it), it_p = it rounded up to a multiple of 4: every row of the padded
        activations is 16-byte aligned and every Linear takes the vector / LDS-staged kernels (hidden 70 = 5 towers x 14 would fall back to
        the scalar kernel: 73 % of the forward).  Pad channels are zero everywhere (zero weight rows / columns, BatchNorm scale 0)."""
        it = Cc // nt
        it_p = (it + 3) // 4 * 4
        c = torch.arange(Cc, device=dev)
        return (c // it) * it_p + c % it, nt * it_p, it, it_p

    def _pna_padded(self):
        """Eval cache: every parameter of the net re-laid-out for the padded, all-towers-side-by-side evaluation.  Per layer:
        sd [2 Cin_p, Cin_p] — rows t*it_p.. of the first / second half hold tower t's pretrans weights for h_src / h_dst (block diagonal:
        a tower reads its own input channels; pna_layer.py:38-44 is a Linear over cat[h_src, h_dst, e] = W_s h_src + W_d h_dst + W_e e + b);
        e [Cin_p, edge_dim] + the pretrans biases; post_w [towers, ot_p, 13 it_p] — the towers' posttrans Linears as one grouped (block-diagonal) Linear over
        the tower-major output of the aggregation kernel; the towers' folded BatchNorms side by side (its epilogue, with snorm_n); the mixing Linear in the padded channel order."""
        return self._cached("pna_padded", self._pad_pna)

    def _pad_pna(self):
        dev = self.embedding_h.weight.device
        mk = lambda W_, b_: ops.PackedLinear(ops.pack_weight(W_.contiguous()), W_.shape[0], W_.shape[1], None if b_ is None else b_.contiguous())
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        nt = self.layers[0].n_towers
        hid = self.embedding_h.weight.shape[1]
        pos0, C0, _, _ = self._pad_map(hid, nt, dev)
        P = {"pos_in": pos0, "C_in": C0}
        E = z(self.embedding_h.weight.shape[0], C0)
        E[:, pos0] = self.embedding_h.weight.detach().float()
        P["emb_h"] = E
        if self.pe_init == "lap_pe":
            Wp_, bp_ = z(C0, self.embedding_p.weight.shape[1]), z(C0)
            Wp_[pos0], bp_[pos0] = self.embedding_p.weight.detach().float(), self.embedding_p.bias.detach().float()
            P["emb_p"] = mk(Wp_, bp_)
        layers = []
        for L in self.layers:
            Cin, Cout = L.in_dim, L.out_dim
            pin, Cin_p, it, it_p = self._pad_map(Cin, nt, dev)
            pout, Cout_p, ot, ot_p = self._pad_map(Cout, nt, dev)
            pre = [T.pretrans_h.fully_connected[0].linear for T in L.towers]
            post = [T.posttrans_h.fully_connected[0].linear for T in L.towers]
            ed = pre[0].weight.shape[1] - 2 * it
            Wsd, We, be = z(2 * Cin_p, Cin_p), z(Cin_p, ed), z(Cin_p)
            Wpo, bpo = z(nt, ot_p, 13 * it_p), z(Cout_p)            # grouped: tower t reads its own 13 it_p tower-major columns
            sc, sh = z(Cout_p), z(Cout_p)
            for t in range(nt):
                W = pre[t].weight.detach().float()
                r = slice(t * it_p, t * it_p + it)
                Wsd[r, r] = W[:, :it]
                Wsd[Cin_p + t * it_p:Cin_p + t * it_p + it, r] = W[:, it:2 * it]
                We[r] = W[:, 2 * it:]
                be[r] = pre[t].bias.detach().float()
                Q = post[t].weight.detach().float()                   # [ot, 13 it]: cat[h_t, (4 s + a) blocks of it]
                ro = slice(t * ot_p, t * ot_p + ot)
                for j in range(13):
                    Wpo[t, :ot, j * it_p:j * it_p + it] = Q[:, j * it:(j + 1) * it]
                bpo[ro] = post[t].bias.detach().float()
                site = self._bn(L.towers[t].batchnorm_h, False)
                sc[ro], sh[ro] = site.scale, site.shift
            ml = L.mixing_network_h.linear
            Wm, bm = z(Cout_p, Cout_p), z(Cout_p)
            Wm[pout[:, None], pout[None, :]] = ml.weight.detach().float()
            bm[pout] = ml.bias.detach().float()
            layers.append({"sd": mk(Wsd, None), "e": mk(We, be), "e_raw": (We, be), "post_w": Wpo.contiguous(), "post_b": bpo, "nt": nt, "it_p": it_p,
                           "grouped": ot_p <= 16 and 13 * it_p <= 256, "scale": sc, "shift": sh, "mix": mk(Wm, bm),
                           "residual": L.residual, "pos_out": pout, "C_out": Cout_p})
        P["layers"] = layers
        P["ok"] = all(F["grouped"] for F in layers)       # (wider towers: the per-tower layer path below serves the net)
        # the edge features do not change from layer to layer (pna_layer.py updates h only): every layer's edge term W_e e + b as ONE
        # [E, L*C] Linear in front of the layer loop, read in place by the aggregation (column block l, row stride L*C)
        P["e_all"] = None
        if len({tuple(F["e_raw"][0].shape) for F in layers}) == 1:
            P["e_all"] = mk(torch.cat([F["e_raw"][0] for F in layers], 0), torch.cat([F["e_raw"][1] for F in layers], 0))
        fc0 = self.MLP_layer.FC_layers[0]
        W0 = z(fc0.weight.shape[0], layers[-1]["C_out"])
        W0[:, layers[-1]["pos_out"]] = fc0.weight.detach().float()
        P["fc0"] = mk(W0, fc0.bias.detach().float())
        return P

    def _forward_eval_padded(self, plan, hidx, p, eidx, sn, avg_log):
        """Eval forward on the padded layout (`_pna_padded`): all towers of a layer side by side, the pretrans gather folded into the
        aggregation (sn_pna_aggregate_gather_f32): 7 launches per layer instead of 9 per tower, every Linear on the vector kernels."""
        P = self._pna_padded()
        x = ops.embedding_sum(hidx, [P["emb_h"]])
        if "emb_p" in P:
            x = ops.masked_linear(p, P["emb_p"], residual=x)                                                     # h + embedding_p(p)  (:124-126)
        ef = ops.embedding_sum(eidx, [self.embedding_e.weight])
        fuse = self.fused_layers
        qe_all = ops.masked_linear(ef, P["e_all"]) if (fuse and P["e_all"] is not None) else None                # [E, L*C]
        for li, F in enumerate(P["layers"]):
            psd = ops.masked_linear(x, F["sd"])                                                                  # [N, 2C] = [W_s h | W_d h]
            if qe_all is not None:
                a = ops.pna_aggregate_gather(psd, qe_all, x, plan, avg_log, tower_width=F["it_p"], qe_layer=li)
            else:
                qe = ops.masked_linear(ef, F["e"])                                                               # [E, C]  = W_e e + b
                a = ops.pna_aggregate_gather(psd, qe, x, plan, avg_log, tower_width=F["it_p"])                   # (:50-56, :69), tower-major
            hc = ops.grouped_linear(a, F["post_w"], F["post_b"], F["nt"], rowscale=sn, scale=F["scale"], shift=F["shift"])   # posttrans,
            #                                                                                            * snorm_n, BatchNorm (:69-79)
            if fuse:      # FCLayer's LeakyReLU and the residual as the mixing Linear's epilogue
                x = ops.masked_linear(hc, F["mix"], leaky=True, residual=x if F["residual"] else None)
            else:
                mix = ops.masked_linear(hc, F["mix"])
                x = ops.pointwise(mix, act="leaky", slope=0.01, residual=x if F["residual"] else None)           # FCLayer LeakyReLU + residual
        self._h_last = x.index_select(1, P["layers"][-1]["pos_out"])
        return self._readout(x, plan, first=P["fc0"])

    def _forward_grad(self, plan, batch, ei, B, hidx, p, eidx, sn, avg_log):
        """Differentiable train-mode forward (SURVEY.md §8 f1 for this net): the same ops as autograd nodes with hand-written adjoints
        (csrc/dgl_layers.hip: CSR walks, no atomics); towers' column slices and concatenations are torch views / copies."""
        vN, vE, vB, k1 = _bucket_rows(self)         # (train_graph.DGLBucketedStep: padding rows enter no statistic and no gradient)
        rplan = ops.build_plan(batch, ei.flip(0).contiguous(), B, 0)           # edges grouped by SOURCE: adjoint of h[src]
        src, dst = ei[0], ei[1]
        snap = self._drop_snap(True, hidx.device)
        x = self._encode_grad(hidx, p, vN, k1, snap)
        ef = AG.embedding_sum(eidx, [self.embedding_e.weight])
        for li, L in enumerate(self.layers):
            it = L.in_dim // L.n_towers
            outs = []
            for t, T in enumerate(L.towers):
                ht = x[:, t * it:(t + 1) * it].contiguous()
                z = torch.cat([AG.gather_rows(ht, src, rplan), AG.gather_rows(ht, dst, plan), ef], dim=1)
                pre, post = T.pretrans_h.fully_connected[0].linear, T.posttrans_h.fully_connected[0].linear
                m = AG.linear(z, pre.weight, pre.bias, vE, k1)
                a = AG.pna_aggregate(m, ht, plan, avg_log)
                y = AG.act_residual(AG.linear(a, post.weight, post.bias, vN, k1), rowscale=sn)     # graph_norm: h * snorm_n
                y = AG.bn_act(y, T.batchnorm_h, vN, k1, relu=False)
                outs.append(AG.dropout(y, T.dropout, snap, 1 + li * L.n_towers + t) if T.dropout else y)
            mixl = L.mixing_network_h.linear
            mix = AG.linear(torch.cat(outs, dim=1), mixl.weight, mixl.bias, vN, k1)
            x = AG.act_residual(mix, residual=x if L.residual else None, act="leaky", slope=0.01)
        self._h_last = x.detach()
        return self._readout_grad(x, plan, vB, k1)


# ---------------------------------------------------------------------------------------------------------------
# Sparse graph Transformer: layers/transformer.py:112-317, nets/ZINC_graph_regression/transformer_net.py:21-150
class MultiHeadAttentionLayer(nn.Module):
    def __init__(self, gamma, in_dim, out_dim, num_heads, full_graph=False):
        super().__init__()
        self.out_dim, self.num_heads, self.gamma = out_dim, num_heads, gamma        # gamma: the owner's Parameter, registered here too
        self.full_graph = full_graph
        self.Q = nn.Linear(in_dim, out_dim * num_heads, bias=False)
        self.K = nn.Linear(in_dim, out_dim * num_heads, bias=False)
        self.E = nn.Linear(in_dim, out_dim * num_heads, bias=False)
        if full_graph:                                                              # (transformer.py:147-150: the fake pairs' own projections)
            self.Q_2 = nn.Linear(in_dim, out_dim * num_heads, bias=False)
            self.K_2 = nn.Linear(in_dim, out_dim * num_heads, bias=False)
            self.E_2 = nn.Linear(in_dim, out_dim * num_heads, bias=False)
        self.V = nn.Linear(in_dim, out_dim * num_heads, bias=False)


class BatchedTransformerLayer(nn.Module):
    """layers/transformer.py:234-317 with the arguments transformer_net.py:69-70 passes (the rest at their defaults: residual,
    batch_norm, no layer_norm, use_bias False).  `dropout` (:281, :299: behind the attention output and behind the FFN's ReLU) is the
    layer's own attribute, as in the reference — whose TransformerNet never hands its net_params['dropout'] to a layer, so a net built
    from a config keeps 0 here."""

    def __init__(self, in_dim, out_dim, num_heads, full_graph, dropout=0.0, use_edge=True):
        super().__init__()
        self.dropout = ops.check_dropout_p(dropout, "HIP BatchedTransformerLayer")
        if not use_edge:
            raise NotImplementedError("HIP graph Transformer: full_graph False with edge features (the shipped sign_inv configs)")
        if out_dim % num_heads or out_dim // num_heads > 32:
            raise ValueError("num_heads must divide out_dim and the head width must be <= 32")
        self.in_channels, self.out_channels, self.num_heads = in_dim, out_dim, num_heads
        self.full_graph = bool(full_graph)
        self.gamma = nn.Parameter(torch.FloatTensor([0.1]))          # unused when full_graph is False, but part of the state_dict
        self.attention_h = MultiHeadAttentionLayer(self.gamma, in_dim, out_dim // num_heads, num_heads, self.full_graph)
        self.O_h = nn.Linear(out_dim, out_dim)
        self.batch_norm1_h = nn.BatchNorm1d(out_dim)
        self.FFN_h_layer1 = nn.Linear(out_dim, out_dim * 2)
        self.FFN_h_layer2 = nn.Linear(out_dim * 2, out_dim)
        self.batch_norm2_h = nn.BatchNorm1d(out_dim)


class _FusedTransformer:
    """Packed eval-mode parameters of a TransformerNet for sn_transformer_net_fused_f32: embeddings, every layer (projections, edge
    attention, O_h, both BatchNorms, the FFN), readout and MLPReadout in ONE launch — a workgroup per graph on the stage kernel of
    csrc/fused_gnn.hip (Transformer mode).  The layers' E projections of the edge embedding stay one Linear in front of it.  `ok`
    False: anything but the shipped shape (hidden = out = 64, 8 heads, BatchNorm, residual, 3-Linear readout; pe_aggregate 'add' or 'concat')."""

    def __init__(self, net):
        from .fused import _GnnParams, GNN_MAX_LAYERS
        self.ok = False
        Ls, fcs = list(net.layers), list(net.MLP_layer.FC_layers)
        nope = net.pe_init != "lap_pe"       # NoPE: a zero projection of a one-column zero encoding (h = embedding_h(h) + 0)
        d, kp = net.embedding_h.weight.shape[1], 1 if nope else net.embedding_p.weight.shape[1]
        if not (d == 64 and net.batch_norm and net.residual and kp <= 64):        # (the net's layer_norm flag is not handed to the layers)
            return
        if len(Ls) > GNN_MAX_LAYERS or len(fcs) != 3 or fcs[2].weight.shape[0] != 1:
            return
        if any(L.in_channels != 64 or L.out_channels != 64 or L.num_heads != 8 for L in Ls):
            return
        dev = net.embedding_h.weight.device
        keep = self._keep = []

        def hold(t):
            keep.append(t)
            return t.data_ptr()

        ones = torch.ones(64, dtype=torch.float32, device=dev)
        w = lambda t: t.detach().float().contiguous()
        P = _GnnParams()
        P.d, P.n_layers, P.n_out = 64, len(Ls), 1
        P.node_discrete, P.node_nf, P.edge_discrete, P.edge_nf = 1, 1, 0, 0
        P.node_vocab, P.edge_vocab = net.embedding_h.weight.shape[0], 0
        P.ntab[0] = hold(w(net.embedding_h.weight))
        P.rho_out_w = None
        if nope:
            P.lin_a = hold(ops.pack_split(torch.eye(64, dtype=torch.float32, device=dev)))
            P.lin_b = hold(ops.pack_split(torch.zeros(64, 64, dtype=torch.float32, device=dev), torch.zeros(64, dtype=torch.float32, device=dev)))
        elif net.pe_aggregate == "concat":
            # h = pe_proj(cat[embedding_h, embedding_p(p)]) (transformer_net.py:96-99) = W[:, :d] emb_h + (W[:, d:] W_p) p + (W[:, d:] b_p + b):
            # the two affine maps behind p folded once, in float64 (as the GINE net folds rho.out into its input Linear)
            Wc, bc = net.pe_proj.weight.detach().double(), net.pe_proj.bias.detach().double()
            Wp_, bp_ = net.embedding_p.weight.detach().double(), net.embedding_p.bias.detach().double()
            P.lin_a = hold(ops.pack_split(Wc[:, :64].float().contiguous()))
            P.lin_b = hold(ops.pack_split(_pad_mat((Wc[:, 64:] @ Wp_).float(), 64), (Wc[:, 64:] @ bp_ + bc).float().contiguous()))
        else:
            P.lin_a = hold(ops.pack_split(torch.eye(64, dtype=torch.float32, device=dev)))
            P.lin_b = hold(ops.pack_split(_pad_mat(net.embedding_p.weight, 64), ops.pad_vec(net.embedding_p.bias, 64)))
        for l, L in enumerate(Ls):
            A = L.attention_h
            s1, s2 = net._bn(L.batch_norm1_h, False), net._bn(L.batch_norm2_h, False)
            W1, b1, W2 = w(L.FFN_h_layer1.weight), w(L.FFN_h_layer1.bias), w(L.FFN_h_layer2.weight)
            mats = [ops.pack_split(w(A.Q.weight)), ops.pack_split(w(A.K.weight)), ops.pack_split(w(A.V.weight)),
                    ops.pack_split(w(L.O_h.weight), w(L.O_h.bias), s1.scale, s1.shift),
                    ops.pack_split(W1[:64].contiguous(), b1[:64].contiguous()), ops.pack_split(W1[64:].contiguous(), b1[64:].contiguous()),
                    ops.pack_split(W2[:, :64].contiguous()),
                    ops.pack_split(W2[:, 64:].contiguous(), w(L.FFN_h_layer2.bias), s2.scale, s2.shift)]
            Lp = P.layers[l]
            for j, m in enumerate(mats):
                Lp.etab[j] = hold(m)
            Lp.w1s, Lp.w2s = Lp.etab[0], Lp.etab[1]
        P.head_w1 = hold(ops.pack_split(_pad_mat(fcs[0].weight, 64), ones, ops.pad_vec(fcs[0].bias, 64)))
        self.head_mid = hold(ops.pack_split(_pad_mat(fcs[1].weight, 64), ones, ops.pad_vec(fcs[1].bias, 64)))
        P.head_w2 = hold(ops.pack_split(_pad_mat(fcs[2].weight, 64), ops.pad_vec(fcs[2].bias, 64)))
        self.params, self.kp, self.pool_mean = P, kp, _READOUT_MODE.get(net.readout, 1)
        self.ok = True

    def run(self, plan, hidx, p, e_proj):
        """atom types [N] int64, positional encoding [N, k], the layers' E projections [E, L*64] -> scores [B, 1]"""
        y = torch.empty(plan.B, 1, dtype=torch.float32, device=p.device)
        with ops._span("sn_transformer_net_fused_f32"):
            check(lib().sn_transformer_net_fused_f32(C.byref(self.params), self.head_mid, self.pool_mean, ptr(hidx), ptr(p), p.shape[1], self.kp,
                                                     ptr(e_proj), e_proj.shape[1], ptr(plan.graph_ptr), plan.B, ptr(plan.rowptr), ptr(plan.col),
                                                     ptr(plan.eperm), ptr(plan.status), ptr(y), ptr(plan.status), 8, stream()),
                  "sn_transformer_net_fused_f32")
        return y


class TransformerNet(_DGLNet):
    """nets/ZINC_graph_regression/transformer_net.py:21-150 for pe_init 'lap_pe', lap_lspe False, edge_feat True, full_graph False
    (Transformer_ZINC_LapPE_signinv_GIN[_masked].json): embedding_h / embedding_p with `add` or `concat` + pe_proj, edge
    embedding, L x [Q/K/V/E projections -> sn_edge_attention_f32 -> O_h + residual -> BatchNorm -> FFN + residual -> BatchNorm],
    sum / mean readout, MLPReadout.  Same constructor, forward contract, state_dict keys and attached `sign_inv_net`.
    Eval, train-mode value and — with gradients enabled — the differentiable path (`_forward_grad`).
    full_graph True (`--full_graph`): `g` is the complete graph of every molecule with g.edata['real'] (ops.make_full_graph); bonds go
    through Q / K / E, all other pairs through Q_2 / K_2 / E_2, mixed by each layer's gamma — `_forward_full`, one sn_full_attention_f32
    launch per layer on the layer path (no one-launch stage kernel).
    `full_graph_input` (a property of a full_graph=True net, default "edges"): "bonds" — `g` is the MOLECULAR graph and `e` its bond
    classes [E], as the sparse net takes them; the attention works the complete graph out from each molecule's node range
    (sn_bond_full_attention_f32: no sn_make_full_graph, nothing with a row per pair).  Such a batch is an ordinary DGL batch, which
    train_graph.DGLBucketedStep, serving.GraphedDGLForward and data.DGLGraphStore carry.  Never a state_dict key."""

    fused_layers = True     # eval: fused projections / epilogues (False: one launch per op, as the train-mode value path)
    fused_stages = True      # eval, the shipped shape: everything behind the E projection in ONE launch (sn_transformer_net_fused_f32)
    _stage_cls = _FusedTransformer

    def __init__(self, net_params):
        super().__init__()
        p = net_params
        hidden, out_dim = p["hidden_dim"], p["out_dim"]
        self.layer_norm, self.pe_aggregate = p["layer_norm"], p["pe_aggregate"]
        self._init_common(p, "TransformerNet", [((p["readout"] == "max" and not self._max_readout) or not p["edge_feat"], "readout sum / mean, edge_feat True")],
                          in_feat_dropout="after_e")
        self.layers = nn.ModuleList([BatchedTransformerLayer(hidden, hidden, p["n_heads"], p["full_graph"], use_edge=True)
                                     for _ in range(self.n_layers - 1)] +
                                    [BatchedTransformerLayer(hidden, out_dim, p["n_heads"], p["full_graph"], use_edge=True)])
        self.full_graph = bool(p["full_graph"])
        self._init_tail(p)

    FULL_GRAPH_INPUTS = ("edges", "bonds")

    @property
    def full_graph_input(self):
        """"edges" | "bonds": what a full_graph=True net's forward takes (class docstring)."""
        return self.__dict__.get("_full_graph_input", "edges")

    @full_graph_input.setter
    def full_graph_input(self, form):
        if form not in self.FULL_GRAPH_INPUTS:
            raise ValueError(f"TransformerNet.full_graph_input: {form!r} (one of {', '.join(self.FULL_GRAPH_INPUTS)})")
        if not self.full_graph:
            raise ValueError("TransformerNet.full_graph_input belongs to a full_graph=True net: the sparse net attends over the bonds only")
        self.__dict__["_full_graph_input"] = form

    def _stage(self, g):
        if self.full_graph:                  # full-graph nets take the layer path: the one-launch stage kernel has no fake-pair form
            return None
        return super()._stage(g) if self._fusable() else None          # (the kernel reads the stacked E projections of `_fused_eval`)

    def _fusable(self):
        """Every layer maps hidden -> hidden (the shipped configs: out_dim == hidden_dim), so that the layers' E projections stack."""
        d = self.layers[0].out_channels
        return self.fused_layers and all(L.in_channels == d and L.out_channels == d for L in self.layers)

    def _fused_eval(self):
        """Eval cache: cat[W_Q; W_K; W_V] per layer and cat over the layers of W_E, packed (no biases: use_bias False)."""
        def pack(ws):
            W = torch.cat([w.detach().float() for w in ws], 0).contiguous()
            return ops.PackedLinear(ops.pack_weight(W), W.shape[0], W.shape[1], None)
        return self._cached("fused", lambda: {
            "qkv": [pack([L.attention_h.Q.weight, L.attention_h.K.weight, L.attention_h.V.weight]) for L in self.layers],
            "E": pack([L.attention_h.E.weight for L in self.layers])})

    def _bn_res(self, y, res, bn, train):
        """BatchNorm1d(res + y): eval folded into one pointwise pass; train: batch statistics of the sum."""
        site = self._bn(bn, train)
        if not train:
            s = ops.pointwise(y, residual=res)
            return ops.pointwise(s, scale=site.scale, shift=site.shift)
        s = ops.pointwise(y, residual=res)
        sc, sh = site.affine(s, True)
        return ops.pointwise(s, scale=sc, shift=sh)

    def forward(self, g, h, p, e, snorm_n=None):
        if self.full_graph:
            return self._forward_bonds(g, h, p, e) if self.full_graph_input == "bonds" else self._forward_full(g, h, p, e)
        pe, N, hidx, p, train, grad = self._prologue(g, h, p)
        eidx = e.long().reshape(-1)
        if grad:
            batch, ei, B = self._plan(g, N)
            hg = self._forward_grad(ops.build_plan(batch, ei, B, 0), batch, ei, B, hidx, p, eidx)
            self.g = g
            return hg, g
        plan = cached_plan(g, N)           # shared with the sign-invariant net: ONE sn_batch_plan per batch
        with torch.no_grad():
            fzs = self._stage(g)
            if fzs is not None:
                # no host sync on this path: a bad atom type / an oversize graph -> NaN score + check_last(); a bond type outside its table
                # is flagged in the plan's status block by the embedding (status[5]) and raised by check_last() as well
                ef = ops.embedding_sum(eidx, [self.embedding_e.weight], status=plan.status[5:6])
                Ee_all = ops.masked_linear(ef, self._fused_eval()["E"])
                self._last_plan = plan
                self.g = g
                return fzs.run(plan, hidx.contiguous(), p if pe else _zero_pe(self, N, h.device)[:N], Ee_all), g
            snap = self._drop_snap(train, h.device)
            # (transformer.py:281, 299: sites 1 + 2l — attention output — and 2 + 2l — FFN hidden — of each layer's own `dropout`)
            x = self._encode(ops.embedding_sum(hidx, [self.embedding_h.weight]), p, snap)                             # (:96-102)
            ef = ops.embedding_sum(eidx, [self.embedding_e.weight])
            if not train and self._fusable():
                # eval (round 4): 5 launches per layer instead of 12.  Q | K | V are ONE [3d, d] Linear whose column blocks the attention
                # reads in place; every layer's E projection of the (layer-independent) edge embedding is one [L*d, d] Linear up front;
                # `BatchNorm(x + Linear(h))` is the Linear's epilogue (residual in front of the folded affine: the same operations in the
                # same order as the add + affine passes they replace — bit-identical).
                fz = self._fused_eval()
                Ee_all = ops.masked_linear(ef, fz["E"])
                for li, L in enumerate(self.layers):
                    qkv = ops.masked_linear(x, fz["qkv"][li])
                    a = ops.edge_attention_fused(qkv, Ee_all, li, plan, L.num_heads)                                  # (:150-228)
                    s1, s2 = self._bn(L.batch_norm1_h, False), self._bn(L.batch_norm2_h, False)
                    x1 = ops.masked_linear(a, self._pk(L.O_h), residual=x, residual_pre=True, scale=s1.scale, shift=s1.shift)       # (:283-290)
                    f = ops.masked_linear(x1, self._pk(L.FFN_h_layer1), relu=True)
                    x = ops.masked_linear(f, self._pk(L.FFN_h_layer2), residual=x1, residual_pre=True, scale=s2.scale, shift=s2.shift)  # (:300-308)
            else:
                for li, L in enumerate(self.layers):
                    A = L.attention_h
                    Q, K, V = (ops.masked_linear(x, self._pk(getattr(A, n))) for n in "QKV")
                    Ee = ops.masked_linear(ef, self._pk(A.E))
                    a = ops.edge_attention(Q, K, V, Ee, plan, L.num_heads)                                            # (:150-228)
                    pd = L.dropout if train else 0.0
                    if pd:
                        a = ops.dropout(a, pd, snap, 1 + 2 * li)
                    o = ops.masked_linear(a, self._pk(L.O_h))
                    x1 = self._bn_res(o, x, L.batch_norm1_h, train)                                                   # residual, BatchNorm (:283-290)
                    f = ops.masked_linear(x1, self._pk(L.FFN_h_layer1), relu=True)
                    if pd:
                        f = ops.dropout(f, pd, snap, 2 + 2 * li)
                    f = ops.masked_linear(f, self._pk(L.FFN_h_layer2))
                    x = self._bn_res(f, x1, L.batch_norm2_h, train)                                                   # (:300-308)
            hg = self._readout(x, plan)
        self.g = g
        self._h_last = x
        return hg, g

    def _forward_grad(self, plan, batch, ei, B, hidx, p, eidx):
        """Differentiable train-mode forward: the sparse attention's adjoint is sn_edge_attention_bwd_f32 (destination pass + source
        pass over the reverse CSR, no atomics); BatchNorm with batch statistics, residuals, FFN as in the value path."""
        vN, vE, vB, k1 = _bucket_rows(self)         # (train_graph.DGLBucketedStep: padding rows enter no statistic and no gradient)
        rplan = ops.build_plan(batch, ei.flip(0).contiguous(), B, 0)
        snap = self._drop_snap(True, hidx.device)
        x = self._encode_grad(hidx, p, vN, k1, snap)
        ef = AG.embedding_sum(eidx, [self.embedding_e.weight])
        for li, L in enumerate(self.layers):
            A = L.attention_h
            Q, K, V = (AG.linear(x, getattr(A, n).weight, None, vN, k1) for n in "QKV")
            Ee = AG.linear(ef, A.E.weight, None, vE, k1)
            a = AG.edge_attention(Q, K, V, Ee, plan, rplan, L.num_heads)
            pd = L.dropout
            if pd:
                a = AG.dropout(a, pd, snap, 1 + 2 * li)
            o = AG.linear(a, L.O_h.weight, L.O_h.bias, vN, k1)
            x1 = AG.bn_act(AG.masked_add(o, x, vN, k1), L.batch_norm1_h, vN, k1, relu=False)
            f = AG.linear(x1, L.FFN_h_layer1.weight, L.FFN_h_layer1.bias, vN, k1, relu=True)
            if pd:
                f = AG.dropout(f, pd, snap, 2 + 2 * li)
            f = AG.linear(f, L.FFN_h_layer2.weight, L.FFN_h_layer2.bias, vN, k1)
            x = AG.bn_act(AG.masked_add(f, x1, vN, k1), L.batch_norm2_h, vN, k1, relu=False)
        self._h_last = x.detach()
        return self._readout_grad(x, plan, vB, k1)

    # ------------------------------------------------------------------ full_graph True: every node attends to its whole molecule
    def _full_eval(self):
        """Eval cache of a full-graph net: cat[W_Q; W_K; W_V; W_Q2; W_K2] per layer as ONE packed [5d, d] Linear, and the layer's two
        class tables E(embedding_e.weight), E_2(embedding_e.weight) [C, d] — in eval they depend on parameters only."""
        def build():
            emb = self.embedding_e.weight.detach().float().contiguous()
            out = {"proj": [], "tab": []}
            for L in self.layers:
                A = L.attention_h
                W = torch.cat([getattr(A, n).weight.detach().float() for n in ("Q", "K", "V", "Q_2", "K_2")], 0).contiguous()
                out["proj"].append(ops.PackedLinear(ops.pack_weight(W), W.shape[0], W.shape[1], None))
                out["tab"].append((ops.masked_linear(emb, _pack(A.E)), ops.masked_linear(emb, _pack(A.E_2))))
            return out
        return self._cached("full", build)

    def _forward_full(self, g, h, p, e):
        """transformer_net.py:86-150 with full_graph True: `g` is the complete graph of every molecule (ops.make_full_graph), g.edata['real']
        marks the bonds and `e` holds a class for every pair.  Per layer the five node projections, the two [C, d] class tables and ONE
        sn_full_attention_f32 launch — no per-edge projection exists.  Dropout sites and their ordinals as in the sparse net."""
        try:
            real = g.edata["real"]
        except (AttributeError, KeyError, TypeError):
            raise ValueError("TransformerNet with full_graph=True reads g.edata['real'] (1 for a bond, 0 for any other pair of the "
                             "complete graph): build the graph with ops.make_full_graph") from None
        pe, N, hidx, p, train, grad = self._prologue(g, h, p)
        if real.numel() != e.numel():
            raise ValueError("TransformerNet: g.edata['real'] and e must both have one entry per edge")
        codes = ops.full_graph_codes(e, real)
        status = torch.zeros(1, dtype=torch.int32, device=h.device)     # a bond class outside embedding_e: one word for all layers
        if grad:
            batch, ei, B = self._plan(g, N)
            hg = self._forward_full_grad(ops.build_plan(batch, ei, B, 0), batch, ei, B, hidx, p, codes, status)
        else:
            plan = cached_plan(g, N)
            attend = lambda Q, K, V, Q2, K2, Tr, Tf, L: ops.full_attention(Q, K, V, Q2, K2, Tr, Tf, codes, L.gamma.detach(), plan,      # noqa: E731
                                                                           L.num_heads, status=status)
            x, hg = self._full_value(plan, hidx, p, train, h.device, attend)
            self._h_last = x
        if ops.deferring():
            ops.defer("embed", status)
        elif int(status.item()):
            raise IndexError(ops.EMBEDDING_INDEX_ERROR)
        self.g = g
        return hg, g

    def _forward_full_grad(self, plan, batch, ei, B, hidx, p, codes, status):
        """Differentiable train-mode forward of a full-graph net: AG.full_attention's adjoint (sn_full_attention_bwd_f32) hands back the
        gradients of the five projections, of the two class tables — which reach E.weight, E_2.weight and embedding_e.weight through
        the [C, d] Linears that made them — and of gamma."""
        rplan = ops.build_plan(batch, ei.flip(0).contiguous(), B, 0)
        attend = lambda Q, K, V, Q2, K2, Tr, Tf, L: AG.full_attention(Q, K, V, Q2, K2, Tr, Tf, L.gamma, codes, plan, rplan, L.num_heads,     # noqa: E731
                                                                      status)
        return self._full_grad(plan, hidx, p, attend)

    def _full_value(self, plan, hidx, p, train, dev, attend):
        """The value paths of a full-graph net (eval with its cached packed projections, train mode) around `attend`, the form's
        attention launch -> (x, hg)."""
        with torch.no_grad():
            snap = self._drop_snap(train, dev)
            x = self._encode(ops.embedding_sum(hidx, [self.embedding_h.weight]), p, snap)
            if not train and self._fusable():
                fz = self._full_eval()
                for li, L in enumerate(self.layers):
                    d = L.out_channels
                    P5 = ops.masked_linear(x, fz["proj"][li])                 # [N, 5d] = Q | K | V | Q_2 | K_2, read in place
                    Q, K, V, Q2, K2 = (P5[:, i * d:(i + 1) * d] for i in range(5))
                    Tr, Tf = fz["tab"][li]
                    a = attend(Q, K, V, Q2, K2, Tr, Tf, L)
                    s1, s2 = self._bn(L.batch_norm1_h, False), self._bn(L.batch_norm2_h, False)
                    x1 = ops.masked_linear(a, self._pk(L.O_h), residual=x, residual_pre=True, scale=s1.scale, shift=s1.shift)
                    f = ops.masked_linear(x1, self._pk(L.FFN_h_layer1), relu=True)
                    x = ops.masked_linear(f, self._pk(L.FFN_h_layer2), residual=x1, residual_pre=True, scale=s2.scale, shift=s2.shift)
            else:
                emb = self.embedding_e.weight.detach().float().contiguous()
                for li, L in enumerate(self.layers):
                    A = L.attention_h
                    Q, K, V, Q2, K2 = (ops.masked_linear(x, self._pk(getattr(A, n))) for n in ("Q", "K", "V", "Q_2", "K_2"))
                    Tr, Tf = ops.masked_linear(emb, self._pk(A.E)), ops.masked_linear(emb, self._pk(A.E_2))
                    a = attend(Q, K, V, Q2, K2, Tr, Tf, L)
                    pd = L.dropout if train else 0.0
                    if pd:
                        a = ops.dropout(a, pd, snap, 1 + 2 * li)
                    o = ops.masked_linear(a, self._pk(L.O_h))
                    x1 = self._bn_res(o, x, L.batch_norm1_h, train)
                    f = ops.masked_linear(x1, self._pk(L.FFN_h_layer1), relu=True)
                    if pd:
                        f = ops.dropout(f, pd, snap, 2 + 2 * li)
                    f = ops.masked_linear(f, self._pk(L.FFN_h_layer2))
                    x = self._bn_res(f, x1, L.batch_norm2_h, train)
            return x, self._readout(x, plan)

    def _full_grad(self, plan, hidx, p, attend):
        """The differentiable train-mode layers of a full-graph net around `attend`, the form's attention node."""
        vN, _, vB, k1 = _bucket_rows(self)          # (a padded batch: the bond form under DGLBucketedStep)
        snap = self._drop_snap(True, hidx.device)
        x = self._encode_grad(hidx, p, vN, k1, snap)
        emb = self.embedding_e.weight
        for li, L in enumerate(self.layers):
            A = L.attention_h
            Q, K, V, Q2, K2 = (AG.linear(x, getattr(A, n).weight, None, vN, k1) for n in ("Q", "K", "V", "Q_2", "K_2"))
            Tr, Tf = AG.linear(emb, A.E.weight), AG.linear(emb, A.E_2.weight)
            a = attend(Q, K, V, Q2, K2, Tr, Tf, L)
            pd = L.dropout
            if pd:
                a = AG.dropout(a, pd, snap, 1 + 2 * li)
            o = AG.linear(a, L.O_h.weight, L.O_h.bias, vN, k1)
            x1 = AG.bn_act(AG.masked_add(o, x, vN, k1), L.batch_norm1_h, vN, k1, relu=False)
            f = AG.linear(x1, L.FFN_h_layer1.weight, L.FFN_h_layer1.bias, vN, k1, relu=True)
            if pd:
                f = AG.dropout(f, pd, snap, 2 + 2 * li)
            f = AG.linear(f, L.FFN_h_layer2.weight, L.FFN_h_layer2.bias, vN, k1)
            x = AG.bn_act(AG.masked_add(f, x1, vN, k1), L.batch_norm2_h, vN, k1, relu=False)
        self._h_last = x.detach()
        return self._readout_grad(x, plan, vB, k1)

    # ------------------------------------------------------------------ full_graph True from the molecular graph (full_graph_input "bonds")
    def _forward_bonds(self, g, h, p, e):
        """The full-graph net on the MOLECULAR graph and its bond classes [E]: the layers of `_forward_full` around
        sn_bond_full_attention_f32 (its adjoint: sn_bond_full_attention_bwd_f32, no reverse plan).  Row validity of a padded batch from
        `_bucket_rows`: the spare graph is skipped, padding edges are no bonds.  One two-word status for all layers (a bond class
        outside embedding_e; a self loop or a repeated bond), handed to ops.defer_status where one collects — no host read then."""
        pe, N, hidx, p, train, grad = self._prologue(g, h, p)
        e = e.long().reshape(-1)
        status = torch.zeros(2, dtype=torch.int32, device=h.device)
        _, vE, vB, _ = _bucket_rows(self)
        if grad:
            batch, ei, B = self._plan(g, N)
            plan = ops.build_plan(batch, ei, B, 0)
            attend = lambda Q, K, V, Q2, K2, Tr, Tf, L: AG.bond_full_attention(Q, K, V, Q2, K2, Tr, Tf, L.gamma, e, plan, L.num_heads,     # noqa: E731
                                                                               status, vB, vE)
            hg = self._full_grad(plan, hidx, p, attend)
        else:
            plan = cached_plan(g, N)
            attend = lambda Q, K, V, Q2, K2, Tr, Tf, L: ops.bond_full_attention(Q, K, V, Q2, K2, Tr, Tf, e, L.gamma.detach(), plan,     # noqa: E731
                                                                                L.num_heads, status=status, graph_valid=vB, edge_valid=vE)
            x, hg = self._full_value(plan, hidx, p, train, h.device, attend)
            self._h_last = x
        ops.check_bond_status(status)
        self.g = g
        return hg, g


# ---------------------------------------------------------------------------------------------------------------
# GAT: nets/ZINC_graph_regression/gat_net.py:19-148 on dgl.nn.pytorch.GATConv
class GATConv(nn.Module):
    """Parameter container with dgl.nn.pytorch.GATConv's names and initialisation (fc without bias, attn_l / attn_r [1, heads, out],
    bias [heads*out]; xavier_normal with the ReLU gain, zero bias); the arithmetic is sn_masked_linear_f32 + sn_gat_aggregate_f32."""

    def __init__(self, in_feats, out_feats, num_heads, negative_slope=0.2):
        super().__init__()
        # (sn_gat_aggregate_f32: one lane per channel up to 64, two up to 128 — GAT_ZINC_NoPE / _LapPE.json have heads of 65)
        if out_feats > 128:
            raise ValueError("HIP GATConv: head width <= 128")
        self.in_feats, self.out_feats, self.num_heads, self.negative_slope = in_feats, out_feats, num_heads, negative_slope
        self.fc = nn.Linear(in_feats, out_feats * num_heads, bias=False)
        self.attn_l = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.attn_r = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.bias = nn.Parameter(torch.zeros(num_heads * out_feats))
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)


class GATNet(_DGLNet):
    """nets/ZINC_graph_regression/gat_net.py:19-148 for pe_init = 'lap_pe', lap_lspe = False (GAT_ZINC_LapPE_signinv_GIN.json):
    h = embedding_h(h) + embedding_p(p), L GATConv(ReLU) layers — the first L-1 with their heads flattened, the last averaged over the
    heads (:108-110) — mean / sum readout, MLPReadout.  'GAT (no edge feature)': the edge embedding is a parameter of the
    state_dict only.  Same constructor, forward contract `model(g, h, p, e, snorm_n) -> (scores, g)`, state_dict keys and attached
    `sign_inv_net`.  No BatchNorm in this net, and `dropout` is read and never used (as in the reference): with in_feat_dropout 0 eval and
    train mode compute the same value; in_feat_dropout > 0 drops embedding_h(h) in train mode (site 0).  With gradients enabled in train
    mode the differentiable path (`_forward_grad`)."""

    def __init__(self, net_params):
        super().__init__()
        p = net_params
        hidden, out_dim = p["hidden_dim"], p["out_dim"]
        H = self.n_heads = p["n_heads"]
        self._init_common(p, "GATNet", [(p["readout"] == "max" and not self._max_readout, "readout sum / mean")], in_feat_dropout="after_e")
        #                     (batch_norm, residual: read and ignored by the reference too)
        if self.n_layers < 2:
            raise ValueError("GATNet: L >= 2 (gat_net.py:62-66 always builds a first and a last layer)")
        self.layers = nn.ModuleList([GATConv(hidden, hidden, H)] + [GATConv(H * hidden, hidden, H) for _ in range(1, self.n_layers - 1)] +
                                    [GATConv(H * hidden, out_dim, H)])
        self._init_tail(p)

    def forward(self, g, h, p, e, snorm_n=None):
        pe, N, hidx, p, train, grad = self._prologue(g, h, p)
        if grad:
            batch, ei, B = self._plan(g, N)
            hg = self._forward_grad(ops.build_plan(batch, ei, B, 0), batch, ei, B, hidx, p)
            self.g = g
            return hg, g
        plan = cached_plan(g, N)
        with torch.no_grad():
            zero_deg = (plan.rowptr[1:] == plan.rowptr[:-1]).any()
            x = ops.embedding_sum(hidx, [self.embedding_h.weight])                    # raises IndexError as nn.Embedding (one host read)
            x = self._encode(x, p, self._drop_snap(train, h.device) if self.p_in_feat else None)                 # h + embedding_p(p)  (:97-99)
            H = self.n_heads
            for i, L in enumerate(self.layers):
                f = ops.masked_linear(x, self._fc(L))
                x = ops.gat_aggregate(f, L.attn_l.detach(), L.attn_r.detach(), L.bias.detach(), plan, H, L.negative_slope, relu=True)
            # the last layer's heads are averaged (:110): sum over the head axis, then 1/H
            x = ops.slot_sum(x.view(N * H, -1), N, H)
            x = ops.pointwise(x, scale=self._const(1.0 / H, x.shape[1]), shift=self._const(0.0, x.shape[1]))
            hg = self._readout(x, plan)
        zero_msg = ("There are 0-in-degree nodes in the graph: GATConv's edge softmax is undefined for them (DGL raises "
                    "DGLError here unless allow_zero_in_degree is set, which gat_net.py:62-66 leaves at False)")
        if ops.deferring():              # a recorded step (serving.GraphedDGLForward) must not wait for the host: its check() reads these
            ops.defer("plan", plan)
            ops.defer("flag", zero_deg, zero_msg)
        else:
            plan.check()                 # malformed batch
            if bool(zero_deg):
                raise ValueError(zero_msg)
        self.g = g
        self._h_last = x
        return hg, g

    def _forward_grad(self, plan, batch, ei, B, hidx, p):
        """Differentiable train-mode forward (SURVEY.md §8 f1 for this net): the same ops as autograd nodes; the GATConv adjoint is
        sn_gat_aggregate_bwd_f32 (CSR walks over the in-edges, then over the out-edges; no atomics)."""
        vN, _, vB, k1 = _bucket_rows(self)          # (train_graph.DGLBucketedStep: padding rows enter no statistic and no gradient)

        def zero_deg():
            z = plan.rowptr[1:] == plan.rowptr[:-1]
            # (a padded batch: E_cap - E self-loops may not reach all N_cap - N padding nodes — only valid nodes count)
            return (z if vN is None else z & (vN != 0)).any()

        zero_msg = "There are 0-in-degree nodes in the graph: GATConv's edge softmax is undefined for them"
        if ops.deferring():              # a captured step must not wait for the host: its check() reads these
            ops.defer("plan", plan)
            ops.defer("flag", zero_deg(), zero_msg)
        else:
            plan.check()
            if bool(zero_deg()):
                raise ValueError(zero_msg)
        rplan = ops.build_plan(batch, ei.flip(0).contiguous(), B, 0)           # edges grouped by SOURCE
        N, H = hidx.shape[0], self.n_heads
        x = self._encode_grad(hidx, p, vN, k1, self._drop_snap(True, hidx.device) if self.p_in_feat else None)
        for L in self.layers:
            x = AG.gat_aggregate(AG.linear(x, L.fc.weight, None, vN, k1), L.attn_l, L.attn_r, L.bias, plan, rplan, H, L.negative_slope, True)
        x = AG.slot_sum(x.view(N * H, -1), N, H)                               # mean over the heads (:110)
        x = AG.act_residual(x, rowscale=torch.full((N,), 1.0 / H, dtype=torch.float32, device=x.device))
        self._h_last = x.detach()
        return self._readout_grad(x, plan, vB, k1)

    def _fc(self, L):
        def build():
            w = L.fc.weight.detach()
            return ops.PackedLinear(ops.pack_weight(w), w.shape[0], w.shape[1], None)
        return build() if self.training else self._cached(("fc", id(L)), build)

    def _const(self, v, n):
        return self._cached(("const", float(v), int(n)),
                            lambda: torch.full((n,), float(v), dtype=torch.float32, device=self.embedding_h.weight.device))
