"""The baselines of the two PyG trees on the HIP stack (the rows SignNet is compared against there).

  Alchemy/main_alchemy.py:24-33        NetGINE(64) (baseline_gin.py): six GINE-style convolutions and a Set2Set readout
  GINESignNetPyG/train/zinc.py:31-46   GNN(None, None, nhid, 1, nlayer, 'GINEConv', dropout, pool, res=True): `pyg.GNN.forward`

Same constructors, same `forward(data)`, same `state_dict` keys as the reference, so its checkpoints load unchanged.  The modules hold
parameters; the arithmetic runs in libsignnet_hip.so (ops.py / autograd.py).  There is no CPU path.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib as _lib_mod
from . import ops
from .pyg import GNN  # noqa: F401  (the second baseline, re-exported)
from .pyg import _drop_eval_cache, _eval_cache, _pack

SET2SET_STEPS = 6        # baseline_gin.py:43
NUM_FEATURES = 6         # baseline_gin.py:33 (Alchemy's node features); edge features: 4 (baseline_gin.py:36-41)
NUM_EDGE_FEATURES = 4
NUM_TARGETS = 12         # baseline_gin.py:46


class GINConv(nn.Module):
    """out_i = mlp((1 + eps) x_i + sum_{j -> i} relu(x_j + bond_encoder(edge_attr_ji)))   (baseline_gin.py:9-26; parameters only)."""

    def __init__(self, emb_dim, dim1, dim2):
        super().__init__()
        self.bond_encoder = nn.Sequential(nn.Linear(emb_dim, dim1), nn.ReLU(), nn.Linear(dim1, dim1))
        self.mlp = nn.Sequential(nn.Linear(dim1, dim1), nn.ReLU(), nn.Linear(dim1, dim2))
        self.eps = nn.Parameter(torch.zeros(1))


class Set2Set(nn.Module):
    """PyG's Set2Set(in_channels, processing_steps) with one LSTM layer: the parameters of `lstm`, the readout of ops.set2set."""

    def __init__(self, in_channels, processing_steps):
        super().__init__()
        self.in_channels, self.out_channels, self.processing_steps = in_channels, 2 * in_channels, processing_steps
        self.lstm = nn.LSTM(self.out_channels, in_channels, 1)

    def reset_parameters(self):
        self.lstm.reset_parameters()

    def _tensors(self):
        m = self.lstm
        return m.weight_ih_l0, m.weight_hh_l0, m.bias_ih_l0, m.bias_hh_l0

    def forward(self, x, graph_ptr):
        """x [N, d], graph_ptr int32 [B+1] (a batch plan's) -> [B, 2d]; differentiable when gradients are recorded."""
        ops.require_cuda(x, graph_ptr)
        if torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in self._tensors())):
            from . import autograd as AG
            return AG.set2set(x, graph_ptr, *self._tensors(), self.processing_steps)
        return ops.set2set(x.contiguous(), graph_ptr, *(t.detach() for t in self._tensors()), self.processing_steps)


class NetGINE(ops.DeferredStatus, nn.Module):
    def __init__(self, dim):
        super().__init__()
        if not 1 <= dim <= 128:
            raise ValueError("NetGINE: the Set2Set kernel serves 1 <= dim <= 128")
        self.conv1 = GINConv(NUM_EDGE_FEATURES, NUM_FEATURES, dim)
        for i in range(2, 7):
            setattr(self, f"conv{i}", GINConv(NUM_EDGE_FEATURES, dim, dim))
        self.set2set = Set2Set(dim, processing_steps=SET2SET_STEPS)
        self.fc1 = nn.Linear(2 * dim, dim)
        self.fc4 = nn.Linear(dim, NUM_TARGETS)

    def _convs(self):
        return [getattr(self, f"conv{i}") for i in range(1, 7)]

    def train(self, mode=True):
        _drop_eval_cache(self)              # the packed weights: parameters may change before the next eval forward
        return super().train(mode)

    def invalidate(self):
        """Call after modifying parameters in place while in eval mode (as SignNetGNN.invalidate)."""
        _drop_eval_cache(self)

    def forward(self, data):
        ops.require_cuda(data.x, data.edge_index, data.edge_attr, data.batch)
        grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if self.training or grad:
            _drop_eval_cache(self)
        with _lib_mod.stream_scope():
            return self._forward_grad(data) if grad else self._forward(data)

    def _forward(self, data):
        """No gradients recorded (the net has no BatchNorm and no dropout: train and eval mode compute the same).  Eval mode keeps the
        packed weights between forwards; train mode packs them per call (an optimiser step may lie between two calls)."""
        cache = {} if self.training else _eval_cache(self)

        def lin(x, m, relu=False):
            if id(m) not in cache:
                cache[id(m)] = _pack(m)
            return ops.masked_linear(x, cache[id(m)], relu=relu)

        plan = ops.build_plan(data.batch, data.edge_index, int(data.num_graphs), 0)
        x, ea = data.x.contiguous(), data.edge_attr.contiguous()
        for conv in self._convs():
            e = lin(lin(ea, conv.bond_encoder[0], relu=True), conv.bond_encoder[2])
            a = ops.gine_aggregate(x, e, plan, conv.eps.detach())
            x = lin(lin(a, conv.mlp[0], relu=True), conv.mlp[2], relu=True)      # (the ReLU behind every conv, baseline_gin.py:51-56)
        q = self.set2set(x, plan.graph_ptr)
        y = lin(lin(q, self.fc1, relu=True), self.fc4)
        plan.check()
        return y

    def _forward_grad(self, data):
        """Under the switch `_bucket` (train_graph.BucketedStep) `data` is a padded batch: every Linear takes the validity vector of its
        rows (K = 1), so padding rows are zeros and enter no weight gradient.  The net has no BatchNorm: the empty graphs [B, B_cap - 1)
        and the spare graph only have to read out finite values (Set2Set: r = 0 / 1e-16 = 0 on a graph without nodes, and the spare
        graph's rows are zeros), which the masked Linears and the masked loss keep out of everything else.  Without the switch every
        launch and argument is as before."""
        from . import autograd as AG
        B = int(data.num_graphs)
        vN, vE, vB, k1 = ops.bucket_validity(self)
        plan = ops.build_plan(data.batch, data.edge_index, B, 0)
        rplan = ops.build_plan(data.batch, data.edge_index.flip(0).contiguous(), B, 0)      # out-edge CSR
        x, ea = data.x.contiguous(), data.edge_attr.contiguous()

        def lin(x_, m, relu=False, v=None):
            return AG.linear(x_, m.weight, m.bias, v, 0 if v is None else k1, relu=relu)

        if k1:
            x = AG.mask_rows(x, vN, k1)             # (the first aggregation reads the raw rows: eps's gradient sums x * da over all rows)
        for conv in self._convs():
            e = lin(lin(ea, conv.bond_encoder[0], relu=True, v=vE), conv.bond_encoder[2], v=vE)
            a = AG.gine_aggregate(x, e, conv.eps, plan, rplan)
            x = lin(lin(a, conv.mlp[0], relu=True, v=vN), conv.mlp[2], relu=True, v=vN)
        q = self.set2set(x, plan.graph_ptr)
        y = lin(lin(q, self.fc1, relu=True, v=vB), self.fc4, v=vB)
        self._finish_train(plan)                    # (a captured step must not synchronise: check_train() reads the status words)
        return y
