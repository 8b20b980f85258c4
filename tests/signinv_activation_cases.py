"""Shared by tests/test_signinv_activation_cpu.py and tests/test_signinv_activation_gpu.py: the case tables, the kernel grid and float64
restatements of what `--sign_inv_activation tanh | elu` adds —

  act_ref / act_grad_ref      the two entry points sn_act_affine_f32 / sn_act_affine_bwd_f32 in float64 (torch)
  ulp32                       the float32 unit in the last place at a float64 value: the unit every kernel error is counted in
  mlp_ref / gin_ref / gcn_ref the reference's layers/mlp.py MLP, layers/gnns.py GIN and GCN with the activation as a parameter, the
                              BatchNorm buffers moved as nn.BatchNorm1d moves them and the dropout sites of tests/signinv_dropout_cases.py
  module_ref                  the four encoders from a reference-keyed state_dict; net_ref: GatedGCNNet behind handle_lap

The activation-free helpers (BatchNorm, GraphConv's propagation, the SetTransformerEncoder) are tests/deepsigns_variant_cases.py's.  The
fixtures (tests/golden/ds_act_*.npz: the reference's own modules, tests/golden/make_signinv_activation.py) pin the restatements in the CPU
test; the GPU test then compares kernels and modules with them in float64.
"""
import types

import numpy as np
import torch
import torch.nn.functional as F

import deepsigns_variant_cases as V
import dropout_cases as DC
import signinv_dropout_cases as SC

ENCODER_CASES = ["ds_act_gin_tanh_h16_c4_l3_k4", "ds_act_masked_gin_tanh_h12_c5_l3_k6", "ds_act_gcn_tanh_h19_c4_l3_k5",
                 "ds_act_tf_tanh_h16_l2_k4", "ds_act_tf_elu_h14_l2_k3", "ds_act_gin_tanh_dropout_h8_c4_l3_k4"]
DROPOUT_CASE = "ds_act_gin_tanh_dropout_h8_c4_l3_k4"
NET_CASE = "ds_act_net_gatedgcn_gin_tanh_add"
CLASSES = SC.CLASSES
ACT_CODES = {"tanh": 1, "elu": 2}          # SN_ACT_TANH, SN_ACT_ELU

# what the reference accepts per encoder (layers/gnns.py:13 looks 'relu' / 'tanh' up before any MLP is built; layers/mlp.py:23-30)
ACCEPTED = {"gin": ("relu", "tanh"), "masked_gin": ("relu", "tanh"), "gcn": ("relu", "tanh"), "transformer": ("relu", "elu", "tanh")}
REFUSED = {"gin": {"elu": KeyError, "swish": KeyError}, "masked_gin": {"elu": KeyError, "swish": KeyError},
           "gcn": {"elu": KeyError, "swish": KeyError}, "transformer": {"swish": ValueError}}

# ----------------------------------------------------------------------------- the kernel grid
ROWS = [0, 1, 63, 64, 65, 1000]            # empty, one row, around a wave, several workgroups
COLS = [1, 3, 4, 19, 64, 95, 128]
K_MASK = 5                                 # rows are (node, slot) with 5 slots; nvalid cycles through 0 .. 5
# layout -> (extra floats per row, pointer offset in floats): a contiguous matrix; rows of a matrix four floats wider (the vector
# condition holds where C % 4 == 0); rows one float wider (ld % 4 != 0 alone falsifies it); a view one float into a buffer (the
# pointer alone falsifies it)
LAYOUTS = {"contiguous": (0, 0), "ld+4": (4, 0), "ld+1": (1, 0), "offset": (0, 1)}
POINTS = [0.0, -0.0, 1e-8, -1e-8, 20.0, -20.0, 100.0, -100.0, float("inf"), float("-inf"), float("nan")]
BIG = (2100, 1024)                         # 2100 * 256 row groups > 2048 * 256: the grid's second pass


def path(C, lds, ptrs, vec_ptrs=()):
    """'row' / 'flat' / 'scalar': the kernel the host picks (csrc/activation.hip: act_launch), restated.  lds: the leading dimensions
    of the matrices, ptrs their byte addresses, vec_ptrs those of scale / shift (0 for NULL)."""
    mats = all(p % 16 == 0 for p in ptrs)
    if mats and all(p % 16 == 0 for p in vec_ptrs) and C % 4 == 0 and all(ld % 4 == 0 for ld in lds):
        return "row"
    if mats and all(ld == C for ld in lds):
        return "flat"
    return "scalar"


def grid_input(R, C, seed):
    """float32 [R, C]: random normal (scaled by 3: both tails of tanh, elu's negative branch) with POINTS written over the first elements."""
    x = 3.0 * torch.randn(R, C, generator=torch.Generator().manual_seed(seed))
    flat = x.view(-1)
    n = min(len(POINTS), flat.numel())
    flat[:n] = torch.tensor(POINTS[:n])
    return x


def nvalid_for(R, K=K_MASK):
    return (torch.arange((R + K - 1) // K) % (K + 1)).to(torch.int32)


def rowvalid(R, nvalid, K=K_MASK):
    r = torch.arange(R)
    return (r % K) < nvalid[r // K].long() if R else torch.zeros(0, dtype=torch.bool)


def act_f(name):
    return {"relu": torch.relu, "tanh": torch.tanh, "elu": F.elu}[name]


def act_ref(x, act, valid=None, scale=None, shift=None):
    """sn_act_affine_f32 in float64: (a = act(x), y = valid ? a * scale + shift : 0)."""
    a = act_f(act)(x.double())
    y = a if scale is None else a * scale.double() + shift.double()
    if valid is not None:
        y = torch.where(valid[:, None], y, torch.zeros_like(y))
    return a, y


def act_grad_ref(dy, a, act, valid=None):
    """sn_act_affine_bwd_f32 in float64 from the SAVED float32 activation output `a` — the only thing the adjoint reads: dy * act'(a)."""
    a, dy = a.double(), dy.double()
    d = 1.0 - a * a if act == "tanh" else torch.where(a > 0, torch.ones_like(a), a + 1.0)
    dx = dy * d
    if valid is not None:
        dx = torch.where(valid[:, None], dx, torch.zeros_like(dx))
    return dx


def ulp32(v):
    """The float32 unit in the last place at the magnitude of the float64 tensor v (the spacing at 0 is the smallest subnormal)."""
    m = v.abs().to(torch.float32).numpy()
    return torch.from_numpy(np.spacing(m).astype(np.float64))


def ulps(got, ref, unit=None):
    """Largest |got - ref| over the finite entries of ref, in units of ulp32(unit or ref); non-finite entries must agree exactly."""
    got, ref = got.detach().cpu().double(), ref.double()
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), "NaN is kept, and nothing else becomes one"
    inf = torch.isinf(ref)
    assert torch.equal(got[inf], ref[inf]), "+-inf saturates as in torch"
    if not bool(fin.any()):
        return 0.0
    u = ulp32(ref if unit is None else unit)
    return float(((got - ref).abs()[fin] / u[fin]).max())


# ----------------------------------------------------------------------------- the modules
def params(fx):
    hidden, out, layers, k = (int(v) for v in fx.meta["params"])
    kind = str(fx.meta["kind"])
    return types.SimpleNamespace(hidden=hidden, out=out, layers=layers, k=k, kind=kind, cls=CLASSES[kind],
                                 act=str(fx.meta["activation"]), p=float(fx.meta["dropout_p"]))


class Drop:
    """The fixture's dropout masks in call order (make_dropout_deepsigns.Sites): site ordinal s multiplies by keep_s / (1 - p)."""

    def __init__(self, fx):
        self.p = float(fx.meta["dropout_p"])
        self.masks, self.s = [], 0
        if self.p > 0.0:
            shapes = fx.meta["dropout_site_shapes"]
            self.masks = [SC.unpack(fx.out[f"dropout_mask/{s}"].numpy(), shapes[s]) for s in range(len(shapes))]

    def __call__(self, x, training):
        if not training or self.p == 0.0:
            return x
        keep = torch.from_numpy(self.masks[self.s]).to(x.dtype) * float(DC.scale_of(self.p))
        self.s += 1
        return x * keep.view(x.shape)


def mlp_ref(sd, pfx, x, n_lins, training, buffers, act, drop=None):
    """layers/mlp.py:37-56 with use_bn: Linear -> act -> BatchNorm -> dropout per hidden layer, final Linear."""
    f = act_f(act)
    for i in range(n_lins - 1):
        x = f(F.linear(x, sd[f"{pfx}.lins.{i}.weight"], sd[f"{pfx}.lins.{i}.bias"]))
        x = V._bn(sd, f"{pfx}.bns.{i}", x, training, buffers)
        if drop is not None:
            x = drop(x, training)
    return F.linear(x, sd[f"{pfx}.lins.{n_lins - 1}.weight"], sd[f"{pfx}.lins.{n_lins - 1}.bias"])


def gin_ref(sd, src, dst, x, training, buffers, act, drop=None):
    """GIN.forward (layers/gnns.py:102-114) on [N, K, c]; GINConv(apply_func, 'sum') = apply_func((1 + eps) h_i + sum_{j -> i} h_j)."""
    L = len({k.split(".")[2] for k in sd if k.startswith("enc.layers.")})
    for l in range(L):
        if l:
            if drop is not None:
                x = drop(x, training)
            x = V._bn(sd, f"enc.bns.{l - 1}", x, training, buffers)
        a = (1 + sd[f"enc.layers.{l}.eps"].to(x.dtype)) * x + torch.zeros_like(x).index_add(0, dst, x.index_select(0, src))
        x = mlp_ref(sd, f"enc.layers.{l}.apply_func", a, 2, training, buffers, act, drop)
    return x


def gcn_ref(sd, src, dst, x, training, buffers, act, drop=None):
    """deepsigns_variant_cases.gcn_ref with GraphConv's activation as a parameter and the inter-layer dropout (gnns.py:33-45)."""
    f = act_f(act)
    L = len({k.split(".")[2] for k in sd if k.startswith("enc.layers.")})
    for l in range(L):
        if l:
            if drop is not None:
                x = drop(x, training)
            x = V._bn(sd, f"enc.bns.{l - 1}", x, training, buffers)
        W, b = sd[f"enc.layers.{l}.weight"], sd[f"enc.layers.{l}.bias"]
        if W.shape[0] > W.shape[1]:
            x = V.gcn_propagate_ref(torch.matmul(x, W), src, dst, b)
        else:
            N = x.shape[0]
            cout, cin = V.gcn_norms(src, dst, N, x.dtype)
            h = x * cout.reshape(N, 1, 1)
            x = torch.matmul(torch.zeros_like(h).index_add(0, dst, h.index_select(0, src)), W) * cin.reshape(N, 1, 1) + b
        if l < L - 1:
            x = f(x)
    return x


def encoder_ref(sd, p, src, dst, sizes, x, training=False, buffers=None, drop=None):
    """The four forwards of layers/deepsigns.py: x [N, k, 1] -> [N, k, 1]."""
    N = x.shape[0]
    n_rho = V._n_lins(sd, "rho")
    if p.kind == "transformer":
        xp = F.linear(x, sd["embed.weight"], sd["embed.bias"])
        xm = F.linear(-x, sd["embed.weight"], sd["embed.bias"])
        z = torch.cat([V.set_transformer_ref(sd, sizes, xp[:, i]) + V.set_transformer_ref(sd, sizes, xm[:, i]) for i in range(p.k)], dim=1)
    else:
        enc = gcn_ref if p.kind == "gcn" else gin_ref
        z = enc(sd, src, dst, x, training, buffers, p.act, drop) + enc(sd, src, dst, -x, training, buffers, p.act, drop)
        if p.kind == "masked_gin":
            n_per_node = torch.repeat_interleave(torch.as_tensor(sizes), torch.as_tensor(sizes))
            mask = torch.arange(p.k)[None, :] < n_per_node[:, None]
            z = z.masked_fill(~mask.unsqueeze(-1), 0.0).sum(dim=1)
        else:
            z = z.reshape(N, -1)
    return mlp_ref(sd, "rho", z, n_rho, training, buffers, p.act, drop).reshape(N, p.k, 1)


def _sd(fx, dtype, grads):
    sd = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in fx.sd.items()}
    if grads:
        for k_, v in sd.items():
            if v.is_floating_point() and not k_.endswith(("running_mean", "running_var", ".eps")):
                v.requires_grad_(True)
    return sd


def module_ref(fx, dtype, training=False, buffers=None, grads=False):
    """The fixture's encoder restated in `dtype` on the fixture's batch and masks -> y, or (y, {parameter: gradient}) for the fixture's
    cotangent (train mode) when grads."""
    p = params(fx)
    sd = _sd(fx, dtype, grads)
    x = fx.inp["pos_enc"].to(dtype).unsqueeze(-1)
    ei = fx.inp["edge_index"]
    y = encoder_ref(sd, p, ei[0], ei[1], [int(s) for s in fx.inp["sizes"]], x, training, buffers, Drop(fx))
    if not grads:
        return y.detach()
    (y * fx.inp["cotangent"].to(dtype)).sum().backward()
    return y.detach(), {k_: v.grad for k_, v in sd.items() if v.requires_grad and v.grad is not None}


def build(fx, device=None, module=None, activation=None, dropout=None):
    """The package's encoder of a fixture (a class of activation_signinv unless `module` says otherwise) with the fixture's
    reference-keyed state_dict loaded strictly."""
    if module is None:
        from signnet_basisnet_amd import activation_signinv as module
    p = params(fx)
    args = (1, p.hidden, p.out, p.layers, p.k) + ((device or "cpu",) if p.kind == "masked_gin" else ())
    net = getattr(module, p.cls)(*args, use_bn=True, dropout=p.p if dropout is None else dropout,
                                 activation=p.act if activation is None else activation)
    net.load_state_dict(fx.sd, strict=True)
    return net if device is None else net.to(device)


# ----------------------------------------------------------------------------- the net-level fixture
def net_params(fx, device):
    hidden, L, k = (int(v) for v in fx.meta["hidden_L_k"])
    return dict(SC.NET_COMMON, hidden_dim=hidden, out_dim=hidden, L=L, pos_enc_dim=k, readout="mean", sign_inv_net=str(fx.meta["kind"]),
                sign_inv_activation=str(fx.meta["activation"]), pe_aggregate=str(fx.meta["pe_aggregate"]),
                sign_inv_layers=int(fx.meta["sign_inv_layers"]), phi_out_dim=int(fx.meta["phi_out_dim"]), device=device, dropout=0.0,
                in_feat_dropout=0.0)


def net_ref(fx, dtype, training=False, grads=False):
    """GatedGCNNet behind handle_lap (train_ZINC_graph_regression.py:20-25, :77-80) in `dtype`: the encoder restated here, the base net by
    oracle.dgl_nets.gatedgcn_net."""
    from oracle import dgl_nets as ON
    hidden, L, k = (int(v) for v in fx.meta["hidden_L_k"])
    sd = _sd(fx, dtype, grads)
    enc_sd = {k_[len("sign_inv_net."):]: v for k_, v in sd.items() if k_.startswith("sign_inv_net.")}
    p = types.SimpleNamespace(kind=str(fx.meta["kind"]), act=str(fx.meta["activation"]), k=k)
    ei, sizes = fx.inp["edge_index"], [int(s) for s in fx.inp["sizes"]]
    pe = encoder_ref(enc_sd, p, ei[0], ei[1], sizes, fx.inp["pos_enc"].to(dtype).unsqueeze(-1), training).squeeze(-1)
    y = ON.gatedgcn_net(sd, ei[0], ei[1], fx.inp["sizes"], fx.inp["x"].squeeze(-1), pe, fx.inp["edge_attr"], L,
                        pe_aggregate=str(fx.meta["pe_aggregate"]), readout="mean", training=training)
    if not grads:
        return y.detach()
    (y * fx.inp["cotangent"].to(dtype)).sum().backward()
    return y.detach(), {k_: v.grad for k_, v in sd.items() if v.requires_grad and v.grad is not None}
