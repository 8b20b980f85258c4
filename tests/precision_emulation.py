"""CPU reference of the matmul-precision modes of the fused eval stages (`matmul_precision`, DESIGN.md "Matmul precision").

The kernels split every fp32 operand EXACTLY into three bf16 planes by truncation — h = top 16 bits of x, m = top 16 bits of x - h,
l = the rest — and a mode issues a subset of the plane products, fp32 accumulate:

    highest  hh + hm + mh + hl + lh + mm        high  hh + hm + mh        medium  hh

`emu_mm` evaluates exactly those products (every plane product and the sum in float64), so at GEMM level it differs from a kernel only by
the kernel's fp32 accumulation.  `emulated_oracle` / `emulated_dgl_oracle` are the float64 oracles with the weight GEMMs of the fused phi /
rho stages replaced by `emu_mm` (the input cast to fp32 first, as the kernels hold it): an approximation at model level — the activations
between the Linears are float64 here and fp32 in the kernels — which the tests allow for with parity_util.close_conditioned's factor.

Derived per-GEMM bounds with mag = |x| . |w|^T: a bf16 plane keeps 8 significant bits, |x - h| < 2^-7 |x|, |x - h - m| < 2^-15 |x|, so
the products a mode drops are bounded by C_MODE[mode] * mag.
"""
import torch

MODES = ("highest", "high", "medium")
_PRODUCTS = {"highest": ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)), "high": ((0, 0), (0, 1), (1, 0)), "medium": ((0, 0),)}
# leading terms: highest drops ml + lm (2 * 2^-22); high drops hl + lh (<= 2^-14) and mm (<= 2^-14), the rest is below 2^-21; medium
# drops hm + mh (2 * 2^-7) and what high drops.  (The plane bounds are strict and never met by every element of a row at once: on
# random normal operands the worst element is 1.6e-5 mag for high and 3.5e-3 mag for medium.)
C_MODE = {"highest": 2.0 ** -21, "high": 2.0 ** -13, "medium": 2.0 ** -6 + 2.0 ** -14}


def planes(x):
    """fp32 tensor -> (h, m, l), fp32 tensors with x == h + m + l exactly; h, m: bf16-representable (truncation of the bit pattern)."""
    x = x.detach().to(torch.float32).contiguous()
    h = (x.view(torch.int32) & -65536).view(torch.float32)
    r = x - h                                             # exact
    m = (r.contiguous().view(torch.int32) & -65536).view(torch.float32)
    return h, m, r - m                                    # (exact; <= 8 significant bits)


def emu_mm(x, w, mode, acc=torch.float64):
    """x [..., K] . w [O, K]^T with the partial products of `mode`, result in `acc` (no bias).  acc = float32: the same planes and
    products, multiplied and summed in float32 — what fp32 arithmetic alone does to the mode."""
    xp = [p.to(acc) for p in planes(x)]
    wp = [p.to(acc) for p in planes(w)]
    y = None
    for i, j in _PRODUCTS[mode]:
        t = xp[i] @ wp[j].transpose(-1, -2)
        y = t if y is None else y + t
    return y


def _is_weight_gemm(W):
    return W.dim() == 2 and W.shape[0] > 1 and W.shape[1] > 1


def emulated_oracle(mode, monkeypatch, sd, cfg, data, max_k=None, acc=torch.float64):
    """oracle.pyg_signnet.signnet_gnn in float64 with `_linear` replaced, for the duration of the call, by emu_mm for the weight GEMMs the
    fused stages evaluate in `mode`: keys under sign_net.phi / sign_net.rho whose weight has both dimensions > 1, rho.out excluded (it is
    folded into the GINE stage, which stays at highest).  acc = float32: the oracle runs in float32 on the float32 state dict, the
    products accumulated in float32.  -> (y, stages dict)."""
    import parity_util as PU
    from oracle import pyg_signnet as O
    orig = O._linear

    def _linear(sd_, pfx, x):
        W = sd_[pfx + ".weight"]
        staged = (pfx.startswith("sign_net.phi") or pfx.startswith("sign_net.rho")) and not pfx.startswith("sign_net.rho.out")
        if not (staged and _is_weight_gemm(W)):
            return orig(sd_, pfx, x)
        y = emu_mm(x, W, mode, acc).to(x.dtype)
        b = sd_.get(pfx + ".bias")
        return y if b is None else y + b

    out = {}
    with monkeypatch.context() as mp, torch.no_grad():
        mp.setattr(O, "_linear", _linear)
        if acc == torch.float64:
            y = O.signnet_gnn(PU.to_f64(sd), cfg, PU.data_f64(data), training=False, max_k=max_k, out=out)
        else:
            y = O.signnet_gnn(sd, cfg, data, training=False, max_k=max_k, out=out)
    return y, out


class _FShim:
    """torch.nn.functional with `linear` = emu_mm (+ bias) for weights with both dimensions > 1."""

    def __init__(self, mode):
        self._mode = mode

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)

    def linear(self, x, W, b=None):
        if not _is_weight_gemm(W):
            return torch.nn.functional.linear(x, W, b)
        y = emu_mm(x, W, self._mode).to(x.dtype)
        return y if b is None else y + b


def _folded_mlp(mode, acc, round_w):
    """oracle.dgl_deepsigns.mlp as dgl_deepsigns._FusedDeepSigns packs it: the eval BatchNorm behind hidden layer i - 1 is folded into
    Linear i — W' = W diag(scale), b' = b + W shift, restated in float64 — and every Linear with more than one input feature is
    emu_mm on W' (the kernels stream all of them, [1, hidden] tails included, as padded split-packed tiles; the first Linear of the
    first GIN layer has one input and is a vector there).  round_w: W' rounded to float32 before it is split, as the kernels hold it."""
    from oracle import dgl_deepsigns as OD

    def mlp(sd, pfx, x, num_layers, use_bn, activation, training):
        assert not training and activation == "relu", "the stage kernels are eval-mode ReLU"
        for i in range(num_layers):
            W, b = sd[f"{pfx}.lins.{i}.weight"].double(), sd[f"{pfx}.lins.{i}.bias"].double()
            if i > 0 and use_bn:
                q = f"{pfx}.bns.{i - 1}"
                scale = sd[q + ".weight"].double() / torch.sqrt(sd[q + ".running_var"].double() + OD.BN_EPS)
                shift = sd[q + ".bias"].double() - sd[q + ".running_mean"].double() * scale
                W, b = W * scale[None, :], b + W @ shift
            if W.shape[1] > 1:
                y = emu_mm(x, W.float() if round_w else W, mode, acc).to(x.dtype) if mode is not None else x @ W.to(x.dtype).t()
            else:
                y = x @ W.to(x.dtype).t()
            x = y + b.to(x.dtype)
            if i < num_layers - 1:
                x = torch.relu(x)
        return x

    return mlp


def emulated_dgl_oracle(mode, monkeypatch, kind, sd, src, dst, sizes, x, num_layers, k, folded=False, acc=torch.float64, round_w=True):
    """oracle.dgl_deepsigns (float64) with its module attribute `F` replaced, for the duration of the call, by the shim above.
    folded: instead, its `mlp` replaced by the BatchNorm-folded restatement above, which truncates the values the DeepSigns stage
    kernels truncate (up to one ulp of W').  With folded, mode = None evaluates the folded Linears as plain matmuls (round_w = False:
    the folding alone, which is algebra), and acc = float32 runs oracle and products in float32."""
    import parity_util as PU
    from oracle import dgl_deepsigns as OD
    if folded:
        sd_, x_ = (PU.to_f64(sd), x.double()) if acc == torch.float64 else (sd, x.float())
        with monkeypatch.context() as mp, torch.no_grad():
            mp.setattr(OD, "mlp", _folded_mlp(mode, acc, round_w))
            if kind == "gin":
                return OD.gin_deepsigns(sd_, src, dst, x_, num_layers, k)
            return OD.masked_gin_deepsigns(sd_, src, dst, sizes, x_, num_layers, k)
    with monkeypatch.context() as mp, torch.no_grad():
        mp.setattr(OD, "F", _FShim(mode))
        if kind == "gin":
            return OD.gin_deepsigns(PU.to_f64(sd), src, dst, x.double(), num_layers, k)
        return OD.masked_gin_deepsigns(PU.to_f64(sd), src, dst, sizes, x.double(), num_layers, k)


def relmax(a, ref64):
    """max|a - f64| / max|f64|"""
    a, r = a.detach().cpu().double().reshape(ref64.shape), ref64.detach().cpu().double()
    return (a - r).abs().max().item() / max(r.abs().max().item(), 1e-300)
