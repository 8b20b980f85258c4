"""-m gpu: the one-layer register-attention rho at d = 128 as ONE twelve-wave workgroup per CU (k_rho_fused<8, true, true, false, 12,
PREC_HIGHEST, RES3>: twelve nodes per bin behind one weight ring), driven through fused.RhoPlan.run(..., waves=12) on random rows.

The set-up is that of tests/test_rho_resident_gpu.py: a seeded SetTransformer (one layer, four heads, LayerNorm affine vectors that are
not the identity) on x ~ N(0, 1) [N, K, d], zero in the slots a node does not have.  `out_sum` of the twelve-wave form is held to

  * the float64 oracle of the same layer (oracle.pyg_signnet.encoder_layer, summed over the slots) with the two rules the stage grid
    uses (parity_util.attributed and parity_util.elementwise),
  * the layer-at-a-time kernels of the forward's `use_fused = False` path with parity_util.close,
  * the four-wave form (waves=4) BIT FOR BIT: a wave's rows, products and accumulation orders do not depend on the number of waves
    that share the weight ring,

and two runs of the twelve-wave form must be equal.  No tolerance of its own.  Each shape is the smallest that reaches one way the
form can go wrong:

    n1          one graph of one node: eleven of the twelve waves run the layer on zero rows and store nothing
    n13         one graph of 13 nodes: a second bin with one live wave, on a grid of one workgroup per bin
    mixed       graphs of 3, 9, 16, 17, 37 nodes, max_k 16: N = 82 is seven bins, the last partial; slot counts below, at and above 16
    mixed-k8    the same graphs with max_k = 8 (K = 8 dense slots: rows 8..15 of every tile are padding)
    rounds      N = 12 * 256 + 5 nodes in graphs of 9..37: 257 bins, more than any part has CUs, so the `bin += gridDim.x` loop and
                the prefetch of the next bin's rows run
"""
import functools

import pytest
import torch

import parity_util as PU
import stage_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 128
ROUNDS_N = 12 * 256 + 5


def _round_sizes():
    """graphs of 9..37 nodes, cycling, that add up to ROUNDS_N exactly"""
    sizes, n, rem = [], 9, ROUNDS_N
    while rem >= n + 9:
        sizes.append(n)
        rem -= n
        n = 9 + (n - 9 + 11) % 29
    sizes += [rem] if rem <= 37 else [rem // 2, rem - rem // 2]
    assert sum(sizes) == ROUNDS_N and min(sizes) >= 9 and max(sizes) <= 37
    return tuple(sizes)


SHAPES = {
    "n1": (16, (1,)),
    "n13": (16, (13,)),
    "mixed": (16, (3, 9, 16, 17, 37)),
    "mixed-k8": (8, (3, 9, 16, 17, 37)),
    "rounds": (16, _round_sizes()),
}


def _seed(name):
    return SC.seed_of(SC.Case("rho-twelve-waves", name, ""))


@functools.lru_cache(maxsize=None)
def _module():
    """the SetTransformer of width D on the CPU (shared by the shapes, never modified)"""
    from signnet_basisnet_amd import pyg
    torch.manual_seed(_seed("module"))
    rho = pyg.SetTransformer(D, 1, "gine")
    SC.randomize(rho, _seed("affine"))
    ln = [m for m in rho.modules() if isinstance(m, torch.nn.LayerNorm)]
    assert len(ln) == 2 and all(not torch.equal(m.weight, torch.ones_like(m.weight)) and bool(m.bias.abs().max() > 0) for m in ln)
    return rho.eval()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """-> (x [N, K, d] float32, mask [N, K], slot sum float32, slot sum float64) from the oracle's encoder layer; computed once"""
    from oracle import pyg_signnet as O
    kmax, sizes = SHAPES[name]
    N, K = sum(sizes), kmax
    nv = torch.repeat_interleave(torch.tensor([min(n, kmax) for n in sizes]), torch.tensor(sizes))
    mask = torch.arange(K)[None, :] < nv[:, None]
    g = torch.Generator().manual_seed(_seed(name))
    x = torch.randn(N, K, D, generator=g) * mask.unsqueeze(-1)
    sd = {"rho." + k: v.detach().clone() for k, v in _module().state_dict().items()}
    with torch.no_grad():
        s32 = O.encoder_layer(sd, "rho.transformer_layers.0", x, mask).sum(dim=1)
        s64 = O.encoder_layer(SC.to_f64(sd), "rho.transformer_layers.0", x.double(), mask).sum(dim=1)
    return x, mask, s32, s64


def _layer_path(rho, x, nv, N, K):
    """the forward's layer-at-a-time rho (pyg.SignNetGNN with use_fused = False): one kernel per Linear / attention / LayerNorm"""
    from signnet_basisnet_amd import ops, pyg
    tl = rho.transformer_layers[0]
    a, f = tl.slf_attn, tl.pos_ffn
    q = ops.masked_linear(x, pyg._pack(a.w_qs), nv, K)
    k = ops.masked_linear(x, pyg._pack(a.w_ks), nv, K)
    v = ops.masked_linear(x, pyg._pack(a.w_vs), nv, K)
    o = ops.set_attention(q, k, v, N, K, pyg.N_HEAD, nv, None)
    o = ops.masked_linear(o, pyg._pack(a.fc), nv, K)
    y = ops.masked_layernorm(o, x, a.norm.ln.weight.detach(), a.norm.ln.bias.detach(), pyg.LN_EPS, nv, K)
    z = ops.masked_linear(y, pyg._pack(f.w_1), nv, K, relu=True)
    z = ops.masked_linear(z, pyg._pack(f.w_2), nv, K)
    return ops.slot_sum(ops.masked_layernorm(z, y, f.norm.ln.weight.detach(), f.norm.ln.bias.detach(), pyg.LN_EPS, nv, K), N, K)


@pytest.mark.parametrize("name", list(SHAPES))
def test_twelve_wave_rho(name):
    import copy
    from signnet_basisnet_amd import fused, ops, pyg
    kmax, sizes = SHAPES[name]
    x, mask, s32, s64 = _reference(name)
    N, K, B = sum(sizes), kmax, len(sizes)
    assert N == mask.shape[0] and (name != "rounds" or (N == ROUNDS_N and (N + 11) // 12 == 257))
    rho = copy.deepcopy(_module()).to(DEV).eval()
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes)).to(DEV)
    plan = ops.build_plan(batch, torch.empty(2, 0, dtype=torch.int64, device=DEV), B, kmax, bins=True)
    assert torch.equal(plan.nvalid.cpu().long(), mask.sum(1)), "the plan's valid slots are the reference's mask"
    xd = x.to(DEV).view(N * K, D).contiguous()
    with torch.no_grad():
        rp = fused.RhoPlan(rho, None, pyg.N_HEAD, pyg.LN_EPS)
        assert rp.params_hp is None and rp.params.n_layers == 1 and rp.params.has_pos == 0, "natural layout, ONE"
        out = rp.run(plan, xd, None, K, waves=12)
        again = rp.run(plan, xd, None, K, waves=12)
        four = rp.run(plan, xd, None, K, waves=4)
        layer = _layer_path(rho, xd, plan.nvalid, N, K)
    plan.check()
    assert out.shape == (N, D) and bool(torch.isfinite(out).all())
    assert torch.equal(out, again), f"{name}: two runs of the twelve-wave form differ"
    assert torch.equal(out, four), f"{name}: the twelve-wave form does not repeat the four-wave form bit for bit"
    label = f"rho twelve waves {name} (d {D}, max_k {kmax}, N {N}) out_sum"
    e = PU.attributed(out, s32, s64, label)
    n = PU.elementwise(out, s32, label + " (element-wise)", ref64=s64)
    print(f"\n{label}: |hip - f64| {e[0]:.2e}, |cpu32 - f64| {e[1]:.2e}, {n} elements attributed", end="")
    PU.close(out, layer, f"{label}: fused vs layer kernels", ref64=s64)
