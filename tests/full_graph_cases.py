"""Full-graph attention of the graph Transformer (GraphPrediction/layers/transformer.py:155-228, full_graph True) and the dataset step
data/molecules.py:211-235 `make_full_graph`, restated in plain torch for the tests: any dtype, differentiable by torch.autograd.
The restatements are pinned to the reference's own runs by tests/test_full_graph_cpu.py (fixtures tests/golden/fullgraph_*.npz) and
are what tests/test_full_graph_gpu.py compares the kernels with.  Also the shared builders: fixture nets and the op grid's inputs."""
import functools
import math
import types

import torch

import golden_util as G

FIXTURES = ["fullgraph_tf_h32_l2_k8_add", "fullgraph_tf_h24_l3_nope_mean", "fullgraph_tf_h16_l2_signinv_concat"]
GRID_SIZES = [1, 2, 3, 5, 9, 17, 33, 65, 70]
COMMON = dict(num_atom_type=28, num_bond_type=4, in_feat_dropout=0.0, dropout=0.0, batch_norm=True, residual=True, edge_feat=True,
              device="cpu", lap_lspe=False, use_lapeig_loss=False, lambda_loss=1, alpha_loss=1e-4, layer_norm=True, full_graph=True)


@functools.lru_cache(maxsize=None)
def fixture(name):
    return G.load(name)


def net_params(fx, **over):
    hidden, L, k, heads = (int(v) for v in fx.meta["params"])
    p = dict(COMMON, hidden_dim=hidden, out_dim=hidden, L=L, pos_enc_dim=k, n_heads=heads, readout=str(fx.meta["readout"]),
             pe_init=str(fx.meta["pe_init"]), lap_method=str(fx.meta["lap_method"]), pe_aggregate=str(fx.meta["pe_aggregate"]),
             sign_inv_net="gin" if str(fx.meta["lap_method"]) == "sign_inv" else "none", sign_inv_layers=3, sign_inv_activation="relu",
             phi_out_dim=4)
    p.update(over)
    return p


# ----------------------------------------------------------------------------- the op
def full_attention_ref(Q, K, V, Q2, K2, T_real, T_fake, codes, gamma, src, dst, heads, want_terms=False):
    """out [N, heads*dk] of the full-graph attention over the edge list (src -> dst) with codes = 2 * class + real, in the reference's
    order of operations (src_dot_dst, scaling, imp_exp_attn, exp_real / exp_fake, the two send_and_recv sums in edge order)."""
    N, d = Q.shape
    dk = d // heads
    cls, real = codes.long() >> 1, (codes.long() & 1).bool()
    v3 = lambda t: t.reshape(-1, heads, dk)
    r3 = real[:, None, None]
    A = torch.where(r3, v3(K)[src], v3(K2)[src])
    B = torch.where(r3, v3(Q)[dst], v3(Q2)[dst])
    T = torch.where(r3, v3(T_real)[cls], v3(T_fake)[cls])
    t = (((A * B) / math.sqrt(dk)) * T).sum(-1, keepdim=True)                  # [E, H, 1]
    L = torch.clamp(gamma, min=0.0, max=1.0)
    ex = torch.exp(t.clamp(-5, 5))
    s = torch.where(r3, ex / (L + 1), L * ex / (L + 1))
    wV = torch.zeros(N, heads, dk, dtype=Q.dtype).index_add(0, dst, v3(V)[src] * s)
    z = torch.zeros(N, heads, 1, dtype=Q.dtype).index_add(0, dst, s)
    out = (wV / (z + torch.full_like(z, 1e-6))).reshape(N, d)
    if want_terms:
        return out, t.squeeze(-1), s.squeeze(-1), z.squeeze(-1)
    return out


def dgamma_terms_rss(inp, dout):
    """Root-sum-square, in float64, of the per-(edge, head) terms ds_e * exp(clamp t_e) * (-/+ 1 / (L + 1)^2) whose sum is dL: the
    scale a one-entry sum with cancellation is judged by."""
    a = to_dtype(inp, torch.float64)
    out, t, s, z = full_attention_ref(a.Q, a.K, a.V, a.Q2, a.K2, a.Tr, a.Tf, a.codes, a.gamma, a.src, a.dst, a.heads, want_terms=True)
    H = a.heads
    dk = a.Q.shape[1] // H
    g = dout.double().reshape(-1, H, dk)
    o3, v3 = out.reshape(-1, H, dk), a.V.reshape(-1, H, dk)
    ds = ((g[a.dst] * v3[a.src]).sum(-1) - (g * o3).sum(-1)[a.dst]) / (z[a.dst] + 1e-6)
    L = float(a.gamma.clamp(0, 1))
    real = (a.codes.long() & 1).bool()[:, None]
    term = ds * torch.exp(t.clamp(-5, 5)) * torch.where(real, -1.0, 1.0) / (L + 1) ** 2
    return float(term.pow(2).sum().sqrt())


FLOATS = ("Q", "K", "V", "Q2", "K2", "Tr", "Tf", "gamma")


def to_dtype(inp, dtype, grad=False):
    out = types.SimpleNamespace(**vars(inp))
    for n in FLOATS:
        t = getattr(inp, n).detach().to(dtype).clone()
        setattr(out, n, t.requires_grad_(True) if grad else t)
    return out


def run_ref(inp, dout, dtype):
    """(out, {name: gradient}) of the restatement in `dtype` by torch.autograd."""
    a = to_dtype(inp, dtype, grad=True)
    out = full_attention_ref(a.Q, a.K, a.V, a.Q2, a.K2, a.Tr, a.Tf, a.codes, a.gamma, a.src, a.dst, a.heads)
    out.backward(dout.to(dtype))
    return out.detach(), {n: getattr(a, n).grad for n in FLOATS}


# ----------------------------------------------------------------------------- the net around the op (what pins the op to the fixtures)
def full_transformer_net(sd, fx, training, out=None):
    """TransformerNet.forward (transformer_net.py:86-150) with full_graph True on a fixture's batch, from a state_dict of any dtype: the
    layers of oracle.dgl_nets' sparse form with the attention replaced by full_attention_ref over the class tables."""
    import torch.nn.functional as F
    from oracle import dgl_deepsigns as OD
    from oracle import dgl_nets as ON
    hidden, L, k, heads = (int(v) for v in fx.meta["params"])
    src, dst = fx.inp["full_src"], fx.inp["full_dst"]
    codes = 2 * fx.inp["e_full"] + fx.inp["real"]
    dtype = sd["embedding_h.weight"].dtype
    h = sd["embedding_h.weight"][fx.inp["x"].reshape(-1)]
    if str(fx.meta["pe_init"]) == "lap_pe":
        p = fx.inp["pos_enc"].to(dtype)
        if str(fx.meta["lap_method"]) == "sign_inv":
            ssd = {kk[len("sign_inv_net."):]: v for kk, v in sd.items() if kk.startswith("sign_inv_net.")}
            p = OD.gin_deepsigns(ssd, src, dst, p.unsqueeze(-1), 3, k, training=training).squeeze(-1)
        pp = F.linear(p, sd["embedding_p.weight"], sd["embedding_p.bias"])
        h = F.linear(torch.cat([h, pp], 1), sd["pe_proj.weight"], sd["pe_proj.bias"]) if str(fx.meta["pe_aggregate"]) == "concat" else h + pp
    emb = sd["embedding_e.weight"]
    for l in range(L):
        a = f"layers.{l}.attention_h"
        lin = lambda n, x: F.linear(x, sd[f"{a}.{n}.weight"])          # noqa: E731
        att = full_attention_ref(lin("Q", h), lin("K", h), lin("V", h), lin("Q_2", h), lin("K_2", h), lin("E", emb), lin("E_2", emb), codes,
                                 sd[f"layers.{l}.gamma"], src, dst, heads)
        x = h + F.linear(att, sd[f"layers.{l}.O_h.weight"], sd[f"layers.{l}.O_h.bias"])
        x = ON._bn_rows(sd, f"layers.{l}.batch_norm1_h", x, training)
        y = F.linear(torch.relu(F.linear(x, sd[f"layers.{l}.FFN_h_layer1.weight"], sd[f"layers.{l}.FFN_h_layer1.bias"])),
                     sd[f"layers.{l}.FFN_h_layer2.weight"], sd[f"layers.{l}.FFN_h_layer2.bias"])
        h = ON._bn_rows(sd, f"layers.{l}.batch_norm2_h", x + y, training)
    if out is not None:
        out["h_last"] = h
    return ON._mlp_readout(sd, ON._readout(h, fx.inp["sizes"], str(fx.meta["readout"])))


# ----------------------------------------------------------------------------- make_full_graph
def full_pairs(sizes):
    """The complete directed graph of every graph, batch node ids: per graph u-major, v ascending, v != u."""
    src, dst, off = [], [], 0
    for n in sizes:
        u = torch.arange(n).repeat_interleave(n)
        v = torch.arange(n).repeat(n)
        keep = u != v
        src.append(u[keep] + off)
        dst.append(v[keep] + off)
        off += n
    return torch.cat(src), torch.cat(dst)


def make_full_graph_ref(sizes, src, dst, e):
    """data/molecules.py:211-235 over a batch -> (src, dst, real, e_full) int64: a pair that is an edge of the sparse graph is real and
    keeps the edge's class; every other pair gets real = 0, class 0."""
    fs, fd = full_pairs(sizes)
    N = int(sum(sizes))
    key = {int(k): i for i, k in enumerate((src * N + dst).tolist())}
    real = torch.zeros(fs.numel(), dtype=torch.int64)
    ef = torch.zeros(fs.numel(), dtype=torch.int64)
    for i, k in enumerate((fs * N + fd).tolist()):
        j = key.get(k)
        if j is not None:
            real[i], ef[i] = 1, int(e[j])
    return fs, fd, real, ef


def molecule_edges(sizes, seed, C=4):
    """A molecule-like sparse batch: per graph a path plus a few chords, both directions, classes in [0, C)."""
    g = torch.Generator().manual_seed(seed)
    src, dst, cls, off = [], [], [], 0
    for n in sizes:
        pairs = {(i, i + 1) for i in range(n - 1)}
        for _ in range(n // 4):
            a, b = sorted(int(v) for v in torch.randint(0, n, (2,), generator=g))
            if a != b:
                pairs.add((a, b))
        for a, b in sorted(pairs):
            c = int(torch.randint(0, C, (1,), generator=g))
            src += [off + a, off + b]
            dst += [off + b, off + a]
            cls += [c, c]
        off += n
    t = lambda v: torch.tensor(v, dtype=torch.int64)
    return t(src), t(dst), t(cls)


# ----------------------------------------------------------------------------- the op grid's inputs
PATTERNS = ("molecule", "all_real", "none_real", "one_direction", "incomplete", "shuffled", "both_kinds")


def op_inputs(heads, dk, C=4, pattern="molecule", gamma=0.1, seed=0, scale=1.0, sizes=tuple(GRID_SIZES)):
    """Inputs of one op case (float32 on the host): node blocks, class tables, the edge list with its codes, gamma, and a cotangent.
    A fake pair may carry any class; `scale` multiplies Q / K / Q_2 / K_2 (the clamp is live for a large one)."""
    sizes = list(sizes)
    g = torch.Generator().manual_seed(1000 + seed)
    N, d = sum(sizes), heads * dk
    rnd = lambda *s: torch.randn(*s, generator=g)
    inp = types.SimpleNamespace(heads=heads, sizes=sizes, C=C)
    inp.Q, inp.K, inp.Q2, inp.K2 = (rnd(N, d) * scale for _ in range(4))
    inp.V = rnd(N, d)
    inp.Tr, inp.Tf = rnd(C, d), rnd(C, d)
    inp.gamma = torch.tensor([gamma], dtype=torch.float32)
    ms, md, mc = molecule_edges(sizes, seed, C)
    fs, fd, real, ef = make_full_graph_ref(sizes, ms, md, mc)
    E = fs.numel()
    fake_cls = torch.randint(0, C, (E,), generator=g)
    cls = torch.where(real.bool(), ef, fake_cls)
    if pattern == "all_real":
        real = torch.ones_like(real)
    elif pattern == "none_real":
        real = torch.zeros_like(real)
    elif pattern == "one_direction":
        real = (fs < fd).long()                       # j -> i real, i -> j fake
    elif pattern == "incomplete":
        keep = torch.rand(E, generator=g) > 0.3
        fs, fd, real, cls = fs[keep], fd[keep], real[keep], cls[keep]
    elif pattern == "shuffled":
        perm = torch.randperm(E, generator=g)
        fs, fd, real, cls = fs[perm], fd[perm], real[perm], cls[perm]
    elif pattern == "both_kinds":                     # every bond once more as a fake edge of another class: a multi-edge
        m = real.bool()
        fs, fd = torch.cat([fs, fs[m]]), torch.cat([fd, fd[m]])
        cls = torch.cat([cls, (cls[m] + 1) % C])
        real = torch.cat([real, torch.zeros(int(m.sum()), dtype=torch.int64)])
    elif pattern != "molecule":
        raise ValueError(pattern)
    inp.src, inp.dst = fs.contiguous(), fd.contiguous()
    inp.codes = (2 * cls + real).to(torch.int32)
    inp.dout = rnd(N, d)
    return inp


# (a few thousand scores: at the grid's ~10^5 some score always falls within 1e-3 of +-5; seed 5 chosen on the CPU so that none does)
CLAMP_CASE = dict(heads=8, dk=8, C=4, pattern="molecule", gamma=0.6, seed=5, scale=2.5, sizes=(3, 5, 9, 17, 2))      # see clamp_conditions


def clamp_conditions(inp):
    """(real beyond +5, fake beyond +5, real beyond -5, fake beyond -5, scores within 1e-3 of +-5) counted in the float64 restatement."""
    a = to_dtype(inp, torch.float64)
    _, t, _, _ = full_attention_ref(a.Q, a.K, a.V, a.Q2, a.K2, a.Tr, a.Tf, a.codes, a.gamma, a.src, a.dst, a.heads, want_terms=True)
    real = (a.codes.long() & 1).bool()[:, None].expand_as(t)
    near = ((t.abs() - 5).abs() < 1e-3).sum()
    return (int((t[real] > 5).sum()), int((t[~real] > 5).sum()), int((t[real] < -5).sum()), int((t[~real] < -5).sum()), int(near))
