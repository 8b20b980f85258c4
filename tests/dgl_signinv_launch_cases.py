"""The cases of tests/test_dgl_signinv_launch_order_gpu.py: which sign-invariant encoder of the DGL tree runs in which mode, how a case's
launches are recorded, and the recorded literals (tests/dgl_signinv_launch_orders.py).  `python tests/dgl_signinv_launch_cases.py`
prints that module's text for the tree it runs on; the literals were printed on the commit before the four encoders were moved under one
base class (dgl_deepsigns._SignInvEncoder), before any edit to the package, and the one `forward` has to reproduce them.

An eager case is the ORDERED list of C-ABI entry points of TWO consecutive calls on a fresh model and a fresh Graph, with MARK between
them: the first call carries the plan and pack launches, the second is the steady state.  The batch is three bidirectional rings of 3, 7
and 5 nodes (N = 15, 30 directed edges) with k = 4: every node has in-edges (GCNDeepSigns does not raise), the 3-node graph is smaller
than k (the masked encoder's slot mask is live); hidden 8, phi_out 4, 3 layers, use_bn: a GIN middle layer with its inter-layer
BatchNorm, a GraphConv with in <= out and one with in > out, 2 attention heads of width 4.  A captured case is the name -> count dict
of one DGLBucketedStep.step of a GINNet behind the encoder (two warm-up runs and the capture: no event can be placed during a
capture, so the order is not available there), in a bucket with padding."""
import collections
import os
import sys
import types

import torch

DEV = "cuda:0"
KINDS = ("gin", "masked_gin", "gcn", "transformer")
MODES = ("eval", "nograd", "grad")  # eval | train-mode forward under no_grad | train-mode forward + backward of y.sum()
SIZES, K, HIDDEN, PHI_OUT, LAYERS = (3, 7, 5), 4, 8, 4, 3
MARK = "|"                          # stands between the two calls of an eager case
CAPTURED_SIZES = [5, 9, 12, 7, 3]


def _cases():
    c = collections.OrderedDict()
    for kind in KINDS:
        for mode in MODES:
            c[f"{kind}-relu-{mode}"] = dict(kind=kind, mode=mode)
        for mode in MODES[1:]:
            c[f"{kind}-dropout-{mode}"] = dict(kind=kind, mode=mode, dropout=0.1)
        for mode in MODES:
            c[f"{kind}-tanh-{mode}"] = dict(kind=kind, mode=mode, activation="tanh")
    for mode in MODES:
        c[f"transformer-elu-{mode}"] = dict(kind="transformer", mode=mode, activation="elu")
    for kind in ("gin", "masked_gin"):
        c[f"{kind}-relu-layers-eval"] = dict(kind=kind, mode="eval", fused_stages=False)
    c["gin-h52-high-eval"] = dict(kind="gin", mode="eval", hidden=52, precision="high")      # padded width 64: the smallest reduced mode
    for kind in ("gin", "gcn"):
        c[f"captured-GINNet-{kind}"] = dict(kind=kind, mode="captured")
    return c


CASES = _cases()
EAGER = [n for n, s in CASES.items() if s["mode"] != "captured"]


def rings():
    """(Graph, x [N, K, 1]) of the eager cases, fresh per call."""
    from signnet_basisnet_amd import dgl_deepsigns as DS
    src, dst, off = [], [], 0
    for n in SIZES:
        for i in range(n):
            a, b = off + i, off + (i + 1) % n
            src += [a, b]
            dst += [b, a]
        off += n
    g = DS.Graph(torch.tensor(src, device=DEV), torch.tensor(dst, device=DEV), list(SIZES))
    x = torch.randn(sum(SIZES), K, 1, generator=torch.Generator().manual_seed(3)).to(DEV)
    return g, x


def encoder(spec):
    """The encoder of an eager case, through the factory of the module that admits its settings."""
    from signnet_basisnet_amd import activation_signinv, dgl_deepsigns, dropout_signinv
    mod = activation_signinv if spec.get("activation") else dropout_signinv if spec.get("dropout") else dgl_deepsigns
    torch.manual_seed(7)
    m = mod.get_sign_inv_net(dict(sign_inv_net=spec["kind"], hidden_dim=spec.get("hidden", HIDDEN), phi_out_dim=PHI_OUT,
                                  sign_inv_layers=LAYERS, pos_enc_dim=K, dropout=spec.get("dropout", 0.0),
                                  sign_inv_activation=spec.get("activation", "relu"), device=DEV))
    with torch.no_grad():                               # GraphConv's bias is zero-initialised: make it count
        for n_, p_ in m.named_parameters():
            if spec["kind"] == "gcn" and n_.startswith("enc.layers.") and n_.endswith(".bias"):
                p_.copy_(0.1 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(5)))
    m = m.to(DEV)
    if spec.get("dropout"):
        m.seed_dropout(11, 0)
    if "fused_stages" in spec:
        m.fused_stages = spec["fused_stages"]
    if spec.get("precision"):
        m.matmul_precision = spec["precision"]
    return m


def call(model, g, x, mode):
    """One call of an eager case; the output."""
    if mode == "grad":
        y = model(g, x)
        y.sum().backward()
        return y.detach()
    with torch.no_grad():
        return model(g, x)


def _captured(spec, rec):
    from signnet_basisnet_amd import dgl_configs, dgl_deepsigns as DS, dgl_nets, optim, synth
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    from test_pyg_bucketed_baselines_gpu import _Count          # (counts launch names, places no event: works through a capture)
    cls, p = dgl_configs.net_params("gin", DEV)
    p["sign_inv_net"] = spec["kind"]
    torch.manual_seed(3)
    net = getattr(dgl_nets, cls)(p).to(DEV).train()
    data = synth.make_batch(len(CAPTURED_SIZES), seed=5, sizes=CAPTURED_SIZES)
    src, dst = data.edge_index
    b = types.SimpleNamespace(g=DS.Graph(src.to(DEV), dst.to(DEV), data.sizes), h=data.x.squeeze(-1).to(DEV),
                              p=synth.dgl_pos_enc(data, p["pos_enc_dim"]).to(DEV), e=data.edge_attr.to(DEV),
                              t=torch.randn(len(CAPTURED_SIZES), 1, generator=torch.Generator().manual_seed(105)).to(DEV))
    N, E = data.batch.numel(), data.edge_index.shape[1]
    step = DGLBucketedStep(net, optim.FlatAdam(net.parameters(), lr=1e-3), max_graphs=8)
    rec.only = _Count()
    with rec:
        step.step(b.g, b.h, b.p, b.e, None, b.t, bucket=(N + 9, E + 14))          # 9 padding nodes, 14 padding edges
    torch.cuda.synchronize()
    step.check()
    assert not rec.spans
    n = dict(rec.only.n)
    step.release()
    torch.cuda.synchronize()
    return n


def record(name):
    """The launches of case `name` on the current tree: a list of entry-point names (eager) or a name -> count dict (captured)."""
    from signnet_basisnet_amd import ops
    spec = CASES[name]
    rec = ops.KernelTimer()
    if spec["mode"] == "captured":
        return _captured(spec, rec)
    (g, x), model = rings(), encoder(spec)
    model.train(spec["mode"] != "eval")
    with rec:
        call(model, g, x, spec["mode"])
        rec.spans.append((MARK, None, None))
        call(model, g, x, spec["mode"])
    torch.cuda.synchronize()
    return [s[0] for s in rec.spans]


def _literal(name, got):
    """One entry of dgl_signinv_launch_orders.py: the names of a list joined by blanks (wrapped), a dict as it is."""
    if isinstance(got, dict):
        items = ", ".join(f"{k!r}: {v}" for k, v in sorted(got.items()))
        return f"    {name!r}: {{{items}}},"
    lines, cur = [], ""
    for n in got:
        if cur and len(cur) + len(n) + 1 > 120:
            lines.append(cur)
            cur = ""
        cur = f"{cur} {n}" if cur else n
    lines.append(cur)
    body = "\n".join(f"        {(l + ' ')!r}" for l in lines[:-1]) + ("\n" if len(lines) > 1 else "") + f"        {lines[-1]!r}"
    return f"    {name!r}: (\n{body}\n    ).split(),"


def main():
    print('"""The recorded launches of tests/dgl_signinv_launch_cases.py (printed by `python tests/dgl_signinv_launch_cases.py`): per case')
    print('the ordered entry points of two consecutive eager calls (MARK between them), or the name -> count dict of a captured step."""')
    print("ORDERS = {")
    for name in CASES:
        print(_literal(name, record(name)), flush=True)
    print("}")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
