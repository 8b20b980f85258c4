"""The cases of tests/test_pyg_launch_order_gpu.py: which models run in which mode, how a case's launches are recorded, and the recorded
literals (tests/pyg_launch_orders.py).  `python tests/pyg_launch_cases.py` prints that module's text for the tree it runs on; the
literals were printed on the commit before pyg.GNN's forwards were written as one skeleton with a hook pair per conv type, and the
skeleton has to reproduce them.

An eager case is the ORDERED list of C-ABI entry points of one forward (and backward) on synth.make_batch(6, seed=5), the smallest
batch that still takes every branch, through 2 layers; a captured case is the name -> count dict of one BucketedStep.step (two warm-up
runs and the capture: no event can be placed during a capture, so the order is not available there)."""
import collections
import os
import sys
import types

import torch

DEV = "cuda:0"
TYPES = ("GINEConv", "GINConv", "GCNConv", "GATConv", "SimplifiedPNAConv")
WIDTHS = (16, 18)                   # train_stage.supported(16, 16): the staged links; 18 is no multiple of 4: one launch per op
MODES = ("eval", "nograd", "grad")  # eval | train-mode forward under no_grad | train-mode forward + backward of y.sum()


def _cases():
    c = collections.OrderedDict()
    for kind in TYPES:
        for w in WIDTHS:
            for mode in MODES:
                c[f"{kind}-h{w}-{mode}"] = dict(net="gnn", kind=kind, nhid=w, mode=mode)
    for mode in MODES:
        c[f"GINEConv-h16-mean-{mode}"] = dict(net="gnn", kind="GINEConv", nhid=16, mode=mode, pooling="mean")
        c[f"GCNConv-h18-mean-{mode}"] = dict(net="gnn", kind="GCNConv", nhid=18, mode=mode, pooling="mean")
        c[f"GINEConv-h16-pe-{mode}"] = dict(net="gnn", kind="GINEConv", nhid=16, mode=mode, pe=True)
        c[f"GATConv-h16-pe-{mode}"] = dict(net="gnn", kind="GATConv", nhid=16, mode=mode, pe=True)
        c[f"GINEConv-h16-dropout-{mode}"] = dict(net="gnn", kind="GINEConv", nhid=16, mode=mode, dropout=0.1)
    c["GINEConv-h18-dropout-grad"] = dict(net="gnn", kind="GINEConv", nhid=18, mode="grad", dropout=0.1)
    c["SimplifiedPNAConv-h16-dropout-grad"] = dict(net="gnn", kind="SimplifiedPNAConv", nhid=16, mode="grad", dropout=0.1)
    c["pyg.GNN-h16-grad"] = dict(net="pyg.GNN", nhid=16, mode="grad")
    c["pyg.GNN-h16-l1-grad"] = dict(net="pyg.GNN", nhid=16, mode="grad", nlayer=1)          # one layer: no stacked edge block
    c["NetGINE-16-grad"] = dict(net="NetGINE", mode="grad")
    for variant in ("gine", "alchemy"):
        for stages in (True, False):
            c[f"SignNetGNN-{variant}-stages{int(stages)}-grad"] = dict(net="SignNetGNN", variant=variant, stages=stages, mode="grad")
    c["captured-SimplifiedPNAConv-h16"] = dict(net="gnn", kind="SimplifiedPNAConv", nhid=16, mode="captured")
    c["captured-NetGINE-16"] = dict(net="NetGINE", mode="captured")
    return c


CASES = _cases()


def _batch(features, eigen):
    from signnet_basisnet_amd import synth
    host = synth.make_batch(6, seed=5, features=features)
    if not eigen:
        host = types.SimpleNamespace(**{k: v for k, v in vars(host).items() if not k.startswith("eigen")})
    return synth.batch_to(host, DEV)


def _model(spec):
    from signnet_basisnet_amd import dropout_models, pyg, pyg_baselines, pyg_gnn_types
    torch.manual_seed(7)
    net = spec["net"]
    if net == "NetGINE":
        return pyg_baselines.NetGINE(16)
    if net == "SignNetGNN":
        feats = (None, None) if spec["variant"] == "gine" else (6, 4)
        m = pyg.SignNetGNN(*feats, 16, 1, 2, 2, variant=spec["variant"], max_k=8)
        m.train_stages = spec["stages"]
        return m
    if net == "pyg.GNN":
        return pyg.GNN(None, None, spec["nhid"], 1, spec.get("nlayer", 2), "gine")
    cls = dropout_models.GNN if spec.get("dropout") else pyg_gnn_types.GNN
    m = cls(None, None, spec["nhid"], 1, 2, spec["kind"], dropout=spec.get("dropout", 0), pooling=spec.get("pooling", "add"))
    if spec.get("dropout"):
        m.seed_dropout(11, 0)
    return m


def record(name):
    """The launches of case `name` on the current tree: a list of entry-point names (eager) or a name -> count dict (captured)."""
    from signnet_basisnet_amd import ops, optim
    spec = CASES[name]
    alchemy = spec["net"] == "NetGINE" or spec.get("variant") == "alchemy"
    data = _batch("alchemy" if alchemy else "zinc", eigen=spec["net"] == "SignNetGNN")
    model = _model(spec).to(DEV)
    mode = spec["mode"]
    model.train(mode != "eval")
    args = ()
    if spec.get("pe"):
        args = (torch.randn(data.batch.numel(), spec["nhid"], generator=torch.Generator().manual_seed(3)).to(DEV),)
    torch.manual_seed(1)                # (SignNetGNN draws its attention-dropout masks from torch's device generator)
    rec = ops.KernelTimer()
    if mode == "captured":
        from signnet_basisnet_amd.train_graph import BucketedStep
        from test_pyg_bucketed_baselines_gpu import _Count          # (counts launch names, places no event: works through a capture)
        N, E = data.batch.numel(), data.edge_index.shape[1]
        target = torch.randn(6, 12 if alchemy else 1, generator=torch.Generator().manual_seed(2)).to(DEV)
        step = BucketedStep(model, optim.FlatAdam(model.parameters(), lr=1e-3), max_graphs=8)
        rec.only = _Count()
        with rec:
            step.step(data, target, bucket=(N + 37, E + 50, 1, 1))          # an adverse bucket: 37 padding nodes, 50 padding edges
        torch.cuda.synchronize()
        step.check()
        assert not rec.spans
        return dict(rec.only.n)
    with rec:
        if mode == "grad":
            model(data, *args).sum().backward()
        else:
            with torch.no_grad():
                model(data, *args)
    torch.cuda.synchronize()
    return [s[0] for s in rec.spans]


def _literal(name, got):
    """One entry of pyg_launch_orders.py: the names of a list joined by blanks (wrapped), a dict as it is."""
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
    print('"""The recorded launches of tests/pyg_launch_cases.py (printed by `python tests/pyg_launch_cases.py`): per case the ordered')
    print('entry points of an eager run, or the name -> count dict of a captured step."""')
    print("ORDERS = {")
    for name in CASES:
        print(_literal(name, record(name)), flush=True)
    print("}")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
