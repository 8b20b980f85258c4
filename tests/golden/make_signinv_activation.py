"""Regenerates tests/golden/ds_act_*.npz: the reference's four sign-invariant encoders (GraphPrediction/layers/deepsigns.py over
layers/gnns.py, layers/mlp.py) with `activation` 'tanh' / 'elu', and one base net behind the reference's handle_lap with
`sign_inv_activation='tanh'`, run through the ORIGINAL code on CPU.  The graph library comes from tests/golden/ref_shim_deepsigns/ in
front of tests/golden/ref_shim/ (their GraphConv applies the activation it is handed).  Arrays only; helpers, shims and graphs are
make_golden.py's, make_deepsigns_variants.py's and make_dropout_deepsigns.py's.

    python tests/golden/make_signinv_activation.py            # needs the reference tree where make_golden.py looks for it
    python tests/golden/make_signinv_activation.py --search [N] [case ...]   # print the margin of the N (12) seeds from the listed one on

Every fixture: the seeded state_dict (BatchNorm running statistics and affines randomised), the batch, its positional encoding and a
fixed cotangent; the eval output; the train-mode output, the BatchNorm buffers after that ONE train-mode forward and the gradient of
sum(y * cotangent) w.r.t. every parameter from the reference in float32 (`out/train/y`, `out/train/buffers/`, `out/grad/`) — and output
and gradients once more from a float64 copy (`out/train/y64`, `out/grad64/`).  The dropout case draws the masks of csrc/dropout.hip's
generator exactly as make_dropout_deepsigns.py does and stores them the same way.

Seeds: a train-mode BatchNorm over a few dozen rows amplifies every rounding in front of it (make_deepsigns_variants.py), and tanh
saturates channels, which makes a nearly constant channel more likely.  A fixture is only written when the reference's OWN float32
train output and every gradient lie within MARGIN = 1e-5 (relative, max norm) of its float64 rerun; the generator refuses it
otherwise.  The margin found is recorded in `meta/margin` (`meta/margin_worst` names the tensor).  The GIN and GCN cases scale the weight of the encoder's
first layer — Linear(1, hidden) of the first GIN update net, GraphConv(1, hidden) — by make_deepsigns_variants.EMBED_SCALE, for the
reason that file gives for `embed.weight`: with |x| ~ 0.1 and the initial weight, tanh(a W + b) is tanh(b) plus a few percent, the
BatchNorm behind it removes nearly all of what the bias does, and the reference's float32 gradient of that bias and weight is then
2e-5 .. 1e-3 from float64 (gcn: at every one of 200 seeds tried; gin: at 39 of 40).  Each listed seed is the one, of the 30 tried per
case from seed 1 on, with the smallest margin.
"""
from __future__ import annotations

import contextlib
import copy
import io
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import data_arrays, randomise, save, sd_arrays, synth  # noqa: E402
import make_deepsigns_variants as MV  # noqa: E402
import make_dropout_deepsigns as MD  # noqa: E402

MARGIN = 1e-5
ZERO_GRAD = 1e-9
CLASSES = {"gin": "GINDeepSigns", "masked_gin": "MaskedGINDeepSigns", "gcn": "GCNDeepSigns", "transformer": "TransformerDeepSigns"}

# name -> (kind, activation, hidden, out, layers, k, dropout, graph sizes, seed).  Five or six graphs of 1 .. 13 nodes, a one-node graph
# wherever the encoder takes one (GraphConv raises for a node without in-edges); masked_gin: k = 6 with graphs of 1, 3, 4 and 5 nodes.
ENCODERS = {
    "ds_act_gin_tanh_h16_c4_l3_k4": ("gin", "tanh", 16, 4, 3, 4, 0.0, [5, 1, 12, 7, 9, 6], 12),
    "ds_act_masked_gin_tanh_h12_c5_l3_k6": ("masked_gin", "tanh", 12, 5, 3, 6, 0.0, [5, 9, 1, 13, 3, 4], 27),
    "ds_act_gcn_tanh_h19_c4_l3_k5": ("gcn", "tanh", 19, 4, 3, 5, 0.0, [6, 4, 11, 2, 9, 8], 25),
    "ds_act_tf_tanh_h16_l2_k4": ("transformer", "tanh", 16, 4, 2, 4, 0.0, [5, 1, 12, 7, 9, 6], 11),
    "ds_act_tf_elu_h14_l2_k3": ("transformer", "elu", 14, 4, 2, 3, 0.0, [6, 4, 11, 1, 9], 29),
    "ds_act_gin_tanh_dropout_h8_c4_l3_k4": ("gin", "tanh", 8, 4, 3, 4, 0.1, [5, 9, 1, 12, 7], 16),
}
# name -> (net module, class, sign_inv_net, activation, pe_aggregate, net parameters, graph sizes, seed)
NETS = {
    "ds_act_net_gatedgcn_gin_tanh_add": ("gatedgcn_net", "GatedGCNNet", "gin", "tanh", "add",
                                         dict(hidden_dim=12, out_dim=12, L=2, pos_enc_dim=4, readout="mean"), [5, 9, 1, 12, 7], 20),
}
NET_COMMON = dict(MD.NET_COMMON, in_feat_dropout=0.0, dropout=0.0)


def _rel(x, y):
    return float(np.abs(x.astype(np.float64) - y).max() / max(np.abs(y).max(), 1e-300))


def margin_of(a):
    """(largest relative distance of the reference's float32 train output / gradients from the float64 rerun, the tensor's key).  Max
    norm per tensor.  A gradient that is zero in exact arithmetic — a bias in front of a train-mode BatchNorm, which removes every
    per-channel constant — has no scale of its own (1e-9 in float32, 1e-18 in float64): a tensor whose float64 gradient is below
    ZERO_GRAD of the model's largest gradient entry is measured against that largest entry instead."""
    worst = (_rel(a["out/train/y"], a["out/train/y64"]), "out/train/y")
    top = max(float(np.abs(a[key]).max()) for key in a if key.startswith("out/grad64/"))
    for key in a:
        if key.startswith("out/grad/"):
            g64 = a["out/grad64/" + key[len("out/grad/"):]]
            scale = float(np.abs(g64).max())
            if scale < ZERO_GRAD * top:
                scale = top
            worst = max(worst, (float(np.abs(a[key].astype(np.float64) - g64).max() / max(scale, 1e-300)), key))
    return worst


def train_arrays(model, forward, cot, p):
    """Eval output; train-mode forward + backward in float32 and on a float64 copy (on the same masks where p > 0)."""
    arrays = {}
    model64 = copy.deepcopy(model).double()
    sites = MD.Sites()
    ctx = (lambda: MD.patched(sites)) if p > 0.0 else contextlib.nullcontext
    model.eval()
    with torch.no_grad(), ctx():
        arrays["out/eval/y"] = forward(model, torch.float32, sites).numpy()
    records = None
    for m, dtype, tag in ((model, torch.float32, ""), (model64, torch.float64, "64")):
        m.train()
        with ctx():
            y = forward(m, dtype, sites)
            (y * cot.to(dtype)).sum().backward()
        arrays[f"out/train/y{tag}"] = y.detach().numpy()
        for k, q in m.named_parameters():
            if q.grad is not None:
                arrays[f"out/grad{tag}/" + k] = q.grad.detach().numpy()
        if not tag:
            for k, v in m.state_dict().items():
                if k.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked"):
                    arrays["out/train/buffers/" + k] = v.detach().clone().numpy()
            records = list(sites.records)
    arrays["meta/dropout_p"] = np.array(p, dtype=np.float64)
    if p > 0.0:
        assert records and len(records) == len(sites.records)
        assert all(a[0] == b[0] and (a[2] == b[2]).all() for a, b in zip(records, sites.records))
        arrays["meta/dropout_seed"] = np.array(MD.SEED, dtype=np.int64)
        arrays["meta/dropout_step"] = np.array(MD.STEP, dtype=np.int64)
        arrays["meta/dropout_sites"] = np.array([r[0] for r in records], dtype=np.int64)
        arrays["meta/dropout_site_shapes"] = np.array([r[2].shape for r in records], dtype=np.int64)
        for s, r in enumerate(records):
            arrays[f"out/dropout_mask/{s}"] = np.packbits(r[2].reshape(-1))
    return arrays


def _finish(name, arrays, write):
    m, key = margin_of(arrays)
    arrays["meta/margin"] = np.array(m, dtype=np.float64)
    arrays["meta/margin_worst"] = np.array(key)
    if write:
        if m > MARGIN:
            raise SystemExit(f"{name}: the reference's float32 run is {m:.1e} from float64 at {key} (> {MARGIN:g}): pick another seed")
        save(name, **arrays)
    return m, key


def _spread_first_layer(enc, kind):
    """The conditioning of make_deepsigns_variants.EMBED_SCALE, one layer in (see the note on seeds above): the weight of the first
    Linear(1, hidden) / GraphConv(1, hidden) of a GIN / GCN encoder times EMBED_SCALE.  Call under torch.no_grad()."""
    if kind == "gcn":
        enc.enc.layers[0].weight.mul_(MV.EMBED_SCALE)
    elif kind in ("gin", "masked_gin"):
        enc.enc.layers[0].apply_func.lins[0].weight.mul_(MV.EMBED_SCALE)


def encoder_case(name, kind, act, hidden, out, layers, k, p, sizes, seed, write=True):
    mod = MV._import("layers.deepsigns")
    import dgl  # the stand-in
    torch.manual_seed(seed)
    args = (1, hidden, out, layers, k) + (("cpu",) if kind == "masked_gin" else ())
    net = getattr(mod, CLASSES[kind])(*args, use_bn=True, dropout=p, activation=act)
    randomise(net, seed + 1)
    with torch.no_grad():                    # (as make_deepsigns_variants.py: GraphConv's zero bias made to count, the embedding spread)
        for n, q in net.named_parameters():
            if kind == "gcn" and n.startswith("enc.layers.") and n.endswith(".bias"):
                q.copy_(0.1 * torch.randn(q.shape, generator=torch.Generator().manual_seed(seed + 5)))
        if kind == "transformer":
            net.embed.weight.mul_(MV.EMBED_SCALE)
        _spread_first_layer(net, kind)
    data = synth.make_batch(len(sizes), seed=seed, sizes=sizes)
    pe = synth.dgl_pos_enc(data, k)
    g = dgl.Graph(data.edge_index[0], data.edge_index[1], torch.tensor(data.sizes))
    x = pe.unsqueeze(-1)
    cot = torch.randn(x.shape, generator=torch.Generator().manual_seed(seed + 3))
    arrays = {**sd_arrays(net), **data_arrays(data), "in/pos_enc": pe.numpy(), "in/cotangent": cot.numpy(),
              "meta/params": np.array([hidden, out, layers, k], dtype=np.int64), "meta/kind": np.array(kind),
              "meta/activation": np.array(act), "meta/seed": np.array(seed, dtype=np.int64)}

    def forward(m, dtype, sites):
        with sites.range(MD.SIGNINV_SITE):
            return m(g, x.clone().to(dtype))

    arrays.update(train_arrays(net, forward, cot, p))
    return _finish(name, arrays, write)


def net_case(name, module, cls, kind, act, pe_aggregate, params, sizes, seed, write=True):
    mod, train_mod = MD._import_both("nets.ZINC_graph_regression." + module, "train.train_ZINC_graph_regression")
    handle_lap = train_mod.handle_lap
    import dgl  # the stand-in
    if not hasattr(dgl, "broadcast_nodes"):      # by its published meaning: graph g's row for every node of graph g
        dgl.broadcast_nodes = lambda g, x: x.repeat_interleave(g.batch_num_nodes(), 0)
    p = dict(NET_COMMON, **params, sign_inv_net=kind, sign_inv_activation=act, pe_aggregate=pe_aggregate)
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        net = getattr(mod, cls)(p)
    randomise(net, seed + 1)
    with torch.no_grad():
        _spread_first_layer(net.sign_inv_net, kind)
    k = p["pos_enc_dim"]
    data = synth.make_batch(len(sizes), seed=seed, sizes=sizes)
    pe = synth.dgl_pos_enc(data, k)
    cot = torch.randn(len(sizes), 1, generator=torch.Generator().manual_seed(seed + 3))
    arrays = {**sd_arrays(net), **data_arrays(data), "in/pos_enc": pe.numpy(), "in/cotangent": cot.numpy(),
              "meta/hidden_L_k": np.array([p["hidden_dim"], p["L"], k], dtype=np.int64), "meta/kind": np.array(kind),
              "meta/activation": np.array(act), "meta/pe_aggregate": np.array(pe_aggregate), "meta/cls": np.array(cls),
              "meta/sign_inv_layers": np.array(p["sign_inv_layers"], dtype=np.int64),
              "meta/phi_out_dim": np.array(p["phi_out_dim"], dtype=np.int64), "meta/seed": np.array(seed, dtype=np.int64)}

    def forward(m, dtype, sites):
        g = dgl.Graph(data.edge_index[0], data.edge_index[1], torch.tensor(data.sizes))
        pp = handle_lap(m, pe.clone().to(dtype), g, "cpu")               # train_ZINC_graph_regression.py:20-25
        return m(g, data.x.squeeze(-1), pp, data.edge_attr, None)[0]      # :77-80

    arrays.update(train_arrays(net, forward, cot, 0.0))
    return _finish(name, arrays, write)


def main():
    argv = [a for a in sys.argv[1:] if a != "--search"]
    search = "--search" in sys.argv
    count = int(argv.pop(0)) if argv and argv[0].isdigit() else 12
    for table, fn in ((ENCODERS, encoder_case), (NETS, net_case)):
        for name, args in table.items():
            if argv and name not in argv:
                continue
            if not search:
                m, key = fn(name, *args)
                print(f"  {name}: seed {args[-1]}  margin {m:.1e} ({key})")
                continue
            for seed in range(args[-1], args[-1] + count):
                with contextlib.redirect_stdout(io.StringIO()):
                    m, key = fn(name, *args[:-1], seed, write=False)
                print(f"  {name}: seed {seed}  margin {m:.1e} ({key})")


if __name__ == "__main__":
    main()
