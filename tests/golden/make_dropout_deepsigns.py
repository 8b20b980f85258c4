"""Regenerates tests/golden/ds_dropout_*.npz: the reference's four sign-invariant encoders (GraphPrediction/layers/deepsigns.py) and two
base nets behind the reference's handle_lap, in TRAIN mode with dropout > 0, the masks drawn by the counter-based generator of
csrc/dropout.hip instead of torch's.  F.dropout and nn.Dropout.forward are replaced, for the duration of a forward, by the numpy
restatement of the mask contract (tests/dropout_cases.keep_mask): call number s of an ENCODER forward — enc(g, x), enc(g, -x), rho — is
site SN_SIGNINV_DROP_SITE + s, call number s of a base net's forward is site s (make_dropout.py's rule); a call with p = 0 (the
nn.Dropout(0) modules inside SetTransformerEncoder) draws nothing and takes no ordinal.  The logical [R, C] shape is the tensor's
(C = its last dimension).  Helpers, shims and graphs are make_golden.py's, make_deepsigns_variants.py's and make_baseline_pe.py's.
Arrays only.  (The files are ds_dropout_*, not dropout_*: tests/test_dropout_cases_cpu.py reads every dropout_*.npz as a fixture whose
sites are the plain ordinals 0, 1, ... of make_dropout.py, and an encoder's sites lie in their own range.)

    python tests/golden/make_dropout_deepsigns.py      # needs the reference tree where make_golden.py looks for it (not needed to run the tests)

  ds_dropout_<case>  state_dict (BatchNorm buffers randomised), batch, positional encoding, cotangent; the eval output; the train-mode
                     output, the BatchNorm buffers after that forward and the gradient of sum(y * cotangent) w.r.t. every parameter,
                     from the reference in float32 — and output and gradients once more from a float64 copy on the same masks (`y64`,
                     `grad64/`); the masks drawn (bit-packed, site order) with their sites, shapes and parameters, which
                     tests/test_signinv_dropout_cpu.py checks against the site table of tests/signinv_dropout_cases.py
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
from make_golden import HERE, data_arrays, randomise, save, sd_arrays, synth  # noqa: E402
import make_deepsigns_variants as MV  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import dropout_cases as DC  # noqa: E402

SEED, STEP = 20241020, 5
SIGNINV_SITE = 0x53490000

# name -> (kind, hidden, out, layers, k, p, graph sizes, seed).  Per encoder one width that is a multiple of four and one odd width; every
# masked case has graphs with fewer nodes than k; gcn: no graph without edges, h8 -> c4 runs GraphConv's weight-first branch (in > out).
# Every seed is that, of the 20 tried per case (first seed 411 + case number, steps of 20), at which the REFERENCE's own fp32 output and
# gradients lie closest to their float64 values (as make_deepsigns_variants.py: a train-mode BatchNorm over a few dozen rows amplifies every rounding in front of it).
ENCODERS = {
    "ds_dropout_gin_h8_c4_l3_k4": ("gin", 8, 4, 3, 4, 0.1, [5, 9, 12, 7], 711),
    "ds_dropout_gin_h19_c3_l4_k5": ("gin", 19, 3, 4, 5, 0.5, [6, 4, 11, 3, 9], 452),
    "ds_dropout_masked_gin_h8_c4_l3_k6": ("masked_gin", 8, 4, 3, 6, 0.5, [5, 9, 12, 3], 573),
    "ds_dropout_masked_gin_h7_c5_l4_k5": ("masked_gin", 7, 5, 4, 5, 0.1, [6, 4, 11, 3, 9], 674),
    "ds_dropout_gcn_h8_c4_l3_k4": ("gcn", 8, 4, 3, 4, 0.5, [5, 9, 12, 7], 675),
    "ds_dropout_gcn_h19_c21_l4_k5": ("gcn", 19, 21, 4, 5, 0.1, [6, 4, 11, 3, 9], 616),
    "ds_dropout_transformer_h16_l3_k4": ("transformer", 16, 4, 3, 4, 0.1, [5, 9, 12, 7], 617),
    "ds_dropout_transformer_h14_l3_k5": ("transformer", 14, 4, 3, 5, 0.5, [6, 4, 11, 3, 9], 658),
}

# name -> (net module, class, sign_inv_net, pe_aggregate, net parameters, graph sizes, seed): handle_lap + net, dropout 0.1 in both and
# in_feat_dropout 0.1: the nets number their sites statically (site 0 is in_feat_dropout), so as in make_dropout.py every site of the
# NET's range is active; only the encoder's range skips p = 0 calls
NETS = {
    "ds_dropout_net_gatedgcn_gin_add": ("gatedgcn_net", "GatedGCNNet", "gin", "add",
                                        dict(hidden_dim=12, out_dim=12, L=2, pos_enc_dim=4, readout="mean"), [5, 9, 12, 7], 421),
    "ds_dropout_net_transformer_masked_gin_concat": ("transformer_net", "TransformerNet", "masked_gin", "concat",
                                                     dict(hidden_dim=16, out_dim=16, L=2, pos_enc_dim=5, n_heads=4, full_graph=False,
                                                          readout="sum", layer_norm=True), [6, 4, 11, 3, 9], 422),
}
NET_P = 0.1
NET_COMMON = dict(num_atom_type=28, num_bond_type=4, in_feat_dropout=NET_P, dropout=NET_P, batch_norm=True, residual=True, edge_feat=True,
                  device="cpu", pe_init="lap_pe", lap_method="sign_inv", lap_lspe=False, use_lapeig_loss=False, lambda_loss=1,
                  alpha_loss=1e-4, sign_inv_layers=3, sign_inv_activation="relu", phi_out_dim=4)


class Sites:
    """The stand-in of F.dropout / nn.Dropout.forward while `current` names a site range: site = its base + the ordinal of the call."""

    def __init__(self):
        self.records = []          # (site, p, keep [R, C])
        self.base, self.count = None, 0

    def reset(self):
        self.records, self.base, self.count = [], None, 0

    @contextlib.contextmanager
    def range(self, base):
        self.base, self.count = base, 0
        try:
            yield
        finally:
            self.base = None

    def __call__(self, x, p=0.5, training=True, inplace=False):
        if not training:
            return x
        assert self.base is not None, "a dropout call outside a site range"
        if p == 0.0:
            assert self.base == SIGNINV_SITE, "a net's site with p = 0 would still take an ordinal: build the fixtures with every site active"
            return x               # inside the encoder: no site, no ordinal
        C = x.shape[-1]
        site = self.base + self.count
        self.count += 1
        keep = DC.keep_mask(x.numel() // C, C, p, SEED, STEP, site)
        self.records.append((site, float(p), keep))
        return x * (torch.from_numpy(keep).to(x.dtype) * float(DC.scale_of(p))).view(x.shape)


@contextlib.contextmanager
def patched(sites):
    import torch.nn.functional as F
    old_f, old_m = F.dropout, torch.nn.Dropout.forward
    F.dropout = sites
    torch.nn.Dropout.forward = lambda self, x: sites(x, self.p, self.training, self.inplace)
    sites.reset()
    try:
        yield sites
    finally:
        F.dropout, torch.nn.Dropout.forward = old_f, old_m


def train_arrays(model, forward, cot, p):
    """make_dropout.train_arrays with site ranges: eval output, then train-mode forward + backward in float32 and on a float64 copy."""
    arrays = {}
    model64 = copy.deepcopy(model).double()
    sites = Sites()
    model.eval()
    with torch.no_grad(), patched(sites):
        arrays["out/eval/y"] = forward(model, torch.float32, sites).numpy()
    assert not sites.records
    records = None
    for m, dtype, tag in ((model, torch.float32, ""), (model64, torch.float64, "64")):
        m.train()
        with patched(sites):
            y = forward(m, dtype, sites)
            (y * cot.to(dtype)).sum().backward()
        arrays[f"out/train/y{tag}"] = y.detach().numpy()
        for k, q in m.named_parameters():
            if q.grad is not None:
                arrays[f"out/train/grad{tag}/" + k] = q.grad.detach().numpy()
        if not tag:
            for k, v in m.state_dict().items():
                if k.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked"):
                    arrays["out/train/buffers/" + k] = v.detach().clone().numpy()
            records = list(sites.records)
    assert records and len(records) == len(sites.records)
    assert all(a[0] == b[0] and (a[2] == b[2]).all() for a, b in zip(records, sites.records))
    arrays["meta/dropout_seed"] = np.array(SEED, dtype=np.int64)
    arrays["meta/dropout_step"] = np.array(STEP, dtype=np.int64)
    arrays["meta/dropout_p"] = np.array(p, dtype=np.float64)
    arrays["meta/dropout_sites"] = np.array([r[0] for r in records], dtype=np.int64)
    arrays["meta/dropout_site_p"] = np.array([r[1] for r in records], dtype=np.float64)
    arrays["meta/dropout_site_shapes"] = np.array([r[2].shape for r in records], dtype=np.int64)
    for s, r in enumerate(records):
        arrays[f"out/dropout_mask/{s}"] = np.packbits(r[2].reshape(-1))
    return arrays


def _encoder(mod, kind, hidden, out, layers, k, p, seed):
    cls = {"gin": "GINDeepSigns", "masked_gin": "MaskedGINDeepSigns", "gcn": "GCNDeepSigns", "transformer": "TransformerDeepSigns"}[kind]
    torch.manual_seed(seed)
    args = (1, hidden, out, layers, k) + (("cpu",) if kind == "masked_gin" else ())
    net = getattr(mod, cls)(*args, use_bn=True, dropout=p, activation="relu")
    randomise(net, seed + 1)
    with torch.no_grad():                    # (as make_deepsigns_variants.py: GraphConv's zero bias made to count, the embedding spread)
        for n, q in net.named_parameters():
            if kind == "gcn" and n.startswith("enc.layers.") and n.endswith(".bias"):
                q.copy_(0.1 * torch.randn(q.shape, generator=torch.Generator().manual_seed(seed + 5)))
        if kind == "transformer":
            net.embed.weight.mul_(MV.EMBED_SCALE)
    return net


def encoder_case(name, kind, hidden, out, layers, k, p, sizes, seed):
    mod = MV._import("layers.deepsigns")
    import dgl  # the stand-in
    net = _encoder(mod, kind, hidden, out, layers, k, p, seed)
    data = synth.make_batch(len(sizes), seed=seed, sizes=sizes)
    pe = synth.dgl_pos_enc(data, k)
    g = dgl.Graph(data.edge_index[0], data.edge_index[1], torch.tensor(data.sizes))
    x = pe.unsqueeze(-1)
    cot = torch.randn(x.shape, generator=torch.Generator().manual_seed(seed + 3))
    arrays = {**sd_arrays(net), **data_arrays(data), "in/pos_enc": pe.numpy(), "in/cotangent": cot.numpy(),
              "meta/params": np.array([hidden, out, layers, k], dtype=np.int64), "meta/kind": np.array(kind)}

    def forward(m, dtype, sites):
        with sites.range(SIGNINV_SITE):
            return m(g, x.clone().to(dtype))

    arrays.update(train_arrays(net, forward, cot, p))
    save(name, **arrays)
    return arrays


def _import_both(first, second):
    """Two reference modules over ONE set of stand-ins (MV._import starts from fresh stand-ins each time)."""
    import importlib
    mod = MV._import(first)
    sys.path[:0] = [MV.SHIM_DEEPSIGNS, MV.SHIM, os.path.join(MV.REF, "GraphPrediction")]
    try:
        return mod, importlib.import_module(second)
    finally:
        del sys.path[:3]


def net_case(name, module, cls, kind, pe_aggregate, params, sizes, seed):
    mod, train_mod = _import_both("nets.ZINC_graph_regression." + module, "train.train_ZINC_graph_regression")
    handle_lap = train_mod.handle_lap
    import dgl  # the stand-in
    if not hasattr(dgl, "broadcast_nodes"):      # by its published meaning: graph g's row for every node of graph g
        dgl.broadcast_nodes = lambda g, x: x.repeat_interleave(g.batch_num_nodes(), 0)
    p = dict(NET_COMMON, **params, sign_inv_net=kind, pe_aggregate=pe_aggregate)
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        net = getattr(mod, cls)(p)
    randomise(net, seed + 1)
    if cls == "TransformerNet":              # transformer_net.py:68-69 never hands `dropout` to its layers: set on the layers themselves
        for L in net.layers:
            L.dropout = NET_P
    k = p["pos_enc_dim"]
    data = synth.make_batch(len(sizes), seed=seed, sizes=sizes)
    pe = synth.dgl_pos_enc(data, k)
    cot = torch.randn(len(sizes), 1, generator=torch.Generator().manual_seed(seed + 3))
    arrays = {**sd_arrays(net), **data_arrays(data), "in/pos_enc": pe.numpy(), "in/cotangent": cot.numpy(),
              "meta/hidden_L_k": np.array([p["hidden_dim"], p["L"], k], dtype=np.int64), "meta/kind": np.array(kind),
              "meta/pe_aggregate": np.array(pe_aggregate), "meta/cls": np.array(cls)}
    if "n_heads" in p:
        arrays["meta/n_heads"] = np.array(p["n_heads"], dtype=np.int64)

    def forward(m, dtype, sites):
        g = dgl.Graph(data.edge_index[0], data.edge_index[1], torch.tensor(data.sizes))
        with sites.range(SIGNINV_SITE):      # train_ZINC_graph_regression.py:20-25: the encoder's forward
            pp = handle_lap(m, pe.clone().to(dtype), g, "cpu")
        with sites.range(0):                 # :77-80: the net's
            return m(g, data.x.squeeze(-1), pp, data.edge_attr, None)[0]

    arrays.update(train_arrays(net, forward, cot, NET_P))
    save(name, **arrays)
    return arrays


def report(name, a):
    """The reference's own fp32 distance from float64 on the same masks: what the case's conditioning costs."""
    def rel(x, y):
        return float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-30))
    worst = max((rel(a[k], a["out/train/grad64/" + k[len("out/train/grad/"):]]), k) for k in a if k.startswith("out/train/grad/"))
    print(f"  {name}: sites {len(a['meta/dropout_sites'])}  |y32 - y64| {rel(a['out/train/y'], a['out/train/y64']):.1e}  "
          f"worst gradient {worst[0]:.1e} ({worst[1][len('out/train/grad/'):]})")


def main():
    for name, args in ENCODERS.items():
        report(name, encoder_case(name, *args))
    for name, args in NETS.items():
        report(name, net_case(name, *args))


if __name__ == "__main__":
    main()
