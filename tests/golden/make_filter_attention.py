"""Regenerates tests/golden/filter_attention_grid6.npz: the last two nets of the LearningFilters table, GatNet and ARMANet, built and
trained on the 6 x 6 grid (N = 36), on CPU.  LearningFilters/training.py:47-223 (get_lap_feat, train, gen_model) is executed from the
reference file and models.py's GatNet / ARMANet class bodies run as they are, exactly as in make_filter_baselines.py; torch_geometric
comes from tests/golden/ref_shim_filters_attn/, whose GATConv and ARMAConv are restated from the library's documentation — so all three
cases are `restated` (meta/restated).  Arrays only.

    python tests/golden/make_filter_attention.py     # needs the reference tree where make_golden.py looks for it (not to run the tests)

Per case `c/<name>/`: the fields of filter_baselines_grid6.npz — args/*, sd/*, feat, pre, losses [4], grad/* (first step), sd1/* (after
one torch.optim.Adam step) and err64/* (the fp32 run against the same classes in float64: max |f32 - f64| / max |f64|).  Every bias is
perturbed away from its zero initialisation.  ARMAConv's `weight` is unused at one layer: it has no gradient and no grad/ entry.
"""
from __future__ import annotations

import copy
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_filter_baselines as MFB  # noqa: E402
from make_golden import HERE, grid_eig, save  # noqa: E402

# The seed is one at which no first-step gradient vanishes identically.  With the 1 + 2 N input the second layer's logits often have one
# sign per head in every row; leaky_relu is then linear on each row, d att_r is exactly zero, and a relative error of it means nothing
# (seeds 4048, 4050, 4051 and 4053 record 3e8 .. 2e9 there).  main() refuses to write such a fixture.
SIDE, SEED = 6, 4049
CASES = [
    dict(name="gatnet", net="GatNet", use_eig=False, lap_method="none"),
    dict(name="gatnet_eig_abs", net="GatNet", use_eig=True, lap_method="abs_val"),       # input width 1 + 2 N
    dict(name="armanet", net="ARMANet", use_eig=False, lap_method="none"),
]
RESTATED = ("gatnet", "gatnet_eig_abs", "armanet")


def run_f64(model, feat, ei, y, m, lr, steps):
    """make_filter_baselines.run_f64 for models with parameters that get no gradient."""
    model = copy.deepcopy(model).double()
    feat, y, m = feat.double(), y.double(), m.double()
    model.train()
    with torch.no_grad():
        pre = model(feat, ei).numpy()
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    losses, grads = [], {}
    for step in range(steps):
        opt.zero_grad()
        loss = torch.square(m * (model(feat, ei) - y)).sum()
        loss.backward()
        if step == 0:
            grads = {k: p.grad.detach().clone().numpy() for k, p in model.named_parameters() if p.grad is not None}
        opt.step()
        losses.append(float(loss))
    return pre, grads, np.array(losses)


def main():
    MFB.SHIM_FILTERS = os.path.join(HERE, "ref_shim_filters_attn")          # ahead of ref_shim on the path of the reference's imports
    ei, N, D, V = grid_eig(SIDE)
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(N, 2, generator=g)
    yv = torch.randn(N, 2, generator=g)
    m = torch.ones(N, 1)
    idx = np.arange(N)
    r, c = idx // SIDE, idx % SIDE
    m[(r == 0) | (c == 0) | (r == SIDE - 1) | (c == SIDE - 1)] = 0.0
    arrays = {"in/eigvals": D.numpy(), "in/eigvecs": V.numpy(), "in/x": x.numpy(), "in/y": yv.numpy(), "in/m": m.numpy(),
              "in/edge_index": np.asarray(ei), "meta/side": np.array(SIDE), "meta/cases": np.array([c_["name"] for c_ in CASES]),
              "meta/restated": np.array(RESTATED)}
    for ci, case in enumerate(CASES):
        a = dict(epochs=4, lr=0.01, filter_type="band", net="GatNet", img_num=1, use_eig=False, lap_method="none", sign_inv_net="DS",
                 basis_inv_net="IGN", hidden_channels=32, num_layers=2)
        a.update({k: v for k, v in case.items() if k != "name"})
        args = types.SimpleNamespace(**a)
        data = types.SimpleNamespace(x=x.clone(), m=m.clone(), edge_index=torch.from_numpy(np.asarray(ei)))
        ns = MFB.reference_script(args, D, V, data, yv.clone())
        torch.manual_seed(SEED + ci)
        model = ns["gen_model"](args)
        MFB.perturb(model, SEED + 10 + ci)
        t = "c/" + case["name"] + "/"
        for k, v in a.items():
            arrays[t + "args/" + k] = np.array(v)
        for k, v in model.state_dict().items():
            arrays[t + "sd/" + k] = v.detach().clone().numpy()
        model.train()
        with torch.no_grad():
            feat = ns["get_lap_feat"](args.use_eig, D, V, x[:, 0:1], args.lap_method, model)
            arrays[t + "feat"] = feat.numpy()
            arrays[t + "pre"] = model(feat, data.edge_index).numpy()
        p64, g64, l64 = run_f64(model, feat, data.edge_index, yv[:, 0:1], m, args.lr, 4)
        opt = torch.optim.Adam(model.parameters(), lr=args.lr)
        losses = []
        for step in range(4):
            loss, _ = ns["train"](0, model, opt)
            losses.append(loss)
            if step == 0:
                for k, p_ in model.named_parameters():
                    if p_.grad is None:
                        assert k.endswith(".weight") and k not in g64, k          # ARMAConv.weight at one layer
                        continue
                    arrays[t + "grad/" + k] = p_.grad.detach().clone().numpy()
                    arrays[t + "err64/grad/" + k] = MFB.rel_err(arrays[t + "grad/" + k], g64[k])
                for k, v in model.state_dict().items():
                    arrays[t + "sd1/" + k] = v.detach().clone().numpy()
        arrays[t + "losses"] = np.array(losses, dtype=np.float64)
        arrays[t + "err64/pre"] = MFB.rel_err(arrays[t + "pre"], p64)
        arrays[t + "err64/losses"] = MFB.rel_err(arrays[t + "losses"], l64)
        print(f"{case['name']}: err64 pre {float(arrays[t + 'err64/pre']):.2e} losses {float(arrays[t + 'err64/losses']):.2e} grads max "
              f"{max(float(arrays[t + 'err64/grad/' + k]) for k in g64):.2e}")
        assert max(float(arrays[t + "err64/grad/" + k]) for k in g64) < 1e-4, "a gradient vanishes identically: choose another seed"
    save("filter_attention_grid6", **arrays)


if __name__ == "__main__":
    main()
