"""Regenerates tests/golden/filter_baselines_grid6.npz: the spectral graph-convolution baselines of the LearningFilters table — BernNet,
GPRNet, ChebNet, GcnNet — built and trained by the ORIGINAL code on the 6 x 6 grid (N = 36), on CPU.  LearningFilters/training.py:47-223
(get_lap_feat, train, gen_model) is executed from the reference file exactly as make_golden.py's filters_case does; models.py's BernConv,
BernNet, GPR_prop and GPRNet class bodies run as they are.  torch_geometric comes from tests/golden/ref_shim_filters/ (a working
MessagePassing.propagate, gcn_norm, get_laplacian, add_self_loops, ChebConv, GCNConv, restated from the library's documentation — so the
ChebNet / GcnNet cases are `restated`, see meta/restated).  Arrays only.

    python tests/golden/make_filter_baselines.py     # needs the reference tree where make_golden.py looks for it (not to run the tests)

Per case `c/<name>/`: args/*, sd/* (state_dict), feat (get_lap_feat's output), pre (train-mode prediction before any step), losses [4]
(four train() calls), grad/* (first step), sd1/* (parameters after one torch.optim.Adam step), and err64/* — the reference's own float32
results against the same classes evaluated in float64 from the same parameters and features: max |f32 - f64| / max |f64| of the
prediction (`pre`), of every first-step gradient (`grad/<key>`) and of the four losses (`losses`).  The tests' tolerance is derived from
these.  `lapfeat/*`: get_lap_feat 'abs_val' and 'sign_flip' outputs with the uniforms the reference drew (`lapfeat/u`).
"""
from __future__ import annotations

import contextlib
import copy
import importlib
import io
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import HERE, REF, SHIM, grid_eig, save  # noqa: E402

SHIM_FILTERS = os.path.join(HERE, "ref_shim_filters")
SIDE, SEED = 6, 2024
CASES = [
    dict(name="bernnet", net="BernNet", use_eig=False, lap_method="none"),
    dict(name="bernnet_eig_none", net="BernNet", use_eig=True, lap_method="none"),
    dict(name="bernnet_eig_abs", net="BernNet", use_eig=True, lap_method="abs_val"),
    dict(name="gprnet", net="GPRNet", use_eig=False, lap_method="none"),
    dict(name="chebnet", net="ChebNet", use_eig=False, lap_method="none"),
    dict(name="gcnnet", net="GcnNet", use_eig=False, lap_method="none"),
]
RESTATED = ("chebnet", "gcnnet")          # ChebConv / GCNConv come from the stand-in, not from the reference tree


def _reference_modules():
    for m in list(sys.modules):
        if m.split(".")[0] in ("ign", "signbasisnet", "models", "torch_geometric"):
            del sys.modules[m]
    sys.path[:0] = [SHIM_FILTERS, SHIM, os.path.join(REF, "LearningFilters")]
    try:
        return [importlib.import_module(n) for n in ("ign", "signbasisnet", "models")]
    finally:
        del sys.path[:3]


def reference_script(args, eigvals, eigvecs, data, y):
    """make_golden.reference_filter_script with the filter stand-in ahead of the path: training.py:47-223 executed in a namespace holding
    what the script has defined by then.  Nothing of that source is stored here."""
    ign, sbn, models = _reference_modules()
    lines = open(os.path.join(REF, "LearningFilters", "training.py")).read().splitlines()
    block = "\n".join(lines[46:223])
    assert block.lstrip().startswith("def around(") and block.rstrip().endswith("return rho"), \
        "the reference file moved: re-check the line range of the script block"
    from sklearn.metrics import r2_score
    ns = {"torch": torch, "np": np, "eigvals": eigvals, "eigvecs": eigvecs, "N": eigvecs.shape[0], "args": args, "data": data, "y": y,
          "device": torch.device("cpu"), "r2_score": r2_score, "SignPlus": sbn.SignPlus, "IGNBasisInv": sbn.IGNBasisInv,
          "IGNShared": sbn.IGNShared}
    for n in ("ChebNet", "BernNet", "GcnNet", "GatNet", "ARMANet", "GPRNet", "MLP", "EqDeepSetsEncoder", "Transformer"):
        ns[n] = getattr(models, n)
    with contextlib.redirect_stdout(io.StringIO()):
        exec(compile(block, "reference:LearningFilters/training.py:47-223", "exec"), ns)
    return ns


def perturb(model, seed):
    """The reference initialises every bias to 0 and coe to 1: make them non-trivial (one coe negative, so relu(coe) gates it)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            if k == "coe":
                p.copy_(1 + 0.5 * torch.randn(p.shape, generator=g))
                p[3] = -0.2


def rel_err(a32, a64):
    a32, a64 = np.asarray(a32, dtype=np.float64), np.asarray(a64, dtype=np.float64)
    return np.array(np.abs(a32 - a64).max() / max(np.abs(a64).max(), 1e-300))


def run_f64(model, feat, ei, y, m, lr, steps):
    """The same classes in float64 from the same parameters and features: prediction, first-step gradients, the losses of `steps` Adam steps."""
    model = copy.deepcopy(model).double()
    feat, y, m = feat.double(), y.double(), m.double()
    model.train()
    with torch.no_grad():
        pre = model(feat, ei).numpy()
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    losses, grads = [], {}
    for step in range(steps):
        opt.zero_grad()
        loss = torch.square(m * (model(feat, ei) - y)).sum()          # training.py:140-141
        loss.backward()
        if step == 0:
            grads = {k: p.grad.detach().clone().numpy() for k, p in model.named_parameters()}
        opt.step()
        losses.append(float(loss))
    return pre, grads, np.array(losses)


def main():
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
        a = dict(epochs=4, lr=0.01, filter_type="band", net="BernNet", img_num=1, use_eig=False, lap_method="none", sign_inv_net="DS",
                 basis_inv_net="IGN", hidden_channels=32, num_layers=2)
        a.update({k: v for k, v in case.items() if k != "name"})
        args = types.SimpleNamespace(**a)
        data = types.SimpleNamespace(x=x.clone(), m=m.clone(), edge_index=torch.from_numpy(np.asarray(ei)))
        ns = reference_script(args, D, V, data, yv.clone())
        torch.manual_seed(SEED + ci)
        np.random.seed(SEED + ci)                       # GPR_prop's Init='Random' draws from np.random (models.py:161)
        model = ns["gen_model"](args)
        perturb(model, SEED + 10 + ci)
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
                    arrays[t + "grad/" + k] = p_.grad.detach().clone().numpy()
                    arrays[t + "err64/grad/" + k] = rel_err(arrays[t + "grad/" + k], g64[k])
                for k, v in model.state_dict().items():
                    arrays[t + "sd1/" + k] = v.detach().clone().numpy()
        arrays[t + "losses"] = np.array(losses, dtype=np.float64)
        arrays[t + "err64/pre"] = rel_err(arrays[t + "pre"], p64)
        arrays[t + "err64/losses"] = rel_err(arrays[t + "losses"], l64)
        print(f"{case['name']}: err64 pre {float(arrays[t + 'err64/pre']):.2e} losses {float(arrays[t + 'err64/losses']):.2e} grads max "
              f"{max(float(arrays[t + 'err64/grad/' + k]) for k in g64):.2e}")
    # get_lap_feat 'abs_val' / 'sign_flip' (training.py:94-100) with the uniforms the reference draws
    args = types.SimpleNamespace(use_eig=True, lap_method="sign_flip", net="MLP", hidden_channels=32, num_layers=2)
    ns = reference_script(args, D, V, types.SimpleNamespace(x=x, m=m, edge_index=torch.from_numpy(np.asarray(ei))), yv)
    torch.manual_seed(SEED + 99)
    arrays["lapfeat/u"] = torch.rand(V.shape[1]).numpy()
    torch.manual_seed(SEED + 99)
    arrays["lapfeat/sign_flip"] = ns["get_lap_feat"](True, D, V, x[:, 0:1], "sign_flip", None).numpy()
    arrays["lapfeat/abs_val"] = ns["get_lap_feat"](True, D, V, x[:, 0:1], "abs_val", None).numpy()
    save("filter_baselines_grid6", **arrays)


if __name__ == "__main__":
    main()
